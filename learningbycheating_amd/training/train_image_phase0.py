"""Phase-0 warm-up of the sensorimotor agent (reference training/train_image_phase0.py), MI355X-native.

The reference moves the teacher's map-space waypoints to the CPU every step, projects them with cv2.projectPoints in
float64 and ships them back (train_image_phase0.py:67-79).  Here the same pinhole projection + clip + normalised L1
against the *selected* branch runs in one HIP kernel (csrc/loss.hip kind 0); no device->host round trip."""
import argparse
import functools

import torch

from ..bird_view.models.birdview import BirdViewPolicyModelSS
from ..bird_view.models.image import ImagePolicyModelSS
from ..bird_view.utils import bz_utils as bzu
from .data import make_loaders
from ..parallel import broadcast_module
from . import loop, resume
from .native import NativeTrainer, camera_struct

BACKBONE = "resnet34"
GAP = 5
N_STEP = 5
PIXELS_PER_METER = 5
CROP_SIZE = 192
SAVE_EPOCHS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 384, 512, 768, 1000]
SPEC = loop.Spec(label="phase 0", images_per_sec=False, nonfinite=None, save_epochs=SAVE_EPOCHS)

train_or_eval = functools.partial(loop.run_pass, SPEC)        # (reference train_image_phase0.py:152-209)


def train(config):
    rank, world, device = config["rank"], config["world_size"], config["device"]
    bzu.log.init(config["log_dir"], rank)
    bzu.log.save_config({k: v for k, v in config.items() if k not in ("rank", "world_size")})
    teacher_backbone = "resnet18"
    if config["teacher_args"]["model_path"]:
        teacher_backbone = bzu.log.load_config(config["teacher_args"]["model_path"])["model_args"]["backbone"]
    net = ImagePolicyModelSS(config["model_args"]["backbone"], pretrained=config["model_args"]["imagenet_pretrained"]).to(device)
    teacher_net = BirdViewPolicyModelSS(teacher_backbone).to(device)
    net.precision = teacher_net.precision = config.get("precision", "fp32")
    if config["teacher_args"]["model_path"]:
        teacher_net.load_state_dict(torch.load(config["teacher_args"]["model_path"], map_location=device))
    teacher_net.eval()
    broadcast_module(net)
    broadcast_module(teacher_net)
    bs = config["data_args"]["batch_size"]
    data_train, data_val = make_loaders(config, device, rank, world, teacher=teacher_net)
    cam = camera_struct(**{k: float(v) for k, v in config["camera_args"].items()})
    trainer = NativeTrainer(net, resume.teacher_for_trainer(config, teacher_net), bs, (3, 160, 384), device, phase=0, lr=config["optimizer_args"]["lr"],
                            world_size=world, camera=cam, **resume.trainer_kwargs(config))
    loaders = {"train": data_train, "val": data_val}
    return loop.run_epochs(SPEC, config, net, trainer, loaders, resume.load(config, trainer, loaders))


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    loop.add_common_arguments(parser, max_epoch=2, batch_size=96)
    parser.add_argument("--pretrained", action="store_true")
    parser.add_argument("--teacher_path", default=None)
    parser.add_argument("--fixed_offset", type=float, default=4.0)
    parser.add_argument("--augment", choices=["None", "medium", "medium_harder", "super_hard"], default=None)
    resume.add_arguments(parser)
    return parser.parse_args(argv)


def build_config(parsed, rank, world, device):
    if parsed.pretrained:
        raise SystemExit("--pretrained downloads ImageNet weights (reference resnet.py:175-178); no network here")
    config = {
        "log_dir": parsed.log_dir, "log_iterations": parsed.log_iterations, "max_epoch": parsed.max_epoch,
        "device": device, "precision": parsed.precision, "optimizer_args": {"lr": parsed.lr},
        "data_args": {"dataset_dir": parsed.dataset_dir, "batch_size": parsed.batch_size, "n_step": N_STEP, "gap": GAP,
                      "augment": parsed.augment, "num_workers": 8},
        "model_args": {"model": "image_ss", "imagenet_pretrained": parsed.pretrained, "backbone": BACKBONE},
        "camera_args": {"w": 384, "h": 160, "fov": 90, "world_y": 1.4, "fixed_offset": parsed.fixed_offset},
        "teacher_args": {"model_path": parsed.teacher_path},
        "synthetic": parsed.synthetic, "iters_per_epoch": parsed.iters_per_epoch, "rank": rank, "world_size": world,
    }
    config.update(resume.config_entries(parsed))
    config["data_args"].update(resume.resident_entries(parsed))
    return config


def main(argv=None):
    loop.launch(parse_arguments(argv), build_config, train)


if __name__ == "__main__":
    main()
