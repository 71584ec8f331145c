"""Phase-1 training of the sensorimotor agent (reference training/train_image_phase1.py), MI355X-native.

Same flags, config.json schema and model-%d.th naming as the reference; the loop body runs on the native executor
(NativeTrainer.step = teacher forward, student forward, unprojection + L1 over the four branches, backward, RCCL
gradient all-reduce, fused Adam).  New flags: --synthetic N (device-resident synthetic frames instead of the LMDB
dataset), --iters_per_epoch, one-process-per-GPU launch through torch.distributed.run, and --save_state / --resume /
--skip-nonfinite (training/resume.py: a run that can be stopped and continued bit for bit, and that survives a step on the loss's pole).

CoordConverter / LocationLoss keep the reference's call signatures (train_image_phase1.py:35-70) for callers that
want the map-space waypoints; they are thin torch expressions over (N,4,5,2) tensors, the timed path uses the fused
HIP loss kernel instead."""
import argparse
import functools

import numpy as np
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
SAVE_EPOCHS = [1, 2, 4, 8, 16, 32, 64, 128, 192, 256]
SPEC = loop.Spec(label="phase 1", images_per_sec=True, save_epochs=SAVE_EPOCHS,
                 nonfinite="phase-1 %s is %s: a predicted waypoint reached the horizon (1/y pole of the unprojection); start from a phase-0 checkpoint")

train_or_eval = functools.partial(loop.run_pass, SPEC)        # (reference train_image_phase1.py:157-229)


class CoordConverter():
    def __init__(self, w=384, h=160, fov=90, world_y=1.4, fixed_offset=2.0, device="cuda"):
        self._img_size = torch.tensor([float(w), float(h)], device=device)
        self._w, self._h, self._fov, self._world_y, self._fixed_offset = w, h, fov, world_y, fixed_offset

    def __call__(self, camera_locations):
        loc = (camera_locations + 1) * self._img_size / 2
        f = self._w / (2 * np.tan(self._fov * np.pi / 360))
        xt = (loc[..., 0] - self._w / 2) / f
        yt = (loc[..., 1] - self._h / 2) / f
        world_z = self._world_y / yt
        world_x = world_z * xt
        return torch.stack([world_x * PIXELS_PER_METER + CROP_SIZE / 2,
                            CROP_SIZE - world_z * PIXELS_PER_METER + self._fixed_offset * PIXELS_PER_METER], dim=-1)


class LocationLoss(torch.nn.Module):
    def forward(self, pred_locations, teac_locations):
        pred_locations = pred_locations / (0.5 * CROP_SIZE) - 1
        return torch.mean(torch.abs(pred_locations - teac_locations), dim=(1, 2, 3))


def train(config):
    rank, world = config["rank"], config["world_size"]
    device = config["device"]
    bzu.log.init(config["log_dir"], rank)
    bzu.log.save_config({k: v for k, v in config.items() if k not in ("rank", "world_size")})
    teacher_config = bzu.log.load_config(config["teacher_args"]["model_path"]) if config["teacher_args"]["model_path"] else {"model_args": {"backbone": "resnet18"}}

    net = ImagePolicyModelSS(config["model_args"]["backbone"], pretrained=config["model_args"]["imagenet_pretrained"], all_branch=True).to(device)
    if config["phase0_ckpt"]:
        net.load_state_dict(torch.load(config["phase0_ckpt"], map_location=device))
    teacher_net = BirdViewPolicyModelSS(teacher_config["model_args"]["backbone"], pretrained=True, all_branch=True).to(device)
    net.precision = teacher_net.precision = config.get("precision", "fp32")
    if config["teacher_args"]["model_path"]:
        teacher_net.load_state_dict(torch.load(config["teacher_args"]["model_path"], map_location=device))
    teacher_net.eval()
    broadcast_module(net)
    broadcast_module(teacher_net)

    bs = config["data_args"]["batch_size"] * int(config["data_args"].get("batch_aug", 1) or 1)
    data_train, data_val = make_loaders(config, device, rank, world, teacher=teacher_net)
    cam = camera_struct(**{k: float(v) for k, v in config["agent_args"]["camera_args"].items()})
    trainer = NativeTrainer(net, resume.teacher_for_trainer(config, teacher_net), bs, (3, 160, 384), device, phase=1, lr=config["optimizer_args"]["lr"],
                            world_size=world, camera=cam, **resume.trainer_kwargs(config))
    loaders = {"train": data_train, "val": data_val}
    return loop.run_epochs(SPEC, config, net, trainer, loaders, resume.load(config, trainer, loaders))


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    loop.add_common_arguments(parser, max_epoch=256, batch_size=24)
    parser.add_argument("--pretrained", action="store_true")
    parser.add_argument("--ckpt", default=None, help="phase-0 checkpoint (required by the reference; optional with --synthetic)")
    parser.add_argument("--teacher_path", default=None)
    parser.add_argument("--fixed_offset", type=float, default=4.)
    parser.add_argument("--batch_aug", type=int, default=1)
    parser.add_argument("--speed_noise", type=float, default=0.0)
    parser.add_argument("--augment", choices=["medium", "medium_harder", "super_hard", "None", "custom"], default="super_hard")
    resume.add_arguments(parser)
    return parser.parse_args(argv)


def build_config(parsed, rank, world, device):
    config = {
        "log_dir": parsed.log_dir, "log_iterations": parsed.log_iterations, "max_epoch": parsed.max_epoch,
        "device": device, "precision": parsed.precision, "phase0_ckpt": parsed.ckpt, "optimizer_args": {"lr": parsed.lr},
        "speed_noise": parsed.speed_noise,
        "data_args": {"dataset_dir": parsed.dataset_dir, "batch_size": parsed.batch_size, "n_step": N_STEP, "gap": GAP,
                      "augment": parsed.augment, "batch_aug": parsed.batch_aug, "num_workers": 8},
        "model_args": {"model": "image_ss", "imagenet_pretrained": parsed.pretrained, "backbone": BACKBONE},
        "teacher_args": {"model_path": parsed.teacher_path},
        "agent_args": {"camera_args": {"w": 384, "h": 160, "fov": 90, "world_y": 1.4, "fixed_offset": 4.0}},
        "synthetic": parsed.synthetic, "iters_per_epoch": parsed.iters_per_epoch, "rank": rank, "world_size": world,
    }
    config.update(resume.config_entries(parsed))
    config["data_args"].update(resume.resident_entries(parsed))
    if config["data_args"].get("cache_teacher") and parsed.speed_noise > 0:
        raise SystemExit("--cache-teacher with --speed_noise: the live teacher reads the noisy speed, which is no function of the frame")
    return config


def main(argv=None):
    loop.launch(parse_arguments(argv), build_config, train)


if __name__ == "__main__":
    main()
