"""Behaviour cloning of the privileged agent (reference training/train_birdview.py), MI355X-native:
BirdViewPolicyModelSS(resnet18) on 7x192x192 maps, L1 (choice='l1', train_birdview.py:161) between the selected
branch and ground-truth waypoints in pixels."""
import argparse
import functools
from pathlib import Path

import torch

from ..bird_view.models.birdview import BirdViewPolicyModelSS
from ..bird_view.utils import bz_utils as bzu
from .data import make_loaders
from ..parallel import broadcast_module
from . import loop, resume
from .native import NativeTrainer

BACKBONE = "resnet18"
GAP = 5
N_STEP = 5
SAVE_EPOCHS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 384, 512, 768, 1000]
SPEC = loop.Spec(label="train_birdview", images_per_sec=False, nonfinite=None, save_epochs=SAVE_EPOCHS)

train_or_eval = functools.partial(loop.run_pass, SPEC)        # (reference train_birdview.py:102-153)


def train(config):
    rank, world, device = config["rank"], config["world_size"], config["device"]
    bzu.log.init(config["log_dir"], rank)
    bzu.log.save_config({k: v for k, v in config.items() if k not in ("rank", "world_size")})
    net = BirdViewPolicyModelSS(config["model_args"]["backbone"]).to(device)
    net.precision = config.get("precision", "fp32")
    full_state = config["resume"] and (Path(config["log_dir"]) / resume.STATE_NAME).exists()
    if config["resume"] and not full_state:
        # the reference takes glob('model-*.th')[-1] unsorted (train_birdview.py:164-169); sort numerically instead
        ckpts = sorted(Path(config["log_dir"]).glob("model-*.th"), key=lambda p: int(p.stem.split("-")[1]))
        if ckpts:
            net.load_state_dict(torch.load(str(ckpts[-1]), map_location=device))
    broadcast_module(net)
    bs = config["data_args"]["batch_size"]
    data_train, data_val = make_loaders(config, device, rank, world)
    trainer = NativeTrainer(net, None, bs, (7, 192, 192), device, phase="birdview", lr=config["optimizer_args"]["lr"], world_size=world,
                            **resume.trainer_kwargs(config))
    loaders = {"train": data_train, "val": data_val}
    # --resume: the full state (train_state.th: optimizer, loaders, RNG, epoch) when there is one; without it, as before, the newest
    # model-%d.th with a fresh Adam from epoch 0
    state = resume.load(config, trainer, loaders) if full_state else None
    return loop.run_epochs(SPEC, config, net, trainer, loaders, state)


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    loop.add_common_arguments(parser, max_epoch=1000, batch_size=256)
    parser.add_argument("--x_jitter", type=int, default=5)
    parser.add_argument("--y_jitter", type=int, default=0)
    parser.add_argument("--angle_jitter", type=int, default=5)
    parser.add_argument("--gap", type=int, default=5)
    parser.add_argument("--max_frames", type=int, default=None)
    parser.add_argument("--cmd-biased", action="store_true")
    parser.add_argument("--resume", action="store_true")
    resume.add_arguments(parser, with_resume=False)
    return parser.parse_args(argv)


def build_config(parsed, rank, world, device):
    resident = resume.resident_entries(parsed, teacher=False)      # (this script trains the teacher: --cache-teacher is refused here)
    config = {
        "log_dir": parsed.log_dir, "log_iterations": parsed.log_iterations, "max_epoch": parsed.max_epoch,
        "device": device, "precision": parsed.precision, "optimizer_args": {"lr": parsed.lr}, "resume": parsed.resume,
        "data_args": {"dataset_dir": parsed.dataset_dir, "batch_size": parsed.batch_size, "n_step": N_STEP, "gap": parsed.gap,
                      "crop_x_jitter": parsed.x_jitter, "crop_y_jitter": parsed.y_jitter, "angle_jitter": parsed.angle_jitter,
                      "max_frames": parsed.max_frames, "cmd_biased": parsed.cmd_biased},
        "model_args": {"model": "birdview_dian", "input_channel": 7, "backbone": BACKBONE},
        "synthetic": parsed.synthetic, "iters_per_epoch": parsed.iters_per_epoch, "rank": rank, "world_size": world,
    }
    config.update(resume.config_entries(parsed))
    config["data_args"].update(resident)
    return config


def main(argv=None):
    loop.launch(parse_arguments(argv), build_config, train)


if __name__ == "__main__":
    main()
