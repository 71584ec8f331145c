"""Score checkpoints on the validation loader: python -m learningbycheating_amd.training.evaluate --phase 1 --model_path model-16.th ...

The pass is the training scripts' validation pass with --val-metrics: non-updating eval-mode steps (NativeTrainer.step(update=False,
train_mode=False, metrics=m)) that add every batch's waypoint errors in metres into one device record, one read-back after the
last batch.  No optimizer step, no updating step.  Prints WaypointMetrics.result() as one JSON line and writes it to metrics.json
beside the checkpoint (model-N.th and model-ema-N.th are both plain state_dicts of the student).  --visuals also draws every batch's
waypoint panels on the device (training/visuals.py) and writes the last grid as visuals.png beside metrics.json."""
import argparse
import json
import os
from pathlib import Path

import torch

from ..bird_view.models.birdview import BirdViewPolicyModelSS
from ..bird_view.models.image import ImagePolicyModelSS
from . import loop, resume
from .data import make_loaders
from .native import NativeTrainer, camera_struct

PHASES = {"0": 0, "1": 1, "birdview": "birdview"}


def validation_pass(trainer, data, device, metrics=None, max_batches=None, visuals=None):
    """one pass over `data` without updates, in eval mode, feeding `metrics` (default: a fresh object that fits the trainer's phase);
    nothing is read back inside the loop.  visuals: a PanelRenderer that draws every batch's panels (one more launch each; its last
    grid is the caller's to read).  -> the metrics object"""
    m = metrics if metrics is not None else trainer.make_metrics()
    draw = {} if visuals is None else {"visuals": visuals}
    for i, batch in enumerate(data):
        if max_batches is not None and i >= max_batches:
            break
        loop.step_batch(trainer, batch, device, update=False, train_mode=False, metrics=m, **draw)
    return m


def build_networks(phase, model_path, teacher_path, precision, device):
    """-> (student loaded from model_path, frozen teacher or None) as the training script of `phase` builds them"""
    if phase == "birdview":
        net = BirdViewPolicyModelSS("resnet18").to(device)
        teacher = None
    else:
        teacher_backbone = "resnet18"
        if teacher_path and (Path(teacher_path).parent / "config.json").exists():
            with open(str(Path(teacher_path).parent / "config.json")) as f:
                teacher_backbone = json.load(f)["model_args"]["backbone"]
        net = ImagePolicyModelSS("resnet34", all_branch=(phase == 1)).to(device)
        teacher = BirdViewPolicyModelSS(teacher_backbone, all_branch=(phase == 1)).to(device)
        teacher.precision = precision
        if teacher_path:
            teacher.load_state_dict(torch.load(teacher_path, map_location=device))
        teacher.eval()
    net.precision = precision
    net.load_state_dict(torch.load(model_path, map_location=device))
    net.eval()
    return net, teacher


def build_trainer(phase, model_path, teacher_path, batch_size, precision, device, fixed_offset=4.0, networks=None):
    """the networks and the trainer of `phase` as the training script of that phase builds them, the student loaded from model_path.
    networks: (student, teacher) built before; a teacher of None in phase 0 / 1 gives a trainer without a teacher engine (--cache-teacher)"""
    net, teacher = networks if networks is not None else build_networks(phase, model_path, teacher_path, precision, device)
    shape = (7, 192, 192) if phase == "birdview" else (3, 160, 384)
    return NativeTrainer(net, teacher, batch_size, shape, device, phase=phase, camera=camera_struct(fixed_offset=float(fixed_offset)))


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--phase", choices=sorted(PHASES), required=True)
    parser.add_argument("--model_path", required=True, help="model-N.th or model-ema-N.th of that phase's training script")
    parser.add_argument("--teacher_path", default=None, help="the privileged agent's checkpoint (image models: phases 0 and 1)")
    parser.add_argument("--dataset_dir", default=None)
    parser.add_argument("--synthetic", type=int, default=2048, help="number of device-resident synthetic frames (used when no --dataset_dir is given)")
    parser.add_argument("--batch_size", type=int, default=32)
    parser.add_argument("--batches", type=int, default=10, help="validation batches (the training scripts' pass has iters_per_epoch / 100)")
    parser.add_argument("--fixed_offset", type=float, default=4.0)
    loop.add_precision_argument(parser)
    resume.add_resident_arguments(parser)
    resume.add_visuals_arguments(parser)
    parsed = parser.parse_args(argv)
    draw = resume.visuals_entries(parsed)
    resident = resume.resident_entries(parsed, teacher=parsed.phase != "birdview")
    _, _, local = loop.ranks()
    device = loop.select_device(local, "evaluation")
    phase = PHASES[parsed.phase]
    net, teacher = build_networks(phase, parsed.model_path, parsed.teacher_path, parsed.precision, device)
    data_args = {"dataset_dir": parsed.dataset_dir, "batch_size": parsed.batch_size, "n_step": 5, "gap": 5}
    if phase == "birdview" and parsed.dataset_dir:
        data_args.update(crop_x_jitter=0, crop_y_jitter=0, angle_jitter=0)
    data_args.update(resident)
    config = {"data_args": data_args, "synthetic": parsed.synthetic, "iters_per_epoch": 100 * int(parsed.batches)}
    _, data_val = make_loaders(config, device, teacher=teacher)      # (--cache-teacher: the loaders run the teacher, once per frame)
    trainer = build_trainer(phase, parsed.model_path, parsed.teacher_path, parsed.batch_size, parsed.precision, device, parsed.fixed_offset,
                            networks=(net, resume.teacher_for_trainer(config, teacher)))
    visuals = trainer.make_visuals(size=draw.get("visuals_size")) if draw else None
    res = validation_pass(trainer, data_val, device, visuals=visuals).result()
    if visuals is not None and visuals.rendered:
        from .visuals import write_png
        write_png(Path(parsed.model_path).parent / "visuals.png", visuals.image())      # (--visuals: the last batch's panels)
    res.update(model_path=str(parsed.model_path), phase=parsed.phase, precision=parsed.precision)
    res["within"] = {"%g" % k: v for k, v in res["within"].items()}
    line = json.dumps(res)
    out = Path(parsed.model_path).parent / "metrics.json"
    tmp = str(out) + ".tmp"
    with open(tmp, "w") as f:
        f.write(line + "\n")
    os.replace(tmp, str(out))
    print(line)
    return res


if __name__ == "__main__":
    main()
