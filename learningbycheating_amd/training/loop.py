"""What runs in the training scripts, once: the launch (ranks, device, process group), the arguments every script declares, one loader
batch -> one NativeTrainer.step, the pass over a loader (`train_or_eval`) and the epoch loop around it.  resume.py holds the options'
flags, config entries and state files; the scripts hold what differs between them (a Spec, their own arguments, build_config, the
networks and the trainer)."""
import collections
import math
import os
import time
from pathlib import Path

import torch
import torch.distributed as dist

from ..bird_view.utils import bz_utils as bzu
from ..bird_view.utils.train_utils import one_hot
from . import resume

# what a script's passes and epochs differ in.  label: the script's name in check_skipped's error; images_per_sec: log it beside fps;
# nonfinite: None, or the message (two %s: which loss, its value) of the FloatingPointError a non-finite loss raises without
# --skip-nonfinite; save_epochs: the epochs that write model-%d.th
Spec = collections.namedtuple("Spec", "label images_per_sec nonfinite save_epochs")


# ---- launch ------------------------------------------------------------------------------------------------------------------------
def ranks():
    """-> (world, rank, local) as torch.distributed.run hands them to every process; (1, 0, 0) without it"""
    return int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))


def select_device(local, what="training"):
    """make GPU `local` the process's device.  -> the torch.device"""
    if not torch.cuda.is_available():
        raise SystemExit("%s needs a ROCm GPU" % what)
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    return device


def launch(parsed, build_config, run):
    """a script's main after its arguments are parsed: build_config(parsed, rank, world, device) -> config runs first and holds every
    check of the flags, so a bad flag line exits before the device is touched; then the device, the process group under
    WORLD_SIZE > 1, run(config), and the group's teardown.  -> what run returns"""
    world, rank, local = ranks()
    config = build_config(parsed, rank, world, torch.device("cuda", local))
    select_device(local)
    if world > 1:
        dist.init_process_group("nccl")
    out = run(config)
    if world > 1:
        dist.destroy_process_group()
    return out


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def add_precision_argument(parser):
    parser.add_argument("--precision", choices=["fp32", "bf16", "bf16_mfma", "bf16x3"], default="fp32",
                        help="fp32 = the reference arithmetic; bf16 = bf16 MFMA operands + bf16 activation storage, f32 master weights; "
                             "bf16x3 = split-bf16 convolution operands (f32-accurate), f32 tensors")


def add_common_arguments(parser, max_epoch, batch_size):
    """the arguments of all three supervised scripts; the two defaults are the reference's, which differ per script"""
    parser.add_argument("--log_dir", required=True)
    parser.add_argument("--log_iterations", default=1000)
    parser.add_argument("--max_epoch", default=max_epoch)
    parser.add_argument("--dataset_dir", default=None)
    parser.add_argument("--batch_size", type=int, default=batch_size)
    parser.add_argument("--lr", type=float, default=1e-4)
    parser.add_argument("--synthetic", type=int, default=2048, help="number of device-resident synthetic frames (used when no --dataset_dir is given)")
    parser.add_argument("--iters_per_epoch", type=int, default=1000)
    add_precision_argument(parser)
    resume.add_visuals_arguments(parser)


# ---- one batch, one pass, the epochs -----------------------------------------------------------------------------------------------
def step_batch(trainer, batch, device, speed_noise=0, **keywords):
    """one loader batch -> one trainer.step(**keywords): the bird-view frames and the ground-truth waypoints for the privileged agent,
    the camera image and slot 1 for the teacher otherwise (--cache-teacher: slot 1 holds the teacher's cached waypoints instead of the
    frames its forward would read).  speed_noise > 0: the reference's noise on the measured speed.  Nothing is read back.  -> the loss"""
    rgb_image, birdview, location, command, speed = batch
    command = one_hot(command).to(device)
    if speed_noise > 0:
        speed = torch.clamp(speed + torch.randn_like(speed) * speed_noise, 0, 10)
    if trainer.phase == "birdview":
        return trainer.step(birdview, speed, command, target=location.float().contiguous(), **keywords)
    return trainer.step(rgb_image, speed, command, **keywords, **resume.teacher_arguments(birdview))


def run_pass(spec, trainer, data, is_train, config, is_first_epoch, epoch=0, loaders=None):
    """the scripts' train_or_eval (reference train_image_phase1.py:157-229, train_image_phase0.py:152-209, train_birdview.py:102-153);
    epoch 0 is the reference's 11-iteration dry run without updates"""
    tick = time.time()
    update = is_train and not is_first_epoch
    first = getattr(data, "resume_at", 0)        # (a loader restored in the middle of its pass hands out the rest of it: the iteration count goes on where it stood)
    windows = resume.Windows(config, trainer, first)                 # (--accumulate: iterations stay loader iterations)
    metrics = resume.pass_metrics(config, trainer, is_train)         # (--val-metrics / --train-metrics; None without them)
    sync_free = metrics is not None and not is_train                 # the validation pass with --val-metrics reads nothing back per batch
    visuals = resume.pass_visuals(config, trainer, is_train)         # (--visuals, rank 0; None without it)
    noise = config.get("speed_noise", 0) if is_train else 0
    for i, batch in enumerate(data, start=first):
        should_log = (i % int(config["log_iterations"]) == 0) or (not is_train) or is_first_epoch
        # (--visuals: a logging iteration's step carries the renderer -- one more launch, nothing read back)
        draw = {"visuals": visuals} if (visuals is not None and should_log) else {}
        loss = step_batch(trainer, batch, config["device"], noise, update=update, train_mode=is_train, metrics=metrics, **draw)
        windows.after_step(update)
        if should_log and not sync_free:
            lm = loss.mean().item()          # device->host sync only when logging, as the reference (train_image_phase1.py:207-221)
            skipped = resume.check_skipped(config, trainer, spec.label) if is_train else None
            if skipped is not None:
                bzu.log.scalar(is_train=is_train, skipped_steps=skipped)
            if is_train:
                resume.log_grad_stats(config, trainer, bzu.log.scalar, is_train=is_train)
                resume.log_lr_stats(config, trainer, bzu.log.scalar, is_train=is_train)
            if spec.nonfinite and not math.isfinite(lm) and not config.get("skip_nonfinite"):
                raise FloatingPointError(spec.nonfinite % ("loss", lm))
            bzu.log.scalar(is_train=is_train, loss_mean=lm)
            if metrics is not None:
                resume.log_train_metrics(metrics, bzu.log.scalar)
            if update:
                windows.log(bzu.log.scalar, is_train=is_train)
        now = time.time()
        rates = {"images_per_sec": batch[0].shape[0] * config["world_size"] / max(now - tick, 1e-9)} if spec.images_per_sec else {}
        bzu.log.scalar(is_train=is_train, fps=1.0 / max(now - tick, 1e-9), **rates)
        tick = now
        if update and loaders is not None:
            resume.maybe_save_inside_epoch(config, trainer, loaders, epoch, i + 1)
        if is_first_epoch and i == 10:
            break
    if update:
        windows.end_pass(bzu.log.scalar, is_train=is_train)
    if sync_free:
        resume.log_val_metrics(config, metrics, bzu.log.scalar, nonfinite=spec.nonfinite and spec.nonfinite % ("validation loss", "%s"))
    resume.log_visuals(visuals, bzu.log.image, is_train)             # (--visuals: the pass's one read-back of the last rendered grid)


def run_epochs(spec, config, net, trainer, loaders, state):
    """a script's epochs: a training pass and a validation pass each (the reference validates after every epoch), model-%d.th on
    spec.save_epochs, the epoch's record, train_state.th.  state: what resume.load returned (the run goes on after its epoch) or None"""
    rank = config["rank"]
    for epoch in range(state["epoch"] + 1 if state else 0, int(config["max_epoch"]) + 1):
        net.train()
        run_pass(spec, trainer, loaders["train"], True, config, epoch == 0, epoch, loaders)
        net.eval()
        with resume.ema_eval(config, trainer):       # (--ema-eval: the validation pass sees the averaged weights)
            run_pass(spec, trainer, loaders["val"], False, config, epoch == 0)
        net.train()
        if epoch in spec.save_epochs and rank == 0:
            torch.save(net.state_dict(), str(Path(config["log_dir"]) / ("model-%d.th" % epoch)))
            resume.save_ema_model(config, trainer, epoch)
        rec = bzu.log.end_epoch()
        if rank == 0:
            print(rec)
        resume.save(config, trainer, loaders, epoch)
    return net
