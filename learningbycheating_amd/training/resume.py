"""What the training scripts share for --save_state / --resume / --skip-nonfinite / --clip-grad-norm / --log-grad-norm / --accumulate.

`train_state.th` in log_dir holds everything a continued run needs: NativeTrainer.state_dict() (student, optimizer sidecar in
torch.optim.Adam's format, guard counters), both loaders' states, the last finished epoch and torch's CPU + device RNG states.
Rank 0 writes it; under WORLD_SIZE > 1 every other rank writes its own loader / RNG part (the loaders are seeded by rank) as
`train_state.rank%d.th` beside it.  Every file is written to `<name>.tmp` in the same directory and moved into place with
os.replace: a writer that dies leaves a .tmp nobody reads.  The model-%d.th files are not touched by any of this."""
import os
from pathlib import Path

import torch
import torch.distributed as dist

STATE_NAME = "train_state.th"


def add_arguments(parser, with_resume=True):
    parser.add_argument("--save_state", action="store_true", help="write train_state.th (model, optimizer, loaders, RNG) after every epoch")
    parser.add_argument("--save_state_every", type=int, default=0, help="... and every N training iterations inside an epoch")
    if with_resume:
        parser.add_argument("--resume", action="store_true", help="continue from log_dir/train_state.th when there is one")
    parser.add_argument("--seed", type=int, default=None,
                        help="seed torch's generators before the networks are built (default: unseeded, as the reference): two runs with "
                             "the same seed and flags start from the same weights")
    parser.add_argument("--skip-nonfinite", action="store_true",
                        help="skip (on the device, without a host round trip) every optimizer step whose gradients hold a NaN or an infinity")
    parser.add_argument("--max-skipped", type=int, default=50,
                        help="with --skip-nonfinite: abort when more steps than this were skipped in a row (checked on logging iterations)")
    add_clip_arguments(parser)
    add_accumulate_argument(parser)


def add_accumulate_argument(parser):
    parser.add_argument("--accumulate", type=int, default=1, metavar="K",
                        help="sum the gradients of K loader iterations (micro-batches) on the device before every optimizer step: "
                             "K x batch_size is the optimizer's batch; BatchNorm still normalises each micro-batch on its own.  Default 1: off")


def accumulate_entries(parsed):
    """config entry of --accumulate; a run without it writes the config.json it always wrote"""
    if parsed.accumulate < 1:
        raise SystemExit("--accumulate needs a positive number of micro-batches")
    return {"accumulate": int(parsed.accumulate)} if parsed.accumulate != 1 else {}


class Windows:
    """what a training pass of a run with --accumulate K counts: loader iterations go on counting as they always did, `optimizer_steps`
    counts the windows of K micro-batches this pass has closed (each one update, applied or skipped by the guard).  Without the flag
    every method does nothing and logs nothing."""

    def __init__(self, config, trainer, first_iteration=0):
        self.k, self.trainer = int(config.get("accumulate", 1)), trainer
        self.optimizer_steps = int(first_iteration) // self.k      # (a pass continued from a state: states are written at boundaries)

    def after_step(self, updated):
        """call after every trainer.step of the pass; updated: the step ran with update=True"""
        if self.k > 1 and updated and self.trainer.accum_index == 0:
            self.optimizer_steps += 1

    def log(self, log_scalar, **tags):
        if self.k > 1:
            log_scalar(optimizer_steps=self.optimizer_steps, **tags)

    def end_pass(self, log_scalar, **tags):
        """the end of an epoch: an incomplete window is discarded (the epoch-end state is then always at a window boundary) and the
        number of micro-batches it held is logged as dropped_micro_batches.  -> that number"""
        if self.k <= 1:
            return 0
        dropped = self.trainer.reset_accumulation()
        log_scalar(dropped_micro_batches=dropped, **tags)
        return dropped


def add_clip_arguments(parser):
    parser.add_argument("--clip-grad-norm", type=float, default=None, metavar="X",
                        help="clip the gradients to global L2 norm X (torch.nn.utils.clip_grad_norm_) on the device, inside the optimizer "
                             "step; implies --skip-nonfinite.  Default: off")
    parser.add_argument("--log-grad-norm", action="store_true",
                        help="measure the global gradient norm on the device without clipping (implies --skip-nonfinite); logging "
                             "iterations report grad_norm, clip_coef and clipped_steps")


def clip_entries(parsed):
    """config entries of --clip-grad-norm / --log-grad-norm: max_grad_norm (0 = measure only) plus the guard they imply"""
    if parsed.clip_grad_norm is not None:
        if not parsed.clip_grad_norm > 0:
            raise SystemExit("--clip-grad-norm needs a positive norm (use --log-grad-norm to measure without clipping)")
        return {"max_grad_norm": float(parsed.clip_grad_norm), "skip_nonfinite": True, "max_skipped": int(parsed.max_skipped)}
    if parsed.log_grad_norm:
        return {"max_grad_norm": 0.0, "skip_nonfinite": True, "max_skipped": int(parsed.max_skipped)}
    return {}


def log_grad_stats(config, trainer, log_scalar, **tags):
    """on a logging iteration of a run with --clip-grad-norm / --log-grad-norm: grad_norm, clip_coef and clipped_steps (a sync)"""
    if config.get("max_grad_norm") is None:
        return None
    st = trainer.grad_stats()
    log_scalar(grad_norm=st["grad_norm"], clip_coef=st["clip_coef"], clipped_steps=st["clipped_total"], **tags)
    return st


def config_entries(parsed):
    """config entries of the options that were given: a run without them writes the config.json it always wrote.  Also applies --seed
    (call this before the networks are built)."""
    out = {}
    if parsed.seed is not None:
        torch.manual_seed(parsed.seed)
        out["seed"] = int(parsed.seed)
    if parsed.save_state or parsed.save_state_every > 0:
        out.update(save_state=True, save_state_every=int(parsed.save_state_every))
    if getattr(parsed, "resume", False):
        out["resume"] = True
    if parsed.skip_nonfinite:
        out.update(skip_nonfinite=True, max_skipped=int(parsed.max_skipped))
    out.update(clip_entries(parsed))
    out.update(accumulate_entries(parsed))
    return out


def _path(log_dir, rank):
    return Path(log_dir) / (STATE_NAME if rank == 0 else "train_state.rank%d.th" % rank)


def _atomic_save(obj, path):
    tmp = str(path) + ".tmp"
    torch.save(obj, tmp)
    os.replace(tmp, str(path))


def save(config, trainer, loaders, epoch, extra=None):
    """epoch: the last FINISHED epoch; a state written inside an epoch carries the epoch before it and loaders that stand in the
    middle of their pass"""
    if not config.get("save_state"):
        return
    rank, device = config["rank"], config["device"]
    part = {"format": 1, "epoch": int(epoch), "world_size": int(config["world_size"]), "rank": int(rank),
            "loaders": {k: v.state_dict() for k, v in loaders.items() if hasattr(v, "state_dict")},
            "rng": {"cpu": torch.get_rng_state(), "device": torch.cuda.get_rng_state(device)}}
    if extra:
        part["extra"] = extra
    if rank == 0:
        part["trainer"] = trainer.state_dict()
    _atomic_save(part, _path(config["log_dir"], rank))
    if config["world_size"] > 1:
        dist.barrier()             # (nobody runs ahead of a state that is only half on disk)


def load(config, trainer, loaders):
    """-> the state's dict (its "epoch" is the last finished one) or None when log_dir has no train_state.th.  Model and optimizer
    are restored on every rank from rank 0's file; loaders and RNG from the rank's own part, unless the world size changed: then
    the loaders start fresh at the epoch boundary, and the log says so."""
    path = _path(config["log_dir"], 0)
    if not config.get("resume") or not path.exists():
        return None
    rank, world, device = config["rank"], config["world_size"], config["device"]
    state = torch.load(str(path), map_location="cpu")
    for note in trainer.load_state_dict(state["trainer"]):
        if rank == 0:
            print("resume: " + note)
    mine = state if rank == 0 else None
    if int(state["world_size"]) != world:
        mine = None
        if rank == 0:
            print("resume: %s was written under world size %d, this run has %d: model and optimizer restored, loaders and random "
                  "streams start fresh at the epoch boundary" % (path.name, state["world_size"], world))
    elif rank != 0:
        own = _path(config["log_dir"], rank)
        if own.exists():
            mine = torch.load(str(own), map_location="cpu")
            if mine["epoch"] != state["epoch"]:
                mine = None
        if mine is None:
            print("resume: rank %d has no loader state of epoch %d: its loaders start fresh" % (rank, state["epoch"]))
    if mine is not None:
        for k, v in loaders.items():
            if k in mine["loaders"]:
                v.load_state_dict(mine["loaders"][k])
        torch.set_rng_state(mine["rng"]["cpu"])
        torch.cuda.set_rng_state(mine["rng"]["device"], device)
    if rank == 0:
        print("resuming from %s: epoch %d finished, Adam step %d" % (path, state["epoch"], trainer.opt.step_count))
    return state


def maybe_save_inside_epoch(config, trainer, loaders, epoch, iteration):
    """--save_state_every N: after training iteration `iteration` (1-based) of epoch `epoch`.  With --accumulate K a state is only
    written at a window boundary (NativeTrainer.state_dict refuses an open window): the first boundary at or after every multiple of N."""
    n = config.get("save_state_every", 0)
    k = int(config.get("accumulate", 1))
    if n > 0 and trainer.accum_index == 0 and iteration // n > (iteration - k) // n:
        save(config, trainer, loaders, epoch - 1)


def check_skipped(config, trainer, phase):
    """on a logging iteration (the loop syncs there anyway): -> steps skipped so far; FloatingPointError when more than --max-skipped
    were skipped in a row -- isolated steps on the 1 / y pole are expected, a run of them means the objective is no longer defined
    where the model is"""
    if not config.get("skip_nonfinite"):
        return None
    total, row = trainer.skipped()
    if row > config["max_skipped"]:
        raise FloatingPointError("%s: %d optimizer steps in a row had non-finite gradients (%d skipped in all, --max-skipped %d): the "
                                 "loss is non-finite wherever the model now predicts" % (phase, row, total, config["max_skipped"]))
    return total
