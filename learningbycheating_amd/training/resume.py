"""The flags, config entries and state files of the options the training scripts share: --save_state / --resume / --skip-nonfinite /
--clip-grad-norm / --log-grad-norm / --accumulate / --lr-schedule / --weight-decay / --ema-decay / --val-metrics / --train-metrics /
--visuals / --resident / --cache-teacher.  Every option is declared here once (add_arguments), turned into config entries here (config_entries,
resident_entries: a run without an option writes the config.json it always wrote) and read back here by what the loop calls on logging
iterations and at epoch ends.  The loop itself -- the pass over a loader, the epochs, the launch -- is training/loop.py.

`train_state.th` in log_dir holds everything a continued run needs: NativeTrainer.state_dict() (student, optimizer sidecar in
torch.optim.Adam's format, guard counters), both loaders' states, the last finished epoch and torch's CPU + device RNG states.
Rank 0 writes it; under WORLD_SIZE > 1 every other rank writes its own loader / RNG part (the loaders are seeded by rank) as
`train_state.rank%d.th` beside it.  Every file is written to `<name>.tmp` in the same directory and moved into place with
os.replace: a writer that dies leaves a .tmp nobody reads.  The model-%d.th files are not touched by any of this."""
import contextlib
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
    add_guard_arguments(parser)
    add_clip_arguments(parser)
    add_accumulate_argument(parser)
    add_recipe_arguments(parser)
    add_metrics_arguments(parser)
    add_resident_arguments(parser)


def add_guard_arguments(parser):
    parser.add_argument("--skip-nonfinite", action="store_true",
                        help="skip (on the device, without a host round trip) every optimizer step whose gradients hold a NaN or an infinity")
    parser.add_argument("--max-skipped", type=int, default=50,
                        help="with --skip-nonfinite: abort when more steps than this were skipped in a row (checked on logging iterations)")


def guard_entries(parsed):
    """config entries of --skip-nonfinite / --max-skipped; a run without them writes the config.json it always wrote"""
    return {"skip_nonfinite": True, "max_skipped": int(parsed.max_skipped)} if parsed.skip_nonfinite else {}


def add_resident_arguments(parser):
    parser.add_argument("--resident", action="store_true",
                        help="with --dataset_dir: read the whole dataset once and keep it on the GPU (ResidentLoader); every batch is then "
                             "gathered, cropped / rotated and given its waypoints by kernels, the host only draws indices.  The batches are "
                             "the ones the host loader hands out.  Fails when the dataset does not fit.  Default: off")
    parser.add_argument("--resident-reserve-gb", type=float, default=None, metavar="GB",
                        help="with --resident: device memory to leave free for networks and workspaces (default: what batch 256 in fp32 needs)")
    parser.add_argument("--cache-teacher", action="store_true",
                        help="with --resident, phases 0 and 1: run the frozen teacher once over every frame of both splits while they are "
                             "loaded and keep its waypoints (200 bytes per frame) instead of the bird-view frames; no teacher forward runs "
                             "in any step afterwards and no teacher engine is built.  Default: off")


def resident_entries(parsed, teacher=True):
    """data_args entries of --resident / --resident-reserve-gb / --cache-teacher; a run without them writes the config.json it always
    wrote.  teacher=False: a script without a frozen teacher (train_birdview), which refuses --cache-teacher"""
    cache = bool(getattr(parsed, "cache_teacher", False))
    if cache and not teacher:
        raise SystemExit("--cache-teacher caches the frozen teacher of phases 0 and 1; this script trains the teacher itself, on a jittered "
                         "window that is no function of the frame")
    if not getattr(parsed, "resident", False):
        if getattr(parsed, "resident_reserve_gb", None) is not None:
            raise SystemExit("--resident-reserve-gb needs --resident")
        if cache:
            raise SystemExit("--cache-teacher needs --resident (the cache is built while the dataset is loaded onto the device)")
        return {}
    if not parsed.dataset_dir:
        raise SystemExit("--resident needs --dataset_dir (synthetic frames already live on the device)")
    out = {"resident": True}
    if parsed.resident_reserve_gb is not None:
        if parsed.resident_reserve_gb < 0:
            raise SystemExit("--resident-reserve-gb must not be negative")
        out["resident_reserve_gb"] = float(parsed.resident_reserve_gb)
    if cache:
        out["cache_teacher"] = True
    return out


def teacher_for_trainer(config, teacher):
    """the teacher argument of NativeTrainer: with --cache-teacher the loaders hold the teacher's waypoints and no engine is built"""
    return None if config["data_args"].get("cache_teacher") else teacher


def teacher_arguments(birdview):
    """slot 1 of a batch as NativeTrainer.step's keywords: the bird-view frames for the teacher's forward, or, from a loader with a
    teacher cache, the waypoints themselves"""
    from ..bird_view.utils.datasets.resident import TeacherWaypoints
    return {"teacher_out": birdview} if isinstance(birdview, TeacherWaypoints) else {"birdview": birdview}


def add_metrics_arguments(parser):
    parser.add_argument("--val-metrics", action="store_true",
                        help="the validation pass accumulates waypoint errors in metres on the device (commanded branch: ADE / FDE, per "
                             "command, lateral / longitudinal, share inside 0.5 / 1 / 2 m) and reads them back once, after its last batch, "
                             "instead of reading the loss back after every batch.  Default: off")
    parser.add_argument("--train-metrics", action="store_true",
                        help="the training pass accumulates the same errors and logs ade / fde / bad_rows since the previous logging "
                             "iteration on every logging iteration.  Default: off")


def metrics_entries(parsed):
    """config entries of --val-metrics / --train-metrics; a run without them writes the config.json it always wrote"""
    out = {}
    if getattr(parsed, "val_metrics", False):
        out["val_metrics"] = True
    if getattr(parsed, "train_metrics", False):
        out["train_metrics"] = True
    return out


def add_visuals_arguments(parser):
    parser.add_argument("--visuals", action="store_true",
                        help="draw the reference's waypoint panels (camera frame, coloured bird-view, teacher blue, student red, command and "
                             "loss) on the device on every logging iteration -- one launch, nothing read back -- and write the last grid of "
                             "every pass to log_dir/visuals/<train|val>_birdview_<epoch>.png.  Default: off")
    parser.add_argument("--visuals-size", type=int, default=None, metavar="N",
                        help="with --visuals: panels per grid, 1..32 (default: the reference's 32 / 8 / 16 for phase 0 / phase 1 / bird-view)")


def visuals_entries(parsed):
    """config entries of --visuals / --visuals-size; a run without them writes the config.json it always wrote"""
    size = getattr(parsed, "visuals_size", None)
    if not getattr(parsed, "visuals", False):
        if size is not None:
            raise SystemExit("--visuals-size needs --visuals")
        return {}
    if size is not None and not 1 <= size <= 32:
        raise SystemExit("--visuals-size must lie in 1..32")
    return {"visuals": True} if size is None else {"visuals": True, "visuals_size": int(size)}


def pass_visuals(config, trainer, is_train):
    """the PanelRenderer a pass hands to trainer.step on its logging iterations: with --visuals, on rank 0 (the rank that writes the
    file); None otherwise (the step then launches what it always launched).  One object per trainer and kind, made on first use."""
    if not config.get("visuals") or config.get("rank", 0) != 0:
        return None
    kept = trainer.__dict__.setdefault("_pass_visuals", {})
    if is_train not in kept:
        kept[is_train] = trainer.make_visuals(size=config.get("visuals_size"))
    kept[is_train].rendered = 0
    return kept[is_train]


def log_visuals(visuals, log_image, is_train):
    """the end of a pass with --visuals: if anything was rendered, ONE read-back of the last grid, handed to the logger as `birdview`
    (the reference's key).  -> the array or None"""
    if visuals is None or not visuals.rendered:
        return None
    img = visuals.image()
    log_image(is_train=is_train, birdview=img)
    return img


def pass_metrics(config, trainer, is_train):
    """the WaypointMetrics object a pass hands to every trainer.step, emptied: the validation pass's with --val-metrics, the training
    pass's with --train-metrics, None otherwise (the step then launches what it always launched).  One object per trainer and kind,
    made on first use."""
    if not config.get("train_metrics" if is_train else "val_metrics"):
        return None
    kept = trainer.__dict__.setdefault("_pass_metrics", {})
    if is_train not in kept:
        kept[is_train] = trainer.make_metrics()
    kept[is_train].reset()
    return kept[is_train]


def log_val_metrics(config, metrics, log_scalar, nonfinite=None):
    """the end of a validation pass with --val-metrics: one all_gather of the record under WORLD_SIZE > 1, one read-back (the pass's
    only sync), then loss_mean -- the pass's mean over its samples -- and ade, fde, ade_cmd1..4, fde_cmd1..4 (absent commands left out),
    lateral, longitudinal, within_<thr> and bad_rows, which the epoch record holds as val_ade, val_fde, ... beside val_loss_mean.  nonfinite: the message of the
    FloatingPointError raised when a per-sample loss was not finite and --skip-nonfinite is off (phase 1).  -> the result"""
    from .metrics import log_entries
    res = metrics.result(metrics.all_gather() if config["world_size"] > 1 else None)
    if nonfinite is not None and res["loss_bad"] > 0 and not config.get("skip_nonfinite"):
        raise FloatingPointError(nonfinite % ("non-finite for %d of %d samples" % (res["loss_bad"], res["samples"])))
    if res["loss_mean"] is not None:
        log_scalar(is_train=False, loss_mean=res["loss_mean"])
    log_scalar(is_train=False, **log_entries(res))
    return res


def log_train_metrics(metrics, log_scalar):
    """a logging iteration of a training pass with --train-metrics (the loop syncs there anyway): ade / fde / bad_rows of this rank's
    batches since the previous logging iteration, then the record is emptied"""
    res = metrics.result()
    entries = {k: res[k] for k in ("ade", "fde") if res[k] is not None}
    log_scalar(is_train=True, bad_rows=res["bad_rows"], **entries)
    metrics.reset()
    return res


def add_recipe_arguments(parser, per_epoch=False):
    """per_epoch: the script re-creates its optimizer every epoch (phase 2), and the schedule with it"""
    again = "  The schedule restarts with the optimizer at every epoch, as Adam's step count does here." if per_epoch else ""
    parser.add_argument("--lr-schedule", choices=["constant", "cosine", "step"], default=None,
                        help="learning-rate schedule with --lr as its base rate, evaluated on the device at Adam's own step count (optimizer "
                             "steps: a skipped step does not advance it, --accumulate K advances it once per K iterations); implies "
                             "--skip-nonfinite.  Default: the constant --lr." + again)
    parser.add_argument("--warmup-steps", type=int, default=0, metavar="W", help="linear warm-up over the first W optimizer steps")
    parser.add_argument("--warmup-start", type=float, default=0.0, metavar="S0", help="the warm-up starts at S0 x --lr (default 0)")
    parser.add_argument("--lr-total-steps", type=int, default=None, metavar="T",
                        help="cosine: the rate reaches --lr-min at optimizer step T and stays there (required for cosine)")
    parser.add_argument("--lr-min", type=float, default=0.0, help="cosine: the final rate")
    parser.add_argument("--lr-step-size", type=int, default=1, metavar="S", help="step: multiply the rate by --lr-gamma every S optimizer steps")
    parser.add_argument("--lr-gamma", type=float, default=0.1, help="step: the factor")
    parser.add_argument("--weight-decay", type=float, default=0.0, metavar="X",
                        help="decoupled weight decay (torch.optim.AdamW: p *= 1 - lr * X in front of every update, every parameter); "
                             "implies --skip-nonfinite.  Default 0: off" + again)
    parser.add_argument("--ema-decay", type=float, default=None, metavar="D",
                        help="keep an exponential moving average of the weights, e += (1 - D) (p - e) inside every applied optimizer step, "
                             "and write model-ema-%%d.th beside every model-%%d.th; implies --skip-nonfinite.  Default: off")
    parser.add_argument("--ema-eval", action="store_true", help="with --ema-decay: run the validation pass on the averaged weights")


def recipe_entries(parsed):
    """config entries of --lr-schedule (and its companions) / --weight-decay / --ema-decay (/ --ema-eval), plus the guard they imply; a run
    without them writes the config.json it always wrote"""
    out = {}
    if parsed.lr_schedule is not None or parsed.warmup_steps:
        kind = parsed.lr_schedule or "constant"
        if kind == "cosine" and parsed.lr_total_steps is None:
            raise SystemExit("--lr-schedule cosine needs --lr-total-steps T (optimizer steps)")
        if parsed.warmup_steps < 0 or not 0.0 <= parsed.warmup_start <= 1.0:
            raise SystemExit("--warmup-steps must not be negative and --warmup-start must lie in [0, 1]")
        sch = {"kind": kind, "warmup_steps": int(parsed.warmup_steps), "warmup_start": float(parsed.warmup_start)}
        if kind == "cosine":
            if parsed.lr_total_steps <= parsed.warmup_steps:
                raise SystemExit("--lr-total-steps must be larger than --warmup-steps")
            sch.update(total_steps=int(parsed.lr_total_steps), min_lr=float(parsed.lr_min))
        if kind == "step":
            if parsed.lr_step_size < 1 or not parsed.lr_gamma > 0:
                raise SystemExit("--lr-step-size must be at least 1 and --lr-gamma positive")
            sch.update(step_size=int(parsed.lr_step_size), gamma=float(parsed.lr_gamma))
        out["lr_schedule"] = sch
    if parsed.weight_decay:
        if not parsed.weight_decay > 0:
            raise SystemExit("--weight-decay must not be negative")
        out["weight_decay"] = float(parsed.weight_decay)
    if parsed.ema_decay is not None:
        if not 0.0 < parsed.ema_decay < 1.0:
            raise SystemExit("--ema-decay must lie in (0, 1)")
        out["ema_decay"] = float(parsed.ema_decay)
        if parsed.ema_eval:
            out["ema_eval"] = True
    elif parsed.ema_eval:
        raise SystemExit("--ema-eval needs --ema-decay")
    if out:
        out.update(skip_nonfinite=True, max_skipped=int(parsed.max_skipped))
    return out


def recipe_kwargs(config):
    """the entries above as NativeTrainer's (lr_schedule, weight_decay, ema_decay) keywords; {} for a run without them"""
    return {k: config[k] for k in ("lr_schedule", "weight_decay", "ema_decay") if k in config}


def trainer_kwargs(config):
    """NativeTrainer's keywords of the guard, the clip, --accumulate and the entries above"""
    return dict(skip_nonfinite=config.get("skip_nonfinite", False), max_grad_norm=config.get("max_grad_norm"),
                accumulate=int(config.get("accumulate", 1)), **recipe_kwargs(config))


def log_lr_stats(config, trainer, log_scalar, **tags):
    """on a logging iteration of a run with a schedule / decay / average: lr of the last applied step and, with the average, ema_updates (a sync)"""
    if not recipe_kwargs(config):
        return None
    st = trainer.lr_stats()
    if st["lr"] is not None:                  # (None: no step has been applied yet)
        log_scalar(lr=st["lr"], **tags)
    if "ema_decay" in config:
        log_scalar(ema_updates=st["ema_updates"], **tags)
    return st


def ema_eval(config, trainer):
    """--ema-eval: the context the validation pass runs in (the averaged weights); without the flag a context that does nothing"""
    return trainer.ema_weights() if config.get("ema_eval") else contextlib.nullcontext()


def save_ema_model(config, trainer, epoch):
    """--ema-decay: model-ema-%d.th beside model-%d.th, the same layout (the student's state_dict with the averaged parameters)"""
    if "ema_decay" in config:
        torch.save(trainer.ema_state_dict(), str(Path(config["log_dir"]) / ("model-ema-%d.th" % epoch)))


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
    out.update(guard_entries(parsed))
    out.update(clip_entries(parsed))
    out.update(accumulate_entries(parsed))
    out.update(recipe_entries(parsed))
    out.update(metrics_entries(parsed))
    out.update(visuals_entries(parsed))
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
