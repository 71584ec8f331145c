"""Phase-2 (on-policy distillation / DAgger) of the sensorimotor agent -- the offline half
(reference training/train_image_phase2.py:152-258 `_train`), MI355X-native.

`rollout` (train_image_phase2.py:61-149) drives a live CARLA server and is outside the hot path; here the replay buffer is
filled from device-resident synthetic frames (BASELINE.json config 5).  `_train` is the phase-1 step plus, per sample,
the resampling weight get_weight(...) of the selected branch (HIP kernel lbc_phase2_weight) written back to the buffer;
the optimizer is re-created every epoch exactly as the reference does (train_image_phase2.py:164, moments reset).

--replay device (default host: the loop above, unchanged) keeps the replay buffer and everything a step touches on the device
(training/replay.py DeviceReplayBuffer, csrc/replay.hip): the weighted draw, the gather of the uint8 frames straight into the networks'
fused u8 input pass and the weight write-back are kernels, and the loop body has no host round trip outside logging iterations.  With it
come the reference buffer's --augment / --aug_fix_iter / --batch_aug (phase2_utils.py:191,224-234) and --save_state / --resume / --seed:
log_dir/train_state.th after every epoch (student, buffer state, augmenter stream, RNG, (episode, epoch)); a resumed run continues with
the next epoch bit for bit.

--dataset_dir DIR (with --replay device) trains on a recorded dataset: the train split is read once and kept in HBM (ResidentLoader),
and every episode begins with an offline rollout (training/rollout.py): --rollout_frames recorded frames are scored with the current
student against the teacher, both in eval mode, and admitted into a buffer of --buffer_limit slots that holds frame indices into the
resident dataset (lbc_replay_admit keeps the highest weights).  Then the epochs above run on it.  The states are the recorded ones, not
the student's own: this is loss-prioritised replay over the dataset, the learner half of DAgger without its on-policy data.

--env MODULE:FACTORY (with --replay device) is the on-policy loop: FACTORY(n_envs=, rank=, world=, **--env_kwargs) builds an object of the
environment protocol (training/rollout.py; `--env synthetic` is the toy training/envs.py SyntheticEnv), and every episode begins with
OnlineRollout.run(episode): the student drives --n_envs environments with the reference's mixing schedule (--beta), the teacher labels the
same states, and --episode_length frames per environment go into a copying buffer of --buffer_limit slots (teaching.TeachingSession; the
tick, the scoring and the recording stay on the device).  Then the epochs above run on it."""
import argparse
import ctypes
import json
import time
from pathlib import Path

import torch
import torch.distributed as dist

from .. import _lib
from ..bird_view import augmenter as augmenter_mod
from ..bird_view.models.birdview import BirdViewPolicyModelSS
from ..bird_view.models.image import ImagePolicyModelSS
from ..bird_view.utils import bz_utils as bzu
from ..bird_view.utils.train_utils import one_hot
from ..optim import FusedAdam
from ..parallel import broadcast_module
from . import loop, resume
from .native import NativeTrainer, camera_struct
from .phase2_utils import ReplayBuffer
from .replay import DeviceReplayBuffer

BACKBONE = "resnet34"
SAVE_EPISODES = list(range(20))


def phase2_weights(trainer, p_sel, t_sel):
    n = p_sel.shape[0]
    w = torch.empty(n, dtype=torch.float32, device=p_sel.device)
    _lib.check(_lib.get().lbc_phase2_weight(ctypes.byref(trainer.cam), _lib.ptr(p_sel), _lib.ptr(t_sel), n, _lib.ptr(w),
                                            _lib.stream_for(p_sel)), "phase2_weight")
    return w


def _fresh_optimizer(trainer, config, lr):
    """fresh moments each epoch, as the reference re-creates its Adam there.  With --clip-grad-norm / --log-grad-norm the number of
    clipped steps goes on counting across the epochs of a run (read and written at the epoch boundary, where the loop syncs anyway).
    --lr-schedule / --weight-decay go to every one of these optimizers: the schedule restarts with Adam's step count at every epoch."""
    clipped = trainer.opt.grad_stats()["clipped_total"]
    # (--accumulate: the optimizer reads the accumulation buffer; the loop closes every epoch at a window boundary)
    grads = trainer.accum_views if trainer.accum_views is not None else trainer.eng.grad_views
    trainer.opt = FusedAdam(list(trainer.student.named_parameters()), grads, lr=lr,
                            guarded=config.get("skip_nonfinite", False), max_grad_norm=config.get("max_grad_norm"), **_recipe(config))
    trainer.opt.set_clipped(clipped)


def _recipe(config):
    """FusedAdam's keywords of --lr-schedule / --weight-decay; {} for a run without them"""
    out = {}
    if "lr_schedule" in config:
        out["schedule"] = config["lr_schedule"]
    if "weight_decay" in config:
        out.update(weight_decay=config["weight_decay"], decoupled_weight_decay=True)
    return out


def _log_guard(trainer, config):
    """on a logging iteration: skipped_steps (and the abort on a run of them), grad_norm / clip_coef / clipped_steps"""
    skipped = resume.check_skipped(config, trainer, "phase 2")
    if skipped is not None:
        bzu.log.scalar(skipped_steps=skipped)
    resume.log_grad_stats(config, trainer, bzu.log.scalar)
    resume.log_lr_stats(config, trainer, bzu.log.scalar)


def _train(replay_buffer, trainer, config, episode):
    device = config["device"]
    bs = config["batch_size"]
    net, teacher_net = trainer.student, trainer.teacher
    for epoch in range(config["epoch_per_episode"]):
        _fresh_optimizer(trainer, config, 1e-4)
        net.train()
        replay_buffer.init_new_weights()
        windows = resume.Windows(config, trainer)
        for i in range(len(replay_buffer) // bs):                                              # drop_last=True
            idx = replay_buffer.sample_indices(bs)
            rgb, bv, cmd, speed = replay_buffer.batch(idx)
            command = one_hot(cmd).to(device)
            if config["speed_noise"] > 0:
                speed = torch.clamp(speed + torch.randn_like(speed) * config["speed_noise"], 0, 10)
            loss = trainer.step(rgb, speed, command, birdview=bv)
            windows.after_step(True)
            replay_buffer.update_weights(idx, phase2_weights(trainer, trainer.last_pred[0], trainer.last_teacher[0]))
            if i % int(config["log_iterations"]) == 0:
                bzu.log.scalar(loss_mean=loss.mean().item())
                windows.log(bzu.log.scalar)
                _log_guard(trainer, config)
        windows.end_pass(bzu.log.scalar)
        replay_buffer.normalize_weights()
        # the reference evaluates (eval mode) and visualises the 32 highest-weight samples here (:229-250); this loop does not draw them
        # (training/visuals.py PanelRenderer(mode=1, size=16) renders such panels on the device from a step's tensors), the forward is
        # kept so that the same kernels run
        top, rgb, bv, cmd, speed = replay_buffer.get_highest_k(min(32, len(replay_buffer)))
        net.eval()
        with torch.no_grad():
            net(rgb, speed, one_hot(cmd).to(device))
        net.train()
        bzu.log.end_epoch()
    if episode in SAVE_EPISODES and config["rank"] == 0:
        torch.save(net.state_dict(), str(Path(config["log_dir"]) / ("model-%d.th" % episode)))


def synthetic_buffer(n_frames, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    buf = ReplayBuffer(device, buffer_limit=n_frames, seed=seed)
    step = 1024
    for s in range(0, n_frames, step):
        n = min(step, n_frames - s)
        buf.add_batch(torch.randint(0, 256, (n, 160, 384, 3), generator=g, dtype=torch.uint8),
                      (torch.rand((n, 192, 192, 7), generator=g) < 0.1).to(torch.uint8),
                      torch.randint(1, 5, (n,), generator=g), torch.rand(n, generator=g) * 10, [1.0] * n)
    return buf


# ---- --replay device ---------------------------------------------------------------------------------------------
def synthetic_buffer_device(n_frames, device, seed=0):
    """synthetic_buffer's frames (same generator, same order) in a DeviceReplayBuffer; the bird view as the dataset stores it, 0/255"""
    g = torch.Generator().manual_seed(seed)
    buf = DeviceReplayBuffer(device, buffer_limit=n_frames, seed=seed)
    step = 1024
    for s in range(0, n_frames, step):
        n = min(step, n_frames - s)
        buf.add_batch(torch.randint(0, 256, (n, 160, 384, 3), generator=g, dtype=torch.uint8),
                      (torch.rand((n, 192, 192, 7), generator=g) < 0.1).to(torch.uint8) * 255,
                      torch.randint(1, 5, (n,), generator=g), torch.rand(n, generator=g) * 10, [1.0] * n)
    return buf


def dataset_buffer(config, trainer, seed=None):
    """--dataset_dir: the train split resident in HBM the way train_image_phase1 --resident holds it (no teacher cache: phase 2 runs
    the teacher), an empty buffer of this rank's share of --buffer_limit slots that indexes it, and the rollout that fills it from this
    rank's share of the frames, --rollout_frames / world of them per episode.  -> (buffer, rollout)"""
    from ..bird_view.utils.datasets.image_lmdb import ImageDataset
    from ..bird_view.utils.datasets.resident import ResidentLoader
    from .rollout import OfflineRollout
    rank, world, device = config["rank"], config["world_size"], config["device"]
    data = ImageDataset(str(Path(config["dataset_dir"]) / "train"))
    store = ResidentLoader(data, config["batch_size"], 0, device, seed=0, rank=rank, reserve_gb=config.get("resident_reserve_gb"))
    buf = DeviceReplayBuffer(device, buffer_limit=max(1, config["buffer_limit"] // world), seed=rank, source=store)
    per_rank = config["rollout_frames"] // world if config["rollout_frames"] else 0
    if config["rollout_frames"] and per_rank < 1:
        raise SystemExit("train_image_phase2: --rollout_frames %d is less than one frame per rank" % config["rollout_frames"])
    rollout = OfflineRollout(store, trainer, buf, per_rank, seed=0 if seed is None else int(seed), rank=rank, world=world)
    return buf, rollout


def make_augmenter(config):
    """the reference buffer's augmenter (phase2_utils.py:201-204,225-226): the recipe at the FIXED image counter aug_fix_iter"""
    strategy = augmenter_mod.get(config.get("augment"))
    if strategy is None:
        return None
    return augmenter_mod.BatchAugmenter(strategy(int(config.get("aug_fix_iter", 1000000))), seed=config["rank"])


def _device_step(replay_buffer, trainer, config, augmenter=None):
    """one iteration of _train_device: draw, gather (+ --batch_aug copies, + augmentation), step, write the weights back.  Everything
    is enqueued; nothing here reads from the device.  -> (indices (B,), per-image loss (B * batch_aug,))"""
    reps = int(config.get("batch_aug", 1) or 1)
    idx = replay_buffer.sample_indices(config["batch_size"])
    rgb, bv, command, speed = replay_buffer.batch(idx, reps)
    if augmenter is not None:
        augmenter.augment_batch(rgb)
    if config["speed_noise"] > 0:
        speed = torch.clamp(speed + torch.randn_like(speed) * config["speed_noise"], 0, 10)
    loss = trainer.step(rgb, speed, command, birdview=bv)
    replay_buffer.update_weights(idx, phase2_weights(trainer, trainer.last_pred[0], trainer.last_teacher[0]), reps)
    return idx, loss


def _state_path(config):
    return resume._path(config["log_dir"], config["rank"])


def online_rollout(config, trainer, seed=None):
    """--env: the environments of this rank, the session that drives them on the trainer's own engines, an empty copying buffer of this
    rank's share of --buffer_limit slots.  -> (buffer, rollout)"""
    import importlib
    from ..teaching import TeachingSession
    from .rollout import OnlineRollout
    rank, world, device = config["rank"], config["world_size"], config["device"]
    if config["env"] == "synthetic":
        from .envs import SyntheticEnv as factory
    else:
        module, _, name = config["env"].partition(":")
        factory = getattr(importlib.import_module(module), name)
    env = factory(n_envs=config["n_envs"], rank=rank, world=world, **config["env_kwargs"])
    session = TeachingSession(trainer.student, trainer.teacher, device, config["n_envs"], config["episode_length"], camera=trainer.cam,
                              seed=(0 if seed is None else int(seed)) * 7919 + rank)
    buf = DeviceReplayBuffer(device, buffer_limit=max(1, config["buffer_limit"] // world), seed=rank)
    return buf, OnlineRollout(session, buf, env, config["episode_length"], beta=config["beta"])


def save_state_device(config, net, replay_buffer, augmenter, episode, epoch, rollout=None):
    """train_state.th (rank 0; train_state.rank%d.th on the others) after epoch `epoch` of episode `episode`.  The optimizer is
    re-created at every epoch, so there are no moments to keep; synthetic frames are a function of the seed and are not written.
    With --dataset_dir the buffer's part is frame indices, and the rollout's permutation and generator are kept beside it."""
    if not config.get("save_state"):
        return
    device = config["device"]
    part = {"format": 1, "phase": 2, "episode": int(episode), "epoch": int(epoch), "world_size": int(config.get("world_size", 1)),
            "rank": int(config["rank"]), "buffer": replay_buffer.state_dict(include_frames=not config.get("synthetic_frames", True)),
            "aug": augmenter.state_dict() if augmenter is not None else None,
            "rng": {"cpu": torch.get_rng_state(), "device": torch.cuda.get_rng_state(device)}}
    if rollout is not None:
        part["rollout"] = rollout.state_dict()
    if config.get("env") and config["rank"] == 0:
        frames = sum(part["buffer"][k].numel() for k in ("rgb", "birdview") if k in part["buffer"])
        print("train_state: the replay buffer is written with its %d frames, %d bytes" % (part["buffer"]["n"], frames))
    if config["rank"] == 0:
        part["student"] = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    resume._atomic_save(part, _state_path(config))
    if config.get("world_size", 1) > 1:
        dist.barrier()


def load_state_device(config, trainer, replay_buffer, augmenter, rollout=None):
    """-> (episode, epoch) to continue with, (0, 0) when log_dir has no state.  The student comes from rank 0's file on every rank,
    buffer / augmenter / RNG from the rank's own."""
    first = resume._path(config["log_dir"], 0)
    if not config.get("resume") or not first.exists():
        return 0, 0
    device = config["device"]
    state = torch.load(str(first), map_location="cpu")
    if state.get("format") != 1 or state.get("phase") != 2:
        raise ValueError("%s is not a phase-2 training state" % first)
    trainer.student.load_state_dict(state["student"])
    trainer.eng.invalidate()
    mine = state
    if int(state["world_size"]) != int(config.get("world_size", 1)):
        mine = None                      # (the buffers are sharded by rank: another world size means other buffers)
        if config["rank"] == 0:
            print("resume: %s was written under world size %d, this run has %d: the student is restored, replay buffers, augmenter and "
                  "random streams start fresh" % (first.name, state["world_size"], config.get("world_size", 1)))
    elif config["rank"] != 0:
        own = _state_path(config)
        mine = torch.load(str(own), map_location="cpu") if own.exists() else None
        if mine is not None and (mine["episode"], mine["epoch"]) != (state["episode"], state["epoch"]):
            mine = None
        if mine is None:
            print("resume: rank %d has no buffer state of episode %d epoch %d: its buffer starts fresh" % (config["rank"], state["episode"], state["epoch"]))
    if mine is not None:
        if (mine["aug"] is None) != (augmenter is None):
            raise ValueError("the state was saved %s augmentation, this run has %s" % (("without", "with") if mine["aug"] is None else ("with", "without")))
        if (mine.get("rollout") is None) != (rollout is None):
            raise ValueError("the state was saved %s a rollout (--dataset_dir / --env), this run is %s one" % (("without", "with") if rollout is not None else ("with", "without")))
        replay_buffer.load_state_dict(mine["buffer"])
        if rollout is not None:
            rollout.load_state_dict(mine["rollout"])
        if augmenter is not None:
            augmenter.load_state_dict(mine["aug"])
        torch.set_rng_state(mine["rng"]["cpu"])
        torch.cuda.set_rng_state(mine["rng"]["device"], device)
    episode, epoch = int(state["episode"]), int(state["epoch"]) + 1
    if epoch >= config["epoch_per_episode"]:
        episode, epoch = episode + 1, 0
    if config["rank"] == 0:
        print("resuming from %s: episode %d epoch %d finished" % (first, state["episode"], state["epoch"]))
    return episode, epoch


def _epoch_steps(replay_buffer, config):
    """whole batches in the buffer.  With --dataset_dir under several ranks the buffers fill at their own pace (a rank's rollout refreshes
    what ITS buffer holds), and every step is a collective: all ranks take the smallest count."""
    steps = len(replay_buffer) // config["batch_size"]
    if (config.get("dataset_dir") or config.get("env")) and config.get("world_size", 1) > 1:
        least = torch.tensor([steps], dtype=torch.int64, device=config["device"])
        dist.all_reduce(least, op=dist.ReduceOp.MIN)
        steps = int(least)
    return steps


def _train_device(replay_buffer, trainer, config, episode, augmenter=None, start_epoch=0, on_epoch_end=None, rollout=None):
    """_train on a DeviceReplayBuffer: the same epoch, with no .cpu() / .item() / .numpy() in the loop body outside logging iterations"""
    bs = config["batch_size"]
    net = trainer.student
    for epoch in range(start_epoch, config["epoch_per_episode"]):
        _fresh_optimizer(trainer, config, config.get("lr", 1e-4))
        net.train()
        replay_buffer.init_new_weights()
        windows = resume.Windows(config, trainer)
        for i in range(_epoch_steps(replay_buffer, config)):                                   # drop_last=True
            _, loss = _device_step(replay_buffer, trainer, config, augmenter)
            windows.after_step(True)
            if i % int(config["log_iterations"]) == 0:
                bzu.log.scalar(loss_mean=loss.mean().item())
                windows.log(bzu.log.scalar)
                _log_guard(trainer, config)
        windows.end_pass(bzu.log.scalar)
        replay_buffer.normalize_weights()                                                      # (the epoch's one read-back)
        # the reference's eval-mode forward over the highest-weight samples (:229-250), on the trainer's own executor
        top, rgb, bv, command, speed = replay_buffer.get_highest_k(min(32, len(replay_buffer), trainer.batch))
        trainer.eng.forward(rgb, speed, command, False)
        net.train()
        bzu.log.end_epoch()
        save_state_device(config, net, replay_buffer, augmenter, episode, epoch, rollout)
        if on_epoch_end is not None:
            on_epoch_end(episode, epoch, replay_buffer, trainer)
    if episode in SAVE_EPISODES and config["rank"] == 0:
        torch.save(net.state_dict(), str(Path(config["log_dir"]) / ("model-%d.th" % episode)))


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--log_dir", required=True)
    parser.add_argument("--log_iterations", default=100)
    parser.add_argument("--max_episode", default=20)
    parser.add_argument("--epoch_per_episode", default=5)
    parser.add_argument("--ckpt", default=None)
    parser.add_argument("--teacher_path", default=None)
    parser.add_argument("--batch_size", type=int, default=128)
    parser.add_argument("--speed_noise", type=float, default=0.0)
    parser.add_argument("--lr", type=float, default=1e-4)
    parser.add_argument("--synthetic", type=int, default=None, help="frames in the synthetic replay buffer (default 20000)")
    parser.add_argument("--dataset_dir", default=None,
                        help="with --replay device: train on the recorded frames of DIR/train, resident in HBM; every episode scores --rollout_frames of "
                             "them with the current student and admits them into the replay buffer (recorded states, not the student's own)")
    parser.add_argument("--rollout_frames", type=int, default=4000,
                        help="with --dataset_dir: frames scored per episode, over all ranks (0 = the whole dataset; the reference: 4 weathers x 1000)")
    parser.add_argument("--buffer_limit", type=int, default=100000, help="with --dataset_dir: slots of the replay buffer, over all ranks")
    parser.add_argument("--env", default=None, metavar="MODULE:FACTORY",
                        help="with --replay device: on-policy phase 2.  FACTORY(n_envs=, rank=, world=, **env_kwargs) builds the environments (the protocol "
                             "is in training/rollout.py; 'synthetic' = the toy SyntheticEnv); every episode begins with a rollout in which the student "
                             "drives, the teacher labels and --episode_length frames per environment go into a buffer of --buffer_limit slots")
    parser.add_argument("--env_kwargs", default=None, metavar="JSON", help="with --env: keyword arguments of the factory, a JSON object")
    parser.add_argument("--n_envs", type=int, default=1, help="with --env: environments per rank, driven in one batch")
    parser.add_argument("--episode_length", type=int, default=1000, help="with --env: frames recorded per environment and episode")
    parser.add_argument("--beta", type=float, default=0.95, help="with --env: P(student drives) = 0.5 + 0.5 (1 - beta^episode)")
    parser.add_argument("--resident-reserve-gb", type=float, default=None, metavar="GB",
                        help="with --dataset_dir: device memory to leave free for networks and workspaces (default: what batch 256 in fp32 needs)")
    loop.add_precision_argument(parser)
    resume.add_guard_arguments(parser)
    resume.add_clip_arguments(parser)
    resume.add_accumulate_argument(parser)
    resume.add_recipe_arguments(parser, per_epoch=True)
    parser.add_argument("--replay", choices=["host", "device"], default="host",
                        help="host = the replay buffer samples on the host and builds float batches; device = buffer, weighted sampling, uint8 gather "
                             "and weight write-back on the GPU, no host round trip inside a step")
    parser.add_argument("--augment", choices=["None", "medium", "medium_harder", "super_hard", "custom"], default="None",
                        help="colour augmentation of the replayed frames on the GPU (needs --replay device)")
    parser.add_argument("--aug_fix_iter", type=int, default=1000000, help="the fixed image counter the augmentation recipe is taken at")
    parser.add_argument("--batch_aug", type=int, default=1, help="copies of every drawn sample in a step (needs --replay device)")
    parser.add_argument("--save_state", action="store_true", help="with --replay device: write train_state.th after every epoch")
    parser.add_argument("--resume", action="store_true", help="with --replay device: continue from log_dir/train_state.th when there is one")
    parser.add_argument("--seed", type=int, default=None, help="with --replay device: seed torch's generators before the networks are built")
    return parser.parse_args(argv)


def build_config(parsed, rank, world, device):
    """the checks of the flag line (a bad combination exits here, before anything is built), then the config; --seed is applied here"""
    device_replay = parsed.replay == "device"
    if parsed.ema_decay is not None or parsed.ema_eval:
        raise SystemExit("train_image_phase2: --ema-decay is not available in phase 2: the optimizer is re-created every epoch and the state file "
                         "is this script's own, so the average has nowhere to live yet (train phase 1 with it, or average afterwards)")
    recipe = resume.recipe_entries(parsed)
    env_kwargs = {}
    if parsed.env:
        if not device_replay:
            raise SystemExit("train_image_phase2: --env needs --replay device (the tick records its frames on the GPU and commits them to the device "
                             "replay buffer)")
        if parsed.dataset_dir:
            raise SystemExit("train_image_phase2: --env and --dataset_dir exclude each other (on-policy frames or recorded ones)")
        if parsed.synthetic is not None:
            raise SystemExit("train_image_phase2: --env and --synthetic exclude each other (the buffer is filled by the rollout)")
        if parsed.env != "synthetic" and not (parsed.env.count(":") == 1 and all(parsed.env.split(":"))):
            raise SystemExit("train_image_phase2: --env is MODULE:FACTORY or 'synthetic', got %r" % parsed.env)
        try:
            env_kwargs = json.loads(parsed.env_kwargs) if parsed.env_kwargs else {}
        except ValueError as e:
            raise SystemExit("train_image_phase2: --env_kwargs is not JSON: %s" % e)
        if not isinstance(env_kwargs, dict):
            raise SystemExit("train_image_phase2: --env_kwargs must be a JSON object")
        if not 1 <= parsed.n_envs <= 1024 or parsed.episode_length < 1 or parsed.buffer_limit < 1 or not 0.0 <= parsed.beta <= 1.0:
            raise SystemExit("train_image_phase2: --n_envs must lie in 1..1024, --episode_length and --buffer_limit must be positive, --beta in [0, 1]")
    else:
        given = [f for f, on in (("--env_kwargs", parsed.env_kwargs is not None), ("--n_envs", parsed.n_envs != 1),
                                 ("--episode_length", parsed.episode_length != 1000), ("--beta", parsed.beta != 0.95)) if on]
        if given:
            raise SystemExit("train_image_phase2: %s need%s --env" % (", ".join(given), "s" if len(given) == 1 else ""))
    if parsed.dataset_dir:
        if not device_replay:
            raise SystemExit("train_image_phase2: --dataset_dir needs --replay device (the recorded frames stay on the GPU and the buffer holds indices "
                             "into them; the host replay buffer stores frames)")
        if parsed.synthetic is not None:
            raise SystemExit("train_image_phase2: --dataset_dir and --synthetic exclude each other (the buffer is filled from the recorded frames)")
        if parsed.rollout_frames < 0 or parsed.buffer_limit < 1:
            raise SystemExit("train_image_phase2: --rollout_frames must not be negative and --buffer_limit must be positive")
        if parsed.resident_reserve_gb is not None and parsed.resident_reserve_gb < 0:
            raise SystemExit("--resident-reserve-gb must not be negative")
    else:
        given = [f for f, on in (("--rollout_frames", parsed.rollout_frames != 4000), ("--buffer_limit", parsed.buffer_limit != 100000 and not parsed.env),
                                 ("--resident-reserve-gb", parsed.resident_reserve_gb is not None)) if on]
        if given:
            raise SystemExit("train_image_phase2: %s need%s --dataset_dir" % (", ".join(given), "s" if len(given) == 1 else ""))
    if parsed.synthetic is None:
        parsed.synthetic = 20000
    if not device_replay:
        given = [f for f, on in (("--augment", parsed.augment != "None"), ("--batch_aug", parsed.batch_aug != 1), ("--save_state", parsed.save_state),
                                 ("--resume", parsed.resume), ("--seed", parsed.seed is not None)) if on]
        if given:
            raise SystemExit("train_image_phase2: %s need%s --replay device (the host replay buffer has no augmentation, no --batch_aug and no "
                             "resumable state)" % (", ".join(given), "s" if len(given) == 1 else ""))
    if parsed.batch_aug < 1:
        raise SystemExit("train_image_phase2: --batch_aug must be at least 1")
    config = {"log_dir": parsed.log_dir, "log_iterations": parsed.log_iterations, "epoch_per_episode": int(parsed.epoch_per_episode),
              "batch_size": parsed.batch_size, "speed_noise": parsed.speed_noise, "device": device, "rank": rank, "world_size": world,
              "precision": parsed.precision,
              "model_args": {"model": "image_ss", "backbone": BACKBONE},
              "agent_args": {"camera_args": {"w": 384, "h": 160, "fov": 90, "world_y": 1.4, "fixed_offset": 4.0}}}
    config.update(resume.guard_entries(parsed))
    config.update(resume.clip_entries(parsed))
    config.update(resume.accumulate_entries(parsed))
    config.update(recipe)
    if device_replay:
        config.update(replay="device", augment=parsed.augment, aug_fix_iter=parsed.aug_fix_iter, batch_aug=parsed.batch_aug, lr=parsed.lr,
                      synthetic_frames=True)
        if parsed.dataset_dir:
            config.update(dataset_dir=parsed.dataset_dir, rollout_frames=int(parsed.rollout_frames), buffer_limit=int(parsed.buffer_limit),
                          synthetic_frames=False)
            if parsed.resident_reserve_gb is not None:
                config["resident_reserve_gb"] = float(parsed.resident_reserve_gb)
        if parsed.env:
            config.update(env=parsed.env, env_kwargs=env_kwargs, n_envs=int(parsed.n_envs), episode_length=int(parsed.episode_length),
                          beta=float(parsed.beta), buffer_limit=int(parsed.buffer_limit), synthetic_frames=False)
        if parsed.seed is not None:
            torch.manual_seed(parsed.seed)
            config["seed"] = int(parsed.seed)
        if parsed.save_state:
            config["save_state"] = True
        if parsed.resume:
            config["resume"] = True
    return config


def train(config, parsed, on_epoch_end=None):
    rank, world, device = config["rank"], config["world_size"], config["device"]
    bzu.log.init(parsed.log_dir, rank)
    bzu.log.save_config({k: v for k, v in config.items() if k not in ("rank", "world_size", "synthetic_frames")})
    net = ImagePolicyModelSS(BACKBONE, all_branch=True).to(device)
    if parsed.ckpt:
        net.load_state_dict(torch.load(parsed.ckpt, map_location=device))
    teacher = BirdViewPolicyModelSS("resnet18", all_branch=True).to(device)
    net.precision = teacher.precision = parsed.precision
    if parsed.teacher_path:
        teacher.load_state_dict(torch.load(parsed.teacher_path, map_location=device))
    broadcast_module(net)
    broadcast_module(teacher)
    trainer = NativeTrainer(net, teacher, parsed.batch_size * parsed.batch_aug, (3, 160, 384), device, phase=1, lr=parsed.lr, world_size=world,
                            camera=camera_struct(), **resume.trainer_kwargs(config))
    if config.get("replay") == "device":
        rollout = None
        if config.get("dataset_dir"):
            buf, rollout = dataset_buffer(config, trainer, seed=parsed.seed)
        elif config.get("env"):
            buf, rollout = online_rollout(config, trainer, seed=parsed.seed)
        else:
            buf = synthetic_buffer_device(parsed.synthetic // world, device, seed=rank)
        if parsed.seed is not None:                       # (unseeded: the streams of the frames' seed, as the host buffer)
            buf.reseed(parsed.seed * 7919 + rank)
        aug = make_augmenter(config)
        episode0, epoch0 = load_state_device(config, trainer, buf, aug, rollout)
        for episode in range(episode0, int(parsed.max_episode)):
            t0 = time.time()
            start = epoch0 if episode == episode0 else 0
            if rollout is not None and start == 0 and config.get("env"):
                rec = rollout.run(episode)
                bzu.log.scalar(rollout_frames=rec["frames"], rollout_ticks=rec["ticks"], rollout_student_share=rec["student_share"],
                               rollout_collisions=rec["collisions"], rollout_skipped_nonfinite=rec["skipped_nonfinite"], buffer_size=rec["n"])
            elif rollout is not None and start == 0:      # (resumed inside an episode: its rollout ran before the state was written)
                rec = rollout.run()
                bzu.log.scalar(rollout_frames=rec["frames"], rollout_admitted=rec["admitted"], rollout_refreshed=rec["refreshed"],
                               rollout_evicted=rec["evicted"], buffer_size=rec["n"])
            _train_device(buf, trainer, config, episode, aug, start, on_epoch_end, rollout)
            if rank == 0:
                print("episode %d: %.1f s" % (episode, time.time() - t0))
        return {"net": net, "buffer": buf, "trainer": trainer, "rollout": rollout}
    buf = synthetic_buffer(parsed.synthetic // world, device, seed=rank)
    for episode in range(int(parsed.max_episode)):
        t0 = time.time()
        _train(buf, trainer, config, episode)
        if rank == 0:
            print("episode %d: %.1f s" % (episode, time.time() - t0))


def main(argv=None, on_epoch_end=None):
    """on_epoch_end(episode, epoch, replay_buffer, trainer), --replay device only: called after every epoch's state is written -- the
    place of the reference's per-epoch evaluation / visualisation of the highest-weight samples (train_image_phase2.py:229-250)"""
    parsed = parse_arguments(argv)
    return loop.launch(parsed, build_config, lambda config: train(config, parsed, on_epoch_end))


if __name__ == "__main__":
    main()
