"""The learner half of phase 2's `rollout` (reference training/train_image_phase2.py:61-149) over RECORDED frames.

The reference drives CARLA with the student, and for every frame the agent saw it runs student and teacher in eval mode, scores their
disagreement with _get_weight and hands the frame to ReplayBuffer.add_data, which keeps the buffer_limit highest weights.  None of
that needs a simulator once the frames exist: OfflineRollout takes a window of a resident dataset (ResidentLoader), runs both networks
on it without a backward (NativeTrainer.step(update=False, train_mode=False)), scores with lbc_phase2_weight and admits the window into
a DeviceReplayBuffer(source=store) that holds frame indices.  The states are the recorded ones, NOT the student's own: this is
loss-prioritised replay over a dataset (DAgger's learner on a fixed state distribution), not on-policy data.

Everything a window needs is enqueued chunk by chunk -- nothing is read back inside the loop; the one read-back is the admit record.

OnlineRollout (below) is the DRIVING half of the same function: the student's own states, from an environment the user supplies
(ENV_PROTOCOL; SingleEnvAdapter wraps reference-style environments), ticked by teaching.TeachingSession and committed into a copying
DeviceReplayBuffer."""
import numpy as np
import torch

from ..bird_view.augmenter import rng_state_from_dict, rng_state_to_dict
from ..bird_view.utils.train_utils import one_hot


def shard_frames(frames, rank=0, world=1):
    """the frames rank `rank` of `world` owns: f = rank (mod world), ascending"""
    if not 0 <= int(rank) < int(world):
        raise ValueError("shard_frames: rank %r outside [0, %r)" % (rank, world))
    return np.arange(int(rank), int(frames), int(world), dtype=np.int64)


class OfflineRollout:
    """frames_per_episode: frames scored per run() (0 = the rank's whole shard; more than the shard holds = the shard; where the shards
    of several ranks differ by a frame, the smaller size, so that every rank scores as many chunks).  The owned
    frames are visited in a seeded permutation, consumed window by window; when fewer than a window are left a fresh permutation is
    drawn and the window starts there, so a window never holds a frame twice."""

    def __init__(self, store, trainer, buffer, frames_per_episode=4000, seed=0, rank=0, world=1):
        from .train_image_phase2 import phase2_weights
        if getattr(buffer, "source", None) is not store:
            raise ValueError("OfflineRollout: the buffer must be a DeviceReplayBuffer(source=store) over the same store")
        self.store, self.trainer, self.buffer = store, trainer, buffer
        self.owned = shard_frames(store.frames, rank, world)
        if len(self.owned) < 1:
            raise ValueError("OfflineRollout: rank %d of %d owns none of the %d frames" % (rank, world, store.frames))
        m = int(frames_per_episode)
        if m < 0:
            raise ValueError("OfflineRollout: frames_per_episode must not be negative")
        whole = int(store.frames) // int(world)              # (the same on every rank: shards differ by one frame at most)
        if whole < 1:
            raise ValueError("OfflineRollout: %d frames are fewer than one per rank of %d" % (store.frames, world))
        self.window = whole if m == 0 else min(m, whole)
        self.rank, self.world = int(rank), int(world)
        self.rng = np.random.RandomState((int(seed) * 7919 + int(rank)) & 0xFFFFFFFF)
        self.perm, self.pos = None, 0
        self._weights = phase2_weights

    def next_window(self):
        """-> the next `window` frame indices (host int64), all distinct"""
        if self.perm is None or self.pos + self.window > len(self.perm):
            self.perm, self.pos = self.owned[self.rng.permutation(len(self.owned))], 0
        out = self.perm[self.pos:self.pos + self.window]
        self.pos += self.window
        return out

    def score(self, frames):
        """-> (cmd i32, speed f32, weight f32) device tensors (len(frames),): both networks in eval mode over chunks of trainer.batch
        frames (a short last chunk runs as it is), no augmentation and no speed noise (the reference scores what the agent saw), nothing
        read back"""
        tr, store, dev = self.trainer, self.store, self.store.device
        m, bs = len(frames), int(tr.batch)
        cmd_host = store.cmd_host[torch.from_numpy(np.asarray(frames, dtype=np.int64))]
        cmd = cmd_host.to(torch.int32).to(dev)
        speed = torch.empty(m, dtype=torch.float32, device=dev)
        weight = torch.empty(m, dtype=torch.float32, device=dev)
        for c0 in range(0, m, bs):
            chunk = frames[c0:c0 + bs]
            rgb, bv, _, sp = store.gather(chunk)
            tr.step(rgb, sp, one_hot(cmd_host[c0:c0 + bs]).to(dev), birdview=bv, update=False, train_mode=False)
            speed[c0:c0 + len(chunk)].copy_(sp)
            weight[c0:c0 + len(chunk)].copy_(self._weights(tr, tr.last_pred[0], tr.last_teacher[0]))
        return cmd, speed, weight

    def run(self):
        """one episode's rollout -> the admit record {"n", "refreshed", "admitted", "evicted"} plus "frames", the window's size"""
        frames = self.next_window()
        cmd, speed, weight = self.score(frames)
        rec = self.buffer.admit(frames, cmd, speed, weight)
        rec["frames"] = int(len(frames))
        return rec

    def state_dict(self):
        return {"format": 1, "frames": int(self.store.frames), "rank": self.rank, "world": self.world, "window": int(self.window),
                "perm": None if self.perm is None else torch.from_numpy(np.asarray(self.perm, dtype=np.int64).copy()), "pos": int(self.pos),
                "rng": rng_state_to_dict(self.rng)}

    def load_state_dict(self, sd):
        if sd.get("format") != 1:
            raise ValueError("OfflineRollout.load_state_dict: unknown state format %r" % (sd.get("format"),))
        mine = (int(self.store.frames), self.rank, self.world, int(self.window))
        theirs = (int(sd["frames"]), int(sd["rank"]), int(sd["world"]), int(sd["window"]))
        if mine != theirs:
            raise ValueError("OfflineRollout.load_state_dict: the state is of (frames, rank, world, window) = %r, this rollout of %r" % (theirs, mine))
        self.perm = None if sd["perm"] is None else sd["perm"].cpu().numpy().astype(np.int64)
        self.pos = int(sd["pos"])
        rng_state_from_dict(self.rng, sd["rng"])


# ---- on-policy: the student drives ----------------------------------------------------------------------------------------------
ENV_PROTOCOL = """The environment protocol of OnlineRollout (a simulator stays outside this repository; the user supplies the object):
  n_envs                 how many environments the object steps at once
  reset(indices)         start a new episode in the listed environments
  observe()              -> {"rgb" (N,160,384,3) u8, "birdview" (N,320,320,7) u8, "speed" (N,), "command" (N,) in 1..4, "done" (N,) bool,
                         "collided" (N,) bool}; done / collided describe the episode AFTER the last apply (the reference's loop condition
                         `not env.is_success() and not env.collided`, train_image_phase2.py:111); calling it again before the next
                         apply / reset returns the same observation
  apply(controls)        (N,3) float64 steer / throttle / brake, one tick of every environment (an all-zero row for an environment that
                         has collected its frames)
  close()
  state_dict() / load_state_dict()   optional: an environment without them is restarted on --resume"""


class SingleEnvAdapter:
    """n reference-style environments (tick, get_observations, apply_control, is_success, collided; train_image_phase2.py:111-123) as one
    object of the protocol above.  make_env(index) -> a fresh environment, called again on every reset(index) after the previous one was
    closed (the reference opens a new suite per episode, :92); make_control(steer, throttle, brake) -> what apply_control takes (default:
    agent.Agent.postprocess's clipped VehicleControl)."""

    def __init__(self, make_env, n, make_control=None):
        self.make_env, self.n_envs = make_env, int(n)
        self.envs = [None] * self.n_envs
        self._obs = [None] * self.n_envs
        self._control = make_control or _clipped_control

    def reset(self, indices):
        for i in indices:
            self._close(i)
            self.envs[i] = self.make_env(int(i))
            self._obs[i] = None

    def observe(self):
        for i, env in enumerate(self.envs):
            if self._obs[i] is None:
                env.tick()
                o = env.get_observations()
                self._obs[i] = {"rgb": np.ascontiguousarray(o["rgb"]), "birdview": np.ascontiguousarray(o["birdview"]),
                                "speed": float(np.linalg.norm(o["velocity"])), "command": int(o["command"])}
        stack = lambda k, dt: np.stack([np.asarray(o[k], dtype=dt) for o in self._obs])
        return {"rgb": stack("rgb", np.uint8), "birdview": stack("birdview", np.uint8), "speed": stack("speed", np.float64),
                "command": stack("command", np.int64), "done": np.array([bool(e.is_success()) for e in self.envs]),
                "collided": np.array([bool(e.collided) for e in self.envs])}

    def apply(self, controls):
        for i, env in enumerate(self.envs):
            env.apply_control(self._control(*[float(v) for v in controls[i]]))
            self._obs[i] = None

    def _close(self, i):
        env, self.envs[i] = self.envs[i], None
        if env is not None and hasattr(env, "close"):
            env.close()

    def close(self):
        for i in range(self.n_envs):
            self._close(i)


def _clipped_control(steer, throttle, brake):
    from ..agent import _vehicle_control
    control = _vehicle_control()
    control.steer, control.throttle, control.brake = float(np.clip(steer, -1.0, 1.0)), float(np.clip(throttle, 0.0, 1.0)), float(np.clip(brake, 0.0, 1.0))
    control.manual_gear_shift = False
    return control


class OnlineRollout:
    """The driving half of phase 2's `rollout` (reference train_image_phase2.py:86-149) for n_envs environments at once: session is a
    teaching.TeachingSession of n_envs agents and at least episode_length staging rows per agent, buffer a copying DeviceReplayBuffer,
    env an object of the protocol above.

    run(episode): every environment starts a fresh episode; the session ticks until every environment has staged episode_length frames
    (an environment that has them sits out: its row of the mask is 0, so nothing is ever dropped); on done / collided an environment's
    episode ends -- both controllers are reset, a collision takes the last five staged frames off that environment's list -- and a new one
    starts; then the staged frames are committed.  -> the commit record {"frames", "skipped_nonfinite", "dropped", "n"} plus "ticks"
    (session ticks), "student_share" (the share of recorded-or-not active agent ticks the student drove) and "collisions"."""

    def __init__(self, session, buffer, env, episode_length, beta=0.95):
        self.session, self.buffer, self.env = session, buffer, env
        self.episode_length, self.beta = int(episode_length), float(beta)
        if int(env.n_envs) != session.n_agents:
            raise ValueError("OnlineRollout: the environment steps %d environments, the session %d agents" % (env.n_envs, session.n_agents))
        if not 1 <= self.episode_length <= session.capacity:
            raise ValueError("OnlineRollout: episode_length = %d outside [1, the session's capacity of %d]" % (self.episode_length, session.capacity))

    def run(self, episode):
        s, env, n, L = self.session, self.env, self.session.n_agents, self.episode_length
        s.set_episode(episode, self.beta)
        s.reset()
        env.reset(list(range(n)))
        staged = np.zeros(n, dtype=np.int64)
        finished = np.zeros(n, dtype=bool)
        ticks = collisions = drove = student = 0
        while True:
            obs = env.observe()
            done, hit = np.asarray(obs["done"], dtype=bool), np.asarray(obs["collided"], dtype=bool)
            ended = [i for i in range(n) if not finished[i] and (done[i] or hit[i])]
            if ended:
                s.end_episode(ended, [bool(hit[i]) for i in ended])
                for i in ended:
                    if hit[i]:
                        collisions += 1
                        staged[i] = max(staged[i] - 5, 0)
            finished |= staged >= L
            again = [i for i in ended if not finished[i]]
            if again:
                env.reset(again)
                obs = env.observe()
            if finished.all():
                break
            active = ~finished
            controls = s.run_step(obs["rgb"], obs["birdview"], obs["speed"], obs["command"], active=active)
            env.apply(controls)
            ticks += 1
            staged = np.where(active, s.debug["staged"], staged)
            drove += int(active.sum())
            student += int(s.debug["who"][active].sum())
        rec = s.commit(self.buffer)
        rec.update(ticks=int(ticks), student_share=float(student) / max(drove, 1), collisions=int(collisions))
        return rec

    def state_dict(self):
        """the session's part and, where the environment has a state_dict, the environment's (staging is empty between rollouts)"""
        env = self.env.state_dict() if hasattr(self.env, "state_dict") else None
        return {"format": "online-1", "episode_length": self.episode_length, "session": self.session.state_dict(), "env": env}

    def load_state_dict(self, sd):
        if sd.get("format") != "online-1":
            raise ValueError("OnlineRollout.load_state_dict: the state is not an on-policy rollout's (format %r): it was written by a run with "
                             "--dataset_dir" % (sd.get("format"),))
        self.session.load_state_dict(sd["session"])
        if sd.get("env") is not None and hasattr(self.env, "load_state_dict"):
            self.env.load_state_dict(sd["env"])
        else:
            print("resume: the environment has no state to restore (no state_dict / load_state_dict): it is restarted")
