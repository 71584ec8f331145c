"""SyntheticEnv: a deterministic TOY environment for OnlineRollout (training/rollout.py has the protocol).  There is no simulator behind
it and nothing about it resembles driving: it exists so that the tests and the benchmark can run the on-policy loop of phase 2 -- tick,
decide, record, end an episode on a collision, resume -- without CARLA.  A real run supplies its own environment (--env MODULE:FACTORY).

What it does have is the one property the loop depends on: the observations depend on the controls.  The frame an environment shows is
picked from a fixed pool (SyntheticFrames) by a hash of (environment, the environment's tick count, the sign and the quantised size of
the last applied steer), and so are its speed and command.  Episodes end where a script says so."""
import numpy as np
import torch

from ..bird_view.utils.datasets.synthetic import SyntheticFrames

_M32 = 0xFFFFFFFF


def _mix(x):
    """the "lowbias32" finaliser (csrc/lbc_hash.hpp hash_u32) on Python integers"""
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & _M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & _M32
    x ^= x >> 16
    return x


def steer_key(steer):
    """sign and quantised size of a steer: 0 for 0 / NaN, else +-(1 + floor(4 min(|steer|, 1)))"""
    steer = float(steer)
    if steer != steer or steer == 0.0:
        return 0
    q = 1 + int(4.0 * min(abs(steer), 1.0))
    return q if steer > 0 else -q


class SyntheticEnv:
    """n_envs toy environments (global indices rank, rank + world, ... so that ranks see different ones).

    script: {environment (global index): {tick: "done" | "collided"}}: the flag observe() shows once the environment has been applied
    `tick` controls in total (ticks count from construction and go on counting across episodes); an episode without a scripted end is
    `done` after episode_ticks ticks.  pool frames of rgb_hw / map_size are drawn once from `seed`."""

    def __init__(self, n_envs=1, pool=16, seed=0, rank=0, world=1, script=None, episode_ticks=1 << 30, rgb_hw=(160, 384), map_size=320):
        self.n_envs, self.pool, self.seed = int(n_envs), int(pool), int(seed) & _M32
        self.ids = [int(rank) + int(world) * i for i in range(self.n_envs)]
        self.script = {int(k): {int(t): str(v) for t, v in ev.items()} for k, ev in (script or {}).items()}
        for ev in self.script.values():
            for v in ev.values():
                if v not in ("done", "collided"):
                    raise ValueError("SyntheticEnv: a scripted event is 'done' or 'collided', got %r" % (v,))
        self.episode_ticks = int(episode_ticks)
        frames = SyntheticFrames(self.pool, "cpu", seed=self.seed, rgb_hw=rgb_hw, birdview_hw=(int(map_size), int(map_size)))
        self.rgb, self.birdview = frames.rgb.numpy(), frames.birdview.numpy()
        self.ticks = np.zeros(self.n_envs, dtype=np.int64)            # controls applied since construction
        self.episode_tick = np.zeros(self.n_envs, dtype=np.int64)     # ... since the last reset
        self.episodes = np.zeros(self.n_envs, dtype=np.int64)
        self.key = np.zeros(self.n_envs, dtype=np.int64)              # steer_key of the last applied control
        self.done = np.zeros(self.n_envs, dtype=bool)
        self.collided = np.zeros(self.n_envs, dtype=bool)

    def reset(self, indices):
        for i in indices:
            self.episode_tick[i], self.key[i], self.done[i], self.collided[i] = 0, 0, False, False
            self.episodes[i] += 1

    def _draw(self, i):
        return _mix(self.seed ^ _mix((self.ids[i] * 0x9E3779B9 + _mix(int(self.ticks[i]) * 16 + int(self.key[i]) + 8)) & _M32))

    def observe(self):
        h = [self._draw(i) for i in range(self.n_envs)]
        pick = np.array([v % self.pool for v in h])
        return {"rgb": self.rgb[pick], "birdview": self.birdview[pick], "speed": np.array([((v >> 8) % 1000) / 100.0 for v in h]),
                "command": np.array([1 + ((v >> 20) & 3) for v in h], dtype=np.int64), "done": self.done.copy(), "collided": self.collided.copy()}

    def apply(self, controls):
        controls = np.asarray(controls, dtype=np.float64)
        for i in range(self.n_envs):
            self.key[i] = steer_key(controls[i, 0])
            self.ticks[i] += 1
            self.episode_tick[i] += 1
            event = self.script.get(self.ids[i], {}).get(int(self.ticks[i]))
            self.collided[i] = self.collided[i] or event == "collided"
            self.done[i] = self.done[i] or event == "done" or self.episode_tick[i] >= self.episode_ticks

    def close(self):
        pass

    def state_dict(self):
        return {"format": 1, "ids": list(self.ids), "pool": self.pool, "seed": self.seed,
                **{k: torch.from_numpy(getattr(self, k).copy()) for k in ("ticks", "episode_tick", "episodes", "key", "done", "collided")}}

    def load_state_dict(self, sd):
        if sd.get("format") != 1 or list(sd["ids"]) != self.ids or int(sd["pool"]) != self.pool or int(sd["seed"]) != self.seed:
            raise ValueError("SyntheticEnv.load_state_dict: the state is of environments %r (pool %r, seed %r), this object of %r (pool %d, seed %d)"
                             % (sd.get("ids"), sd.get("pool"), sd.get("seed"), self.ids, self.pool, self.seed))
        for k in ("ticks", "episode_tick", "episodes", "key", "done", "collided"):
            getattr(self, k)[:] = sd[k].numpy()
