"""The learner half of phase 2's `rollout` (reference training/train_image_phase2.py:61-149) over RECORDED frames.

The reference drives CARLA with the student, and for every frame the agent saw it runs student and teacher in eval mode, scores their
disagreement with _get_weight and hands the frame to ReplayBuffer.add_data, which keeps the buffer_limit highest weights.  None of
that needs a simulator once the frames exist: OfflineRollout takes a window of a resident dataset (ResidentLoader), runs both networks
on it without a backward (NativeTrainer.step(update=False, train_mode=False)), scores with lbc_phase2_weight and admits the window into
a DeviceReplayBuffer(source=store) that holds frame indices.  The states are the recorded ones, NOT the student's own: this is
loss-prioritised replay over a dataset (DAgger's learner on a fixed state distribution), not on-policy data.

Everything a window needs is enqueued chunk by chunk -- nothing is read back inside the loop; the one read-back is the admit record."""
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
