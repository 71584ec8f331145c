"""Device-resident prioritised replay buffer of phase 2 (reference training/phase2_utils.py:190-289 ReplayBuffer).

DeviceReplayBuffer keeps phase2_utils.ReplayBuffer's interface (add_batch / add_data / init_new_weights / sample_indices / batch /
update_weights / normalize_weights / get_highest_k) with everything a training step touches on the device: `buffer_limit` slots are
allocated once (rgb u8 (limit,160,384,3), birdview u8 (limit,192,192,7), cmd i32, speed f32, weights f32, new_weights f32, cdf f64);
the weighted draw, the gather of the drawn frames with the --batch_aug fan-out, and the write-back of the new weights are the
lbc_replay_* kernels (csrc/replay.hip), none of which copies to the host.  Frames are held as the dataset stores them, 0..255 (the
bird view as 0/255 masks): the same contract as SyntheticFrames and the LMDB DeviceLoader, a batch goes straight into
NativeTrainer.step / lbc_net_forward_u8.  The one host read-back is normalize_weights(), once per epoch: (total weight, number of
unusable weights).

DeviceReplayBuffer(..., source=store) is the buffer over a recorded dataset: `store` is a ResidentLoader that already keeps every camera
frame and the fixed bird-view window in HBM, and the buffer holds frame INDICES into it -- frame i32 (limit,) and slot_of_frame i32
(F,) -- and no frame storage of its own.  admit(frames, cmd, speed, weight) decides who stays in one lbc_replay_admit launch and reads
back its 16-byte record (the one sync outside normalize_weights); batch / get_highest_k gather through the slot's frame index
(lbc_replay_gather_indirect_u8) straight out of the store.  Everything else -- draws, write-back, prefix sums -- is the same code."""
import logging

import numpy as np
import torch

from .. import _lib
from ..bird_view.augmenter import rng_state_from_dict, rng_state_to_dict

RGB_SHAPE = (160, 384, 3)
BIRDVIEW_SHAPE = (192, 192, 7)
WRITEBACK_MAX = 1024          # lbc_replay_writeback resolves duplicate indices inside one workgroup


class DeviceReplayBuffer:
    def __init__(self, device, buffer_limit=100000, sampling=True, seed=0, rgb_shape=RGB_SHAPE, birdview_shape=BIRDVIEW_SHAPE, source=None):
        self.device = torch.device(device)
        self.buffer_limit = int(buffer_limit)
        self._sampling = sampling
        self.normalized = False
        self.n = 0
        lim = self.buffer_limit
        self.source = source
        if source is not None:
            self._check_source(source)
            rgb_shape, birdview_shape = tuple(source.rgb.shape[1:]), tuple(source.birdview.shape[1:])
        for name, shape in (("rgb", rgb_shape), ("birdview", birdview_shape)):
            if int(np.prod(shape)) % 16:
                raise ValueError("DeviceReplayBuffer: a %s frame of shape %s is %d bytes, rows move as 16-byte words" % (name, tuple(shape), int(np.prod(shape))))
        if source is not None:
            # the store's frames ARE the buffer's; a slot holds the index of its frame, slot_of_frame the slot of a stored frame (-1: none)
            self.rgb, self.birdview = source.rgb, source.birdview
            self.frame = torch.full((lim,), -1, dtype=torch.int32, device=self.device)
            self.slot_of_frame = torch.full((int(source.frames),), -1, dtype=torch.int32, device=self.device)
            self._record = torch.zeros(4, dtype=torch.int32, device=self.device)
            self._admit_ws = None
        else:
            self.rgb = torch.empty((lim,) + tuple(rgb_shape), dtype=torch.uint8, device=self.device)
            self.birdview = torch.empty((lim,) + tuple(birdview_shape), dtype=torch.uint8, device=self.device)
        self.cmd = torch.zeros(lim, dtype=torch.int32, device=self.device)
        self.speed = torch.zeros(lim, dtype=torch.float32, device=self.device)
        self.weights = torch.zeros(lim, dtype=torch.float32, device=self.device)
        self.new_weights = torch.zeros(lim, dtype=torch.float32, device=self.device)
        self.cdf = torch.zeros(lim, dtype=torch.float64, device=self.device)
        self._bad = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.seed = int(seed) & 0xFFFFFFFF
        self.draws = 0                                   # batches drawn by the kernel so far: the counter of its stream
        self._rng = np.random.RandomState(seed)          # the epoch shuffle while the weights are not normalised yet
        self._perm, self._perm_dev, self._perm_pos = None, None, 0
        _lib.require_device(self.rgb)

    def __len__(self):
        return self.n

    def _check_source(self, source):
        if getattr(source, "teacher_rows", None) is not None or getattr(source, "birdview", None) is None:
            raise ValueError("DeviceReplayBuffer: the source has a teacher cache in place of its bird-view frames (--cache-teacher); phase 2 runs "
                             "the teacher on the frames it replays, build the ResidentLoader without teacher=")
        if getattr(source, "whole_map", False) or getattr(source, "jitter", False):
            raise ValueError("DeviceReplayBuffer: the source's bird-view window is jittered (it keeps the whole 320 x 320 map and cuts the window per "
                             "draw); the buffer replays the fixed window, build the ResidentLoader over an ImageDataset")
        if getattr(source, "rgb", None) is None:
            raise ValueError("DeviceReplayBuffer: the source holds no camera frames")
        if torch.device(source.device).type != self.device.type:
            raise ValueError("DeviceReplayBuffer: the source lives on %s, the buffer on %s" % (source.device, self.device))
        if int(source.frames) < 1:
            raise ValueError("DeviceReplayBuffer: the source holds no frames")

    def reseed(self, seed):
        """new index streams (the epoch shuffle's generator and the kernel sampler's seed, counter back to 0); the frames stay"""
        self.seed, self.draws = int(seed) & 0xFFFFFFFF, 0
        self._rng = np.random.RandomState(int(seed) & 0xFFFFFFFF)
        self._set_perm(None, 0)

    # ---- kernels -----------------------------------------------------------------------------------------------
    def _stream(self):
        return _lib.stream_for(self.rgb)

    def _index(self, idx):
        """-> contiguous int32 tensor on the buffer's device (what sample_indices hands out passes through)"""
        if not torch.is_tensor(idx):
            idx = torch.as_tensor(np.asarray(idx))
        return idx.to(device=self.device, dtype=torch.int32).contiguous()

    def _scatter(self, dst, src, slots):
        src = src.contiguous()
        row = int(dst[0].numel())
        _lib.check(_lib.get().lbc_replay_scatter_u8(_lib.ptr(src), row, _lib.ptr(slots), int(slots.numel()), _lib.ptr(dst), self._stream()),
                   "replay_scatter_u8")

    # ---- filling -----------------------------------------------------------------------------------------------
    def add_batch(self, rgb_u8, birdview_u8, cmd, speed, weight):
        """rgb_u8 (m,160,384,3), birdview_u8 (m,192,192,7) as 0/255, cmd (m,), speed (m,), weight (m,).  While there is room the frames
        are appended; beyond it the `buffer_limit` highest weights of old + new stay (reference phase2_utils.py:257-261), and the new
        frames among them take the slots of the evicted ones."""
        if self.source is not None:
            raise RuntimeError("DeviceReplayBuffer.add_batch: this buffer holds frame indices into its source, not frames; use admit(frames, ...)")
        self.normalized = False
        dev = self.device
        rgb_u8, birdview_u8 = rgb_u8.to(dev), birdview_u8.to(dev)
        if rgb_u8.dtype != torch.uint8 or birdview_u8.dtype != torch.uint8:
            raise ValueError("DeviceReplayBuffer.add_batch: frames must be uint8 (the dataset's 0..255 storage)")
        m = int(rgb_u8.shape[0])
        if tuple(rgb_u8.shape[1:]) != tuple(self.rgb.shape[1:]) or tuple(birdview_u8.shape) != (m,) + tuple(self.birdview.shape[1:]):
            raise ValueError("DeviceReplayBuffer.add_batch: frames of shape %s / %s, the buffer holds %s / %s"
                             % (tuple(rgb_u8.shape[1:]), tuple(birdview_u8.shape[1:]), tuple(self.rgb.shape[1:]), tuple(self.birdview.shape[1:])))
        cmd = torch.as_tensor(cmd).to(dev).to(torch.int32)
        speed = torch.as_tensor(speed).to(dev).float()
        weight = torch.as_tensor(np.asarray(weight, dtype=np.float32) if not torch.is_tensor(weight) else weight).to(dev).float()
        k = min(self.buffer_limit - self.n, m)                       # appended
        slots = torch.arange(self.n, self.n + k, dtype=torch.int32, device=dev)
        take = torch.arange(0, k, dtype=torch.int64, device=dev)     # rows of the new batch that go into `slots`
        if m > k:                                                    # the rest competes with what is stored
            lim = self.buffer_limit
            stored = torch.cat([self.weights[:self.n], weight[:k]])  # (= lim entries: the buffer is full after the append)
            keep = torch.zeros(lim + m - k, dtype=torch.bool, device=dev)
            keep[torch.topk(torch.cat([stored, weight[k:]]), lim).indices] = True
            evicted = torch.nonzero(~keep[:lim]).reshape(-1)
            survivors = torch.nonzero(keep[lim:]).reshape(-1) + k
            # an appended frame that is evicted by the same call: its slot is written once, by the survivor
            gone = evicted >= self.n
            if bool(gone.any()):
                alive = torch.ones(k, dtype=torch.bool, device=dev)
                alive[evicted[gone] - self.n] = False
                slots, take = slots[alive], take[alive]
            slots = torch.cat([slots, evicted.to(torch.int32)])
            take = torch.cat([take, survivors])
        if slots.numel():
            whole = take.numel() == m and k == m
            self._scatter(self.rgb, rgb_u8 if whole else rgb_u8[take], slots)
            self._scatter(self.birdview, birdview_u8 if whole else birdview_u8[take], slots)
            sl = slots.long()
            self.cmd[sl], self.speed[sl], self.weights[sl] = cmd[take], speed[take], weight[take]
        self.n += k

    def add_data(self, rgb_img, cmd, speed, target, birdview_img, weight):
        """the reference's per-sample form (phase2_utils.py:256); birdview_img as 0/255"""
        self.add_batch(torch.as_tensor(rgb_img)[None], torch.as_tensor(birdview_img)[None], torch.tensor([cmd]), torch.tensor([speed]), [weight])

    def admit(self, frames, cmd, speed, weight):
        """frames: m distinct indices into the source (host integers or a tensor); cmd (m,), speed (m,), weight (m,) device tensors.
        One lbc_replay_admit launch -- a stored frame takes the new weight, the others fill the free slots, and once the buffer is full
        the `buffer_limit` highest weights of stored + new stay (include/lbc_hip.h has the rule for ties) -- and one read-back of its
        record -> {"n", "refreshed", "admitted", "evicted"}."""
        if self.source is None:
            raise RuntimeError("DeviceReplayBuffer.admit: this buffer stores frames (no source=); use add_batch")
        host = frames.detach().cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
        if host.ndim != 1 or host.shape[0] < 1 or not np.issubdtype(host.dtype, np.integer):
            raise ValueError("DeviceReplayBuffer.admit: frames must be a vector of at least one integer index")
        m, F = int(host.shape[0]), int(self.slot_of_frame.numel())
        if int(host.min()) < 0 or int(host.max()) >= F:
            raise ValueError("DeviceReplayBuffer.admit: frame index %d outside the source's %d frames" % (int(host.min() if host.min() < 0 else host.max()), F))
        if np.unique(host).shape[0] != m:
            raise ValueError("DeviceReplayBuffer.admit: %d of the %d frame indices are repeats; a frame is admitted once per call" % (m - np.unique(host).shape[0], m))
        dev, lib = self.device, _lib.get()
        cf = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(dev)
        cc = torch.as_tensor(cmd).to(dev).to(torch.int32).contiguous()
        cs = torch.as_tensor(speed).to(dev).float().contiguous()
        cw = torch.as_tensor(weight).detach().to(dev).float().contiguous()
        if not (cc.numel() == cs.numel() == cw.numel() == m):
            raise ValueError("DeviceReplayBuffer.admit: %d frames with %d commands, %d speeds, %d weights" % (m, cc.numel(), cs.numel(), cw.numel()))
        need = int(lib.lbc_replay_admit_workspace(self.buffer_limit, m))
        if need == 0:
            raise ValueError("DeviceReplayBuffer.admit: %d slots / %d candidates are more than lbc_replay_admit takes (2^20 each)" % (self.buffer_limit, m))
        if self._admit_ws is None or self._admit_ws.numel() < need:
            self._admit_ws = torch.empty(need, dtype=torch.uint8, device=dev)
        self.normalized = False
        _lib.check(lib.lbc_replay_admit(_lib.ptr(self.weights), _lib.ptr(self.frame), _lib.ptr(self.cmd), _lib.ptr(self.speed), _lib.ptr(self.slot_of_frame),
                                        F, self.n, self.buffer_limit, _lib.ptr(cw), _lib.ptr(cf), _lib.ptr(cc), _lib.ptr(cs), m, _lib.ptr(self._admit_ws), need,
                                        _lib.ptr(self._record), self._stream()), "replay_admit")
        rec = [int(v) for v in self._record.cpu()]                    # (the read-back also keeps cf / cc / cs / cw alive until the kernel has run)
        self.n = rec[0]
        self._perm = None
        return {"n": rec[0], "refreshed": rec[1], "admitted": rec[2], "evicted": rec[3]}

    # ---- one epoch ---------------------------------------------------------------------------------------------
    def init_new_weights(self):
        """start of an epoch (reference train_image_phase2.py:168): fresh write-back array, fresh shuffle"""
        self.new_weights[:self.n].copy_(self.weights[:self.n])
        self._perm = None

    def sample_indices(self, batch_size):
        """-> int32 device tensor (batch_size,).  Once the weights are normalised: loss-weighted draws with replacement by
        lbc_replay_sample, batch t of this buffer = counter t of the stream `seed`.  Before that: consecutive slices of one host-drawn
        permutation per epoch, uploaded once (DataLoader(shuffle=True, drop_last=True), reference train_image_phase2.py:170): every
        sample is visited exactly once."""
        if self._sampling and self.normalized:
            idx = torch.empty(batch_size, dtype=torch.int32, device=self.device)
            _lib.check(_lib.get().lbc_replay_sample(_lib.ptr(self.cdf), self.n, self.seed, self.draws, batch_size, _lib.ptr(idx), self._stream()),
                       "replay_sample")
            self.draws += 1
            return idx
        if self._perm is None or self._perm_pos + batch_size > len(self._perm) or len(self._perm) != self.n:
            self._set_perm(self._rng.permutation(self.n), 0)             # a new epoch (or the buffer changed)
        out = self._perm_dev[self._perm_pos:self._perm_pos + batch_size]
        self._perm_pos += batch_size
        return out

    def _set_perm(self, perm, pos):
        self._perm, self._perm_pos = perm, int(pos)
        self._perm_dev = None if perm is None else torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int32)).to(self.device)

    def batch(self, idx, reps=1):
        """-> (rgb u8 (B*reps,160,384,3), birdview u8 (B*reps,192,192,7), command one-hot (B*reps,4), speed (B*reps,)), each source
        sample `reps` times in a row (--batch_aug): what NativeTrainer.step takes"""
        idx = self._index(idx)
        b, reps, lib, s = int(idx.numel()), int(reps), _lib.get(), self._stream()
        rows = b * reps
        rgb = torch.empty((rows,) + tuple(self.rgb.shape[1:]), dtype=torch.uint8, device=self.device)
        bv = torch.empty((rows,) + tuple(self.birdview.shape[1:]), dtype=torch.uint8, device=self.device)
        onehot = torch.empty((rows, 4), dtype=torch.float32, device=self.device)
        speed = torch.empty(rows, dtype=torch.float32, device=self.device)
        if self.source is not None:                                   # slot -> frame -> the store's row
            for src, dst in ((self.rgb, rgb), (self.birdview, bv)):
                _lib.check(lib.lbc_replay_gather_indirect_u8(_lib.ptr(src), int(src[0].numel()), _lib.ptr(self.frame), _lib.ptr(idx), b, reps, _lib.ptr(dst), s),
                           "replay_gather_indirect_u8")
        else:
            _lib.check(lib.lbc_replay_gather_u8(_lib.ptr(self.rgb), int(self.rgb[0].numel()), _lib.ptr(idx), b, reps, _lib.ptr(rgb), s), "replay_gather_u8")
            _lib.check(lib.lbc_replay_gather_u8(_lib.ptr(self.birdview), int(self.birdview[0].numel()), _lib.ptr(idx), b, reps, _lib.ptr(bv), s), "replay_gather_u8")
        _lib.check(lib.lbc_replay_meta(_lib.ptr(self.speed), _lib.ptr(self.cmd), _lib.ptr(idx), b, reps, _lib.ptr(speed), _lib.ptr(onehot), s), "replay_meta")
        return rgb, bv, onehot, speed

    def update_weights(self, idx, w_batch, reps=1):
        """new_weights[idx[b]] = mean of w_batch[b*reps : (b+1)*reps]; of equal indices the last wins; nothing leaves the device"""
        idx = self._index(idx)
        w = w_batch.detach().to(device=self.device, dtype=torch.float32).contiguous()
        b, reps = int(idx.numel()), int(reps)
        if int(w.numel()) != b * reps:
            raise ValueError("DeviceReplayBuffer.update_weights: %d weights for %d indices x %d copies" % (w.numel(), b, reps))
        for b0 in range(0, b, WRITEBACK_MAX):                         # (in order: a later chunk overwrites an earlier one)
            nb = min(WRITEBACK_MAX, b - b0)
            _lib.check(_lib.get().lbc_replay_writeback(_lib.ptr(w[b0 * reps:]), _lib.ptr(idx[b0:]), nb, reps, self.n, _lib.ptr(self.new_weights),
                                                       self._stream()), "replay_writeback")

    def normalize_weights(self):
        """end of an epoch: the written-back weights become the sampling weights and their prefix sums are rebuilt.  Reads back (total,
        bad) -- the buffer's one sync per epoch.  -> the number of weights that are negative, NaN or infinite (they count as 0; logged
        when there are any); ValueError when no weight is left to sample from."""
        self.weights, self.new_weights = self.new_weights, self.weights
        self._rebuild_cdf()
        got = torch.cat([self.cdf[self.n - 1:self.n], self._bad.to(torch.float64)]).cpu()
        total, bad = float(got[0]), int(got[1])
        if bad:
            logging.getLogger(__name__).warning("DeviceReplayBuffer.normalize_weights: %d of %d weights are negative, NaN or infinite and count as 0", bad, self.n)
        if not total > 0:
            self.normalized = False
            raise ValueError("DeviceReplayBuffer.normalize_weights: the %d weights sum to %r, there is nothing to sample from" % (self.n, total))
        self.normalized = True
        return bad

    def _rebuild_cdf(self):
        if self.n < 1:
            raise ValueError("DeviceReplayBuffer: the buffer is empty")
        _lib.check(_lib.get().lbc_replay_cdf(_lib.ptr(self.weights), self.n, _lib.ptr(self.cdf), _lib.ptr(self._bad), self._stream()), "replay_cdf")

    def get_highest_k(self, k):
        top = torch.topk(self.weights[:self.n], int(k)).indices.to(torch.int32)
        return (top,) + self.batch(top)

    # ---- resumable state ---------------------------------------------------------------------------------------
    def state_dict(self, include_frames=False):
        """what the next index streams depend on: the weights (the prefix sums are rebuilt from them), the shuffle and its position,
        the sampler's seed and counter, the host generator; cmd / speed; the frames only on request (442 KB each).  With a source:
        the slots' frame indices and the source's frame count instead (include_frames has nothing to include)"""
        n = self.n
        cpu = lambda t: t[:n].detach().cpu().clone()
        sd = {"format": 1, "n": n, "buffer_limit": self.buffer_limit, "normalized": bool(self.normalized), "weights": cpu(self.weights),
              "new_weights": cpu(self.new_weights), "cmd": cpu(self.cmd), "speed": cpu(self.speed),
              "perm": None if self._perm is None else torch.from_numpy(np.asarray(self._perm, dtype=np.int64).copy()), "perm_pos": int(self._perm_pos),
              "seed": int(self.seed), "draws": int(self.draws), "rng": rng_state_to_dict(self._rng)}
        if self.source is not None:
            sd["frame"], sd["source_frames"] = cpu(self.frame), int(self.slot_of_frame.numel())
        elif include_frames:
            sd["rgb"], sd["birdview"] = cpu(self.rgb), cpu(self.birdview)
        return sd

    def load_state_dict(self, sd):
        if sd.get("format") != 1:
            raise ValueError("DeviceReplayBuffer.load_state_dict: unknown state format %r" % (sd.get("format"),))
        n = int(sd["n"])
        if n > self.buffer_limit:
            raise ValueError("DeviceReplayBuffer.load_state_dict: the state holds %d samples, this buffer has %d slots" % (n, self.buffer_limit))
        if self.source is not None or "frame" in sd:
            if self.source is None or "frame" not in sd:
                raise ValueError("DeviceReplayBuffer.load_state_dict: the state %s frame indices into a source, this buffer %s"
                                 % (("holds", "stores frames") if "frame" in sd else ("holds no", "needs them")))
            if int(sd["source_frames"]) != int(self.slot_of_frame.numel()):
                raise ValueError("DeviceReplayBuffer.load_state_dict: the state indexes a dataset of %d frames, this buffer's source holds %d"
                                 % (sd["source_frames"], self.slot_of_frame.numel()))
            frame = sd["frame"].to(torch.int64)
            if n and (int(frame.min()) < 0 or int(frame.max()) >= self.slot_of_frame.numel() or frame.unique().numel() != n):
                raise ValueError("DeviceReplayBuffer.load_state_dict: the state's frame indices are not %d distinct frames of the source" % n)
            self.frame.fill_(-1)
            self.frame[:n].copy_(sd["frame"])
            self.slot_of_frame.fill_(-1)
            self.slot_of_frame[frame.to(self.device)] = torch.arange(n, dtype=torch.int32, device=self.device)
        elif "rgb" in sd:
            self.rgb[:n].copy_(sd["rgb"])
            self.birdview[:n].copy_(sd["birdview"])
        elif n != self.n:
            raise ValueError("DeviceReplayBuffer.load_state_dict: the state was saved without frames for %d samples, this buffer holds %d" % (n, self.n))
        self.n = n
        for name in ("weights", "new_weights", "cmd", "speed"):
            getattr(self, name)[:n].copy_(sd[name])
        self.seed, self.draws = int(sd["seed"]), int(sd["draws"])
        rng_state_from_dict(self._rng, sd["rng"])
        self._set_perm(None if sd["perm"] is None else sd["perm"].cpu().numpy(), sd["perm_pos"])
        self.normalized = bool(sd["normalized"])
        if self.normalized:
            self._rebuild_cdf()
