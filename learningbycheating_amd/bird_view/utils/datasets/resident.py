"""The LMDB frame dataset held in HBM (--resident): DeviceLoader's batches without DeviceLoader's per-sample host work.

DeviceLoader._fill looks every sample up in the LMDB files, copies 184 KB + 717 KB into staging, derives the waypoints in numpy and
sends the batch across PCIe, for every batch.  ResidentLoader reads every episode ONCE, at construction, and keeps on the device:
  rgb            u8 [F,160,384,3]                     (only when dataset.needs_rgb)
  birdview       u8 [F,192,192,7] rows 58:250, cols 64:256 for datasets whose window is fixed (ImageDataset),
                 u8 [F,320,320,7] whole for BirdViewDataset, whose window moves and rotates
  table          f32 [rows,5] = (x, y, heading, speed, cmd), one row per stored frame of every episode -- the gap * n_step tail frames
                 that only serve as futures included -- episodes contiguous; heading / speed by the expressions of ImageDataset.raw()
  row_of_sample  int32 [F]
  warp_table     one lbc_warp_params per integer angle in [-angle_jitter, angle_jitter], by image_lmdb.warp_params()
and a host copy of the cmd column.  Per batch the host draws -- the same RandomState(seed * 9973 + rank), the same order of draws as
DeviceLoader._fill -- and uploads B records of (idx, delta_angle, dx, dy) int32; csrc/dataset.hip does the rest on the current stream:
lbc_dataset_gather_crop_u8 (camera frames, fixed window), lbc_dataset_gather_warp_crop_u8 (jittered window), lbc_dataset_targets
(waypoints, speed).  Nothing is read back and nothing is prefetched.

The batches are DeviceLoader's: same 5-tuple, shapes, dtypes and placement, same batch_aug replication and colour augmentation, bytes
equal bit for bit (waypoints: the kernel restates raw()'s arithmetic in double with device cos / sin, equal within 1e-3 px).  The state
format is DeviceLoader's too, and a state saved by either class continues in the other.  One difference in what the sampler has drawn:
DeviceLoader stages one batch ahead, so a pass the consumer ABANDONS leaves its sampler one batch further than this loader's."""
import time

import numpy as np
import torch

from ... import augmenter as augmenter_mod
from .... import _lib
from .image_lmdb import CROP_X0, CROP_Y0, PIXEL_OFFSET, warp_params

# What a training run needs beside the dataset, in GB (10^9 bytes): DESIGN.md section 2 gives the bump-allocated workspaces at batch 256
# in f32 as 13 GB for the student and 4 GB for the teacher; parameters, gradients, Adam moments, the weight average (5 x 92 MB), the
# batch itself (256 x 443 KB, twice) and the caching allocator's slack are covered by 3 GB more.
RESERVE_GB = 13 + 4 + 3
UPLOAD_CHUNK_BYTES = 64 << 20           # the one staging buffer every tensor is uploaded through
MAP_SIZE, MAP_CHANNELS = 320, 7
RGB_SHAPE = (160, 384, 3)


class ResidentLoader:
    """DeviceLoader's constructor arguments and batches; reserve_gb: device memory (GB) to leave free for networks and workspaces
    (default RESERVE_GB); mem_info: a callable -> (free, total) bytes in place of torch.cuda.mem_get_info (tests)."""

    def __init__(self, dataset, batch_size, samples, device, augment=None, batch_aug=1, seed=0, rank=0, reserve_gb=None, mem_info=None):
        self.data, self.batch, self.samples, self.device = dataset, int(batch_size), samples, torch.device(device)
        self.batch_aug = int(batch_aug)
        self.rng = np.random.RandomState(seed * 9973 + rank)
        self.strategy = augmenter_mod.get(augment)
        self.aug = augmenter_mod.BatchAugmenter(None, seed=seed * 31 + rank) if self.strategy else None
        self.images_seen = dataset.batch_read_number
        self.position = 0                    # batches handed out by the pass in progress (0 between passes)
        self.resume_at = 0
        self.angle_jitter = int(getattr(dataset, "angle_jitter", 0) or 0)
        self.jitter = bool(self.angle_jitter or getattr(dataset, "crop_x_jitter", 0) or getattr(dataset, "crop_y_jitter", 0))
        self.with_rgb = bool(getattr(dataset, "needs_rgb", True))
        self.whole_map = hasattr(dataset, "angle_jitter")          # (a dataset with jitter attributes: its window is not fixed)
        if self.device.type != "cuda":
            _lib.require_device(torch.empty(0))                    # (only the emulated test build takes CPU tensors)
        t0 = time.time()
        self._plan(reserve_gb, mem_info)
        self._load()
        self.load_seconds = time.time() - t0
        print("ResidentLoader: %d frames, %d bytes resident on %s (%d table rows), loaded in %.2f s"
              % (self.frames, self.resident_bytes, self.device, self.rows, self.load_seconds))

    def __len__(self):
        return self.samples

    # ---- construction ------------------------------------------------------------------------------------------
    def _plan(self, reserve_gb, mem_info):
        """table rows per episode, bytes needed, and the comparison with what the device has left"""
        ds = self.data
        F = self.frames = len(ds)
        tail = ds.gap * ds.n_step
        file_map, idx_map = np.asarray(ds.file_map, np.int64), np.asarray(ds.idx_map, np.int64)
        count = np.zeros(len(ds.envs), np.int64)                   # stored frames of each episode that the table holds
        if F:
            np.maximum.at(count, file_map, idx_map + 1 + tail)
        self._episode_rows = count
        base = np.concatenate([[0], np.cumsum(count)[:-1]])
        self.rows = int(count.sum())
        self._row_of_sample = (base[file_map] + idx_map).astype(np.int32) if F else np.zeros(0, np.int32)
        side = ds.img_size if self.whole_map else ds.crop_size
        self._map_shape = (side, side, MAP_CHANNELS)
        rgb_bytes = F * int(np.prod(RGB_SHAPE)) if self.with_rgb else 0
        self.resident_bytes = int(rgb_bytes + F * int(np.prod(self._map_shape)) + self.rows * 5 * 4 + F * 4 + (2 * self.angle_jitter + 1) * 56)
        self.reserved_bytes = int(round((RESERVE_GB if reserve_gb is None else float(reserve_gb)) * 1e9))
        if mem_info is None and self.device.type == "cuda":
            mem_info = lambda: torch.cuda.mem_get_info(self.device)
        if mem_info is not None:                                   # (the emulated test build has no device memory to ask about)
            free = int(mem_info()[0])
            if self.resident_bytes > free - self.reserved_bytes:
                raise RuntimeError("ResidentLoader: the dataset needs %d bytes on %s, %d bytes are free and %d bytes are reserved for networks "
                                   "and workspaces (--resident-reserve-gb): it does not fit; run without --resident"
                                   % (self.resident_bytes, self.device, free, self.reserved_bytes))

    def _load(self):
        ds, dev, F = self.data, self.device, self.frames
        # the measurement table: every stored frame the samples or their futures touch
        table = np.zeros((self.rows, 5), np.float32)
        r = 0
        for e, env in enumerate(ds.envs):
            for i in range(int(self._episode_rows[e])):
                m = np.frombuffer(env.get("measurements_%04d" % i), np.float32)
                ox, oy, oz, ori_ox, ori_oy, vx, vy, vz = m[:8]
                table[r] = (ox, oy, np.arctan2(ori_oy, ori_ox), np.linalg.norm([vx, vy, vz]), m[11])       # (as ImageDataset.raw())
                r += 1
        self.cmd_host = torch.from_numpy(table[:, 4][self._row_of_sample].copy()) if F else torch.zeros(0)
        self.table = torch.from_numpy(table).to(dev)
        self.row_of_sample = torch.from_numpy(self._row_of_sample).to(dev)
        A = self.angle_jitter
        self.warp_table = torch.from_numpy(np.stack([warp_params(a, 0, 0, ds.crop_size) for a in range(-A, A + 1)])).to(dev)
        # the frames, through one pageable staging buffer (a pinned one that the GPU has read is slow to rewrite: image_lmdb.py DeviceLoader)
        self.rgb = torch.empty((F,) + RGB_SHAPE, dtype=torch.uint8, device=dev) if self.with_rgb else None
        self.birdview = torch.empty((F,) + self._map_shape, dtype=torch.uint8, device=dev)
        stage = torch.empty(UPLOAD_CHUNK_BYTES, dtype=torch.uint8)
        if self.with_rgb:
            self._upload(self.rgb, stage, lambda env, i: np.frombuffer(env.get("rgb_%04d" % i), np.uint8).reshape(RGB_SHAPE))
        s = ds.crop_size
        full = lambda env, i: np.frombuffer(env.get("birdview_%04d" % i), np.uint8).reshape(MAP_SIZE, MAP_SIZE, MAP_CHANNELS)
        self._upload(self.birdview, stage, full if self.whole_map else (lambda env, i: full(env, i)[CROP_Y0:CROP_Y0 + s, CROP_X0:CROP_X0 + s]))

    def _upload(self, dst, stage, read):
        ds = self.data
        per = max(1, stage.numel() // max(1, int(dst[0].numel()) if dst.shape[0] else 1))
        for f0 in range(0, self.frames, per):
            n = min(per, self.frames - f0)
            view = stage[:n * dst[0].numel()].view((n,) + tuple(dst.shape[1:]))
            buf = view.numpy()
            for k in range(n):
                np.copyto(buf[k], read(ds.envs[ds.file_map[f0 + k]], ds.idx_map[f0 + k]))
            dst[f0:f0 + n].copy_(view)               # (pageable source: the copy has left the buffer when this returns)

    # ---- one batch ---------------------------------------------------------------------------------------------
    def _draw(self):
        """the draws of DeviceLoader._fill in its order: all indices, then one jitter triple per sample -> int32 (B,4)"""
        rec = np.empty((self.batch, 4), np.int32)
        draw = getattr(self.data, "sample_index", None)          # command-biased sampling (BiasedBirdViewDataset), else uniform with replacement
        rec[:, 0] = [draw(self.rng) for _ in range(self.batch)] if draw else self.rng.randint(len(self.data), size=self.batch)
        rec[:, 1:] = (0, 0, -PIXEL_OFFSET)
        if self.jitter:
            for i in range(self.batch):
                rec[i, 1:] = self.data.draw_jitter(self.rng)
        return rec

    def gather(self, records, reps=1):
        """records: host integers (n,4) = (idx, delta_angle, dx, dy), or (n,) indices at the fixed window.  -> (rgb or None, birdview,
        loc, speed) on the device, every sample `reps` times back to back.  An index outside the dataset or an angle outside the
        table is refused here: the kernels trust what they are handed."""
        rec = np.asarray(records)
        if rec.ndim == 1:
            rec = np.concatenate([rec.reshape(-1, 1), np.tile(np.array([[0, 0, -PIXEL_OFFSET]]), (rec.shape[0], 1))], axis=1)
        if rec.ndim != 2 or rec.shape[1] != 4 or rec.shape[0] < 1 or not np.issubdtype(rec.dtype, np.integer):
            raise ValueError("ResidentLoader.gather: records must be integers of shape (n, 4) or (n,), n >= 1")
        if rec[:, 0].min() < 0 or rec[:, 0].max() >= self.frames:
            raise RuntimeError("ResidentLoader.gather: frame index %d outside the %d resident frames"
                               % (int(rec[:, 0].min() if rec[:, 0].min() < 0 else rec[:, 0].max()), self.frames))
        if np.abs(rec[:, 1]).max() > self.angle_jitter:
            raise RuntimeError("ResidentLoader.gather: delta_angle %d outside the warp table's [-%d, %d]"
                               % (int(rec[np.abs(rec[:, 1]).argmax(), 1]), self.angle_jitter, self.angle_jitter))
        warp = self.whole_map and bool((rec[:, 1] != 0).any() or (rec[:, 2] != 0).any() or (rec[:, 3] != -PIXEL_OFFSET).any())
        if not self.whole_map and (rec[:, 1:] != (0, 0, -PIXEL_OFFSET)).any():
            raise RuntimeError("ResidentLoader.gather: this dataset's window is fixed (the map is resident as its 192 x 192 crop)")
        ds, dev, lib = self.data, self.device, _lib.get()
        n, reps = int(rec.shape[0]), int(reps)
        draws = torch.from_numpy(np.ascontiguousarray(rec, dtype=np.int32)).to(dev)
        s, side = _lib.stream_for(self.birdview), ds.crop_size
        rgb = None
        if self.with_rgb:
            rgb = torch.empty((n * reps,) + RGB_SHAPE, dtype=torch.uint8, device=dev)
            idx = draws[:, 0].contiguous()
            _lib.check(lib.lbc_dataset_gather_crop_u8(_lib.ptr(self.rgb), _lib.ptr(idx), n, reps, RGB_SHAPE[0], RGB_SHAPE[1], RGB_SHAPE[2], 0, 0,
                                                      RGB_SHAPE[0], RGB_SHAPE[1], _lib.ptr(rgb), s), "dataset_gather_crop_u8")
        bv = torch.empty((n * reps, side, side, MAP_CHANNELS), dtype=torch.uint8, device=dev)
        if self.jitter or warp:
            _lib.check(lib.lbc_dataset_gather_warp_crop_u8(_lib.ptr(self.birdview), _lib.ptr(draws), _lib.ptr(self.warp_table), self.angle_jitter, n, reps,
                                                           MAP_SIZE, MAP_SIZE, MAP_CHANNELS, side, side, _lib.ptr(bv), s), "dataset_gather_warp_crop_u8")
        else:
            idx = draws[:, 0].contiguous()
            y0, x0 = (CROP_Y0, CROP_X0) if self.whole_map else (0, 0)
            _lib.check(lib.lbc_dataset_gather_crop_u8(_lib.ptr(self.birdview), _lib.ptr(idx), n, reps, self._map_shape[0], self._map_shape[1], MAP_CHANNELS,
                                                      y0, x0, side, side, _lib.ptr(bv), s), "dataset_gather_crop_u8")
        loc = torch.empty((n * reps, ds.n_step, 2), dtype=torch.float32, device=dev)
        speed = torch.empty(n * reps, dtype=torch.float32, device=dev)
        _lib.check(lib.lbc_dataset_targets(_lib.ptr(self.table), _lib.ptr(self.row_of_sample), _lib.ptr(draws), n, reps, ds.gap, ds.n_step, ds.img_size,
                                           ds.crop_size, _lib.ptr(loc), _lib.ptr(speed), s), "dataset_targets")
        return rgb, bv, loc, speed

    def __iter__(self):
        start, self.resume_at = self.resume_at, 0     # (a state restored in the middle of a pass: only the rest of that pass)
        try:
            for i in range(start, self.samples):
                rec = self._draw()
                rgb, bv, loc, speed = self.gather(rec, self.batch_aug)
                cmd = self.cmd_host[torch.from_numpy(rec[:, 0].astype(np.int64))]
                if self.batch_aug > 1:               # reference train_image_phase1.py:131-154,183-189: every frame batch_aug times, back to back
                    cmd = cmd.repeat_interleave(self.batch_aug, dim=0)
                if self.strategy is not None and rgb is not None:
                    self.aug.recipe = self.strategy(self.images_seen)       # strength schedule by images read (image_lmdb.py:138,220)
                    self.aug.augment_batch(rgb)      # (rgb is a gathered copy of the resident frames)
                self.images_seen += self.batch * self.batch_aug
                self.position = i + 1
                yield rgb, bv, loc, cmd, speed
        finally:
            self.position = 0

    # ---- state: DeviceLoader's format ----------------------------------------------------------------------------
    def state_dict(self):
        """sampler stream, augmenter stream, strength counter and the position inside the pass in progress, as DeviceLoader.state_dict().
        Exact at every batch boundary: nothing is prefetched, the sampler stands where the next batch's draws begin -- which is what
        DeviceLoader records for its staged batch."""
        return {"images_seen": int(self.images_seen), "position": int(self.position), "frames": len(self.data),
                "rng": augmenter_mod.rng_state_to_dict(self.rng), "aug": self.aug.state_dict() if self.aug is not None else None}

    def load_state_dict(self, sd):
        if int(sd["frames"]) != len(self.data):
            raise ValueError("ResidentLoader.load_state_dict: the state samples %d frames, this dataset holds %d" % (sd["frames"], len(self.data)))
        if (sd["aug"] is None) != (self.aug is None):
            raise ValueError("ResidentLoader.load_state_dict: the state and this loader disagree about augmentation")
        augmenter_mod.rng_state_from_dict(self.rng, sd["rng"])
        if self.aug is not None:
            self.aug.load_state_dict(sd["aug"])
        self.images_seen = int(sd["images_seen"])
        self.resume_at = int(sd.get("position", 0))
