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
DeviceLoader stages one batch ahead, so a pass the consumer ABANDONS leaves its sampler one batch further than this loader's.

teacher=... (--cache-teacher): in phases 0 and 1 the privileged teacher is frozen and its three inputs -- the fixed bird-view window,
table[row][3], table[row][4] -- are constants of a frame, so its waypoints are a function of the frame index.  Given a teacher the
loader runs it ONCE over the dataset while it loads, chunk by chunk in dataset order, and keeps
  teacher_rows   f32 [F,50] = `all` (4 x 5 x 2) then `sel` (5 x 2) of every frame, exactly as the forward returned them
instead of the bird-view frames, which are then never resident as a whole (200 bytes per frame in place of 258,048).  Slot 1 of a
batch is then a TeacherWaypoints(sel, all) out of one lbc_dataset_gather_rows_f32 launch; everything else -- draws, replication,
augmentation stream, state -- is what it is without a teacher."""
import collections
import ctypes
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
TEACHER_ROW = 4 * 5 * 2 + 5 * 2           # floats of a cached frame: every branch's waypoints, then the commanded branch's

# slot 1 of a batch of a loader with a teacher cache: the frozen teacher's waypoints, (n,5,2) and (n,4,5,2) f32.  Both are views of the
# gathered (n,50) rows -- row pitch 50 floats; NativeTrainer.step(teacher_out=...) packs the one its loss reads
TeacherWaypoints = collections.namedtuple("TeacherWaypoints", ["sel", "all"])


def tensor_versions(module):
    """torch's in-place version counters of a module's parameters and buffers (NativeTrainer._versions: the same tuple)"""
    return tuple(t._version for t in list(module.parameters()) + list(module.buffers()))


class ResidentLoader:
    """DeviceLoader's constructor arguments and batches; reserve_gb: device memory (GB) to leave free for networks and workspaces
    (default RESERVE_GB); mem_info: a callable -> (free, total) bytes in place of torch.cuda.mem_get_info (tests).
    teacher: a frozen BirdViewPolicyModelSS, or any callable (birdview u8 (n,192,192,7), speed (n,), one-hot command (n,4)) -> (sel
    (n,5,2), all (n,4,5,2)): its waypoints are cached per frame and handed out in the bird-view's place (see the module text);
    teacher_batch: frames per forward of that one pass over the dataset (default: batch_size)."""

    def __init__(self, dataset, batch_size, samples, device, augment=None, batch_aug=1, seed=0, rank=0, reserve_gb=None, mem_info=None,
                 teacher=None, teacher_batch=None):
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
        self.teacher, self.teacher_rows, self.build_seconds = teacher, None, 0.0
        self.teacher_batch = self.batch if teacher_batch is None else int(teacher_batch)
        if teacher is not None:
            if self.whole_map:
                raise ValueError("ResidentLoader: a teacher cache needs a dataset whose bird-view window is fixed (ImageDataset); %s rotates "
                                 "and shifts it per draw, so the teacher's input is not a function of the frame index" % type(dataset).__name__)
            if self.teacher_batch < 1:
                raise ValueError("ResidentLoader: teacher_batch must be positive, got %r" % (teacher_batch,))
        if self.device.type != "cuda":
            _lib.require_device(torch.empty(0))                    # (only the emulated test build takes CPU tensors)
        t0 = time.time()
        self._plan(reserve_gb, mem_info)
        self._load()
        self.load_seconds = time.time() - t0
        cache = "" if teacher is None else (", teacher cache %d bytes in place of %d bytes of bird-view frames, built in %.2f s"
                                            % (self.cache_bytes, self.frames * int(np.prod(self._map_shape)), self.build_seconds))
        print("ResidentLoader: %d frames, %d bytes resident on %s (%d table rows), loaded in %.2f s%s"
              % (self.frames, self.resident_bytes, self.device, self.rows, self.load_seconds, cache))

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
        map_bytes = F * int(np.prod(self._map_shape))
        # with a teacher cache the maps only pass through: 200 bytes per frame stay, and while the cache is built one chunk of
        # teacher_batch maps and the inference engine's workspace stand beside the steady state
        self.cache_bytes = self.build_bytes = 0
        if self.teacher is not None:
            self.cache_bytes = F * TEACHER_ROW * 4
            self.build_bytes = min(self.teacher_batch, max(F, 1)) * int(np.prod(self._map_shape)) + self._teacher_workspace_bytes()
            map_bytes = self.cache_bytes
        self.resident_bytes = int(rgb_bytes + map_bytes + self.rows * 5 * 4 + F * 4 + (2 * self.angle_jitter + 1) * 56)
        self.peak_bytes = self.resident_bytes + self.build_bytes
        self.reserved_bytes = int(round((RESERVE_GB if reserve_gb is None else float(reserve_gb)) * 1e9))
        if mem_info is None and self.device.type == "cuda":
            mem_info = lambda: torch.cuda.mem_get_info(self.device)
        if mem_info is not None:                                   # (the emulated test build has no device memory to ask about)
            free = int(mem_info()[0])
            if self.teacher is not None and self.peak_bytes > free - self.reserved_bytes:
                raise RuntimeError("ResidentLoader: the dataset with its teacher cache needs %d bytes on %s (%d of them the cache) and, while "
                                   "the cache is built, %d bytes more for one chunk of %d maps and the teacher's workspace: %d bytes at the "
                                   "peak; %d bytes are free and %d bytes are reserved for networks and workspaces (--resident-reserve-gb): it "
                                   "does not fit; run without --resident"
                                   % (self.resident_bytes, self.device, self.cache_bytes, self.build_bytes, self.teacher_batch, self.peak_bytes,
                                      free, self.reserved_bytes))
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
        stage = torch.empty(UPLOAD_CHUNK_BYTES, dtype=torch.uint8)
        if self.with_rgb:
            self._upload(self.rgb, stage, lambda env, i: np.frombuffer(env.get("rgb_%04d" % i), np.uint8).reshape(RGB_SHAPE))
        s = ds.crop_size
        full = lambda env, i: np.frombuffer(env.get("birdview_%04d" % i), np.uint8).reshape(MAP_SIZE, MAP_SIZE, MAP_CHANNELS)
        window = lambda env, i: full(env, i)[CROP_Y0:CROP_Y0 + s, CROP_X0:CROP_X0 + s]
        if self.teacher is not None:
            self.birdview = None                     # (the maps pass through the staging buffer into the teacher, chunk by chunk)
            t0 = time.time()
            self._build_teacher_rows(stage, window)
            self.build_seconds = time.time() - t0
            return
        self.birdview = torch.empty((F,) + self._map_shape, dtype=torch.uint8, device=dev)
        self._upload(self.birdview, stage, full if self.whole_map else window)

    def _upload(self, dst, stage, read, first=0):
        """dataset frames first, first + 1, ... -> dst[0], dst[1], ..., through the staging buffer"""
        ds, count = self.data, int(dst.shape[0])
        per = max(1, stage.numel() // max(1, int(dst[0].numel()) if count else 1))
        for f0 in range(0, count, per):
            n = min(per, count - f0)
            view = stage[:n * dst[0].numel()].view((n,) + tuple(dst.shape[1:]))
            buf = view.numpy()
            for k in range(n):
                np.copyto(buf[k], read(ds.envs[ds.file_map[first + f0 + k]], ds.idx_map[first + f0 + k]))
            dst[f0:f0 + n].copy_(view)               # (pageable source: the copy has left the buffer when this returns)

    # ---- the teacher cache -------------------------------------------------------------------------------------
    def _teacher_net_desc(self):
        """the executor plan of a policy-model teacher at the resident window and teacher_batch, None for a plain callable"""
        from ...models.common import PolicyBase
        t = self.teacher
        if not isinstance(t, PolicyBase):
            return None
        prec = {"fp32": 0, "bf16_mfma": 1, "bf16": 2, "bf16x3": 3}[t.precision]
        side = self.data.crop_size
        return (t._arch(), t.input_channel, side, side, t._normalize, max(1, min(self.teacher_batch, self.frames)), self.device, prec)

    def _teacher_workspace_bytes(self):
        desc = self._teacher_net_desc()
        if desc is None:
            return 0
        lib, h = _lib.get(), ctypes.c_void_p()
        nd = _lib.NetDesc(desc[0], desc[1], desc[2], desc[3], int(desc[4]), desc[5], desc[7])
        _lib.check(lib.lbc_net_create(ctypes.byref(nd), ctypes.byref(h)), "net_create")
        try:
            return int(lib.lbc_net_workspace_bytes(h))
        finally:
            lib.lbc_net_destroy(h)

    def _teacher_forward(self):
        """-> f(birdview u8 chunk, speed, one-hot command) -> (sel, all).  A policy model runs on an inference engine of its own --
        no gradients, frozen (weight copies and folded BatchNorm derived once), the model's precision -- that lives as long as f does."""
        desc = self._teacher_net_desc()
        if desc is None:
            return self.teacher
        from ....engine import PolicyEngine
        t = self.teacher
        eng = PolicyEngine(*desc)
        tensors = dict(t.named_parameters())
        tensors.update(dict(t.named_buffers()))
        eng.bind({k: v.data for k, v in tensors.items() if k in set(eng.names)}, False, param_order=t._param_names)
        eng.set_frozen(True)
        return lambda bv, speed, cmd: eng.forward(bv, speed, cmd, False)

    def _build_teacher_rows(self, stage, read):
        """one pass over the dataset in its own order, teacher_batch frames at a time (the last chunk may be short): the chunk's maps
        through the staging buffer, speed and command from the table entries lbc_dataset_targets and __iter__ read, the forward, the
        50 floats per frame stored; the chunk, the engine and its workspace are gone when this returns"""
        from ..train_utils import one_hot
        dev, F, n = self.device, self.frames, self.teacher_batch
        self.teacher_rows = torch.empty((F, TEACHER_ROW), dtype=torch.float32, device=dev)
        speed = self.table[:, 3][self.row_of_sample.long()].contiguous() if F else torch.zeros(0, device=dev)
        cmd = one_hot(self.cmd_host).to(dev) if F else torch.zeros((0, 4), device=dev)
        forward = self._teacher_forward()
        chunk = torch.empty((min(n, F),) + self._map_shape, dtype=torch.uint8, device=dev)
        with torch.no_grad():
            for f0 in range(0, F, n):
                m = min(n, F - f0)
                self._upload(chunk[:m], stage, read, first=f0)
                sel, every = forward(chunk[:m], speed[f0:f0 + m].contiguous(), cmd[f0:f0 + m].contiguous())
                if tuple(sel.shape) != (m, 5, 2) or tuple(every.shape) != (m, 4, 5, 2):
                    raise RuntimeError("ResidentLoader: the teacher returned %s and %s for %d frames, expected (n,5,2) and (n,4,5,2)"
                                       % (tuple(sel.shape), tuple(every.shape), m))
                self.teacher_rows[f0:f0 + m, :40] = every.reshape(m, 40)
                self.teacher_rows[f0:f0 + m, 40:] = sel.reshape(m, 10)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)          # (the engine is destroyed behind its last kernel; build_seconds is the work, not the enqueue)
        del forward, chunk
        self._teacher_versions = tensor_versions(self.teacher) if isinstance(self.teacher, torch.nn.Module) else ()

    def _check_teacher(self):
        if isinstance(self.teacher, torch.nn.Module) and tensor_versions(self.teacher) != self._teacher_versions:
            raise RuntimeError("ResidentLoader: the teacher cache is stale -- a parameter or buffer of the teacher was written in place after "
                               "the cache was built; build the loader again (a frozen teacher is what makes its waypoints cacheable)")

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
        loc, speed) on the device, every sample `reps` times back to back; with a teacher cache a TeacherWaypoints stands in the
        bird-view's position.  An index outside the dataset or an angle outside the table is refused here: the kernels trust what they
        are handed."""
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
        s, side = _lib.stream_for(draws), ds.crop_size
        rgb = None
        if self.with_rgb:
            rgb = torch.empty((n * reps,) + RGB_SHAPE, dtype=torch.uint8, device=dev)
            idx = draws[:, 0].contiguous()
            _lib.check(lib.lbc_dataset_gather_crop_u8(_lib.ptr(self.rgb), _lib.ptr(idx), n, reps, RGB_SHAPE[0], RGB_SHAPE[1], RGB_SHAPE[2], 0, 0,
                                                      RGB_SHAPE[0], RGB_SHAPE[1], _lib.ptr(rgb), s), "dataset_gather_crop_u8")
        if self.teacher_rows is not None:
            # the cached waypoints in the map's place: one row copy through the record, then two views of the copied rows
            rows = torch.empty((n * reps, TEACHER_ROW), dtype=torch.float32, device=dev)
            _lib.check(lib.lbc_dataset_gather_rows_f32(_lib.ptr(self.teacher_rows), _lib.ptr(draws), 4, n, reps, TEACHER_ROW, _lib.ptr(rows), s),
                       "dataset_gather_rows_f32")
            bv = TeacherWaypoints(rows[:, 40:].unflatten(1, (5, 2)), rows[:, :40].unflatten(1, (4, 5, 2)))
        else:
            bv = torch.empty((n * reps, side, side, MAP_CHANNELS), dtype=torch.uint8, device=dev)
            if self.jitter or warp:
                _lib.check(lib.lbc_dataset_gather_warp_crop_u8(_lib.ptr(self.birdview), _lib.ptr(draws), _lib.ptr(self.warp_table), self.angle_jitter, n,
                                                               reps, MAP_SIZE, MAP_SIZE, MAP_CHANNELS, side, side, _lib.ptr(bv), s),
                           "dataset_gather_warp_crop_u8")
            else:
                idx = draws[:, 0].contiguous()
                y0, x0 = (CROP_Y0, CROP_X0) if self.whole_map else (0, 0)
                _lib.check(lib.lbc_dataset_gather_crop_u8(_lib.ptr(self.birdview), _lib.ptr(idx), n, reps, self._map_shape[0], self._map_shape[1],
                                                          MAP_CHANNELS, y0, x0, side, side, _lib.ptr(bv), s), "dataset_gather_crop_u8")
        loc = torch.empty((n * reps, ds.n_step, 2), dtype=torch.float32, device=dev)
        speed = torch.empty(n * reps, dtype=torch.float32, device=dev)
        _lib.check(lib.lbc_dataset_targets(_lib.ptr(self.table), _lib.ptr(self.row_of_sample), _lib.ptr(draws), n, reps, ds.gap, ds.n_step, ds.img_size,
                                           ds.crop_size, _lib.ptr(loc), _lib.ptr(speed), s), "dataset_targets")
        return rgb, bv, loc, speed

    def __iter__(self):
        if self.teacher is not None:
            self._check_teacher()                     # (a teacher written in place since the build: its cached waypoints are no longer its own)
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
