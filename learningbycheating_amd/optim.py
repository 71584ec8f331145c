"""Multi-tensor Adam on the HIP kernel (csrc/adam.hip) -- torch.optim.Adam semantics
(reference call sites training/train_image_phase{0,1}.py:231,252, lr 1e-4)."""
import ctypes
import dataclasses

import numpy as np
import torch

from . import _lib

CHUNK = 32768


@dataclasses.dataclass(frozen=True)
class LRSchedule:
    """The learning-rate schedule of FusedAdam's recipe path (csrc/adam.hip), evaluated on the device at k = the number of updates
    applied so far: k < warmup_steps: base * (warmup_start + (1 - warmup_start) * k / warmup_steps); afterwards, with j = k - warmup_steps,
    "constant": base; "cosine": min_lr + (base - min_lr) * 0.5 * (1 + cos(pi * min(j, T - W) / (T - W))) with T = total_steps;
    "step": base * gamma ** (j // step_size).  The base rate is the optimizer's `lr`."""
    kind: str = "constant"
    warmup_steps: int = 0
    warmup_start: float = 0.0
    total_steps: int = 0
    min_lr: float = 0.0
    step_size: int = 1
    gamma: float = 1.0

    @classmethod
    def of(cls, x):
        """None (constant, no warm-up), a dict with these fields, or an LRSchedule"""
        if x is None:
            return cls()
        sch = x if isinstance(x, cls) else cls(**dict(x))
        if sch.kind not in _lib.LR_SCHEDULES:
            raise ValueError("LRSchedule: unknown kind %r (one of %s)" % (sch.kind, ", ".join(_lib.LR_SCHEDULES)))
        if int(sch.warmup_steps) != sch.warmup_steps or sch.warmup_steps < 0:
            raise ValueError("LRSchedule: warmup_steps must be a non-negative integer, got %r" % (sch.warmup_steps,))
        if not 0.0 <= sch.warmup_start <= 1.0:
            raise ValueError("LRSchedule: warmup_start must lie in [0, 1], got %r" % (sch.warmup_start,))
        if sch.kind == "cosine" and not int(sch.total_steps) > int(sch.warmup_steps):
            raise ValueError("LRSchedule: a cosine schedule needs total_steps (%r) > warmup_steps (%r)" % (sch.total_steps, sch.warmup_steps))
        if sch.kind == "cosine" and sch.min_lr != sch.min_lr:
            raise ValueError("LRSchedule: min_lr is NaN")
        if sch.kind == "step" and not (int(sch.step_size) == sch.step_size and sch.step_size >= 1 and sch.gamma > 0):
            raise ValueError("LRSchedule: a step schedule needs an integer step_size >= 1 and gamma > 0, got %r and %r" % (sch.step_size, sch.gamma))
        return sch

    def as_dict(self):
        return dataclasses.asdict(self)


class FusedAdam:
    """Adam over (param, grad) pairs whose physical memory is dense (any stride permutation);
    grads are the engine's flat-buffer views, so p, g, m, v share one element order.

    guarded=True: every step first scans the gradients for NaN / +-Inf on the device (csrc/adam.hip) and skips the whole
    update when it finds one -- parameters, both moments and the step count keep their bits.  The step count then lives in a device
    record (lbc_adam_state), no step ever syncs; `step_count` and `skipped()` read the record back (a device-to-host copy: for logging
    and checkpoints only).

    max_grad_norm=X (a number; implies guarded): the gradient pass of the guard also sums the squares (csrc/adam.hip), and the update
    multiplies every gradient element by torch.nn.utils.clip_grad_norm_'s coefficient min(1, X / (norm + 1e-6)), all on the device and
    still without a sync.  X = 0 measures the norm and never clips.  THE GRADIENT VIEWS KEEP THE UNCLIPPED VALUES: the coefficient is
    applied inside the update, the gradient buffer is not written.  `grad_stats()` reads norm, coefficient and the number of clipped
    steps back (a sync, like `skipped()`).  None (the default) leaves the two paths above exactly as they are.  The attribute
    `max_grad_norm` of a clipped optimizer may be assigned another number between steps: step() passes its current value with every
    call (the choice between the clipped and the other paths is made once, here).

    schedule=... / decoupled_weight_decay=True / ema_decay=D: any of them selects the recipe path (csrc/adam.hip), built like the
    clipped step and like it without a sync; it always guards and always measures the norm (max_grad_norm=None measures only there).
    `schedule` (an LRSchedule or a dict of its fields) makes `lr` the BASE rate: the rate of a step is a function of the device record's
    step count, which a skipped step does not advance.  decoupled_weight_decay: p *= 1 - lr * weight_decay in front of the update
    (torch.optim.AdamW) instead of the coupled L2 term.  ema_decay: `ema`, a flat shadow in the element order and padding of `exp_avg`
    (a copy of the parameters at construction, or the buffer passed as `ema=`), moves by e += (1 - D) * (p' - e) inside the update
    launch; a skipped step leaves it alone.  `ema_of(name)` is a view in the parameter's logical shape, `lr_stats()` reads the last
    applied step's rate and the number of average updates back (a sync, like grad_stats()).  Schedule and shadow are not part of torch's
    format: NativeTrainer.state_dict carries them.

    state_dict() / load_state_dict() speak torch.optim.Adam's own format (moments in the parameters' logical shapes, parameters indexed
    in named_parameters() order), so a sidecar written here loads into a torch.optim.Adam over the reference-layout module and back."""

    def __init__(self, named_params, grads, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, guarded=False,
                 max_grad_norm=None, schedule=None, decoupled_weight_decay=False, ema_decay=None, ema=None):
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.decoupled = bool(decoupled_weight_decay)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        if self.ema_decay is not None and not 0.0 < self.ema_decay < 1.0:
            raise ValueError("FusedAdam: ema_decay must lie in (0, 1), got %r (None = no average)" % (ema_decay,))
        self.recipe = schedule is not None or self.decoupled or self.ema_decay is not None
        self.schedule = LRSchedule.of(schedule) if self.recipe else None
        if ema is not None and self.ema_decay is None:
            raise ValueError("FusedAdam: an ema buffer was passed without ema_decay")
        if self.recipe and max_grad_norm is None:
            max_grad_norm = 0.0                                       # the recipe path always measures the norm; 0 never clips
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        if self.max_grad_norm is not None and self.max_grad_norm != self.max_grad_norm:
            raise ValueError("FusedAdam: max_grad_norm is NaN")
        self.clipped = self.max_grad_norm is not None
        self.guarded = bool(guarded) or self.clipped
        self._step_count = 0
        self.all_names = [n for n, _ in named_params]
        self.names = [n for n, _ in named_params if n in grads]
        params = dict(named_params)
        # moments in the gradients' element order, every tensor starting on a 64-element (256-byte) boundary: adam_update_k moves
        # 16 bytes per lane, so p, g, m and v of every chunk must be 16-byte aligned (the engine's flat gradient buffer pads
        # the same way; the 5-element head biases would otherwise misalign everything behind them)
        from .engine import _pad
        total = sum(_pad(params[n].numel()) for n in self.names)
        dev = params[self.names[0]].device
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        rows, off = [], 0
        self.offsets = {}
        for n in self.names:
            p, g = params[n].data, grads[n]
            assert p.stride() == g.stride() and p.dtype == torch.float32
            assert p.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0, "adam: %s is not 16-byte aligned" % n
            self.offsets[n] = (off, p.numel())
            for c in range(0, p.numel(), CHUNK):
                k = min(CHUNK, p.numel() - c)
                rows.append((p.data_ptr() + 4 * c, g.data_ptr() + 4 * c, self.exp_avg.data_ptr() + 4 * (off + c),
                             self.exp_avg_sq.data_ptr() + 4 * (off + c), k))
            off += _pad(p.numel())
        table = np.zeros(len(rows), dtype=[("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i4"), ("pad", "<i4")])
        for i, r in enumerate(rows):
            table[i] = r + (0,)
        assert table.itemsize == ctypes.sizeof(_lib.AdamChunk)
        self.nchunks = len(rows)
        lib = _lib.get()
        lib.lbc_adam_profile_elems(sum(params[n].numel() for n in self.names))     # (books the launch profiler's 28 bytes per element)
        self.table = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
        self._keep = (params, grads)
        # one device record per guarded mode: its header and, from the clipped step on, one partial sum of squares per chunk behind it
        self._State, nbytes = ((None, 0) if not self.guarded else
                               (_lib.AdamRecipeState, lib.lbc_adam_recipe_state_bytes(self.nchunks)) if self.recipe else
                               (_lib.AdamClipState, lib.lbc_adam_clip_state_bytes(self.nchunks)) if self.clipped else
                               (_lib.AdamState, lib.lbc_adam_state_bytes()))
        self.record = None
        if self.guarded:
            assert int(nbytes) == ctypes.sizeof(self._State) + (8 * self.nchunks if self.clipped else 0), "lbc_%s layout" % self._State.__name__
            self.record = torch.zeros(int(nbytes), dtype=torch.uint8, device=dev)      # (torch allocations are 256-byte aligned)
        self.ema, self.ema_table = None, None
        if self.ema_decay is not None:
            if ema is None:
                ema = torch.zeros(total, dtype=torch.float32, device=dev)
                fresh = True
            else:
                if ema.dtype != torch.float32 or ema.numel() != total or not ema.is_contiguous() or ema.device != self.exp_avg.device:
                    raise ValueError("FusedAdam: the ema buffer must be a contiguous float32 tensor of %d elements on %s" % (total, dev))
                fresh = False
            assert ema.data_ptr() % 16 == 0, "adam: the ema buffer is not 16-byte aligned"
            self.ema = ema
            if fresh:
                for n in self.names:
                    self.ema_of(n).copy_(params[n].data)
            ptrs = np.array([self.ema.data_ptr() + (r[2] - self.exp_avg.data_ptr()) for r in rows], dtype=np.uint64)
            self.ema_table = torch.from_numpy(ptrs.view(np.int64).copy()).to(dev)   # one float* per chunk: the chunk's slice of the shadow

    # ---- the step ---------------------------------------------------------------------------
    def _recipe_struct(self):
        sch = self.schedule
        return _lib.AdamRecipe(schedule=_lib.LR_SCHEDULES[sch.kind], base_lr=float(self.lr), warmup_steps=int(sch.warmup_steps),
                               warmup_start=float(sch.warmup_start), total_steps=int(sch.total_steps), min_lr=float(sch.min_lr),
                               step_size=int(sch.step_size), gamma=float(sch.gamma), weight_decay=float(self.weight_decay),
                               decoupled=int(self.decoupled), max_norm=float(self.max_grad_norm),
                               ema_decay=0.0 if self.ema_decay is None else self.ema_decay, beta1=float(self.betas[0]),
                               beta2=float(self.betas[1]), eps=float(self.eps))

    def step(self):
        if self.recipe:
            rc = self._recipe_struct()
            _lib.check(_lib.get().lbc_adam_step_recipe(_lib.ptr(self.table), self.nchunks, ctypes.byref(rc), _lib.ptr(self.ema_table),
                                                       _lib.ptr(self.record), _lib.stream_for(self.table)), "adam_step_recipe")
            return
        if self.clipped:
            _lib.check(_lib.get().lbc_adam_step_clipped(_lib.ptr(self.table), self.nchunks, self.lr, self.betas[0], self.betas[1], self.eps,
                                                        self.weight_decay, self.max_grad_norm, _lib.ptr(self.record),
                                                        _lib.stream_for(self.table)), "adam_step_clipped")
            return
        if self.guarded:
            _lib.check(_lib.get().lbc_adam_step_guarded(_lib.ptr(self.table), self.nchunks, self.lr, self.betas[0], self.betas[1], self.eps,
                                                        self.weight_decay, _lib.ptr(self.record), _lib.stream_for(self.table)), "adam_step_guarded")
            return
        self._step_count += 1
        _lib.check(_lib.get().lbc_adam_step(_lib.ptr(self.table), self.nchunks, self.lr, self.betas[0], self.betas[1], self.eps,
                                            self.weight_decay, self._step_count, _lib.stream_for(self.table)), "adam_step")

    def _read_record(self):
        head = self.record[:ctypes.sizeof(self._State)]
        return self._State.from_buffer_copy(head.cpu().numpy().tobytes())       # (the copy waits for the steps in flight)

    def _write_record(self, **counters):
        """read-modify-write of the header: sets the counters that are passed (step, skipped_total, skipped_in_a_row, clipped_total,
        ema_updates -- the latter two only where the record has them) and keeps the rest, telemetry of the last clean step included"""
        rec = self._read_record()
        if self.recipe and rec.step == 0:
            # A record that has not applied a step holds no rate: NaN marks "not computed since the step count was set from outside" (a
            # resume), which lr_stats() reports as None until the next clean step writes the schedule's value at that count
            rec.lr = rec.decay_factor = float("nan")
        for name, value in counters.items():
            assert hasattr(type(rec), name), "%s has no %s" % (type(rec).__name__, name)
            setattr(rec, name, int(value))
        # the coefficients are zeroed: the bookkeeping kernel derives them from `step` before the next applied update reads them
        rec.bad = rec.scan_flag = 0
        rec.lr_over_bc1 = rec.inv_bc2_sqrt = 0.0
        self.record[:ctypes.sizeof(rec)].copy_(torch.frombuffer(bytearray(bytes(rec)), dtype=torch.uint8))

    @property
    def step_count(self):
        """number of applied updates (guarded: read from the device record -- a sync)"""
        return int(self._read_record().step) if self.guarded else self._step_count

    @step_count.setter
    def step_count(self, value):
        if self.guarded:
            self._write_record(step=value)
        else:
            self._step_count = int(value)

    def skipped(self):
        """(steps skipped in total, steps skipped since the last applied one); (0, 0) without the guard.  A sync when guarded."""
        if not self.guarded:
            return (0, 0)
        r = self._read_record()
        return (int(r.skipped_total), int(r.skipped_in_a_row))

    def set_skipped(self, total, in_a_row):
        if self.guarded:
            self._write_record(skipped_total=total, skipped_in_a_row=in_a_row)

    def grad_stats(self):
        """{"grad_norm", "clip_coef", "clipped_total"} of the clipped mode: global L2 norm of the gradients (before clipping) and the
        coefficient of the last applied step, number of applied steps that were clipped.  Reads the device record: a sync, for logging
        and checkpoints only.  Without max_grad_norm the optimizer measures nothing: None / 1.0 / 0."""
        if not self.clipped:
            return {"grad_norm": None, "clip_coef": 1.0, "clipped_total": 0}
        r = self._read_record()
        return {"grad_norm": float(r.grad_norm), "clip_coef": float(r.clip_coef), "clipped_total": int(r.clipped_total)}

    def set_clipped(self, total):
        if self.clipped:
            self._write_record(clipped_total=total)

    def lr_stats(self):
        """{"lr", "ema_updates"}: the rate the schedule gave the last applied step and the number of applied steps that moved the average.
        lr is None while this record has not applied a step itself: before the first one, and after load_state_dict / a step count set by
        the host until the next clean step (the kernel derives the rate from the step count then; nothing is restored).  Reads the device
        record: a sync.  Without the recipe path: the constant rate and 0."""
        if not self.recipe:
            return {"lr": float(self.lr), "ema_updates": 0}
        r = self._read_record()
        return {"lr": float(r.lr) if r.step > 0 and r.lr == r.lr else None, "ema_updates": int(r.ema_updates)}

    def set_ema_updates(self, total):
        if self.recipe:
            self._write_record(ema_updates=total)

    def ema_of(self, name):
        """the moving average of `name` as a view of `ema` in the parameter's logical shape"""
        if self.ema is None:
            raise RuntimeError("FusedAdam.ema_of: this optimizer keeps no average (ema_decay=None)")
        p = self._keep[0][name].data
        off, n = self.offsets[name]
        return torch.as_strided(self.ema[off:off + n], p.shape, p.stride())

    def state_of(self, name):
        off, n = self.offsets[name]
        return self.exp_avg[off:off + n], self.exp_avg_sq[off:off + n]

    # ---- torch.optim.Adam's state_dict format ------------------------------------------------
    def _logical(self, name):
        """the two moments of `name` as views in the parameter's logical shape (the flat buffers are in its physical order)"""
        p = self._keep[0][name].data
        m, v = self.state_of(name)
        return torch.as_strided(m, p.shape, p.stride()), torch.as_strided(v, p.shape, p.stride())

    def state_dict(self):
        """{"state": {i: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups": [...]} as torch.optim.Adam.state_dict() writes it: i counts
        named_parameters(); a parameter that is never stepped (conv.fc.* has no gradient) has no entry, and before the first applied
        step nobody has one -- exactly what torch keeps for never-stepped parameters.  Tensors are CPU copies."""
        step = self.step_count
        state = {}
        if step > 0:
            for i, n in enumerate(self.all_names):
                if n in self.offsets:
                    m, v = self._logical(n)
                    state[i] = {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m.cpu().clone(), "exp_avg_sq": v.cpu().clone()}
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": self.decoupled, "params": list(range(len(self.all_names)))}
        if self.recipe:
            group["initial_lr"] = self.lr          # (what torch's schedulers add: `lr` is the base rate, the schedule lives on the device)
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        """takes what state_dict() or a torch.optim.Adam over the same parameters (in named_parameters() order) wrote; the guard counters
        are not part of torch's format and are left alone (NativeTrainer.state_dict carries them)"""
        groups = sd["param_groups"]
        if len(groups) != 1 or list(groups[0]["params"]) != list(range(len(self.all_names))):
            raise ValueError("FusedAdam.load_state_dict: expected one parameter group over %d parameters in named_parameters() order, got %s"
                             % (len(self.all_names), [len(g["params"]) for g in groups]))
        g = groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("FusedAdam.load_state_dict: amsgrad / maximize are not implemented")
        if bool(g.get("decoupled_weight_decay")) != self.decoupled and not (self.decoupled and g["weight_decay"] == 0):     # (no decay is no decay)
            raise ValueError("FusedAdam.load_state_dict: the group has decoupled_weight_decay=%r, this optimizer was built with %r"
                             % (bool(g.get("decoupled_weight_decay")), self.decoupled) +
                             ("" if self.decoupled else " (decoupled weight decay is not implemented on this path: pass decoupled_weight_decay=True)"))
        state = sd["state"]
        steps = set()
        for i, n in enumerate(self.all_names):
            st = state.get(i)
            if n not in self.offsets:
                if st:
                    raise ValueError("FusedAdam.load_state_dict: %s carries optimizer state, but has no gradient here" % n)
                continue
            if not st:
                steps.add(0)
                continue
            p = self._keep[0][n]
            if tuple(st["exp_avg"].shape) != tuple(p.shape) or tuple(st["exp_avg_sq"].shape) != tuple(p.shape):
                raise ValueError("FusedAdam.load_state_dict: moments of %s have shape %s, the parameter %s"
                                 % (n, tuple(st["exp_avg"].shape), tuple(p.shape)))
            steps.add(int(st["step"]))
        if len(steps) > 1:
            raise ValueError("FusedAdam.load_state_dict: the parameters carry different step counts %s; this optimizer keeps one" % sorted(steps))
        step = steps.pop() if steps else 0
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        if step > 0:
            for i, n in enumerate(self.all_names):
                if n in self.offsets:
                    m, v = self._logical(n)
                    m.copy_(state[i]["exp_avg"])            # (copy_ maps logical indices: any memory format on the other side)
                    v.copy_(state[i]["exp_avg_sq"])
        # (a torch scheduler leaves the rate of the moment in "lr" and the base rate in "initial_lr"; here the schedule lives on the device)
        lr = g.get("initial_lr", g["lr"]) if self.recipe else g["lr"]
        self.lr, self.betas, self.eps, self.weight_decay = lr, tuple(g["betas"]), g["eps"], g["weight_decay"]
        self.step_count = step
