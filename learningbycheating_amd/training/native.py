"""The LbC training step on the native executor, without autograd bookkeeping:
    teacher forward (eval) -> student forward (train) -> loss kernel -> staged backward
    (+ bucketed RCCL all-reduce) -> fused Adam
= reference training/train_image_phase1.py:174-205 (phase 1), train_image_phase0.py:163-189
(phase 0) and train_birdview.py:116-128 (bird-view behaviour cloning)."""
import contextlib
import ctypes

import torch

from .. import _lib
from ..engine import PolicyEngine
from ..optim import FusedAdam, LRSchedule
from ..parallel import StageAllReducer, stage_ranges

CAMERA = dict(w=384.0, h=160.0, fov=90.0, world_y=1.4, fixed_offset=4.0, pixels_per_meter=5.0, crop_size=192.0)


def camera_struct(**kw):
    c = dict(CAMERA)
    c.update(kw)
    return _lib.Camera(c["w"], c["h"], c["fov"], c["world_y"], c["fixed_offset"], c["pixels_per_meter"], c["crop_size"])


class NativeTrainer:
    """phase: 1 (student vs teacher, all branches, map space), 0 (student vs teacher, selected branch,
    image space), 'birdview' (privileged agent vs ground-truth waypoints), 'l1_all' (all branches vs
    given normalised targets; used to warm-start synthetic benchmarks below the horizon).

    skip_nonfinite=True: the optimizer scans the (all-reduced) gradients on the device and skips the update of a step that holds a NaN
    or an infinity -- the phase-1 / phase-2 loss has a 1 / y pole on the horizon row -- without a host round trip.  What a skipped step
    leaves behind: parameters, both Adam moments and Adam's step count bit-identical to before the step; the BatchNorm running
    statistics and counters HAVE advanced, because the forward wrote them before the loss existed (what a `continue` after the forward
    would do in the reference loop).  The scan sits behind StageAllReducer.wait(): non-finite values survive the sum and the bf16
    wire, every rank reads the same reduced bytes, so every rank takes the same decision with no extra collective.
    `skipped()` -> (total, in a row) reads the device counters (a sync: call it where the loop syncs anyway).

    max_grad_norm=X (a number; implies the guard): the same device pass also measures the global L2 norm of the (all-reduced) gradients,
    and the update applies torch.nn.utils.clip_grad_norm_'s coefficient min(1, X / (norm + 1e-6)); X = 0 measures without clipping.
    It sits where the guarded step sits, behind StageAllReducer.wait(): every rank sums the same reduced bytes in the same fixed order,
    so every rank derives the same coefficient, bit for bit, with no extra collective.  The gradient buffer is not written: `eng.grad_views`
    keep the UNCLIPPED values.  `grad_stats()` -> {"grad_norm", "clip_coef", "clipped_total"} reads the device record (a sync).

    accumulate=K (default 1: exactly the path above, nothing allocated, nothing launched): gradient accumulation over K micro-batches,
    what K calls of loss.backward() before one optimizer.step() would do in the reference loop.  Every `step(update=True)` is one
    micro-step of a window of K: its loss gradient is scaled by 1 / (n * world * K), and right behind every backward stage that stage's
    range of the gradient buffer is added into `accum_flat` (csrc/grad_accum.hip; the first micro-step of a window stores instead of
    adding and never reads the buffer).  Only the LAST micro-step launches the stage all-reduces -- over the accumulation buffer, still
    overlapped with the rest of that backward -- and runs the optimizer: K micro-batches cost one set of six bucket all-reduces and one
    Adam launch chain.  The optimizer and the reducer are built over `accum_flat` / `accum_views` (the layout of `eng.grad_flat` /
    `eng.grad_views`, pads included), so guard and clipping need no new pass: a NaN or an infinity of any micro-batch survives the sum and
    the scan of the accumulated buffer skips the whole update; `grad_norm` and `clip_coef` are those of the ACCUMULATED gradient.
    `eng.grad_views` keep the last micro-batch's values (scaled by 1 / K, and, as above, unclipped).  BatchNorm normalises every
    micro-batch with its own statistics and advances its running statistics K times per update (as torch does): K x batch is the
    optimizer's batch, not BatchNorm's.  `accum_index` (0 .. K - 1) is the position of the next micro-step; `reset_accumulation()`
    abandons an open window; `step(update=False)` never touches the window.

    lr_schedule=... / weight_decay=X / ema_decay=D (any of them implies the guard and the norm measurement: FusedAdam's recipe path,
    csrc/adam.hip).  lr_schedule (an optim.LRSchedule or a dict of its fields) makes `lr` the base rate of a schedule that the
    optimizer's bookkeeping thread evaluates at Adam's own step count: a skipped step does not advance it, with accumulate=K it advances
    once per window, and no step syncs.  weight_decay is DECOUPLED (torch.optim.AdamW; every parameter, BatchNorm and biases included,
    as AdamW with one group).  ema_decay keeps an exponential moving average of the student's parameters (`opt.ema`), updated inside
    the optimizer's update launch and left alone by a skipped step; BatchNorm buffers are not averaged.  `lr_stats()` ->
    {"lr", "ema_updates"} reads the record (a sync); `ema_state_dict()` is the student's state_dict with the averaged parameters;
    `with trainer.ema_weights():` runs on them.  Under data parallelism the ranks agree bit for bit: lr is a function of the record's
    step, the average a function of identical updated parameters.

    step(..., metrics=m) (training/metrics.py WaypointMetrics; default None: the launches of a step are exactly what they were): right
    behind the loss launch, on its stream, the step adds this batch's waypoint errors in metres into m's device record -- from the
    tensors the loss just read and the per-sample loss it wrote (phase 1 / 'l1_all': all four branches, the commanded rows picked out
    on the device; phase 0 / bird-view: the selected branch).  One small launch that only reads: it works for updating and
    non-updating steps, in train and eval mode, and never syncs.  `make_metrics()` builds an object that fits this trainer's phase;
    one whose frame (or, for bird-view, target scale / shift) does not fit is refused with ValueError before anything is launched.

    step(..., teacher_out=(sel, all)) (phases 0 and 1): the frozen teacher's waypoints, computed before -- per frame of the dataset by
    ResidentLoader's teacher cache -- take the place of the teacher's forward: nothing of the teacher is launched and the side stream
    is not touched.  teacher=None in phase 0 / 1 builds a trainer without a teacher engine (no workspace, no side stream) whose every
    step needs teacher_out; birdview= and teacher_out= together, or a teacher_out of the wrong shape, dtype or device, are refused with
    ValueError before anything is launched.

    step(..., visuals=v) (training/visuals.py PanelRenderer; default None: the launches of a step are exactly what they were): right
    behind the loss launch (and the metrics launch, if there is one), on their stream, one more launch draws this batch's panels --
    camera frame, coloured bird-view, the teacher's waypoints in blue, the student's in red, command and per-sample loss as text -- into
    v's device image.  It only reads what the loss read and wrote, and nothing is read back: `v.image()` is the copy.  `make_visuals()`
    builds a renderer that fits this trainer's phase; one of another mode is refused with ValueError before anything is launched.
    With teacher_out= there is no bird-view on the device: the canvas is background and dots.

    state_dict() / load_state_dict(): everything the trainer owns that a continued run needs -- see there."""

    def __init__(self, student, teacher, batch, image_shape, device, phase=1, lr=1e-4, world_size=1, group=None, camera=None, grad_dtype=None,
                 sync_bn=False, teacher_shape=(7, 192, 192), skip_nonfinite=False, max_grad_norm=None, accumulate=1, lr_schedule=None, weight_decay=0.0,
                 ema_decay=None):
        self.student, self.teacher, self.phase, self.batch, self.world = student, teacher, phase, batch, world_size
        self.device = device
        if int(accumulate) != accumulate or int(accumulate) < 1:
            raise ValueError("NativeTrainer: accumulate must be a positive integer, got %r" % (accumulate,))
        self.accumulate = int(accumulate)
        self.accum_index = 0
        self.accum_flat, self.accum_views = None, None
        student.train()
        self.eng = student.engine((batch,) + tuple(image_shape), device, max_batch=batch, with_grads=True)
        self.teng = None
        if teacher is not None:
            teacher.eval()
            self.teng = teacher.engine((batch,) + tuple(teacher_shape), device, max_batch=batch, with_grads=False)
            # the privileged teacher is frozen (train_image_phase1.py:244-248: loaded, eval(), never stepped): its bf16 weight copies and
            # folded BatchNorm affines are derived on the first forward only
            self.teng.set_frozen(True)
            self._teacher_versions = self._versions(teacher)
        self.cam = camera or camera_struct()
        self.max_grad_norm = max_grad_norm
        self.lr_schedule = None if lr_schedule is None else LRSchedule.of(lr_schedule)
        self.weight_decay = float(weight_decay)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        if self.weight_decay < 0 or self.weight_decay != self.weight_decay:
            raise ValueError("NativeTrainer: weight_decay must be a non-negative number, got %r" % (weight_decay,))
        self.recipe = self.lr_schedule is not None or self.weight_decay != 0.0 or self.ema_decay is not None
        self.skip_nonfinite = bool(skip_nonfinite) or max_grad_norm is not None or self.recipe
        self._in_ema_weights = False
        grad_flat, grad_views = self.eng.grad_flat, self.eng.grad_views
        if self.accumulate > 1:
            # the sum of a window's micro-batch gradients: the layout of the executor's flat gradient buffer (pads included, zero like
            # its own), the same strided views; optimizer and reducer read THIS buffer
            self.accum_flat = torch.zeros_like(self.eng.grad_flat)
            self.accum_views = {n: torch.as_strided(self.accum_flat, g.shape, g.stride(), g.storage_offset()) for n, g in self.eng.grad_views.items()}
            self._accum_ranges = stage_ranges(self.eng.grad_spans)
            grad_flat, grad_views = self.accum_flat, self.accum_views
        recipe = {}
        if self.recipe:
            recipe = dict(schedule=self.lr_schedule or LRSchedule(), weight_decay=self.weight_decay, decoupled_weight_decay=self.weight_decay != 0.0,
                          ema_decay=self.ema_decay)
        self.opt = FusedAdam(list(student.named_parameters()), grad_views, lr=lr, guarded=self.skip_nonfinite,
                             max_grad_norm=max_grad_norm, **recipe)
        self.reducer = StageAllReducer(grad_flat, self.eng.grad_spans, group, grad_dtype=grad_dtype)   # grad_dtype: see parallel.py
        self.sync_bn = bool(sync_bn and world_size > 1)
        if sync_bn and world_size > 1:
            # BatchNorm over the global batch (not in the reference: it trains 256 images on one device, which is what this
            # restores for 8 x 32).  On a GPU the reductions run on the library's own RCCL communicator (`group` only carries
            # its id); the torch.distributed transport of the CPU emulator gets a process group of its own
            import torch.distributed as dist
            rccl = torch.device(device).type == "cuda" and dist.get_backend(group) == "nccl"
            self.eng.set_sync_bn(group if (rccl or group is not None) else dist.new_group())
        self.loss = torch.zeros(batch, dtype=torch.float32, device=device)
        self.dpred_all = torch.zeros((batch, 4, 5, 2), dtype=torch.float32, device=device)
        self.dpred_sel = torch.zeros((batch, 5, 2), dtype=torch.float32, device=device)
        self.nstages = PolicyEngine.num_stages()
        # the frozen teacher's forward is independent of the student's: it runs on a side stream, which fills the GPU at
        # small per-GPU batches (both networks launch kernels far smaller than the chip there)
        self.side = torch.cuda.Stream(device=device) if (teacher is not None and torch.device(device).type == "cuda") else None
        self.overlap_teacher = True      # False: one stream (per-kernel timing of an instrumented step stays meaningful)

    @staticmethod
    def _versions(module):
        """torch's in-place version counters of a module's tensors: an optimizer step, an EMA update or a `p.copy_()` on the frozen teacher
        moves them (writes through `p.data` do not: after those call `trainer.teng.invalidate()`)"""
        return tuple(t._version for t in list(module.parameters()) + list(module.buffers()))

    def _loss(self, kind, pred, target, rows, dpred):
        n = pred.shape[0]
        _lib.check(_lib.get().lbc_loss(kind, ctypes.byref(self.cam), _lib.ptr(pred), _lib.ptr(target), n, rows,
                                       1.0 / (n * self.world * self.accumulate), _lib.ptr(self.loss), _lib.ptr(dpred), _lib.stream_for(pred)), "loss")

    def _metrics_frame(self):
        """(pred_frame, target_scale, target_shift) of a WaypointMetrics that fits this trainer's loss"""
        if self.phase == "birdview":
            return "map", 1.0 / (0.5 * float(self.cam.crop_size)), -1.0       # lbc_loss kind 2: ground truth in crop pixels
        return "camera", 1.0, 0.0

    def make_metrics(self, thresholds=(0.5, 1.0, 2.0)):
        from .metrics import WaypointMetrics
        frame, scale, shift = self._metrics_frame()
        return WaypointMetrics(self.device, camera=self.cam, pred_frame=frame, thresholds=thresholds, target_scale=scale, target_shift=shift)

    def _check_metrics(self, metrics):
        frame, scale, shift = self._metrics_frame()
        if metrics.pred_frame != frame:
            raise ValueError("NativeTrainer.step: phase %r predicts in the %s frame, the metrics object was built for the %s frame"
                             % (self.phase, frame, metrics.pred_frame))
        if (metrics.target_scale, metrics.target_shift) != (scale, shift):
            raise ValueError("NativeTrainer.step: phase %r compares against target * %r + %r, the metrics object was built for target * %r + %r"
                             % (self.phase, scale, shift, metrics.target_scale, metrics.target_shift))

    def _visuals_mode(self):
        from .visuals import MODES
        if self.phase not in MODES:
            raise ValueError("NativeTrainer: phase %r has no panels to draw (phases 0, 1 and 'birdview' have)" % (self.phase,))
        return MODES[self.phase]

    def make_visuals(self, size=None, ncols=4):
        """a training/visuals.py PanelRenderer that fits this trainer's phase; size / sort default to the reference's: 32 panels sorted by
        loss in phase 0, 8 unsorted in phase 1, 16 sorted for the bird-view"""
        from .visuals import PanelRenderer
        return PanelRenderer(self.device, self.cam, self._visuals_mode(), size=size, ncols=ncols)

    def _check_teacher_out(self, teacher_out, birdview, n, device):
        """the refusals of step(teacher_out=...), before anything is launched -> (sel, all), the one this phase's loss reads packed"""
        if self.phase not in (0, 1):
            raise ValueError("NativeTrainer.step: teacher_out is for phases 0 and 1, this trainer runs phase %r" % (self.phase,))
        if birdview is not None:
            raise ValueError("NativeTrainer.step: birdview= and teacher_out= together: the teacher's waypoints are either computed or given")
        try:
            sel, every = teacher_out
        except (TypeError, ValueError):
            raise ValueError("NativeTrainer.step: teacher_out must be a pair (sel, all)") from None
        for name, t, shape in (("sel", sel, (n, 5, 2)), ("all", every, (n, 4, 5, 2))):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape or t.device != device:
                raise ValueError("NativeTrainer.step: teacher_out.%s must be a float32 tensor of shape %s on %s, got %s"
                                 % (name, shape, device, "%s %s on %s" % (t.dtype, tuple(t.shape), t.device) if isinstance(t, torch.Tensor)
                                    else type(t).__name__))
        # (the loss takes a raw pointer to dense rows: the views a loader's teacher cache hands out have the cached row's pitch)
        return (sel, every.contiguous()) if self.phase == 1 else (sel.contiguous(), every)

    def step(self, x, speed, command, birdview=None, target=None, update=True, train_mode=True, on_forward=None, metrics=None, teacher_out=None,
             visuals=None):
        """x: student input, float32 (N,C,H,W) in [0,1] or the dataset's uint8 (N,H,W,C) frames; command one-hot (N,4);
        returns the per-sample loss (device tensor).  update=False: forward + loss only.  train_mode=False: the student runs
        in eval mode (running statistics, no buffer update) -- the reference's validation pass (train_image_phase1.py:162-165,256).
        on_forward (parity tests): called with the trainer after the student's forward, before the loss and the backward.
        teacher_out=(sel, all) (phases 0 and 1, instead of birdview=): the frozen teacher's waypoints for this batch, float32 (N,5,2)
        and (N,4,5,2), computed earlier (ResidentLoader's teacher cache).  No teacher forward is launched and no side stream is
        involved; loss, metrics and `last_teacher` see these tensors where they see the forward's.  A trainer built with teacher=None
        has no teacher engine and takes every phase-0 / phase-1 step this way."""
        if not train_mode and update:
            raise ValueError("an eval-mode step cannot update (backward through running-statistics BatchNorm is not implemented)")
        if update and self._in_ema_weights:
            raise RuntimeError("NativeTrainer.step: an updating step inside ema_weights() would train the average")
        if metrics is not None:
            self._check_metrics(metrics)
        if visuals is not None and visuals.mode != self._visuals_mode():
            raise ValueError("NativeTrainer.step: phase %r draws panels of mode %d, the renderer was built for mode %d"
                             % (self.phase, self._visuals_mode(), visuals.mode))
        n = x.shape[0]
        if teacher_out is not None:
            teacher_out = self._check_teacher_out(teacher_out, birdview, n, x.device)
        elif self.phase in (0, 1) and self.teng is None:
            raise ValueError("NativeTrainer.step: this trainer was built without a teacher (teacher=None): every step needs teacher_out=(sel, all)")
        # the executor takes raw pointers to dense tensors; a permuted / sliced view is packed first (the reference's
        # nn.Module accepts any strides)
        x, speed, command = x.contiguous(), speed.contiguous(), command.contiguous()
        if birdview is not None:
            birdview = birdview.contiguous()
        overlapped = False                                       # the teacher's forward runs on the side stream in this step
        if teacher_out is not None:
            t_sel, t_all = self.last_teacher = teacher_out
        elif self.phase in (0, 1):
            if not getattr(self.teng, "_frozen", False):        # (somebody ran the teacher through its module API since: the promise is ours again)
                self.teng.set_frozen(True)
            v = self._versions(self.teacher)
            if v != self._teacher_versions:                     # the "frozen" teacher was written in place: derive its weight copies again
                self.teng.invalidate()
                self._teacher_versions = v
            overlapped = self.side is not None and self.overlap_teacher
            if overlapped:
                main = torch.cuda.current_stream(self.device)
                self.side.wait_stream(main)                      # inputs (and last step's use of the teacher outputs) are ordered before
                with torch.cuda.stream(self.side):
                    t_sel, t_all = self.teng.forward(birdview, speed, command, False)
                t_sel.record_stream(main); t_all.record_stream(main)
            else:
                t_sel, t_all = self.teng.forward(birdview, speed, command, False)
            self.last_teacher = (t_sel, t_all)
        p_sel, p_all = self.eng.forward(x, speed, command, bool(train_mode))
        if overlapped:
            torch.cuda.current_stream(self.device).wait_stream(self.side)      # the loss reads the teacher's waypoints
        self.last_pred = (p_sel, p_all)
        if on_forward is not None:
            on_forward(self)
        d_sel = d_all = None
        if self.phase == 1:
            self._loss(1, p_all, t_all, 20, self.dpred_all); d_all = self.dpred_all[:n]
        elif self.phase == 0:
            self._loss(0, p_sel, t_sel, 5, self.dpred_sel); d_sel = self.dpred_sel[:n]
        elif self.phase == "birdview":
            self._loss(2, p_sel, target, 5, self.dpred_sel); d_sel = self.dpred_sel[:n]
        elif self.phase == "l1_all":
            self._loss(3, p_all, target, 20, self.dpred_all); d_all = self.dpred_all[:n]
        else:
            raise ValueError(self.phase)
        if metrics is not None:
            # the tensors the loss just read, the per-sample loss it just wrote, on its stream; the kernel only reads them
            if self.phase in (1, "l1_all"):
                metrics.update(p_all, t_all if self.phase == 1 else target, command, self.loss[:n])
            else:
                metrics.update(p_sel, t_sel if self.phase == 0 else target, command, self.loss[:n])
        if visuals is not None:
            # one more launch that only reads, behind the loss (and the metrics) on their stream: the frames and the waypoints the loss
            # just read, the per-sample loss it just wrote.  With teacher_out= there is no bird-view: background and dots
            if self.phase == "birdview":
                visuals.render(None, x, p_sel, target, command, self.loss[:n])
            elif self.phase == 1:
                visuals.render(x, birdview, p_all, t_all, command, self.loss[:n])
            else:
                visuals.render(x, birdview, p_sel, t_sel, command, self.loss[:n])
        if update and self.accumulate > 1:
            self._accumulating_backward(d_sel, d_all)
        elif update:
            for st in range(self.nstages):
                self.eng.backward(d_sel, d_all, st)
                self.reducer.launch(st)
                if self.sync_bn:
                    # two communicators (the buckets' and the BatchNorm rows') must meet in ONE order on every rank: kernels of two
                    # RCCL communicators that become resident in different orders on two devices can wait for each other forever.
                    # With synchronized BatchNorm the next stage's rows therefore queue behind this stage's bucket (no overlap of the
                    # bucket with the backward in this mode; local BatchNorm -- the default -- has a single communicator and keeps it)
                    self.reducer.fence()
            self.reducer.wait()
            self.opt.step()
        return self.loss[:n]

    def _accumulating_backward(self, d_sel, d_all):
        """micro-step `accum_index` of a window of `accumulate`: every backward stage is followed by the accumulation of its range; the
        last micro-step also launches the stage's bucket (over the accumulation buffer) behind it, then waits and runs the optimizer"""
        lib, first, last = _lib.get(), int(self.accum_index == 0), self.accum_index == self.accumulate - 1
        g, acc = self.eng.grad_flat, self.accum_flat
        for st in range(self.nstages):
            self.eng.backward(d_sel, d_all, st)
            lo, hi = self._accum_ranges[st]
            _lib.check(lib.lbc_grad_accumulate(ctypes.c_void_p(g.data_ptr() + 4 * lo), ctypes.c_void_p(acc.data_ptr() + 4 * lo), hi - lo, first,
                                               _lib.stream_for(g)), "grad_accumulate")
            if last:
                self.reducer.launch(st)
                if self.sync_bn:
                    self.reducer.fence()        # (the one-order rule between the two communicators: see step())
        if last:
            self.reducer.wait()
            self.opt.step()
            self.accum_index = 0
        else:
            self.accum_index += 1

    def reset_accumulation(self):
        """abandon an open window (the end of an epoch, a loader that ran dry): -> the number of micro-batches dropped.  Nothing is
        launched: the next window's first micro-step overwrites the accumulation buffer without reading it.  Parameters, moments and
        the optimizer's counters are untouched; the BatchNorm running statistics keep what the dropped forwards wrote."""
        dropped, self.accum_index = self.accum_index, 0
        return dropped

    # ---- resumable state ---------------------------------------------------------------------
    def skipped(self):
        return self.opt.skipped()

    def grad_stats(self):
        return self.opt.grad_stats()

    def lr_stats(self):
        return self.opt.lr_stats()

    # ---- the averaged weights ----------------------------------------------------------------
    def ema_state_dict(self):
        """the student's state_dict() (same keys, devices and memory formats, so it loads wherever that does) with every trained parameter
        replaced by its moving average; BatchNorm buffers and parameters without a gradient are the student's own.  Copies; a sync."""
        if self.opt.ema is None:
            raise RuntimeError("NativeTrainer.ema_state_dict: this trainer keeps no average (ema_decay=None)")
        sd = {k: v.detach().clone() for k, v in self.student.state_dict().items()}
        for n in self.opt.names:
            sd[n].copy_(self.opt.ema_of(n))
        return sd

    def _exchange_ema(self):
        params = dict(self.student.named_parameters())
        for n in self.opt.names:
            p, e = params[n].data, self.opt.ema_of(n)
            tmp = p.clone()
            p.copy_(e)
            e.copy_(tmp)
        self.eng.invalidate()              # (written through .data: the engine derives its weight copies again)

    @contextlib.contextmanager
    def ema_weights(self):
        """inside the block the student's parameters ARE the averaged weights and `opt.ema` holds the trained ones: an exchange in
        place, nothing allocated beyond one tensor at a time; the engine's derived weight copies are invalidated on entry and on exit.
        For `step(update=False)` (the validation pass); an updating step inside is refused, and so is opening it inside an accumulation
        window."""
        if self.opt.ema is None:
            raise RuntimeError("NativeTrainer.ema_weights: this trainer keeps no average (ema_decay=None)")
        if self.accum_index != 0:
            raise RuntimeError("NativeTrainer.ema_weights: an accumulation window is open (%d of %d micro-batches summed)"
                               % (self.accum_index, self.accumulate))
        if self._in_ema_weights:
            raise RuntimeError("NativeTrainer.ema_weights: already inside")
        self._exchange_ema()
        self._in_ema_weights = True
        try:
            yield self
        finally:
            self._in_ema_weights = False
            self._exchange_ema()

    def _recipe_entry(self):
        return {"schedule": None if self.lr_schedule is None else self.lr_schedule.as_dict(), "weight_decay": self.weight_decay,
                "ema_decay": self.ema_decay}

    def _layout(self):
        return [[n, list(p.shape)] for n, p in self.student.named_parameters()]

    def state_dict(self):
        """student state_dict (parameters + BatchNorm buffers, CPU copies), the optimizer in torch.optim.Adam's format, the guard's
        counters (with the number of clipped steps), and what the state was produced under (phase, parameter layout, precision, world
        size, micro-batches per update).  The frozen teacher is not part of it: the scripts load it from its own checkpoint.  Syncs the
        device.  A half-summed accumulation window is not part of the state: inside an open window (accum_index != 0) this raises
        RuntimeError -- save at a window boundary, or call reset_accumulation() first."""
        if self.accum_index != 0:
            raise RuntimeError("NativeTrainer.state_dict: an accumulation window is open (%d of %d micro-batches summed); save at a window "
                               "boundary or call reset_accumulation() first" % (self.accum_index, self.accumulate))
        if self._in_ema_weights:
            raise RuntimeError("NativeTrainer.state_dict: inside ema_weights() the parameters and the average are exchanged; leave the block first")
        total, row = self.opt.skipped()
        sd = {"format": 1, "phase": self.phase, "precision": getattr(self.student, "precision", "fp32"), "world_size": int(self.world),
                "accumulate": int(self.accumulate), "layout": self._layout(),
                "student": {k: v.detach().cpu().clone() for k, v in self.student.state_dict().items()},
                "optimizer": self.opt.state_dict(),
                "guard": {"enabled": self.skip_nonfinite, "skipped_total": total, "skipped_in_a_row": row,
                          "clipped_total": self.opt.grad_stats()["clipped_total"]}}
        if self.recipe:
            # what the optimizer's torch-format sidecar cannot carry: the schedule, the decay, the average (CPU tensors by parameter name,
            # logical shapes) and the number of its updates
            sd["recipe"] = self._recipe_entry()
            sd["guard"]["ema_updates"] = self.opt.lr_stats()["ema_updates"]
            if self.opt.ema is not None:
                sd["ema"] = {n: self.opt.ema_of(n).detach().cpu().clone() for n in self.opt.names}
        return sd

    def load_state_dict(self, sd):
        """the inverse; refuses a state of another phase or parameter layout (ValueError), accepts another world size, precision,
        number of micro-batches per update, schedule, weight decay or use of the moving average and says so (returned notes, also logged):
        schedule, decay and ema_decay are always THIS trainer's arguments, never the state's.  The guard setting need not match: counters are
        restored where this trainer has them.  Parameters and buffers are written in place, and the engine derives its weight copies (bf16 / split planes, folded
        BatchNorm) again."""
        import logging
        if self._in_ema_weights:
            raise RuntimeError("NativeTrainer.load_state_dict: inside ema_weights() the parameters and the average are exchanged; leave the block first")
        if sd.get("format") != 1:
            raise ValueError("NativeTrainer.load_state_dict: unknown state format %r" % (sd.get("format"),))
        if sd["phase"] != self.phase:
            raise ValueError("NativeTrainer.load_state_dict: the state was saved in phase %r, this trainer runs phase %r" % (sd["phase"], self.phase))
        if [[n, list(s)] for n, s in sd["layout"]] != self._layout():
            raise ValueError("NativeTrainer.load_state_dict: the state was saved for another parameter layout (%d tensors, this model has %d "
                             "or other names / shapes)" % (len(sd["layout"]), len(self._layout())))
        notes = []
        if int(sd["world_size"]) != int(self.world):
            notes.append("state saved under world size %d, continuing under %d" % (sd["world_size"], self.world))
        if sd["precision"] != getattr(self.student, "precision", "fp32"):
            notes.append("state saved in precision %s, continuing in %s" % (sd["precision"], getattr(self.student, "precision", "fp32")))
        if int(sd.get("accumulate", 1)) != self.accumulate:      # (a state from before the field: one micro-batch per update)
            notes.append("state saved with %d micro-batches per update, continuing with %d" % (sd.get("accumulate", 1), self.accumulate))
        neutral = {"schedule": None, "weight_decay": 0.0, "ema_decay": None}
        saved, mine = dict(neutral, **(sd.get("recipe") or {})), self._recipe_entry() if self.recipe else neutral      # (a state from before the field: none of them)
        if saved["schedule"] != mine["schedule"]:
            notes.append("state saved under the learning-rate schedule %r, continuing under %r" % (saved["schedule"], mine["schedule"]))
        # The decay is this trainer's argument, like the schedule: the optimizer group is handed on with THIS trainer's decay, so what the
        # note says is what the next step does.  What the state trained with is read off its optimizer group, the value the kernel was given
        group = sd["optimizer"]["param_groups"][0]
        saved_decay = float(group["weight_decay"]) if group.get("decoupled_weight_decay") else 0.0
        if saved_decay != mine["weight_decay"]:
            notes.append("state saved with weight decay %g, continuing with %g" % (saved_decay, mine["weight_decay"]))
        if (saved["ema_decay"] is None) != (mine["ema_decay"] is None):
            notes.append("state saved without a moving average of the weights: it starts here as a copy of the restored parameters"
                         if saved["ema_decay"] is None else "state saved with a moving average of the weights, which this trainer does not keep: dropped")
        elif saved["ema_decay"] != mine["ema_decay"]:
            notes.append("state saved with ema_decay %g, continuing with %g" % (saved["ema_decay"], mine["ema_decay"]))
        for n in notes:
            logging.getLogger(__name__).warning("NativeTrainer.load_state_dict: %s", n)
        self.accum_index = 0             # (a state is always taken at a window boundary; whatever window was open here is abandoned)
        self.student.load_state_dict(sd["student"])
        if self.recipe or group.get("decoupled_weight_decay"):
            ours = dict(group, weight_decay=self.weight_decay, decoupled_weight_decay=self.opt.decoupled)
            self.opt.load_state_dict(dict(sd["optimizer"], param_groups=[ours] + list(sd["optimizer"]["param_groups"][1:])))
        else:
            self.opt.load_state_dict(sd["optimizer"])       # (neither side knows decoupled decay: the group as it is, as always)
        g = sd.get("guard") or {}
        self.opt.set_skipped(g.get("skipped_total", 0), g.get("skipped_in_a_row", 0))
        self.opt.set_clipped(g.get("clipped_total", 0))
        if self.opt.ema is not None:
            params = dict(self.student.named_parameters())
            kept = sd.get("ema")
            for n in self.opt.names:
                self.opt.ema_of(n).copy_(kept[n] if kept is not None else params[n].data)
            self.opt.set_ema_updates(g.get("ema_updates", 0) if kept is not None else 0)
        self.eng.invalidate()
        return notes
