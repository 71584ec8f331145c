"""Waypoint error metrics in metres, accumulated on the device (csrc/metrics.hip, include/lbc_hip.h lbc_waypoint_metrics_update).

What a run could say about its network so far was `loss_mean`, a mean L1 in normalised map units over all four branches.  This is the
quantity a checkpoint is judged by: the displacement error of the COMMANDED branch's waypoints against the teacher's (or the ground
truth), in metres, per command and per horizon step, split into a lateral and a longitudinal part, with the share of waypoints
inside given tolerances.  `update()` is one small launch on the stream of the loss and reads nothing back; `result()` is the one sync."""
import ctypes
import math

import numpy as np
import torch

from .. import _lib

N_COMMANDS, N_STEPS, MAX_THRESHOLDS = 4, 5, 4

# lbc_waypoint_metrics_state as a numpy record: 248 fields of 8 bytes, [c] command, [t] horizon step, [b] branch, [k] threshold
STATE_DTYPE = np.dtype([("samples", "<i8"), ("updates", "<i8"), ("cmd_count", "<i8", (4,)),
                        ("sum_e", "<f8", (4, 5)), ("sum_e2", "<f8", (4, 5)), ("sum_abs_dx", "<f8", (4, 5)), ("sum_abs_dy", "<f8", (4, 5)),
                        ("max_e", "<f8", (4, 5)), ("bad", "<i8", (4, 5)), ("within", "<i8", (4, 4, 5)),
                        ("all_sum_e", "<f8", (4, 5)), ("all_bad", "<i8", (4, 5)), ("loss_sum", "<f8"), ("loss_bad", "<i8")])
STATE_WORDS = STATE_DTYPE.itemsize // 8
_MAX_FIELDS = ("max_e",)
FRAMES = {"camera": 0, "map": 1}


def merge(states):
    """records (numpy, as `state()` returns them) combined on the host in the order given: sums and counts add, maxima take the
    maximum.  The order is part of the result (floating-point sums): every caller that merges the same records in the same order
    holds the same bits."""
    states = list(states)
    if not states:
        raise ValueError("merge: no records")
    out = np.array(states[0], dtype=STATE_DTYPE, copy=True).reshape(())
    for s in states[1:]:
        s = np.asarray(s, dtype=STATE_DTYPE).reshape(())
        for name in STATE_DTYPE.names:
            out[name] = np.maximum(out[name], s[name]) if name in _MAX_FIELDS else out[name] + s[name]
    return out


def _ratio(num, den):
    return float(num) / float(den) if den > 0 else None


def summarize(state, thresholds, all_branch=None, with_loss=True):
    """a record -> the dict `WaypointMetrics.result()` returns (plain Python numbers; None where there is nothing to average)"""
    s = np.asarray(state, dtype=STATE_DTYPE).reshape(())
    count = s["cmd_count"][:, None] - s["bad"]                 # finite rows behind every cell [c][t]
    total = int(count.sum())
    out = {"samples": int(s["samples"]), "updates": int(s["updates"]),
           "ade": _ratio(s["sum_e"].sum(), total), "fde": _ratio(s["sum_e"][:, -1].sum(), count[:, -1].sum()),
           "ade_by_command": [_ratio(s["sum_e"][c].sum(), count[c].sum()) for c in range(N_COMMANDS)],
           "fde_by_command": [_ratio(s["sum_e"][c, -1], count[c, -1]) for c in range(N_COMMANDS)],
           "ade_by_step": [_ratio(s["sum_e"][:, t].sum(), count[:, t].sum()) for t in range(N_STEPS)],
           "rmse": None if total == 0 else math.sqrt(float(s["sum_e2"].sum()) / total),
           "lateral": _ratio(s["sum_abs_dx"].sum(), total), "longitudinal": _ratio(s["sum_abs_dy"].sum(), total),
           "max": float(s["max_e"].max()) if total > 0 else None,
           "within": {float(thr): _ratio(s["within"][k].sum(), total) for k, thr in enumerate(thresholds)},
           "bad_rows": int(s["bad"].sum()),
           "command_count": [int(v) for v in s["cmd_count"]]}
    fed_all = bool(s["all_sum_e"].any() or s["all_bad"].any()) if all_branch is None else bool(all_branch)
    if fed_all:
        out["all_branch_ade"] = _ratio(s["all_sum_e"].sum(), int(s["samples"]) * N_COMMANDS * N_STEPS - int(s["all_bad"].sum()))
        out["all_branch_bad_rows"] = int(s["all_bad"].sum())
    if with_loss:
        out["loss_mean"] = _ratio(s["loss_sum"], int(s["samples"]) - int(s["loss_bad"]))
        out["loss_bad"] = int(s["loss_bad"])
    return out


class WaypointMetrics:
    """device-resident waypoint metrics of one pass.

    pred_frame "camera": predictions are normalised image coordinates (the image models, phases 0 and 1) and are unprojected to the
    map frame as lbc_loss kind 1 does; "map": predictions are normalised map coordinates (the bird-view model).  The target is
    `target * target_scale + target_shift` in normalised map coordinates (the bird-view loss's ground truth in crop pixels:
    scale 1 / (crop_size / 2), shift -1).  thresholds: up to four tolerances in metres.

    update(pred, target, command, loss=None): one launch on the current stream, no sync, no allocation; pred / target (N,4,5,2) --
      the commanded rows are picked out, and the all-branch fields see everything -- or (N,5,2); command one-hot (N,4); loss (N,).
      All float32, contiguous, on this object's device.
    reset(): a device memset.  result(): reads the record (THE sync) -> plain dict.  state(): the raw record as numpy (a sync too).
    all_gather(group): every rank's record through one torch.distributed.all_gather on `group`'s backend, merged in rank order ->
      the merged record (numpy), the same bits on every rank; pass it to result()."""

    def __init__(self, device, camera=None, pred_frame="camera", thresholds=(0.5, 1.0, 2.0), target_scale=1.0, target_shift=0.0):
        if pred_frame not in FRAMES:
            raise ValueError("WaypointMetrics: pred_frame must be 'camera' or 'map', got %r" % (pred_frame,))
        thresholds = tuple(float(t) for t in thresholds)
        if len(thresholds) > MAX_THRESHOLDS or any(not (t >= 0.0) or math.isinf(t) for t in thresholds):
            raise ValueError("WaypointMetrics: at most %d thresholds, each a finite non-negative number of metres, got %r" % (MAX_THRESHOLDS, thresholds))
        self.device, self.pred_frame, self.thresholds = torch.device(device), pred_frame, thresholds
        self.target_scale, self.target_shift = float(target_scale), float(target_shift)
        if camera is None:
            from .native import camera_struct
            camera = camera_struct()
        self.camera = camera
        lib = _lib.get()
        if lib.lbc_waypoint_metrics_state_bytes() != STATE_DTYPE.itemsize:
            raise RuntimeError("WaypointMetrics: the library's record has %d bytes, this binding was written for %d"
                               % (lib.lbc_waypoint_metrics_state_bytes(), STATE_DTYPE.itemsize))
        self.record = torch.zeros(STATE_WORDS, dtype=torch.int64, device=self.device)
        self._desc = {rows: _lib.WaypointMetricsDesc(pred_frame=FRAMES[pred_frame], rows=rows, nthresholds=len(thresholds),
                                                     target_scale=self.target_scale, target_shift=self.target_shift,
                                                     thresholds_m=(ctypes.c_double * 4)(*thresholds), camera=camera) for rows in (5, 20)}
        self._fed_all = self._fed_loss = False

    def update(self, pred, target, command, loss=None):
        rows = {4: 20, 3: 5}.get(pred.dim())
        n = pred.shape[0]
        if rows is None or tuple(pred.shape[1:]) != ((4, 5, 2) if rows == 20 else (5, 2)) or target.shape != pred.shape:
            raise ValueError("WaypointMetrics.update: pred and target must both be (N,4,5,2) or (N,5,2), got %s and %s"
                             % (tuple(pred.shape), tuple(target.shape)))
        if tuple(command.shape) != (n, N_COMMANDS) or (loss is not None and tuple(loss.shape) != (n,)):
            raise ValueError("WaypointMetrics.update: command must be (N,4) and loss (N,) for N = %d" % n)
        for name, t in (("pred", pred), ("target", target), ("command", command), ("loss", loss)):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.record.device):
                raise ValueError("WaypointMetrics.update: %s must be a contiguous float32 tensor on %s" % (name, self.record.device))
        _lib.require_device(pred)
        _lib.check(_lib.get().lbc_waypoint_metrics_update(ctypes.byref(self._desc[rows]), _lib.ptr(pred), _lib.ptr(target), _lib.ptr(command),
                                                          _lib.ptr(loss), n, _lib.ptr(self.record), _lib.stream_for(pred)), "waypoint_metrics_update")
        if n:
            self._fed_all |= rows == 20
            self._fed_loss |= loss is not None

    def reset(self):
        self.record.zero_()
        self._fed_all = self._fed_loss = False

    def state(self):
        return self.record.cpu().numpy().view(STATE_DTYPE).reshape(()).copy()

    merge = staticmethod(merge)

    def all_gather(self, group=None):
        import torch.distributed as dist
        world = dist.get_world_size(group)
        parts = [torch.empty_like(self.record) for _ in range(world)]
        dist.all_gather(parts, self.record, group=group)
        return merge(p.cpu().numpy().view(STATE_DTYPE).reshape(()) for p in parts)

    def result(self, state=None):
        """state: a record to summarise instead of this object's own (all_gather()'s merge)"""
        return summarize(self.state() if state is None else state, self.thresholds, all_branch=self._fed_all, with_loss=self._fed_loss)


def log_entries(res, prefix=""):
    """a result() -> the scalars the validation pass logs: ade, fde, ade_cmd1..4 / fde_cmd1..4 (absent commands left out), lateral,
    longitudinal, within_<thr>, bad_rows (the logger puts val_ in front: val_ade, ...).  Averages over nothing are left out."""
    out = {prefix + "bad_rows": res["bad_rows"]}
    for k in ("ade", "fde", "lateral", "longitudinal"):
        if res[k] is not None:
            out[prefix + k] = res[k]
    for c in range(N_COMMANDS):
        for k in ("ade", "fde"):
            if res[k + "_by_command"][c] is not None:
                out["%s%s_cmd%d" % (prefix, k, c + 1)] = res[k + "_by_command"][c]
    for thr, share in res["within"].items():
        if share is not None:
            out["%swithin_%g" % (prefix, thr)] = share
    return out
