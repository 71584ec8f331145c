"""Waypoint error metrics in metres on the device (csrc/metrics.hip, training/metrics.py, NativeTrainer.step(metrics=), --val-metrics).

The reference has no such metric.  The yardstick is `_ref_rows` / `_ref_add` below: a float64 numpy restatement of the definition -- the
CoordConverter formula of training/train_image_phase1.py for camera-frame predictions, (v + 1) crop / 2 for map-frame ones,
target * scale + shift as a normalised map coordinate, differences / pixels_per_meter -- written from the formula, not from the
kernel.  Both sides start from the same f32 inputs and compute in double, so what separates them is double rounding (1.1e-16)
x the conditioning of the unprojection (<= ~1e3 for y in [0.1, 0.9]: 1 / yt <= 10 / (h / 2f)) x at most a few thousand addends in
another order: below 1e-10.  Sums are asserted to 1e-9 relative (10x that derived bound), maxima to 1e-12, counts exactly.

1. kernel against float64; 2. non-finite rows; 3. accumulation over launches and reset; 4. determinism (repeat on the GPU);
5. entry-point validation; 6. NativeTrainer.step(metrics=) in phases 1, 0 and bird-view; 7. two ranks over gloo; 8. the scripts.
Every kernel case runs on the emulator and, gpu-marked, on gfx950."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import WHERE, check_guard, guarded_input, on_both, repeat
from tests.test_resume_guard import _init_state, _script, _sync
from tests.test_step import _models

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the camera travels as lbc_camera, whose fields are f32: the yardstick starts from the same f32 values (world_y = 1.4 is the one field
# that f32 does not hold exactly; both sides then compute in double from 1.39999997615814208984375)
CAM = {k: float(np.float32(v)) for k, v in dict(w=384.0, h=160.0, fov=90.0, world_y=1.4, fixed_offset=4.0, pixels_per_meter=5.0, crop_size=192.0).items()}
THRESHOLDS = (0.5, 1.0, 2.0)
SUM_RTOL, MAX_RTOL = 1e-9, 1e-12
COUNTS = ("samples", "updates", "cmd_count", "bad", "within", "all_bad", "loss_bad")
SUMS = ("sum_e", "sum_e2", "sum_abs_dx", "sum_abs_dy", "all_sum_e", "loss_sum")
MAP_SCALE, MAP_SHIFT = 1.0 / (0.5 * CAM["crop_size"]), -1.0          # ground truth in crop pixels -> normalised map (the bird-view loss)


# ---- the float64 yardstick ---------------------------------------------------------------------------------------------------------
def _ref_rows(pred, target, frame, scale, shift, cam=CAM):
    """f32 arrays (..., 2) -> (dx, dy, e) in metres, float64"""
    p = np.asarray(pred, dtype=np.float32).astype(np.float64)
    t = np.asarray(target, dtype=np.float32).astype(np.float64) * scale + shift
    w, h, crop, ppm = cam["w"], cam["h"], cam["crop_size"], cam["pixels_per_meter"]
    with np.errstate(all="ignore"):
        if frame == "camera":
            f = w / (2 * np.tan(cam["fov"] * np.pi / 360))
            loc = (p + 1) * np.array([w, h]) / 2
            xt = (loc[..., 0] - w / 2) / f
            yt = (loc[..., 1] - h / 2) / f
            world_z = cam["world_y"] / yt
            world_x = world_z * xt
            px = world_x * ppm + crop / 2
            py = crop - world_z * ppm + cam["fixed_offset"] * ppm
        else:
            px, py = (p[..., 0] + 1) * crop / 2, (p[..., 1] + 1) * crop / 2
        qx, qy = (t[..., 0] + 1) * crop / 2, (t[..., 1] + 1) * crop / 2
        dx, dy = (px - qx) / ppm, (py - qy) / ppm
        return dx, dy, np.sqrt(dx * dx + dy * dy)


def _empty_ref():
    z, zi = (lambda *s: np.zeros(s, dtype=np.float64)), (lambda *s: np.zeros(s, dtype=np.int64))
    return {"samples": 0, "updates": 0, "cmd_count": zi(4), "sum_e": z(4, 5), "sum_e2": z(4, 5), "sum_abs_dx": z(4, 5), "sum_abs_dy": z(4, 5),
            "max_e": z(4, 5), "bad": zi(4, 5), "within": zi(4, 4, 5), "all_sum_e": z(4, 5), "all_bad": zi(4, 5), "loss_sum": 0.0, "loss_bad": 0}


def _ref_add(ref, pred, target, command, loss, frame, scale=1.0, shift=0.0, thresholds=THRESHOLDS):
    """one batch into the reference record (dict of numpy arrays, the record's field names)"""
    pred, target, command = (np.asarray(a, dtype=np.float32) for a in (pred, target, command))
    n = pred.shape[0]
    if n == 0:
        return ref
    cmd = np.array([int(np.flatnonzero(row)[0]) for row in command])
    dx, dy, e = _ref_rows(pred, target, frame, scale, shift)
    if pred.ndim == 4:
        fin_all = np.isfinite(e)                                                       # (N,4,5)
        ref["all_sum_e"] += np.where(fin_all, e, 0.0).sum(axis=0)
        ref["all_bad"] += (~fin_all).sum(axis=0)
        pick = np.arange(n)
        dx, dy, e = dx[pick, cmd], dy[pick, cmd], e[pick, cmd]                      # (N,5)
    fin = np.isfinite(e)
    for c in range(4):
        mine = cmd == c
        ref["cmd_count"][c] += int(mine.sum())
        good = fin & mine[:, None]
        ref["sum_e"][c] += np.where(good, e, 0.0).sum(axis=0)
        ref["sum_e2"][c] += np.where(good, e * e, 0.0).sum(axis=0)
        ref["sum_abs_dx"][c] += np.where(good, np.abs(dx), 0.0).sum(axis=0)
        ref["sum_abs_dy"][c] += np.where(good, np.abs(dy), 0.0).sum(axis=0)
        ref["max_e"][c] = np.maximum(ref["max_e"][c], np.where(good, e, 0.0).max(axis=0, initial=0.0))
        ref["bad"][c] += (~fin & mine[:, None]).sum(axis=0)
        for k, thr in enumerate(thresholds):
            with np.errstate(invalid="ignore"):
                ref["within"][k, c] += (good & (e <= thr)).sum(axis=0)
    ref["samples"] += n
    ref["updates"] += 1
    if loss is not None:
        l = np.asarray(loss, dtype=np.float32).astype(np.float64)
        ref["loss_sum"] += float(l[np.isfinite(l)].sum())
        ref["loss_bad"] += int((~np.isfinite(l)).sum())
    return ref


def _assert_state(state, ref, sum_rtol=SUM_RTOL, what=""):
    for k in COUNTS:
        assert np.array_equal(np.asarray(state[k]), np.asarray(ref[k])), (what, k, state[k], ref[k])
    for k in SUMS:
        a, b = np.asarray(state[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        assert np.isfinite(a).all(), (what, k)
        err = np.abs(a - b)
        print("%s %s: worst relative difference %.3g" % (what, k, float((err / np.maximum(np.abs(b), 1e-300)).max())))
        assert (err <= sum_rtol * np.abs(b)).all(), (what, k, a, b)
    a, b = np.asarray(state["max_e"]), np.asarray(ref["max_e"])
    assert np.isfinite(a).all() and (np.abs(a - b) <= MAX_RTOL * np.abs(b)).all(), (what, "max_e", a, b)


def _assert_result(res, ref, rtol, thresholds=THRESHOLDS):
    """a result() against the summary of a reference record, written out here from the definitions"""
    count = ref["cmd_count"][:, None] - ref["bad"]
    total = count.sum()
    div = lambda a, b: None if b == 0 else float(a) / float(b)
    want = {"ade": div(ref["sum_e"].sum(), total), "fde": div(ref["sum_e"][:, 4].sum(), count[:, 4].sum()),
            "rmse": None if total == 0 else float(np.sqrt(ref["sum_e2"].sum() / total)),
            "lateral": div(ref["sum_abs_dx"].sum(), total), "longitudinal": div(ref["sum_abs_dy"].sum(), total),
            "max": None if total == 0 else float(ref["max_e"].max())}
    for c in range(4):
        want["ade_by_command/%d" % c] = div(ref["sum_e"][c].sum(), count[c].sum())
        want["fde_by_command/%d" % c] = div(ref["sum_e"][c, 4], count[c, 4])
    for t in range(5):
        want["ade_by_step/%d" % t] = div(ref["sum_e"][:, t].sum(), count[:, t].sum())
    for k, thr in enumerate(thresholds):
        want["within/%r" % float(thr)] = div(ref["within"][k].sum(), total)
    got = dict(res)
    for name in ("ade_by_command", "fde_by_command", "ade_by_step"):
        for i, v in enumerate(got.pop(name)):
            got["%s/%d" % (name, i)] = v
    for thr, v in got.pop("within").items():
        got["within/%r" % float(thr)] = v
    assert got["samples"] == ref["samples"] and got["bad_rows"] == int(ref["bad"].sum())
    for k, w in want.items():
        g = got[k]
        assert (g is None) == (w is None), (k, g, w)
        if w is not None:
            assert isinstance(g, float) and abs(g - w) <= rtol * abs(w), (k, g, w)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _draw(n, rows, frame, seed, absent=None, thresholds=THRESHOLDS):
    """f32 numpy (pred, target, command, loss).  Camera-frame predictions have y in [0.1, 0.9] (below the horizon) and x in
    [-0.9, 0.9]; all four commands occur (from n = 4 on) unless `absent` names one that never does.  Every error lies at least
    1e-6 m away from every threshold -- a sample that comes closer is drawn again -- so that `within` can be compared exactly:
    the two sides differ by ~1e-13 m at most."""
    rng = np.random.RandomState(seed)
    shape = (n, 4, 5, 2) if rows == 20 else (n, 5, 2)
    scale, shift = (MAP_SCALE, MAP_SHIFT) if frame == "map" else (1.0, 0.0)

    def sample(k):
        p = rng.uniform(-0.9, 0.9, size=(k,) + shape[1:])
        if frame == "camera":
            p[..., 1] = rng.uniform(0.1, 0.9, size=p.shape[:-1])
            t = rng.uniform(-0.9, 0.9, size=p.shape)
        else:
            t = rng.uniform(0.0, 192.0, size=p.shape)
        return p.astype(np.float32), t.astype(np.float32)
    pred, target = sample(n)
    for _ in range(20):
        e = _ref_rows(pred, target, frame, scale, shift)[2].reshape(n, -1)
        close = np.zeros(n, dtype=bool)
        for thr in thresholds:
            close |= (np.abs(e - thr) < 1e-6).any(axis=1)
        if not close.any():
            break
        pred[close], target[close] = sample(int(close.sum()))
    else:
        raise AssertionError("could not draw errors away from the thresholds")
    allowed = [c for c in range(4) if c != absent]
    cmd = np.array([allowed[i % len(allowed)] for i in range(n)])
    rng.shuffle(cmd)
    command = np.zeros((n, 4), dtype=np.float32)
    command[np.arange(n), cmd] = 1.0
    loss = rng.uniform(0.01, 1.0, size=n).astype(np.float32)
    return pred, target, command, loss


def _dev(dev, *arrays):
    """numpy -> device tensors between NaN fences"""
    return [None if a is None else guarded_input(torch.from_numpy(np.ascontiguousarray(a)).to(dev)) for a in arrays]


def _fenced_metrics(dev, frame, thresholds=THRESHOLDS, **kw):
    """a WaypointMetrics whose record lies between NaN fences; -> (metrics, fence buffer)"""
    from learningbycheating_amd.training.metrics import STATE_WORDS, WaypointMetrics
    from learningbycheating_amd.training.native import camera_struct
    if frame == "map":
        kw = dict(dict(target_scale=MAP_SCALE, target_shift=MAP_SHIFT), **kw)
    m = WaypointMetrics(dev, camera=camera_struct(**CAM), pred_frame=frame, thresholds=thresholds, **kw)
    buf = torch.full((STATE_WORDS + 512,), float("nan"), dtype=torch.float64, device=dev)
    rec = buf[256:256 + STATE_WORDS]
    rec.zero_()
    m.record = rec.view(torch.int64)
    return m, buf


def _fences_ok(dev, buf):
    from learningbycheating_amd.training.metrics import STATE_WORDS
    _sync(dev)
    check_guard(buf, STATE_WORDS)


# ---- 1. kernel against float64 --------------------------------------------------------------------------------------------------------
CASES = [(n, rows, frame) for n in (1, 3, 63, 64, 65, 255, 256, 257, 513) for rows in (5, 20) for frame in ("camera", "map")]


@pytest.mark.parametrize("case", on_both("case", CASES))
def test_kernel_matches_float64(env, case):
    dev, _ = env
    n, rows, frame = case
    pred, target, command, loss = _draw(n, rows, frame, seed=1000 + n + rows)
    if n >= 4:
        assert command.sum(axis=0).min() >= 1, "all four commands occur"
    m, buf = _fenced_metrics(dev, frame)
    m.update(*_dev(dev, pred, target, command, loss))
    _fences_ok(dev, buf)
    ref = _ref_add(_empty_ref(), pred, target, command, loss, frame, m.target_scale, m.target_shift)
    state = m.state()
    _assert_state(state, ref, what="N=%d rows=%d %s" % case)
    if rows == 5:
        assert not state["all_sum_e"].any() and not state["all_bad"].any(), "rows = 5 leaves the all-branch fields alone"
    res = m.result()
    _assert_result(res, ref, SUM_RTOL)
    assert ("all_branch_ade" in res) == (rows == 20)
    if rows == 20:
        assert abs(res["all_branch_ade"] - ref["all_sum_e"].sum() / (n * 20)) <= SUM_RTOL * res["all_branch_ade"]
    assert abs(res["loss_mean"] - float(loss.astype(np.float64).mean())) <= 1e-12 * res["loss_mean"] and res["loss_bad"] == 0


@pytest.mark.parametrize("where", WHERE)
def test_absent_command_stays_zero_and_gives_none(env, where):
    dev, _ = env
    pred, target, command, loss = _draw(65, 20, "camera", seed=7, absent=2)        # (command 3 of 1..4)
    m, buf = _fenced_metrics(dev, "camera")
    m.update(*_dev(dev, pred, target, command, None))
    _fences_ok(dev, buf)
    state = m.state()
    _assert_state(state, _ref_add(_empty_ref(), pred, target, command, None, "camera"))
    for k in ("sum_e", "sum_e2", "sum_abs_dx", "sum_abs_dy", "max_e", "bad"):
        assert not state[k][2].any(), k
    assert state["cmd_count"][2] == 0 and not state["within"][:, 2].any()
    assert state["loss_sum"] == 0.0 and state["loss_bad"] == 0, "a NULL loss leaves the loss fields alone"
    res = m.result()
    assert res["ade_by_command"][2] is None and res["fde_by_command"][2] is None
    assert all(res["ade_by_command"][c] > 0 for c in (0, 1, 3)) and "loss_mean" not in res
    empty = _fenced_metrics(dev, "camera")[0].result()
    assert empty["samples"] == 0 and empty["ade"] is None and empty["fde"] is None and empty["max"] is None and empty["within"] == {0.5: None, 1.0: None, 2.0: None}


# ---- 2. non-finite rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", on_both("case", [5, 20]))
def test_nonfinite_rows_are_counted_and_excluded(env, case):
    dev, _ = env
    rows = case
    pred, target, command, loss = _draw(70, rows, "camera", seed=11)
    cmd = command.argmax(axis=1)
    at = (lambda a, s, t: a[s, cmd[s], t]) if rows == 20 else (lambda a, s, t: a[s, t])
    at(pred, 5, 1)[1] = 0.0                    # on the horizon row: yt = 0
    at(pred, 17, 3)[0] = np.nan
    at(target, 66, 0)[1] = np.inf
    if rows == 20:                             # rows of branches that are not commanded: the all-branch fields only
        pred[9, (cmd[9] + 1) % 4, 2, 0] = np.nan
        pred[30, (cmd[30] + 2) % 4, 4, 1] = 0.0
    loss[40] = np.nan
    loss[41] = np.inf
    m, buf = _fenced_metrics(dev, "camera")
    m.update(*_dev(dev, pred, target, command, loss))
    _fences_ok(dev, buf)
    state = m.state()
    want_bad = np.zeros((4, 5), dtype=np.int64)
    for s, t in ((5, 1), (17, 3), (66, 0)):
        want_bad[cmd[s], t] += 1
    assert np.array_equal(state["bad"], want_bad) and want_bad.sum() == 3 and want_bad.max() == 1
    ref = _ref_add(_empty_ref(), pred, target, command, loss, "camera")
    _assert_state(state, ref)                  # (every sum and max_e finite, equal to numpy over the remaining rows)
    if rows == 20:
        want_all = np.zeros((4, 5), dtype=np.int64)
        for s, b, t in ((5, cmd[5], 1), (17, cmd[17], 3), (66, cmd[66], 0), (9, (cmd[9] + 1) % 4, 2), (30, (cmd[30] + 2) % 4, 4)):
            want_all[b, t] += 1
        assert np.array_equal(state["all_bad"], want_all)
    assert state["loss_bad"] == 2
    keep = np.isfinite(loss)
    assert abs(state["loss_sum"] - loss[keep].astype(np.float64).sum()) <= 1e-12 * state["loss_sum"]
    res = m.result()
    assert res["bad_rows"] == 3 and res["loss_bad"] == 2 and np.isfinite(res["loss_mean"]) and np.isfinite(res["max"])


# ---- 3. accumulation over launches, 4. determinism ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", on_both("case", [("camera", 20), ("map", 5)]))
def test_accumulation_reset_and_determinism(env, case):
    from learningbycheating_amd.training.metrics import STATE_DTYPE
    dev, _ = env
    frame, rows = case
    pred, target, command, loss = _draw(96, rows, frame, seed=21)
    whole = _dev(dev, pred, target, command, loss)
    thirds = [_dev(dev, *(a[i:i + 32] for a in (pred, target, command, loss))) for i in (0, 32, 64)]

    def three_launches():
        m, buf = _fenced_metrics(dev, frame)
        for part in thirds:
            m.update(*part)
        _fences_ok(dev, buf)
        return (m.record.clone(),)
    rec3 = repeat(dev, three_launches)[0]       # (GPU: the same sequence three times, bit-identical records)
    s3 = rec3.cpu().numpy().view(STATE_DTYPE).reshape(())
    m, buf = _fenced_metrics(dev, frame)
    m.update(*whole)
    s1 = m.state()
    assert s1["samples"] == s3["samples"] == 96 and s1["updates"] == 1 and s3["updates"] == 3
    s1["updates"] = 3
    _assert_state(s3, s1, sum_rtol=1e-12, what="three launches vs one")
    ref = _empty_ref()
    for i in (0, 32, 64):
        _ref_add(ref, pred[i:i + 32], target[i:i + 32], command[i:i + 32], loss[i:i + 32], frame, m.target_scale, m.target_shift)
    _assert_state(s3, ref)
    m.reset()
    _fences_ok(dev, buf)
    assert m.state().tobytes() == bytes(STATE_DTYPE.itemsize) and "loss_mean" not in m.result()


# ---- 5. entry-point validation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_entry_point_refusals(env, where):
    from learningbycheating_amd import _lib
    from learningbycheating_amd.training.metrics import STATE_DTYPE
    from learningbycheating_amd.training.native import camera_struct
    dev, _ = env
    lib = _lib.get()
    assert lib.lbc_waypoint_metrics_state_bytes() == STATE_DTYPE.itemsize == ctypes.sizeof(_lib.WaypointMetricsState) == 248 * 8
    pred, target, command, loss = _dev(dev, *_draw(6, 20, "camera", seed=3))
    m, buf = _fenced_metrics(dev, "camera")
    m.update(pred, target, command, loss)
    before = m.state().tobytes()

    def desc(**kw):
        d = dict(pred_frame=0, rows=20, nthresholds=3, thresholds_m=(ctypes.c_double * 4)(0.5, 1.0, 2.0), camera=camera_struct(**CAM))
        d.update(kw)
        return _lib.WaypointMetricsDesc(**d)

    def call(d, pred=pred, target=target, command=command, loss=loss, n=6, state="own"):
        state = _lib.ptr(m.record) if state == "own" else state
        return lib.lbc_waypoint_metrics_update(ctypes.byref(d) if d is not None else None, _lib.ptr(pred), _lib.ptr(target), _lib.ptr(command),
                                               _lib.ptr(loss), n, state, _lib.stream_for(m.record))
    inf, nan = float("inf"), float("nan")
    refusals = {"null state": dict(d=desc(), state=None),
                "misaligned state": dict(d=desc(), state=ctypes.c_void_p(m.record.data_ptr() + 4)),
                "null pred": dict(d=desc(), pred=None), "null target": dict(d=desc(), target=None), "null command": dict(d=desc(), command=None),
                "negative N": dict(d=desc(), n=-1), "rows 10": dict(d=desc(rows=10)), "rows 0": dict(d=desc(rows=0)),
                "pred_frame 2": dict(d=desc(pred_frame=2)), "pred_frame -1": dict(d=desc(pred_frame=-1)),
                "nthresholds 5": dict(d=desc(nthresholds=5)), "nthresholds -1": dict(d=desc(nthresholds=-1)),
                "negative threshold": dict(d=desc(thresholds_m=(ctypes.c_double * 4)(0.5, -1.0, 2.0))),
                "infinite threshold": dict(d=desc(thresholds_m=(ctypes.c_double * 4)(inf, 1.0, 2.0))),
                "NaN threshold": dict(d=desc(thresholds_m=(ctypes.c_double * 4)(0.5, 1.0, nan))),
                "struct_size 0": dict(d=desc(struct_size=0)), "struct_size + 8": dict(d=desc(struct_size=ctypes.sizeof(_lib.WaypointMetricsDesc) + 8)),
                "null descriptor": dict(d=None)}
    for what, kw in refusals.items():
        assert call(**kw) == -1, what                                          # LBC_EINVAL
        assert lib.lbc_last_error().decode() != "", what
        _sync(dev)
        assert m.state().tobytes() == before, what
    assert call(desc(), n=0) == 0 and call(desc(nthresholds=0), n=0) == 0
    _fences_ok(dev, buf)
    assert m.state().tobytes() == before, "N = 0 changes nothing"
    # a threshold beyond nthresholds is not looked at, and its counters are not touched
    assert call(desc(nthresholds=1, thresholds_m=(ctypes.c_double * 4)(0.5, nan, -3.0))) == 0
    after = m.state()
    assert after["updates"] == 2 and np.array_equal(after["within"][1:], np.frombuffer(before, dtype=STATE_DTYPE)[0]["within"][1:])
    # the Python object refuses what the kernel cannot read
    from learningbycheating_amd.training.metrics import WaypointMetrics
    with pytest.raises(ValueError):
        m.update(pred[:, 0], target, command)
    with pytest.raises(ValueError):
        m.update(pred.double(), target.double(), command)
    with pytest.raises(ValueError):
        m.update(pred, target, command[:, :3].contiguous())
    with pytest.raises(ValueError):
        WaypointMetrics(dev, pred_frame="world")
    with pytest.raises(ValueError):
        WaypointMetrics(dev, thresholds=(1.0, -1.0))
    with pytest.raises(ValueError):
        WaypointMetrics(dev, thresholds=(1, 2, 3, 4, 5))


# ---- 6. NativeTrainer.step(metrics=) -----------------------------------------------------------------------------------------------------
class _TrainerCase:
    """two trainers of one phase built from the same bits (`make()`), and seeded inputs; emulator: ResNet-18, 32 x 64, batch 3; GPU: the
    reference's sizes at batch 4.  Phases 0 and 1 start from a student warm-started below the horizon (tests/test_resume_guard._init_state)."""

    def __init__(self, dev, phase):
        self.dev, self.phase, self.small = dev, phase, torch.device(dev).type != "cuda"
        self.n = 3 if self.small else 4
        self.kind = "birdview" if phase == "birdview" else "image"
        self.hw = ((32, 64) if self.small else (160, 384)) if self.kind == "image" else ((64, 64) if self.small else (192, 192))
        self.thw = (64, 64) if self.small else (192, 192)
        if phase == "birdview":
            self.init = {"student": {k: v.detach().cpu().clone() for k, v in _models("birdview", dev, self.small, 61).state_dict().items()}}
        else:
            self.init = _init_state(dev, self.small, "fp32", self.n)
        self.frame = "map" if phase == "birdview" else "camera"
        self.scale, self.shift = (MAP_SCALE, MAP_SHIFT) if phase == "birdview" else (1.0, 0.0)

    def make(self, **keywords):
        from learningbycheating_amd.training.native import NativeTrainer
        student = _models(self.kind, self.dev, self.small, 1)
        student.load_state_dict(self.init["student"])
        teacher = None
        if self.phase != "birdview":
            teacher = _models("birdview", self.dev, self.small, 2)
            teacher.load_state_dict(self.init["teacher"])
        return NativeTrainer(student, teacher, self.n, (7 if self.kind == "birdview" else 3,) + self.hw, self.dev, phase=self.phase, lr=1e-4,
                             teacher_shape=(7,) + self.thw, **keywords)

    def inputs(self, i):
        from oracle import lbc_oracle as O
        from oracle.make_golden import seeded_inputs
        x, speed, cmd = seeded_inputs(self.kind, self.n, 100 + i, *self.hw)
        kw = {}
        if self.phase == "birdview":
            kw["target"] = (torch.rand((self.n, 5, 2), generator=torch.Generator().manual_seed(200 + i)) * 192).to(self.dev)
        else:
            kw["birdview"] = seeded_inputs("birdview", self.n, 300 + i, *self.thw)[0].to(self.dev)
        return (x.contiguous().to(self.dev), speed.to(self.dev), O.one_hot(cmd).to(self.dev)), kw

    def seen(self, tr, kw):
        """(pred, target) the loss of the last step read, as numpy"""
        _sync(self.dev)
        if self.phase == 1:
            return tr.last_pred[1].cpu().numpy(), tr.last_teacher[1].cpu().numpy()
        return tr.last_pred[0].cpu().numpy(), (kw["target"] if self.phase == "birdview" else tr.last_teacher[0]).cpu().numpy()


def _params_and_moments(tr, dev):
    _sync(dev)
    out = {"sd." + k: v.detach().cpu().clone() for k, v in tr.student.state_dict().items()}
    out["m"], out["v"] = tr.opt.exp_avg.cpu().clone(), tr.opt.exp_avg_sq.cpu().clone()
    return out


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("phase", [1, 0, "birdview"])
def test_trainer_feeds_metrics(env, where, phase):
    from learningbycheating_amd.training.metrics import WaypointMetrics
    from tests.test_model import _launch_counts
    dev, _ = env
    case = _TrainerCase(dev, phase)
    a, b = case.make(), case.make()                      # b: the twin that never sees a metrics object
    m = a.make_metrics()
    assert m.pred_frame == case.frame and (m.target_scale, m.target_shift) == (case.scale, case.shift)
    ref, losses = _empty_ref(), []
    for i in range(4):
        args, kw = case.inputs(i)
        la = a.step(*args, update=False, train_mode=False, metrics=m, **kw)
        pred, target = case.seen(a, kw)
        la = la.cpu().clone()
        _ref_add(ref, pred, target, args[2].cpu().numpy(), la.numpy(), case.frame, case.scale, case.shift)
        losses.append(la.numpy().astype(np.float64))
        lb = b.step(*args, update=False, train_mode=False, **kw)
        _sync(dev)
        assert torch.equal(la, lb.cpu()), "per-sample loss with and without metrics (step %d)" % i
        assert all(torch.equal(p.cpu(), q.cpu()) for p, q in zip(a.last_pred, b.last_pred)), "predictions with and without metrics"
    state = m.state()
    assert state["samples"] == 4 * case.n and state["updates"] == 4
    _assert_state(state, ref, what="phase %s" % (phase,))
    res = m.result()
    _assert_result(res, ref, SUM_RTOL)
    assert ("all_branch_ade" in res) == (phase == 1)
    mean = float(np.concatenate(losses).mean())
    assert abs(res["loss_mean"] - mean) <= 1e-12 * abs(mean) and res["loss_bad"] == 0
    # launches: the step without metrics launches what it always launched; with metrics, one more launch of a class of its own
    args, kw = case.inputs(4)
    plain = _launch_counts(lambda: b.step(*args, update=False, train_mode=False, **kw))
    fed = _launch_counts(lambda: a.step(*args, update=False, train_mode=False, metrics=m, **kw))
    assert "waypoint_metrics" not in plain and fed == dict(plain, waypoint_metrics=1)
    # an updating train-mode step: parameters and moments bit-identical to the twin's
    args, kw = case.inputs(5)
    la, lb = a.step(*args, metrics=m, **kw), b.step(*args, **kw)
    pa, pb = _params_and_moments(a, dev), _params_and_moments(b, dev)
    assert torch.equal(la.cpu(), lb.cpu()) and pa.keys() == pb.keys() and all(torch.equal(pa[k], pb[k]) for k in pa)
    assert a.opt.step_count == b.opt.step_count == 1 and m.state()["updates"] == 6
    # a metrics object of the other frame (or, bird-view, of another target scale) is refused before anything is launched
    wrong = [WaypointMetrics(dev, pred_frame="camera" if case.frame == "map" else "map")]
    if phase == "birdview":
        wrong.append(WaypointMetrics(dev, pred_frame="map"))
    for w in wrong:
        with pytest.raises(ValueError):
            a.step(*args, update=False, train_mode=False, metrics=w, **kw)
        assert w.state()["updates"] == 0


# ---- 7. two ranks ------------------------------------------------------------------------------------------------------------------------
def _two_rank_worker(rank, port, out):
    import torch.distributed as dist
    from tests import emu
    torch.set_num_threads(2)
    emu.activate()
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=2)
    try:
        dev = torch.device("cpu")
        data = _draw(22, 20, "camera", seed=31)
        lo, hi = (0, 12) if rank == 0 else (12, 22)
        m, buf = _fenced_metrics(dev, "camera")
        for i in range(lo, hi, 6):                            # two launches per rank, the second one partial on rank 1
            m.update(*_dev(dev, *(a[i:min(i + 6, hi)] for a in data)))
        merged = m.all_gather()
        _fences_ok(dev, buf)
        with open(out % rank, "wb") as f:
            f.write(merged.tobytes())
        with open((out % rank) + ".own", "wb") as f:
            f.write(m.state().tobytes())
    finally:
        dist.destroy_process_group()


def test_two_ranks_gather_identical_records(env, tmp_path):
    import torch.multiprocessing as mp
    from learningbycheating_amd.training.metrics import STATE_DTYPE, merge, summarize
    dev, _ = env
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "rank%d.bin")
    mp.start_processes(_two_rank_worker, args=(port, out), nprocs=2, join=True, start_method="spawn")
    raw = [open(out % r, "rb").read() for r in (0, 1)]
    assert raw[0] == raw[1] and len(raw[0]) == STATE_DTYPE.itemsize, "both ranks hold the same bytes"
    merged = np.frombuffer(raw[0], dtype=STATE_DTYPE)[0]
    own = [np.frombuffer(open((out % r) + ".own", "rb").read(), dtype=STATE_DTYPE)[0] for r in (0, 1)]
    assert merge(own).tobytes() == raw[0], "the merge is rank 0's record, then rank 1's"
    assert own[0]["samples"] == 12 and own[1]["samples"] == 10
    data = _draw(22, 20, "camera", seed=31)
    m, _buf = _fenced_metrics(dev, "camera")
    m.update(*_dev(dev, *data))
    single = m.state()
    assert merged["samples"] == single["samples"] == 22 and merged["updates"] == 4
    single["updates"] = 4
    _assert_state(merged, single, sum_rtol=1e-12, what="two ranks vs one process")
    assert summarize(merged, THRESHOLDS)["samples"] == 22


# ---- 8. the scripts ----------------------------------------------------------------------------------------------------------------------
VAL_KEYS = {"val_loss_mean", "val_ade", "val_fde", "val_lateral", "val_longitudinal", "val_bad_rows", "val_within_0.5", "val_within_1", "val_within_2"}
PARENT_VAL_KEYS = {"train_image_phase1": {"val_loss_mean", "val_fps", "val_images_per_sec"}, "train_image_phase0": {"val_loss_mean", "val_fps"},
                   "train_birdview": {"val_loss_mean", "val_fps"}}
PARENT_TRAIN_KEYS = {k: {n.replace("val_", "train_") for n in v} for k, v in PARENT_VAL_KEYS.items()}
PHASE_OF = {"train_image_phase1": 1, "train_image_phase0": 0, "train_birdview": "birdview"}


def _parse(*argv):
    import argparse
    from learningbycheating_amd.training import resume
    p = argparse.ArgumentParser()
    resume.add_arguments(p)
    return resume.config_entries(p.parse_args(list(argv)))


def _check_val_record(rec, commands=None):
    assert VAL_KEYS <= set(rec), sorted(VAL_KEYS - set(rec))
    assert rec["val_fde"]["min"] >= 0 and rec["val_ade"]["min"] >= 0 and rec["val_ade"]["n"] == 1 and rec["val_loss_mean"]["n"] == 1
    for k in rec:
        if k.startswith("val_within_"):
            assert 0.0 <= rec[k]["min"] <= rec[k]["max"] <= 1.0, k
    assert rec["val_within_0.5"]["mean"] <= rec["val_within_1"]["mean"] <= rec["val_within_2"]["mean"]
    cmds = {int(k[len("val_ade_cmd"):]) for k in rec if k.startswith("val_ade_cmd")}
    assert cmds and cmds <= {1, 2, 3, 4} and cmds == {int(k[len("val_fde_cmd"):]) for k in rec if k.startswith("val_fde_cmd")}
    if commands is not None:
        assert cmds == commands, "absent commands are left out"


@pytest.mark.parametrize("module", sorted(PHASE_OF))
def test_script_loops_emulated(env, tmp_path, monkeypatch, module):
    """the scripts' own loop functions on the emulator (the scripts themselves need a GPU: test_scripts_log_val_metrics): with
    --val-metrics the validation pass reads nothing back per batch -- Tensor.item is never called, Tensor.cpu once, by result() --
    and logs the val_* keys; without the flags both passes log exactly the parent's keys; --train-metrics logs ade / fde / bad_rows on
    logging iterations and empties the record between them"""
    import importlib
    from learningbycheating_amd.bird_view.utils import bz_utils as bzu
    from learningbycheating_amd.bird_view.utils.datasets.synthetic import SyntheticFrames
    from learningbycheating_amd.training.data import _SyntheticLoader
    from learningbycheating_amd.training.metrics import WaypointMetrics
    dev, _ = env
    assert _parse() == {} and _parse("--val-metrics") == {"val_metrics": True} and _parse("--train-metrics") == {"train_metrics": True}
    script = importlib.import_module("learningbycheating_amd.training." + module)
    case = _TrainerCase(dev, PHASE_OF[module])
    trainer = case.make()
    frames = SyntheticFrames(4 * case.n, dev, seed=3, rgb_hw=(32, 64), birdview_hw=(64, 64))
    loader = lambda nb: _SyntheticLoader(frames, case.n, nb)
    base = dict(device=dev, log_iterations=2, rank=0, world_size=1, speed_noise=0.0)
    calls = {"item": 0, "cpu": 0, "result": 0, "reset": 0}

    def counting(cls, name, key):
        real = getattr(cls, name)

        def counted(self, *a, **k):
            calls[key] += 1
            return real(self, *a, **k)
        monkeypatch.setattr(cls, name, counted)
    counting(torch.Tensor, "item", "item")
    counting(torch.Tensor, "cpu", "cpu")
    counting(WaypointMetrics, "result", "result")
    counting(WaypointMetrics, "reset", "reset")
    bzu.log.init(str(tmp_path))
    # without the flags: the parent's keys, one read-back per validation batch
    script.train_or_eval(trainer, loader(2), False, dict(base), False)
    assert calls == {"item": 2, "cpu": 0, "result": 0, "reset": 0}
    script.train_or_eval(trainer, loader(2), True, dict(base), True)
    rec = bzu.log.end_epoch()
    assert set(rec) - {"epoch", "time"} == PARENT_VAL_KEYS[module] | PARENT_TRAIN_KEYS[module]
    # --val-metrics: no read-back inside the loop, one after it
    for k in calls:
        calls[k] = 0
    script.train_or_eval(trainer, loader(2), False, dict(base, val_metrics=True), False)
    assert calls == {"item": 0, "cpu": 1, "result": 1, "reset": 1}, calls
    assert trainer._pass_metrics[False].state()["samples"] == 2 * case.n
    rec = bzu.log.end_epoch()
    _check_val_record(rec)
    assert set(rec) - {"epoch", "time"} - PARENT_VAL_KEYS[module] <= VAL_KEYS | {"val_%s_cmd%d" % (k, c) for k in ("ade", "fde") for c in (1, 2, 3, 4)}
    # the epoch-0 dry run stops after 11 batches and behaves the same way (the three loops share the code: run on the cheapest one)
    if module == "train_birdview":
        for k in calls:
            calls[k] = 0
        script.train_or_eval(trainer, loader(13), False, dict(base, val_metrics=True), True)
        assert calls["item"] == 0 and calls["result"] == 1
        rec = bzu.log.end_epoch()
        _check_val_record(rec)
        assert trainer._pass_metrics[False].state()["samples"] == 11 * case.n
    # --train-metrics: logging iterations 0 and 2 of 0..3 log ade / fde / bad_rows and empty the record (a third reset opens the pass)
    for k in calls:
        calls[k] = 0
    script.train_or_eval(trainer, loader(4), True, dict(base, train_metrics=True), False, epoch=1)
    assert calls["result"] == 2 and calls["reset"] == 3
    rec = bzu.log.end_epoch()
    assert rec["train_ade"]["n"] == rec["train_fde"]["n"] == rec["train_bad_rows"]["n"] == 2 and rec["train_ade"]["min"] >= 0
    assert trainer._pass_metrics[True].state()["samples"] == case.n, "the record holds what came after the last logging iteration"
    assert trainer.opt.step_count == 4


# the record of one epoch with the options on; every script logs the same keys, phase 1 images_per_sec beside fps
OPTION_TRAIN_KEYS = {"train_loss_mean", "train_fps", "train_skipped_steps", "train_grad_norm", "train_clip_coef", "train_clipped_steps", "train_lr",
                     "train_optimizer_steps", "train_dropped_micro_batches", "train_ade", "train_fde", "train_bad_rows"}


@pytest.mark.parametrize("module", sorted(PHASE_OF))
def test_script_loops_log_the_options_keys_emulated(env, tmp_path, module):
    """the scripts' loop functions with the options on at once -- --accumulate 2, --log-grad-norm, --skip-nonfinite, a constant schedule
    with a warm-up, --train-metrics: a training pass of four batches and a validation pass log exactly these keys (the epoch record's
    keys are part of what a log reader depends on; the order inside a record is not)"""
    import importlib
    from learningbycheating_amd.bird_view.utils import bz_utils as bzu
    from learningbycheating_amd.bird_view.utils.datasets.synthetic import SyntheticFrames
    from learningbycheating_amd.training.data import _SyntheticLoader
    dev, _ = env
    script = importlib.import_module("learningbycheating_amd.training." + module)
    case = _TrainerCase(dev, PHASE_OF[module])
    schedule = {"kind": "constant", "warmup_steps": 2, "warmup_start": 0.0}
    trainer = case.make(accumulate=2, max_grad_norm=0.0, skip_nonfinite=True, lr_schedule=schedule)
    frames = SyntheticFrames(4 * case.n, dev, seed=3, rgb_hw=(32, 64), birdview_hw=(64, 64))
    config = dict(device=dev, log_iterations=2, rank=0, world_size=1, speed_noise=0.0, accumulate=2, max_grad_norm=0.0, skip_nonfinite=True,
                  max_skipped=50, lr_schedule=schedule, train_metrics=True)
    bzu.log.init(str(tmp_path))
    script.train_or_eval(trainer, _SyntheticLoader(frames, case.n, 4), True, dict(config), False, epoch=1)
    script.train_or_eval(trainer, _SyntheticLoader(frames, case.n, 2), False, dict(config), False)
    rec = bzu.log.end_epoch()
    # (logging iterations 0 and 2: the second window closes after iteration 3, which does not log)
    assert trainer.opt.step_count == 2 and rec["train_optimizer_steps"]["max"] == 1 and rec["train_dropped_micro_batches"]["max"] == 0
    want = OPTION_TRAIN_KEYS | {"val_loss_mean", "val_fps"} | ({"train_images_per_sec", "val_images_per_sec"} if module == "train_image_phase1" else set())
    assert set(rec) - {"epoch", "time"} == want, sorted(set(rec) ^ (want | {"epoch", "time"}))
    assert rec["train_loss_mean"]["n"] == rec["train_skipped_steps"]["n"] == rec["train_grad_norm"]["n"] == rec["train_ade"]["n"] == 2
    assert rec["train_fps"]["n"] == 4 and rec["val_fps"]["n"] == rec["val_loss_mean"]["n"] == 2


def test_phase1_validation_raises_once_after_the_pass_emulated(env, tmp_path):
    """--val-metrics in phase 1: a non-finite loss is found by ONE check after the pass (FloatingPointError unless --skip-nonfinite)"""
    from learningbycheating_amd.bird_view.utils import bz_utils as bzu
    from learningbycheating_amd.training import resume
    dev, _ = env
    m, _buf = _fenced_metrics(dev, "camera")
    pred, target, command, loss = _draw(8, 20, "camera", seed=41)
    loss[3] = np.nan
    m.update(*_dev(dev, pred, target, command, loss))
    bzu.log.init(str(tmp_path))
    with pytest.raises(FloatingPointError, match="1 of 8"):
        resume.log_val_metrics({"world_size": 1}, m, bzu.log.scalar, nonfinite="phase-1 validation loss is %s")
    res = resume.log_val_metrics({"world_size": 1, "skip_nonfinite": True}, m, bzu.log.scalar, nonfinite="phase-1 validation loss is %s")
    assert res["loss_bad"] == 1 and np.isfinite(bzu.log.end_epoch()["val_loss_mean"]["mean"])


@gpu
@pytest.mark.parametrize("module", sorted(PHASE_OF))
def test_scripts_log_val_metrics(env, tmp_path, module):
    """the script itself on --synthetic data: epoch 0 (the dry run) and one training epoch with both flags"""
    _script(module, tmp_path, 1, "--val-metrics", "--train-metrics")
    recs = [json.loads(line) for line in (tmp_path / "log.jsonl").read_text().splitlines()]
    assert len(recs) == 2
    for rec in recs:
        _check_val_record(rec)
        assert rec["train_ade"]["n"] == 3 and rec["train_fde"]["min"] >= 0 and "train_bad_rows" in rec
    cfg = json.loads((tmp_path / "config.json").read_text())
    assert cfg["val_metrics"] == 1 and cfg["train_metrics"] == 1


@gpu
def test_scripts_without_the_flags_log_the_parents_keys(env, tmp_path):
    _script("train_birdview", tmp_path, 1)
    recs = [json.loads(line) for line in (tmp_path / "log.jsonl").read_text().splitlines()]
    for rec in recs:
        assert set(rec) - {"epoch", "time"} == PARENT_VAL_KEYS["train_birdview"] | PARENT_TRAIN_KEYS["train_birdview"]
    cfg = json.loads((tmp_path / "config.json").read_text())
    assert "val_metrics" not in cfg and "train_metrics" not in cfg


@gpu
def test_evaluate_scores_a_checkpoint(env, tmp_path):
    """python -m learningbycheating_amd.training.evaluate on a bird-view checkpoint: metrics.json loads and holds the numbers of a
    WaypointMetrics fed by hand -- steps without metrics=, then update() -- over the same loader and checkpoint"""
    from learningbycheating_amd.bird_view.utils.train_utils import one_hot
    from learningbycheating_amd.training import evaluate
    from learningbycheating_amd.training.data import make_loaders
    dev, _ = env
    _script("train_birdview", tmp_path, 1)
    ckpt = tmp_path / "model-1.th"
    before = ckpt.read_bytes()
    environ = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "learningbycheating_amd.training.evaluate", "--phase", "birdview", "--model_path", str(ckpt),
                        "--synthetic", "64", "--batch_size", "4", "--batches", "3"], env=environ, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with open(str(tmp_path / "metrics.json")) as f:
        got = json.load(f)
    assert json.loads(p.stdout.strip().splitlines()[-1]) == got and ckpt.read_bytes() == before
    trainer = evaluate.build_trainer("birdview", str(ckpt), None, 4, "fp32", dev)
    _, val = make_loaders({"data_args": {"dataset_dir": None, "batch_size": 4}, "synthetic": 64, "iters_per_epoch": 300}, dev)
    m = trainer.make_metrics()
    for rgb, bv, loc, cmd, speed in val:
        command, target = one_hot(cmd).to(dev), loc.float().contiguous()
        loss = trainer.step(bv, speed, command, target=target, update=False, train_mode=False)
        m.update(trainer.last_pred[0], target, command, loss)
    want = m.result()
    assert got["samples"] == want["samples"] == 12 and trainer.opt.step_count == 0
    for k in ("ade", "fde", "rmse", "lateral", "longitudinal", "max", "loss_mean", "ade_by_command", "fde_by_command", "ade_by_step", "bad_rows"):
        assert got[k] == want[k], k
    assert got["within"] == {"%g" % k: v for k, v in want["within"].items()}


@gpu
@pytest.mark.parametrize("phase", [0, 1])
def test_evaluate_builds_the_image_phases(env, tmp_path, phase):
    from learningbycheating_amd.bird_view.models import BirdViewPolicyModelSS, ImagePolicyModelSS
    from learningbycheating_amd.training import evaluate
    from learningbycheating_amd.training.data import make_loaders
    dev, _ = env
    torch.manual_seed(5)
    torch.save(ImagePolicyModelSS("resnet34", all_branch=(phase == 1)).state_dict(), str(tmp_path / "model-1.th"))
    (tmp_path / "teacher").mkdir()
    torch.save(BirdViewPolicyModelSS("resnet18", all_branch=(phase == 1)).state_dict(), str(tmp_path / "teacher" / "model-1.th"))
    trainer = evaluate.build_trainer(phase, str(tmp_path / "model-1.th"), str(tmp_path / "teacher" / "model-1.th"), 4, "bf16", dev)
    _, val = make_loaders({"data_args": {"dataset_dir": None, "batch_size": 4}, "synthetic": 32, "iters_per_epoch": 200}, dev)
    res = evaluate.validation_pass(trainer, val, dev).result()
    assert res["samples"] == 8 and res["updates"] == 2 and ("all_branch_ade" in res) == (phase == 1) and trainer.opt.step_count == 0
    assert res["bad_rows"] + sum(1 for v in res["ade_by_step"] if v is not None) > 0 and json.loads(json.dumps(res["ade_by_step"])) == res["ade_by_step"]
