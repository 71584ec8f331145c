"""The agent half of the tick on the device (csrc/agent.hip, learningbycheating_amd/agent.py): waypoints -> steer / throttle / brake.

Two yardsticks.
1. tests/golden/agent_controls.npz: what the REAL reference agents (ImageAgent.run_step / BirdViewAgent.run_step with their
   controllers) answered on a CPU for 16 episodes of 35 ticks per kind (tests/golden/make_agent_fixture.py).
2. `Twin` below: a double-precision restatement of include/lbc_hip.h's definition in plain Python floats, one object per agent,
   written from the header and not from the kernel.  It rounds to float32 exactly where the reference's float32 arrays do
   (`pred + 1` for the image kind, `(pred + 1) / 2 * CROP_SIZE` for the bird-view kind) and nowhere else.

Bounds.  Image kind against the reference, and kernel against twin for both kinds: 1e-9 absolute.  Both sides compute in double from
the same float32 inputs; the fit's conditioning is capped at 1e2 (the generator asserts |det| / (Suu Svv) >= 1e-2 on every tick), a
tick is a few hundred operations and libm's sqrt / atan2 differ by a few ulp between hosts and the device: 1.1e-16 x 1e2 x ~1e3 stays
below 1e-11, and the PID sums over <= 30 values of magnitude <= ~10 add nothing visible.  Bird-view kind against the reference:
3 x twin_max_dev_birdview as stored in the fixture -- the reference itself computes pixel offsets, distances and the target speed of
that kind in float32 scalars (under the recorded NumPy version), so its own arithmetic is ~1e-5 away from any double restatement; 3 x
covers another libm.  No brake decision can flip inside these bounds: the generator keeps every target speed 1e-3 away from its threshold.

(a) kernel against the fixture and the twin; (b) shapes and a changing active mask; (c) known answers for the cases the reference
leaves undefined, reset, refusals; (d) the fixture regenerates bit for bit where the reference tree is present; (e) DrivingSession
and (f) ImageAgent on the GPU.  Every kernel case runs on the emulator and, gpu-marked, on gfx950."""
import collections
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import WHERE, check_guard, guarded, guarded_input, on_both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "agent_controls.npz")
TOL = 1e-9
BAD_ROW = np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 2.0])
INACTIVE_ROW = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 4.0])


# ---- the double-precision twin -------------------------------------------------------------------------------------------------------
def _config(kind, **changes):
    from learningbycheating_amd.agent import ControllerConfig
    cfg = ControllerConfig.image({"w": 384, "h": 160, "fov": 90, "world_y": 1.4, "fixed_offset": 4.0}) if kind == "image" else ControllerConfig.birdview()
    for k, v in changes.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    return cfg


def twin_geometry(cfg, pred):
    """pred: (5,2) float32 -> (targets [(forward, lateral)] x 6, target_speed, bad) in Python floats"""
    c = cfg
    p = np.asarray(pred, dtype=np.float32)
    targets, bad = [(0.0, 0.0)], not bool(np.isfinite(p).all())
    if c["kind"] == "image":
        f = c["w"] / (2.0 * math.tan(c["fov"] * math.pi / 360.0))
        one = np.float32(1.0)
        for k in range(5):
            px = float(np.float32(p[k, 0] + one)) * c["w"] / 2.0
            py = float(np.float32(p[k, 1] + one)) * c["h"] / 2.0
            xt, yt = (px - c["w"] / 2.0) / f, (py - c["h"] / 2.0) / f
            if not yt > 0.0:
                bad = True
                targets.append((float("nan"), float("nan")))
                continue
            z = c["world_y"] / yt
            targets.append((z - c["fixed_offset"], z * xt))
        if bad:
            return targets, float("nan"), True
        seg = [math.sqrt((targets[k][0] - targets[k + 1][0]) ** 2 + (targets[k][1] - targets[k + 1][1]) ** 2) for k in range(5)]
        return targets, sum(seg) / 5.0 / (c["gap"] * c["dt"]), False
    crop = np.float32(c["crop_size"])
    q = ((p + np.float32(1.0)) / np.float32(2.0) * crop).astype(np.float32)
    assert q.dtype == np.float32
    if bad:
        return targets, float("nan"), True
    q = q.astype(np.float64)
    for k in range(5):
        targets.append(((c["crop_size"] - float(q[k, 1])) / c["pixels_per_meter"], (float(q[k, 0]) - c["crop_size"] / 2.0) / c["pixels_per_meter"]))
    ts = 0.0
    for k in range(1, c["speed_steps"]):
        d = math.sqrt(float(q[k, 0] - q[k - 1, 0]) ** 2 + float(q[k, 1] - q[k - 1, 1]) ** 2)
        ts += d / (c["pixels_per_meter"] * (c["gap"] * c["dt"])) / (c["speed_steps"] - 1)
    return targets, ts, False


def twin_fit(targets):
    """the least-squares circle of the header -> (centre x, centre y, r, conditioning |det| / (Suu Svv), Suu Svv)"""
    xs, ys = [t[0] for t in targets], [t[1] for t in targets]
    mx, my = sum(xs) / 6.0, sum(ys) / 6.0
    us, vs = [x - mx for x in xs], [y - my for y in ys]
    Suu, Suv, Svv = sum(u * u for u in us), sum(u * v for u, v in zip(us, vs)), sum(v * v for v in vs)
    Suuu, Suvv = sum(u * u * u for u in us), sum(u * v * v for u, v in zip(us, vs))
    Svvv, Svuu = sum(v * v * v for v in vs), sum(v * u * u for u, v in zip(us, vs))
    det = Suu * Svv - Suv * Suv
    if not abs(det) > 1e-12 * (Suu * Svv):
        return None, None, None, (abs(det) / (Suu * Svv) if Suu * Svv > 0 else 0.0), Suu * Svv
    b0, b1 = 0.5 * Suuu + 0.5 * Suvv, 0.5 * Svvv + 0.5 * Svuu
    cx, cy = (b0 * Svv - b1 * Suv) / det, (Suu * b1 - Suv * b0) / det
    r = math.sqrt(cx * cx + cy * cy + (Suu + Svv) / 6.0)
    return cx + mx, cy + my, r, abs(det) / (Suu * Svv), Suu * Svv


class Twin:
    """one agent: step(pred (5,2) f32, speed f32, command row (4,) f32) -> the 8 outputs of lbc_agent_control as a float64 array"""

    def __init__(self, cfg):
        self.c = cfg.as_dict() if hasattr(cfg, "as_dict") else dict(cfg)
        self.reset()

    def reset(self):
        self.turn = collections.deque(maxlen=self.c["turn_window"])
        self.speed = collections.deque(maxlen=self.c["speed_window"])

    @staticmethod
    def _pid(window, v, dt):
        window.append(v)
        if len(window) >= 2:
            return sum(window) * dt, (window[-1] - window[-2]) / dt
        return 0.0, 0.0

    def step(self, pred, speed, command):
        c = self.c
        command = [float(v) for v in command]
        onehot = sorted(command) == [0.0, 0.0, 0.0, 1.0]
        targets, ts, bad = twin_geometry(c, pred)
        if bad or not onehot:
            return BAD_ROW.copy()
        cmd = command.index(1.0)
        sx, sy = targets[c["steer_points"][cmd]]
        cx, cy, r, _, _ = twin_fit(targets)
        flags, aim = 0.0, (sx, sy)
        if cx is None:
            flags = 1.0
        else:
            dx, dy = sx - cx, sy - cy
            dn = math.sqrt(dx * dx + dy * dy)
            if dn > 0.0:
                aim = (cx + dx / dn * r, cy + dy / dn * r)
            else:
                flags = 1.0
        alpha = math.atan2(aim[1], aim[0])
        kp, ki, kd = c["turn_pid"][cmd]
        ie, de = self._pid(self.turn, alpha, c["dt"])
        steer = kp * alpha + kd * de + ki * ie
        err = ts - float(np.float32(speed))
        ie, de = self._pid(self.speed, err, c["dt"])
        throttle = c["speed_pid"][0] * err + c["speed_pid"][1] * ie + c["speed_pid"][2] * de
        brake = 0.0
        if c["kind"] == "image":
            if ts <= c["engine_brake_threshold"]:
                steer = throttle = 0.0
            if ts <= c["brake_threshold"]:
                brake = 1.0
        elif ts < c["stop_threshold"]:
            steer, throttle, brake = 0.0, 0.0, 1.0
        clip = lambda v, lo, hi: min(max(v, lo), hi)
        return np.array([clip(steer, -1.0, 1.0), clip(throttle, 0.0, 1.0), clip(brake, 0.0, 1.0), ts, aim[0], aim[1], alpha, flags])


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def arc_waypoints(kind, curvature, v, gap=5, dt=0.1):
    """five points `gap * dt` seconds apart on an arc of the given curvature (1 / m) driven at v m/s -> (5,2) float64 normalised
    camera (image) or map (bird-view) coordinates under the reference's default geometry"""
    s = v * gap * dt * np.arange(1, 6)
    fwd = np.sin(curvature * s) / curvature
    lat = (1.0 - np.cos(curvature * s)) / curvature
    out = np.empty((5, 2))
    if kind == "image":
        f, z = 192.0, fwd + 4.0
        out[:, 0] = (192.0 + lat / z * f) / 192.0 - 1.0
        out[:, 1] = (80.0 + 1.4 / z * f) / 80.0 - 1.0
    else:
        out[:, 0] = (96.0 + lat * 5.0) / 96.0 - 1.0
        out[:, 1] = (192.0 - fwd * 5.0) / 96.0 - 1.0
    return out


def draw_episodes(kind, n, ticks, seed, slow=()):
    """-> pred (n,ticks,5,2) f32, speed (n,ticks) f32, command (n,ticks) int64 (1..4).  Arcs of curvature +-U(0.03, 0.3) per metre (capped
    where five waypoints would cover more than 1 rad), a speed that swings through the kind's stop threshold (episodes listed in `slow`
    go down to 0.2 m/s), Gaussian noise of 1e-3 on the normalised waypoints, random commands, measured speeds in [0, 8].  A tick whose
    fit is conditioned worse than 2e-2 or whose target speed comes within 2e-3 of the threshold gets fresh noise."""
    cfg = _config(kind).as_dict()
    thr = 2.0 if kind == "image" else 1.0
    rng = np.random.RandomState(seed)
    pred = np.empty((n, ticks, 5, 2), dtype=np.float32)
    speed = rng.uniform(0.0, 8.0, size=(n, ticks)).astype(np.float32)
    command = rng.randint(1, 5, size=(n, ticks)).astype(np.int64)
    for e in range(n):
        k = rng.uniform(0.03, 0.3) * (1.0 if rng.rand() < 0.5 else -1.0)
        lo = 0.2 if e in slow else rng.uniform(0.4, 0.8) * thr
        hi, phase = rng.uniform(1.5, 3.0) * thr, rng.uniform(0.0, 1.0)
        for t in range(ticks):
            v = lo + (hi - lo) * 0.5 * (1.0 + math.cos(2.0 * math.pi * (t / float(ticks) + phase)))
            kk = math.copysign(min(abs(k), 1.0 / (2.5 * v)), k)
            clean = arc_waypoints(kind, kk, v)
            for _ in range(200):
                p = (clean + rng.normal(0.0, 1e-3, size=(5, 2))).astype(np.float32)
                targets, ts, bad = twin_geometry(cfg, p)
                if not bad and twin_fit(targets)[3] >= 2e-2 and abs(ts - thr) >= 2e-3:
                    break
            else:
                raise AssertionError("could not draw a well-conditioned tick")
            pred[e, t] = p
    return pred, speed, command


def one_hot(command):
    out = np.zeros(command.shape + (4,), dtype=np.float32)
    np.put_along_axis(out, (command - 1)[..., None], 1.0, axis=-1)
    return out


# ---- the kernel between fences -----------------------------------------------------------------------------------------------------------
class Fenced:
    """a WaypointController whose records and output rows lie between NaN fences"""

    def __init__(self, dev, cfg, n):
        from learningbycheating_amd.agent import STATE_WORDS, WaypointController
        self.dev, self.n, self.words = dev, n, n * STATE_WORDS
        self.c = WaypointController(cfg, n, dev)
        self.sbuf, st = guarded((self.words,), dev, dtype=torch.float64)
        st.zero_()
        self.c.state = st.view(torch.int64).view(n, STATE_WORDS)
        self.obuf, self.c.out = guarded((n, 8), dev, dtype=torch.float64)

    def step(self, pred, speed, command_row, active=None):
        put = lambda a, dt: guarded_input(torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.dev))
        act = None if active is None else torch.from_numpy(np.ascontiguousarray(active, dtype=np.uint8)).to(self.dev)
        out = self.c.step(put(pred, np.float32), put(speed, np.float32), put(command_row, np.float32), act)
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        check_guard(self.sbuf, self.words)
        check_guard(self.obuf, self.n * 8)
        return out.cpu().numpy().copy()

    def state(self):
        return self.c.state.cpu().numpy().copy()


def _close(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.isfinite(got).all(), what
    err = float(np.abs(got - want).max())
    print("%s: worst absolute difference %.3g (bound %.3g)" % (what, err, tol))
    assert err <= tol, (what, err, tol)


_FIXTURE = {}


def fixture():
    if not _FIXTURE:
        with np.load(FIXTURE) as z:
            _FIXTURE.update({k: z[k] for k in z.files})
    return _FIXTURE


# ---- (a) kernel against the reference's recorded answers and against the twin ----------------------------------------------------------
@pytest.mark.parametrize("kind", on_both("kind", ["image", "birdview"]))
def test_kernel_matches_reference_fixture_and_twin(env, kind):
    dev, _ = env
    fx = fixture()
    pred, speed, command, ref = fx[kind + "_pred"], fx[kind + "_speed"], fx[kind + "_command"], fx[kind + "_ref"]
    n, ticks = speed.shape
    assert (n, ticks) == (16, 35) and float(fx[kind + "_cond"].min()) >= 1e-2
    thr = 2.0 if kind == "image" else 1.0
    assert (ref[..., 3] > thr).any() and (ref[..., 3] < thr).any() and float(np.abs(ref[..., 3] - thr).min()) >= 1e-3
    tol_ref = TOL if kind == "image" else 3.0 * float(fx["twin_max_dev_birdview"])
    assert 0.0 < tol_ref < 1e-3
    cfg = _config(kind)
    k = Fenced(dev, cfg, n)
    twins = [Twin(cfg) for _ in range(n)]
    rows = one_hot(command)
    got, want = np.empty((ticks, n, 8)), np.empty((ticks, n, 8))
    for t in range(ticks):
        got[t] = k.step(pred[:, t], speed[:, t], rows[:, t])
        want[t] = [twins[i].step(pred[i, t], speed[i, t], rows[i, t]) for i in range(n)]
    assert not got[..., 7].any(), "no tick of the fixture is degenerate or bad"
    _close(got.transpose(1, 0, 2)[..., :6], ref, tol_ref, "%s kernel vs reference" % kind)
    _close(got, want, TOL, "%s kernel vs twin" % kind)
    st = k.state().view(np.int32).reshape(n, -1)
    assert (st[:, 80] == 10).all() and (st[:, 81] == 35 % 10).all() and (st[:, 82] == 30).all() and (st[:, 83] == 35 % 30).all(), "counts and heads"


# ---- (b) shapes and a changing active mask -------------------------------------------------------------------------------------------------
SHAPES = [(kind, n) for kind in ("image", "birdview") for n in (1, 3, 64, 65)]


@pytest.mark.parametrize("case", on_both("case", SHAPES))
def test_shapes_and_active_mask(env, case):
    dev, _ = env
    kind, n = case
    ticks = 13                                   # more than the steering window: its ring wraps
    pred, speed, command = draw_episodes(kind, n, ticks, seed=100 + n)
    rows = one_hot(command)
    rng = np.random.RandomState(7 + n)
    cfg = _config(kind)
    k = Fenced(dev, cfg, n)
    twins = [Twin(cfg) for _ in range(n)]
    stepped = np.zeros(n, dtype=np.int64)
    for t in range(ticks):
        active = (rng.rand(n) < 0.6).astype(np.uint8) if t % 4 != 3 else np.ones(n, dtype=np.uint8)
        before = k.state()
        got = k.step(pred[:, t], speed[:, t], rows[:, t], None if t == 3 else active)
        if t == 3:
            active = np.ones(n, dtype=np.uint8)          # (a null mask: everyone)
        after = k.state()
        for i in range(n):
            if active[i]:
                want = twins[i].step(pred[i, t], speed[i, t], rows[i, t])
                assert np.isfinite(got[i]).all() and np.abs(got[i] - want).max() <= TOL, (kind, n, t, i, got[i], want)
                stepped[i] += 1
            else:
                assert np.array_equal(got[i], INACTIVE_ROW), (t, i, got[i])
                assert after[i].tobytes() == before[i].tobytes(), "an inactive agent's record is untouched"
    st = k.state().view(np.int32).reshape(n, -1)
    assert np.array_equal(st[:, 80], np.minimum(stepped, 10)) and np.array_equal(st[:, 82], np.minimum(stepped, 30))


# ---- (c) known answers for our own definitions ---------------------------------------------------------------------------------------------
def _straight(kind):
    """five exactly collinear waypoints: dead ahead (lateral exactly 0), and for the map a diagonal whose pixels are exact in float32"""
    if kind == "image":
        y = np.array([0.6, 0.45, 0.36, 0.3, 0.26], dtype=np.float32)          # 1.6 .. 8.9 m ahead
        return [np.stack([np.zeros(5, dtype=np.float32), y], 1)]
    j = np.arange(1, 6, dtype=np.float32)
    ahead = np.stack([np.zeros(5, dtype=np.float32), 1.0 - j / 8.0], 1)          # pixels (96, 192 - 12 j)
    diagonal = np.stack([j / 16.0, 1.0 - j / 8.0], 1)                            # pixels (96 + 6 j, 192 - 12 j): lateral = forward / 2
    return [ahead.astype(np.float32), diagonal.astype(np.float32)]


@pytest.mark.parametrize("kind", on_both("kind", ["image", "birdview"]))
def test_collinear_waypoints_aim_at_the_steer_point(env, kind):
    dev, _ = env
    cfg = _config(kind, engine_brake_threshold=0.5, brake_threshold=0.5, stop_threshold=0.5)       # (so that the controls are not all zero)
    for wp in _straight(kind):
        n = 4                                    # one agent per command
        k = Fenced(dev, cfg, n)
        twins = [Twin(cfg) for _ in range(n)]
        rows = np.eye(4, dtype=np.float32)
        for t in range(3):
            speed = np.full(n, 0.1 + 0.1 * t, dtype=np.float32)
            got = k.step(np.repeat(wp[None], n, 0), speed, rows)
            want = np.array([twins[i].step(wp, speed[i], rows[i]) for i in range(n)])
            assert (got[:, 7] == 1.0).all(), got[:, 7]
            targets = twin_geometry(cfg.as_dict(), wp)[0]
            for i in range(n):
                # (targets[n] is a handful of double operations on values below 40 m: two sides agree to a few ulp, 1e-14; asserted at 1e-12)
                assert np.abs(got[i, 4:6] - np.array(targets[cfg.steer_points[i]])).max() <= 1e-12, "the aim point is targets[n] itself"
            _close(got, want, TOL, "%s collinear tick %d" % (kind, t))
            assert np.abs(got[:, :3]).max() > 0.0


BAD = [("horizon", "image"), ("nan", "image"), ("nan", "birdview"), ("inf", "birdview"), ("command-zero", "image"), ("command-two", "birdview"),
       ("command-half", "image"), ("command-nan", "birdview")]


@pytest.mark.parametrize("case", on_both("case", BAD))
def test_bad_waypoint_brakes_and_keeps_the_windows(env, case):
    dev, _ = env
    what, kind = case
    n, ticks = 3, 4
    pred, speed, command = draw_episodes(kind, n, ticks, seed=31)
    rows = one_hot(command)
    cfg = _config(kind)
    k = Fenced(dev, cfg, n)
    twins = [Twin(cfg) for _ in range(n)]
    for t in range(ticks):
        p, r = pred[:, t].copy(), rows[:, t].copy()
        if t == 2:                               # agent 1 gets the bad input, after two good ticks
            if what == "horizon":
                p[1, 3, 1] = 0.0                 # (y + 1) h / 2 = h / 2: yt = 0
            elif what == "nan":
                p[1, 0, 0] = np.nan
            elif what == "inf":
                p[1, 4, 1] = np.inf
            else:
                r[1] = {"command-zero": [0, 0, 0, 0], "command-two": [1, 0, 1, 0], "command-half": [0, 0.5, 0, 0], "command-nan": [0, 1, np.nan, 0]}[what]
        before = k.state()
        got = k.step(p, speed[:, t], r)
        after = k.state()
        for i in range(n):
            if t == 2 and i == 1:
                assert np.array_equal(got[i], BAD_ROW), got[i]
                assert after[i].tobytes() == before[i].tobytes(), "a bad waypoint leaves the windows untouched"
                assert np.array_equal(twins[i].step(p[i], speed[i, t], r[i]), BAD_ROW)
            else:
                _close(got[i], twins[i].step(p[i], speed[i, t], r[i]), TOL, "%s tick %d agent %d" % (what, t, i))
    if kind == "image":                           # above the horizon is bad too
        p = pred[:, 0].copy()
        p[0, 2, 1] = -0.25
        assert np.array_equal(k.step(p, speed[:, 0], rows[:, 0])[0], BAD_ROW)


@pytest.mark.parametrize("kind", on_both("kind", ["image", "birdview"]))
def test_reset_of_a_subset_and_zero_bytes_are_fresh(env, kind):
    dev, _ = env
    n, ticks = 5, 6
    pred, speed, command = draw_episodes(kind, n, ticks, seed=41)
    rows = one_hot(command)
    cfg = _config(kind)
    k = Fenced(dev, cfg, n)
    twins = [Twin(cfg) for _ in range(n)]
    for t in range(ticks):
        if t == 3:
            k.c.reset(agents=[1, 4])
            twins[1].reset()
            twins[4].reset()
            st = k.state()
            assert not st[[1, 4]].any() and st[[0, 2, 3]].any(axis=1).all()
        got = k.step(pred[:, t], speed[:, t], rows[:, t])
        _close(got, [twins[i].step(pred[i, t], speed[i, t], rows[i, t]) for i in range(n)], TOL, "%s reset tick %d" % (kind, t))
    check_guard(k.sbuf, k.words)
    # a saved state continues where it was; all-zero bytes are the fresh state
    saved = k.c.state_dict()
    nxt = k.step(pred[:, 0], speed[:, 0], rows[:, 0])
    k.c.load_state_dict(saved)
    assert np.array_equal(k.step(pred[:, 0], speed[:, 0], rows[:, 0]), nxt)
    k.c.load_state_dict(dict(saved, state=torch.zeros_like(saved["state"])))
    fresh = Fenced(dev, cfg, n)
    assert np.array_equal(k.step(pred[:, 1], speed[:, 1], rows[:, 1]), fresh.step(pred[:, 1], speed[:, 1], rows[:, 1]))
    k.c.reset()
    assert not k.state().any()
    with pytest.raises(ValueError):
        k.c.reset(agents=[n])
    with pytest.raises(ValueError):
        k.c.load_state_dict(dict(saved, turn_window=5))


REFUSALS = [("struct_size", dict(struct_size=0)), ("struct_size", dict(struct_size=264)), ("kind", dict(kind=2)), ("n_steps", dict(n_steps=4)),
            ("speed_steps", dict(speed_steps=1)), ("speed_steps", dict(speed_steps=6)), ("turn_window", dict(turn_window=1)),
            ("turn_window", dict(turn_window=11)), ("speed_window", dict(speed_window=1)), ("speed_window", dict(speed_window=31)),
            ("steer_points", dict(steer_point=-1)), ("steer_points", dict(steer_point=6)), ("gap", dict(gap=0.0)), ("gap", dict(gap=-5.0)),
            ("dt", dict(dt=0.0)), ("dt", dict(dt=float("nan"))), ("fov", dict(fov=0.0)), ("fov", dict(fov=180.0)), ("w =", dict(w=0.0)),
            ("h =", dict(h=-160.0)), ("crop_size", dict(crop_size=0.0)), ("pixels_per_meter", dict(pixels_per_meter=-5.0)),
            ("not finite", dict(world_y=float("inf")))]


@pytest.mark.parametrize("where", WHERE)
def test_entry_point_refusals(env, where):
    from learningbycheating_amd import _lib
    from learningbycheating_amd.agent import STATE_WORDS
    dev, _ = env
    lib = _lib.get()
    assert lib.lbc_agent_state_bytes(1) == ctypes.sizeof(_lib.AgentState) == 336 == STATE_WORDS * 8
    assert lib.lbc_agent_state_bytes(7) == 7 * 336 and lib.lbc_agent_state_bytes(0) == 0 and lib.lbc_agent_state_bytes(-3) == 0
    assert ctypes.sizeof(_lib.AgentDesc) == 256
    n = 2
    pred, speed, command = draw_episodes("image", n, 1, seed=5)
    k = Fenced(dev, _config("image"), n)
    good = k.step(pred[:, 0], speed[:, 0], one_hot(command)[:, 0])
    state0 = k.state()
    args = [guarded_input(torch.from_numpy(a).to(dev)) for a in (pred[:, 0].copy(), speed[:, 0].copy(), one_hot(command)[:, 0].copy())]
    call = lambda d, p=None, st=None, out=None, cnt=n: lib.lbc_agent_control(
        ctypes.byref(d) if d is not None else None, *(p or [_lib.ptr(a) for a in args]), None, cnt,
        _lib.ptr(k.c.state) if st is None else st, _lib.ptr(k.c.out) if out is None else out, _lib.stream_for(args[0]))
    for kind in ("image", "birdview"):
        for needle, change in REFUSALS:
            d = _config(kind).desc()
            for f, v in change.items():
                if f == "steer_point":
                    d.steer_points[2] = v
                else:
                    setattr(d, f, v)
            rc = call(d)
            msg = lib.lbc_last_error().decode()
            assert rc != 0 and msg.startswith("agent_control:") and needle in msg, (kind, change, rc, msg)
    d = _config("image").desc()
    for what, kw in (("descriptor", dict(d=None)), ("null pred", dict(d=d, p=[None, _lib.ptr(args[1]), _lib.ptr(args[2])])),
                     ("null state", dict(d=d, st=ctypes.c_void_p(0))), ("misaligned state", dict(d=d, st=ctypes.c_void_p(k.c.state.data_ptr() + 4))),
                     ("null out", dict(d=d, out=ctypes.c_void_p(0))), ("negative N", dict(d=d, cnt=-1))):
        assert call(**kw) != 0 and lib.lbc_last_error().decode().startswith("agent_control:"), what
    assert lib.lbc_agent_reset(None, n, None, None) != 0 and lib.lbc_last_error().decode().startswith("agent_reset:")
    assert lib.lbc_agent_reset(None, -1, _lib.ptr(k.c.state), None) != 0 and b"negative" in lib.lbc_last_error()
    assert call(d, cnt=0) == 0 and lib.lbc_agent_reset(None, 0, _lib.ptr(k.c.state), None) == 0       # N = 0 launches nothing
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert k.state().tobytes() == state0.tobytes() and np.array_equal(k.c.out.cpu().numpy(), good), "a refused call writes nothing"
    check_guard(k.sbuf, k.words)
    check_guard(k.obuf, n * 8)


def test_config_takes_the_reference_argument_shapes():
    from learningbycheating_amd.agent import ControllerConfig
    a = ControllerConfig.image()
    assert (a.w, a.h, a.fov, a.world_y, a.fixed_offset) == (384.0, 160.0, 90.0, 1.4, 4.0) and a.steer_points == [4, 3, 2, 2]
    assert a.turn_pid[3] == [1.0, 0.5, 0.0] and a.speed_pid == [0.8, 0.08, 0.0] and (a.turn_window, a.speed_window) == (10, 30)
    b = ControllerConfig.image(camera_args={"x": 400, "h": 200, "fov": 100, "world_y": 1.5, "fixed_offset": 3.0})      # the reference's own key
    c = ControllerConfig.image(camera_args={"w": 400, "h": 200, "fov": 100, "world_y": 1.5, "fixed_offset": 3.0})
    assert b.as_dict() == c.as_dict() and b.w == 400.0 and b.fixed_offset == 3.0
    v = ControllerConfig.birdview(steer_points={"1": 1, "2": 5}, pid={str(i): {"Kp": i, "Ki": 0.5, "Kd": 0.25} for i in range(1, 5)}, gap=3)
    assert v.steer_points == [1, 5, 1, 1] and v.turn_pid[1] == [2.0, 0.5, 0.25] and v.gap == 3.0 and v.speed_pid == [1.0, 0.1, 2.5]
    d = v.desc()
    assert d.struct_size == 256 and d.kind == 1 and d.steer_points[1] == 5 and d.turn_pid[3][0] == 4.0 and d.stop_threshold == 1.0


# ---- (d) the fixture regenerates bit for bit ---------------------------------------------------------------------------------------------
def test_fixture_regenerates_bit_for_bit():
    from oracle import ref_shim
    if not ref_shim.available():
        pytest.skip("the reference tree is not on this machine")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_agent_fixture", os.path.join(ROOT, "tests", "golden", "make_agent_fixture.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh, stored = gen.generate(), fixture()
    assert sorted(fresh) == sorted(stored)
    for name in sorted(stored):
        a, b = np.asarray(fresh[name]), stored[name]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name


# ---- (e) DrivingSession on the GPU ---------------------------------------------------------------------------------------------------------
def _model(kind, seed):
    """a resnet18 policy with the oracle's synthetic weights.  The image model's soft-argmax rows are moved below the horizon
    (pos_y in [0.2, 0.9] instead of [-1, 1]): untrained weights answer waypoints around y = 0, which the controller rightly refuses"""
    from learningbycheating_amd.bird_view.models import BirdViewPolicyModelSS, ImagePolicyModelSS
    from oracle import lbc_oracle as O
    sd = O.make_state_dict(kind, "resnet18", seed)
    if kind == "image":
        for name in sd:
            if name.endswith("pos_y"):
                sd[name] = sd[name] * 0.35 + 0.55
    net = ImagePolicyModelSS("resnet18") if kind == "image" else BirdViewPolicyModelSS("resnet18")
    net.load_state_dict(sd)
    return net


def _frames(kind, n, ticks, seed):
    rng = np.random.RandomState(seed)
    shape = (160, 384, 3) if kind == "image" else (320, 320, 7)
    frames = rng.randint(0, 256, size=(ticks, n) + shape).astype(np.uint8)
    if kind == "birdview":
        frames = (frames > 200).astype(np.uint8) * 255
    return frames, rng.uniform(0.0, 8.0, size=(ticks, n)).astype(np.float32), rng.randint(1, 5, size=(ticks, n))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,ticks", [("image", 12), ("birdview", 4)])
def test_driving_session(env, kind, ticks):
    from learningbycheating_amd.agent import DrivingSession
    from learningbycheating_amd.inference import PolicySession
    dev, _ = env
    n = 3
    cfg = _config(kind, engine_brake_threshold=0.05, brake_threshold=0.02, stop_threshold=0.05)       # untrained waypoints lie close together
    net = _model(kind, 3)
    frames, speeds, commands = _frames(kind, n, ticks, 11)
    graph, eager = DrivingSession(net, dev, n_agents=n, config=cfg), DrivingSession(net, dev, n_agents=n, use_graph=False, config=cfg)
    assert graph.graph is not None and eager.graph is None
    single = PolicySession(net, dev)
    twins = [Twin(cfg) for _ in range(n)]
    reset_at = ticks // 2
    seen_flags = set()
    for t in range(ticks):
        if t == reset_at:
            graph.reset(agents=[1])
            eager.reset(agents=[1])
            twins[1].reset()
        active = None if t != 1 else [1, 0, 1]
        a = graph.run_step(frames[t], speeds[t], commands[t], active)
        b = eager.run_step(frames[t], speeds[t], commands[t], active)
        assert a.shape == (n, 3) and a.dtype == np.float64 and a.tobytes() == b.tobytes(), "graph replay = eager launches, bit for bit"
        for key in ("target_speed", "target", "alpha", "flags", "waypoints"):
            assert graph.debug[key].tobytes() == eager.debug[key].tobytes(), key
        wp = graph.debug["waypoints"]
        assert wp.shape == (n, 5, 2) and wp.dtype == np.float32
        rows = one_hot(np.asarray(commands[t]))
        for i in range(n):
            crop = frames[t, i] if kind == "image" else np.ascontiguousarray(frames[t, i][58:250, 64:256])
            assert single.run_step(crop, speeds[t, i], commands[t, i]).tobytes() == wp[i].tobytes(), "PolicySession's waypoints, bit for bit"
            got = np.concatenate([a[i], graph.debug["target_speed"][i:i + 1], graph.debug["target"][i], graph.debug["alpha"][i:i + 1],
                                  graph.debug["flags"][i:i + 1].astype(np.float64)])
            if active is not None and not active[i]:
                assert np.array_equal(got, INACTIVE_ROW)
                continue
            _close(got, twins[i].step(wp[i], speeds[t, i], rows[i]), TOL, "%s session tick %d agent %d" % (kind, t, i))
            seen_flags.add(int(got[7]))
    assert 0 in seen_flags, "the session's ticks exercise the controllers, not only the refusal"
    st = graph.controller.state.cpu().numpy().view(np.int32).reshape(n, -1)
    assert st[0, 80] == min(ticks, 10) and st[1, 80] <= ticks - reset_at, "only agent 1 restarted"
    with pytest.raises(ValueError):
        graph.run_step(frames[0][:, :-1], speeds[0], commands[0])


# ---- (f) the reference-shaped agent ----------------------------------------------------------------------------------------------------------
def test_agent_modules_import_without_carla():
    code = ("import sys; sys.modules['carla'] = None; sys.modules['torchvision'] = None\n"
            "from learningbycheating_amd.bird_view.models.image import ImageAgent\n"
            "from learningbycheating_amd.bird_view.models.birdview import BirdViewAgent\n"
            "from learningbycheating_amd import agent\n"
            "c = agent.Agent.postprocess(None, 2.0, -1.0, 0.5)\n"
            "assert (c.steer, c.throttle, c.brake, c.manual_gear_shift) == (1.0, 0.0, 0.5, False), vars(c)\n"
            "print('ok')")
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr


@pytest.mark.gpu
def test_image_agent_equals_a_one_agent_session(env):
    from learningbycheating_amd.agent import DrivingSession
    from learningbycheating_amd.bird_view.models.image import ImageAgent
    dev, _ = env
    ticks = 12
    net, net2 = _model("image", 5), _model("image", 5)
    frames, speeds, commands = _frames("image", 1, ticks, 13)
    agent = ImageAgent(model=net)
    assert agent.model is agent.session.model and agent.debug == {}
    session = DrivingSession(net2, dev, n_agents=1)
    for t in range(ticks):
        obs = {"rgb": frames[t, 0], "velocity": np.array([speeds[t, 0], 0.0, 0.0], dtype=np.float32), "command": int(commands[t, 0])}
        want = session.run_step(frames[t], [float(np.linalg.norm(obs["velocity"]))], commands[t])[0]
        if t % 2:
            control, wp = agent.run_step(obs, teaching=True)
            assert wp.shape == (5, 2) and wp.tobytes() == session.debug["waypoints"][0].tobytes()
        else:
            control = agent.run_step(obs)
        assert (control.steer, control.throttle, control.brake) == tuple(want) and control.manual_gear_shift is False
        assert agent.debug["target_speed"] == session.debug["target_speed"][0] and agent.debug["flags"] == session.debug["flags"][0]
    agent.reset()
    assert not agent.session.controller.state.cpu().numpy().any()
