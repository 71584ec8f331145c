"""The on-policy tick of phase 2: lbc_rollout_decide / lbc_rollout_stage_u8 (csrc/rollout.hip) against their numpy twins
(tests/rollout_twin.py), teaching.TeachingSession against its parts, training/rollout.py OnlineRollout against a restatement of the
reference's lists, and train_image_phase2 --env.

Kernel cases run on the CPU emulator (the unmodified kernel source) and, marked gpu, on the gfx950 library, where every launch sequence
runs helpers.REPEATS times from the same initial state with bit-identical results.  All comparisons are bitwise: decide selects and
copies doubles, stage copies bytes."""
import ctypes
import json

import numpy as np
import pytest
import torch

from learningbycheating_amd import _lib
from tests.helpers import WHERE, on_both, repeat
from tests.rollout_twin import DecideState, ReferenceBuffer, draw, np_decide, np_stage, reference_rollout

gpu = pytest.mark.gpu
SENTINEL, PAD, TICKS = 0xA5, 256, 6


def same(a, b):
    """bit for bit (NaN payloads and signed zeros included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. decide + stage against the twin -------------------------------------------------------------------------------------
def tick_inputs(rng, n, rgb_bytes, bv_bytes):
    """one tick's inputs; weights include NaN and infinities, the controller rows -0.0 and a NaN (values are moved, never computed on)"""
    student, teacher = rng.randn(n, 8), rng.randn(n, 8)
    student[:, 7], teacher[:, 7] = rng.randint(0, 4, size=n), rng.randint(0, 4, size=n)
    student[0, 1], teacher[0, 2] = -0.0, np.nan
    weight = rng.rand(n).astype(np.float32)
    weight[rng.rand(n) < 0.25] = np.float32(rng.choice([np.nan, np.inf, -np.inf]))
    speed = (rng.rand(n) * 10).astype(np.float32)
    onehot = np.zeros((n, 4), np.float32)
    onehot[np.arange(n), rng.randint(0, 4, size=n)] = 1
    return {"student": student, "teacher": teacher, "weight": weight, "speed": speed, "onehot": onehot,
            "rgb": rng.randint(0, 256, size=(n, rgb_bytes)).astype(np.uint8), "birdview": rng.randint(0, 256, size=(n, bv_bytes)).astype(np.uint8)}


def scenarios(n, cap):
    """(p_student, first tick, initial cursors, the mask of each tick or None)"""
    full = np.zeros(n, np.int32)
    full[n - 1] = cap                                                    # the last agent starts at capacity: its frames are dropped
    masks = [None, None] + [(np.arange(n) + t) % 3 != 0 for t in range(TICKS - 2)]       # ... then ticks with inactive agents
    masks[3] = np.zeros(n, bool)                                         # one tick with nobody active
    return [(0.5, (1 << 32) - 2, full, masks),                           # the counter's high word enters the hash at the third tick
            (0.0, 0, np.zeros(n, np.int32), [None] * TICKS),
            (1.0, 7, np.minimum(np.arange(n), cap).astype(np.int32), [None] * TICKS)]


def k_ticks(dev, n, cap, rgb_bytes, bv_bytes, seed, p, tick0, cursor0, masks, inputs):
    """TICKS consecutive decide + stage launches from one initial state on the device -> the same tuple np_ticks returns"""
    lib = _lib.get()
    init = DecideState(n, cap, tick0, p, cursor0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ins = [{k: up(v) for k, v in t.items()} for t in inputs]
    act = [None if m is None else up(m.astype(np.uint8)) for m in masks]
    p_dev = up(np.array([p], np.float64))

    def launch():
        tick = up(np.array([tick0], np.int64))
        cursor, dropped = up(init.cursor), up(init.dropped)
        meta = [up(init.slot_cmd), up(init.slot_speed), up(init.slot_weight)]
        stages = [torch.full((n * cap * b + 2 * PAD,), SENTINEL, dtype=torch.uint8, device=dev) for b in (rgb_bytes, bv_bytes)]
        outs = torch.full((TICKS, n, 16), -7.0, dtype=torch.float64, device=dev)
        slots = torch.full((TICKS, n), -9, dtype=torch.int32, device=dev)
        for t in range(TICKS):
            i = ins[t]
            _lib.check(lib.lbc_rollout_decide(_lib.ptr(i["student"]), _lib.ptr(i["teacher"]), _lib.ptr(i["weight"]), _lib.ptr(i["speed"]), _lib.ptr(i["onehot"]),
                                              _lib.ptr(act[t]), n, cap, seed, _lib.ptr(p_dev), _lib.ptr(tick), _lib.ptr(cursor), _lib.ptr(dropped),
                                              _lib.ptr(slots[t]), _lib.ptr(meta[0]), _lib.ptr(meta[1]), _lib.ptr(meta[2]), _lib.ptr(outs[t]),
                                              _lib.stream_for(outs)), "rollout_decide")
            _lib.check(lib.lbc_rollout_stage_u8(_lib.ptr(i["rgb"]), rgb_bytes, _lib.ptr(i["birdview"]), bv_bytes, _lib.ptr(slots[t]), n, n * cap,
                                                _lib.ptr(stages[0][PAD:]), _lib.ptr(stages[1][PAD:]), _lib.stream_for(outs)), "rollout_stage_u8")
        # (as integers: repeat compares with torch.equal, and NaN != NaN)
        return (outs.view(torch.int64), slots, cursor, dropped, tick, meta[0], meta[1].view(torch.int32), meta[2].view(torch.int32), stages[0], stages[1])
    got = [t.cpu().numpy() for t in repeat(dev, launch)]
    got[0], got[6], got[7] = got[0].view(np.float64), got[6].view(np.float32), got[7].view(np.float32)
    return got


def np_ticks(n, cap, rgb_bytes, bv_bytes, seed, p, tick0, cursor0, masks, inputs):
    st = DecideState(n, cap, tick0, p, cursor0)
    stages = [np.full(n * cap * b + 2 * PAD, SENTINEL, np.uint8) for b in (rgb_bytes, bv_bytes)]
    inner = [s[PAD:len(s) - PAD].reshape(n * cap, b) for s, b in zip(stages, (rgb_bytes, bv_bytes))]
    outs, slots = [], []
    for t in range(TICKS):
        i = inputs[t]
        out, slot = np_decide(st, seed, i["student"], i["teacher"], i["weight"], i["speed"], i["onehot"], masks[t])
        np_stage(i["rgb"], i["birdview"], slot, inner[0], inner[1])
        outs.append(out)
        slots.append(slot)
    return [np.stack(outs), np.stack(slots), st.cursor, st.dropped, np.array([st.tick], np.int64), st.slot_cmd, st.slot_speed, st.slot_weight] + stages


NAMES = ("rows", "slot", "cursor", "dropped", "tick", "slot_cmd", "slot_speed", "slot_weight", "rgb staging (with its canaries)", "bird-view staging (with its canaries)")


def check_ticks(dev, n, cap, rgb_bytes, bv_bytes, seed=11):
    for k, (p, tick0, cursor0, masks) in enumerate(scenarios(n, cap)):
        rng = np.random.RandomState(1000 * n + 10 * cap + k)
        inputs = [tick_inputs(rng, n, rgb_bytes, bv_bytes) for _ in range(TICKS)]
        args = (n, cap, rgb_bytes, bv_bytes, seed + k, p, tick0, cursor0, masks, inputs)
        got, want = k_ticks(dev, *args), np_ticks(*args)
        for name, g, w in zip(NAMES, got, want):
            assert same(g, w), (k, name)
        rows, slot = got[0], got[1]
        for t, m in enumerate(masks):
            if m is not None:
                assert not rows[t][~m].any() and (slot[t][~m] == -1).all(), "an inactive agent's row is all zero and its slot -1"
        assert int(got[4][0]) == tick0 + TICKS
        if k == 0:                                                     # the agent that started at capacity: counted, its slots untouched
            assert got[3][n - 1] == sum(1 for m in masks if m is None or m[n - 1]) and got[2][n - 1] == cap
            assert same(got[7][(n - 1) * cap:], DecideState(n, cap).slot_weight[(n - 1) * cap:])
        if p in (0.0, 1.0):
            assert (rows[..., 3] == p).all()


SMALL = [(n, cap, rows) for n in (1, 3, 5) for cap in (1, 4) for rows in ((48, 16), (80, 112))]


@pytest.mark.parametrize("case", on_both("case", SMALL, real=[pytest.param((2, 3, (184320, 258048)), marks=gpu, id="real_rows-gfx950")]))
def test_decide_and_stage_equal_the_twin(env, case):
    """six consecutive ticks from one initial state, three scenarios per shape: p_student 0.5 with a tick counter that starts at 2^32 - 2,
    masked ticks, a tick with nobody active and one agent at capacity from the start; p_student 0; p_student 1 with staggered cursors.  The
    (N,16) rows, slots, cursors, dropped counts, the counter, the slots' cmd / speed / weight and every byte of both staging arrays and the
    canaries around them equal the twin's.  The gpu-only case moves the real rows (184,320 and 258,048 bytes) at N = 2, capacity 3."""
    n, cap, (rgb_bytes, bv_bytes) = case
    check_ticks(env[0], n, cap, rgb_bytes, bv_bytes)


@pytest.mark.parametrize("where", WHERE)
def test_stage_wide_launch(env, where):
    """128 agents x 8,196 words = 1.05 M words: the four-words-per-lane form of the copy.  An agent's run is eight whole spans and a last
    span of four words, and the camera row ends one word into the fifth span, so one workgroup's lanes split between the two kinds; slots
    are a permutation with holes, every eighth agent has none (-1) and one slot lies outside the staging rows (nothing moves)"""
    dev, _ = env
    n, rows, rgb_bytes, bv_bytes = 128, 160, 64 * 1024 + 16, 64 * 1024 + 48
    assert n * (rgb_bytes + bv_bytes) // 16 >= 1 << 20 and (rgb_bytes // 16) % 1024 == 1 and ((rgb_bytes + bv_bytes) // 16) % 1024 == 4
    rng = np.random.RandomState(17)
    rgb, bv = rng.randint(0, 256, size=(n, rgb_bytes)).astype(np.uint8), rng.randint(0, 256, size=(n, bv_bytes)).astype(np.uint8)
    slot = rng.permutation(rows)[:n].astype(np.int32)
    slot[::8] = -1
    slot[3] = rows
    rgb_d, bv_d, slot_d = (torch.from_numpy(a).to(dev) for a in (rgb, bv, slot))

    def launch():
        stages = [torch.full((rows * b + 2 * PAD,), SENTINEL, dtype=torch.uint8, device=dev) for b in (rgb_bytes, bv_bytes)]
        _lib.check(_lib.get().lbc_rollout_stage_u8(_lib.ptr(rgb_d), rgb_bytes, _lib.ptr(bv_d), bv_bytes, _lib.ptr(slot_d), n, rows, _lib.ptr(stages[0][PAD:]),
                                                   _lib.ptr(stages[1][PAD:]), _lib.stream_for(rgb_d)), "rollout_stage_u8")
        return tuple(stages)
    got = [t.cpu().numpy() for t in repeat(dev, launch)]
    want = [np.full(rows * b + 2 * PAD, SENTINEL, np.uint8) for b in (rgb_bytes, bv_bytes)]
    np_stage(rgb, bv, np.where(slot < rows, slot, -1), *[w[PAD:len(w) - PAD].reshape(rows, b) for w, b in zip(want, (rgb_bytes, bv_bytes))])
    assert same(got[0], want[0]) and same(got[1], want[1])


# ---- 2. the draw ------------------------------------------------------------------------------------------------------------
DRAW_SEED = 3


@pytest.mark.parametrize("where", WHERE)
def test_draw_equals_the_twin_and_has_the_share(env, where):
    """64 agents x 64 ticks at p_student = 0.7: `who` is the twin's bit for bit, and the student's share lies within four standard
    deviations of 0.7 (sqrt(4096 x 0.7 x 0.3) = 29.3; +-118 of 4,096) -- for the twin alone too, which is how DRAW_SEED was picked"""
    dev, _ = env
    n, ticks, p = 64, 64, 0.7
    want = np.array([[draw(DRAW_SEED, t, a) < p for a in range(n)] for t in range(ticks)])
    assert abs(int(want.sum()) - p * n * ticks) <= 118, int(want.sum())
    lib = _lib.get()
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
    ctl, onehot, weight, speed = z(n, 8, dt=torch.float64), z(n, 4), z(n), z(n)
    onehot[:, 0] = 1
    p_dev = torch.tensor([p], dtype=torch.float64).to(dev)

    def launch():
        tick, cursor, dropped, slot = z(1, dt=torch.int64), z(n, dt=torch.int32), z(n, dt=torch.int32), z(n, dt=torch.int32)
        meta = [z(n * ticks, dt=torch.int32), z(n * ticks), z(n * ticks)]
        outs = z(ticks, n, 16, dt=torch.float64)
        for t in range(ticks):
            _lib.check(lib.lbc_rollout_decide(_lib.ptr(ctl), _lib.ptr(ctl), _lib.ptr(weight), _lib.ptr(speed), _lib.ptr(onehot), None, n, ticks, DRAW_SEED,
                                              _lib.ptr(p_dev), _lib.ptr(tick), _lib.ptr(cursor), _lib.ptr(dropped), _lib.ptr(slot), _lib.ptr(meta[0]),
                                              _lib.ptr(meta[1]), _lib.ptr(meta[2]), _lib.ptr(outs[t]), _lib.stream_for(outs)), "rollout_decide")
        return outs, cursor, dropped
    outs, cursor, dropped = [t.cpu().numpy() for t in repeat(dev, launch)]
    assert np.array_equal(outs[..., 3] == 1.0, want) and np.isin(outs[..., 3], (0.0, 1.0)).all()
    assert (cursor == ticks).all() and not dropped.any()
    assert abs(int(outs[..., 3].sum()) - p * n * ticks) <= 118


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_refusals_launch_nothing(env, where):
    """a null pointer, N outside 1..1024, capacity < 1, row bytes that are no multiple of 16, no staging rows: a negative code, a message
    that starts with the entry point's name, and every array keeps its bytes"""
    dev, _ = env
    lib = _lib.get()
    n, cap = 3, 2
    t = lambda *shape, dt=torch.float32, fill=5: torch.full(shape, fill, dtype=dt, device=dev)
    a = {"student": t(n, 8, dt=torch.float64), "teacher": t(n, 8, dt=torch.float64), "weight": t(n), "speed": t(n), "onehot": t(n, 4),
         "p": t(1, dt=torch.float64), "tick": t(1, dt=torch.int64), "cursor": t(n, dt=torch.int32, fill=0), "dropped": t(n, dt=torch.int32),
         "slot": t(n, dt=torch.int32), "slot_cmd": t(n * cap, dt=torch.int32), "slot_speed": t(n * cap), "slot_weight": t(n * cap),
         "out": t(n, 16, dt=torch.float64)}
    before = {k: v.clone() for k, v in a.items()}

    def decide(n=n, cap=cap, **kw):
        p = {k: _lib.ptr(v) for k, v in a.items()}
        p.update(kw)
        return lib.lbc_rollout_decide(p["student"], p["teacher"], p["weight"], p["speed"], p["onehot"], None, n, cap, 1, p["p"], p["tick"], p["cursor"],
                                      p["dropped"], p["slot"], p["slot_cmd"], p["slot_speed"], p["slot_weight"], p["out"], None)
    msg = lambda: lib.lbc_last_error().decode()
    for k in a:
        assert decide(**{k: None}) < 0 and msg().startswith("rollout_decide:") and "null" in msg(), k
    for kw, word in ((dict(n=0), "N = 0"), (dict(n=-1), "N = -1"), (dict(n=1025), "N = 1025"), (dict(cap=0), "capacity = 0"), (dict(cap=-3), "capacity = -3")):
        assert decide(**kw) < 0 and msg().startswith("rollout_decide:") and word in msg(), kw
    rgb, bv = t(n, 48, dt=torch.uint8), t(n, 32, dt=torch.uint8)
    rs, bs = t(n * cap, 48, dt=torch.uint8, fill=9), t(n * cap, 32, dt=torch.uint8, fill=9)
    slot = torch.arange(n, dtype=torch.int32).to(dev)

    def stage(rgb=rgb, rb=48, bv=bv, bb=32, slot=slot, n=n, rows=n * cap, rs=rs, bs=bs):
        return lib.lbc_rollout_stage_u8(_lib.ptr(rgb), rb, _lib.ptr(bv), bb, _lib.ptr(slot), n, rows, _lib.ptr(rs), _lib.ptr(bs), None)
    for kw in (dict(rgb=None), dict(bv=None), dict(slot=None), dict(rs=None), dict(bs=None)):
        assert stage(**kw) < 0 and msg().startswith("rollout_stage_u8:") and "null" in msg(), kw
    for kw, word in ((dict(rb=40), "row_bytes"), (dict(bb=8), "row_bytes"), (dict(rb=0), "row_bytes"), (dict(bb=-16), "row_bytes"), (dict(n=0), "N = 0"),
                     (dict(n=1025), "N = 1025"), (dict(rows=0), "stage_rows = 0")):
        assert stage(**kw) < 0 and msg().startswith("rollout_stage_u8:") and word in msg(), kw
    for k, v in a.items():
        assert torch.equal(v, before[k]), k
    assert bool((rs == 9).all()) and bool((bs == 9).all())
    assert decide() == 0 and stage() == 0
    assert a["cursor"].cpu().tolist() == [1, 1, 1] and int(a["tick"].cpu()) == 6 and torch.equal(rs[:n].cpu(), rgb.cpu())


# ---- stand-in networks (cases 6 and the emulator) -----------------------------------------------------------------------------
TINY_RGB, TINY_BV, TINY_MAP, TINY_ORIGIN = (4, 4), (4, 4), 8, (3, 2)


class StandInEngine:
    """what TeachingSession asks of an engine: forward(frames u8, speed, command, train) -> (selected waypoints (N,5,2) f32, None).  Two fixed
    functions of the batch, as tests/test_phase2_dataset.py StandInTrainer: camera-space waypoints from the camera frames' means, the command
    and the speed; map-space waypoints from the bird-view frames' means.  A speed above 9 m/s puts the student's waypoints ON the horizon
    row, where the unprojection has its pole: that frame's weight is not finite."""

    def __init__(self, kind, max_batch):
        self.kind, self.max_batch = kind, max_batch

    def forward(self, x, speed, command, train):
        assert not train and x.dtype == torch.uint8
        n = x.shape[0]
        m = x.reshape(n, -1).float().mean(1) / 255
        t = torch.arange(5, dtype=torch.float32, device=x.device)
        if self.kind == "student":
            branch = command.argmax(1).float()
            y = 0.3 + 0.1 * t[None] + 0.01 * speed[:, None]
            y = torch.where(speed[:, None] > 9.0, torch.zeros_like(y), y)
            sel = torch.stack([(m - 0.5 + 0.05 * branch)[:, None] * (1 + t) * 0.2, y], -1)
        else:
            sel = torch.stack([(m - 0.05)[:, None] * (1 + t), 0.35 + 0.1 * t[None].expand(n, 5)], -1)
        return sel.contiguous(), None


class StandInModel:
    def __init__(self, kind):
        self.kind, self.input_channel = kind, 3 if kind == "student" else 7
        self.input_hw = TINY_RGB if kind == "student" else TINY_BV
        self._engines = {}

    def engine(self, shape, device, max_batch=None, with_grads=True):
        return self._engines.setdefault("only", StandInEngine(self.kind, max_batch or shape[0]))


def tiny_session(dev, n, capacity, seed=4):
    from learningbycheating_amd.teaching import TeachingSession
    return TeachingSession(StandInModel("student"), StandInModel("teacher"), dev, n, capacity, seed=seed, map_size=TINY_MAP, crop_origin=TINY_ORIGIN)


def tiny_buffer(dev, limit):
    from learningbycheating_amd.training.replay import DeviceReplayBuffer
    return DeviceReplayBuffer(dev, buffer_limit=limit, seed=1, rgb_shape=TINY_RGB + (3,), birdview_shape=TINY_BV + (7,))


def buffer_samples(buf):
    n = len(buf)
    rgb, bv = buf.rgb[:n].cpu().numpy(), buf.birdview[:n].cpu().numpy()
    cmd, speed, w = buf.cmd[:n].cpu().numpy(), buf.speed[:n].cpu().numpy(), buf.weights[:n].cpu().numpy()
    return sorted((rgb[i].tobytes(), bv[i].tobytes(), int(cmd[i]), speed[i:i + 1].view(np.uint32).item(), w[i:i + 1].view(np.uint32).item()) for i in range(n))


def crop_of(maps, origin=TINY_ORIGIN, hw=TINY_BV):
    return maps[:, origin[0]:origin[0] + hw[0], origin[1]:origin[1] + hw[1]]


class Recorder:
    """spies on session.run_step: per environment the list of what the reference's loop would have seen at every tick the environment took
    part in -- the datum it appends, the weight, and (filled in at the next observation) the flags after the tick's apply"""

    def __init__(self, session, env, origin=TINY_ORIGIN, hw=TINY_BV):
        self.ticks = [[] for _ in range(session.n_agents)]
        self.who = []
        run_step, observe = session.run_step, env.observe

        def spy_step(rgb, maps, speeds, commands, active=None):
            controls = run_step(rgb, maps, speeds, commands, active)
            d = session.debug
            for i in range(session.n_agents):
                if active is None or active[i]:
                    datum = {"rgb": np.ascontiguousarray(rgb[i]).tobytes(), "birdview": np.ascontiguousarray(crop_of(np.asarray(maps), origin, hw)[i]).tobytes(),
                             "cmd": int(commands[i]), "speed": np.array([speeds[i]], np.float32).view(np.uint32).item()}
                    self.ticks[i].append([datum, np.float32(d["weight"][i]), None, None])
                    self.who.append(int(d["who"][i]))
                    assert same(controls[i], d["student"][i] if d["who"][i] else d["teacher"][i])
            return controls

        def spy_observe():
            obs = observe()
            for i, rec in enumerate(self.ticks):
                if rec and rec[-1][2] is None:
                    rec[-1][2], rec[-1][3] = bool(obs["done"][i] or obs["collided"][i]), bool(obs["collided"][i])
            return obs
        session.run_step, env.observe = spy_step, spy_observe


def reference_counts(recorder, ref, episode_length):
    """the reference's loop replayed per environment, in order, over what the recorder saw -> [(ticks, collisions, skipped)] per environment"""
    out = []
    for i, ticks in enumerate(recorder.ticks):
        it = iter(ticks)
        out.append(reference_rollout(ref, lambda _len: tuple(next(it)), episode_length))
        assert next(it, None) is None, "the rollout ticked environment %d more often than the reference's loop does" % i
        recorder.ticks[i] = []
    return out


@pytest.mark.parametrize("n_envs", [1, 3])
@pytest.mark.parametrize("where", WHERE)
def test_online_rollout_equals_the_reference_lists(env, where, n_envs):
    """SyntheticEnv with scripted ends -- a collision, a second one two ticks into the episode that follows, a plain `done` -- three
    rollouts of episode_length 7 into 16 slots (eviction from the second rollout on with one environment, inside the first with three):
    after every rollout the buffer's (frame bytes, bird-view crop bytes, cmd, speed, weight) set equals the reference's lists
    (train_image_phase2.py:86-149, one list per environment) pushed through ReplayBuffer.add_data (phase2_utils.py:256-265); ticks,
    collisions and the frames left out for a non-finite weight are the restatement's; nothing is dropped"""
    from learningbycheating_amd.training.envs import SyntheticEnv
    from learningbycheating_amd.training.rollout import OnlineRollout
    dev, _ = env
    L, limit = 7, 16
    script = {0: {4: "collided", 6: "collided", 13: "done", 25: "collided"}, 1: {3: "done", 9: "collided"}, 2: {7: "collided", 30: "done"}}
    sim = SyntheticEnv(n_envs, pool=12, seed=5, script=script, rgb_hw=TINY_RGB, map_size=TINY_MAP)
    session, buf = tiny_session(dev, n_envs, L), tiny_buffer(dev, limit)
    rec = Recorder(session, sim)
    ro = OnlineRollout(session, buf, sim, L)
    ref = ReferenceBuffer(limit)
    seen, skipped_total = [], 0
    for episode in range(3):
        out = ro.run(episode)
        weights = [t[1] for ticks in rec.ticks for t in ticks]
        seen += [float(w) for w in weights if np.isfinite(w)]
        counts = reference_counts(rec, ref, L)
        collisions, skipped = sum(c[1] for c in counts), sum(c[2] for c in counts)
        skipped_total += skipped
        assert out["dropped"] == 0 and out["collisions"] == collisions and out["skipped_nonfinite"] == skipped
        assert out["frames"] == n_envs * L - skipped and out["n"] == len(buf) == min(limit, len(ref.data))
        assert buffer_samples(buf) == ref.samples(), episode
        assert out["ticks"] == max(c[0] for c in counts) and out["student_share"] == float(np.mean(rec.who))
        rec.who = []
    assert len(set(seen)) == len(seen), "the restatement needs distinct weights (argsort picks among equal ones)"
    assert skipped_total >= 1, "no frame with a non-finite weight was met: the case does not cover it"
    assert len(ref.data) == limit and (3 * n_envs * L - skipped_total) > limit, "nothing was evicted"
    sim.close()


@pytest.mark.parametrize("where", WHERE)
def test_session_trim_commit_and_state(env, where):
    """end_episode(collided) takes five staged ticks or as many as there are; commit hands the rows over in agent order, zeroes the cursors
    and counts; state_dict / load_state_dict continue the draws, the cursors and both controllers bit for bit; a buffer over a dataset
    and a short staging are refused"""
    from learningbycheating_amd.training.rollout import OnlineRollout
    dev, _ = env
    n, cap = 2, 9
    rng = np.random.RandomState(8)
    frames = lambda: (rng.randint(0, 256, size=(n,) + TINY_RGB + (3,)).astype(np.uint8), rng.randint(0, 256, size=(n, TINY_MAP, TINY_MAP, 7)).astype(np.uint8),
                      rng.rand(n) * 9, rng.randint(1, 5, size=n))
    a, b = tiny_session(dev, n, cap, seed=21), tiny_session(dev, n, cap, seed=99)
    a.set_episode(3)
    assert a.p_student == 0.5 + 0.5 * (1 - 0.95 ** 3)
    fed = [frames() for _ in range(8)]
    for f in fed[:3]:
        a.run_step(*f)
    a.end_episode([1], collided=True)                                     # three staged: all of them go
    assert a.cursor.cpu().tolist() == [3, 0]
    for f in fed[3:5]:
        a.run_step(*f, active=[1, 0])
    b.load_state_dict(a.state_dict())
    for f in fed[5:]:
        ca, cb = a.run_step(*f), b.run_step(*f)
        assert same(ca, cb) and all(same(a.debug[k], b.debug[k]) for k in a.debug)
    assert a.debug["staged"].tolist() == [8, 3] and not a.debug["dropped"].any()
    a.end_episode([0, 1], collided=[True, False])
    assert a.cursor.cpu().tolist() == [3, 3]
    buf = tiny_buffer(dev, 16)
    out = a.commit(buf)
    assert out == {"frames": 6, "skipped_nonfinite": 0, "dropped": 0, "n": 6} and a.cursor.cpu().tolist() == [0, 0]
    want = np.concatenate([np.stack([f[0][0] for f in fed[:3]]), np.stack([f[0][1] for f in fed[5:]])])
    assert same(buf.rgb[:6].cpu().numpy(), want)
    want = np.concatenate([np.stack([crop_of(f[1])[0] for f in fed[:3]]), np.stack([crop_of(f[1])[1] for f in fed[5:]])])
    assert same(buf.birdview[:6].cpu().numpy(), np.ascontiguousarray(want))
    assert buf.cmd[:6].cpu().tolist() == [int(f[3][0]) for f in fed[:3]] + [int(f[3][1]) for f in fed[5:]]
    assert same(buf.speed[:6].cpu().numpy(), np.array([f[2][0] for f in fed[:3]] + [f[2][1] for f in fed[5:]], np.float32))
    for _ in range(cap + 2):                                              # a staging of 9 rows and eleven ticks: two are dropped and counted
        a.run_step(*fed[0])
    assert a.debug["dropped"].tolist() == [1, 1] and a.debug["staged"].tolist() == [cap, cap]
    assert a.commit(buf)["dropped"] == 4
    with pytest.raises(ValueError, match="capacity"):
        OnlineRollout(a, buf, type("E", (), {"n_envs": n})(), cap + 1)
    with pytest.raises(ValueError, match="environments"):
        OnlineRollout(a, buf, type("E", (), {"n_envs": n + 1})(), cap)
    with pytest.raises(ValueError, match="frame indices"):
        a.commit(type("B", (), {"source": object()})())


def test_single_env_adapter_speaks_the_reference_interface():
    """tick / get_observations / apply_control / is_success / collided (train_image_phase2.py:111-123) -> the protocol: one tick per
    observation however often observe() is called, a fresh environment per reset, speed = |velocity|"""
    from learningbycheating_amd.training.rollout import SingleEnvAdapter
    made = []

    class Env:
        def __init__(self, index):
            self.index, self.ticks, self.applied, self.collided, self.closed = index, 0, [], False, False
            made.append(self)

        def tick(self):
            self.ticks += 1

        def get_observations(self):
            return {"rgb": np.full((2, 2, 3), self.ticks, np.uint8), "birdview": np.zeros((4, 4, 7), np.uint8), "velocity": np.array([3.0, 4.0, 0.0]),
                    "command": 2 + self.index}

        def apply_control(self, c):
            self.applied.append(c)
            self.collided = len(self.applied) == 2 and self.index == 1

        def is_success(self):
            return len(self.applied) == 3

        def close(self):
            self.closed = True
    ad = SingleEnvAdapter(Env, 2, make_control=lambda s, t, b: (s, t, b))
    ad.reset([0, 1])
    o = ad.observe()
    o = ad.observe()
    assert o["rgb"].shape == (2, 2, 2, 3) and o["rgb"].max() == 1 and o["speed"].tolist() == [5.0, 5.0] and o["command"].tolist() == [2, 3]
    ad.apply(np.array([[0.1, 0.2, 0.0], [0.3, 0.4, 0.5]]))
    ad.apply(np.array([[0.1, 0.2, 0.0], [0.3, 0.4, 0.5]]))
    o = ad.observe()
    assert o["collided"].tolist() == [False, True] and o["done"].tolist() == [False, False] and made[1].applied[0] == (0.3, 0.4, 0.5)
    ad.reset([1])
    assert made[1].closed and len(made) == 3 and ad.observe()["rgb"][:, 0, 0, 0].tolist() == [2, 1]
    ad.close()
    assert made[0].closed and made[2].closed


# ---- 4. / 5. the session on the real networks (gpu) -----------------------------------------------------------------------------
def real_models(dev, student_state=None):
    """(student, teacher): a ResNet-34 camera student with the warm-started weights of tests/test_replay_device.py warm_student and a seeded
    ResNet-18 bird-view teacher, fp32"""
    from learningbycheating_amd.bird_view.models.birdview import BirdViewPolicyModelSS
    from learningbycheating_amd.bird_view.models.image import ImagePolicyModelSS
    student = ImagePolicyModelSS("resnet34", all_branch=True).to(dev)
    student.load_state_dict(student_state)
    torch.manual_seed(71)
    teacher = BirdViewPolicyModelSS("resnet18", all_branch=True).to(dev)
    return student, teacher


@pytest.fixture(scope="module")
def warm_state():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests.test_replay_device import warm_student
    _lib._inject_for_tests(None)
    return {k: v.detach().clone() for k, v in warm_student(torch.device("cuda", 0)).state_dict().items()}


def real_frames(seed, n, ticks):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(ticks):
        out.append((torch.randint(0, 256, (n, 160, 384, 3), generator=g, dtype=torch.uint8).numpy(),
                    ((torch.rand((n, 320, 320, 7), generator=g) < 0.1).to(torch.uint8) * 255).numpy(),
                    (torch.rand(n, generator=g) * 10).numpy().astype(np.float64), torch.randint(1, 5, (n,), generator=g).numpy()))
    return out


@gpu
def test_session_equals_its_parts(env, warm_state):
    """N = 3, ten ticks with a masked tick and a reset of one agent: the student's and the teacher's controls and waypoints are bitwise those
    of two DrivingSessions fed the same frames; the weight is bitwise lbc_phase2_weight on those waypoints; graph replay equals eager launches;
    the applied control is the row `who` names; the staged camera frames, bird-view crops (rows 58..250, columns 64..256 of the map), commands
    and speeds are the uploaded ones"""
    from learningbycheating_amd.agent import DrivingSession
    from learningbycheating_amd.teaching import TeachingSession
    from learningbycheating_amd.training.native import camera_struct
    dev, _ = env
    n, ticks, cap = 3, 10, 12
    student, teacher = real_models(dev, warm_state)
    graph = TeachingSession(student, teacher, dev, n, cap, seed=9)
    eager = TeachingSession(student, teacher, dev, n, cap, seed=9, use_graph=False)
    assert graph.graph is not None and eager.graph is None
    ds, dt = DrivingSession(student, dev, n_agents=n), DrivingSession(teacher, dev, n_agents=n)
    cam, lib = camera_struct(), _lib.get()
    fed = real_frames(81, n, ticks)
    whos = []
    for t, (rgb, maps, speeds, commands) in enumerate(fed):
        active = [1, 0, 1] if t == 4 else None
        if t == 6:
            for s in (graph, eager):
                s.end_episode([1], collided=False)
            ds.reset([1])
            dt.reset([1])
        c = graph.run_step(rgb, maps, speeds, commands, active)
        ce = eager.run_step(rgb, maps, speeds, commands, active)
        cs, ct = ds.run_step(rgb, speeds, commands, active), dt.run_step(maps, speeds, commands, active)
        d = graph.debug
        assert same(ce, c) and all(same(eager.debug[k], d[k]) for k in d), "graph replay differs from eager launches at tick %d" % t
        live = [i for i in range(n) if active is None or active[i]]
        assert same(d["student"][live], cs[live]) and same(d["teacher"][live], ct[live]), t
        assert same(d["student_waypoints"], ds.debug["waypoints"]) and same(d["teacher_waypoints"], dt.debug["waypoints"]), t
        assert same(d["student_flags"][live], ds.debug["flags"][live]) and same(d["teacher_flags"][live], dt.debug["flags"][live])
        w = torch.empty(n, dtype=torch.float32, device=dev)
        sw, tw = torch.from_numpy(ds.debug["waypoints"]).to(dev), torch.from_numpy(dt.debug["waypoints"]).to(dev)
        _lib.check(lib.lbc_phase2_weight(ctypes.byref(cam), _lib.ptr(sw), _lib.ptr(tw), n, _lib.ptr(w), _lib.stream_for(w)), "phase2_weight")
        assert same(d["weight"][live], w.cpu().numpy()[live]), t
        for i in range(n):
            if i in live:
                assert same(c[i], d["student"][i] if d["who"][i] else d["teacher"][i])
            else:
                assert not c[i].any() and d["staged"][i] == 0 and d["who"][i] == 0
        whos.append(d["who"][live])
    assert {0, 1} == set(np.concatenate(whos).tolist()), "ten ticks at p_student = 0.5 with both drivers"
    assert graph.debug["staged"].tolist() == [ticks, ticks - 1, ticks] and not graph.debug["dropped"].any()
    for s in (graph, eager):
        for i in range(n):
            mine = [t for t in range(ticks) if not (t == 4 and i == 1)]
            rows = slice(i * cap, i * cap + len(mine))
            assert same(s.rgb_stage[rows].cpu().numpy(), np.stack([fed[t][0][i] for t in mine]))
            assert same(s.birdview_stage[rows].cpu().numpy(), np.ascontiguousarray(np.stack([fed[t][1][i, 58:250, 64:256] for t in mine])))
            assert s.slot_cmd[rows].cpu().tolist() == [int(fed[t][3][i]) for t in mine]
            assert same(s.slot_speed[rows].cpu().numpy(), np.array([fed[t][2][i] for t in mine], np.float32))


@gpu
def test_session_follows_trained_weights_and_replaced_engines(env, warm_state):
    """the session replays its graph on the engine NativeTrainer trains on: after one step the next tick's student waypoints equal a fresh
    eager eval forward's and differ from the tick before, and the step itself is bitwise the step of a run with no tick in between; after a
    module-API forward at batch N + 1 replaced the cached engine, the session captures again and the next tick equals a freshly built
    session's"""
    from learningbycheating_amd.teaching import TeachingSession
    from learningbycheating_amd.training.native import NativeTrainer
    dev, _ = env
    n, cap = 3, 8
    fed = real_frames(82, n, 4)
    g = torch.Generator().manual_seed(83)
    batch = (torch.randint(0, 256, (n, 160, 384, 3), generator=g, dtype=torch.uint8).to(dev), (torch.rand(n, generator=g) * 10).to(dev),
             torch.eye(4)[:n].contiguous().to(dev), ((torch.rand((n, 192, 192, 7), generator=g) < 0.1).to(torch.uint8) * 255).to(dev))

    def run(with_ticks):
        student, teacher = real_models(dev, warm_state)
        session = TeachingSession(student, teacher, dev, n, cap, seed=5) if with_ticks else None
        trainer = NativeTrainer(student, teacher, n, (3, 160, 384), dev, phase=1, lr=1e-3)
        before = None
        if session is not None:
            session.run_step(*fed[0])
            before = session.debug["student_waypoints"]
        trainer.step(batch[0], batch[1], batch[2], birdview=batch[3])
        torch.cuda.synchronize()
        params = {k: v.detach().clone() for k, v in student.state_dict().items()}
        return student, teacher, session, trainer, before, params
    _, _, _, _, _, plain = run(False)
    student, teacher, session, trainer, before, params = run(True)
    for k in plain:
        assert torch.equal(plain[k], params[k]), "the step after a tick differs from the step alone in %s" % k
    assert session.captures == 1
    session.run_step(*fed[0])                                             # the same frames as before the step
    after = session.debug["student_waypoints"]
    assert session.captures == 1 and not same(after, before)
    onehot = torch.zeros((n, 4), device=dev)
    onehot[torch.arange(n), torch.from_numpy(fed[0][3]).to(dev) - 1] = 1
    sel, _ = trainer.eng.forward(torch.from_numpy(fed[0][0]).to(dev), torch.from_numpy(fed[0][2]).float().to(dev), onehot, False)
    assert same(after, sel.cpu().numpy())
    # a larger batch through the module API replaces the cached engine
    eng = session.s_eng
    student.eval()
    with torch.no_grad():
        student(torch.rand((n + 1, 3, 160, 384), device=dev), torch.rand(n + 1, device=dev), torch.eye(4).to(dev)[:n + 1].contiguous())
    assert not any(e is eng for e in student._engines.values())
    fresh = TeachingSession(student, teacher, dev, n, cap, seed=5)
    fresh.load_state_dict(session.state_dict())
    c = session.run_step(*fed[1])
    assert session.captures == 2 and session.s_eng is not eng and any(e is session.s_eng for e in student._engines.values())
    cf = fresh.run_step(*fed[1])
    assert same(c, cf) and all(same(session.debug[k], fresh.debug[k]) for k in fresh.debug)


# ---- 7. the script --------------------------------------------------------------------------------------------------------------
ENV_KWARGS = {"pool": 8, "seed": 2, "script": {"0": {"4": "collided", "15": "done"}, "1": {"3": "collided"}}}
SCRIPT = ["--batch_size", "4", "--precision", "fp32", "--log_iterations", "1", "--replay", "device", "--env", "synthetic", "--n_envs", "2",
          "--episode_length", "6", "--buffer_limit", "16", "--env_kwargs", json.dumps(ENV_KWARGS), "--epoch_per_episode", "1", "--seed", "3", "--save_state"]


@pytest.fixture(scope="module")
def warm_ckpt(tmp_path_factory, warm_state):
    path = tmp_path_factory.mktemp("online_warm") / "student.th"
    torch.save(warm_state, str(path))
    return str(path)


def run_script(tmp, warm_ckpt, episodes, extra=()):
    """-> (what main returns, [(the rollout's record, the reference's per-environment counts)] per rollout of this run)"""
    from learningbycheating_amd.training import train_image_phase2 as P2
    from learningbycheating_amd.training.rollout import OnlineRollout
    seen, run, spies = [], OnlineRollout.run, {}

    def spy(self, episode):
        if id(self) not in spies:
            spies[id(self)] = (Recorder(self.session, self.env, origin=(58, 64), hw=(192, 192)), ReferenceBuffer(self.buffer.buffer_limit))
        rec, ref = spies[id(self)]
        ref.data, ref.weights = [], []                                     # the epochs since the last rollout wrote new weights into the buffer
        if len(self.buffer):
            for s in buffer_samples(self.buffer):
                ref.add_data({"rgb": s[0], "birdview": s[1], "cmd": s[2], "speed": s[3]}, np.array([s[4]], np.uint32).view(np.float32)[0])
        out = run(self, episode)
        seen.append((dict(out), reference_counts(rec, ref, self.episode_length), ref.samples() == buffer_samples(self.buffer)))
        return out
    OnlineRollout.run = spy
    try:
        out = P2.main(["--log_dir", str(tmp), "--ckpt", warm_ckpt, "--max_episode", str(episodes)] + SCRIPT + list(extra))
    finally:
        OnlineRollout.run = run
    torch.cuda.synchronize()
    return out, seen


@pytest.fixture(scope="module")
def full_run(tmp_path_factory, warm_ckpt):
    tmp = tmp_path_factory.mktemp("online_full")
    return (tmp,) + run_script(tmp, warm_ckpt, 3)


@gpu
def test_script_trains_on_policy(env, full_run):
    """three episodes at batch 4 with two synthetic environments, six frames each, into 16 slots: log.jsonl carries the new keys with the
    counts of the reference's lists replayed over what the session saw, the buffer after every rollout is the restatement's, model-2.th
    exists, config.json gains the new keys, the state carries the buffer's frames"""
    tmp, out, seen = full_run
    assert len(seen) == 3 and (tmp / "model-2.th").exists()
    log = [json.loads(l) for l in open(tmp / "log.jsonl")]
    assert len(log) == 3
    for episode, ((rec, counts, equal), line) in enumerate(zip(seen, log)):
        skipped = sum(c[2] for c in counts)
        want = {"rollout_frames": 12 - skipped, "rollout_ticks": max(c[0] for c in counts), "rollout_collisions": sum(c[1] for c in counts),
                "rollout_skipped_nonfinite": skipped, "buffer_size": min(16, sum(12 - sum(c[2] for c in s[1]) for s in seen[:episode + 1]))}
        for k, v in want.items():
            assert line["train_" + k]["mean"] == v and line["train_" + k]["n"] == 1, (episode, k, line["train_" + k], v)
        assert line["train_rollout_student_share"]["mean"] == rec["student_share"] and 0.0 <= rec["student_share"] <= 1.0
        assert rec["dropped"] == 0 and equal, episode
    assert sum(sum(c[1] for c in s[1]) for s in seen) >= 2, "the scripted collisions were not met"
    print("rollout records:", [s[0] for s in seen])
    buf = out["buffer"]
    assert len(buf) == 16 and buf.normalized
    config = json.loads((tmp / "config.json").read_text())
    assert (config["env"], config["n_envs"], config["episode_length"], config["beta"], config["buffer_limit"]) == ("synthetic", 2, 6, 0.95, 16)
    assert config["env_kwargs"] == ENV_KWARGS
    state = torch.load(str(tmp / "train_state.th"), map_location="cpu")
    assert tuple(state["buffer"]["rgb"].shape) == (16, 160, 384, 3) and tuple(state["buffer"]["birdview"].shape) == (16, 192, 192, 7)
    assert state["rollout"]["format"] == "online-1" and state["rollout"]["env"] is not None and not state["rollout"]["session"]["cursor"].any()


@gpu
def test_script_resume_is_bitwise(env, full_run, warm_ckpt, tmp_path):
    """stopped after episode 1 and continued with --resume: student, buffer (frames included), session and environment state equal the
    uninterrupted run bit for bit"""
    _, ref, ref_seen = full_run
    run_script(tmp_path, warm_ckpt, 2)
    state = torch.load(str(tmp_path / "train_state.th"), map_location="cpu")
    assert (state["episode"], state["epoch"]) == (1, 0)
    out, seen = run_script(tmp_path, warm_ckpt, 3, ["--resume"])
    assert len(seen) == 1 and seen[0][0] == ref_seen[2][0] and seen[0][1] == ref_seen[2][1] and seen[0][2]
    sa, sb = ref["net"].state_dict(), out["net"].state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    a, b = ref["buffer"], out["buffer"]
    assert len(a) == len(b) == 16 and a.draws == b.draws and a.normalized == b.normalized
    for name in ("rgb", "birdview", "cmd", "speed", "weights", "new_weights"):
        assert same(getattr(a, name)[:16].cpu().numpy(), getattr(b, name)[:16].cpu().numpy()), name

    def flat(sd, prefix=""):
        out = {}
        for k, v in sd.items():
            if isinstance(v, dict):
                out.update(flat(v, prefix + k + "."))
            else:
                out[prefix + k] = v.numpy().tobytes() if torch.is_tensor(v) else v
        return out
    assert flat(ref["rollout"].state_dict()) == flat(out["rollout"].state_dict())


def test_script_env_flags_and_config_keys(tmp_path):
    """--env with --replay host, with --dataset_dir, with --synthetic, with a malformed name or --env_kwargs, and the environment's flags
    without --env exit in build_config with their messages; a run without --env builds the config tests/test_phase2_dataset.py pins; with
    it, the new keys and only those"""
    from learningbycheating_amd.training import train_image_phase2 as P2
    from tests.test_phase2_dataset import PARENT_DEVICE_KEYS, PARENT_KEYS
    base = ["--log_dir", str(tmp_path)]
    dev = ["--replay", "device"]
    for extra, words in ((["--env", "synthetic"], ["--env", "--replay device"]),
                         (dev + ["--env", "synthetic", "--dataset_dir", "D"], ["--env", "--dataset_dir"]),
                         (dev + ["--env", "synthetic", "--synthetic", "64"], ["--env", "--synthetic"]),
                         (dev + ["--env", "nocolon"], ["MODULE:FACTORY"]),
                         (dev + ["--env", "synthetic", "--env_kwargs", "{"], ["--env_kwargs", "JSON"]),
                         (dev + ["--env", "synthetic", "--env_kwargs", "[1]"], ["--env_kwargs", "object"]),
                         (dev + ["--env", "synthetic", "--n_envs", "0"], ["--n_envs"]),
                         (dev + ["--n_envs", "2"], ["--n_envs", "--env"]),
                         (dev + ["--episode_length", "5", "--beta", "0.5"], ["--episode_length", "--beta", "--env"]),
                         (dev + ["--buffer_limit", "8"], ["--buffer_limit", "--dataset_dir"])):
        with pytest.raises(SystemExit) as e:
            P2.main(base + extra)
        assert all(w in str(e.value) for w in words), (extra, str(e.value))
    build = lambda argv: P2.build_config(P2.parse_arguments(base + argv), 0, 1, torch.device("cuda", 0))
    assert set(build([])) == PARENT_KEYS and set(build(dev)) == PARENT_KEYS | PARENT_DEVICE_KEYS
    assert set(build(dev + ["--dataset_dir", "D"])) == PARENT_KEYS | PARENT_DEVICE_KEYS | {"dataset_dir", "rollout_frames", "buffer_limit"}
    got = build(dev + ["--env", "pkg.mod:make", "--env_kwargs", '{"town": 1}', "--n_envs", "4", "--buffer_limit", "64"])
    assert set(got) == PARENT_KEYS | PARENT_DEVICE_KEYS | {"env", "env_kwargs", "n_envs", "episode_length", "beta", "buffer_limit"}
    assert (got["env"], got["env_kwargs"], got["n_envs"], got["episode_length"], got["beta"], got["buffer_limit"], got["synthetic_frames"]) == \
        ("pkg.mod:make", {"town": 1}, 4, 1000, 0.95, 64, False)
