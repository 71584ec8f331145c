"""The bits of the fused Adam step, anchored outside the code under test.

Every path of the step (lbc_adam_step, lbc_adam_step_guarded, lbc_adam_step_clipped and the four instantiations of
lbc_adam_step_recipe, one of them again under a cosine schedule with warm-up) runs four steps on test_resume_guard's SMALL_TABLE, laid
out as FusedAdam lays it out (64-element padding, 32768-element chunks, NaN in the padding of g).  Inputs come from
np.random.RandomState, whose stream does not change between versions.  Steps 1 and 2 are clipped (MAX_NORM lies below their norm), step 3
carries one +Inf in the last tail element of the 70001-element tensor and is skipped by every guarded path (the plain step, which has no
guard, is not called for it), step 4 is clean and not clipped.  Weight decay is non-zero.

* emulated: p, m, v (and e) after every step equal, bit for bit, a numpy float32 reference written here on its own, which rounds every
  operation separately in the order of the emulated build:
      gs = g * coef;  gg = gs + wd * p;  m' = m + (gg - m) * omb1;  v' = beta2 * v + (omb2 * gg) * gg;
      denom = sqrt(v') * inv_bc2_sqrt + eps;  p' = p - lr_over_bc1 * (m' / denom);   decoupled: p * decay_factor in front;
      average: e' = e + w * (p' - e).
  lr_over_bc1, inv_bc2_sqrt, clip_coef and decay_factor are read back from the device record after each step (the plain step's two are
  computed here with the formula of lbc_adam_launch), so the comparison does not depend on pow / cos; each is checked against its
  float64 formula on the side.
* gpu: a numpy reference of the device build would have to emulate the f32 fma exactly, and going through float64 rounds twice.  So the
  gfx950 library is compared with tests/golden/adam_bits_gfx950.json: per mode and step the SHA-256 of the raw bytes of p, m, v (and e),
  the record header in hex and, for diagnosis, the bit patterns of the first 8 elements and of the last 8 logical elements of the
  70001-element tensor.  The file was recorded on an MI355X from a build of the csrc of commit
  dd704d6c9e2983953e43a8a090543a66cbcbb0f8 ("Waypoint error metrics in metres on the device, sync-free validation"), the last commit
  with four separate step implementations (adam.hip, adam_guarded.hip, adam_clip.hip, adam_recipe.hip).
* both: every record lies as a slice inside a larger buffer of 0xFF bytes (NaN as floats).  The surrounding bytes stay as they are, and
  a kernel that read clip_coef or decay_factor past the end of a narrower record would turn the results into NaN."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests.test_optim_recipe import closed_form
from tests.test_resume_guard import SMALL_TABLE, _sync

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_bits_gfx950.json")

CHUNK = 32768
LR, BETAS, EPS, WD = 1e-3, (0.9, 0.999), 1e-8, 0.01
MAX_NORM = 100.0                        # the gradients of steps 1 and 2 have a norm near 328, those of step 4 near 41
GRAD_SCALE = {1: 1.0, 2: 1.0, 3: 1.0, 4: 0.125}
BAD_STEP = 3
EMA_DECAY = 0.9
COSINE = dict(schedule=1, warmup_steps=2, warmup_start=0.25, total_steps=6, min_lr=1e-5)
COSINE_FORM = dict(kind="cosine", warmup_steps=2, warmup_start=0.25, total_steps=6, min_lr=1e-5)
FENCE = 64                              # bytes of 0xFF on either side of a record (a multiple of 8: the record stays aligned)
# mode -> (entry point, decoupled, average, schedule)
MODES = {
    "plain": ("plain", False, False, None),
    "guarded": ("guarded", False, False, None),
    "clipped": ("clipped", False, False, None),
    "recipe": ("recipe", False, False, {}),
    "recipe_ema": ("recipe", False, True, {}),
    "recipe_decoupled": ("recipe", True, False, {}),
    "recipe_decoupled_ema": ("recipe", True, True, {}),
    "recipe_decoupled_ema_cosine": ("recipe", True, True, COSINE),
}
_INPUTS = {}


def _inputs():
    """the seeded inputs, made once and only ever copied from: p, m, v, e and one gradient per step, float32 numpy"""
    if not _INPUTS:
        off = np.cumsum([0] + [(n + 63) // 64 * 64 for n in SMALL_TABLE])
        total = int(off[-1])
        logical = np.zeros(total, dtype=bool)
        for o, n in zip(off[:-1], SMALL_TABLE):
            logical[int(o):int(o) + n] = True
        rs = np.random.RandomState(20261019)
        d = {"off": off, "total": total, "logical": logical}
        d["p"] = rs.randn(total).astype(np.float32)
        d["m"] = (rs.randn(total) * 0.1).astype(np.float32)
        d["v"] = (rs.rand(total) * 0.01).astype(np.float32)
        d["e"] = rs.randn(total).astype(np.float32)
        big = int(np.argmax(SMALL_TABLE))
        assert SMALL_TABLE[big] == 70001
        d["big"] = (int(off[big]), SMALL_TABLE[big])
        for k in sorted(GRAD_SCALE):
            g = (rs.randn(total) * GRAD_SCALE[k]).astype(np.float32)
            g[~logical] = np.float32("nan")
            if k == BAD_STEP:
                g[d["big"][0] + d["big"][1] - 1] = np.float32("inf")       # the last element of a 1-element scalar tail
            d["g%d" % k] = g
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _INPUTS.update(d)
    return _INPUTS


class _Bits:
    """one mode's buffers on `dev`, its chunk table and its record inside a fence of 0xFF bytes"""

    def __init__(self, dev, mode):
        from learningbycheating_amd import _lib
        self.L, self.lib, self.dev, self.mode = _lib, _lib.get(), dev, mode
        self.entry, self.decoupled, self.ema, self.schedule = MODES[mode]
        inp = _inputs()
        self.t = {k: torch.from_numpy(inp[k].copy()).to(dev) for k in "pmve"}
        self.t["g"] = torch.from_numpy(inp["g1"].copy()).to(dev)
        rows, eptr = [], []
        for o, n in zip(inp["off"][:-1], SMALL_TABLE):
            for c in range(0, n, CHUNK):
                rows.append(tuple(self.t[k].data_ptr() + 4 * (int(o) + c) for k in "pgmv") + (min(CHUNK, n - c), 0))
                eptr.append(self.t["e"].data_ptr() + 4 * (int(o) + c))
        tab = np.zeros(len(rows), dtype=[("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i4"), ("pad", "<i4")])
        for i, r in enumerate(rows):
            tab[i] = r
        self.nchunks = len(rows)
        assert self.nchunks == 8
        self.table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
        self.ema_table = torch.from_numpy(np.array(eptr, dtype=np.uint64).view(np.int64).copy()).to(dev)
        self.State, self.nbytes = {"plain": (None, 0),
                                   "guarded": (_lib.AdamState, int(self.lib.lbc_adam_state_bytes())),
                                   "clipped": (_lib.AdamClipState, int(self.lib.lbc_adam_clip_state_bytes(self.nchunks))),
                                   "recipe": (_lib.AdamRecipeState, int(self.lib.lbc_adam_recipe_state_bytes(self.nchunks)))}[self.entry]
        assert self.nbytes == {"plain": 0, "guarded": 40, "clipped": 64 + 8 * self.nchunks, "recipe": 88 + 8 * self.nchunks}[self.entry]
        self.wide = torch.full((FENCE + self.nbytes + FENCE,), 0xFF, dtype=torch.uint8, device=dev)
        self.wide[FENCE:FENCE + self.nbytes] = 0
        assert self.wide.data_ptr() % 8 == 0
        self.record = ctypes.c_void_p(self.wide.data_ptr() + FENCE)
        self.applied = 0

    def step(self, k):
        """step k of the run -> the record's header afterwards (None for the plain step, which is not called on the bad gradient)"""
        L, lib = self.L, self.lib
        self.t["g"].copy_(torch.from_numpy(_inputs()["g%d" % k].copy()))
        args = (L.ptr(self.table), self.nchunks)
        stream = L.stream_for(self.table)
        if self.entry == "plain":
            if k == BAD_STEP:
                return None
            L.check(lib.lbc_adam_step(*args, LR, BETAS[0], BETAS[1], EPS, WD, self.applied + 1, stream), "adam_step")
        elif self.entry == "guarded":
            L.check(lib.lbc_adam_step_guarded(*args, LR, BETAS[0], BETAS[1], EPS, WD, self.record, stream), "adam_step_guarded")
        elif self.entry == "clipped":
            L.check(lib.lbc_adam_step_clipped(*args, LR, BETAS[0], BETAS[1], EPS, WD, MAX_NORM, self.record, stream), "adam_step_clipped")
        else:
            rc = L.AdamRecipe(base_lr=LR, max_norm=MAX_NORM, weight_decay=WD, decoupled=int(self.decoupled),
                              ema_decay=EMA_DECAY if self.ema else 0.0, beta1=BETAS[0], beta2=BETAS[1], eps=EPS, **self.schedule)
            L.check(lib.lbc_adam_step_recipe(*args, ctypes.byref(rc), L.ptr(self.ema_table) if self.ema else None, self.record, stream),
                    "adam_step_recipe")
        _sync(self.dev)
        if k != BAD_STEP:
            self.applied += 1
        return self.header()

    def header_bytes(self):
        _sync(self.dev)
        return bytes(self.wide[FENCE:FENCE + ctypes.sizeof(self.State)].cpu().numpy().tobytes()) if self.State else None

    def header(self):
        return self.State.from_buffer_copy(self.header_bytes()) if self.State else None

    def numpy(self, name):
        _sync(self.dev)
        return self.t[name].cpu().numpy().copy()

    def assert_fence(self):
        _sync(self.dev)
        w = self.wide.cpu().numpy()
        assert w.size == 2 * FENCE + self.nbytes
        assert bool((w[:FENCE] == 0xFF).all()) and bool((w[FENCE + self.nbytes:] == 0xFF).all()), "%s wrote outside its record" % self.mode


def _same_bits(got, want, what):
    a, b = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b)
        i = int(bad[0])
        raise AssertionError("%s: %d of %d elements differ, the first at %d: got %r (0x%08x), expected %r (0x%08x)"
                             % (what, bad.size, a.size, i, float(got[i]), int(a[i]), float(want[i]), int(b[i])))


def _check_header(mode, k, r, applied):
    """the record after step k: counters, and every coefficient the reference is about to use against its float64 formula"""
    bad = k == BAD_STEP
    assert (r.step, r.bad, r.scan_flag, r.skipped_total, r.skipped_in_a_row) == (applied, int(bad), 0, int(k >= BAD_STEP), int(bad)), (mode, k)
    entry, decoupled, ema, schedule = MODES[mode]
    lr = LR
    if entry == "recipe":
        form = COSINE_FORM if schedule else dict(kind="constant")
        want = closed_form(LR, applied - 1, **form)
        assert abs(r.lr - want) <= 1e-12 * want, (mode, k, r.lr, want)
        lr = r.lr
        df = np.float64(1.0) - np.float64(lr) * WD if decoupled else 1.0
        assert abs(float(r.decay_factor) - df) <= 2.0 ** -24 and (r.decay_factor < 1.0) == decoupled, (mode, k, r.decay_factor)
        assert r.ema_updates == (applied if ema else 0)
    bc1, bc2 = 1.0 - BETAS[0] ** applied, 1.0 - BETAS[1] ** applied
    for got, want in ((r.lr_over_bc1, lr / bc1), (r.inv_bc2_sqrt, 1.0 / np.sqrt(bc2))):
        assert abs(got - want) <= 2.0 ** -23 * want, (mode, k, got, want)            # within an f32 ulp of the float64 value
    if entry in ("clipped", "recipe"):
        clipped_steps = sum(1 for j in range(1, k + 1) if j != BAD_STEP and GRAD_SCALE[j] == 1.0)
        assert r.clipped_total == clipped_steps, (mode, k, r.clipped_total)
        last = k if not bad else k - 1
        if GRAD_SCALE[last] == 1.0:
            want = MAX_NORM / (r.grad_norm + 1e-6)
            assert r.clip_coef < 1.0 and abs(r.clip_coef - want) <= 2.0 ** -23 * want, (mode, k, r.clip_coef, want)
        else:
            assert r.clip_coef == 1.0 and 0.0 < r.grad_norm < MAX_NORM, (mode, k, r.clip_coef, r.grad_norm)


class _Reference:
    """the update in numpy float32, one rounding per operation, on the logical elements"""

    def __init__(self, mode):
        inp = _inputs()
        self.mode, self.logical = mode, inp["logical"]
        self.s = {k: inp[k].copy() for k in "pmve"}

    def step(self, g, lr_over_bc1, inv_bc2_sqrt, coef, decay_factor):
        f = np.float32
        _, decoupled, ema, _ = MODES[self.mode]
        wd = f(0.0 if decoupled else WD)
        beta2, omb1, omb2, eps = f(BETAS[1]), f(1.0 - BETAS[0]), f(1.0 - BETAS[1]), f(EPS)
        lr, inv, coef = f(lr_over_bc1), f(inv_bc2_sqrt), f(coef)
        p, m, v, e = (self.s[k] for k in "pmve")
        with np.errstate(all="ignore"):                # (the padding of g is NaN; its results are dropped below)
            if decoupled:
                p = p * f(decay_factor)
            gs = g * coef
            gg = gs + wd * p
            m2 = m + (gg - m) * omb1
            v2 = beta2 * v + (omb2 * gg) * gg
            denom = np.sqrt(v2) * inv + eps
            p2 = p - lr * (m2 / denom)
            e2 = e + f(1.0 - EMA_DECAY) * (p2 - e) if ema else e
        for k, new in zip("pmve", (p2, m2, v2, e2)):
            assert new.dtype == np.float32
            self.s[k] = np.where(self.logical, new, self.s[k])


def _emulated_case(dev, mode):
    t, ref = _Bits(dev, mode), _Reference(mode)
    entry = MODES[mode][0]
    for k in sorted(GRAD_SCALE):
        r = t.step(k)
        if entry == "plain":
            if k != BAD_STEP:
                bc1, bc2 = 1.0 - BETAS[0] ** t.applied, 1.0 - BETAS[1] ** t.applied
                ref.step(_inputs()["g%d" % k], np.float32(LR / bc1), np.float32(1.0 / np.sqrt(bc2)), 1.0, 1.0)
        else:
            _check_header(mode, k, r, t.applied)
            if k != BAD_STEP:
                ref.step(_inputs()["g%d" % k], r.lr_over_bc1, r.inv_bc2_sqrt, r.clip_coef if entry != "guarded" else 1.0,
                         r.decay_factor if entry == "recipe" else 1.0)
        for name in "pmve":
            _same_bits(t.numpy(name), ref.s[name], "%s, step %d, %s" % (mode, k, name))
        assert np.array_equal(t.numpy("g").view(np.uint32), _inputs()["g%d" % k].view(np.uint32)), "the gradient buffer must not be written"
    assert t.applied == 3 and not np.array_equal(ref.s["p"], _inputs()["p"])
    assert np.array_equal(ref.s["e"], _inputs()["e"]) == (not MODES[mode][2])
    t.assert_fence()


@pytest.mark.parametrize("mode", list(MODES))
def test_adam_bits_match_numpy_float32_emulated(env, mode):
    dev, _ = env
    _emulated_case(dev, mode)


# ---- the gfx950 library against the recorded bits -----------------------------------------------------------------------------------
def inputs_digest():
    inp = _inputs()
    return {k: hashlib.sha256(inp[k].tobytes()).hexdigest() for k in ("p", "m", "v", "e", "g1", "g2", "g3", "g4")}


def trace(dev, mode):
    """what the fixture holds of one mode: a list with one entry per step"""
    t = _Bits(dev, mode)
    o, n = _inputs()["big"]
    out = []
    for k in sorted(GRAD_SCALE):
        t.step(k)
        names = "pmve" if MODES[mode][2] else "pmv"
        arrs = {name: t.numpy(name) for name in names}
        head = t.header_bytes()
        out.append({"step": k,
                    "sha256": {name: hashlib.sha256(a.tobytes()).hexdigest() for name, a in arrs.items()},
                    "header": head.hex() if head is not None else None,
                    "first8": {name: ["%08x" % x for x in a[:8].view(np.uint32)] for name, a in arrs.items()},
                    "last8_of_70001": {name: ["%08x" % x for x in a[o + n - 8:o + n].view(np.uint32)] for name, a in arrs.items()}})
    t.assert_fence()
    if not MODES[mode][2]:
        assert np.array_equal(t.numpy("e").view(np.uint32), _inputs()["e"].view(np.uint32)), "without the average the shadow is not touched"
    return out


@gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_adam_bits_match_recorded_gfx950(env, mode):
    dev, _ = env
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["inputs_sha256"] == inputs_digest(), "the seeded inputs differ from the recorded run's: nothing below would be comparable"
    want, got = golden["modes"][mode], trace(dev, mode)
    assert len(want) == len(got) == 4
    for w, g in zip(want, got):
        for field in ("header", "first8", "last8_of_70001", "sha256"):        # (the readable fields first: they say where it went wrong)
            assert g[field] == w[field], "%s, step %d, %s: got %r, recorded %r" % (mode, w["step"], field, g[field], w[field])
