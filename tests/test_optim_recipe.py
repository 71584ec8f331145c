"""The recipe path of the fused optimizer (csrc/adam.hip, lbc_adam_step_recipe): learning-rate schedule on the device, decoupled
weight decay and the moving average of the weights inside the update.

1. a neutral recipe (constant, no warm-up, coupled decay, no average) is lbc_adam_step_clipped bit for bit, record included;
2. the read-back lr of every step against the closed form in float64 (relative 1e-12: a handful of double operations plus cos / pow,
   each good to a few 2^-53), and each step is the clipped step called with that double;
3. a NaN / +-Inf skips the step: p, m, v, e, lr, decay_factor, ema_updates and step keep their bits, the next clean step uses lr(k = 1);
4. decoupled decay: the clipped step on parameters first multiplied by the read-back float, bit for bit; against torch.optim.AdamW +
   LambdaLR at test_fused_adam_matches_torch's tolerances;
5. the average: every e' within 4 f32 ulps of max(|e|, |p'|) from the float64 value of e + w (p' - e) (two or three f32 roundings, fused
   or not), a lerp_ chain in torch after 4 steps, p / m / v untouched by it, ema_updates;
6. every refusal of the entry point leaves p, m, v, e and the record alone;
7. the student's real table on the GPU;
8. NativeTrainer: neutral schedule == max_grad_norm=0 trainer, bitwise resume inside the warm-up, accumulate=2, ema_state_dict() /
   ema_weights(), two gloo ranks;
9. the scripts' flags.

CPU cases run the kernel sources on the emulator, GPU cases (-m gpu) the gfx950 library; bitwise comparisons are always between two
kernels on the same backend."""
import argparse
import ctypes
import json
import struct

import numpy as np
import pytest
import torch

from oracle import lbc_oracle as O
from tests.test_grad_clip import _ClipTable, _init
from tests.test_resume_guard import SMALL_TABLE, _assert_same, _full_table, _script, _sync
from tests.test_step import _models

gpu = pytest.mark.gpu
VALUES = pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
WHERE = pytest.mark.parametrize("where", ["first", "tail_last", "middle_chunk"])
KINDS = {"constant": dict(kind="constant"), "cosine": dict(kind="cosine", total_steps=7, min_lr=1e-5), "step": dict(kind="step", step_size=2, gamma=0.5)}
BETAS, EPS = (0.9, 0.999), 1e-8


def _bits(x):
    return struct.pack("<d", float(x))


def _fbits(x):
    return struct.pack("<f", float(x))


def closed_form(base, k, kind="constant", warmup_steps=0, warmup_start=0.0, total_steps=0, min_lr=0.0, step_size=1, gamma=1.0):
    """the issue's schedule in float64, written here on its own (not the library's)"""
    base, W = np.float64(base), int(warmup_steps)
    if k < W:
        return float(base * (np.float64(warmup_start) + (1.0 - np.float64(warmup_start)) * np.float64(k) / np.float64(W)))
    j = k - W
    if kind == "cosine":
        span = int(total_steps) - W
        return float(np.float64(min_lr) + (base - np.float64(min_lr)) * 0.5 * (1.0 + np.cos(np.pi * np.float64(min(j, span)) / np.float64(span))))
    if kind == "step":
        return float(base * np.float64(gamma) ** np.float64(j // int(step_size)))
    return float(base)


# ---- the kernel cases -----------------------------------------------------------------------------------------------------------------
class _RecipeTable(_ClipTable):
    """_ClipTable (p, g, m, v; NaN in the padding of g) with the shadow e, whose padding is a fence of NaNs with distinct payloads, the
    per-chunk pointer table into it, and the recipe record"""

    def __init__(self, dev, sizes, seed):
        super().__init__(dev, sizes, seed)
        L = self._lib
        total = int(self.off[-1])
        gen = torch.Generator().manual_seed(seed + 1000)
        e = torch.randn(total, generator=gen)
        fence = (0x7fc00000 | (np.arange(total, dtype=np.int64) & 0xffff) | 0x10000).astype(np.uint32).view(np.int32)
        bits = e.numpy().view(np.int32).copy()
        pad = ~self.logical.numpy()
        bits[pad] = fence[pad]
        self.fence = torch.from_numpy(bits.copy())[~self.logical]
        self.e = torch.from_numpy(bits).view(torch.float32).to(dev)
        ptrs = []
        for o, n in zip(self.off[:-1], sizes):
            for c in range(0, n, 32768):
                ptrs.append(self.e.data_ptr() + 4 * (int(o) + c))
        assert len(ptrs) == self.nchunks
        self.ema_table = torch.from_numpy(np.array(ptrs, dtype=np.uint64).view(np.int64).copy()).to(dev)
        self.rhead = ctypes.sizeof(L.AdamRecipeState)
        nbytes = int(self.lib.lbc_adam_recipe_state_bytes(self.nchunks))
        assert self.rhead == 88 and nbytes == 88 + 8 * self.nchunks
        self.rrecord = torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    def recipe_rc(self, lr=1e-3, max_norm=0.0, wd=0.0, decoupled=False, ema_decay=0.0, ema=True, **schedule):
        """-> the return code of lbc_adam_step_recipe"""
        L = self._lib
        sch = dict(schedule)
        if "schedule" not in sch:
            sch["schedule"] = {"constant": 0, "cosine": 1, "step": 2}[sch.pop("kind", "constant")]
        rc = L.AdamRecipe(base_lr=lr, max_norm=max_norm, weight_decay=wd, decoupled=int(decoupled), ema_decay=ema_decay, beta1=BETAS[0],
                          beta2=BETAS[1], eps=EPS, **sch)
        return self.lib.lbc_adam_step_recipe(L.ptr(self.table), self.nchunks, ctypes.byref(rc), L.ptr(self.ema_table) if ema else None,
                                             L.ptr(self.rrecord), L.stream_for(self.table))

    def recipe(self, **kw):
        self._lib.check(self.recipe_rc(**kw), "adam_step_recipe")
        return self.read()

    def read(self):
        _sync(self.dev)
        return self._lib.AdamRecipeState.from_buffer_copy(self.rrecord[:self.rhead].cpu().numpy().tobytes())

    def clipped_lr(self, lr, max_norm=0.0, wd=0.0):
        """lbc_adam_step_clipped with a rate of the caller's (the double is passed as it is)"""
        L = self._lib
        L.check(self.lib.lbc_adam_step_clipped(L.ptr(self.table), self.nchunks, lr, BETAS[0], BETAS[1], EPS, wd, max_norm, L.ptr(self.record),
                                               L.stream_for(self.table)), "adam_step_clipped")
        _sync(self.dev)

    def head64(self, which):
        _sync(self.dev)
        return bytes((self.rrecord if which == "recipe" else self.record)[:64].cpu().numpy().tobytes())

    def shadow(self):
        _sync(self.dev)
        return self.e.cpu().clone()

    def assert_fence(self):
        got = self.shadow().view(torch.int32)[~self.logical]
        assert torch.equal(got, self.fence), "the padding of the shadow was written"


def _same_pmv(a, b, what):
    for x, y, name in zip(a.clone_state(), b.clone_state(), "pmv"):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "%s differs: %s" % (name, what)


def _grad(gen, t, scale=1.0):
    return torch.randn(t.g.numel(), generator=gen) * scale


# 1.
def _neutral_case(dev, sizes, mode, wd, steps=3):
    a, b = _RecipeTable(dev, sizes, 31), _RecipeTable(dev, sizes, 31)
    gen = torch.Generator().manual_seed(32)
    e0 = a.shadow()
    for step in range(1, steps + 1):
        gr = _grad(gen, a, 10.0 ** (step - 2))
        a.set_grad(gr)
        b.set_grad(gr)
        g_before = a.g.clone()
        max_norm = 0.0 if mode == "zero" else a.norm64()[1] / 8
        r = a.recipe(max_norm=max_norm, wd=wd, ema=False)
        b.clipped_lr(1e-3, max_norm, wd)
        assert (r.step, r.bad) == (step, 0) and (r.clip_coef < 1.0) == (mode == "clip") and r.decay_factor == 1.0 and r.ema_updates == 0
        assert _bits(r.lr) == _bits(1e-3)
        _same_pmv(a, b, "neutral recipe vs lbc_adam_step_clipped, step %d, max_norm %g, weight decay %g" % (step, max_norm, wd))
        assert a.head64("recipe") == b.head64("clip"), "the first 64 bytes of the record"
        assert torch.equal(a.g.cpu().view(torch.int32), g_before.cpu().view(torch.int32)), "the gradient buffer must not be written"
    assert torch.equal(a.shadow().view(torch.int32), e0.view(torch.int32)), "without ema_decay the shadow is not touched"


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("mode", ["zero", "clip"])
def test_neutral_recipe_is_the_clipped_step_emulated(env, mode, wd):
    dev, _ = env
    _neutral_case(dev, SMALL_TABLE, mode, wd)


@gpu
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("mode", ["zero", "clip"])
def test_neutral_recipe_is_the_clipped_step(env, mode, wd):
    dev, _ = env
    _neutral_case(dev, SMALL_TABLE, mode, wd)


# 2.
def _check_lr(r, sch, base, k):
    want = closed_form(base, k, **sch)
    rel = abs(r.lr - want) / abs(want) if want != 0.0 else abs(r.lr)
    print("k = %d: lr %r, closed form %r, relative error %.3g" % (k, r.lr, want, rel))
    assert rel <= 1e-12, (k, r.lr, want)
    return want


def _schedule_case(dev, sizes, kind, s0, steps=10):
    sch = dict(KINDS[kind], warmup_steps=3, warmup_start=s0)
    a, b = _RecipeTable(dev, sizes, 33), _RecipeTable(dev, sizes, 33)
    gen = torch.Generator().manual_seed(34)
    seen = []
    for step in range(1, steps + 1):
        gr = _grad(gen, a)
        a.set_grad(gr)
        b.set_grad(gr)
        r = a.recipe(lr=1e-3, wd=0.01, ema=False, **sch)
        assert (r.step, r.bad) == (step, 0)
        _check_lr(r, sch, 1e-3, step - 1)
        seen.append(r.lr)
        b.clipped_lr(r.lr, 0.0, 0.01)
        _same_pmv(a, b, "%s schedule vs the clipped step at the read-back lr, step %d" % (kind, step))
        assert a.head64("recipe") == b.head64("clip")
    assert seen[0] == 1e-3 * s0 and seen[0] < seen[1] < seen[2] < seen[3] and abs(seen[3] - 1e-3) <= 1e-15, "the warm-up"
    if kind == "cosine":
        assert seen[9] == seen[8] == seen[7] == 1e-5 and seen[6] > 1e-5, "from total_steps on the rate stays at min_lr"
    if kind == "step":
        assert seen[3:] == [1e-3, 1e-3, 5e-4, 5e-4, 2.5e-4, 2.5e-4, 1.25e-4]
    if kind == "constant":
        assert seen[3:] == [1e-3] * 7


@pytest.mark.parametrize("s0", [0.0, 0.25])
@pytest.mark.parametrize("kind", list(KINDS))
def test_schedule_matches_closed_form_and_clipped_step_emulated(env, kind, s0):
    dev, _ = env
    _schedule_case(dev, SMALL_TABLE, kind, s0)


@gpu
@pytest.mark.parametrize("s0", [0.0, 0.25])
@pytest.mark.parametrize("kind", list(KINDS))
def test_schedule_matches_closed_form_and_clipped_step(env, kind, s0):
    dev, _ = env
    _schedule_case(dev, SMALL_TABLE, kind, s0)


# 3.
def _skip_case(dev, sizes, where, value):
    sch = dict(KINDS["cosine"], warmup_steps=3, warmup_start=0.25)
    kw = dict(lr=1e-2, wd=0.01, decoupled=True, ema_decay=0.9, **sch)
    t = _RecipeTable(dev, sizes, 35)
    big = int(np.argmax(sizes))
    assert sizes[big] > 2 * 32768 and sizes[big] % 4 != 0
    spot = {"first": int(t.off[0]), "tail_last": int(t.off[big]) + sizes[big] - 1, "middle_chunk": int(t.off[big]) + 32768 + 1001}[where]
    gen = torch.Generator().manual_seed(36)
    t.set_grad(_grad(gen, t))
    r1 = t.recipe(**kw)
    assert (r1.step, r1.bad, r1.ema_updates) == (1, 0, 1) and r1.decay_factor < 1.0
    _check_lr(r1, sch, 1e-2, 0)
    before, e_before = t.clone_state(), t.shadow()
    t.set_grad(_grad(gen, t))
    good = float(t.g[spot])
    t.g[spot] = value
    r2 = t.recipe(**kw)
    assert (r2.step, r2.bad, r2.skipped_total, r2.skipped_in_a_row, r2.scan_flag) == (1, 1, 1, 1, 0)
    for x, y, name in zip(before, t.clone_state(), "pmv"):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "%s changed by a skipped step" % name
    assert torch.equal(e_before.view(torch.int32), t.shadow().view(torch.int32)), "the shadow changed by a skipped step"
    assert _bits(r2.lr) == _bits(r1.lr) and _fbits(r2.decay_factor) == _fbits(r1.decay_factor) and r2.ema_updates == 1
    assert _bits(r2.grad_norm) == _bits(r1.grad_norm)
    t.g[spot] = good
    r3 = t.recipe(**kw)
    assert (r3.step, r3.bad, r3.skipped_total, r3.skipped_in_a_row, r3.ema_updates) == (2, 0, 1, 0, 2)
    lr1 = _check_lr(r3, sch, 1e-2, 1)
    assert abs(r3.lr - closed_form(1e-2, 2, **sch)) > 1e-4 * lr1, "the step after a skipped one must use lr(k = 1), not lr(k = 2)"
    assert not torch.equal(t.clone_state()[0], before[0]) and not torch.equal(t.shadow()[t.logical], e_before[t.logical])
    t.set_grad(_grad(gen, t))
    r4 = t.recipe(**kw)
    _check_lr(r4, sch, 1e-2, 2)
    assert (r4.step, r4.ema_updates) == (3, 3)
    t.assert_fence()


@VALUES
@WHERE
def test_recipe_step_skips_nonfinite_emulated(env, where, value):
    dev, _ = env
    _skip_case(dev, SMALL_TABLE, where, value)


@gpu
@VALUES
@WHERE
def test_recipe_step_skips_nonfinite(env, where, value):
    dev, _ = env
    _skip_case(dev, SMALL_TABLE, where, value)


# 4. (bitwise) and 5. (ulp), shared with 7.
def _ema_ulp_check(e_before, e_after, p_after, logical, decay, what):
    """|e' - (e + w (p' - e))| <= 4 ulp_f32(max(|e|, |p'|)), the reference in float64 at the read-back p'"""
    w = np.float64(np.float32(1.0 - decay))
    e, p, got = (x.numpy()[logical].astype(np.float64) for x in (e_before, p_after, e_after))
    want = e + w * (p - e)
    scale = np.maximum(np.abs(e), np.abs(p)).astype(np.float32)
    ulp = np.spacing(scale).astype(np.float64)
    worst = float(np.max(np.abs(got - want) / ulp))
    print("%s: the average is within %.3f f32 ulps of max(|e|, |p'|) of its float64 value (bound 4)" % (what, worst))
    assert worst <= 4.0
    assert np.any(got != e), "the average did not move"


def _decoupled_ema_case(dev, sizes, kind, wd, ema_decay, steps, lr=1e-3, twin_without_ema=False):
    """a: the recipe step.  b: lbc_adam_step_clipped at the read-back lr on parameters first multiplied, in torch f32, by the read-back
    decay_factor.  c (optional): a without the average"""
    sch = dict(KINDS[kind], warmup_steps=3, warmup_start=0.25)
    a, b = _RecipeTable(dev, sizes, 37), _RecipeTable(dev, sizes, 37)
    c = _RecipeTable(dev, sizes, 37) if twin_without_ema else None
    logical, logical_dev = a.logical.numpy(), a.logical.to(dev)
    gen = torch.Generator().manual_seed(38)
    chain = a.shadow()
    w32 = float(np.float32(1.0 - ema_decay)) if ema_decay else 0.0
    for step in range(1, steps + 1):
        gr = _grad(gen, a)
        for t in (a, b, c):
            if t is not None:
                t.set_grad(gr)
        e_before = a.shadow()
        r = a.recipe(lr=lr, wd=wd, decoupled=True, ema_decay=ema_decay, ema=bool(ema_decay), **sch)
        _check_lr(r, sch, lr, step - 1)
        df64 = 1.0 - r.lr * wd
        assert abs(float(r.decay_factor) - df64) <= 2.0 ** -24, "decay_factor is (float)(1 - lr * wd): within half an ulp at 1"
        assert (r.decay_factor == 1.0) == (wd == 0.0)
        df = torch.tensor(r.decay_factor, dtype=torch.float32, device=dev)
        b.p.copy_(torch.where(logical_dev, b.p * df, b.p))                               # a separately rounded f32 product, in torch
        b.clipped_lr(r.lr, 0.0, 0.0)
        _same_pmv(a, b, "decoupled decay vs the clipped step on pre-multiplied parameters, step %d" % step)
        if ema_decay:
            assert r.ema_updates == step
            e_after, p_after = a.shadow(), a.clone_state()[0].cpu()
            _ema_ulp_check(e_before, e_after, p_after, logical, ema_decay, "step %d" % step)
            chain[a.logical] = chain[a.logical].lerp_(p_after[a.logical], w32)
        else:
            assert r.ema_updates == 0 and torch.equal(a.shadow().view(torch.int32), e_before.view(torch.int32))
        if c is not None:
            c.recipe(lr=lr, wd=wd, decoupled=True, ema=False, **sch)
            _same_pmv(a, c, "with and without the average, step %d" % step)
    a.assert_fence()
    if ema_decay:
        got = a.shadow()
        assert torch.allclose(got[a.logical], chain[a.logical], rtol=1e-5, atol=1e-6), "the average against a lerp_ chain in torch"
    return a


@pytest.mark.parametrize("wd", [0.01, 0.0])
def test_decoupled_decay_is_the_clipped_step_on_decayed_parameters_emulated(env, wd):
    dev, _ = env
    _decoupled_ema_case(dev, SMALL_TABLE, "cosine", wd, 0.0, 3)


@gpu
@pytest.mark.parametrize("wd", [0.01, 0.0])
def test_decoupled_decay_is_the_clipped_step_on_decayed_parameters(env, wd):
    dev, _ = env
    _decoupled_ema_case(dev, SMALL_TABLE, "cosine", wd, 0.0, 3)


def _decoupled_zero_is_neutral(dev, sizes):
    """decoupled decay of 0 multiplies by 1.0f: the neutral recipe, and so the clipped step"""
    a, b = _RecipeTable(dev, sizes, 39), _RecipeTable(dev, sizes, 39)
    gen = torch.Generator().manual_seed(40)
    for step in range(1, 4):
        gr = _grad(gen, a)
        a.set_grad(gr)
        b.set_grad(gr)
        r = a.recipe(wd=0.0, decoupled=True, ema=False)
        b.clipped_lr(1e-3, 0.0, 0.0)
        assert r.decay_factor == 1.0
        _same_pmv(a, b, "decoupled decay 0 vs the clipped step, step %d" % step)
        assert a.head64("recipe") == b.head64("clip")


def test_decoupled_decay_zero_is_the_neutral_recipe_emulated(env):
    dev, _ = env
    _decoupled_zero_is_neutral(dev, SMALL_TABLE)


@gpu
def test_decoupled_decay_zero_is_the_neutral_recipe(env):
    dev, _ = env
    _decoupled_zero_is_neutral(dev, SMALL_TABLE)


def _adamw_case(dev):
    """FusedAdam(schedule, decoupled) against torch.optim.AdamW + LambdaLR on the CPU in f32: test_fused_adam_matches_torch's small shapes
    and tolerances"""
    from learningbycheating_amd.optim import FusedAdam
    sch = dict(KINDS["cosine"], warmup_steps=2, warmup_start=0.25)
    base, wd = 1e-3, 0.01
    g = torch.Generator().manual_seed(2)
    shapes = [(64, 3, 7, 7), (64,), (5, 64, 1, 1), (128, 64, 3, 3), (7,)]
    ps = [torch.randn(s, generator=g) for s in shapes]
    ps = [p.contiguous(memory_format=torch.channels_last) if p.dim() == 4 else p for p in ps]
    ref = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.AdamW(ref, lr=base, weight_decay=wd)
    lam = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: closed_form(base, k, **sch) / base)
    mine = [(("p%d" % i), torch.nn.Parameter(p.clone().to(dev))) for i, p in enumerate(ps)]
    grads = {n: torch.zeros_like(p.data) for n, p in mine}
    fa = FusedAdam(mine, grads, lr=base, weight_decay=wd, schedule=sch, decoupled_weight_decay=True)
    assert fa.recipe and fa.guarded and fa.clipped and fa.max_grad_norm == 0.0 and fa.ema is None
    assert fa.lr_stats() == {"lr": None, "ema_updates": 0}
    for step in range(4):
        for (n, p), r in zip(mine, ref):
            gr = torch.randn(r.shape, generator=g)
            gr = gr.contiguous(memory_format=torch.channels_last) if gr.dim() == 4 else gr
            r.grad = gr.clone()
            grads[n].copy_(gr)
        used = opt.param_groups[0]["lr"]
        opt.step()
        lam.step()
        fa.step()
        st = fa.lr_stats()
        assert abs(st["lr"] - used) <= 1e-12 * used and st["ema_updates"] == 0
    assert fa.step_count == 4 and fa.grad_stats()["grad_norm"] > 0 and fa.grad_stats()["clip_coef"] == 1.0
    for (n, p), r in zip(mine, ref):
        assert torch.allclose(p.data.cpu(), r.data, rtol=1e-5, atol=1e-6), n
        m, v = fa.state_of(n)
        st = opt.state[r]
        assert torch.allclose(torch.as_strided(m.cpu(), r.shape, r.stride()), st["exp_avg"], rtol=1e-5, atol=1e-7)
        assert torch.allclose(torch.as_strided(v.cpu(), r.shape, r.stride()), st["exp_avg_sq"], rtol=1e-5, atol=1e-9)
    # torch's format: lr and initial_lr hold the base rate, decoupled_weight_decay the real value; torch's own AdamW state loads
    sd = fa.state_dict()
    grp = sd["param_groups"][0]
    assert grp["lr"] == grp["initial_lr"] == base and grp["decoupled_weight_decay"] is True and grp["weight_decay"] == wd
    fa.load_state_dict(sd)
    their = opt.state_dict()
    their["param_groups"][0].setdefault("decoupled_weight_decay", True)
    fa.load_state_dict(their)
    assert fa.lr == base and fa.step_count == 4
    plain = FusedAdam(mine, grads, lr=base)
    assert not plain.recipe and plain.state_dict()["param_groups"][0]["decoupled_weight_decay"] is False
    assert "initial_lr" not in plain.state_dict()["param_groups"][0]
    with pytest.raises(ValueError, match="decoupled"):
        plain.load_state_dict(sd)
    for flag in ("amsgrad", "maximize"):
        bad = dict(sd, param_groups=[dict(grp, **{flag: True})])
        with pytest.raises(ValueError, match="amsgrad"):
            fa.load_state_dict(bad)


def test_decoupled_schedule_matches_torch_adamw_emulated(env):
    dev, _ = env
    _adamw_case(dev)


@gpu
def test_decoupled_schedule_matches_torch_adamw(env):
    dev, _ = env
    _adamw_case(dev)


def _fused_adam_ema_case(dev):
    """FusedAdam(ema_decay=...): the shadow starts as a copy of the parameters, ema_of() is a view in the logical shape (channels_last
    parameters included), a caller's buffer is used as it is, and the average follows torch's lerp_ on the updated parameters"""
    from learningbycheating_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(4)
    shapes = [(8, 3, 3, 3), (5,), (70, 4, 1, 1)]
    ps = [torch.randn(s, generator=g) for s in shapes]
    ps = [p.contiguous(memory_format=torch.channels_last) if p.dim() == 4 else p for p in ps]
    mine = [(("p%d" % i), torch.nn.Parameter(p.clone().to(dev))) for i, p in enumerate(ps)]
    grads = {n: torch.randn(p.shape, generator=g).to(dev).contiguous(memory_format=torch.channels_last) if p.dim() == 4
             else torch.randn(p.shape, generator=g).to(dev) for n, p in mine}
    fa = FusedAdam(mine, grads, lr=1e-1, ema_decay=0.75)
    assert fa.recipe and not fa.decoupled and fa.ema.numel() == fa.exp_avg.numel()
    for n, p in mine:
        assert fa.ema_of(n).shape == p.shape and torch.equal(fa.ema_of(n), p.data), n
    ref = {n: p.data.cpu().clone() for n, p in mine}
    for _ in range(2):
        fa.step()
        _sync(dev)
        for n, p in mine:
            ref[n].lerp_(p.data.cpu(), 0.25)
    for n, p in mine:
        assert torch.allclose(fa.ema_of(n).cpu(), ref[n], rtol=1e-5, atol=1e-6) and not torch.equal(fa.ema_of(n), p.data), n
    assert fa.lr_stats() == {"lr": 1e-1, "ema_updates": 2}
    # a caller's buffer: used where it is, not initialised again
    own = torch.full_like(fa.ema, 3.0)
    fb = FusedAdam(mine, grads, lr=1e-1, ema_decay=0.75, ema=own)
    assert fb.ema is own and float(fb.ema_of("p1")[0]) == 3.0
    with pytest.raises(ValueError, match="ema buffer"):
        FusedAdam(mine, grads, ema_decay=0.75, ema=own[:-1])
    with pytest.raises(ValueError, match="without ema_decay"):
        FusedAdam(mine, grads, ema=own)
    with pytest.raises(ValueError, match="ema_decay"):
        FusedAdam(mine, grads, ema_decay=1.0)
    with pytest.raises(ValueError, match="cosine"):
        FusedAdam(mine, grads, schedule={"kind": "cosine", "warmup_steps": 3, "total_steps": 3})
    with pytest.raises(ValueError, match="unknown kind"):
        FusedAdam(mine, grads, schedule={"kind": "linear"})
    for bad in ({"warmup_steps": -1}, {"warmup_start": 1.5}, {"warmup_start": -0.1}, {"kind": "step", "step_size": 0, "gamma": 0.5},
                {"kind": "step", "step_size": 2, "gamma": 0.0}, {"kind": "cosine", "total_steps": 5, "min_lr": float("nan")}):
        with pytest.raises(ValueError, match="LRSchedule"):
            FusedAdam(mine, grads, schedule=bad)
    with pytest.raises(RuntimeError, match="no average"):
        FusedAdam(mine, grads, schedule={"kind": "constant"}).ema_of("p0")


def test_fused_adam_keeps_the_average_emulated(env):
    dev, _ = env
    _fused_adam_ema_case(dev)


@gpu
def test_fused_adam_keeps_the_average(env):
    dev, _ = env
    _fused_adam_ema_case(dev)


# 5.
def test_ema_inside_the_update_emulated(env):
    dev, _ = env
    _decoupled_ema_case(dev, SMALL_TABLE, "constant", 0.0, 0.9, 4, lr=1e-1, twin_without_ema=True)


@gpu
def test_ema_inside_the_update(env):
    dev, _ = env
    _decoupled_ema_case(dev, SMALL_TABLE, "constant", 0.0, 0.9, 4, lr=1e-1, twin_without_ema=True)


def _ema_coupled_case(dev, sizes):
    """the <coupled, average> instantiation: p, m, v of lbc_adam_step_clipped with weight decay, the average beside them"""
    a, b = _RecipeTable(dev, sizes, 41), _RecipeTable(dev, sizes, 41)
    gen = torch.Generator().manual_seed(42)
    for step in range(1, 3):
        gr = _grad(gen, a)
        a.set_grad(gr)
        b.set_grad(gr)
        e_before = a.shadow()
        max_norm = a.norm64()[1] / 8
        r = a.recipe(lr=1e-1, max_norm=max_norm, wd=0.01, ema_decay=0.99)
        b.clipped_lr(1e-1, max_norm, 0.01)
        _same_pmv(a, b, "coupled decay with the average vs the clipped step, step %d" % step)
        assert a.head64("recipe") == b.head64("clip") and r.ema_updates == step and r.clip_coef < 1.0
        _ema_ulp_check(e_before, a.shadow(), a.clone_state()[0].cpu(), a.logical.numpy(), 0.99, "coupled, step %d" % step)
    a.assert_fence()


def test_ema_with_coupled_decay_and_clipping_emulated(env):
    dev, _ = env
    _ema_coupled_case(dev, SMALL_TABLE)


@gpu
def test_ema_with_coupled_decay_and_clipping(env):
    dev, _ = env
    _ema_coupled_case(dev, SMALL_TABLE)


# 6.
def _validation_case(dev):
    t = _RecipeTable(dev, [64, 5], 1)
    L, lib = t._lib, t.lib
    assert lib.lbc_adam_recipe_state_bytes(1) == 96 and lib.lbc_adam_recipe_state_bytes(1000) == 88 + 8000
    t.set_grad(torch.randn(t.g.numel(), generator=torch.Generator().manual_seed(2)))
    before, e0, rec0 = t.clone_state(), t.shadow(), t.rrecord.clone()
    nan = float("nan")

    def untouched(what):
        for x, y in zip(before, t.clone_state()):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), what
        assert torch.equal(e0.view(torch.int32), t.shadow().view(torch.int32)), what
        assert torch.equal(rec0, t.rrecord), what

    def refused(word, **kw):
        assert t.recipe_rc(**kw) != 0, "accepted: %r" % (kw,)
        msg = lib.lbc_last_error()
        assert word in msg, (kw, msg)
        untouched(repr(kw))

    refused(b"unknown schedule", schedule=3)
    refused(b"unknown schedule", schedule=-1)
    for name in ("lr", "max_norm", "wd", "ema_decay", "warmup_start", "min_lr", "gamma"):
        refused(b"NaN", **{name: nan})
    refused(b"base_lr", lr=-1e-3)
    refused(b"warmup_steps", warmup_steps=-1)
    refused(b"warmup_start", warmup_start=-0.1)
    refused(b"warmup_start", warmup_start=1.5)
    refused(b"total_steps", kind="cosine", warmup_steps=3, total_steps=3)
    refused(b"total_steps", kind="cosine", total_steps=0)
    refused(b"step_size", kind="step", step_size=0, gamma=0.5)
    refused(b"gamma", kind="step", step_size=2, gamma=0.0)
    refused(b"ema_decay", ema_decay=1.0)
    refused(b"ema_decay", ema_decay=-0.1)
    refused(b"shadow pointers", ema_decay=0.9, ema=False)
    refused(b"decoupled weight decay", decoupled=True, wd=-0.01)
    # the pointers, the count and the descriptor's size
    ok = L.AdamRecipe(base_lr=1e-3)
    args = (L.ptr(t.table), t.nchunks, ctypes.byref(ok), None, L.ptr(t.rrecord), None)

    def call(i, v, word):
        a = list(args)
        a[i] = v
        assert lib.lbc_adam_step_recipe(*a) != 0
        assert word in lib.lbc_last_error(), lib.lbc_last_error()
        untouched(word)

    call(2, None, b"null recipe")
    call(4, None, b"state record")
    call(0, None, b"chunk table")
    call(4, ctypes.c_void_p(t.rrecord.data_ptr() + 4), b"aligned to 8 bytes")
    for n in (0, -3):
        call(1, n, b"nchunks")
    for size in (0, ctypes.sizeof(ok) - 8, ctypes.sizeof(ok) + 8):
        bad = L.AdamRecipe(base_lr=1e-3, struct_size=size)
        call(2, ctypes.byref(bad), b"struct_size")
    for beta in ("beta1", "beta2", "eps"):
        bad = L.AdamRecipe(base_lr=1e-3, **{beta: nan})
        call(2, ctypes.byref(bad), b"NaN")
    # what is allowed: a negative coupled decay (as lbc_adam_step), an infinite max_norm, a zero rate
    r = t.recipe(lr=0.0, wd=-0.01, max_norm=float("inf"), ema=False)
    assert (r.step, r.bad, r.clip_coef, r.lr) == (1, 0, 1.0, 0.0)


def test_recipe_entry_point_validates_emulated(env):
    dev, _ = env
    _validation_case(dev)


@gpu
def test_recipe_entry_point_validates(env):
    dev, _ = env
    _validation_case(dev)


# 7.
@gpu
def test_recipe_step_student_table(env):
    """the real table: 136 tensors / 23.1 M elements of the ResNet-34 student, cosine + decoupled decay + average, three steps"""
    dev, _ = env
    sizes = _full_table()
    assert len(sizes) == 136 and 23.0e6 < sum(sizes) < 23.3e6
    _decoupled_ema_case(dev, sizes, "cosine", 0.01, 0.9, 3, lr=1e-2)


# ---- 8. the trainer -------------------------------------------------------------------------------------------------------------------
RECIPE = dict(lr_schedule=dict(KINDS["cosine"], warmup_steps=3, warmup_start=0.25), weight_decay=0.01, ema_decay=0.9)


class _Run:
    """tests/test_grad_clip.py's _Run with the recipe's arguments (any NativeTrainer keyword) and the shadow in the snapshot"""

    def __init__(self, dev, small, precision, init, batch, n_batches=6, world=1, group=None, rank=0, **trainer_kw):
        from learningbycheating_amd.bird_view.utils.datasets.synthetic import SyntheticFrames
        from learningbycheating_amd.training.data import _SyntheticLoader
        from learningbycheating_amd.training.native import NativeTrainer
        self.dev, self.small, self.precision = dev, small, precision
        sh, sw = (32, 64) if small else (160, 384)
        th = tw = 64 if small else 192
        self.student = _models("image", dev, small, 1, precision)
        self.teacher = _models("birdview", dev, small, 2, precision)
        self.student.load_state_dict(init["student"])
        self.teacher.load_state_dict(init["teacher"])
        self.trainer = NativeTrainer(self.student, self.teacher, batch, (3, sh, sw), dev, phase=1, lr=1e-4, teacher_shape=(7, th, tw),
                                     world_size=world, group=group, **trainer_kw)
        frames = SyntheticFrames(2 * batch, dev, seed=3, rank=rank, rgb_hw=(sh, sw), birdview_hw=(th, tw))
        self.loader = _SyntheticLoader(frames, batch, n_batches, augment="super_hard", seed=rank)

    def steps(self, it, k):
        lrs = []
        for _ in range(k):
            rgb, bv, loc, cmd, speed = next(it)
            self.trainer.step(rgb, speed, O.one_hot(cmd).to(self.dev), birdview=bv)
            _sync(self.dev)
            lrs.append(self.trainer.lr_stats()["lr"])
        return lrs

    def snapshot(self):
        _sync(self.dev)
        s = {"sd." + k: v.detach().cpu().clone() for k, v in self.student.state_dict().items()}
        s["m"], s["v"] = self.trainer.opt.exp_avg.cpu().clone(), self.trainer.opt.exp_avg_sq.cpu().clone()
        s["t"] = torch.tensor(self.trainer.opt.step_count)
        if self.trainer.opt.ema is not None:
            s["e"] = self.trainer.opt.ema.cpu().clone()
        return s


def _neutral_trainer(dev, small, precision, batch):
    init = _init(dev, small, precision, batch)
    a = _Run(dev, small, precision, init, batch, lr_schedule={"kind": "constant"})
    b = _Run(dev, small, precision, init, batch, max_grad_norm=0)
    assert a.trainer.opt.recipe and a.trainer.skip_nonfinite and not b.trainer.opt.recipe and a.trainer.opt.ema is None
    assert a.steps(iter(a.loader), 3) == [1e-4] * 3
    b.steps(iter(b.loader), 3)
    _assert_same(a.snapshot(), b.snapshot(), "a neutral schedule vs max_grad_norm = 0, three steps")
    assert _bits(a.trainer.grad_stats()["grad_norm"]) == _bits(b.trainer.grad_stats()["grad_norm"]) and a.trainer.opt.step_count == 3
    assert b.trainer.lr_stats() == {"lr": 1e-4, "ema_updates": 0} and "recipe" not in b.trainer.state_dict()


def test_neutral_schedule_is_the_measuring_trainer_emulated(env):
    dev, _ = env
    _neutral_trainer(dev, True, "fp32", 3)


@gpu
def test_neutral_schedule_is_the_measuring_trainer(env):
    dev, _ = env
    _neutral_trainer(dev, False, "bf16", 4)


def _recipe_resume(dev, small, precision, batch, tmp_path):
    init = _init(dev, small, precision, batch)
    sch = RECIPE["lr_schedule"]
    a = _Run(dev, small, precision, init, batch, **RECIPE)
    e0 = a.trainer.opt.ema.cpu().clone()
    for n, p in a.student.named_parameters():
        if n in a.trainer.opt.offsets:
            assert torch.equal(a.trainer.opt.ema_of(n), p.data), "the average starts as a copy of the parameters (%s)" % n
    lrs = a.steps(iter(a.loader), 4)
    for k, lr in enumerate(lrs):
        want = closed_form(1e-4, k, **sch)
        assert abs(lr - want) <= 1e-12 * want, (k, lr, want)
    b = _Run(dev, small, precision, init, batch, **RECIPE)
    it = iter(b.loader)
    assert b.steps(it, 2) == lrs[:2]
    sd = b.trainer.state_dict()
    assert sd["recipe"] == {"schedule": dict(dict(kind="constant", warmup_steps=0, warmup_start=0.0, total_steps=0, min_lr=0.0, step_size=1, gamma=1.0), **sch),
                            "weight_decay": 0.01, "ema_decay": 0.9}
    assert sd["guard"]["ema_updates"] == 2 and set(sd["ema"]) == set(b.trainer.opt.names)
    grp = sd["optimizer"]["param_groups"][0]
    assert grp["lr"] == grp["initial_lr"] == 1e-4 and grp["decoupled_weight_decay"] is True and grp["weight_decay"] == 0.01
    path = str(tmp_path / "state.th")
    torch.save({"trainer": sd, "loader": b.loader.state_dict()}, path)
    del it, b
    c = _Run(dev, small, precision, init, batch, **RECIPE)
    saved = torch.load(path)
    assert c.trainer.load_state_dict(saved["trainer"]) == []
    c.loader.load_state_dict(saved["loader"])
    assert c.trainer.opt.step_count == 2 and c.trainer.lr_stats() == {"lr": None, "ema_updates": 2}, "no rate until this record applies a step"
    assert c.steps(iter(c.loader), 2) == lrs[2:], "the cut lies inside the warm-up: the rate goes on from Adam's step count"
    _assert_same(a.snapshot(), c.snapshot(), "after 4 steps")
    assert a.trainer.lr_stats() == c.trainer.lr_stats() == {"lr": lrs[3], "ema_updates": 4}
    assert not torch.equal(a.snapshot()["e"], e0), "the average moved"
    # another schedule, the average switched off or on: notes, not errors; a state from before the fields loads as it always did
    d = _Run(dev, small, precision, init, batch, lr_schedule={"kind": "constant"}, weight_decay=0.01)
    notes = d.trainer.load_state_dict(saved["trainer"])
    assert len(notes) == 2 and "schedule" in notes[0] and "moving average" in notes[1] and d.trainer.opt.step_count == 2
    old = {k: v for k, v in saved["trainer"].items() if k not in ("recipe", "ema")}
    old["guard"] = {k: v for k, v in old["guard"].items() if k != "ema_updates"}
    old["optimizer"] = dict(old["optimizer"], param_groups=[dict(grp, decoupled_weight_decay=False, weight_decay=0.0)])
    plain = _Run(dev, small, precision, init, batch, skip_nonfinite=True)
    assert plain.trainer.load_state_dict(old) == [] and plain.trainer.opt.step_count == 2
    e = _Run(dev, small, precision, init, batch, ema_decay=0.9)
    notes = e.trainer.load_state_dict(old)
    assert len(notes) == 1 and "copy of the restored parameters" in notes[0] and e.trainer.lr_stats()["ema_updates"] == 0
    for n in e.trainer.opt.names[:3]:
        assert torch.equal(e.trainer.opt.ema_of(n).cpu(), saved["trainer"]["student"][n])


def test_recipe_run_resumes_bitwise_emulated(env, tmp_path):
    dev, _ = env
    _recipe_resume(dev, True, "fp32", 3, tmp_path)


@gpu
def test_recipe_run_resumes_bitwise(env, tmp_path):
    dev, _ = env
    _recipe_resume(dev, False, "bf16", 4, tmp_path)


def _decay_change_case(dev, small, precision, batch):
    """the decay is the trainer's argument: a state loads under another decay with a note, and the note is what the next step does --
    its decay_factor is (float)(1 - lr * the trainer's decay), and the next state carries one decay, not two"""
    init = _init(dev, small, precision, batch)
    sch = {"kind": "constant"}

    def saved_after_one_step(**kw):
        r = _Run(dev, small, precision, init, batch, lr_schedule=sch, **kw)
        r.steps(iter(r.loader), 1)
        return r, r.trainer.state_dict()

    def next_step(r, sd, decay_before, decay):
        notes = r.trainer.load_state_dict(sd)
        assert notes == ["state saved with weight decay %g, continuing with %g" % (decay_before, decay)], notes
        opt = r.trainer.opt
        assert opt.weight_decay == r.trainer.weight_decay == decay and opt.decoupled == (decay != 0.0) and opt.step_count == 1
        before = r.snapshot()
        assert r.steps(iter(r.loader), 1) == [1e-4]
        rec = opt._read_record()
        want = np.float32(1.0 - 1e-4 * decay)
        assert rec.step == 2 and _fbits(rec.decay_factor) == _fbits(want), (rec.decay_factor, want)
        assert not torch.equal(before["m"], r.snapshot()["m"])
        out = r.trainer.state_dict()
        grp = out["optimizer"]["param_groups"][0]
        assert out["recipe"]["weight_decay"] == grp["weight_decay"] == decay and grp["decoupled_weight_decay"] == (decay != 0.0)

    a, s_decay = saved_after_one_step(weight_decay=0.01)           # trained with 0.01
    b, s_none = saved_after_one_step()                             # trained without decay
    assert a.trainer.opt._read_record().decay_factor == np.float32(1.0 - 1e-4 * 0.01) and b.trainer.opt._read_record().decay_factor == 1.0
    c = _Run(dev, small, precision, init, batch, lr_schedule=sch, weight_decay=0.02)
    next_step(c, s_decay, 0.01, 0.02)                              # 0.01 -> 0.02
    next_step(a, s_none, 0.0, 0.01)                                # 0 -> 0.01 (also: a state without decoupled decay into a decoupled optimizer)
    next_step(b, s_decay, 0.01, 0.0)                               # 0.01 -> 0
    # the same state into a trainer without any of the recipe: the decay is dropped with a note, nothing is refused half way
    plain = _Run(dev, small, precision, init, batch, skip_nonfinite=True)
    notes = plain.trainer.load_state_dict(s_decay)
    assert len(notes) == 2 and "schedule" in notes[0] and notes[1] == "state saved with weight decay 0.01, continuing with 0"
    assert plain.trainer.opt.weight_decay == 0.0 and not plain.trainer.opt.decoupled and plain.trainer.opt.step_count == 1
    plain.steps(iter(plain.loader), 1)
    assert plain.trainer.state_dict()["optimizer"]["param_groups"][0]["decoupled_weight_decay"] is False


def test_state_loads_under_another_decay_emulated(env):
    dev, _ = env
    _decay_change_case(dev, True, "fp32", 3)


@gpu
def test_state_loads_under_another_decay(env):
    dev, _ = env
    _decay_change_case(dev, False, "bf16", 4)


def _accumulate_case(dev, small, precision, batch):
    """accumulate = 2: the schedule advances once per window, because it reads Adam's step count"""
    init = _init(dev, small, precision, batch)
    sch = RECIPE["lr_schedule"]
    a = _Run(dev, small, precision, init, batch, accumulate=2, **RECIPE)
    lrs = a.steps(iter(a.loader), 4)
    want = [closed_form(1e-4, k, **sch) for k in (0, 1)]
    assert lrs[0] is None, "the first micro-step of the first window: nothing applied yet"
    assert [lrs[1], lrs[3]] == [pytest.approx(w, rel=1e-12, abs=0) for w in want] and lrs[2] == lrs[1]
    assert a.trainer.opt.step_count == 2 and a.trainer.lr_stats()["ema_updates"] == 2
    it = iter(a.loader)
    a.steps(it, 1)
    with pytest.raises(RuntimeError, match="accumulation window"):
        with a.trainer.ema_weights():
            pass
    assert a.trainer.reset_accumulation() == 1


def test_schedule_advances_once_per_accumulation_window_emulated(env):
    dev, _ = env
    _accumulate_case(dev, True, "fp32", 3)


@gpu
def test_schedule_advances_once_per_accumulation_window(env):
    dev, _ = env
    _accumulate_case(dev, False, "bf16", 4)


def _ema_weights_case(dev, small, precision, batch):
    init = _init(dev, small, precision, batch)
    a = _Run(dev, small, precision, init, batch, ema_decay=0.5)
    a.trainer.opt.lr = 1e-2                                       # (so that the average differs visibly from the parameters)
    it = iter(a.loader)
    a.steps(it, 2)
    before = a.snapshot()
    esd = a.trainer.ema_state_dict()
    assert list(esd) == list(a.student.state_dict())
    params = dict(a.student.named_parameters())
    for k, v in esd.items():
        if k in a.trainer.opt.offsets:
            assert torch.equal(v, a.trainer.opt.ema_of(k)) and not torch.equal(v, params[k].data), k
            assert v.stride() == params[k].stride()
        else:
            assert torch.equal(v, a.student.state_dict()[k]), k
    rgb, bv, loc, cmd, speed = next(it)
    args = (rgb, speed, O.one_hot(cmd).to(dev))
    plain = a.trainer.step(*args, birdview=bv, update=False, train_mode=False).detach().cpu().clone()
    sd_outside = a.trainer.state_dict()
    with a.trainer.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):     # (leaving the block would exchange the restored parameters and average)
            a.trainer.load_state_dict(sd_outside)
        inside = a.trainer.step(*args, birdview=bv, update=False, train_mode=False).detach().cpu().clone()
        with pytest.raises(RuntimeError, match="ema_weights"):
            a.trainer.step(*args, birdview=bv)
        with pytest.raises(RuntimeError, match="ema_weights"):
            a.trainer.state_dict()
    _assert_same(before, a.snapshot(), "after the context: parameters, moments and the average are back")
    again = a.trainer.step(*args, birdview=bv, update=False, train_mode=False).detach().cpu().clone()
    assert torch.equal(again, plain) and not torch.equal(inside, plain)
    # a student loaded from ema_state_dict()
    b = _Run(dev, small, precision, init, batch)
    b.student.load_state_dict(esd)
    b.trainer.eng.invalidate()
    loaded = b.trainer.step(*args, birdview=bv, update=False, train_mode=False).detach().cpu().clone()
    assert torch.equal(inside, loaded), "the loss inside ema_weights() is the loss of a student loaded from ema_state_dict()"
    with pytest.raises(RuntimeError, match="no average"):
        b.trainer.ema_state_dict()


def test_ema_weights_and_ema_state_dict_emulated(env):
    dev, _ = env
    _ema_weights_case(dev, True, "fp32", 3)


@gpu
def test_ema_weights_and_ema_state_dict(env):
    dev, _ = env
    _ema_weights_case(dev, False, "bf16", 4)


def _two_rank_worker(rank, port, out):
    import torch.distributed as dist
    from tests import emu
    from tests.test_resume_guard import _init_state
    torch.set_num_threads(2)
    emu.activate()
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=2)
    try:
        dev = torch.device("cpu")
        init = _init_state(dev, True, "fp32", 2)                  # (seeded: the same bits on both ranks)
        r = _Run(dev, True, "fp32", init, 2, world=2, group=dist.group.WORLD, rank=rank, **RECIPE)
        lrs = r.steps(iter(r.loader), 3)
        end = r.snapshot()
        par = {k: v for k, v in end.items() if not k.startswith("sd.") or not ("running_" in k or "num_batches" in k)}
        torch.save({"lrs": [_bits(x) for x in lrs], "end": par, "stats": r.trainer.lr_stats(), "skipped": r.trainer.skipped()}, out % rank)
    finally:
        dist.destroy_process_group()


def test_two_ranks_agree_on_rate_and_average(tmp_path):
    """lr is a function of the reduced record's step, the average a function of identical updated parameters (gloo, f32 wire)"""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "rank%d.th")
    mp.start_processes(_two_rank_worker, args=(port, out), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(out % 0), torch.load(out % 1)
    assert r0["lrs"] == r1["lrs"] and len(set(r0["lrs"])) == 3
    assert r0["stats"] == r1["stats"] and r0["stats"]["ema_updates"] == 3 and tuple(r0["skipped"]) == tuple(r1["skipped"]) == (0, 0)
    _assert_same(r0["end"], r1["end"], "rank 0 vs rank 1")
    assert "e" in r0["end"]


# ---- 9. the scripts --------------------------------------------------------------------------------------------------------------------
def test_script_flags_reach_the_trainer_and_the_log_emulated(env):
    """--lr-schedule (and its companions) / --weight-decay / --ema-decay / --ema-eval through training/resume.py: the config entries, the
    keywords the scripts hand to NativeTrainer, and what a logging iteration reports (the scripts themselves need a GPU)"""
    from learningbycheating_amd.training import resume
    dev, _ = env

    def parse(*argv):
        p = argparse.ArgumentParser()
        resume.add_arguments(p)
        return resume.config_entries(p.parse_args(list(argv)))

    assert parse() == {} and resume.recipe_kwargs({}) == {}
    guard = {"skip_nonfinite": True, "max_skipped": 50}
    cos = {"kind": "cosine", "warmup_steps": 2, "warmup_start": 0.25, "total_steps": 6, "min_lr": 1e-6}
    assert parse("--lr-schedule", "cosine", "--warmup-steps", "2", "--warmup-start", "0.25", "--lr-total-steps", "6", "--lr-min", "1e-6") == dict(guard, lr_schedule=cos)
    assert parse("--lr-schedule", "step", "--lr-step-size", "3", "--lr-gamma", "0.5") == \
        dict(guard, lr_schedule={"kind": "step", "warmup_steps": 0, "warmup_start": 0.0, "step_size": 3, "gamma": 0.5})
    assert parse("--warmup-steps", "4") == dict(guard, lr_schedule={"kind": "constant", "warmup_steps": 4, "warmup_start": 0.0})
    assert parse("--weight-decay", "0.01", "--max-skipped", "7") == {"weight_decay": 0.01, "skip_nonfinite": True, "max_skipped": 7}
    assert parse("--ema-decay", "0.9", "--ema-eval") == dict(guard, ema_decay=0.9, ema_eval=True)
    with pytest.raises(SystemExit, match="--lr-total-steps"):
        parse("--lr-schedule", "cosine")
    for bad in (("--ema-eval",), ("--ema-decay", "1.0"), ("--weight-decay", "-1"), ("--lr-schedule", "cosine", "--lr-total-steps", "2", "--warmup-steps", "2"),
                ("--lr-schedule", "step", "--lr-step-size", "0")):
        with pytest.raises(SystemExit):
            parse(*bad)
    config = parse("--lr-schedule", "cosine", "--warmup-steps", "2", "--warmup-start", "0.25", "--lr-total-steps", "6", "--lr-min", "1e-6",
                   "--weight-decay", "0.01", "--ema-decay", "0.9", "--ema-eval", "--log-grad-norm")
    kw = resume.recipe_kwargs(config)
    assert kw == {"lr_schedule": cos, "weight_decay": 0.01, "ema_decay": 0.9} and config["max_grad_norm"] == 0.0
    init = _init(dev, True, "fp32", 3)
    r = _Run(dev, True, "fp32", init, 3, max_grad_norm=config["max_grad_norm"], **kw)
    opt = r.trainer.opt
    assert opt.recipe and opt.decoupled and opt.weight_decay == 0.01 and opt.ema_decay == 0.9 and opt.schedule.as_dict()["total_steps"] == 6
    logged = {}
    assert resume.log_lr_stats(config, r.trainer, lambda **k: logged.update(k), is_train=True) == {"lr": None, "ema_updates": 0}
    assert logged == {"ema_updates": 0, "is_train": True}, "before the first applied step there is no rate to report"
    r.steps(iter(r.loader), 2)
    st = resume.log_lr_stats(config, r.trainer, lambda **k: logged.update(k), is_train=True)
    assert logged == {"lr": st["lr"], "ema_updates": 2, "is_train": True} and st["lr"] == pytest.approx(closed_form(1e-4, 1, **cos), rel=1e-12)
    assert resume.log_grad_stats(config, r.trainer, lambda **k: logged.update(k))["grad_norm"] > 0
    assert resume.log_lr_stats({}, r.trainer, lambda **k: logged.update(never=1)) is None and "never" not in logged
    before = r.snapshot()
    with resume.ema_eval(config, r.trainer):
        assert not torch.equal(r.snapshot()["e"], before["e"])
    with resume.ema_eval({}, r.trainer):
        _assert_same(before, r.snapshot(), "without --ema-eval the context does nothing")
    _assert_same(before, r.snapshot(), "after the contexts")


def test_phase2_takes_schedule_and_decay_and_refuses_the_average_emulated(env, tmp_path):
    """phase 2 re-creates its optimizer every epoch: schedule and decay go to every one of them and start again there; --ema-decay is
    refused before anything is built"""
    from learningbycheating_amd.training import train_image_phase2 as p2
    dev, _ = env
    with pytest.raises(SystemExit, match="--ema-decay is not available in phase 2"):
        p2.main(["--log_dir", str(tmp_path), "--ema-decay", "0.9"])
    with pytest.raises(SystemExit, match="--lr-total-steps"):
        p2.main(["--log_dir", str(tmp_path), "--lr-schedule", "cosine"])
    assert not list(tmp_path.iterdir())
    sch = {"kind": "step", "warmup_steps": 1, "warmup_start": 0.5, "step_size": 1, "gamma": 0.5}
    config = {"lr_schedule": sch, "weight_decay": 0.01, "skip_nonfinite": True, "max_skipped": 50}
    init = _init(dev, True, "fp32", 3)
    r = _Run(dev, True, "fp32", init, 3, lr_schedule=sch, weight_decay=0.01)
    it = iter(r.loader)
    assert r.steps(it, 2) == [0.5e-4, 1e-4]
    p2._fresh_optimizer(r.trainer, config, 1e-4)
    opt = r.trainer.opt
    assert opt.recipe and opt.decoupled and opt.weight_decay == 0.01 and opt.ema is None and opt.step_count == 0
    assert r.steps(it, 3) == [0.5e-4, 1e-4, 0.5e-4], "the schedule starts again with the optimizer"
    p2._fresh_optimizer(r.trainer, {}, 1e-4)
    assert not r.trainer.opt.recipe and not r.trainer.opt.guarded


@gpu
def test_script_recipe_resumes_to_identical_checkpoints(env, tmp_path):
    """train_image_phase1 with a cosine schedule, decay, the average and --ema-eval: epochs 0..2 in one process == epochs 0..1, then a
    fresh process with --resume for epoch 2: byte-identical model-2.th and model-ema-2.th; log.jsonl carries lr"""
    extra = ("--lr-schedule", "cosine", "--warmup-steps", "2", "--lr-total-steps", "6", "--weight-decay", "0.01", "--ema-decay", "0.9", "--ema-eval")
    one, two = tmp_path / "one", tmp_path / "two"
    _script("train_image_phase1", one, 2, *extra)
    _script("train_image_phase1", two, 1, *extra)
    assert (two / "train_state.th").exists() and (two / "model-ema-1.th").exists() and not (two / "model-2.th").exists()
    p = _script("train_image_phase1", two, 2, "--resume", *extra)
    assert "resuming" in (p.stdout + p.stderr)
    for name in ("model-1.th", "model-2.th", "model-ema-1.th", "model-ema-2.th"):
        assert (one / name).read_bytes() == (two / name).read_bytes(), name
    m, e = torch.load(str(one / "model-2.th"), map_location="cpu"), torch.load(str(one / "model-ema-2.th"), map_location="cpu")
    assert list(m) == list(e) and all(m[k].shape == e[k].shape and m[k].dtype == e[k].dtype for k in m)
    assert not torch.equal(m["conv.conv1.weight"], e["conv.conv1.weight"]) and torch.equal(m["conv.bn1.running_mean"], e["conv.bn1.running_mean"])
    s1, s2 = torch.load(str(one / "train_state.th")), torch.load(str(two / "train_state.th"))
    assert s1["epoch"] == s2["epoch"] == 2 and s1["trainer"]["guard"]["ema_updates"] == s2["trainer"]["guard"]["ema_updates"] == 6
    assert s1["trainer"]["recipe"]["ema_decay"] == 0.9 and s1["trainer"]["recipe"]["schedule"]["kind"] == "cosine"
    recs = [json.loads(line) for line in (one / "log.jsonl").read_text().splitlines()]
    last = recs[-1]
    cos = dict(kind="cosine", warmup_steps=2, total_steps=6)           # epoch 2 applies optimizer steps k = 3, 4, 5
    assert last["train_lr"]["max"] == pytest.approx(closed_form(1e-4, 3, **cos), rel=1e-12)
    assert last["train_lr"]["min"] == pytest.approx(closed_form(1e-4, 5, **cos), rel=1e-12) and last["train_ema_updates"]["max"] == 6
    cfg = json.loads((one / "config.json").read_text())
    assert cfg["lr_schedule"]["kind"] == "cosine" and cfg["weight_decay"] == 0.01 and cfg["ema_decay"] == 0.9 and cfg["ema_eval"] is True
