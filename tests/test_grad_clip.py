"""Gradient clipping by global norm on the device, and the grad-norm telemetry (csrc/adam.hip, lbc_adam_step_clipped).

1. the norm: grad_norm^2 against a float64 sum over the logical elements, the padding between tensors poisoned with NaN;
2. the same gradients give the same 8 bytes of grad_norm;
3. without clipping (max_norm = 0, max_norm = 2 * norm) the step is lbc_adam_step_guarded bit for bit;
4. with clipping it is lbc_adam_step_guarded on gradients multiplied by the read-back float (weight decay 0 and 0.01); g is not written;
5. a NaN / +-Inf skips the step, keeps norm / coefficient / count of the last clean step, and does not leak into the next one;
6. the entry point refuses a null or misaligned record, nchunks <= 0 and a NaN max_norm;
7. FusedAdam / NativeTrainer: max_grad_norm = 1e30 is the guarded trainer; a clipped first step gives exp_avg = (g * coef) * (1 - beta1);
8. two data-parallel ranks derive the same norm bits and coefficient;
9. a clipped run resumes bit for bit, clipped_total included; phase 2's per-epoch optimizer carries the count over; the scripts'
   --clip-grad-norm (GPU: the scripts need one).

CPU cases run the kernel sources on the emulator at reduced sizes, GPU cases (-m gpu) at the reference's."""
import ctypes
import json
import struct

import numpy as np
import pytest
import torch

from oracle import lbc_oracle as O
from tests.test_resume_guard import SMALL_TABLE, _assert_same, _full_table, _init_state, _script, _sync
from tests.test_step import _models

gpu = pytest.mark.gpu
VALUES = pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
WHERE = pytest.mark.parametrize("where", ["first", "tail_last", "middle_chunk"])


def _bits(x):
    return struct.pack("<d", float(x))


def _ulp_apart(a, b):
    """|a - b| in float32 units in the last place (both finite and positive)"""
    ia, ib = np.float32(a).view(np.int32), np.float32(b).view(np.int32)
    return abs(int(ia) - int(ib))


# ---- the kernel cases: a table as FusedAdam builds it, with both records -----------------------------------------------------------
class _ClipTable:
    """p, g, m, v over tensors of the given sizes (each on a 64-element boundary, 32768-element chunks); the padding between the tensors
    of g is NaN: the norm pass must read exactly the n elements of every chunk"""

    def __init__(self, dev, sizes, seed):
        from learningbycheating_amd import _lib
        self.lib, self.dev, self._lib, self.sizes = _lib.get(), dev, _lib, sizes
        pad = lambda n: (n + 63) // 64 * 64
        self.off = np.cumsum([0] + [pad(n) for n in sizes])
        total = int(self.off[-1])
        gen = torch.Generator().manual_seed(seed)
        self.p = torch.randn(total, generator=gen).to(dev)
        g = torch.randn(total, generator=gen)
        self.m = (torch.randn(total, generator=gen) * 0.1).to(dev)
        self.v = (torch.rand(total, generator=gen) * 0.01).to(dev)
        self.logical = torch.zeros(total, dtype=torch.bool)
        for o, n in zip(self.off[:-1], sizes):
            self.logical[int(o):int(o) + n] = True
        self.g = self.poison_padding(g).to(dev)
        rows = []
        for o, n in zip(self.off[:-1], sizes):
            for c in range(0, n, 32768):
                rows.append(tuple(t.data_ptr() + 4 * (int(o) + c) for t in (self.p, self.g, self.m, self.v)) + (min(32768, n - c), 0))
        tab = np.zeros(len(rows), dtype=[("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i4"), ("pad", "<i4")])
        for i, r in enumerate(rows):
            tab[i] = r
        self.nchunks = len(rows)
        self.table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
        self.head = ctypes.sizeof(_lib.AdamClipState)
        nbytes = int(self.lib.lbc_adam_clip_state_bytes(self.nchunks))
        assert self.head == 64 and nbytes == self.head + 8 * self.nchunks
        self.record = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        assert self.lib.lbc_adam_state_bytes() == 40
        self.guard_record = torch.zeros(40, dtype=torch.uint8, device=dev)

    def poison_padding(self, g):
        g = g.clone()
        g[~self.logical] = float("nan")
        return g

    def set_grad(self, g_cpu):
        self.g.copy_(self.poison_padding(g_cpu))

    def grad_numpy(self):
        """the logical elements, in table order"""
        _sync(self.dev)
        return self.g.cpu()[self.logical].numpy()

    def norm64(self):
        """(sum of squares, norm): exact float64 squares added in extended precision -- the reference's own error is far below 2^-53"""
        g = self.grad_numpy().astype(np.float64)
        s = float(np.sum((g * g).astype(np.longdouble)))
        return s, float(np.sqrt(s))

    def clone_state(self):
        _sync(self.dev)
        return self.p.clone(), self.m.clone(), self.v.clone()

    def set_state(self, pmv):
        for t, s in zip((self.p, self.m, self.v), pmv):
            t.copy_(s)

    def clipped(self, max_norm, wd=0.0):
        L = self._lib
        L.check(self.lib.lbc_adam_step_clipped(L.ptr(self.table), self.nchunks, 1e-3, 0.9, 0.999, 1e-8, wd, max_norm, L.ptr(self.record),
                                               L.stream_for(self.table)), "adam_step_clipped")
        _sync(self.dev)
        return L.AdamClipState.from_buffer_copy(self.record[:self.head].cpu().numpy().tobytes())

    def guarded(self, wd=0.0):
        L = self._lib
        L.check(self.lib.lbc_adam_step_guarded(L.ptr(self.table), self.nchunks, 1e-3, 0.9, 0.999, 1e-8, wd, L.ptr(self.guard_record),
                                               L.stream_for(self.table)), "adam_step_guarded")
        _sync(self.dev)
        return L.AdamState.from_buffer_copy(self.guard_record.cpu().numpy().tobytes())


def _check_norm(t, r):
    """test 1's bound: any-order float64 summation of n exact non-negative terms is within n * 2^-53 of the true sum"""
    s, norm = t.norm64()
    n = int(t.logical.sum())
    rel = abs(r.grad_norm * r.grad_norm - s) / s
    print("grad_norm %r, numpy %r, relative error of the square %.3g (bound %.3g, %d elements)" % (r.grad_norm, norm, rel, n * 2.0 ** -53, n))
    assert rel <= n * 2.0 ** -53
    return norm


# 1. + 2.
def _norm_case(dev, sizes):
    t = _ClipTable(dev, sizes, 21)
    assert max(sizes) > 2 * 32768 and max(sizes) % 4 != 0 and 5 in sizes and 64 in sizes and 32768 in sizes
    before = t.clone_state()
    rec0 = t.record.clone()
    r = t.clipped(0.0)
    assert (r.step, r.skipped_total, r.skipped_in_a_row, r.bad, r.scan_flag) == (1, 0, 0, 0, 0), "NaN in the padding must not skip the step"
    assert (r.clip_coef, r.clipped_total) == (1.0, 0)
    _check_norm(t, r)
    # the same gradients again, everything else restored: the same 8 bytes
    t.set_state(before)
    t.record.copy_(rec0)
    r2 = t.clipped(0.0)
    assert _bits(r2.grad_norm) == _bits(r.grad_norm)
    for x, y in zip(t.clone_state(), before):
        assert not torch.equal(x, y)


def test_norm_matches_float64_and_is_deterministic_emulated(env):
    dev, _ = env
    _norm_case(dev, SMALL_TABLE)


@gpu
def test_norm_matches_float64_and_is_deterministic(env):
    dev, _ = env
    _norm_case(dev, SMALL_TABLE)


# 3.
def _no_clip_case(dev, sizes, mode, steps=3):
    a, b = _ClipTable(dev, sizes, 22), _ClipTable(dev, sizes, 22)
    gen = torch.Generator().manual_seed(23)
    for step in range(1, steps + 1):
        gr = torch.randn(a.g.numel(), generator=gen) * (10.0 ** (step - 2))
        a.set_grad(gr)
        b.set_grad(gr)
        max_norm = 0.0 if mode == "zero" else 2.0 * a.norm64()[1]
        r = a.clipped(max_norm)
        rb = b.guarded()
        assert (r.step, r.bad, r.skipped_total) == (rb.step, rb.bad, rb.skipped_total) == (step, 0, 0)
        assert r.clip_coef == 1.0 and r.clipped_total == 0
        assert (r.lr_over_bc1, r.inv_bc2_sqrt) == (rb.lr_over_bc1, rb.inv_bc2_sqrt)
        for x, y, name in zip(a.clone_state(), b.clone_state(), "pmv"):
            assert torch.equal(x, y), "%s differs from the guarded step at step %d" % (name, step)
    return a, r


@pytest.mark.parametrize("mode", ["zero", "twice"])
def test_unclipped_step_is_the_guarded_step_emulated(env, mode):
    dev, _ = env
    _no_clip_case(dev, SMALL_TABLE, mode)


@gpu
@pytest.mark.parametrize("mode", ["zero", "twice"])
def test_unclipped_step_is_the_guarded_step(env, mode):
    dev, _ = env
    _no_clip_case(dev, SMALL_TABLE, mode)


# 4.
def _clip_case(dev, sizes, wd, steps=2):
    a, b = _ClipTable(dev, sizes, 24), _ClipTable(dev, sizes, 24)
    gen = torch.Generator().manual_seed(25)
    for step in range(1, steps + 1):
        gr = torch.randn(a.g.numel(), generator=gen)
        a.set_grad(gr)
        g_before = a.g.clone()
        norm = a.norm64()[1]
        max_norm = norm / 8
        r = a.clipped(max_norm, wd)
        _check_norm(a, r)
        expect = np.float32(max_norm / (norm + 1e-6))
        assert r.clip_coef < 1.0 and _ulp_apart(r.clip_coef, expect) <= 1, (r.clip_coef, expect)
        assert (r.step, r.bad, r.clipped_total) == (step, 0, step)
        assert torch.equal(a.g.cpu().view(torch.int32), g_before.cpu().view(torch.int32)), "the gradient buffer must not be written"
        b.set_grad(torch.from_numpy(gr.numpy() * np.float32(r.clip_coef)))        # a separately rounded float32 product on the host
        b.guarded(wd)
        for x, y, name in zip(a.clone_state(), b.clone_state(), "pmv"):
            assert torch.equal(x, y), "%s differs from the guarded step on host-scaled gradients (step %d, weight decay %g)" % (name, step, wd)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_clipped_step_is_the_guarded_step_on_scaled_gradients_emulated(env, wd):
    dev, _ = env
    _clip_case(dev, SMALL_TABLE, wd)


@gpu
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_clipped_step_is_the_guarded_step_on_scaled_gradients(env, wd):
    dev, _ = env
    _clip_case(dev, SMALL_TABLE, wd)


@gpu
def test_clipped_step_student_table(env):
    """the real table: 136 tensors / 23.1 M elements of the ResNet-34 student -- norm, coefficient, bitwise twin, one skipped step"""
    dev, _ = env
    sizes = _full_table()
    assert len(sizes) == 136 and 23.0e6 < sum(sizes) < 23.3e6
    _clip_case(dev, sizes, 0.01, steps=1)
    a, r = _no_clip_case(dev, sizes, "zero", steps=1)
    before = a.clone_state()
    spot = int(a.off[60]) + sizes[60] // 2
    good = float(a.g[spot])
    a.g[spot] = float("inf")
    r2 = a.clipped(1.0)
    assert (r2.step, r2.bad, r2.skipped_total, r2.clipped_total) == (1, 1, 1, 0) and _bits(r2.grad_norm) == _bits(r.grad_norm)
    for x, y in zip(before, a.clone_state()):
        assert torch.equal(x, y)
    a.g[spot] = good
    r3 = a.clipped(0.0)
    assert (r3.step, r3.bad) == (2, 0) and _bits(r3.grad_norm) == _bits(r.grad_norm)


# 5.
def _nonfinite_case(dev, sizes, where, value):
    t = _ClipTable(dev, sizes, 26)
    big = int(np.argmax(sizes))
    assert sizes[big] > 2 * 32768 and sizes[big] % 4 != 0
    spot = {"first": int(t.off[0]), "tail_last": int(t.off[big]) + sizes[big] - 1, "middle_chunk": int(t.off[big]) + 32768 + 1001}[where]
    max_norm = t.norm64()[1] / 8
    r0 = t.clipped(max_norm)
    assert (r0.step, r0.skipped_total, r0.skipped_in_a_row, r0.bad, r0.scan_flag, r0.clipped_total) == (1, 0, 0, 0, 0, 1) and r0.clip_coef < 1.0
    before = t.clone_state()
    good = float(t.g[spot])
    t.g[spot] = value
    for k in (1, 2):                                              # the flag does not stick to a gradient that stays bad
        r = t.clipped(max_norm)
        for x, y, name in zip(before, t.clone_state(), "pmv"):
            assert torch.equal(x, y), "%s changed by a skipped step" % name
        assert (r.step, r.skipped_total, r.skipped_in_a_row, r.bad, r.scan_flag) == (1, k, k, 1, 0)
        assert _bits(r.grad_norm) == _bits(r0.grad_norm) and r.clip_coef == r0.clip_coef and r.clipped_total == 1, "telemetry of the last clean step"
    t.g[spot] = good
    r = t.clipped(max_norm)
    assert (r.step, r.skipped_total, r.skipped_in_a_row, r.bad, r.scan_flag, r.clipped_total) == (2, 2, 0, 0, 0, 2)
    _check_norm(t, r)
    assert _bits(r.grad_norm) == _bits(r0.grad_norm) and r.clip_coef == r0.clip_coef, "the bad step's partial sums must not leak"
    assert not torch.equal(t.clone_state()[0], before[0])


@VALUES
@WHERE
def test_clipped_step_skips_nonfinite_emulated(env, where, value):
    dev, _ = env
    _nonfinite_case(dev, SMALL_TABLE, where, value)


@gpu
@VALUES
@WHERE
def test_clipped_step_skips_nonfinite(env, where, value):
    dev, _ = env
    _nonfinite_case(dev, SMALL_TABLE, where, value)


# 6.
def test_clipped_entry_point_validates(env):
    dev, _ = env
    t = _ClipTable(dev, [64], 1)
    L, lib = t._lib, t.lib
    args = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert lib.lbc_adam_clip_state_bytes(1) == 72 and lib.lbc_adam_clip_state_bytes(1000) == 64 + 8000
    assert lib.lbc_adam_step_clipped(L.ptr(t.table), 1, *args, 1.0, None, None) != 0
    assert b"state record" in lib.lbc_last_error()
    wide = torch.zeros(128, dtype=torch.uint8, device=dev)
    odd = ctypes.c_void_p(wide.data_ptr() + 4)
    assert wide.data_ptr() % 8 == 0
    assert lib.lbc_adam_step_clipped(L.ptr(t.table), 1, *args, 1.0, odd, None) != 0
    assert b"aligned to 8 bytes" in lib.lbc_last_error()
    for n in (0, -3):
        assert lib.lbc_adam_step_clipped(L.ptr(t.table), n, *args, 1.0, L.ptr(t.record), None) != 0
        assert b"nchunks" in lib.lbc_last_error()
    assert lib.lbc_adam_step_clipped(L.ptr(t.table), 1, *args, float("nan"), L.ptr(t.record), None) != 0
    assert b"NaN" in lib.lbc_last_error()
    assert int(wide.count_nonzero()) == 0 and int(t.record.count_nonzero()) == 0, "a refused call must not touch the record"
    assert t.clipped(float("inf")).clip_coef == 1.0               # an infinite max_norm is a number: it never clips


# ---- 7. optimizer and trainer -----------------------------------------------------------------------------------------------------------
_INIT = {}


def _init(dev, small, precision, batch):
    """test_resume_guard's seeded, warm-started student + teacher, computed once per configuration and shared (state_dicts of CPU
    tensors, only ever copied from)"""
    key = (torch.device(dev).type, small, precision, batch)
    if key not in _INIT:
        _INIT[key] = _init_state(dev, small, precision, batch)
    return _INIT[key]


class _Run:
    """tests/test_resume_guard.py's _Run with max_grad_norm"""

    def __init__(self, dev, small, precision, init, batch, skip_nonfinite=False, max_grad_norm=None, n_batches=4, world=1, group=None, rank=0,
                 grad_dtype=None):
        from learningbycheating_amd.bird_view.utils.datasets.synthetic import SyntheticFrames
        from learningbycheating_amd.training.data import _SyntheticLoader
        from learningbycheating_amd.training.native import NativeTrainer
        self.dev = dev
        sh, sw = (32, 64) if small else (160, 384)
        th = tw = 64 if small else 192
        self.student = _models("image", dev, small, 1, precision)
        self.teacher = _models("birdview", dev, small, 2, precision)
        self.student.load_state_dict(init["student"])
        self.teacher.load_state_dict(init["teacher"])
        self.trainer = NativeTrainer(self.student, self.teacher, batch, (3, sh, sw), dev, phase=1, lr=1e-4, teacher_shape=(7, th, tw),
                                     skip_nonfinite=skip_nonfinite, max_grad_norm=max_grad_norm, world_size=world, group=group,
                                     grad_dtype=grad_dtype)
        frames = SyntheticFrames(2 * batch, dev, seed=3, rank=rank, rgb_hw=(sh, sw), birdview_hw=(th, tw))
        self.loader = _SyntheticLoader(frames, batch, n_batches, augment="super_hard", seed=rank)

    def steps(self, it, k):
        for _ in range(k):
            rgb, bv, loc, cmd, speed = next(it)
            self.trainer.step(rgb, speed, O.one_hot(cmd).to(self.dev), birdview=bv)
            _sync(self.dev)

    def snapshot(self):
        _sync(self.dev)
        s = {"sd." + k: v.detach().cpu().clone() for k, v in self.student.state_dict().items()}
        s["m"], s["v"] = self.trainer.opt.exp_avg.cpu().clone(), self.trainer.opt.exp_avg_sq.cpu().clone()
        s["t"] = torch.tensor(self.trainer.opt.step_count)
        return s

    def grads(self):
        """{name: the gradient's elements in memory order (the optimizer's element order), float32 numpy}"""
        _sync(self.dev)
        eng = self.trainer.eng
        flat = eng.grad_flat.cpu().numpy()
        return {n: flat[eng.grad_offsets[n][0]:eng.grad_offsets[n][0] + eng.grad_offsets[n][1]].copy() for n in self.trainer.opt.names}


def _huge_max_norm_is_the_guarded_trainer(dev, small, precision, batch):
    init = _init(dev, small, precision, batch)
    a = _Run(dev, small, precision, init, batch, max_grad_norm=1e30)
    b = _Run(dev, small, precision, init, batch, skip_nonfinite=True)
    assert a.trainer.skip_nonfinite and a.trainer.opt.guarded and a.trainer.opt.clipped and not b.trainer.opt.clipped
    a.steps(iter(a.loader), 2)
    b.steps(iter(b.loader), 2)
    _assert_same(a.snapshot(), b.snapshot(), "max_grad_norm = 1e30 vs skip_nonfinite alone, two steps")
    st = a.trainer.grad_stats()
    assert a.trainer.opt.step_count == 2 and st["clip_coef"] == 1.0 and st["clipped_total"] == 0 and st["grad_norm"] > 0
    assert b.trainer.grad_stats() == {"grad_norm": None, "clip_coef": 1.0, "clipped_total": 0}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_huge_max_norm_is_the_guarded_trainer_emulated(env, precision):
    dev, _ = env
    _huge_max_norm_is_the_guarded_trainer(dev, True, precision, 3)


@gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_huge_max_norm_is_the_guarded_trainer(env, precision):
    dev, _ = env
    _huge_max_norm_is_the_guarded_trainer(dev, False, precision, 32)


def _measured_norm(dev, small, precision, init, batch):
    """the first step's gradient norm, from a run that measures without clipping"""
    m = _Run(dev, small, precision, init, batch, max_grad_norm=0)
    m.steps(iter(m.loader), 1)
    st = m.trainer.grad_stats()
    assert st["clip_coef"] == 1.0 and st["clipped_total"] == 0 and st["grad_norm"] > 0
    return m, st["grad_norm"]


def _first_clipped_step(dev, small, precision, batch):
    init = _init(dev, small, precision, batch)
    m, norm = _measured_norm(dev, small, precision, init, batch)
    # grad_stats() against numpy on the gradient buffer
    g = m.grads()
    allg = np.concatenate([g[n] for n in m.trainer.opt.names]).astype(np.float64)
    s = float(np.sum((allg * allg).astype(np.longdouble)))
    rel = abs(norm * norm - s) / s
    print("trainer grad_norm %r, numpy %r, relative error of the square %.3g (%d elements)" % (norm, np.sqrt(s), rel, allg.size))
    assert rel <= allg.size * 2.0 ** -53
    # the same first step, clipped to half its norm, from zero moments
    a = _Run(dev, small, precision, init, batch, max_grad_norm=norm / 2)
    a.steps(iter(a.loader), 1)
    st = a.trainer.grad_stats()
    assert _bits(st["grad_norm"]) == _bits(norm) and st["clipped_total"] == 1 and a.trainer.opt.step_count == 1
    expect = np.float32((norm / 2) / (norm + 1e-6))
    assert _ulp_apart(st["clip_coef"], expect) <= 1 and st["clip_coef"] < 1.0
    ga = a.grads()
    coef, omb1 = np.float32(st["clip_coef"]), np.float32(1.0 - 0.9)
    for n in a.trainer.opt.names:
        assert np.array_equal(ga[n].view(np.int32), g[n].view(np.int32)), "the gradient views keep the unclipped values (%s)" % n
        mom = a.trainer.opt.state_of(n)[0].cpu().numpy()
        assert np.array_equal(mom, (ga[n] * coef) * omb1), "exp_avg of %s after one clipped step from zero moments" % n


def test_first_clipped_step_and_grad_stats_emulated(env):
    dev, _ = env
    _first_clipped_step(dev, True, "fp32", 3)


@gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_first_clipped_step_and_grad_stats(env, precision):
    dev, _ = env
    _first_clipped_step(dev, False, precision, 32)


# ---- 8. two ranks agree -----------------------------------------------------------------------------------------------------------------
def _two_rank_worker(rank, port, wire, out):
    import torch.distributed as dist
    from tests import emu
    torch.set_num_threads(2)
    emu.activate()
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=2)
    try:
        dev = torch.device("cpu")
        init = _init_state(dev, True, "fp32", 2)                  # (seeded: the same bits on both ranks)
        r = _Run(dev, True, "fp32", init, 2, max_grad_norm=0, world=2, group=dist.group.WORLD, rank=rank,
                 grad_dtype=torch.bfloat16 if wire == "bf16" else None)
        it = iter(r.loader)
        r.steps(it, 1)
        first = r.trainer.grad_stats()
        r.trainer.opt.max_grad_norm = first["grad_norm"] / 4        # (the ranks see different frames; the reduced gradients are one)
        stats = []
        for _ in range(2):
            r.steps(it, 1)
            stats.append(r.trainer.grad_stats())
        end = r.snapshot()
        par = {k: v for k, v in end.items() if not k.startswith("sd.") or not ("running_" in k or "num_batches" in k)}
        torch.save({"first": first, "stats": stats, "end": par, "skipped": r.trainer.skipped(), "t": r.trainer.opt.step_count}, out % rank)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("wire", ["f32", "bf16"])
def test_two_ranks_derive_the_same_coefficient(tmp_path, wire):
    """the norm pass reads the all-reduced gradients in a fixed order: both ranks hold the same 8 bytes of grad_norm and the same clip_coef"""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "rank%d.th")
    mp.start_processes(_two_rank_worker, args=(port, wire, out), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(out % 0), torch.load(out % 1)
    for a, b in zip([r0["first"]] + r0["stats"], [r1["first"]] + r1["stats"]):
        assert _bits(a["grad_norm"]) == _bits(b["grad_norm"]) and a["clip_coef"] == b["clip_coef"] and a["clipped_total"] == b["clipped_total"]
    for r in (r0, r1):
        assert tuple(r["skipped"]) == (0, 0) and r["t"] == 3
        assert r["first"]["clip_coef"] == 1.0 and r["stats"][-1]["clipped_total"] >= 1 and min(s_["clip_coef"] for s_ in r["stats"]) < 1.0
    _assert_same(r0["end"], r1["end"], "rank 0 vs rank 1")


# ---- 9. resume ---------------------------------------------------------------------------------------------------------------------------
def _clipped_resume(dev, small, precision, batch, tmp_path):
    init = _init(dev, small, precision, batch)
    _, norm = _measured_norm(dev, small, precision, init, batch)
    clip = norm / 2
    a = _Run(dev, small, precision, init, batch, max_grad_norm=clip)
    a.steps(iter(a.loader), 4)
    b = _Run(dev, small, precision, init, batch, max_grad_norm=clip)
    it = iter(b.loader)
    b.steps(it, 2)
    sd = b.trainer.state_dict()
    assert sd["format"] == 1 and sd["guard"]["clipped_total"] == b.trainer.grad_stats()["clipped_total"] >= 1
    path = str(tmp_path / "state.th")
    torch.save({"trainer": sd, "loader": b.loader.state_dict()}, path)
    del it, b
    c = _Run(dev, small, precision, init, batch, max_grad_norm=clip)
    saved = torch.load(path)
    assert c.trainer.load_state_dict(saved["trainer"]) == []
    c.loader.load_state_dict(saved["loader"])
    assert c.trainer.opt.step_count == 2 and c.trainer.grad_stats()["clipped_total"] == sd["guard"]["clipped_total"]
    c.steps(iter(c.loader), 2)
    _assert_same(a.snapshot(), c.snapshot(), "after 4 steps")
    sa, sc = a.trainer.grad_stats(), c.trainer.grad_stats()
    assert _bits(sa["grad_norm"]) == _bits(sc["grad_norm"]) and sa["clip_coef"] == sc["clip_coef"] and sa["clipped_total"] == sc["clipped_total"] >= 1
    assert a.trainer.opt.step_count == 4 and a.trainer.skipped() == (0, 0)
    # a state written without the count (an older file) restores as zero; an unclipped trainer ignores the count
    old = dict(saved["trainer"], guard={k: v for k, v in saved["trainer"]["guard"].items() if k != "clipped_total"})
    c.trainer.load_state_dict(old)
    assert c.trainer.grad_stats()["clipped_total"] == 0 and c.trainer.opt.step_count == 2


def test_clipped_run_resumes_bitwise_emulated(env, tmp_path):
    dev, _ = env
    _clipped_resume(dev, True, "fp32", 3, tmp_path)


@gpu
def test_clipped_run_resumes_bitwise(env, tmp_path):
    dev, _ = env
    _clipped_resume(dev, False, "bf16", 32, tmp_path)


def test_script_flags_reach_the_trainer_and_the_log_emulated(env):
    """--clip-grad-norm / --log-grad-norm through training/resume.py: the config entries the scripts hand to NativeTrainer and the three
    fields a logging iteration reports (the scripts themselves need a GPU: see test_script_clips_and_resumes)"""
    import argparse
    from learningbycheating_amd.training import resume
    dev, _ = env

    def parse(*argv):
        p = argparse.ArgumentParser()
        resume.add_arguments(p)
        return resume.config_entries(p.parse_args(list(argv)))

    assert parse() == {}
    assert parse("--clip-grad-norm", "0.5") == {"max_grad_norm": 0.5, "skip_nonfinite": True, "max_skipped": 50}
    assert parse("--log-grad-norm", "--max-skipped", "7") == {"max_grad_norm": 0.0, "skip_nonfinite": True, "max_skipped": 7}
    with pytest.raises(SystemExit):
        parse("--clip-grad-norm", "0")
    init = _init(dev, True, "fp32", 3)
    r = _Run(dev, True, "fp32", init, 3, **{k: v for k, v in parse("--clip-grad-norm", "1e-3").items() if k != "max_skipped"})
    r.steps(iter(r.loader), 1)
    logged = {}
    st = resume.log_grad_stats({"max_grad_norm": 1e-3}, r.trainer, lambda **kw: logged.update(kw), is_train=True)
    assert logged == {"grad_norm": st["grad_norm"], "clip_coef": st["clip_coef"], "clipped_steps": 1, "is_train": True} and st["clip_coef"] < 1.0
    assert resume.log_grad_stats({}, r.trainer, lambda **kw: logged.update(never=1)) is None and "never" not in logged


def test_phase2_fresh_optimizer_carries_clipped_total_emulated(env):
    """phase 2 re-creates its optimizer every epoch (train_image_phase2._fresh_optimizer): moments, step count and skip counters start
    again, the number of clipped steps goes on counting, and the new optimizer clips with the run's max_grad_norm"""
    from learningbycheating_amd.training.train_image_phase2 import _fresh_optimizer
    dev, _ = env
    init = _init(dev, True, "fp32", 3)
    config = {"max_grad_norm": 1e-3, "skip_nonfinite": True, "max_skipped": 50}
    r = _Run(dev, True, "fp32", init, 3, max_grad_norm=config["max_grad_norm"])
    it = iter(r.loader)
    r.steps(it, 2)
    assert r.trainer.grad_stats()["clipped_total"] == 2 and r.trainer.opt.step_count == 2
    old = r.trainer.opt
    _fresh_optimizer(r.trainer, config, 1e-4)
    opt = r.trainer.opt
    assert opt is not old and opt.clipped and opt.guarded and opt.max_grad_norm == 1e-3
    assert opt.step_count == 0 and opt.skipped() == (0, 0)
    assert int(opt.exp_avg.count_nonzero()) == 0 and int(opt.exp_avg_sq.count_nonzero()) == 0
    assert r.trainer.grad_stats()["clipped_total"] == 2
    r.steps(it, 1)
    st = r.trainer.grad_stats()
    assert st["clipped_total"] == 3 and st["clip_coef"] < 1.0 and opt.step_count == 1
    # a run without the flags: the fresh optimizer neither clips nor counts
    _fresh_optimizer(r.trainer, {}, 1e-4)
    assert not r.trainer.opt.clipped and not r.trainer.opt.guarded
    assert r.trainer.grad_stats() == {"grad_norm": None, "clip_coef": 1.0, "clipped_total": 0}


@gpu
def test_script_clips_and_resumes(env, tmp_path):
    """train_image_phase1 --clip-grad-norm: log.jsonl carries grad_norm / clip_coef / clipped_steps, and epochs 0..2 in one process ==
    epochs 0..1, then a fresh process with --resume for epoch 2: byte-identical model-2.th, the same clipped_total"""
    extra = ("--clip-grad-norm", "1e-3")
    one, two = tmp_path / "one", tmp_path / "two"
    _script("train_image_phase1", one, 2, *extra)
    _script("train_image_phase1", two, 1, *extra)
    assert (two / "train_state.th").exists() and not (two / "model-2.th").exists()
    p = _script("train_image_phase1", two, 2, "--resume", *extra)
    assert "resuming" in (p.stdout + p.stderr)
    for name in ("model-1.th", "model-2.th"):
        assert (one / name).read_bytes() == (two / name).read_bytes(), name
    s1, s2 = torch.load(str(one / "train_state.th")), torch.load(str(two / "train_state.th"))
    assert s1["epoch"] == s2["epoch"] == 2
    assert s1["trainer"]["guard"]["clipped_total"] == s2["trainer"]["guard"]["clipped_total"] >= 1
    recs = [json.loads(line) for line in (one / "log.jsonl").read_text().splitlines()]
    last = recs[-1]
    assert last["train_grad_norm"]["mean"] > 0 and last["train_clip_coef"]["max"] < 1.0 and last["train_clipped_steps"]["max"] >= 1
    cfg = json.loads((one / "config.json").read_text())
    assert cfg["max_grad_norm"] == 1e-3 and cfg["skip_nonfinite"] in (True, 1, "True")
