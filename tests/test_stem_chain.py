"""The input side of the step, kernel by kernel through the C ABI: uint8 frames -> padded image (lbc_u8nhwc_to_input), the 7x7/2 stem
(lbc_stem_fwd) with its (sum, sum of squares) rows, and bn1 + relu + maxpool with its backward (lbc_maxpool3x3s2_fwd / _bwd).  These
cases pin what an implementation of those kernels has to keep: the uint8 path bit-identical to the f32 one from any source pointer, the
arg-max taps exactly torch's on inputs full of ties, both statistics within the worst case of an f32 running sum.  Shapes are the
smallest that reach every path: rows narrower than a 16-byte piece, more rows than a run, a tile and two pixels, one output row, more
tiles than resident workgroups.  Unmarked cases run on the emulator, "-gfx950" twins on the MI355X; every input lies between NaN
fences, every output is guarded, and every launch runs three times bit-identically on the GPU (tests/helpers)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from learningbycheating_amd import _lib
from tests.helpers import guarded, guarded_input as G, check_guard, nhwc, nchw, on_both, relerr, repeat

gpu = pytest.mark.gpu
P = _lib.ptr


def rbf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _stream(t):
    return _lib.stream_for(t)


# ---------------------------------------------------------------------------------------------------------------
# uint8 NHWC frames -> padded image
# ---------------------------------------------------------------------------------------------------------------
# (frame shape, bytes by which the uint8 view starts inside its buffer, elements by which the padded image starts past a 16-byte boundary)
PREP_CASES = [((2, 3, 4, 6), 0, 0), ((3, 7, 6, 10), 0, 0), ((2, 3, 2, 22), 0, 0),
              ((2, 4, 4, 4), 0, 0), ((1, 8, 2, 2), 0, 0), ((2, 1, 4, 6), 0, 0), ((2, 5, 4, 6), 0, 0),
              ((2, 3, 4, 6), 1, 0), ((2, 3, 4, 6), 3, 0), ((3, 7, 6, 10), 1, 0), ((3, 7, 6, 10), 3, 0),
              ((2, 3, 4, 6), 0, 3), ((2, 1, 4, 6), 0, 1)]
# More elements than one launch covers in a single sweep of its grid (2048 workgroups x 256 lanes x 16 bytes: 4.2 M bf16 or 2.1 M f32
# elements), from a padded image off its 16-byte boundary: every lane advances (image, row, offset) by the stride at least once.
# 170 x 1 x 94 x 250: rows of exactly 256 elements, so the stride is a whole number of rows and the lane that owns the partial first
# piece lands in front of a row start again; with one channel the elements in front of it are frame pixels of the row before.
PREP_SWEEPS = [("sweep-c1", ((170, 1, 94, 250), 0, 5)), ("sweep-c3", ((24, 3, 160, 384), 0, 3)), ("sweep-c7", ((16, 7, 192, 192), 0, 2)),
               ("sweep-c3-bytes", ((24, 3, 160, 384), 1, 7)), ("sweep-c2", ((90, 2, 94, 250), 0, 7))]


@pytest.mark.parametrize("xbf", [0, 1])
@pytest.mark.parametrize("case", on_both("case", PREP_CASES, edge=PREP_SWEEPS))
def test_prep_u8_matches_f32_path(env, case, xbf):
    dev, _ = env
    lib = _lib.get()
    (N, C, H, W), off, xoff = case
    g = torch.Generator().manual_seed(700 + C + W)
    u8 = torch.randint(0, 256, (N, H, W, C), generator=g, dtype=torch.uint8)
    u8[0, 0, 0] = 0
    u8[-1, -1, -1] = 255
    x = (u8.float() / 255.0).permute(0, 3, 1, 2).contiguous()
    store = torch.zeros(u8.numel() + off, dtype=torch.uint8, device=dev)
    u8d = store[off:off + u8.numel()].view(N, H, W, C)
    u8d.copy_(u8)
    assert u8d.data_ptr() % 4 == off
    xd = G(x.to(dev))
    dt = torch.bfloat16 if xbf else torch.float32
    shape = (N, H + 6, W + 6, C)
    n = N * (H + 6) * (W + 6) * C

    def padded():
        """a NaN-filled padded image `xoff` elements past a 16-byte boundary, NaN fences of at least 256 elements around it"""
        buf = torch.full((n + 512 + 8,), float("nan"), dtype=dt, device=dev)
        lo = 256 + xoff
        return buf, lo, buf[lo:lo + n].view(shape)

    def fences(buf, lo):
        assert torch.isnan(buf[:lo]).all() and torch.isnan(buf[lo + n:]).all(), "kernel wrote outside the padded image"

    def launch():
        ba, la, xa = padded()
        bb, lb, xb = padded()
        assert xa.data_ptr() % 16 == xoff * xa.element_size() % 16
        _lib.check(lib.lbc_nchw_to_input(P(xd), P(xa), xbf, N, C, H, W, int(C == 3), _stream(xd)))
        _lib.check(lib.lbc_u8nhwc_to_input(P(u8d), P(xb), xbf, N, C, H, W, int(C == 3), _stream(xd)))
        fences(ba, la)
        fences(bb, lb)
        return xa, xb
    xa, xb = repeat(dev, launch)
    assert not torch.isnan(xb.float()).any()           # every element of the NaN-filled image was written
    assert torch.equal(xa, xb)                         # the uint8 frames give bit-identical padded images
    border = xb.float().clone()
    border[:, 3:3 + H, 3:3 + W] = 0
    assert border.abs().max().item() == 0.0            # 3-pixel zero border
    inner = xb[:, 3:3 + H, 3:3 + W].float().cpu().permute(0, 3, 1, 2)
    ref = x
    if C == 3:
        ref = (x - torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)) / torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    assert (inner - ref).abs().max().item() < (2.0 ** -7 if xbf else 2e-6)


@pytest.mark.parametrize("xbf", [0, 1])
@pytest.mark.parametrize("where", ["emulator", pytest.param("mi355x", marks=gpu)])
def test_prep_u8_frame_without_pixels(env, where, xbf):
    """H = 0: there is no frame byte to read, and the padded image is six rows of border"""
    dev, _ = env
    lib = _lib.get()
    N, C, H, W = 2, 3, 0, 10
    u8d = torch.zeros(16, dtype=torch.uint8, device=dev)
    buf, xp = guarded((N, H + 6, W + 6, C), dev, dtype=torch.bfloat16 if xbf else torch.float32)
    _lib.check(lib.lbc_u8nhwc_to_input(P(u8d), P(xp), xbf, N, C, H, W, 1, _stream(u8d)))
    check_guard(buf, xp.numel())
    assert xp.float().abs().max().item() == 0.0


# ---------------------------------------------------------------------------------------------------------------
# bn1 -> relu -> maxpool(3,2,1) and its backward on inputs full of ties
# ---------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 64, 2, 2), (1, 64, 6, 4), (3, 64, 10, 6), (2, 8, 4, 4), (2, 128, 4, 6), (2, 64, 20, 4)]


def _taps(ind, H, W):
    """F.max_pool2d's flat input indices [N, C, OH, OW] -> window taps 0..8 of MaxPool2d(3, 2, 1)"""
    OH, OW = ind.shape[2:]
    oy = torch.arange(OH).view(1, 1, OH, 1)
    ox = torch.arange(OW).view(1, 1, 1, OW)
    iy, ix = ind // W, ind % W
    return ((iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1))).to(torch.uint8)


@pytest.mark.parametrize("bf", [0, 1])
@pytest.mark.parametrize("shape", on_both("shape", POOL_SHAPES))
def test_pool_ties_fwd_bwd(env, shape, bf):
    """y is drawn from the integers -2..2 and the affine from a few binary fractions, so y * scale + shift is exact however it is
    evaluated (fused or not, f32 or bf16 storage) and equal values are equal on both sides: the taps must match torch's exactly.
    Image 0 is all -2: every window there is all zeros after the ReLU, and the first in-bounds tap wins."""
    dev, _ = env
    lib = _lib.get()
    N, C, H, W = shape
    g = torch.Generator().manual_seed(900 + H + C)
    y = torch.randint(-2, 3, shape, generator=g).float()
    y[0] = -2.0
    pick = lambda vals: torch.tensor(vals)[torch.randint(0, len(vals), (C,), generator=g)]
    scale, shift = pick([0.5, 1.0, 1.5]), pick([-0.5, 0.0, 0.25, 0.5])
    mean, invstd = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    z = (y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).requires_grad_(True)
    p_ref, ind = F.max_pool2d(F.relu(z), 3, 2, 1, return_indices=True)
    assert p_ref[0].abs().max().item() == 0.0
    dp = torch.randn(p_ref.shape, generator=g)
    if bf:
        dp = rbf(dp)
    (p_ref * dp).sum().backward()
    at = torch.bfloat16 if bf else torch.float32
    yd = G(nhwc(y).to(dev).to(at))
    sd, shd, md, ivd = G(scale.to(dev)), G(shift.to(dev)), G(mean.to(dev)), G(invstd.to(dev))

    def pool_fwd():
        bufp, p = guarded((N, H // 2, W // 2, C), dev, dtype=at)
        bufi, idx = guarded((N, H // 2, W // 2, C), dev, fill=255, dtype=torch.uint8)
        _lib.check(lib.lbc_maxpool3x3s2_fwd(P(yd), P(sd), P(shd), P(p), P(idx), N, H, W, C, bf, _stream(yd)))
        check_guard(bufp, p.numel())
        assert (bufi[:256] == 255).all() and (bufi[256 + idx.numel():] == 255).all(), "kernel wrote outside idx"
        return p, idx
    p, idx = repeat(dev, pool_fwd)
    assert torch.equal(nchw(idx).cpu(), _taps(ind, H, W))
    pr = p_ref.detach()
    if bf:
        assert relerr(nchw(p).float().cpu(), pr) < 2.0 ** -8
    else:
        assert torch.allclose(nchw(p).cpu(), pr, rtol=1e-6, atol=1e-6)
    rows = ctypes.c_int(0)
    _lib.check(lib.lbc_maxpool3x3s2_bwd(None, None, None, None, None, None, None, None, None, ctypes.byref(rows), N, H, W, C, bf, None))
    dpd = G(nhwc(dp).to(dev).to(at))

    def pool_bwd():
        part = torch.zeros((rows.value, 2, C), device=dev)
        bufg, gg = guarded((N, H, W, C), dev, dtype=at)
        _lib.check(lib.lbc_maxpool3x3s2_bwd(P(dpd), P(idx), P(yd), P(sd), P(shd), P(md), P(ivd), P(gg), P(part), ctypes.byref(rows),
                                            N, H, W, C, bf, _stream(yd)))
        check_guard(bufg, gg.numel())
        return gg, part
    gg, part = repeat(dev, pool_bwd)
    gref = z.grad
    got = nchw(gg).float().cpu()
    assert got[0].abs().max().item() == 0.0            # no gradient passes the all-negative image
    if bf:
        assert relerr(got, gref) < 2.0 ** -8
    else:
        assert torch.allclose(got, gref, rtol=0, atol=1e-6)
    xhat = (y - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
    assert torch.allclose(part[:, 0].sum(0).cpu(), gref.sum((0, 2, 3)), rtol=1e-3, atol=1e-3 * gref.abs().sum((0, 2, 3)).max().item())
    assert torch.allclose(part[:, 1].sum(0).cpu(), (gref * xhat).sum((0, 2, 3)), rtol=1e-3, atol=1e-3 * (gref * xhat).abs().sum((0, 2, 3)).max().item())


# ---------------------------------------------------------------------------------------------------------------
# stem forward, bf16 operands: output and both statistics
# ---------------------------------------------------------------------------------------------------------------
MEAN = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
STD = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
STEM_SHAPES = [(3, 3, 6, 24), (2, 7, 2, 128), (2, 3, 10, 132), (1, 7, 6, 24)]
STEM_MANY_TILES = [pytest.param(s, marks=gpu) for s in [(16, 3, 200, 16), (12, 7, 200, 16)]]    # more tiles than resident workgroups


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("shape", on_both("shape", STEM_SHAPES, STEM_MANY_TILES))
def test_stem_forward_and_statistics(env, shape, mode):
    """mode 1: bf16 padded image and operands, f32 output.  mode 2: bf16 output too.  In mode 1 y holds the f32 accumulators the
    statistics were summed from, so both sums are held to the worst case of an f32 running sum over the pixels of one statistics
    row: |error| <= P * 2^-24 * sum |y| (resp. sum y^2, whose terms carry one more rounding each), with P the pixels per row rounded
    up to whole 64-pixel tiles; the rows themselves are added in float64."""
    dev, _ = env
    lib = _lib.get()
    N, C, H, W = shape
    g = torch.Generator().manual_seed(1100 + C + H)
    u8 = torch.randint(0, 256, (N, H, W, C), generator=g, dtype=torch.uint8)
    x = (u8.float() / 255.0).permute(0, 3, 1, 2).contiguous()
    w = torch.randn((64, C, 7, 7), generator=g) * (2.0 / (49 * 64)) ** 0.5
    xn = (x - MEAN) / STD if C == 3 else x
    ref = F.conv2d(rbf(xn), rbf(w), None, 2, 3)
    xd = G(x.to(dev))
    xp = torch.full((N, H + 6, W + 6, C), float("nan"), dtype=torch.bfloat16, device=dev)
    _lib.check(lib.lbc_nchw_to_input(P(xd), P(xp), 1, N, C, H, W, int(C == 3), _stream(xd)))
    xp = G(xp)
    wd = G(w.permute(0, 2, 3, 1).contiguous().to(dev))
    at = torch.bfloat16 if mode == 2 else torch.float32
    rows = ctypes.c_int(0)
    _lib.check(lib.lbc_stem_fwd(None, None, None, None, ctypes.byref(rows), N, H, W, C, mode, None))

    def stem_fwd():
        bufs, st = guarded((rows.value, 2, 64), dev)
        buf, y = guarded((N, H // 2, W // 2, 64), dev, dtype=at)
        _lib.check(lib.lbc_stem_fwd(P(xp), P(wd), P(y), P(st), ctypes.byref(rows), N, H, W, C, mode, _stream(xd)))
        check_guard(buf, y.numel())
        check_guard(bufs, st.numel())
        return y, st
    y, st = repeat(dev, stem_fwd)
    assert not torch.isnan(st).any()                   # lbc_stem_fwd's row count is exactly what the launch writes
    got = nchw(y).float().cpu()
    assert relerr(got, ref) < 2e-3 + (2.0 ** -8 if mode == 2 else 0)
    assert relerr(got, F.conv2d(xn, w, None, 2, 3)) < 2e-2
    s1, s2 = st[:, 0].double().sum(0).cpu(), st[:, 1].double().sum(0).cpu()
    yd = got.double()
    pixels = N * (H // 2) * (W // 2)
    per_row = -(-pixels // rows.value)
    Pmax = -(-per_row // 64) * 64
    e1 = (s1 - yd.sum((0, 2, 3))).abs()
    if mode == 1:
        e2 = (s2 - (yd * yd).sum((0, 2, 3))).abs()
        b1 = Pmax * 2.0 ** -24 * yd.abs().sum((0, 2, 3))
        b2 = Pmax * 2.0 ** -24 * (yd * yd).sum((0, 2, 3))
        print("stem statistics %s: sum error / bound %.3g, sum of squares error / bound %.3g" % (shape, (e1 / b1).max().item(), (e2 / b2).max().item()))
        assert (e1 <= b1).all() and (e2 <= b2).all()
    else:
        # y was rounded to bf16 after the statistics were taken: every element is off by at most 2^-9 of itself
        assert (e1 <= (2.0 ** -9 * 1.01 + Pmax * 2.0 ** -24) * yd.abs().sum((0, 2, 3))).all()
