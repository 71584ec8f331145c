"""Split-bf16 ("bf16x3") precision: lbc_conv_desc.bf16 = 4 / lbc_net_desc.precision = 3 / precision = "bf16x3".

Every f32 MFMA operand v is split into hi = bf16(v) and lo = bf16(v - hi) when the tile is written to LDS, and each fragment pair
costs three bf16 MFMAs (lo*hi + hi*lo + hi*hi) into the f32 accumulator.  Tensors stay f32 as in precision 0 / 1.

Kernel parity is checked two ways on the same inputs: (a) against a float64 torch result on the UNROUNDED operands, and (b) against
precision 1 (operands rounded to bf16 once), whose error must be >= 50x larger -- the check that fails if a lo product is dropped or a
lo plane is mis-addressed (either leaves bf16-level error behind).  Small shapes run the kernel sources under the CPU emulator and, as
"-gfx950" cases, the real gfx950 library; the other gpu-marked cases run that library at layer shapes."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from learningbycheating_amd import WAYPOINT_MEAN_TOLERANCE, WAYPOINT_TOLERANCE, _lib
from oracle import lbc_oracle as O
from tests.helpers import WHERE, Conv, engine_from_state_dict, on_both, relerr
from tests.test_kernels import BF_REAL, BF_SMALL, make
from tests.test_model import _diag, _frozen_gradient_check, _inputs, _launch_counts, seeded_inputs
from tests.test_step import _k_steps

gpu = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (a) bound against float64 on the unrounded operands, (b) required ratio of precision 1's error to bf16x3's
X3_TOL = 2e-5
GAIN = 50.0


class ConvX3(Conv):
    """tests.helpers.Conv with lbc_conv_desc.bf16 = 4 where the caller asks for mode 1: helpers.Conv reads bf16 >= 2 as bf16
    tensors, so the calls below say bf16=1 (f32 tensors, transposed weights where mode 1 needs them) and the descriptor carries 4"""

    def desc(self, N, H, W, C, K, k, s, p, relu=0, bf16=0, wt=0):
        return super().desc(N, H, W, C, K, k, s, p, relu, 4 if bf16 == 1 else bf16, wt)


def _both(fn):
    """fn(conv_class) run with split operands and with mode 1: (bf16x3 result, mode-1 result)"""
    return fn(ConvX3), fn(Conv)


def _check(name, got3, got1, ref64, tol=X3_TOL):
    e3, e1 = relerr(got3.double(), ref64), relerr(got1.double(), ref64)
    print("%s: bf16x3 %.2e, bf16 operands %.2e (x%.0f)" % (name, e3, e1, e1 / max(e3, 1e-30)))
    assert e3 < tol, (name, e3)
    assert e1 > GAIN * e3, (name, "bf16x3 is not clearly better than bf16 operands", e3, e1)


def _bn_on_load(x, C, seed):
    g = torch.Generator().manual_seed(seed)
    ps, pt = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    return ps, pt, F.relu(x.double() * ps.double().view(1, -1, 1, 1) + pt.double().view(1, -1, 1, 1))


@pytest.mark.parametrize("cfg", on_both("cfg", BF_SMALL, BF_REAL))
def test_conv_fwd_x3(env, cfg):
    """forward with BatchNorm+ReLU on load (f32, before the split) and the statistics partials"""
    dev, _ = env
    N, H, W, C, K, k, s, p = cfg
    x, w = make(cfg, 120)
    ps, pt, xin = _bn_on_load(x, C, 121)
    ref = F.conv2d(xin, w.double(), None, s, p)
    (y3, st3), (y1, _) = _both(lambda cls: cls(dev).fwd(x, w, s, p, pre=(ps, pt, True), stats=True, bf16=1))
    _check("fwd %s" % (cfg,), y3, y1, ref)
    # statistics rows, as in test_conv_fwd_bf16_mode: they come from the f32 accumulators
    assert torch.allclose(st3[:, 0].sum(0).double(), ref.sum((0, 2, 3)), rtol=1e-4, atol=1e-4 * ref.abs().sum((0, 2, 3)).max().item())
    assert torch.allclose(st3[:, 1].sum(0).double(), (ref * ref).sum((0, 2, 3)), rtol=1e-4)


@pytest.mark.parametrize("cfgid", [0, 1, 2])
@pytest.mark.parametrize("cfg", on_both("cfg", [(2, 9, 8, 128, 128, 3, 1, 1), (1, 10, 12, 64, 128, 3, 2, 1)],
                                         [pytest.param((32, 20, 48, 128, 128, 3, 1, 1), marks=gpu), pytest.param((32, 10, 24, 256, 512, 1, 2, 0), marks=gpu)]))
def test_conv_x3_every_tile_config(env, cfg, cfgid, lbc_config):
    """the three register-staged tile shapes (128 x 64, 128 x 128, 64 x 64; LBC_FORCE_CFG pins the policy) in both GEMM orientations:
    forward (gather) with bias + residual + ReLU, and the input gradient (transposed) through the depth-contiguous weight copy"""
    dev, _ = env
    N, H, W, C, K, k, s, p = cfg
    lbc_config("LBC_FORCE_CFG", cfgid)
    x, w = make(cfg, 130 + cfgid)
    g = torch.Generator().manual_seed(131)
    b = torch.randn(K, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), s, p)
    r = torch.randn(ref.shape, generator=g)
    ref = F.relu(ref + r.double())
    (y3, _), (y1, _) = _both(lambda cls: cls(dev).fwd(x, w, s, p, bias=b, resid=r, relu=1, bf16=1))
    _check("fwd cfg %d %s" % (cfgid, cfg), y3, y1, ref)
    xg = x.double().requires_grad_(True)
    yy = F.conv2d(xg, w.double(), None, s, p)
    dy = torch.randn(yy.shape, generator=g)
    yy.backward(dy.double())
    dx3, dx1 = _both(lambda cls: cls(dev).dgrad(dy, w, H, W, s, p, bf16=1, transposed=True))
    ref = xg.grad if k == 3 else xg.grad * (torch.arange(H).view(-1, 1) % 2 == 0) * (torch.arange(W) % 2 == 0)
    _check("dgrad cfg %d %s" % (cfgid, cfg), dx3, dx1, ref)


@pytest.mark.parametrize("where", WHERE)
def test_conv_fwd_x3_residual_relu(env, where):
    dev, _ = env
    cfg = (2, 6, 8, 64, 64, 3, 1, 1)
    x, w = make(cfg, 140)
    r = torch.randn((2, 64, 6, 8), generator=torch.Generator().manual_seed(141))
    ref = F.relu(F.conv2d(x.double(), w.double(), None, 1, 1) + r.double())
    (y3, _), (y1, _) = _both(lambda cls: cls(dev).fwd(x, w, 1, 1, resid=r, relu=1, bf16=1))
    _check("fwd residual", y3, y1, ref)


@pytest.mark.parametrize("cfg", on_both("cfg", BF_SMALL[:3], [pytest.param((4, 20, 48, 128, 128, 3, 1, 1), marks=gpu), pytest.param((2, 20, 48, 128, 256, 3, 2, 1), marks=gpu)]))
def test_conv_dgrad_x3(env, cfg):
    """input gradient (+ the identity gradient in the epilogue), stride 1 and the four-phase stride-2 launch"""
    dev, _ = env
    N, H, W, C, K, k, s, p = cfg
    x, w = make(cfg, 150)
    xg = x.double().requires_grad_(True)
    y = F.conv2d(xg, w.double(), None, s, p)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(151))
    y.backward(dy.double())
    r = torch.randn(x.shape, generator=torch.Generator().manual_seed(152))
    dx3, dx1 = _both(lambda cls: cls(dev).dgrad(dy, w, H, W, s, p, resid=r, bf16=1, transposed=True))
    _check("dgrad %s" % (cfg,), dx3, dx1, xg.grad + r.double())


@pytest.mark.parametrize("cfg", on_both("cfg", BF_SMALL + [(40, 5, 6, 64, 64, 3, 1, 1)], BF_REAL))
def test_conv_wgrad_x3(env, cfg):
    dev, _ = env
    N, H, W, C, K, k, s, p = cfg
    x, w = make(cfg, 160)
    wg = w.double().requires_grad_(True)
    y = F.conv2d(x.double(), wg, None, s, p)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(161))
    y.backward(dy.double())
    dw3, dw1 = _both(lambda cls: cls(dev).wgrad(x, dy, k, s, p, bf16=1))
    _check("wgrad %s" % (cfg,), dw3, dw1, wg.grad)


@pytest.mark.parametrize("cfg", on_both("cfg", [(3, 6, 8, 64, 128, 3, 1, 1)], [pytest.param((8, 20, 48, 128, 128, 3, 1, 1), marks=gpu)]))
def test_conv_wgrad_x3_bn_relu_on_load(env, cfg):
    """conv2's weight gradient: y1 read with bn1 + ReLU applied on load (f32, before the split)"""
    dev, _ = env
    N, H, W, C, K, k, s, p = cfg
    x, w = make(cfg, 170)
    ps, pt, xin = _bn_on_load(x, C, 171)
    wg = w.double().requires_grad_(True)
    y = F.conv2d(xin, wg, None, s, p)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(172))
    y.backward(dy.double())
    dw3, dw1 = _both(lambda cls: cls(dev).wgrad(x, dy, k, s, p, pre=(ps, pt, True), bf16=1))
    _check("wgrad bn-on-load %s" % (cfg,), dw3, dw1, wg.grad)


@pytest.mark.parametrize("cfg", on_both("cfg", [(2, 3, 4, 64, 64), (1, 5, 12, 128, 64)], [pytest.param((4, 5, 12, 640, 256), marks=gpu), pytest.param((2, 20, 48, 128, 64), marks=gpu)]))
def test_deconv_x3(env, cfg):
    """lbc_deconv3x3s2_fwd (four output-parity phases in one launch, BatchNorm on load, bias, ReLU, statistics), _dgrad, _wgrad"""
    dev, _ = env
    N, H, W, C, K = cfg
    g = torch.Generator().manual_seed(180)
    x = torch.randn((N, C, H, W), generator=g)
    w = torch.randn((C, K, 3, 3), generator=g) * (2.0 / (C * 2.25)) ** 0.5
    b = torch.randn(K, generator=g)
    ps, pt = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    xn = (x.double() * ps.double().view(1, -1, 1, 1) + pt.double().view(1, -1, 1, 1)).requires_grad_(True)
    wd = w.double().requires_grad_(True)
    u = F.conv_transpose2d(xn, wd, b.double(), 2, 1, 1)
    dy = torch.randn(u.shape, generator=g)
    u.backward(dy.double())
    (y3, st3, bwd3), (y1, _, bwd1) = _both(lambda cls: cls(dev).deconv_all(x, w, b, (ps, pt), relu=1, bf16=1))
    ref = F.relu(u.detach())
    _check("deconv fwd %s" % (cfg,), y3, y1, ref)
    assert torch.allclose(st3[:, 0].sum(0).double(), ref.sum((0, 2, 3)), rtol=1e-4, atol=1e-4 * ref.abs().sum((0, 2, 3)).max().item())
    (dx3, dw3), (dx1, dw1) = bwd3(dy), bwd1(dy)
    _check("deconv dgrad %s" % (cfg,), dx3, dx1, xn.grad)
    _check("deconv wgrad %s" % (cfg,), dw3, dw1, wd.grad)


@pytest.mark.parametrize("where", WHERE)
def test_mode4_descriptor_decoding(env, where):
    """bf16 = 4 is its own mode: f32 tensors (a mode read as 'bf16 tensors' would have refused the f32 weight layout or read half the
    bytes), no grouped weight gradient; the modes around it decode as before"""
    dev, _ = env
    lib = _lib.get()
    sup = lambda m: lib.lbc_conv2d_wgrad_group_supported(ctypes.byref(_lib.ConvDesc(2, 8, 8, 64, 64, 3, 3, 1, 1, 0, m, 0)))
    assert [sup(m) for m in (0, 1, 2, 3, 4)] == [0, 0, 1, 1, 0]
    assert lib.lbc_version() == _lib.ABI_VERSION == 201


# ---- the executor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,backbone,h,w,n", [("birdview", "resnet18", 64, 64, 4), ("image", "resnet18", 32, 64, 5)])
def test_gradients_with_frozen_decisions_bf16x3_emulated(env, kind, backbone, h, w, n):
    """precision 3 against the exact float64 oracle (no rounding flags: bf16x3 is meant to be f32-accurate) on the executor's own
    ReLU / max-pool decisions: every gradient within 6e-4 of its tensor's largest entry (measured on the emulator: max 2.4e-4 bird-view,
    4.2e-4 image -- 2x2 maps in layer 4 and BatchNorm over 16 values amplify round-off; the f32 path: 2.5e-5 under a 1e-4 bound)"""
    dev, _ = env
    _frozen_gradient_check(dev, kind, backbone, h, w, n, 3, 6e-4)


def _census(dev, kind, backbone, h, w, n, precision):
    sd = O.make_state_dict(kind, backbone, 23, h, w)
    x, speed, cmd = _inputs(kind, n, h, w, 24)
    g = torch.Generator().manual_seed(25)
    d_all, d_sel = torch.randn((n, 4, 5, 2), generator=g), torch.randn((n, 5, 2), generator=g)
    eng, tens = engine_from_state_dict(sd, kind, backbone, h, w, n, dev, precision=precision)

    def step():
        eng.forward(x.to(dev), speed.to(dev), cmd.to(dev), True)
        eng.backward(d_sel.to(dev), d_all.to(dev))
    step()                                      # (first call: allocations and one-time setup outside the census)
    return _launch_counts(step)


X3_CLASSES = {"conv_igemm_x3_gather", "conv_igemm_x3_transposed", "conv_wgrad_x3"}


@pytest.mark.parametrize("kind,backbone,h,w,n", [("image", "resnet18", 32, 64, 2), ("birdview", "resnet18", 64, 64, 2),
                                                 pytest.param("image", "resnet34", 160, 384, 32, marks=gpu)])
def test_bf16x3_training_step_launch_census(env, kind, backbone, h, w, n):
    """a precision-3 training step runs the split kernels for every convolution but the stem, and nothing else of the convolution
    family: no exact-f32 or rounded-bf16 class, no bf16-tensor kernel (halo / LDS-DMA / tap-fused weight gradient), no bf16 weight
    copies.  Launch for launch it is precision 1's step with the convolution classes renamed."""
    dev, _ = env
    c3 = _census(dev, kind, backbone, h, w, n, 3)
    c1 = _census(dev, kind, backbone, h, w, n, 1)
    conv3 = {k for k in c3 if k.startswith("conv")}
    assert conv3 == X3_CLASSES, c3
    assert c3.get("stem_fwd", 0) >= 1 and c3.get("stem_wgrad", 0) >= 1, c3
    assert "weight_prep" not in c3, c3
    # every convolution launch of precision 1 is a split launch here (the BatchNorm passes around the stem differ: only the bf16 stem's
    # weight-gradient kernel applies the stem BatchNorm's backward itself)
    assert {k.replace("_x3", ""): v for k, v in c3.items() if k in conv3} == {k: v for k, v in c1.items() if k.startswith("conv")}, (c3, c1)
    assert c3.get("weight_transpose") == c1.get("weight_transpose"), (c3, c1)


# ---- full size on the MI355X ----------------------------------------------------------------------------------------------------
@gpu
def test_bf16x3_forward_parity_at_bench_batch_256(env):
    """student (r34, 160x384) and teacher (r18, 7x192x192) at the bench's 256 images, eval and train, precision 3 vs the float32
    oracle: max |waypoint - oracle| <= 1e-3 (the north-star bar), asserted at 8.5e-4, and the mean <= 1e-4, asserted at 5e-5.  Measured on
    MI355X (max / mean): student eval 4.2e-4 / 2.8e-5, train 5.6e-4 / 2.4e-5; teacher eval 1.3e-4 / 8.9e-6, train 1.5e-4 / 8.1e-6 -- the
    f32 path's 2e-4 is not met by the student"""
    dev, _ = env
    for kind, backbone, h, w in (("image", "resnet34", 160, 384), ("birdview", "resnet18", 192, 192)):
        n = 256
        sd = O.make_state_dict(kind, backbone, 21, h, w)
        x, speed, cmd = _inputs(kind, n, h, w, 22)
        O.calibrate_running_stats(sd, kind, backbone, x[:32], speed[:32], cmd[:32])
        eng, tens = engine_from_state_dict(sd, kind, backbone, h, w, n, dev, precision=3)
        for train in (False, True):
            ps, pa = eng.forward(x.to(dev), speed.to(dev), cmd.to(dev), train)
            with torch.no_grad():
                os_, oa = O.policy_forward({k: v.clone() for k, v in sd.items()}, kind, backbone, x, speed, cmd, train)
            e = max((pa.cpu() - oa).abs().max().item(), (ps.cpu() - os_).abs().max().item())
            em = (pa.cpu() - oa).abs().mean().item()
            _diag(dev, "engine bf16x3 %s %s N=256 train=%s: max |waypoint - oracle| = %.3e, mean %.3e" % (kind, backbone, train, e, em))
            assert e < WAYPOINT_TOLERANCE["bf16x3"] and e < 8.5e-4, (kind, train, e)
            assert em < WAYPOINT_MEAN_TOLERANCE["bf16x3"] and em < 5e-5, (kind, train, em)
        del eng, tens
        torch.cuda.empty_cache()


@gpu
def test_bf16x3_modules_match_reference_fixtures(env):
    """ImagePolicyModelSS / BirdViewPolicyModelSS with precision = "bf16x3" reproduce the real reference classes' outputs
    (tests/golden/reference_outputs.pt) within the 1e-3 bar, eval and train mode: asserted at 7e-4 (measured on MI355X: image r34 eval
    1.0e-4 / train 1.6e-4, bird-view r18 eval 4.4e-4 / train 9.4e-5)"""
    dev, _ = env
    from learningbycheating_amd.bird_view.models import BirdViewPolicyModelSS, ImagePolicyModelSS
    gold = torch.load(os.path.join(GOLD, "reference_outputs.pt"))
    for name, cls, kind, backbone in (("image_resnet34", ImagePolicyModelSS, "image", "resnet34"),
                                      ("birdview_resnet18", BirdViewPolicyModelSS, "birdview", "resnet18")):
        c = gold[name]
        sd = O.make_state_dict(kind, backbone, c["seed"])
        net = cls(backbone, all_branch=True)
        net.precision = "bf16x3"
        net.load_state_dict(sd, strict=True)
        net.to(dev)
        x, speed, cmd = seeded_inputs(kind, 2, c["input_seed"])
        onehot = O.one_hot(cmd)
        net.eval()
        with torch.no_grad():
            p, pa = net(x.to(dev), speed.to(dev), onehot.to(dev))
        e = (pa.cpu() - c["eval_preds"]).abs().max().item()
        net.train()
        with torch.no_grad():
            _, pt = net(x.to(dev), speed.to(dev), onehot.to(dev))
        et = (pt.cpu() - c["train_preds"]).abs().max().item()
        _diag(dev, "module bf16x3 %s vs reference fixture: eval %.3e, train %.3e" % (name, e, et))
        assert max(e, et) < WAYPOINT_TOLERANCE["bf16x3"] and max(e, et) < 7e-4, (name, e, et)
        assert (p.cpu() - c["eval_pred"]).abs().max().item() < WAYPOINT_TOLERANCE["bf16x3"]


@gpu
@pytest.mark.parametrize("kind,backbone,h,w,n", [("image", "resnet34", 160, 384, 32), ("birdview", "resnet18", 192, 192, 4)])
def test_bf16x3_gradients_with_frozen_decisions_full_size(env, kind, backbone, h, w, n):
    """every parameter gradient of the reference-sized networks in precision 3 vs the float64 oracle on the executor's own branch
    decisions.  Measured on MI355X: r34 N = 32 median 6.0e-4, max 1.01e-3 (location_pred.0.0.weight; every group but the head <= 7.9e-4);
    r18 bird-view N = 4 median 2.1e-4, max 3.4e-4.  Asserted: every tensor within 1.5e-3 of its largest entry, the median within 9e-4
    (the exact-f32 path: 3e-4 / 1e-4)"""
    dev, _ = env
    es = _frozen_gradient_check(dev, kind, backbone, h, w, n, 3, 1.5e-3)
    assert es[len(es) // 2] < 9e-4, es[len(es) // 2]


@gpu
@pytest.mark.parametrize("phase", [1, "birdview"])
def test_native_trainer_k_steps_bf16x3(env, phase):
    """three whole training steps (teacher, student, loss, backward, Adam) at the reference's sizes in precision 3 against the float64
    oracle, with the f32 path's structural checks (Adam update of the executor's own gradient, counters, running statistics, conv.fc).
    Measured on MI355X (worst per-tensor over the steps): phase 1 trunk gradients 2.7e-4, head / decoder 2.5e-4, Adam v 5.5e-4; bird-view
    1.4e-4 / 1.6e-4 / 2.8e-4 -- bounds 1e-3 (the f32 path: 5e-4 / 3e-4)"""
    dev, _ = env
    _k_steps(dev, phase, False, 3, 8, 1e-3, 1e-3, precision="bf16x3", fwd_tol=2e-4, stat_rtol=2e-4)
