"""Characterisation of the convolution planner through the C ABI's query-only calls: lbc_conv2d_fwd / lbc_deconv3x3s2_fwd with a
NULL output launch nothing and answer the statistics rows (= M tiles of the kernel the launch would take), so the table pins, on the
CPU and in milliseconds, which tile shape every launch of the grid gets under every option the kernel tests use.
tests/golden/conv_stats_rows.json holds the answers of the commit before the descriptor builders / lbc_igemm_plan replaced the
hand-written call sites (tests/golden/make_conv_rows_fixture.py); a policy change regenerates it, a refactor must not move it."""
import ctypes
import hashlib
import json
import os

import torch

from learningbycheating_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_stats_rows.json")

CHANNELS = [(64, 64), (64, 128), (128, 128), (256, 512), (640, 256)]
SPATIAL = [(4, 8), (10, 24), (20, 48)]             # H x W: 8, 24 and 48 wide
BATCHES = [1, 3, 32]
MODES = [0, 1, 3, 4]                               # lbc_conv_desc.bf16
KERNELS = [(3, 1, 1), (3, 2, 1), (1, 2, 0)]        # (k, stride, pad) of the Conv2d queries
_MIN1 = ("LBC_GEMM256_MIN_TILES", 1)
OPTIONS = ([[]] + [[("LBC_FORCE_CFG", v)] for v in (0, 1, 2)] + [[("LBC_GEMM256_CFG", v), _MIN1] for v in range(7)] +
           [[("LBC_HDMA_CFG", v), _MIN1] for v in (1, 2, 3, 4)] + [[("LBC_HDMA_CFG", 4)], [("LBC_NO_HDMA", 1)], [("LBC_NO_HDMA", 1), _MIN1],
            [("LBC_NO_GEMM256", 1)], [_MIN1], [("LBC_NO_GLDS_PHASED", 1)], [("LBC_NO_GLDS_PHASED", 1), _MIN1], [("LBC_NO_C64P_PRE", 1)],
            [("LBC_NO_C64P_PRE", 1), _MIN1], [("LBC_HDMAP_SPLIT", 0), _MIN1], [("LBC_HDMAP_SPLIT", 2), _MIN1]])


def cases():
    """(op, N, H, W, C, K, k, s, p, mode, w_transposed, pre, resid) in a fixed order"""
    out = []
    for c, k in CHANNELS:
        for h, w in SPATIAL:
            for n in BATCHES:
                for mode in MODES:
                    for kk, s, p in KERNELS:
                        for pre in (0, 1):
                            for resid in (0, 1):
                                out.append(("conv", n, h, w, c, k, kk, s, p, mode, 0, pre, resid))
                    for wt in ((0, 1) if mode == 0 else (1,)):       # (the bf16 modes need the transposed weight copy)
                        for pre in (0, 1):
                            out.append(("deconv", n, h, w, c, k, 3, 2, 1, mode, wt, pre, 0))
    return out


def cases_digest():
    return hashlib.sha256(json.dumps([cases(), OPTIONS]).encode()).hexdigest()


def query_rows(lib):
    """the stats_rows answer of every case with the options as they are set now"""
    dummy = torch.zeros(1024)      # stands for pre_scale / pre_shift / resid: a query only tests them for NULL
    dp = ctypes.c_void_p(dummy.data_ptr())
    rows = ctypes.c_int()
    out = []
    for op, n, h, w, c, k, kk, s, p, mode, wt, pre, resid in cases():
        d = _lib.ConvDesc(n, h, w, c, k, kk, kk, s, p, 1, mode, wt)
        rows.value = -1
        if op == "conv":
            rc = lib.lbc_conv2d_fwd(ctypes.byref(d), None, None, None, dp if resid else None, dp if pre else None, dp if pre else None, pre,
                                    None, None, ctypes.byref(rows), None)
        else:
            rc = lib.lbc_deconv3x3s2_fwd(ctypes.byref(d), None, None, None, dp if pre else None, dp if pre else None, 0, None, None,
                                         ctypes.byref(rows), None)
        assert rc == 0, (op, n, h, w, c, k, kk, s, p, mode, wt, pre, resid, lib.lbc_last_error().decode())
        out.append(rows.value)
    return out


def test_conv_stats_rows_match_the_recorded_table(env, lbc_config):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["cases_digest"] == cases_digest(), "the case grid changed: regenerate tests/golden/conv_stats_rows.json at the policy's commit"
    assert len(golden["rows"]) == len(OPTIONS)
    lib = _lib.get()
    cs = cases()
    for opts, want in zip(OPTIONS, golden["rows"]):
        for name, value in opts:
            lbc_config(name, value)
        got = query_rows(lib)
        for name, _ in opts:
            lbc_config(name, -1)
        assert len(got) == len(want) == len(cs)
        bad = [(c, g, w) for c, g, w in zip(cs, got, want) if g != w]
        assert not bad, "options %s: %d of %d launches changed their row count, first (case, got, recorded): %s" % (opts, len(bad), len(cs), bad[:5])
    # the table is not trivial: more than one tile height occurs for one and the same launch across the options
    assert any(len({r[i] for r in golden["rows"]}) > 2 for i in range(len(cs)))
