// Launch descriptors of the convolution family, built in ONE place for the executor (engine.cpp) and the C ABI (c_api.cpp).  Every
// builder returns a zero-initialised descriptor with the whole geometry and the precision flags set and NULL tensor pointers: a call
// site attaches pointers, epilogue flags and scratch, then plans (lbc_igemm_plan) and launches.
#pragma once
#include <string.h>

#include "lbc_common.hpp"

// Conv2d(Cin -> Cout, kh x kw, stride s, padding p) over an NHWC tensor [N][H][W][Cin], with the precision as the kernels read it
struct ConvGeom {
    int N, H, W, Cin, Cout, kh, kw, s, p;
    int bf16, act_bf16, w_bf16, x3;
    int OH() const { return (H + 2 * p - kh) / s + 1; }
    int OW() const { return (W + 2 * p - kw) / s + 1; }
};

// ConvTranspose2d(Cin -> Cout, 3, 2, 1, 1) over [N][H][W][Cin] as the Conv2d(Cout -> Cin, 3, 2, 1) over [N][2H][2W][Cout] whose input
// gradient it is: the transposed convolution's channels_last weight [Cin][kh][kw][Cout] is exactly that convolution's weight tensor
inline ConvGeom lbc_deconv_as_conv(ConvGeom d)
{
    return ConvGeom{d.N, 2 * d.H, 2 * d.W, d.Cout, d.Cin, 3, 3, 2, 1, d.bf16, d.act_bf16, d.w_bf16, d.x3};
}

inline IgemmArgs lbc_igemm_args_zero(const ConvGeom& g)
{
    IgemmArgs a;
    memset(&a, 0, sizeof(a));
    a.N = g.N; a.KH = g.kh; a.KW = g.kw; a.S = g.s; a.P = g.p;
    a.bf16 = g.bf16; a.act_bf16 = g.act_bf16; a.w_bf16 = g.w_bf16; a.x3 = g.x3;
    return a;
}

// Conv2d forward (mode 0, gather).  prologue: the launch applies a BatchNorm on load -- the pickers only test pre_scale for NULL, so a
// planning query gets a placeholder that is never read; a real launch overwrites pre_scale / pre_shift with its tensors.
inline IgemmArgs lbc_conv_fwd_args(const ConvGeom& g, bool prologue)
{
    static const float placeholder = 0.f;
    IgemmArgs a = lbc_igemm_args_zero(g);
    a.H = g.H; a.W = g.W; a.C = g.Cin;
    a.OH = g.OH(); a.OW = g.OW(); a.K = g.Cout;
    a.LH = a.OH; a.LW = a.OW; a.ostep = 1;
    a.M = g.N * a.OH * a.OW;
    if (prologue) { a.pre_scale = &placeholder; a.pre_shift = &placeholder; }
    return a;
}

// Conv2d input gradient (mode 1, transposed): gathered tensor dy [N][OH][OW][Cout], output dx [N][H][W][Cin].  Stride 1: the dense
// lattice.  Stride 2: the lattice of one output-parity phase, all four phases in one launch -- a 1x1 kernel has taps in the even-even
// phase only, and a caller that accumulates onto dx in place (skip_empty_phases) launches just that one.
inline IgemmArgs lbc_conv_dgrad_args(const ConvGeom& g, bool skip_empty_phases = false)
{
    IgemmArgs a = lbc_igemm_args_zero(g);
    a.H = g.OH(); a.W = g.OW(); a.C = g.Cout;
    a.OH = g.H; a.OW = g.W; a.K = g.Cin;
    a.ostep = g.s == 1 ? 1 : 2;
    a.LH = g.H / a.ostep; a.LW = g.W / a.ostep;
    if (g.s != 1) a.nphase = (skip_empty_phases && g.kh == 1 && g.kw == 1) ? 1 : 4;     // (statistics rows of phase ph: ph * per + tile)
    a.M = g.N * a.LH * a.LW;
    return a;
}

// ConvTranspose2d forward and input gradient (the gather form over the 2H x 2W tensor), from the transposed convolution's own geometry
inline IgemmArgs lbc_deconv_fwd_args(const ConvGeom& d) { return lbc_conv_dgrad_args(lbc_deconv_as_conv(d)); }
inline IgemmArgs lbc_deconv_dgrad_args(const ConvGeom& d) { return lbc_conv_fwd_args(lbc_deconv_as_conv(d), false); }

// Conv2d weight gradient: P = dy (dense rows), Q = x gathered; nsplit is the caller's (lbc_wgrad_pick_split, clamped to its scratch)
inline WgradArgs lbc_conv_wgrad_args(const ConvGeom& g)
{
    WgradArgs a;
    memset(&a, 0, sizeof(a));
    a.N = g.N; a.OH = g.OH(); a.OW = g.OW(); a.CP = g.Cout;
    a.H = g.H; a.W = g.W; a.CQ = g.Cin;
    a.KH = g.kh; a.KW = g.kw; a.S = g.s; a.P = g.p;
    a.bf16 = g.bf16; a.act_bf16 = g.act_bf16; a.x3 = g.x3;
    return a;
}
// ConvTranspose2d weight gradient: dw[c][kh][kw][k] = sum x'[n,iy,ix,c] * dy[n,2iy-1+kh,2ix-1+kw,k] == the Conv2d weight gradient
// of the transposed geometry with P = x (dense rows) and Q = dy gathered with stride 2
inline WgradArgs lbc_deconv_wgrad_args(const ConvGeom& d) { return lbc_conv_wgrad_args(lbc_deconv_as_conv(d)); }

// floats of one split-K slab of a weight gradient (= of the gradient itself), and of the slabs lbc_wgrad_pick_split asks for
inline size_t lbc_wgrad_count(const WgradArgs& a) { return (size_t)a.CP * (size_t)(a.KH * a.KW) * (size_t)a.CQ; }
inline size_t lbc_wgrad_need(const WgradArgs& a) { return (size_t)lbc_wgrad_pick_split(a) * lbc_wgrad_count(a); }

// One weight gradient of a.nsplit slabs: grad = beta * grad + sum of the slabs written to `slabs`; a single slab with beta = 0 is
// written as the gradient itself (no reduce launch)
inline int lbc_wgrad_run(WgradArgs a, float* slabs, float* grad, float beta, hipStream_t s)
{
    const bool direct = a.nsplit == 1 && beta == 0.f;
    a.partial = direct ? grad : slabs;
    const int rc = lbc_wgrad_launch(a, s);
    if (rc || direct) return rc;
    return lbc_splitk_reduce(a.partial, a.nsplit, (long long)lbc_wgrad_count(a), grad, beta, s);
}
