// C-ABI entry points (include/lbc_hip.h) over the internal launchers.
#include "conv_desc.hpp"
#include "lbc_common.hpp"
#include "lbc_hip.h"
#include "lbc_kernels.hpp"
#include <stddef.h>
#include <string.h>

extern "C" {

const char* lbc_backend(void)
{
#ifdef LBC_HIP_EMULATED_FOR_TESTS
    return "emu-cpu";
#else
    return "hip-gfx950";
#endif
}
int lbc_version(void) { return LBC_HIP_ABI_VERSION; }

size_t lbc_adam_state_bytes(void) { return sizeof(lbc_adam_state); }

int lbc_adam_step_guarded(const lbc_adam_chunk* chunks_dev, int nchunks, double lr, double beta1, double beta2,
                          double eps, double weight_decay, lbc_adam_state* state_dev, lbc_stream_t stream)
{
    static_assert(sizeof(lbc_adam_chunk) == sizeof(AdamChunk), "chunk layout");
    static_assert(sizeof(lbc_adam_state) == 40, "lbc_adam_state layout (include/lbc_hip.h)");
    return lbc_adam_guarded_launch(reinterpret_cast<const AdamChunk*>(chunks_dev), nchunks, lr, beta1, beta2, eps, weight_decay,
                                   state_dev, (hipStream_t)stream);
}

size_t lbc_adam_clip_state_bytes(int nchunks) { return sizeof(lbc_adam_clip_state) + sizeof(double) * (size_t)(nchunks > 0 ? nchunks : 0); }

int lbc_adam_step_clipped(const lbc_adam_chunk* chunks_dev, int nchunks, double lr, double beta1, double beta2,
                          double eps, double weight_decay, double max_norm, lbc_adam_clip_state* state_dev, lbc_stream_t stream)
{
    static_assert(sizeof(lbc_adam_clip_state) == 64 && offsetof(lbc_adam_clip_state, grad_norm) == sizeof(lbc_adam_state) &&
                  offsetof(lbc_adam_clip_state, clipped_total) == 56, "lbc_adam_clip_state layout (include/lbc_hip.h)");
    return lbc_adam_clipped_launch(reinterpret_cast<const AdamChunk*>(chunks_dev), nchunks, lr, beta1, beta2, eps, weight_decay,
                                   max_norm, state_dev, (hipStream_t)stream);
}

size_t lbc_adam_recipe_state_bytes(int nchunks) { return sizeof(lbc_adam_recipe_state) + sizeof(double) * (size_t)(nchunks > 0 ? nchunks : 0); }

int lbc_adam_step_recipe(const lbc_adam_chunk* chunks_dev, int nchunks, const lbc_adam_recipe* recipe, float* const* ema_dev,
                         lbc_adam_recipe_state* state_dev, lbc_stream_t stream)
{
    static_assert(sizeof(lbc_adam_recipe_state) == 88 && offsetof(lbc_adam_recipe_state, lr) == sizeof(lbc_adam_clip_state) &&
                  offsetof(lbc_adam_recipe_state, clipped_total) == offsetof(lbc_adam_clip_state, clipped_total) &&
                  offsetof(lbc_adam_recipe_state, decay_factor) == 72 && offsetof(lbc_adam_recipe_state, ema_updates) == 80,
                  "lbc_adam_recipe_state layout (include/lbc_hip.h)");
    return lbc_adam_recipe_launch(reinterpret_cast<const AdamChunk*>(chunks_dev), nchunks, recipe, ema_dev, state_dev, (hipStream_t)stream);
}

int lbc_grad_accumulate(const float* g, float* acc, long long n, int first, lbc_stream_t stream)
{
    return lbc_grad_accumulate_launch(g, acc, n, first, (hipStream_t)stream);
}

size_t lbc_waypoint_metrics_state_bytes(void) { return sizeof(lbc_waypoint_metrics_state); }

int lbc_waypoint_metrics_update(const lbc_waypoint_metrics_desc* desc, const float* pred, const float* target, const float* command_onehot,
                                const float* loss, int N, void* state, lbc_stream_t stream)
{
    static_assert(sizeof(lbc_waypoint_metrics_desc) == 96 && offsetof(lbc_waypoint_metrics_desc, target_scale) == 16 &&
                  offsetof(lbc_waypoint_metrics_desc, thresholds_m) == 32 && offsetof(lbc_waypoint_metrics_desc, camera) == 64,
                  "lbc_waypoint_metrics_desc layout (include/lbc_hip.h)");
    return lbc_waypoint_metrics_launch(desc, pred, target, command_onehot, loss, N, state, (hipStream_t)stream);
}

int lbc_visuals_image_shape(const lbc_visuals_desc* desc, int* rows, int* cols) { return lbc_visuals_shape(desc, rows, cols); }

int lbc_visuals_render(const lbc_visuals_desc* desc, const void* rgb, const void* birdview, const float* pred, const float* teacher_or_target,
                       const float* command_onehot, const float* loss, const unsigned char* font, unsigned char* out, lbc_stream_t stream)
{
    static_assert(sizeof(lbc_visuals_desc) == 76 && offsetof(lbc_visuals_desc, camera) == 4 && offsetof(lbc_visuals_desc, mode) == 32 &&
                  offsetof(lbc_visuals_desc, N) == 48 && offsetof(lbc_visuals_desc, birdview_f32) == 72, "lbc_visuals_desc layout (include/lbc_hip.h)");
    return lbc_visuals_launch(desc, rgb, birdview, pred, teacher_or_target, command_onehot, loss, font, out, (hipStream_t)stream);
}

size_t lbc_agent_state_bytes(int n_agents) { return n_agents > 0 ? sizeof(lbc_agent_state) * (size_t)n_agents : 0; }

int lbc_agent_control(const lbc_agent_desc* desc, const float* pred, const float* speed, const float* command_onehot,
                      const unsigned char* active, int N, void* state, double* out, lbc_stream_t stream)
{
    static_assert(sizeof(lbc_agent_desc) == 256 && offsetof(lbc_agent_desc, w) == 16 && offsetof(lbc_agent_desc, gap) == 72 &&
                  offsetof(lbc_agent_desc, steer_points) == 88 && offsetof(lbc_agent_desc, turn_pid) == 104 &&
                  offsetof(lbc_agent_desc, speed_pid) == 200 && offsetof(lbc_agent_desc, turn_window) == 224 &&
                  offsetof(lbc_agent_desc, engine_brake_threshold) == 232, "lbc_agent_desc layout (include/lbc_hip.h)");
    return lbc_agent_control_launch(desc, pred, speed, command_onehot, active, N, state, out, (hipStream_t)stream);
}

int lbc_agent_reset(const unsigned char* mask, int N, void* state, lbc_stream_t stream)
{
    return lbc_agent_reset_launch(mask, N, state, (hipStream_t)stream);
}

// Every entry point that takes a descriptor checks it: struct_size must cover the fields of the first checked layout (ABI 200: everything up to
// and including split_workspace_bytes) and must not exceed this library's struct.  A host built against an OLDER header of the same major
// ABI (fewer trailing fields) stays valid: whoever appends a field must read it only where struct_size covers it (today the checked
// layout IS the struct: the two bounds coincide).  A host that forgot LBC_CONV_DESC_INIT (struct_size 0 / garbage) is refused.
static const unsigned kDescMinSize = (unsigned)(offsetof(lbc_conv_desc, split_workspace_bytes) + sizeof(((lbc_conv_desc*)0)->split_workspace_bytes));
static bool desc_ok(const lbc_conv_desc* d, const char* who)
{
    if (!d) { lbc_set_error("%s: null descriptor", who); return false; }
    if (d->struct_size < kDescMinSize || d->struct_size > sizeof(lbc_conv_desc)) {
        lbc_set_error("%s: lbc_conv_desc.struct_size is %u, this library (ABI %d) accepts %u .. %zu -- initialise the descriptor with LBC_CONV_DESC_INIT "
                      "and build the host against a lbc_hip.h of this ABI", who, d->struct_size, LBC_HIP_ABI_VERSION, kDescMinSize, sizeof(lbc_conv_desc));
        return false;
    }
    return true;
}
#define LBC_DESC(d, who) do { if (!desc_ok((d), (who))) return LBC_EINVAL; } while (0)

// lbc_conv_desc.bf16 = 4 (split bf16, "bf16x3") reads f32 tensors; every other mode >= 2 means bf16 tensors, as before
static int act_bf16_mode(int m) { return m >= 2 && m != 4; }

// the descriptor's geometry and precision as the shared builders (conv_desc.hpp) take them
static ConvGeom geom_of(const lbc_conv_desc* d)
{
    ConvGeom g;
    g.N = d->N; g.H = d->H; g.W = d->W; g.Cin = d->C; g.Cout = d->K;
    g.kh = d->KH; g.kw = d->KW; g.s = d->S; g.p = d->P;
    g.bf16 = d->bf16 != 0; g.act_bf16 = act_bf16_mode(d->bf16); g.w_bf16 = d->bf16 == 3; g.x3 = d->bf16 == 4;
    return g;
}

static void attach_split(IgemmArgs& a, const lbc_conv_desc* d) { a.split_ws = static_cast<float*>(d->split_workspace); a.split_ws_floats = (long long)(d->split_workspace_bytes / 4); }

// gather-form launch over geometry g (Conv2d forward, ConvTranspose2d input gradient); d: the caller's split scratch
static int conv_fwd_impl(const ConvGeom& g, const lbc_conv_desc* d, int relu, const void* x, const void* w, const float* bias,
                         const void* resid, const float* pre_scale, const float* pre_shift, int pre_relu,
                         void* y, float* stats, int* stats_rows, hipStream_t s)
{
    IgemmArgs a = lbc_conv_fwd_args(g, pre_scale != nullptr);
    a.relu = relu;
    attach_split(a, d);
    a.pre_scale = pre_scale; a.pre_shift = pre_shift; a.pre_relu = pre_relu;
    a.resid = resid;
    // NB a row-count query must describe the launch it is for: pass the same pre_scale and resid (NULL or not) as the real call
    const IgemmPlan p = lbc_igemm_plan(a, /*wmajor=*/1, /*mode=*/0);
    if (stats_rows) *stats_rows = p.rows;
    if (!y) return LBC_OK;   // query only
    a.x = x; a.w = w; a.y = y; a.bias = bias; a.stats = stats;
    return lbc_igemm_launch(a, p, s);
}

int lbc_conv2d_fwd(const lbc_conv_desc* d, const void* x, const void* w, const float* bias,
                   const void* resid, const float* pre_scale, const float* pre_shift, int pre_relu,
                   void* y, float* stats, int* stats_rows, lbc_stream_t stream)
{
    LBC_DESC(d, "conv2d_fwd");
    return conv_fwd_impl(geom_of(d), d, d->relu, x, w, bias, resid, pre_scale, pre_shift, pre_relu, y, stats, stats_rows, (hipStream_t)stream);
}

// dgrad of a Conv2d with geometry g: gathered tensor = dy [N,OH,OW,K], output = dx [N,H,W,C] (every pixel of it is written: at
// stride 2 the launch covers the four output-parity phases)
static int conv_dgrad_impl(const ConvGeom& g, const lbc_conv_desc* d, const void* dy, const void* w, int wmajor, const void* resid,
                           const float* bias, const float* pre_scale, const float* pre_shift, int pre_relu,
                           int relu, void* dx, float* stats, int* stats_rows, hipStream_t s)
{
    LBC_REQUIRE(g.s == 1 || (g.H % 2 == 0 && g.W % 2 == 0), "dgrad s2: odd spatial size %dx%d", g.H, g.W);
    IgemmArgs a = lbc_conv_dgrad_args(g);
    a.x = dy; a.w = w; a.y = dx; a.resid = resid; a.bias = bias; a.relu = relu;
    a.pre_scale = pre_scale; a.pre_shift = pre_shift; a.pre_relu = pre_relu;
    attach_split(a, d);
    a.stats = stats;
    const IgemmPlan p = lbc_igemm_plan(a, wmajor, 1);
    if (stats_rows) *stats_rows = (a.nphase == 4 ? 4 : 1) * p.rows;
    if (!dx) return LBC_OK;
    return lbc_igemm_launch(a, p, s);
}

int lbc_weight_transpose_f32(const float* w, float* wt, int A, int T, int B, lbc_stream_t stream)
{
    LBC_REQUIRE(w && wt && A > 0 && T > 0 && B > 0, "weight_transpose: bad arguments");
    return lbc_weight_transpose(w, wt, A, T, B, (hipStream_t)stream);
}

int lbc_conv2d_dgrad(const lbc_conv_desc* d, const void* dy, const void* w, const void* resid,
                     void* dx, lbc_stream_t stream)
{
    LBC_DESC(d, "conv2d_dgrad");
    LBC_REQUIRE(!d->bf16 || d->w_transposed, "conv2d_dgrad: bf16 needs w_transposed = 1 (see lbc_weight_transpose_f32)");
    // weights [K][T][C]: depth index (gathered channel) = k is the slow axis -> wmajor 0 with row length C;
    // the transposed copy [C][T][K] is depth-contiguous -> wmajor 1
    return conv_dgrad_impl(geom_of(d), d, dy, w, /*wmajor=*/d->w_transposed ? 1 : 0, resid, nullptr, nullptr, nullptr, 0, 0, dx, nullptr, nullptr,
                           (hipStream_t)stream);
}

// ConvTranspose2d(C->K, 3, 2, 1, 1) forward == dgrad of a Conv2d(K->C, 3, 2, 1) whose weight tensor
// [C_T][kh][kw][K_T] is exactly the transposed conv's channels_last weight (lbc_deconv_as_conv).

int lbc_deconv3x3s2_fwd(const lbc_conv_desc* d, const void* x, const void* w, const float* bias,
                        const float* pre_scale, const float* pre_shift, int pre_relu,
                        void* y, float* stats, int* stats_rows, lbc_stream_t stream)
{
    LBC_DESC(d, "deconv3x3s2_fwd");
    LBC_REQUIRE(d->KH == 3 && d->KW == 3 && d->S == 2 && d->P == 1, "deconv3x3s2_fwd: geometry must be k3 s2 p1 op1");
    LBC_REQUIRE(!d->bf16 || d->w_transposed, "deconv3x3s2_fwd: bf16 needs w_transposed = 1 (see lbc_weight_transpose_f32)");
    return conv_dgrad_impl(lbc_deconv_as_conv(geom_of(d)), d, x, w, /*wmajor=*/d->w_transposed ? 1 : 0, nullptr, bias, pre_scale, pre_shift, pre_relu,
                           d->relu, y, stats, stats_rows, (hipStream_t)stream);
}

int lbc_deconv3x3s2_dgrad(const lbc_conv_desc* d, const void* dy, const void* w, void* dx, lbc_stream_t stream)
{
    LBC_DESC(d, "deconv3x3s2_dgrad");
    LBC_REQUIRE(d->KH == 3 && d->KW == 3 && d->S == 2 && d->P == 1, "deconv3x3s2_dgrad: geometry must be k3 s2 p1 op1");
    // forward gather conv over dy with the deconv weight read as [O=C_T][kh][kw][I=K_T]
    return conv_fwd_impl(lbc_deconv_as_conv(geom_of(d)), d, /*relu=*/0, dy, w, nullptr, nullptr, nullptr, nullptr, 0, dx, nullptr, nullptr,
                         (hipStream_t)stream);
}


// a weight gradient's descriptor with the split its workspace query sized
static WgradArgs with_split(WgradArgs a) { a.nsplit = lbc_wgrad_pick_split(a); return a; }
static WgradArgs conv_wgrad_args(const lbc_conv_desc* d) { return with_split(lbc_conv_wgrad_args(geom_of(d))); }
static WgradArgs deconv_wgrad_args(const lbc_conv_desc* d) { return with_split(lbc_deconv_wgrad_args(geom_of(d))); }

size_t lbc_conv2d_wgrad_workspace(const lbc_conv_desc* d)
{
    if (!desc_ok(d, "conv2d_wgrad_workspace")) return 0;
    const WgradArgs a = conv_wgrad_args(d);
    return (size_t)a.nsplit * lbc_wgrad_count(a) * sizeof(float);
}

int lbc_conv2d_wgrad(const lbc_conv_desc* d, const void* x, const void* dy,
                     const float* pre_scale, const float* pre_shift, int pre_relu,
                     float* dw, float beta, void* workspace, lbc_stream_t stream)
{
    LBC_DESC(d, "conv2d_wgrad");
    LBC_REQUIRE(workspace, "conv2d_wgrad: null workspace");
    WgradArgs a = conv_wgrad_args(d);
    a.p = dy; a.q = x;
    a.q_scale = pre_scale; a.q_shift = pre_shift; a.q_relu = pre_relu;
    return lbc_wgrad_run(a, (float*)workspace, dw, beta, (hipStream_t)stream);
}

// n same-shaped 3x3 / stride-1 convolutions on bf16 tensors in one launch (+ one reduce launch)
int lbc_conv2d_wgrad_group_supported(const lbc_conv_desc* d)
{
    if (!desc_ok(d, "conv2d_wgrad_group_supported")) return 0;
    WgradArgs a = conv_wgrad_args(d);
    a.p = d; a.q = d;     // (eligibility looks at geometry and flags only)
    return lbc_wgrad_tr_eligible(a) ? 1 : 0;
}

size_t lbc_conv2d_wgrad_group_workspace(const lbc_conv_desc* d, int n)
{
    if (!d || n < 1 || !lbc_conv2d_wgrad_group_supported(d)) return 0;
    WgradArgs a = conv_wgrad_args(d);
    return (size_t)lbc_wgrad_tr_group_split(a, n) * n * (size_t)a.CP * 9 * (size_t)a.CQ * sizeof(float);
}

int lbc_conv2d_wgrad_group(const lbc_conv_desc* d, int n, const void* const* x, const void* const* dy,
                           const float* const* pre_scale, const float* const* pre_shift, int pre_relu,
                           float* const* dw, void* workspace, lbc_stream_t stream)
{
    LBC_DESC(d, "conv2d_wgrad_group");
    LBC_REQUIRE(x && dy && dw && workspace && n >= 1 && n <= kLbcWgradGroupMax, "conv2d_wgrad_group: null argument or group size %d outside [1,%d]", n, kLbcWgradGroupMax);
    LBC_REQUIRE(lbc_conv2d_wgrad_group_supported(d), "conv2d_wgrad_group: 3x3 / stride 1 / pad 1 on bf16 tensors (bf16 mode >= 2), channels multiples of 64");
    WgradArgs a = conv_wgrad_args(d);
    a.nsplit = lbc_wgrad_tr_group_split(a, n);
    a.q_relu = pre_relu;
    const size_t count = (size_t)a.CP * 9 * (size_t)a.CQ;
    WgradGroup g;
    memset(&g, 0, sizeof(g));
    g.n = n;
    for (int i = 0; i < n; ++i) {
        g.p[i] = dy[i]; g.q[i] = x[i];
        g.q_scale[i] = pre_scale ? pre_scale[i] : nullptr; g.q_shift[i] = pre_shift ? pre_shift[i] : nullptr;
        g.out[i] = a.nsplit == 1 ? dw[i] : (float*)workspace + (size_t)i * a.nsplit * count;
    }
    a.q_scale = g.q_scale[0]; a.q_shift = g.q_shift[0];
    const int rc = lbc_wgrad_tr_group_launch(a, g, (hipStream_t)stream);
    if (rc || a.nsplit == 1) return rc;
    return lbc_splitk_reduce_group((const float*)workspace, a.nsplit, (long long)count, n, dw, (hipStream_t)stream);
}

// ConvTranspose2d wgrad: P-side = x (dense rows), Q-side = dy gathered with stride 2 (lbc_deconv_wgrad_args)
size_t lbc_deconv3x3s2_wgrad_workspace(const lbc_conv_desc* d)
{
    if (!desc_ok(d, "deconv3x3s2_wgrad_workspace")) return 0;
    const WgradArgs a = deconv_wgrad_args(d);
    return (size_t)a.nsplit * lbc_wgrad_count(a) * sizeof(float);
}

int lbc_deconv3x3s2_wgrad(const lbc_conv_desc* d, const void* x, const void* dy,
                          const float* pre_scale, const float* pre_shift, int pre_relu,
                          float* dw, float beta, void* workspace, lbc_stream_t stream)
{
    LBC_DESC(d, "deconv3x3s2_wgrad");
    LBC_REQUIRE(workspace, "deconv_wgrad: null workspace");
    LBC_REQUIRE(!pre_relu, "deconv_wgrad: ReLU-on-load of the dense operand is not supported");
    WgradArgs a = deconv_wgrad_args(d);
    a.p = x; a.q = dy;
    a.p_scale = pre_scale; a.p_shift = pre_shift;
    return lbc_wgrad_run(a, (float*)workspace, dw, beta, (hipStream_t)stream);
}

}  // extern "C"
