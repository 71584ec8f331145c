// Waypoint error metrics in metres for gfx950 (include/lbc_hip.h lbc_waypoint_metrics_update): one launch adds a batch's
// displacement errors of the commanded branch -- per command c and horizon step t -- into the device record
// lbc_waypoint_metrics_state.  Nothing is read back: the validation pass syncs once, when it wants the numbers.
//
// Shape: ONE workgroup of 240 threads = 5 horizon steps x 48 sample lanes.  Thread (t, lane) walks the samples lane, lane + 48, ...
// and keeps its partial sums in registers: the command of a sample is data, so each of the four command slots is updated under a
// predicate (sum += mine ? e : 0, which adds an exact zero elsewhere) -- no dynamically indexed array, hence no scratch.  Then two
// rounds through one LDS buffer, doubles first, counters second: every thread stores its partials as row (t, value) x column lane
// (rows padded to 49 words: the readers of consecutive rows hit different banks), one barrier, and thread o < rows folds row o in a
// fixed order -- four interleaved chains of twelve, (s0 + s1) + (s2 + s3); maxima and counters one chain -- and adds the result to
// its own field of the record.  One launch, one workgroup, every field written by exactly one thread: no atomics, no workspace,
// and a given sequence of launches gives the same bits on every run.  All arithmetic is double on the f32 inputs converted
// first; at 5,120 rows per launch (batch 256) its cost does not matter, and it keeps rows near the horizon from being f32 cancellation noise.
// Reads: pred / target [N][R][2], command [N][4], loss [N] (optional), each at an index below its extent.  Writes: the record only.
#include "lbc_common.hpp"
#include "lbc_hip.h"
#include "lbc_kernels.hpp"
#include <math.h>
#include <stddef.h>

namespace {

constexpr int kSteps = 5, kLanes = 48, kThreads = kSteps * kLanes;
constexpr int kND = 25;          // doubles per thread: 5 fields x 4 commands, 4 all-branch sums, the loss sum
constexpr int kNI = 29;          // counters per thread: bad[4], within[4][4], all_bad[4], cmd_count[4], loss_bad
constexpr int kStride = kLanes + 1;
// the record as 8-byte slots (lbc_waypoint_metrics_state; c_api.cpp asserts the offsets)
constexpr int kSlotSamples = 0, kSlotUpdates = 1, kSlotCmd = 2, kSlotSumE = 6, kSlotBad = 106, kSlotWithin = 126, kSlotAllE = 206,
              kSlotAllBad = 226, kSlotLoss = 246, kSlotLossBad = 247;

struct MetricsArgs {
    const float* pred; const float* target; const float* cmd; const float* loss;
    int N, R, frame, nthr;
    double t_scale, t_shift;
    double thr[4];               // unused entries are -1: no e >= 0 passes
    double w, h, f, world_y, fixed_offset, ppm, crop;
};

struct RowErr { double dx, dy, e; };

// one (x, y) waypoint at float offset o of pred and target -> its error in metres
__device__ __forceinline__ RowErr row_err(const MetricsArgs& a, size_t o)
{
    const double x = (double)a.pred[o], y = (double)a.pred[o + 1];
    const double tx = (double)a.target[o] * a.t_scale + a.t_shift, ty = (double)a.target[o + 1] * a.t_scale + a.t_shift;
    double px, py;
    if (a.frame == 0) {
        // training/train_image_phase1.py CoordConverter: normalised image -> pixels -> rays -> ground plane at world_y -> map pixels
        const double lx = (x + 1.0) * a.w / 2.0, ly = (y + 1.0) * a.h / 2.0;
        const double xt = (lx - a.w / 2.0) / a.f, yt = (ly - a.h / 2.0) / a.f;
        const double wz = a.world_y / yt, wx = wz * xt;
        px = wx * a.ppm + a.crop / 2.0;
        py = a.crop - wz * a.ppm + a.fixed_offset * a.ppm;
    } else {
        px = (x + 1.0) * a.crop / 2.0;
        py = (y + 1.0) * a.crop / 2.0;
    }
    const double qx = (tx + 1.0) * a.crop / 2.0, qy = (ty + 1.0) * a.crop / 2.0;
    RowErr r;
    r.dx = (px - qx) / a.ppm;
    r.dy = (py - qy) / a.ppm;
    r.e = sqrt(r.dx * r.dx + r.dy * r.dy);
    return r;
}

__global__ __launch_bounds__(kThreads) void waypoint_metrics_k(MetricsArgs a, double* __restrict__ rec)
{
    __shared__ double red[kND * kSteps * kStride];       // 49,000 bytes; the counter round reuses it as int[kNI * kSteps * kStride]
    const int tid = threadIdx.x, t = tid / kLanes, lane = tid % kLanes;
    double sum_e[4] = {0, 0, 0, 0}, sum_e2[4] = {0, 0, 0, 0}, sum_dx[4] = {0, 0, 0, 0}, sum_dy[4] = {0, 0, 0, 0}, max_e[4] = {0, 0, 0, 0};
    double all_e[4] = {0, 0, 0, 0}, loss_sum = 0.0;
    int bad[4] = {0, 0, 0, 0}, within[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}, all_bad[4] = {0, 0, 0, 0};
    int cmd_count[4] = {0, 0, 0, 0}, loss_bad = 0;

    for (int s = lane; s < a.N; s += kLanes) {
        const float* cm = a.cmd + (size_t)s * 4;
        int c = -1;
#pragma unroll
        for (int k = 3; k >= 0; --k) c = (cm[k] != 0.f) ? k : c;      // the first non-zero entry
        RowErr r = {0.0, 0.0, 0.0};
        if (a.R == 20) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const RowErr rb = row_err(a, (((size_t)s * 4 + b) * kSteps + t) * 2);
                const bool fin = __builtin_isfinite(rb.e);
                all_e[b] += fin ? rb.e : 0.0;
                all_bad[b] += fin ? 0 : 1;
                if (b == c) r = rb;
            }
        } else {
            r = row_err(a, ((size_t)s * kSteps + t) * 2);
        }
        const bool fin = __builtin_isfinite(r.e);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const bool mine = cc == c, good = mine && fin;
            sum_e[cc] += good ? r.e : 0.0;
            sum_e2[cc] += good ? r.e * r.e : 0.0;
            sum_dx[cc] += good ? fabs(r.dx) : 0.0;
            sum_dy[cc] += good ? fabs(r.dy) : 0.0;
            max_e[cc] = (good && r.e > max_e[cc]) ? r.e : max_e[cc];
            bad[cc] += (mine && !fin) ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) within[k][cc] += (good && r.e <= a.thr[k]) ? 1 : 0;
            cmd_count[cc] += (mine && t == 0) ? 1 : 0;
        }
        if (t == 0 && a.loss) {
            const double l = (double)a.loss[s];
            const bool ok = __builtin_isfinite(l);
            loss_sum += ok ? l : 0.0;
            loss_bad += ok ? 0 : 1;
        }
    }

    // ---- round 1: the doubles.  Row (t, j), j = field * 4 + command | 20 + branch | 24 (loss) ----
    double* rowd = red + (size_t)(t * kND) * kStride + lane;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        rowd[(0 + cc) * kStride] = sum_e[cc];
        rowd[(4 + cc) * kStride] = sum_e2[cc];
        rowd[(8 + cc) * kStride] = sum_dx[cc];
        rowd[(12 + cc) * kStride] = sum_dy[cc];
        rowd[(16 + cc) * kStride] = max_e[cc];
        rowd[(20 + cc) * kStride] = all_e[cc];
    }
    rowd[24 * kStride] = loss_sum;
    __syncthreads();
    if (tid < kND * kSteps) {
        const int ot = tid / kND, j = tid % kND;
        const double* p = red + (size_t)tid * kStride;
        const bool is_max = j >= 16 && j < 20;
        double v;
        if (is_max) {
            v = 0.0;
            for (int i = 0; i < kLanes; ++i) v = p[i] > v ? p[i] : v;
        } else {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            for (int i = 0; i < kLanes; i += 4) { s0 += p[i]; s1 += p[i + 1]; s2 += p[i + 2]; s3 += p[i + 3]; }
            v = (s0 + s1) + (s2 + s3);
        }
        int slot = -1;
        if (j < 20) slot = kSlotSumE + (j / 4) * 20 + (j % 4) * kSteps + ot;      // sum_e, sum_e2, sum_abs_dx, sum_abs_dy, max_e: consecutive [4][5] blocks
        else if (j < 24) slot = a.R == 20 ? kSlotAllE + (j - 20) * kSteps + ot : -1;
        else slot = (ot == 0 && a.loss) ? kSlotLoss : -1;
        if (slot >= 0) {
            const double old = rec[slot];
            rec[slot] = is_max ? (v > old ? v : old) : old + v;
        }
    }
    __syncthreads();

    // ---- round 2: the counters.  Row (t, i), i = command (bad) | 4 + threshold * 4 + command | 20 + branch | 24 + command | 28 ----
    int* redi = reinterpret_cast<int*>(red);
    int* rowi = redi + (size_t)(t * kNI) * kStride + lane;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        rowi[cc * kStride] = bad[cc];
#pragma unroll
        for (int k = 0; k < 4; ++k) rowi[(4 + k * 4 + cc) * kStride] = within[k][cc];
        rowi[(20 + cc) * kStride] = all_bad[cc];
        rowi[(24 + cc) * kStride] = cmd_count[cc];
    }
    rowi[28 * kStride] = loss_bad;
    __syncthreads();
    long long* reci = reinterpret_cast<long long*>(rec);
    if (tid < kNI * kSteps) {
        const int ot = tid / kNI, i = tid % kNI;
        const int* p = redi + (size_t)tid * kStride;
        long long v = 0;
        for (int l = 0; l < kLanes; ++l) v += p[l];
        int slot = -1;
        if (i < 4) slot = kSlotBad + i * kSteps + ot;
        else if (i < 20) slot = ((i - 4) / 4 < a.nthr) ? kSlotWithin + (i - 4) * kSteps + ot : -1;      // (i - 4) = threshold * 4 + command
        else if (i < 24) slot = a.R == 20 ? kSlotAllBad + (i - 20) * kSteps + ot : -1;
        else if (i < 28) slot = ot == 0 ? kSlotCmd + (i - 24) : -1;
        else slot = (ot == 0 && a.loss) ? kSlotLossBad : -1;
        if (slot >= 0) reci[slot] += v;
    }
    if (tid == kThreads - 1) {       // (a thread that owns no row of either round)
        reci[kSlotSamples] += a.N;
        reci[kSlotUpdates] += 1;
    }
}

}  // namespace

int lbc_waypoint_metrics_launch(const lbc_waypoint_metrics_desc* d, const float* pred, const float* target, const float* command_onehot,
                                const float* loss, int N, void* state, hipStream_t s)
{
    static_assert(sizeof(lbc_waypoint_metrics_state) == 248 * 8, "lbc_waypoint_metrics_state layout (include/lbc_hip.h)");
    static_assert(offsetof(lbc_waypoint_metrics_state, cmd_count) == 8 * kSlotCmd && offsetof(lbc_waypoint_metrics_state, sum_e) == 8 * kSlotSumE &&
                  offsetof(lbc_waypoint_metrics_state, max_e) == 8 * (kSlotSumE + 80) && offsetof(lbc_waypoint_metrics_state, bad) == 8 * kSlotBad &&
                  offsetof(lbc_waypoint_metrics_state, within) == 8 * kSlotWithin && offsetof(lbc_waypoint_metrics_state, all_sum_e) == 8 * kSlotAllE &&
                  offsetof(lbc_waypoint_metrics_state, all_bad) == 8 * kSlotAllBad && offsetof(lbc_waypoint_metrics_state, loss_sum) == 8 * kSlotLoss &&
                  offsetof(lbc_waypoint_metrics_state, loss_bad) == 8 * kSlotLossBad, "lbc_waypoint_metrics_state slots");
    static_assert(kNI * kSteps <= kThreads - 1 && kNI * 4 <= kND * 8, "counter round fits the threads and the LDS buffer");
    LBC_REQUIRE(d, "waypoint_metrics: null descriptor");
    LBC_REQUIRE(d->struct_size == sizeof(lbc_waypoint_metrics_desc),
                "waypoint_metrics: lbc_waypoint_metrics_desc.struct_size is %u, this library (ABI %d) accepts %zu -- initialise the descriptor "
                "with LBC_WAYPOINT_METRICS_DESC_INIT", d->struct_size, LBC_HIP_ABI_VERSION, sizeof(lbc_waypoint_metrics_desc));
    LBC_REQUIRE(state && (reinterpret_cast<uintptr_t>(state) & 7) == 0, "waypoint_metrics: the record (%p) must be non-null and 8-byte aligned", state);
    LBC_REQUIRE(pred && target && command_onehot, "waypoint_metrics: null argument (pred %p, target %p, command %p)", (const void*)pred,
                (const void*)target, (const void*)command_onehot);
    LBC_REQUIRE(N >= 0, "waypoint_metrics: N = %d is negative", N);
    LBC_REQUIRE(d->rows == 5 || d->rows == 20, "waypoint_metrics: rows = %d, must be 5 (one branch) or 20 (four branches)", d->rows);
    LBC_REQUIRE(d->pred_frame == 0 || d->pred_frame == 1, "waypoint_metrics: pred_frame = %d, must be 0 (camera) or 1 (map)", d->pred_frame);
    LBC_REQUIRE(d->nthresholds >= 0 && d->nthresholds <= 4, "waypoint_metrics: nthresholds = %d outside 0..4", d->nthresholds);
    for (int k = 0; k < d->nthresholds; ++k)
        LBC_REQUIRE(isfinite(d->thresholds_m[k]) && d->thresholds_m[k] >= 0.0, "waypoint_metrics: threshold %d (%g m) is negative or not finite", k,
                    d->thresholds_m[k]);
    if (N == 0) return LBC_OK;
    MetricsArgs a;
    a.pred = pred; a.target = target; a.cmd = command_onehot; a.loss = loss;
    a.N = N; a.R = d->rows; a.frame = d->pred_frame; a.nthr = d->nthresholds;
    a.t_scale = d->target_scale; a.t_shift = d->target_shift;
    for (int k = 0; k < 4; ++k) a.thr[k] = k < d->nthresholds ? d->thresholds_m[k] : -1.0;
    const lbc_camera& c = d->camera;
    a.w = c.w; a.h = c.h; a.world_y = c.world_y; a.fixed_offset = c.fixed_offset; a.ppm = c.pixels_per_meter; a.crop = c.crop_size;
    a.f = (double)c.w / (2.0 * tan((double)c.fov * 3.14159265358979323846 / 360.0));      // the focal length, once, on the host
    // algorithmic bytes: pred + target + command (+ loss) read once
    LbcProfScope prof("waypoint_metrics", 0.0, (double)N * (16.0 * d->rows + 16.0 + (loss ? 4.0 : 0.0)), s);
    hipLaunchKernelGGL(waypoint_metrics_k, dim3(1), dim3(kThreads), 0, s, a, static_cast<double*>(state));
    return lbc_check_launch("waypoint_metrics");
}
