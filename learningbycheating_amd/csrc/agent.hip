// The agent half of the tick for gfx950 (include/lbc_hip.h lbc_agent_control / lbc_agent_reset): the network's five waypoints ->
// steer / throttle / brake, for N independent agents in ONE launch behind the forward, so that a captured tick ends in the controls
// and the controller state never leaves the device.
//
// Shape: one thread per agent, 64-thread workgroups.  An agent is ~300 double operations and 42 doubles of state; at the N <= a few
// dozen agents of a simulator the launch is latency, not throughput, so nothing is shared between threads: no LDS, no atomics, every
// word of `out` and of a record is written by exactly one thread with an ordinary store, and equal inputs give equal bits on every run.
// All arithmetic is double on the f32 inputs (after the ONE f32 rounding per kind that the reference's f32 arrays apply, see the
// header).  Nothing is indexed dynamically but global memory: the per-command gains and steer points are picked under predicates and
// the six targets stay in registers (a dynamically indexed local array would live in scratch).
// A record that does not come from this kernel (a host upload) cannot make it write outside the record: heads and counts are brought
// into range before they index anything.
// Reads: pred [N][5][2], speed [N], command [N][4], active [N] (optional), records [N].  Writes: out [N][8], records of active agents.
#include "lbc_common.hpp"
#include "lbc_hip.h"
#include "lbc_kernels.hpp"
#include <math.h>
#include <stddef.h>

namespace {

constexpr int kThreads = 64, kSteps = 5, kPoints = kSteps + 1, kOut = 8;
constexpr int kStateWords = sizeof(lbc_agent_state) / 8;

struct AgentArgs {
    const float* pred; const float* speed; const float* cmd; const unsigned char* active;
    lbc_agent_state* state; double* out;
    int N, kind, speed_steps, turn_window, speed_window;
    int steer_points[4];
    float crop_f;
    double w, h, f, world_y, fixed_offset, crop, ppm, gap_dt, dt;
    double turn_pid[4][3], speed_pid[3];
    double engine_brake, brake, stop;
};

// v enters the window of the last W values kept in ring[0 .. W - 1]; -> integral and derivative over the window (0 below two values)
__device__ __forceinline__ void window_push(double* ring, int* count_p, int* head_p, int W, double v, double dt, double& integral, double& derivative)
{
    int count = *count_p, head = *head_p;
    head = (head >= 0 && head < W) ? head : 0;
    count = count < 0 ? 0 : (count > W ? W : count);
    const double before = ring[head == 0 ? W - 1 : head - 1];      // the newest value so far (meaningful when count >= 1)
    ring[head] = v;
    head = head + 1 == W ? 0 : head + 1;
    count = count < W ? count + 1 : W;
    int j = head - count;                                          // the oldest value
    j = j < 0 ? j + W : j;
    double sum = 0.0;
    for (int i = 0; i < count; ++i) {
        sum += ring[j];
        j = j + 1 == W ? 0 : j + 1;
    }
    *count_p = count;
    *head_p = head;
    integral = count >= 2 ? sum * dt : 0.0;
    derivative = count >= 2 ? (v - before) / dt : 0.0;
}

__device__ __forceinline__ double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kThreads) void agent_control_k(AgentArgs a)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.N) return;
    double* o = a.out + (size_t)i * kOut;
    if (a.active && a.active[i] == 0) {
#pragma unroll
        for (int k = 0; k < kOut - 1; ++k) o[k] = 0.0;
        o[kOut - 1] = (double)LBC_AGENT_FLAG_INACTIVE;
        return;
    }
    // ---- the command: exactly one entry 1, the others 0 ----
    const float* cm = a.cmd + (size_t)i * 4;
    int c = 0, ones = 0, zeros = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float v = cm[k];
        c = v == 1.f ? k : c;
        ones += v == 1.f ? 1 : 0;
        zeros += v == 0.f ? 1 : 0;
    }
    bool bad = !(ones == 1 && zeros == 3);
    // ---- waypoints -> targets (forward, lateral) in metres, and the target speed ----
    const float* p = a.pred + (size_t)i * kSteps * 2;
    double tx[kPoints], ty[kPoints];
    tx[0] = 0.0; ty[0] = 0.0;
    double target_speed = 0.0;
    if (a.kind == LBC_AGENT_IMAGE) {
#pragma unroll
        for (int k = 0; k < kSteps; ++k) {
            const float x = p[2 * k], y = p[2 * k + 1];
            const float x1 = x + 1.0f, y1 = y + 1.0f;
            const double px = (double)x1 * a.w / 2.0, py = (double)y1 * a.h / 2.0;
            const double xt = (px - a.w / 2.0) / a.f, yt = (py - a.h / 2.0) / a.f;
            bad = bad || !(__builtin_isfinite(x) && __builtin_isfinite(y)) || !(yt > 0.0);
            const double z = a.world_y / yt;
            tx[k + 1] = z - a.fixed_offset;
            ty[k + 1] = z * xt;
        }
        double len = 0.0;
#pragma unroll
        for (int k = 0; k < kSteps; ++k) {
            const double dx = tx[k] - tx[k + 1], dy = ty[k] - ty[k + 1];
            len += sqrt(dx * dx + dy * dy);
        }
        target_speed = len / (double)kSteps / a.gap_dt;
    } else {
        double qx[kSteps], qy[kSteps];
#pragma unroll
        for (int k = 0; k < kSteps; ++k) {
            const float x = p[2 * k], y = p[2 * k + 1];
            const float xf = (x + 1.0f) / 2.0f * a.crop_f, yf = (y + 1.0f) / 2.0f * a.crop_f;
            bad = bad || !(__builtin_isfinite(x) && __builtin_isfinite(y));
            qx[k] = (double)xf; qy[k] = (double)yf;
            tx[k + 1] = (a.crop - qy[k]) / a.ppm;
            ty[k + 1] = (qx[k] - a.crop / 2.0) / a.ppm;
        }
#pragma unroll
        for (int k = 1; k < kSteps; ++k) {
            const double dx = qx[k] - qx[k - 1], dy = qy[k] - qy[k - 1];
            const double v = sqrt(dx * dx + dy * dy) / (a.ppm * a.gap_dt) / (double)(a.speed_steps - 1);
            target_speed += k < a.speed_steps ? v : 0.0;
        }
    }
    if (bad) {
        o[0] = 0.0; o[1] = 0.0; o[2] = 1.0; o[3] = 0.0; o[4] = 0.0; o[5] = 0.0; o[6] = 0.0;
        o[7] = (double)LBC_AGENT_FLAG_BAD;
        return;
    }
    // ---- the per-command constants, picked without a dynamic index ----
    int n = 0;
    double kp = 0.0, ki = 0.0, kd = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool mine = k == c;
        n = mine ? a.steer_points[k] : n;
        kp = mine ? a.turn_pid[k][0] : kp;
        ki = mine ? a.turn_pid[k][1] : ki;
        kd = mine ? a.turn_pid[k][2] : kd;
    }
    // ---- least-squares circle through the six targets ----
    double mx = 0.0, my = 0.0;
#pragma unroll
    for (int k = 0; k < kPoints; ++k) { mx += tx[k]; my += ty[k]; }
    mx /= (double)kPoints; my /= (double)kPoints;
    double Suu = 0.0, Suv = 0.0, Svv = 0.0, Suuu = 0.0, Suvv = 0.0, Svvv = 0.0, Svuu = 0.0, sx = 0.0, sy = 0.0;
#pragma unroll
    for (int k = 0; k < kPoints; ++k) {
        const double u = tx[k] - mx, v = ty[k] - my;
        Suu += u * u; Suv += u * v; Svv += v * v;
        Suuu += u * u * u; Suvv += u * v * v; Svvv += v * v * v; Svuu += v * u * u;
        sx = k == n ? tx[k] : sx;                  // the steer point
        sy = k == n ? ty[k] : sy;
    }
    const double det = Suu * Svv - Suv * Suv;
    bool degenerate = !(fabs(det) > 1e-12 * (Suu * Svv));
    double aim_x = sx, aim_y = sy;
    if (!degenerate) {
        const double b0 = 0.5 * Suuu + 0.5 * Suvv, b1 = 0.5 * Svvv + 0.5 * Svuu;
        double cx = (b0 * Svv - b1 * Suv) / det, cy = (Suu * b1 - Suv * b0) / det;
        const double r = sqrt(cx * cx + cy * cy + (Suu + Svv) / (double)kPoints);
        cx += mx; cy += my;
        const double dx = sx - cx, dy = sy - cy, dn = sqrt(dx * dx + dy * dy);
        const double ax = cx + dx / dn * r, ay = cy + dy / dn * r;
        degenerate = !(dn > 0.0) || !(__builtin_isfinite(ax) && __builtin_isfinite(ay));
        aim_x = degenerate ? sx : ax;
        aim_y = degenerate ? sy : ay;
    }
    const double alpha = atan2(aim_y, aim_x);
    // ---- the two controllers: both windows advance on every tick that reaches this point ----
    lbc_agent_state* st = a.state + i;
    double ie, de;
    window_push(st->turn_ring, &st->turn_count, &st->turn_head, a.turn_window, alpha, a.dt, ie, de);
    double steer = kp * alpha + kd * de + ki * ie;
    const double err = target_speed - (double)a.speed[i];
    window_push(st->speed_ring, &st->speed_count, &st->speed_head, a.speed_window, err, a.dt, ie, de);
    double throttle = a.speed_pid[0] * err + a.speed_pid[1] * ie + a.speed_pid[2] * de;
    double brake = 0.0;
    if (a.kind == LBC_AGENT_IMAGE) {
        if (target_speed <= a.engine_brake) { steer = 0.0; throttle = 0.0; }
        if (target_speed <= a.brake) brake = 1.0;
    } else if (target_speed < a.stop) {
        steer = 0.0; throttle = 0.0; brake = 1.0;
    }
    o[0] = clip(steer, -1.0, 1.0);
    o[1] = clip(throttle, 0.0, 1.0);
    o[2] = clip(brake, 0.0, 1.0);
    o[3] = target_speed;
    o[4] = aim_x;
    o[5] = aim_y;
    o[6] = alpha;
    o[7] = degenerate ? (double)LBC_AGENT_FLAG_DEGENERATE : 0.0;
}

__global__ __launch_bounds__(kThreads) void agent_reset_k(const unsigned char* __restrict__ mask, int N, long long* __restrict__ state)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N || (mask && mask[i] == 0)) return;
    long long* s = state + (size_t)i * kStateWords;
    for (int k = 0; k < kStateWords; ++k) s[k] = 0;
}

bool positive(double v) { return isfinite(v) && v > 0.0; }

}  // namespace

int lbc_agent_control_launch(const lbc_agent_desc* d, const float* pred, const float* speed, const float* command_onehot,
                             const unsigned char* active, int N, void* state, double* out, hipStream_t s)
{
    static_assert(sizeof(lbc_agent_state) == 336 && sizeof(lbc_agent_state) % 8 == 0 && offsetof(lbc_agent_state, speed_ring) == 80 &&
                  offsetof(lbc_agent_state, turn_count) == 320 && offsetof(lbc_agent_state, speed_head) == 332,
                  "lbc_agent_state layout (include/lbc_hip.h)");
    LBC_REQUIRE(d, "agent_control: null descriptor");
    LBC_REQUIRE(d->struct_size == sizeof(lbc_agent_desc),
                "agent_control: lbc_agent_desc.struct_size is %u, this library (ABI %d) accepts %zu -- initialise the descriptor with "
                "LBC_AGENT_DESC_IMAGE_INIT or LBC_AGENT_DESC_BIRDVIEW_INIT", d->struct_size, LBC_HIP_ABI_VERSION, sizeof(lbc_agent_desc));
    LBC_REQUIRE(state && (reinterpret_cast<uintptr_t>(state) & 7) == 0, "agent_control: the state (%p) must be non-null and 8-byte aligned", state);
    LBC_REQUIRE(out && (reinterpret_cast<uintptr_t>(out) & 7) == 0, "agent_control: out (%p) must be non-null and 8-byte aligned", (void*)out);
    LBC_REQUIRE(pred && speed && command_onehot, "agent_control: null argument (pred %p, speed %p, command %p)", (const void*)pred,
                (const void*)speed, (const void*)command_onehot);
    LBC_REQUIRE(N >= 0, "agent_control: N = %d is negative", N);
    LBC_REQUIRE(d->kind == LBC_AGENT_IMAGE || d->kind == LBC_AGENT_BIRDVIEW, "agent_control: kind = %d, must be 0 (image) or 1 (bird-view)", d->kind);
    LBC_REQUIRE(d->n_steps == kSteps, "agent_control: n_steps = %d, the networks predict %d waypoints", d->n_steps, kSteps);
    LBC_REQUIRE(d->speed_steps >= 2 && d->speed_steps <= d->n_steps, "agent_control: speed_steps = %d outside 2..%d", d->speed_steps, d->n_steps);
    LBC_REQUIRE(d->turn_window >= 2 && d->turn_window <= LBC_AGENT_TURN_WINDOW_MAX, "agent_control: turn_window = %d outside 2..%d", d->turn_window,
                LBC_AGENT_TURN_WINDOW_MAX);
    LBC_REQUIRE(d->speed_window >= 2 && d->speed_window <= LBC_AGENT_SPEED_WINDOW_MAX, "agent_control: speed_window = %d outside 2..%d",
                d->speed_window, LBC_AGENT_SPEED_WINDOW_MAX);
    for (int k = 0; k < 4; ++k)
        LBC_REQUIRE(d->steer_points[k] >= 0 && d->steer_points[k] <= d->n_steps, "agent_control: steer_points[%d] = %d outside 0..%d", k,
                    d->steer_points[k], d->n_steps);
    LBC_REQUIRE(positive(d->gap), "agent_control: gap = %g must be a positive finite number", d->gap);
    LBC_REQUIRE(positive(d->dt), "agent_control: dt = %g must be a positive finite number", d->dt);
    LBC_REQUIRE(positive(d->fov) && d->fov < 180.0, "agent_control: fov = %g degrees must lie in (0, 180)", d->fov);
    LBC_REQUIRE(positive(d->w) && positive(d->h), "agent_control: the frame size w = %g, h = %g must be positive finite numbers", d->w, d->h);
    LBC_REQUIRE(positive(d->crop_size) && positive(d->pixels_per_meter),
                "agent_control: crop_size = %g and pixels_per_meter = %g must be positive finite numbers", d->crop_size, d->pixels_per_meter);
    bool fin = isfinite(d->world_y) && isfinite(d->fixed_offset) && isfinite(d->engine_brake_threshold) && isfinite(d->brake_threshold) &&
               isfinite(d->stop_threshold);
    for (int k = 0; k < 3; ++k) fin = fin && isfinite(d->speed_pid[k]);
    for (int k = 0; k < 12; ++k) fin = fin && isfinite(d->turn_pid[k / 3][k % 3]);
    LBC_REQUIRE(fin, "agent_control: a gain, a threshold, world_y or fixed_offset is not finite");
    if (N == 0) return LBC_OK;
    AgentArgs a;
    a.pred = pred; a.speed = speed; a.cmd = command_onehot; a.active = active;
    a.state = static_cast<lbc_agent_state*>(state); a.out = out;
    a.N = N; a.kind = d->kind; a.speed_steps = d->speed_steps; a.turn_window = d->turn_window; a.speed_window = d->speed_window;
    for (int k = 0; k < 4; ++k) {
        a.steer_points[k] = d->steer_points[k];
        for (int j = 0; j < 3; ++j) a.turn_pid[k][j] = d->turn_pid[k][j];
    }
    for (int j = 0; j < 3; ++j) a.speed_pid[j] = d->speed_pid[j];
    a.crop_f = (float)d->crop_size;
    a.w = d->w; a.h = d->h; a.world_y = d->world_y; a.fixed_offset = d->fixed_offset; a.crop = d->crop_size; a.ppm = d->pixels_per_meter;
    a.f = d->w / (2.0 * tan(d->fov * 3.14159265358979323846 / 360.0));      // the focal length, once, on the host
    a.gap_dt = d->gap * d->dt; a.dt = d->dt;
    a.engine_brake = d->engine_brake_threshold; a.brake = d->brake_threshold; a.stop = d->stop_threshold;
    // algorithmic bytes: inputs read once, the records read and written, the output rows
    LbcProfScope prof("agent_control", 0.0, (double)N * (40.0 + 4.0 + 16.0 + 2.0 * sizeof(lbc_agent_state) + 8.0 * kOut), s);
    hipLaunchKernelGGL(agent_control_k, dim3(lbc_cdiv(N, kThreads)), dim3(kThreads), 0, s, a);
    return lbc_check_launch("agent_control");
}

int lbc_agent_reset_launch(const unsigned char* mask, int N, void* state, hipStream_t s)
{
    LBC_REQUIRE(state && (reinterpret_cast<uintptr_t>(state) & 7) == 0, "agent_reset: the state (%p) must be non-null and 8-byte aligned", state);
    LBC_REQUIRE(N >= 0, "agent_reset: N = %d is negative", N);
    if (N == 0) return LBC_OK;
    hipLaunchKernelGGL(agent_reset_k, dim3(lbc_cdiv(N, kThreads)), dim3(kThreads), 0, s, mask, N, static_cast<long long*>(state));
    return lbc_check_launch("agent_reset");
}
