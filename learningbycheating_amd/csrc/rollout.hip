// The on-policy tick of phase 2 (DAgger; reference training/train_image_phase2.py:61-149 rollout / get_control): after both networks and
// both controllers have run for N agents, two launches decide who drives and record what the agents saw, with nothing read back.
//   decide  ONE workgroup, one thread per agent (N <= 1024).  u = hash3(seed ^ tick_hi, tick_lo, agent) / 2^32 in double; the applied
//           control is the student's iff u < *p_student (get_control, :45-58), otherwise the teacher's.  An active agent whose cursor is
//           below `capacity` takes slot agent * capacity + cursor: the slot's cmd (1..4), speed and weight are written and the cursor
//           advances; at capacity the slot is -1 and dropped[agent] advances (the reference stops appending at episode_length, :137).
//           An inactive agent gets slot -1, an all-zero row, and keeps its cursor.  Every thread reads the tick counter, a barrier
//           follows, then thread 0 advances it: the counter and the cursors belong to this one workgroup.  Double arithmetic, no atomics;
//           every word is written by exactly one thread.
//   stage   the copy: camera row and bird-view row of every agent with slot >= 0 go to row slot of the two staging arrays, both kinds in
//           one launch, 16 bytes per lane.  An agent's two rows are addressed as ONE run of words (camera first); workgroup (x, y) moves
//           the spans x, x + gridDim.x, ... of 256 * U words of the agents y, y + gridDim.y, ...  It reads `slot` only -- never a cursor
//           or the tick counter, which a late workgroup could see advanced.  A slot outside [0, stage_rows) moves nothing.
#include "lbc_common.hpp"
#include "lbc_hash.hpp"
#include "lbc_kernels.hpp"

namespace {

constexpr int kDecideMax = 1024, kOutCols = 16, kCtlCols = 8;
constexpr unsigned kStageGridX = 2048, kStageGridY = 65535;

struct DecideArgs {
    const double* student; const double* teacher; const float* weight; const float* speed; const float* cmd; const unsigned char* active;
    const double* p_student; unsigned long long* tick; int* cursor; int* dropped;
    int* slot; int* slot_cmd; float* slot_speed; float* slot_weight; double* out;
    int N, capacity; unsigned seed;
};

__global__ __launch_bounds__(kDecideMax) void rollout_decide_k(DecideArgs a)
{
    const int i = (int)threadIdx.x;
    const unsigned long long tick = *a.tick;             // (every thread reads it before thread 0 advances it)
    const double p = *a.p_student;
    __syncthreads();
    if (i == 0) *a.tick = tick + 1ULL;
    if (i >= a.N) return;
    double* o = a.out + (size_t)i * kOutCols;
    if (a.active && a.active[i] == 0) {
#pragma unroll
        for (int k = 0; k < kOutCols; ++k) o[k] = 0.0;
        a.slot[i] = -1;
        return;
    }
    const double* s = a.student + (size_t)i * kCtlCols;
    const double* t = a.teacher + (size_t)i * kCtlCols;
    const double u = (double)hash3(a.seed ^ (unsigned)(tick >> 32), (unsigned)tick, (unsigned)i) * (1.0 / 4294967296.0);
    const bool who = u < p;
    const float w = a.weight[i];
    const int cur = a.cursor[i];
    const bool room = cur >= 0 && cur < a.capacity;
    int staged = cur;
    if (room) {
        const float* cm = a.cmd + (size_t)i * 4;
        int c = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) c = cm[k] == 1.f ? k : c;
        const int at = i * a.capacity + cur;
        a.slot_cmd[at] = c + 1;
        a.slot_speed[at] = a.speed[i];
        a.slot_weight[at] = w;
        a.slot[i] = at;
        staged = cur + 1;
        a.cursor[i] = staged;
    } else {
        a.slot[i] = -1;
        a.dropped[i] = a.dropped[i] + 1;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = who ? s[k] : t[k];
        o[8 + k] = s[k];
        o[11 + k] = t[k];
    }
    o[3] = who ? 1.0 : 0.0;
    o[4] = (double)w;
    o[5] = (double)staged;
    o[6] = s[kCtlCols - 1];
    o[7] = t[kCtlCols - 1];
    o[14] = room ? 0.0 : 1.0;
    o[15] = 0.0;
}

// words [0, rc) of an agent's run are its camera row, words [rc, rc + bc) its bird-view row
template <int U>
__global__ __launch_bounds__(256) void rollout_stage_k(const uint4* __restrict__ rgb, const uint4* __restrict__ bv, const int* __restrict__ slot, int N,
                                                       long long stage_rows, long long rc, long long bc, uint4* __restrict__ rgb_stage,
                                                       uint4* __restrict__ bv_stage)
{
    const long long words = rc + bc, span = 256LL * U;
    for (long long a = blockIdx.y; a < N; a += gridDim.y) {
        const long long s = (long long)slot[a];
        if (s < 0 || s >= stage_rows) continue;
        const uint4* src_r = rgb + a * rc;
        const uint4* src_b = bv + a * bc;
        uint4* dst_r = rgb_stage + s * rc;
        uint4* dst_b = bv_stage + s * bc;
        for (long long w0 = (long long)blockIdx.x * span; w0 < words; w0 += (long long)gridDim.x * span) {
            const long long c0 = w0 + threadIdx.x;
            if (w0 + span <= words) {                    // a whole span: U loads in flight, then U stores
                uint4 v[U];
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    const long long c = c0 + k * 256;
                    v[k] = c < rc ? src_r[c] : src_b[c - rc];
                }
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    const long long c = c0 + k * 256;
                    if (c < rc) dst_r[c] = v[k]; else dst_b[c - rc] = v[k];
                }
            } else {                                     // the run's last span
                for (long long c = c0; c < words; c += 256) {
                    if (c < rc) dst_r[c] = src_r[c]; else dst_b[c - rc] = src_b[c - rc];
                }
            }
        }
    }
}

bool aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

}  // namespace

int lbc_rollout_decide_launch(const double* student, const double* teacher, const float* weight, const float* speed, const float* command_onehot,
                              const unsigned char* active, int N, int capacity, unsigned seed, const double* p_student, unsigned long long* tick,
                              int* cursor, int* dropped, int* slot, int* slot_cmd, float* slot_speed, float* slot_weight, double* out, hipStream_t s)
{
    LBC_REQUIRE(student && teacher && weight && speed && command_onehot, "rollout_decide: null input (student %p, teacher %p, weight %p, speed %p, command %p)",
                (const void*)student, (const void*)teacher, (const void*)weight, (const void*)speed, (const void*)command_onehot);
    LBC_REQUIRE(p_student && tick && cursor && dropped, "rollout_decide: null state (p_student %p, tick %p, cursor %p, dropped %p)", (const void*)p_student,
                (void*)tick, (void*)cursor, (void*)dropped);
    LBC_REQUIRE(slot && slot_cmd && slot_speed && slot_weight && out, "rollout_decide: null output (slot %p, slot_cmd %p, slot_speed %p, slot_weight %p, out %p)",
                (void*)slot, (void*)slot_cmd, (void*)slot_speed, (void*)slot_weight, (void*)out);
    LBC_REQUIRE(N >= 1 && N <= kDecideMax, "rollout_decide: N = %d outside [1, %d] (one workgroup owns the cursors and the tick counter)", N, kDecideMax);
    LBC_REQUIRE(capacity >= 1 && (long long)N * capacity <= 0x7fffffffLL, "rollout_decide: capacity = %d, need at least 1 and N * capacity below 2^31", capacity);
    LBC_REQUIRE(aligned(student, 8) && aligned(teacher, 8) && aligned(out, 8) && aligned(p_student, 8) && aligned(tick, 8),
                "rollout_decide: student, teacher, out, p_student and tick must be 8-byte aligned");
    DecideArgs a{student, teacher, weight, speed, command_onehot, active, p_student, tick, cursor, dropped, slot, slot_cmd, slot_speed, slot_weight, out,
                 N, capacity, seed};
    LbcProfScope prof("rollout_decide", 0.0, (double)N * (2.0 * 8 * kCtlCols + 8.0 * kOutCols + 48.0), s);
    hipLaunchKernelGGL(rollout_decide_k, dim3(1), dim3((unsigned)(lbc_cdiv(N, 64) * 64)), 0, s, a);
    return lbc_check_launch("rollout_decide");
}

int lbc_rollout_stage_launch(const unsigned char* rgb, long long rgb_row_bytes, const unsigned char* birdview, long long birdview_row_bytes, const int* slot, int N,
                             long long stage_rows, unsigned char* rgb_stage, unsigned char* birdview_stage, hipStream_t s)
{
    LBC_REQUIRE(rgb && birdview && slot && rgb_stage && birdview_stage, "rollout_stage_u8: null argument");
    LBC_REQUIRE(N >= 1 && N <= kDecideMax, "rollout_stage_u8: N = %d outside [1, %d]", N, kDecideMax);
    LBC_REQUIRE(stage_rows >= 1 && stage_rows <= 0x7fffffffLL, "rollout_stage_u8: stage_rows = %lld, need at least one staging row (N * capacity) and fewer than 2^31", stage_rows);
    LBC_REQUIRE(rgb_row_bytes > 0 && rgb_row_bytes % 16 == 0 && birdview_row_bytes > 0 && birdview_row_bytes % 16 == 0,
                "rollout_stage_u8: row_bytes = %lld / %lld must be positive multiples of 16 (rows move as 16-byte words)", rgb_row_bytes, birdview_row_bytes);
    LBC_REQUIRE(aligned(rgb, 16) && aligned(birdview, 16) && aligned(rgb_stage, 16) && aligned(birdview_stage, 16),
                "rollout_stage_u8: the frames and the staging arrays must be 16-byte aligned");
    const long long rc = rgb_row_bytes / 16, bc = birdview_row_bytes / 16, words = rc + bc;
    // 16 KB per workgroup once that still yields a thousand workgroups, 4 KB below (16 agents: 1,728 workgroups instead of 432)
    const bool wide = (long long)N * words >= 1024LL * 1024;
    const long long span = wide ? 1024 : 256, spans = (words + span - 1) / span;
    const dim3 grid((unsigned)(spans < kStageGridX ? spans : kStageGridX), (unsigned)(N < (int)kStageGridY ? N : (int)kStageGridY));
    LbcProfScope prof("rollout_stage_u8", 0.0, 2.0 * N * (double)(rgb_row_bytes + birdview_row_bytes), s);
    const uint4* r4 = reinterpret_cast<const uint4*>(rgb);
    const uint4* b4 = reinterpret_cast<const uint4*>(birdview);
    uint4* rs4 = reinterpret_cast<uint4*>(rgb_stage);
    uint4* bs4 = reinterpret_cast<uint4*>(birdview_stage);
    if (wide)
        hipLaunchKernelGGL((rollout_stage_k<4>), grid, dim3(256), 0, s, r4, b4, slot, N, stage_rows, rc, bc, rs4, bs4);
    else
        hipLaunchKernelGGL((rollout_stage_k<1>), grid, dim3(256), 0, s, r4, b4, slot, N, stage_rows, rc, bc, rs4, bs4);
    return lbc_check_launch("rollout_stage_u8");
}
