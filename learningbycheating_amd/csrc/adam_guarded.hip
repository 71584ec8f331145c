// Guarded multi-tensor Adam for gfx950: the step of adam.hip behind a non-finite scan of the gradients, with every decision
// taken on the device (no device-to-host copy, no stream synchronisation).  Three launches in stream order over the chunk table of
// adam_k and one lbc_adam_state record in HBM:
//   1. adam_scan_k   reads every gradient element once (4 B/element, 16-byte loads) and raises state->scan_flag when one has an
//                    all-ones exponent (NaN, +Inf, -Inf).  One plain store of 1 per workgroup that found something: every writer
//                    stores the same value, so the stores need no ordering among themselves.
//   2. adam_book_k   one thread: bad = scan_flag, scan_flag = 0 (ready for the next step, the host never clears it);
//                    clean  -> step += 1, skipped_in_a_row = 0, bias-correction coefficients of the new step in double
//                              (the formula of lbc_adam_launch), stored as floats;
//                    bad    -> skipped_total += 1, skipped_in_a_row += 1 (step and coefficients stay).
//   3. adam_guarded_k  the arithmetic of adam_k, statement for statement, coefficients read from the record; the whole grid
//                    returns before its first load when bad != 0, so p, m and v keep their bits.
// Kernel boundaries order the three: a launch on a stream sees every store of the launches before it.
#include "lbc_common.hpp"
#include "lbc_hip.h"
#include "lbc_kernels.hpp"

namespace {

constexpr unsigned kExpMask = 0x7f800000u;     // f32 exponent field: all ones = NaN or +-Inf

// largest |x| bit pattern seen: a non-finite element is one whose pattern with the sign removed is >= kExpMask
__device__ __forceinline__ unsigned absbits_max(unsigned acc, uint4 q)
{
    const unsigned a = q.x & 0x7fffffffu, b = q.y & 0x7fffffffu, c = q.z & 0x7fffffffu, d = q.w & 0x7fffffffu;
    const unsigned ab = a > b ? a : b, cd = c > d ? c : d, m = ab > cd ? ab : cd;
    return acc > m ? acc : m;
}

__global__ __launch_bounds__(256) void adam_scan_k(const AdamChunk* __restrict__ chunks, lbc_adam_state* __restrict__ st)
{
    __shared__ unsigned wave_acc[4];
    const AdamChunk ch = chunks[blockIdx.x];
    const uint4* __restrict__ g4 = reinterpret_cast<const uint4*>(ch.g);
    const int n4 = ch.n >> 2;
    unsigned acc = 0;
    int i = threadIdx.x;
    // four independent 16-byte loads in flight per lane (a full chunk of 32768 elements is eight such rounds)
    for (; i + 768 < n4; i += 1024) {
        const uint4 q0 = g4[i], q1 = g4[i + 256], q2 = g4[i + 512], q3 = g4[i + 768];
        acc = absbits_max(absbits_max(absbits_max(absbits_max(acc, q0), q1), q2), q3);
    }
    for (; i < n4; i += 256) acc = absbits_max(acc, g4[i]);
    const unsigned* __restrict__ g1 = reinterpret_cast<const unsigned*>(ch.g);
    for (int j = (n4 << 2) + threadIdx.x; j < ch.n; j += 256) {
        const unsigned a = g1[j] & 0x7fffffffu;
        acc = acc > a ? acc : a;
    }
    // wave-level OR of "found one" (as a max of the patterns), then one store per workgroup
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = __shfl_xor(acc, off);
        acc = acc > o ? acc : o;
    }
    if ((threadIdx.x & 63) == 0) wave_acc[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned a = wave_acc[0] > wave_acc[1] ? wave_acc[0] : wave_acc[1];
        const unsigned b = wave_acc[2] > wave_acc[3] ? wave_acc[2] : wave_acc[3];
        if ((a > b ? a : b) >= kExpMask) st->scan_flag = 1;
    }
}

__global__ __launch_bounds__(64) void adam_book_k(lbc_adam_state* __restrict__ st, double lr, double beta1, double beta2)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int bad = st->scan_flag != 0;
    st->scan_flag = 0;
    st->bad = bad;
    if (bad) {
        st->skipped_total += 1;
        st->skipped_in_a_row += 1;
        return;
    }
    const long long step = st->step + 1;
    st->step = step;
    st->skipped_in_a_row = 0;
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    st->lr_over_bc1 = (float)(lr / bc1);
    st->inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
}

__global__ __launch_bounds__(256) void adam_guarded_k(const AdamChunk* __restrict__ chunks, const lbc_adam_state* __restrict__ st,
                                                      float beta1, float beta2, float omb1, float omb2, float eps, float wd)
{
    if (st->bad != 0) return;         // (uniform over the grid: the record is not written between the bookkeeping launch and the next scan)
    const float lr_over_bc1 = st->lr_over_bc1, inv_bc2_sqrt = st->inv_bc2_sqrt;
    const AdamChunk ch = chunks[blockIdx.x];
    const int n4 = ch.n >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
        float4 p = reinterpret_cast<float4*>(ch.p)[i];
        float4 g = reinterpret_cast<const float4*>(ch.g)[i];
        float4 m = reinterpret_cast<float4*>(ch.m)[i];
        float4 v = reinterpret_cast<float4*>(ch.v)[i];
#define LBC_ADAM1(c)                                                   \
        {                                                              \
            float gg = g.c + wd * p.c;                                 \
            m.c = m.c + (gg - m.c) * omb1;                    \
            v.c = beta2 * v.c + omb2 * gg * gg;               \
            const float denom = sqrtf(v.c) * inv_bc2_sqrt + eps;       \
            p.c = p.c - lr_over_bc1 * (m.c / denom);                   \
        }
        LBC_ADAM1(x) LBC_ADAM1(y) LBC_ADAM1(z) LBC_ADAM1(w)
#undef LBC_ADAM1
        reinterpret_cast<float4*>(ch.p)[i] = p;
        reinterpret_cast<float4*>(ch.m)[i] = m;
        reinterpret_cast<float4*>(ch.v)[i] = v;
    }
    for (int i = (n4 << 2) + threadIdx.x; i < ch.n; i += 256) {
        float p = ch.p[i], m = ch.m[i], v = ch.v[i];
        const float gg = ch.g[i] + wd * p;
        m = m + (gg - m) * omb1;
        v = beta2 * v + omb2 * gg * gg;
        const float denom = sqrtf(v) * inv_bc2_sqrt + eps;
        p = p - lr_over_bc1 * (m / denom);
        ch.p[i] = p; ch.m[i] = m; ch.v[i] = v;
    }
}

}  // namespace

int lbc_adam_guarded_launch(const AdamChunk* chunks_dev, int nchunks, double lr, double beta1, double beta2, double eps,
                            double weight_decay, lbc_adam_state* state_dev, hipStream_t s)
{
    LBC_REQUIRE(chunks_dev && nchunks > 0, "adam_guarded: bad args");
    LBC_REQUIRE(state_dev && ((uintptr_t)state_dev & 7) == 0, "adam_guarded: the state record must be a device pointer aligned to 8 bytes");
    // algorithmic bytes: the scan reads g once (4 B/element) on top of Adam's 28 (a skipped step moves the 4 only; the class books the clean step)
    LbcProfScope prof("adam_guarded", 0.0, 32.0 * (double)lbc_adam_profile_elems_get(), s);
    hipLaunchKernelGGL(adam_scan_k, dim3((unsigned)nchunks), dim3(256), 0, s, chunks_dev, state_dev);
    hipLaunchKernelGGL(adam_book_k, dim3(1), dim3(64), 0, s, state_dev, lr, beta1, beta2);
    hipLaunchKernelGGL(adam_guarded_k, dim3((unsigned)nchunks), dim3(256), 0, s, chunks_dev, (const lbc_adam_state*)state_dev, (float)beta1,
                       (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)weight_decay);
    return lbc_check_launch("adam_guarded");
}
