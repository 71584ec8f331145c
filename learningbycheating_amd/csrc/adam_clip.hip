// Guarded multi-tensor Adam with global-norm gradient clipping for gfx950: the step of adam_guarded.hip whose gradient pass also
// sums the squares, so that the global L2 norm of the gradients, the clipping coefficient of torch.nn.utils.clip_grad_norm_ and
// the decision to skip a non-finite step are all taken on the device (no device-to-host copy, no stream synchronisation).
// Three launches in stream order over the chunk table of adam_k and one caller-owned device buffer: an lbc_adam_clip_state
// header followed by one double per chunk.
//   1. adam_norm_k      one workgroup per chunk reads its n gradient elements once (4 B/element, 16-byte loads, the access
//                       pattern of adam_scan_k).  Per lane: the largest |x| bit pattern (the non-finite test) and the sum of
//                       (double)x * (double)x -- the product of two f32 is exact in f64.  Lanes, then waves, are combined in a
//                       fixed order; one thread stores the chunk's partial and, for a non-finite chunk, a plain 1 to scan_flag.
//                       No atomics: the norm must not depend on the order in which workgroups arrive.
//   2. adam_clip_book_k one workgroup adds the partials in a fixed order in double; one thread then does the bookkeeping of
//                       adam_book_k and, on a clean step, stores grad_norm = sqrt(sum), clip_coef and clipped_total.  A bad
//                       step keeps all three (its partials are NaN / Inf and are overwritten by the next call's first launch).
//   3. adam_clipped_k   adam_guarded_k with every gradient element first multiplied by clip_coef as a SEPARATELY ROUNDED f32
//                       product (never contracted into the weight-decay fma), and every rounding behind it pinned to the one
//                       adam_guarded_k compiles to: with clip_coef == 1 the step is bit for bit the guarded step, with
//                       clip_coef < 1 the guarded step on gradients scaled by that float.  g is not written.
// Kernel boundaries order the three: a launch on a stream sees every store of the launches before it.
#include "lbc_common.hpp"
#include "lbc_hip.h"
#include "lbc_kernels.hpp"
#include "adam_update.hpp"      // clipped_update<kTail>: one element of the update, shared with adam_recipe.hip

namespace {

constexpr unsigned kExpMask = 0x7f800000u;     // f32 exponent field: all ones = NaN or +-Inf

// one 16-byte load's worth: largest |x| bit pattern and the exact squares, added in element order
__device__ __forceinline__ void norm_acc4(unsigned& bits, double& sq, uint4 q)
{
    const unsigned a = q.x & 0x7fffffffu, b = q.y & 0x7fffffffu, c = q.z & 0x7fffffffu, d = q.w & 0x7fffffffu;
    const unsigned ab = a > b ? a : b, cd = c > d ? c : d, m = ab > cd ? ab : cd;
    bits = bits > m ? bits : m;
    const double x = (double)__builtin_bit_cast(float, q.x), y = (double)__builtin_bit_cast(float, q.y);
    const double z = (double)__builtin_bit_cast(float, q.z), w = (double)__builtin_bit_cast(float, q.w);
    sq += x * x;
    sq += y * y;
    sq += z * z;
    sq += w * w;
}

__global__ __launch_bounds__(256) void adam_norm_k(const AdamChunk* __restrict__ chunks, lbc_adam_clip_state* __restrict__ st,
                                                   double* __restrict__ partial)
{
    __shared__ unsigned wave_bits[4];
    __shared__ double wave_sq[4];
    const AdamChunk ch = chunks[blockIdx.x];
    const uint4* __restrict__ g4 = reinterpret_cast<const uint4*>(ch.g);
    const int n4 = ch.n >> 2;
    unsigned bits = 0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;      // one accumulator per load in flight: four independent f64 chains
    int i = threadIdx.x;
    // four independent 16-byte loads in flight per lane (a full chunk of 32768 elements is eight such rounds)
    for (; i + 768 < n4; i += 1024) {
        const uint4 q0 = g4[i], q1 = g4[i + 256], q2 = g4[i + 512], q3 = g4[i + 768];
        norm_acc4(bits, s0, q0);
        norm_acc4(bits, s1, q1);
        norm_acc4(bits, s2, q2);
        norm_acc4(bits, s3, q3);
    }
    for (; i < n4; i += 256) norm_acc4(bits, s0, g4[i]);
    const unsigned* __restrict__ g1 = reinterpret_cast<const unsigned*>(ch.g);
    for (int j = (n4 << 2) + threadIdx.x; j < ch.n; j += 256) {
        const unsigned u = g1[j];
        const unsigned a = u & 0x7fffffffu;
        bits = bits > a ? bits : a;
        const double x = (double)__builtin_bit_cast(float, u);
        s0 += x * x;
    }
    double sq = (s0 + s1) + (s2 + s3);
    // lanes in a fixed order: the xor butterfly adds the same two values on both partners (a + b == b + a bit for bit), so every
    // lane of the wave ends with the same sum, whatever the hardware does around it
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = __shfl_xor(bits, off);
        bits = bits > o ? bits : o;
        sq += __shfl_xor(sq, off);
    }
    if ((threadIdx.x & 63) == 0) {
        wave_bits[threadIdx.x >> 6] = bits;
        wave_sq[threadIdx.x >> 6] = sq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned a = wave_bits[0] > wave_bits[1] ? wave_bits[0] : wave_bits[1];
        const unsigned b = wave_bits[2] > wave_bits[3] ? wave_bits[2] : wave_bits[3];
        partial[blockIdx.x] = (wave_sq[0] + wave_sq[1]) + (wave_sq[2] + wave_sq[3]);
        if ((a > b ? a : b) >= kExpMask) st->scan_flag = 1;
    }
}

__global__ __launch_bounds__(256) void adam_clip_book_k(lbc_adam_clip_state* __restrict__ st, const double* __restrict__ partial,
                                                        int nchunks, double lr, double beta1, double beta2, double max_norm)
{
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nchunks; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    // the bookkeeping of adam_book_k, statement for statement
    const int bad = st->scan_flag != 0;
    st->scan_flag = 0;
    st->bad = bad;
    if (bad) {
        st->skipped_total += 1;
        st->skipped_in_a_row += 1;
        return;                       // grad_norm, clip_coef and clipped_total keep the last clean step's values
    }
    const long long step = st->step + 1;
    st->step = step;
    st->skipped_in_a_row = 0;
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    st->lr_over_bc1 = (float)(lr / bc1);
    st->inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    // torch.nn.utils.clip_grad_norm_: coef = max_norm / (norm + 1e-6), clamped to 1 -- with the norm kept in double
    const double norm = sqrt(red[0]);
    const double c = max_norm / (norm + 1e-6);
    const float coef = (max_norm > 0.0 && c < 1.0) ? (float)c : 1.0f;
    st->grad_norm = norm;
    st->clip_coef = coef;
    st->clipped_total += (coef < 1.0f) ? 1 : 0;
}

__global__ __launch_bounds__(256) void adam_clipped_k(const AdamChunk* __restrict__ chunks, const lbc_adam_clip_state* __restrict__ st,
                                                      float beta1, float beta2, float omb1, float omb2, float eps, float wd)
{
    if (st->bad != 0) return;         // (uniform over the grid: the record is not written between the bookkeeping launch and the next norm pass)
    const float lr_over_bc1 = st->lr_over_bc1, inv_bc2_sqrt = st->inv_bc2_sqrt, coef = st->clip_coef;
    const AdamChunk ch = chunks[blockIdx.x];
    const int n4 = ch.n >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
        float4 p = reinterpret_cast<float4*>(ch.p)[i];
        const float4 g = reinterpret_cast<const float4*>(ch.g)[i];
        float4 m = reinterpret_cast<float4*>(ch.m)[i];
        float4 v = reinterpret_cast<float4*>(ch.v)[i];
        clipped_update<false>(p.x, g.x, m.x, v.x, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
        clipped_update<false>(p.y, g.y, m.y, v.y, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
        clipped_update<false>(p.z, g.z, m.z, v.z, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
        clipped_update<false>(p.w, g.w, m.w, v.w, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
        reinterpret_cast<float4*>(ch.p)[i] = p;
        reinterpret_cast<float4*>(ch.m)[i] = m;
        reinterpret_cast<float4*>(ch.v)[i] = v;
    }
    for (int i = (n4 << 2) + threadIdx.x; i < ch.n; i += 256) {
        float p = ch.p[i], m = ch.m[i], v = ch.v[i];
        clipped_update<true>(p, ch.g[i], m, v, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
        ch.p[i] = p; ch.m[i] = m; ch.v[i] = v;
    }
}

}  // namespace

int lbc_adam_clipped_launch(const AdamChunk* chunks_dev, int nchunks, double lr, double beta1, double beta2, double eps,
                            double weight_decay, double max_norm, lbc_adam_clip_state* state_dev, hipStream_t s)
{
    LBC_REQUIRE(chunks_dev && nchunks > 0, "adam_clipped: bad args (chunk table %p, nchunks %d)", (const void*)chunks_dev, nchunks);
    LBC_REQUIRE(state_dev && ((uintptr_t)state_dev & 7) == 0,
                "adam_clipped: the state record must be a device pointer aligned to 8 bytes (lbc_adam_clip_state_bytes(nchunks) bytes)");
    LBC_REQUIRE(max_norm == max_norm, "adam_clipped: max_norm is NaN (<= 0 measures without clipping)");
    double* partial = reinterpret_cast<double*>(state_dev + 1);      // (the header is a multiple of 8 bytes)
    // algorithmic bytes: the norm pass reads g once (4 B/element) on top of Adam's 28, exactly what the guarded step moves
    LbcProfScope prof("adam_clipped", 0.0, 32.0 * (double)lbc_adam_profile_elems_get(), s);
    hipLaunchKernelGGL(adam_norm_k, dim3((unsigned)nchunks), dim3(256), 0, s, chunks_dev, state_dev, partial);
    hipLaunchKernelGGL(adam_clip_book_k, dim3(1), dim3(256), 0, s, state_dev, (const double*)partial, nchunks, lr, beta1, beta2, max_norm);
    hipLaunchKernelGGL(adam_clipped_k, dim3((unsigned)nchunks), dim3(256), 0, s, chunks_dev, (const lbc_adam_clip_state*)state_dev,
                       (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)weight_decay);
    return lbc_check_launch("adam_clipped");
}

// the norm pass alone, for adam_recipe.hip: its record starts with the 64 bytes of lbc_adam_clip_state (the pass writes scan_flag only)
void lbc_adam_norm_pass(const AdamChunk* chunks_dev, int nchunks, lbc_adam_clip_state* state_dev, double* partial, hipStream_t s)
{
    hipLaunchKernelGGL(adam_norm_k, dim3((unsigned)nchunks), dim3(256), 0, s, chunks_dev, state_dev, partial);
}
