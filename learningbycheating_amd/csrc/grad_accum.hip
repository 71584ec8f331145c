// Gradient accumulation over micro-batches for gfx950: acc[i] = first ? g[i] : acc[i] + g[i], i < n, over a range of the executor's
// flat gradient buffer (one backward stage's bucket) and the same range of the trainer's accumulation buffer.
// One launch, HBM-bound: 16-byte loads and stores, a grid-stride loop over the n / 4 whole vectors (the grid of the other elementwise
// passes: 256 threads, at most 4096 workgroups) and a scalar tail of n % 4 elements on the first lanes of workgroup 0.
// FIRST is a template argument: the kernel of a window's first micro-batch has no load of acc in it at all, so whatever a skipped or
// abandoned window left there (a NaN included) cannot reach the sum.  Every element is one f32 add of two loaded values, by exactly one
// thread: no atomics, nothing to reassociate or fuse -- the same inputs give the same bits on every run and every rank.
#include "lbc_common.hpp"
#include "lbc_hip.h"
#include "lbc_kernels.hpp"

namespace {

template <bool FIRST>
__global__ __launch_bounds__(256) void grad_accum_k(const float* __restrict__ g, float* __restrict__ acc, long long n)
{
    const long long n4 = n >> 2;
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    float4* __restrict__ a4 = reinterpret_cast<float4*>(acc);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 v = g4[i];
        if (!FIRST) {
            const float4 a = a4[i];
            v.x = a.x + v.x; v.y = a.y + v.y; v.z = a.z + v.z; v.w = a.w + v.w;
        }
        a4[i] = v;
    }
    if (blockIdx.x == 0) {
        const long long j = (n4 << 2) + threadIdx.x;
        if (j < n) acc[j] = FIRST ? g[j] : acc[j] + g[j];
    }
}

}  // namespace

int lbc_grad_accumulate_launch(const float* g, float* acc, long long n, int first, hipStream_t s)
{
    LBC_REQUIRE(n >= 0, "grad_accumulate: n = %lld is negative", n);
    LBC_REQUIRE(g && acc, "grad_accumulate: null argument (g %p, acc %p)", (const void*)g, (const void*)acc);
    LBC_REQUIRE((reinterpret_cast<uintptr_t>(g) & 15) == 0 && (reinterpret_cast<uintptr_t>(acc) & 15) == 0,
                "grad_accumulate: g and acc must be 16-byte aligned (elements move as 16-byte words)");
    if (n == 0) return LBC_OK;
    // algorithmic bytes: read g, read acc, write acc (the first micro-batch of a window does not read acc)
    LbcProfScope prof("grad_accumulate", first ? 0.0 : (double)n, (first ? 8.0 : 12.0) * (double)n, s);
    long long blocks = ((n >> 2) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    if (first) hipLaunchKernelGGL((grad_accum_k<true>), dim3((unsigned)blocks), dim3(256), 0, s, g, acc, n);
    else       hipLaunchKernelGGL((grad_accum_k<false>), dim3((unsigned)blocks), dim3(256), 0, s, g, acc, n);
    return lbc_check_launch("grad_accumulate");
}
