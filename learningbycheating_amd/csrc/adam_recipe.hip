// The training recipe on top of the clipped step for gfx950: a learning-rate schedule (linear warm-up, then constant / cosine / step),
// decoupled weight decay (AdamW) and an exponential moving average of the parameters, all inside the optimizer step and without a host
// round trip.  Three launches in stream order over the chunk table of adam_k, one caller-owned record (an lbc_adam_recipe_state header
// followed by one double per chunk) and, with the average, a device array of one float* per chunk into the shadow:
//   1. adam_norm_k         the gradient pass of adam_clip.hip itself (lbc_adam_norm_pass): same kernel, same fixed summation order, no
//                          atomics.  The record's first 64 bytes ARE an lbc_adam_clip_state; the pass writes scan_flag only.
//   2. adam_recipe_book_k  the bookkeeping of adam_clip_book_k statement for statement, except that lr is not an argument: on a clean step
//                          one thread evaluates the schedule in double at k = step - 1, the number of updates applied before this one.  The
//                          step count lives in this record and a skipped step does not advance it, so the schedule can only be evaluated
//                          here without a sync.  It also stores lr, decay_factor = (float)(1 - lr * wd) (decoupled; else 1) and counts
//                          ema_updates.  A bad step keeps all of them, as it keeps grad_norm.
//   3. adam_recipe_k<kDecoupled, kEma>  the update of adam_clipped_k through the same clipped_update<kTail> (adam_update.hpp).  kDecoupled:
//                          p is first multiplied by decay_factor as a SEPARATELY ROUNDED f32 product (never contracted into what follows;
//                          the coupled wd is then 0).  kEma: e = e + w * (p' - e), w = (float)(1 - decay), on the updated p' still in
//                          registers; e moves 16 bytes per lane like m and v (8 B/element on top of the clipped step's 32).  The grid
//                          returns before its first load on a bad step: e keeps its bits like p, m and v.
// <false, false> is adam_clipped_k's arithmetic exactly: a neutral recipe is the clipped step bit for bit.
#include "lbc_common.hpp"
#include "lbc_hip.h"
#include "lbc_kernels.hpp"
#include "adam_update.hpp"
#include <math.h>
#include <stddef.h>

namespace {

// what the bookkeeping thread needs of lbc_adam_recipe (validated on the host), passed by value
struct RecipeBook {
    double base_lr, s0, min_lr, gamma, wd, max_norm, beta1, beta2;
    long long W, T, S;
    int kind, decoupled, ema;
};

__device__ __forceinline__ double recipe_lr(const RecipeBook& r, long long k)
{
    if (k < r.W) return r.base_lr * (r.s0 + (1.0 - r.s0) * (double)k / (double)r.W);
    const long long j = k - r.W;
    if (r.kind == LBC_LR_COSINE) {
        const long long span = r.T - r.W;
        const long long jj = j < span ? j : span;
        return r.min_lr + (r.base_lr - r.min_lr) * 0.5 * (1.0 + cos(3.14159265358979323846 * (double)jj / (double)span));
    }
    if (r.kind == LBC_LR_STEP) return r.base_lr * pow(r.gamma, (double)(j / r.S));
    return r.base_lr;
}

__global__ __launch_bounds__(256) void adam_recipe_book_k(lbc_adam_recipe_state* __restrict__ st, const double* __restrict__ partial,
                                                          int nchunks, RecipeBook r)
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
    // the bookkeeping of adam_clip_book_k, statement for statement, with lr from the schedule
    const int bad = st->scan_flag != 0;
    st->scan_flag = 0;
    st->bad = bad;
    if (bad) {
        st->skipped_total += 1;
        st->skipped_in_a_row += 1;
        return;                       // grad_norm, clip_coef, clipped_total, lr, decay_factor and ema_updates keep the last clean step's values
    }
    const long long step = st->step + 1;
    st->step = step;
    st->skipped_in_a_row = 0;
    const double lr = recipe_lr(r, step - 1);
    const double bc1 = 1.0 - pow(r.beta1, (double)step);
    const double bc2 = 1.0 - pow(r.beta2, (double)step);
    st->lr_over_bc1 = (float)(lr / bc1);
    st->inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    const double norm = sqrt(red[0]);
    const double c = r.max_norm / (norm + 1e-6);
    const float coef = (r.max_norm > 0.0 && c < 1.0) ? (float)c : 1.0f;
    st->grad_norm = norm;
    st->clip_coef = coef;
    st->clipped_total += (coef < 1.0f) ? 1 : 0;
    st->lr = lr;
    st->decay_factor = r.decoupled ? (float)(1.0 - lr * r.wd) : 1.0f;
    if (r.ema) st->ema_updates += 1;
}

// p * decay_factor, rounded on its own: the bitwise contract is "the clipped step on parameters multiplied by that float"
__device__ __forceinline__ float decayed(float p, float df)
{
#pragma clang fp contract(off)
    const float q = p * df;
    return q;
}

// e + w * (p' - e).  On the device the multiply-add is one fused operation, written out; the emulated build fuses nothing
__device__ __forceinline__ float ema_step(float e, float p, float w)
{
#pragma clang fp contract(off)
    const float d = p - e;
#ifdef LBC_HIP_EMULATED_FOR_TESTS
    const float t = w * d;
    return e + t;
#else
    return __builtin_fmaf(w, d, e);
#endif
}

template <bool kDecoupled, bool kEma>
__global__ __launch_bounds__(256) void adam_recipe_k(const AdamChunk* __restrict__ chunks, float* const* __restrict__ ema,
                                                     const lbc_adam_recipe_state* __restrict__ st, float beta1, float beta2, float omb1,
                                                     float omb2, float eps, float wd, float ema_w)
{
    if (st->bad != 0) return;         // (uniform over the grid, and before the first load: a skipped step touches nothing)
    const float lr_over_bc1 = st->lr_over_bc1, inv_bc2_sqrt = st->inv_bc2_sqrt, coef = st->clip_coef;
    const float df = kDecoupled ? st->decay_factor : 1.0f;
    const AdamChunk ch = chunks[blockIdx.x];
    float* __restrict__ const ce = kEma ? ema[blockIdx.x] : nullptr;
    const int n4 = ch.n >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
        float4 p = reinterpret_cast<float4*>(ch.p)[i];
        const float4 g = reinterpret_cast<const float4*>(ch.g)[i];
        float4 m = reinterpret_cast<float4*>(ch.m)[i];
        float4 v = reinterpret_cast<float4*>(ch.v)[i];
        float4 e;
        if (kEma) e = reinterpret_cast<float4*>(ce)[i];
        if (kDecoupled) { p.x = decayed(p.x, df); p.y = decayed(p.y, df); p.z = decayed(p.z, df); p.w = decayed(p.w, df); }
        clipped_update<false>(p.x, g.x, m.x, v.x, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
        clipped_update<false>(p.y, g.y, m.y, v.y, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
        clipped_update<false>(p.z, g.z, m.z, v.z, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
        clipped_update<false>(p.w, g.w, m.w, v.w, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
        reinterpret_cast<float4*>(ch.p)[i] = p;
        reinterpret_cast<float4*>(ch.m)[i] = m;
        reinterpret_cast<float4*>(ch.v)[i] = v;
        if (kEma) {
            e.x = ema_step(e.x, p.x, ema_w); e.y = ema_step(e.y, p.y, ema_w); e.z = ema_step(e.z, p.z, ema_w); e.w = ema_step(e.w, p.w, ema_w);
            reinterpret_cast<float4*>(ce)[i] = e;
        }
    }
    for (int i = (n4 << 2) + threadIdx.x; i < ch.n; i += 256) {
        float p = ch.p[i], m = ch.m[i], v = ch.v[i];
        if (kDecoupled) p = decayed(p, df);
        clipped_update<true>(p, ch.g[i], m, v, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
        ch.p[i] = p; ch.m[i] = m; ch.v[i] = v;
        if (kEma) ce[i] = ema_step(ce[i], p, ema_w);
    }
}

}  // namespace

int lbc_adam_recipe_launch(const AdamChunk* chunks_dev, int nchunks, const lbc_adam_recipe* rc, float* const* ema_dev,
                           lbc_adam_recipe_state* state_dev, hipStream_t s)
{
    LBC_REQUIRE(rc, "adam_recipe: null recipe");
    LBC_REQUIRE(rc->struct_size == sizeof(lbc_adam_recipe),
                "adam_recipe: lbc_adam_recipe.struct_size is %u, this library (ABI %d) accepts %zu -- initialise the recipe with LBC_ADAM_RECIPE_INIT",
                rc->struct_size, LBC_HIP_ABI_VERSION, sizeof(lbc_adam_recipe));
    LBC_REQUIRE(chunks_dev && nchunks > 0, "adam_recipe: bad args (chunk table %p, nchunks %d)", (const void*)chunks_dev, nchunks);
    LBC_REQUIRE(state_dev && ((uintptr_t)state_dev & 7) == 0,
                "adam_recipe: the state record must be a device pointer aligned to 8 bytes (lbc_adam_recipe_state_bytes(nchunks) bytes)");
    LBC_REQUIRE(rc->schedule == LBC_LR_CONSTANT || rc->schedule == LBC_LR_COSINE || rc->schedule == LBC_LR_STEP,
                "adam_recipe: unknown schedule kind %d (LBC_LR_CONSTANT, LBC_LR_COSINE or LBC_LR_STEP)", rc->schedule);
    const double all[] = {rc->base_lr, rc->warmup_start, rc->min_lr, rc->gamma, rc->weight_decay, rc->max_norm, rc->ema_decay, rc->beta1, rc->beta2, rc->eps};
    static const char* const names[] = {"base_lr", "warmup_start", "min_lr", "gamma", "weight_decay", "max_norm", "ema_decay", "beta1", "beta2", "eps"};
    for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i) LBC_REQUIRE(all[i] == all[i], "adam_recipe: %s is NaN", names[i]);
    LBC_REQUIRE(rc->base_lr >= 0.0, "adam_recipe: base_lr %g is negative", rc->base_lr);
    LBC_REQUIRE(rc->warmup_steps >= 0, "adam_recipe: warmup_steps %lld is negative", rc->warmup_steps);
    LBC_REQUIRE(rc->warmup_start >= 0.0 && rc->warmup_start <= 1.0, "adam_recipe: warmup_start %g outside [0, 1]", rc->warmup_start);
    LBC_REQUIRE(rc->schedule != LBC_LR_COSINE || rc->total_steps > rc->warmup_steps,
                "adam_recipe: a cosine schedule needs total_steps (%lld) > warmup_steps (%lld)", rc->total_steps, rc->warmup_steps);
    LBC_REQUIRE(rc->schedule != LBC_LR_STEP || (rc->step_size >= 1 && rc->gamma > 0.0),
                "adam_recipe: a step schedule needs step_size >= 1 and gamma > 0 (got %lld, %g)", rc->step_size, rc->gamma);
    LBC_REQUIRE(rc->ema_decay >= 0.0 && rc->ema_decay < 1.0, "adam_recipe: ema_decay %g outside [0, 1) (0 = no average)", rc->ema_decay);
    const bool ema = rc->ema_decay > 0.0, decoupled = rc->decoupled != 0;
    LBC_REQUIRE(!ema || ema_dev, "adam_recipe: ema_decay > 0 needs the table of shadow pointers (ema_dev is null)");
    LBC_REQUIRE(!decoupled || rc->weight_decay >= 0.0, "adam_recipe: decoupled weight decay %g is negative", rc->weight_decay);
    RecipeBook b;
    b.base_lr = rc->base_lr; b.s0 = rc->warmup_start; b.min_lr = rc->min_lr; b.gamma = rc->gamma; b.wd = rc->weight_decay;
    b.max_norm = rc->max_norm; b.beta1 = rc->beta1; b.beta2 = rc->beta2;
    b.W = rc->warmup_steps; b.T = rc->total_steps; b.S = rc->step_size;
    b.kind = rc->schedule; b.decoupled = decoupled; b.ema = ema;
    lbc_adam_clip_state* head = reinterpret_cast<lbc_adam_clip_state*>(state_dev);       // (the record starts with its 64 bytes)
    double* partial = reinterpret_cast<double*>(state_dev + 1);                          // (the header is a multiple of 8 bytes)
    // algorithmic bytes: the clipped step's 32 per element; the average reads and writes e on top
    LbcProfScope prof("adam_recipe", 0.0, (ema ? 40.0 : 32.0) * (double)lbc_adam_profile_elems_get(), s);
    lbc_adam_norm_pass(chunks_dev, nchunks, head, partial, s);
    hipLaunchKernelGGL(adam_recipe_book_k, dim3(1), dim3(256), 0, s, state_dev, (const double*)partial, nchunks, b);
    const float beta1 = (float)rc->beta1, beta2 = (float)rc->beta2, omb1 = (float)(1.0 - rc->beta1), omb2 = (float)(1.0 - rc->beta2);
    const float eps = (float)rc->eps, wd = decoupled ? 0.0f : (float)rc->weight_decay, w = (float)(1.0 - rc->ema_decay);
    const dim3 grid((unsigned)nchunks), block(256);
    const lbc_adam_recipe_state* cst = state_dev;
#define LBC_RECIPE(D, E) hipLaunchKernelGGL((adam_recipe_k<D, E>), grid, block, 0, s, chunks_dev, ema_dev, cst, beta1, beta2, omb1, omb2, eps, wd, w)
    if (decoupled) { if (ema) LBC_RECIPE(true, true); else LBC_RECIPE(true, false); }
    else           { if (ema) LBC_RECIPE(false, true); else LBC_RECIPE(false, false); }
#undef LBC_RECIPE
    return lbc_check_launch("adam_recipe");
}
