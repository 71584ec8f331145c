// Multi-tensor Adam for gfx950, every step of include/lbc_hip.h in one place.  ONE update launch covers every parameter tensor of the
// model (136 tensors / 23.1 M elements for the ResNet-34 student): one workgroup per chunk of the table, 256 threads, 16 bytes per lane,
// reading p, g, m, v and writing p, m, v exactly once (28 B/element: HBM roofline).
// Semantics = torch.optim.Adam(lr, betas, eps, weight_decay, amsgrad=False) as called at reference training/train_image_phase1.py:252
// (container torch 2.10 formulation):
//   m = m + (g - m)*(1-b1);  v = b2*v + (1-b2)*g*g
//   p -= (lr / (1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// Four levels, each the one before it plus something, all through the same element update (adam_update<kTail>):
//   plain    lbc_adam_launch          one launch; the host counts the steps and passes the two bias-correction coefficients.
//   guarded  lbc_adam_guarded_launch  the step behind a non-finite scan of the gradients, every decision taken on the device (no
//                                     device-to-host copy, no stream synchronisation).  Three launches in stream order over the chunk
//                                     table and one lbc_adam_state record in HBM:
//              1. adam_grad_pass_k<false>  reads every gradient element once (4 B/element, 16-byte loads) and raises scan_flag when one
//                                     has an all-ones exponent (NaN, +Inf, -Inf).  One plain store of 1 per workgroup that found
//                                     something: every writer stores the same value, so the stores need no ordering among themselves.
//              2. adam_book_k         one thread: bad = scan_flag, scan_flag = 0 (ready for the next step, the host never clears it);
//                                     clean -> step += 1, skipped_in_a_row = 0, the coefficients of the new step in double (the formula
//                                     of lbc_adam_launch), stored as floats; bad -> skipped_total += 1, skipped_in_a_row += 1 (step
//                                     and coefficients stay).
//              3. adam_update_k       coefficients read from the record; the whole grid returns before its first load when bad != 0,
//                                     so p, m and v keep their bits.
//   clipped  lbc_adam_clipped_launch  the gradient pass also sums the squares (adam_grad_pass_k<true>: per lane (double)x * (double)x,
//                                     exact in f64; lanes, then waves, combined in a fixed order; one partial per chunk behind the
//                                     record's header; no atomics, the norm must not depend on the order in which workgroups arrive).
//                                     The bookkeeping workgroup adds the partials in a fixed order and, on a clean step, stores
//                                     grad_norm = sqrt(sum), torch.nn.utils.clip_grad_norm_'s clip_coef and clipped_total; a bad step
//                                     keeps all three (its partials are NaN / Inf and are overwritten by the next call's first launch).
//                                     The update multiplies every gradient element by clip_coef as a SEPARATELY ROUNDED f32 product:
//                                     with clip_coef == 1 the step is the guarded step, with clip_coef < 1 the guarded step on gradients
//                                     scaled by that float.  g is not written.
//   recipe   lbc_adam_recipe_launch   lr is not an argument: on a clean step the bookkeeping thread evaluates the schedule (linear
//                                     warm-up, then constant / cosine / step) in double at k = step - 1, the number of updates applied
//                                     before this one.  The step count lives in the record and a skipped step does not advance it, so
//                                     the schedule can only be evaluated there without a sync.  It also stores lr, decay_factor =
//                                     (float)(1 - lr * wd) (decoupled; else 1) and counts ema_updates; a bad step keeps all of them.
//                                     kDecoupled: p is first multiplied by decay_factor as a SEPARATELY ROUNDED f32 product (the coupled
//                                     wd is then 0).  kEma: e = e + w * (p' - e), w = (float)(1 - decay), on the updated p' still in
//                                     registers; e moves 16 bytes per lane like m and v (8 B/element on top of the clipped step's 32)
//                                     and keeps its bits on a bad step like p, m and v.  Without either it IS the clipped update.
// Kernel boundaries order the launches of a step: a launch on a stream sees every store of the launches before it.
// The three records are prefix-compatible (lbc_adam_state's 40 bytes open lbc_adam_clip_state's 64, which open lbc_adam_recipe_state's 88:
// the static_asserts of c_api.cpp), so the kernels take the widest type and each level touches only the fields of its own record.
#include "lbc_common.hpp"
#include "lbc_hip.h"
#include "lbc_kernels.hpp"
#include <math.h>
#include <stddef.h>

namespace {

enum { kPlain = 0, kGuarded = 1, kClipped = 2, kRecipe = 3 };

static_assert(offsetof(lbc_adam_state, bad) == offsetof(lbc_adam_recipe_state, bad) && offsetof(lbc_adam_clip_state, bad) == offsetof(lbc_adam_recipe_state, bad) &&
              offsetof(lbc_adam_state, inv_bc2_sqrt) == offsetof(lbc_adam_recipe_state, inv_bc2_sqrt) &&
              offsetof(lbc_adam_clip_state, clip_coef) == offsetof(lbc_adam_recipe_state, clip_coef), "the records share their leading fields");

// ---- one element of the update -------------------------------------------------------------------------------------------------------
// THE definition of the step's arithmetic, for every level.  On the device nothing is left to the compiler: contraction is off for the
// whole function and every fused operation is written out, so the bits do not depend on what a compiler chooses to fuse:
//     gs = g * coef (rounded on its own; the plain and guarded levels pass 1, which is exact)
//     gg = fma(wd, p, gs)       m' = fma(omb1, gg - m, m)        denom = fma(inv_bc2_sqrt, sqrt(v'), eps)        p' = fma(-lr, m' / denom, p)
//     16-byte loop:  v' = fma(gg, omb2 * gg, beta2 * v)          scalar tail:  v' = beta2 * v + (omb2 * gg) * gg   (two roundings)
// kTail is history kept for bit compatibility: the list was first read off what hipcc emitted for the compiler-contracted kernels this
// function replaced, whose vector loop and scalar tail differed in exactly that way, and trained checkpoints resume bit for bit only if it
// stays.  tests/test_adam_bits.py holds these bits against a record taken before the function became the only one.
// The emulated build fuses nothing (x86-64 baseline has no fma): every operation is rounded on its own.
template <bool kTail>
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float coef, float wd, float beta2, float omb1,
                                            float omb2, float eps, float lr_over_bc1, float inv_bc2_sqrt)
{
#pragma clang fp contract(off)
    const float gs = g * coef;
#ifdef LBC_HIP_EMULATED_FOR_TESTS
    const float gg = gs + wd * p;
    m = m + (gg - m) * omb1;
    v = beta2 * v + omb2 * gg * gg;
    const float denom = sqrtf(v) * inv_bc2_sqrt + eps;
    p = p - lr_over_bc1 * (m / denom);
#else
    const float gg = __builtin_fmaf(wd, p, gs);
    m = __builtin_fmaf(omb1, gg - m, m);
    const float t = omb2 * gg, bv = beta2 * v;
    v = kTail ? bv + t * gg : __builtin_fmaf(gg, t, bv);
    const float denom = __builtin_fmaf(inv_bc2_sqrt, sqrtf(v), eps);
    p = __builtin_fmaf(-lr_over_bc1, m / denom, p);
#endif
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

// the host's constants of one update launch (lr_over_bc1 and inv_bc2_sqrt: the plain level only, the others read the record)
struct UpdateArgs { float lr_over_bc1, inv_bc2_sqrt, beta2, omb1, omb2, eps, wd, ema_w; };

// kLevel: kPlain (no record), kGuarded (the first 40 bytes of the record) or kClipped (clip_coef too; the recipe step's update is this
// level with kDecoupled / kEma).  <kClipped, false, false> under a recipe record is the clipped update itself.
template <int kLevel, bool kDecoupled, bool kEma>
__global__ __launch_bounds__(256) void adam_update_k(const AdamChunk* __restrict__ chunks, float* const* __restrict__ ema,
                                                     const lbc_adam_recipe_state* __restrict__ st, UpdateArgs a)
{
    float lr_over_bc1 = a.lr_over_bc1, inv_bc2_sqrt = a.inv_bc2_sqrt, coef = 1.0f, df = 1.0f;
    if (kLevel != kPlain) {
        if (st->bad != 0) return;     // (uniform over the grid, and before the first load: a skipped step touches nothing.  The record is not
                                      // written between the bookkeeping launch and the next gradient pass)
        lr_over_bc1 = st->lr_over_bc1;
        inv_bc2_sqrt = st->inv_bc2_sqrt;
        if (kLevel == kClipped) coef = st->clip_coef;
        if (kDecoupled) df = st->decay_factor;
    }
    const float beta2 = a.beta2, omb1 = a.omb1, omb2 = a.omb2, eps = a.eps, wd = a.wd, ema_w = a.ema_w;
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
        adam_update<false>(p.x, g.x, m.x, v.x, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
        adam_update<false>(p.y, g.y, m.y, v.y, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
        adam_update<false>(p.z, g.z, m.z, v.z, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
        adam_update<false>(p.w, g.w, m.w, v.w, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
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
        adam_update<true>(p, ch.g[i], m, v, coef, wd, beta2, omb1, omb2, eps, lr_over_bc1, inv_bc2_sqrt);
        ch.p[i] = p; ch.m[i] = m; ch.v[i] = v;
        if (kEma) ce[i] = ema_step(ce[i], p, ema_w);
    }
}

// ---- the gradient pass ---------------------------------------------------------------------------------------------------------------
constexpr unsigned kExpMask = 0x7f800000u;     // f32 exponent field: all ones = NaN or +-Inf

// one 16-byte load's worth: the largest |x| bit pattern seen (a non-finite element is one whose pattern with the sign removed is
// >= kExpMask) and, with kNorm, the exact squares, added in element order
template <bool kNorm>
__device__ __forceinline__ void grad_acc4(unsigned& bits, double& sq, uint4 q)
{
    const unsigned a = q.x & 0x7fffffffu, b = q.y & 0x7fffffffu, c = q.z & 0x7fffffffu, d = q.w & 0x7fffffffu;
    const unsigned ab = a > b ? a : b, cd = c > d ? c : d, m = ab > cd ? ab : cd;
    bits = bits > m ? bits : m;
    if (kNorm) {
        const double x = (double)__builtin_bit_cast(float, q.x), y = (double)__builtin_bit_cast(float, q.y);
        const double z = (double)__builtin_bit_cast(float, q.z), w = (double)__builtin_bit_cast(float, q.w);
        sq += x * x;
        sq += y * y;
        sq += z * z;
        sq += w * w;
    }
}

// kNorm = false is the scan alone: no f64 work, no partial store (st is then any of the three records, partial unused)
template <bool kNorm>
__global__ __launch_bounds__(256) void adam_grad_pass_k(const AdamChunk* __restrict__ chunks, lbc_adam_state* __restrict__ st,
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
        grad_acc4<kNorm>(bits, s0, q0);
        grad_acc4<kNorm>(bits, s1, q1);
        grad_acc4<kNorm>(bits, s2, q2);
        grad_acc4<kNorm>(bits, s3, q3);
    }
    for (; i < n4; i += 256) grad_acc4<kNorm>(bits, s0, g4[i]);
    const unsigned* __restrict__ g1 = reinterpret_cast<const unsigned*>(ch.g);
    for (int j = (n4 << 2) + threadIdx.x; j < ch.n; j += 256) {
        const unsigned u = g1[j];
        const unsigned a = u & 0x7fffffffu;
        bits = bits > a ? bits : a;
        if (kNorm) {
            const double x = (double)__builtin_bit_cast(float, u);
            s0 += x * x;
        }
    }
    double sq = (s0 + s1) + (s2 + s3);
    // lanes in a fixed order: the xor butterfly adds the same two values on both partners (a + b == b + a bit for bit), so every
    // lane of the wave ends with the same sum, whatever the hardware does around it.  "Found one" travels as a max of the patterns
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = __shfl_xor(bits, off);
        bits = bits > o ? bits : o;
        if (kNorm) sq += __shfl_xor(sq, off);
    }
    if ((threadIdx.x & 63) == 0) {
        wave_bits[threadIdx.x >> 6] = bits;
        if (kNorm) wave_sq[threadIdx.x >> 6] = sq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned a = wave_bits[0] > wave_bits[1] ? wave_bits[0] : wave_bits[1];
        const unsigned b = wave_bits[2] > wave_bits[3] ? wave_bits[2] : wave_bits[3];
        if (kNorm) partial[blockIdx.x] = (wave_sq[0] + wave_sq[1]) + (wave_sq[2] + wave_sq[3]);
        if ((a > b ? a : b) >= kExpMask) st->scan_flag = 1;
    }
}

// ---- the bookkeeping -----------------------------------------------------------------------------------------------------------------
// what the bookkeeping thread needs of the call (validated on the host), passed by value.  The guarded and clipped steps fill in base_lr
// (their argument lr), the betas, eps, wd and max_norm; the schedule is the recipe step's
struct Book {
    double base_lr, s0, min_lr, gamma, wd, max_norm, ema_decay, beta1, beta2, eps;
    long long W, T, S;
    int kind, decoupled;
};

__device__ __forceinline__ double schedule_lr(const Book& r, long long k)
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

// the chunks' partial sums of squares, added by 256 threads in a fixed order (valid in thread 0)
__device__ __forceinline__ double sum_partials(const double* __restrict__ partial, int nchunks)
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
    return red[0];
}

// one workgroup (256 threads from kClipped on, where it first adds the partials); one thread does the bookkeeping of level kLevel
template <int kLevel>
__global__ __launch_bounds__(256) void adam_book_k(lbc_adam_recipe_state* __restrict__ st, const double* __restrict__ partial, int nchunks, Book r)
{
    const double sumsq = kLevel >= kClipped ? sum_partials(partial, nchunks) : 0.0;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int bad = st->scan_flag != 0;
    st->scan_flag = 0;
    st->bad = bad;
    if (bad) {
        st->skipped_total += 1;
        st->skipped_in_a_row += 1;
        return;                       // step, the coefficients and every field behind them keep the last clean step's values
    }
    const long long step = st->step + 1;
    st->step = step;
    st->skipped_in_a_row = 0;
    const double lr = kLevel == kRecipe ? schedule_lr(r, step - 1) : r.base_lr;      // (below kRecipe lr is the call's argument)
    const double bc1 = 1.0 - pow(r.beta1, (double)step);
    const double bc2 = 1.0 - pow(r.beta2, (double)step);
    st->lr_over_bc1 = (float)(lr / bc1);
    st->inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    if (kLevel >= kClipped) {
        // torch.nn.utils.clip_grad_norm_: coef = max_norm / (norm + 1e-6), clamped to 1 -- with the norm kept in double
        const double norm = sqrt(sumsq);
        const double c = r.max_norm / (norm + 1e-6);
        const float coef = (r.max_norm > 0.0 && c < 1.0) ? (float)c : 1.0f;
        st->grad_norm = norm;
        st->clip_coef = coef;
        st->clipped_total += (coef < 1.0f) ? 1 : 0;
    }
    if (kLevel == kRecipe) {
        st->lr = lr;
        st->decay_factor = r.decoupled ? (float)(1.0 - lr * r.wd) : 1.0f;
        if (r.ema_decay > 0.0) st->ema_updates += 1;
    }
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------
long long g_adam_prof_elems = 0;      // lbc_adam_profile_elems: what the launch profiler books for an optimizer launch

// every step: (gradient pass, bookkeeping,) update.  state_dev is the record of `level` (null for kPlain, which takes `step` from the host
// instead), followed from kClipped on by one double per chunk (every header is a multiple of 8 bytes)
int launch_step(int level, const AdamChunk* chunks, int nchunks, void* state_dev, float* const* ema_dev, const Book& b, int step, hipStream_t s)
{
    static const char* const labels[] = {"adam", "adam_guarded", "adam_clipped", "adam_recipe"};
    static const size_t headers[] = {0, sizeof(lbc_adam_state), sizeof(lbc_adam_clip_state), sizeof(lbc_adam_recipe_state)};
    const bool ema = b.ema_decay > 0.0;
    // algorithmic bytes per element: read p, g, m, v and write p, m, v = 7 x 4 (648 MB for the 23.13 M parameters of the student); the
    // gradient pass reads g once more (a skipped step moves those 4 only; the class books the clean step); the average reads and writes e
    LbcProfScope prof(labels[level], 0.0, (level == kPlain ? 28.0 : ema ? 40.0 : 32.0) * (double)g_adam_prof_elems, s);
    const dim3 grid((unsigned)nchunks), block(256);
    lbc_adam_recipe_state* st = static_cast<lbc_adam_recipe_state*>(state_dev);
    double* partial = reinterpret_cast<double*>(static_cast<char*>(state_dev) + headers[level]);
    UpdateArgs a = {0.0f, 0.0f, (float)b.beta2, (float)(1.0 - b.beta1), (float)(1.0 - b.beta2), (float)b.eps,
                    b.decoupled ? 0.0f : (float)b.wd, (float)(1.0 - b.ema_decay)};
    const lbc_adam_recipe_state* cst = st;
#define LBC_UPDATE(L, D, E) hipLaunchKernelGGL((adam_update_k<L, D, E>), grid, block, 0, s, chunks, ema_dev, cst, a)
    if (level == kPlain) {
        a.lr_over_bc1 = (float)(b.base_lr / (1.0 - pow(b.beta1, (double)step)));
        a.inv_bc2_sqrt = (float)(1.0 / sqrt(1.0 - pow(b.beta2, (double)step)));
        LBC_UPDATE(kPlain, false, false);
    } else if (level == kGuarded) {
        hipLaunchKernelGGL(adam_grad_pass_k<false>, grid, block, 0, s, chunks, static_cast<lbc_adam_state*>(state_dev), (double*)nullptr);
        hipLaunchKernelGGL(adam_book_k<kGuarded>, dim3(1), dim3(64), 0, s, st, (const double*)nullptr, nchunks, b);
        LBC_UPDATE(kGuarded, false, false);
    } else {
        hipLaunchKernelGGL(adam_grad_pass_k<true>, grid, block, 0, s, chunks, static_cast<lbc_adam_state*>(state_dev), partial);
        if (level == kClipped) hipLaunchKernelGGL(adam_book_k<kClipped>, dim3(1), block, 0, s, st, (const double*)partial, nchunks, b);
        else                   hipLaunchKernelGGL(adam_book_k<kRecipe>, dim3(1), block, 0, s, st, (const double*)partial, nchunks, b);
        if (b.decoupled) { if (ema) LBC_UPDATE(kClipped, true, true); else LBC_UPDATE(kClipped, true, false); }
        else             { if (ema) LBC_UPDATE(kClipped, false, true); else LBC_UPDATE(kClipped, false, false); }
    }
#undef LBC_UPDATE
    return lbc_check_launch(labels[level]);
}

// the arguments of the plain, guarded and clipped steps: a constant lr, coupled decay, no average
Book constant_book(double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm)
{
    Book b = {};
    b.base_lr = lr; b.beta1 = beta1; b.beta2 = beta2; b.eps = eps; b.wd = weight_decay; b.max_norm = max_norm; b.kind = LBC_LR_CONSTANT;
    return b;
}

}  // namespace

extern "C" void lbc_adam_profile_elems(long long n) { g_adam_prof_elems = n > 0 ? n : 0; }

int lbc_adam_launch(const AdamChunk* chunks_dev, int nchunks, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int step, hipStream_t s)
{
    LBC_REQUIRE(nchunks > 0 && step >= 1, "adam: bad args");
    return launch_step(kPlain, chunks_dev, nchunks, nullptr, nullptr, constant_book(lr, beta1, beta2, eps, weight_decay, 0.0), step, s);
}

int lbc_adam_guarded_launch(const AdamChunk* chunks_dev, int nchunks, double lr, double beta1, double beta2, double eps,
                            double weight_decay, lbc_adam_state* state_dev, hipStream_t s)
{
    LBC_REQUIRE(chunks_dev && nchunks > 0, "adam_guarded: bad args");
    LBC_REQUIRE(state_dev && ((uintptr_t)state_dev & 7) == 0, "adam_guarded: the state record must be a device pointer aligned to 8 bytes");
    return launch_step(kGuarded, chunks_dev, nchunks, state_dev, nullptr, constant_book(lr, beta1, beta2, eps, weight_decay, 0.0), 0, s);
}

int lbc_adam_clipped_launch(const AdamChunk* chunks_dev, int nchunks, double lr, double beta1, double beta2, double eps,
                            double weight_decay, double max_norm, lbc_adam_clip_state* state_dev, hipStream_t s)
{
    LBC_REQUIRE(chunks_dev && nchunks > 0, "adam_clipped: bad args (chunk table %p, nchunks %d)", (const void*)chunks_dev, nchunks);
    LBC_REQUIRE(state_dev && ((uintptr_t)state_dev & 7) == 0,
                "adam_clipped: the state record must be a device pointer aligned to 8 bytes (lbc_adam_clip_state_bytes(nchunks) bytes)");
    LBC_REQUIRE(max_norm == max_norm, "adam_clipped: max_norm is NaN (<= 0 measures without clipping)");
    return launch_step(kClipped, chunks_dev, nchunks, state_dev, nullptr, constant_book(lr, beta1, beta2, eps, weight_decay, max_norm), 0, s);
}

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
    Book b = constant_book(rc->base_lr, rc->beta1, rc->beta2, rc->eps, rc->weight_decay, rc->max_norm);
    b.s0 = rc->warmup_start; b.min_lr = rc->min_lr; b.gamma = rc->gamma; b.ema_decay = rc->ema_decay;
    b.W = rc->warmup_steps; b.T = rc->total_steps; b.S = rc->step_size;
    b.kind = rc->schedule; b.decoupled = decoupled;
    return launch_step(kRecipe, chunks_dev, nchunks, state_dev, ema_dev, b, 0, s);
}
