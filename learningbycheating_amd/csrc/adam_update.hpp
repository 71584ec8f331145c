// The element update shared by adam_clip.hip (adam_clipped_k) and adam_recipe.hip (adam_recipe_k): one definition, because its list of
// fused operations is pinned to the compiler (below) and a second copy would be a second thing to keep pinned.
#pragma once
#include "lbc_common.hpp"

// One element of the update.  The contract with adam_guarded_k is bitwise, and that kernel leaves the choice of which multiply fuses
// into which add to the compiler (-ffp-contract=fast), and a second copy of its expressions behind a product by the coefficient is
// not guaranteed the same choices.  So on the device nothing here is left to the compiler: contraction is off for the whole function
// and every fused operation is written out, mirroring what hipcc emits for adam_guarded_k (read from its gfx950 ISA as compiled by
// ROCm 7.2.0):
//     gg = fma(wd, p, g)        m' = fma(omb1, gg - m, m)        denom = fma(inv_bc2_sqrt, sqrt(v'), eps)        p' = fma(-lr, m' / denom, p)
//     16-byte loop:  v' = fma(gg, omb2 * gg, beta2 * v)          scalar tail:  v' = beta2 * v + (omb2 * gg) * gg   (two roundings)
// with g = g * coef rounded on its own in front.  THIS LIST DEPENDS ON THE COMPILER: a hipcc that fuses adam_guarded_k differently
// breaks the bitwise contract.  tests/test_grad_clip.py compares the two kernels bit for bit on the GPU with and without weight
// decay and fails then; the list is read off adam_guarded_k's ISA again (kTail separates the two loops because they differ today).
// The emulated build fuses nothing (x86-64 baseline has no fma): there the expressions of adam_guarded_k are kept as they are, with
// only the product by the coefficient kept from contracting.
template <bool kTail>
__device__ __forceinline__ void clipped_update(float& p, float g, float& m, float& v, float coef, float wd, float beta2, float omb1,
                                               float omb2, float eps, float lr_over_bc1, float inv_bc2_sqrt)
{
#ifdef LBC_HIP_EMULATED_FOR_TESTS
    float gs;
    {
#pragma clang fp contract(off)
        gs = g * coef;
    }
    const float gg = gs + wd * p;
    m = m + (gg - m) * omb1;
    v = beta2 * v + omb2 * gg * gg;
    const float denom = sqrtf(v) * inv_bc2_sqrt + eps;
    p = p - lr_over_bc1 * (m / denom);
#else
#pragma clang fp contract(off)
    const float gs = g * coef;
    const float gg = __builtin_fmaf(wd, p, gs);
    m = __builtin_fmaf(omb1, gg - m, m);
    const float t = omb2 * gg, bv = beta2 * v;
    v = kTail ? bv + t * gg : __builtin_fmaf(gg, t, bv);
    const float denom = __builtin_fmaf(inv_bc2_sqrt, sqrtf(v), eps);
    p = __builtin_fmaf(-lr_over_bc1, m / denom, p);
#endif
}
