// Shared by the slab-streaming fused kernels (vv_motion.hip, vv_chain.hip): the LDS-DMA copy of the weight ring and the GELU of the GEGLU feed-forward.
#pragma once
#include "vv_lds_dma.h"

// exact (erf) GELU through Abramowitz-Stegun 7.1.26 (|erf error| <= 1.5e-7, far below the h16 rounding that follows): 2 transcendentals
// + ~12 VALU instead of the ~30 of erff -- with ONE wave per SIMD the activation is not hidden behind another wave's MFMAs
// (two GELUs at once on packed fp32 math: v_pk_fma_f32)
__device__ __forceinline__ vv_f32x2 gelu2(vv_f32x2 x) {
    const vv_f32x2 ax = {fabsf(x.x), fabsf(x.y)};
    const vv_f32x2 z = ax * 0.70710678118654752f;
    const vv_f32x2 d = __builtin_elementwise_fma(z, (vv_f32x2){0.3275911f, 0.3275911f}, (vv_f32x2){1.0f, 1.0f});
    const vv_f32x2 t = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    vv_f32x2 q = __builtin_elementwise_fma(t, (vv_f32x2){1.061405429f, 1.061405429f}, (vv_f32x2){-1.453152027f, -1.453152027f});
    q = __builtin_elementwise_fma(q, t, (vv_f32x2){1.421413741f, 1.421413741f});
    q = __builtin_elementwise_fma(q, t, (vv_f32x2){-0.284496736f, -0.284496736f});
    q = __builtin_elementwise_fma(q, t, (vv_f32x2){0.254829592f, 0.254829592f});
    q = q * t;
    const vv_f32x2 ez = z * z * -1.4426950408889634f;
    const vv_f32x2 e = {__builtin_amdgcn_exp2f(ez.x), __builtin_amdgcn_exp2f(ez.y)};
    const vv_f32x2 erfc = q * e;                                       // 1 - erf(|x| / sqrt 2)
    return __builtin_elementwise_fma(ax * 0.5f, (vv_f32x2){1.0f, 1.0f} - erfc, x * 0.5f);      // 0.5 x (1 + sign(x) (1 - erfc))
}
// The fused kernels evaluate this A&S form.  gelu_poly2 (vv_common.h: packed fp32 polynomial, no v_rcp / v_exp -- the GEMM kernels' GEGLU epilogue since
// round 6, +4.5..6.6 % there) was measured here too: the motion module LOSES 3 % (3.04 -> 3.13 ms), the chain tail is unchanged -- these kernels
// run one or two waves per SIMD beside the matrix pipe, the transcendental unit is otherwise idle and the polynomial's 14 extra packed FMAs are not (profiles/r6_gelu_ab.txt)
