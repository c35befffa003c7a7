// What the byte-image kernels (the image-stage features: vv_spans, vv_mask, vv_tone, vv_grain, vv_blend, vv_plate, vv_align, vv_flicker,
// vv_shadow, vv_platetone, vv_detail, and the boxes of vv_roi) share, one statement each: the wave-64 butterfly reductions their counts and extents go through before
// they reach LDS or a global atomic, the luma of the cut statistics and the tracker, and the 4-pixel loads and stores of masks and RGB bytes.
// All integer: a reduction gives the same value in every lane whatever the order.  A file takes what it uses with using-declarations; a helper
// that differs between two files in any token stays in its file.
#pragma once
#include "vv_common.h"

namespace vvwave {

typedef unsigned long long u64;

// ---- reductions over the 64 lanes of a wave: every lane gets the result ------------------------------------------------------------------
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}
__device__ __forceinline__ u64 wave_min64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
        const u64 other = ((u64)hi << 32) | lo;
        v = other < v ? other : v;
    }
    return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- pixels ------------------------------------------------------------------------------------------------------------------------------
// Rec. 601 luma of an RGB byte triple, rounded (include/vvspans.h, include/vvalign.h)
__device__ __forceinline__ unsigned luma(unsigned r, unsigned g, unsigned b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

struct __attribute__((aligned(4))) U3 { unsigned a, b, c; };

// VEC: a unit is P = 4 pixels whose first is 4-byte aligned (the launcher's business); otherwise one pixel.
// the P mask bytes at m, byte p in bits 8 p ..
template <bool VEC> __device__ __forceinline__ unsigned load_mask(const uint8_t* m) {
    if constexpr (VEC) return *reinterpret_cast<const unsigned*>(m);
    else return *m;
}
template <bool VEC> __device__ __forceinline__ void store_mask(uint8_t* m, unsigned w) {
    if constexpr (VEC) *reinterpret_cast<unsigned*>(m) = w;
    else *m = (uint8_t)w;
}
// the 3 P image bytes at px, as values
template <bool VEC> __device__ __forceinline__ void load_px(const uint8_t* px, unsigned* v) {
    if constexpr (VEC) {
        const U3 q = *reinterpret_cast<const U3*>(px);
        const unsigned w[3] = {q.a, q.b, q.c};
#pragma unroll
        for (int j = 0; j < 12; ++j) v[j] = (w[j >> 2] >> ((j & 3) * 8)) & 255u;
    } else {
        v[0] = px[0]; v[1] = px[1]; v[2] = px[2];
    }
}
// the 3 P image bytes at px from values (load_px's inverse)
template <bool VEC> __device__ __forceinline__ void store_px(uint8_t* px, const unsigned* v) {
    if constexpr (VEC) {
        unsigned w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
        *reinterpret_cast<U3*>(px) = U3{w[0], w[1], w[2]};
    } else {
        px[0] = (uint8_t)v[0]; px[1] = (uint8_t)v[1]; px[2] = (uint8_t)v[2];
    }
}

}  // namespace vvwave
