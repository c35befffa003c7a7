// Per-pixel steps the fused paste kernels share (vv_grain.hip: table + grain; vv_blend.hip: table + membrane + grain), so both compute the
// same bytes from one statement: the window's pixel as vv_roi_paste_composite reads it, and the stateless noise of include/vvgrain.h.
#pragma once
#include "vv_image_px.h"

namespace vvpaste {

typedef unsigned long long u64;

// the window's pixel (xx, yy) of frame t's Hm x Wm image `src`, as vv_roi_paste_composite reads it
__device__ __forceinline__ void window_px(const uint8_t* src, int Hm, int Wm, int xx, int yy, int h, int w, uint8_t* p) {
    if (Hm == h && Wm == w) {
        const uint8_t* s = src + ((int64_t)yy * w + xx) * 3;
        p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
    } else {
        vvpx::bilinear_px(src, Hm, Wm, 3, xx, yy, h, w, p);
    }
}

// the noise of one key (include/vvgrain.h): splitmix64's finaliser, the sum of its eight bytes centred
__device__ __forceinline__ int noise_sum(u64 key) {
    u64 z = key + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    // byte sums in parallel: pairs, then quads, then all eight
    z = (z & 0x00FF00FF00FF00FFull) + ((z >> 8) & 0x00FF00FF00FF00FFull);
    z = (z & 0x0000FFFF0000FFFFull) + ((z >> 16) & 0x0000FFFF0000FFFFull);
    return (int)((unsigned)z + (unsigned)(z >> 32)) - 1020;
}

// the key of frame-coordinate pixel (x, y) of the frame with index `frame_id` in the caller's clip
__device__ __forceinline__ u64 noise_key(int seed, int frame_id, int H, int W, int x, int y) {
    return ((u64)(unsigned)seed << 32) ^ (((u64)(int64_t)frame_id * (u64)H + (u64)y) * (u64)W + (u64)x);
}

// g[c] = the grain of include/vvgrain.h for the amplitudes a[c] (1/16 levels): (a s 5017 + 2^23) >> 24
__device__ __forceinline__ void grain_px(u64 key, int mode, const int* a, int* g) {
    const int s0 = noise_sum(mode ? key * 3ull : key);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int s = (mode && c) ? noise_sum(key * 3ull + (u64)c) : s0;
        g[c] = (a[c] * s * 5017 + (1 << 23)) >> 24;
    }
}

}  // namespace vvpaste
