// Per-pixel device arithmetic of the uint8 image steps (K11), shared by vv_image.hip (resize, feather composite) and vv_roi.hip (the fused
// paste + composite of mask-region inference), so both compute the same bytes from one statement of the arithmetic.
#pragma once
#include "vv_common.h"
#pragma clang fp contract(off)

namespace vvpx {

// ---- cv2.resize on uint8 (legacy fixed-point INTER_LINEAR) ---------------------------------------------------
__device__ __forceinline__ void lin_coef(int d, int ssize, int dsize, int& s0, int& s1, int& a0, int& a1) {
    const double scale = (double)ssize / (double)dsize;
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
    a0 = __float2int_rn((1.0f - f) * 2048.0f);
    a1 = __float2int_rn(f * 2048.0f);
    s0 = s; s1 = min(s + 1, ssize - 1);
}
// pixel (x, y) of one Hs x Ws x ch image resized to Hd x Wd: ch bytes to dst
__device__ __forceinline__ void bilinear_px(const uint8_t* img, int Hs, int Ws, int ch, int x, int y, int Hd, int Wd, uint8_t* dst) {
    int x0, x1, ax0, ax1, y0, y1, by0, by1;
    lin_coef(x, Ws, Wd, x0, x1, ax0, ax1);
    lin_coef(y, Hs, Hd, y0, y1, by0, by1);
    const uint8_t* r0 = img + (int64_t)y0 * Ws * ch;
    const uint8_t* r1 = img + (int64_t)y1 * Ws * ch;
    for (int c = 0; c < ch; ++c) {
        const int h0 = r0[x0 * ch + c] * ax0 + r0[x1 * ch + c] * ax1;
        const int h1 = r1[x0 * ch + c] * ax0 + r1[x1 * ch + c] * ax1;
        int v = (((by0 * (h0 >> 4)) >> 16) + ((by1 * (h1 >> 4)) >> 16) + 2) >> 2;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        dst[c] = (uint8_t)v;
    }
}

// ---- 5x5 chamfer distance (16.16 fixed point; a=1, b=1.4, c=2.1969), windowed closed form ---------------------
constexpr int C_HV = 65536, C_DIAG = 91750, C_LONG = 143976;
constexpr int DIST_BIG = (0x7fffffff >> 2);
__device__ __forceinline__ int chamfer_fixed(int dx, int dy) {
    dx = dx < 0 ? -dx : dx; dy = dy < 0 ? -dy : dy;
    if (dx < dy) { const int tmp = dx; dx = dy; dy = tmp; }
    return dx >= 2 * dy ? dy * C_LONG + (dx - 2 * dy) * C_HV : (dx - dy) * C_LONG + (2 * dy - dx) * C_DIAG;
}
// distance (fixed) from (x,y) to the nearest pixel whose "is-zero" predicate holds, searched in a (2R+1)^2 window.
// want_nonzero=false: nearest pixel with bin==0; true: nearest pixel with bin!=0 (== zero pixel of the inverse)
__device__ __forceinline__ int window_dist(const uint8_t* img, int H, int W, int x, int y, int R, bool want_nonzero) {
    int best = DIST_BIG;
    for (int dy = -R; dy <= R; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
        for (int dx = -R; dx <= R; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= W) continue;
            const bool nz = img[(int64_t)yy * W + xx] > 0;
            if (nz == want_nonzero) { const int d = chamfer_fixed(dx, dy); best = d < best ? d : best; }
        }
    }
    return best;
}

// ---- feathered composite (reference diffuerase.py:77-112) ----------------------------------------------------
// alpha of pixel (x, y) of one H x W mask: 0 wherever no mask pixel lies in its (2R+1)^2 window, R = ceil(feather)
__device__ __forceinline__ float feather_alpha(const uint8_t* img, int H, int W, int x, int y, float feather, int R) {
    const bool inside = img[(int64_t)y * W + x] > 0;
    float alpha;
    if (feather > 0.f) {
        // d_in: distance of masked pixels to the nearest unmasked one; d_out: the converse (0 on the own side)
        const int d = window_dist(img, H, W, x, y, R, !inside);
        const float df = (float)d * (1.0f / 65536.0f);
        const float d_in = inside ? df : 0.f, d_out = inside ? 0.f : df;
        alpha = 0.5f + (d_in - d_out) / (2.0f * feather);
        alpha = fminf(fmaxf(alpha, 0.f), 1.f);
    } else alpha = inside ? 1.f : 0.f;
    return alpha;
}
// out[c] = clip(rint(alpha * inp[c] + (1 - alpha) * orig[c])), 3 channels
__device__ __forceinline__ void feather_blend(float alpha, const uint8_t* inp, const uint8_t* orig, uint8_t* out) {
    const float om = 1.0f - alpha;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = alpha * (float)inp[c];
        const float b = om * (float)orig[c];
        float v = rintf(a + b);
        v = fminf(fmaxf(v, 0.f), 255.f);
        out[c] = (uint8_t)v;
    }
}

}  // namespace vvpx
