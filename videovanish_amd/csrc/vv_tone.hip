// Seam tone matching (videovanish_amd/tonematch.py): the two device steps around the host's per-frame fit.
//   vvt_ring_stats            16 integer sums per frame over the ring: the unmasked pixels of the window within `ring` pixels (a box) of a mask
//                             pixel, where both the model's pixel x and the original pixel y exist
//   vvt_paste_lut_composite   vv_roi_paste_composite with the window's bytes sent through a per-frame, per-channel table first
// The ring test is a separable box dilation on bits (vv_ring_bits.h, shared with vv_grain.hip): two ballots per halo row, a log-step shift-OR,
// a column OR per tile row.  Nothing is searched per pixel; a tile without a ring pixel ends after the mask reads.
// The sums go registers -> wave reduction -> 64-bit LDS atomics -> one set of 64-bit global integer atomics per block (as vv_spans.hip's pair
// statistics): integer adds, so the result does not depend on the order.  The per-pixel arithmetic (resize, feather) is vv_image_px.h, the
// statement vv_roi.hip uses, so an identity table gives vv_roi_paste_composite's bytes.
#include "vv_image_px.h"
#include "vv_ring_bits.h"
#include "vv_wave_bytes.h"
#include "../../include/vvtone.h"
#pragma clang fp contract(off)

namespace {

using vvwave::wave_sum64;
using vvring::TB;                                // threads per block: 4 waves
using vvring::TW;                                // the tile: one lane per column, TH * TW / TB = 8 rows per thread
using vvring::TH;
using vvring::u64;
constexpr int NSUM = 16;
static_assert(VVT_MAX_RING == vvring::MAX_RING, "the ring of vv_ring_bits.h");

// the window's pixel (xx, yy) of frame t's Hm x Wm image `src`, as vv_roi_paste_composite reads it
__device__ __forceinline__ void window_px(const uint8_t* src, int Hm, int Wm, int xx, int yy, int h, int w, uint8_t* p) {
    if (Hm == h && Wm == w) {
        const uint8_t* s = src + ((int64_t)yy * w + xx) * 3;
        p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
    } else {
        vvpx::bilinear_px(src, Hm, Wm, 3, xx, yy, h, w, p);
    }
}

// grid: tiles_x * tiles_y * T blocks; block b = tile (b % tiles_x, (b / tiles_x) % tiles_y) of frame b / (tiles_x * tiles_y).  Every read of the
// mask and of orig is bounds-checked against the frame, every read of patch lies inside frame t's Hm x Wm image (xx < w, yy < h), whatever the
// offsets hold; the only writes are the atomics into sums[t].
__global__ __launch_bounds__(TB) void ring_stats_kernel(const uint8_t* __restrict__ patch, int Hm, int Wm, const uint8_t* __restrict__ orig,
                                                        const uint8_t* __restrict__ mask, const int* __restrict__ offsets, int H, int W, int h, int w,
                                                        int r, int tiles_x, int tiles_y, u64* __restrict__ sums) {
    __shared__ u64 rowbits[vvring::HALO_ROWS];   // scratch of the row pass
    __shared__ u64 own[TH];                      // tile row y: bit px = the pixel's own mask
    __shared__ u64 ringbits[TH];                 // tile row y: bit px = the pixel belongs to the ring
    __shared__ u64 tot[NSUM];
    const int tile = (int)blockIdx.x % (tiles_x * tiles_y), t = (int)blockIdx.x / (tiles_x * tiles_y);
    const int tx0 = (tile % tiles_x) * TW, ty0 = (tile / tiles_x) * TH;        // the tile's origin in the window
    const int oy = offsets[t * 2 + 0], ox = offsets[t * 2 + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < NSUM) tot[threadIdx.x] = 0;
    vvring::ring_bits<false>(mask + (int64_t)t * H * W, H, W, oy, ox, tx0, ty0, h, w, r, rowbits, own, ringbits, nullptr);

    u64 acc[NSUM];
#pragma unroll
    for (int i = 0; i < NSUM; ++i) acc[i] = 0;
    bool any = false;
    const uint8_t* src = patch + (int64_t)t * Hm * Wm * 3;
    for (int y = wave; y < TH; y += TB / 64) {                                 // wave-uniform
        const u64 bits = ringbits[y];
        if (!bits) continue;
        any = true;
        if (!((bits >> lane) & 1ull)) continue;
        const int xx = tx0 + lane, yy = ty0 + y;
        uint8_t p[3];
        window_px(src, Hm, Wm, xx, yy, h, w, p);
        const uint8_t* o = orig + (((int64_t)t * H + (oy + yy)) * W + (ox + xx)) * 3;
        acc[0] += 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned xv = p[c], yv = o[c];                               // products <= 255^2: 32 bits per pixel, 64 from there on
            acc[1 + c] += xv; acc[4 + c] += yv;
            acc[7 + c] += xv * xv; acc[10 + c] += xv * yv; acc[13 + c] += yv * yv;
        }
    }
    if (any) {                                                                 // wave-uniform: `any` was set from an LDS word every lane read
#pragma unroll
        for (int i = 0; i < NSUM; ++i) {
            const u64 s = wave_sum64(acc[i]);
            if (lane == 0 && s) atomicAdd(&tot[i], s);
        }
    }
    __syncthreads();
    if (threadIdx.x < NSUM && tot[threadIdx.x]) atomicAdd(&sums[(int64_t)t * NSUM + threadIdx.x], tot[threadIdx.x]);
}

// pixel (x, y) of frame t, as roi_paste_kernel of vv_roi.hip; inside the window the three bytes go through frame t's tables first
__global__ __launch_bounds__(TB) void paste_lut_kernel(const uint8_t* __restrict__ patch, int Hm, int Wm, const uint8_t* __restrict__ orig,
                                                       const uint8_t* __restrict__ mask, const int* __restrict__ offsets, const uint8_t* __restrict__ lut,
                                                       int T, int H, int W, int h, int w, float feather, int R, uint8_t* __restrict__ out) {
    const int64_t n = (int64_t)T * H * W;
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % W); const int y = (int)((i / W) % H); const int t = (int)(i / ((int64_t)W * H));
    const int yy = y - offsets[t * 2 + 0], xx = x - offsets[t * 2 + 1];
    const uint8_t* o = orig + i * 3;
    uint8_t* d = out + i * 3;
    if (yy < 0 || yy >= h || xx < 0 || xx >= w) {
        d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
        return;
    }
    uint8_t p[3];
    window_px(patch + (int64_t)t * Hm * Wm * 3, Hm, Wm, xx, yy, h, w, p);
    const uint8_t* tab = lut + (int64_t)t * 3 * 256;
    p[0] = tab[p[0]]; p[1] = tab[256 + p[1]]; p[2] = tab[512 + p[2]];
    if (feather < 0.f) {
        d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
        return;
    }
    const float alpha = vvpx::feather_alpha(mask + (int64_t)t * H * W, H, W, x, y, feather, R);
    vvpx::feather_blend(alpha, p, o, d);
}

bool bad_sizes(int Hm, int Wm, int T, int H0, int W0, int h, int w) {
    return T <= 0 || H0 <= 0 || W0 <= 0 || Hm <= 0 || Wm <= 0 || h <= 0 || w <= 0 || h > H0 || w > W0;
}

}  // namespace

extern "C" int vvt_abi_version(void) { return VVT_ABI_VERSION; }
extern "C" const char* vvt_last_error(void) { return vv_last_error(); }

extern "C" int vvt_ring_stats(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets, int T, int H0, int W0,
                              int h, int w, int ring, int64_t* sums, void* stream) {
    if (!patch || !orig || !mask2d || !offsets || !sums || bad_sizes(Hm, Wm, T, H0, W0, h, w))
        VV_FAIL(VV_E_ARG, "vvt_ring_stats: bad args (no null pointer, sizes > 0, h <= H0, w <= W0)");
    if (ring < 1 || ring > VVT_MAX_RING) VV_FAIL(VV_E_UNSUPPORTED, "vvt_ring_stats: ring 1 .. %d is supported, not %d", VVT_MAX_RING, ring);
    const int tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * T;
    if (blocks > 0x7fffffff) VV_FAIL(VV_E_UNSUPPORTED, "vvt_ring_stats: %lld tiles are more than one launch holds", (long long)blocks);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, (size_t)T * NSUM * sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vvt_ring_stats: memset failed");
    hipLaunchKernelGGL(ring_stats_kernel, dim3((unsigned)blocks), dim3(TB), 0, st, patch, Hm, Wm, orig, mask2d, offsets, H0, W0, h, w, ring, tiles_x, tiles_y,
                       (u64*)sums);
    VV_CHECK_LAUNCH("vvt_ring_stats");
    return VV_OK;
}

extern "C" int vvt_paste_lut_composite(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets,
                                       const uint8_t* lut, int T, int H0, int W0, int h, int w, float feather_px, uint8_t* out, void* stream) {
    if (!patch || !orig || !offsets || !lut || !out || bad_sizes(Hm, Wm, T, H0, W0, h, w))
        VV_FAIL(VV_E_ARG, "vvt_paste_lut_composite: bad args (no null pointer, sizes > 0, h <= H0, w <= W0)");
    if (feather_px >= 0.f && !mask2d) VV_FAIL(VV_E_ARG, "vvt_paste_lut_composite: the feathered composite needs mask2d");
    if (feather_px > 64.f) VV_FAIL(VV_E_UNSUPPORTED, "vvt_paste_lut_composite: feather_px %.1f > 64", feather_px);
    const int R = feather_px > 0.f ? (int)ceilf(feather_px) : 0;
    const int64_t n = (int64_t)T * H0 * W0;
    hipLaunchKernelGGL(paste_lut_kernel, dim3((unsigned)((n + TB - 1) / TB)), dim3(TB), 0, (hipStream_t)stream, patch, Hm, Wm, orig, mask2d, offsets, lut, T,
                       H0, W0, h, w, feather_px, R, out);
    VV_CHECK_LAUNCH("vvt_paste_lut_composite");
    return VV_OK;
}
