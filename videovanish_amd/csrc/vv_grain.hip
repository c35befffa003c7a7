// Seam grain matching (videovanish_amd/grainmatch.py): the two device steps around the host's per-frame fit.
//   vvg_ring_grain_stats        36 integer sums per frame over the flat part of the ring: per channel and brightness band the count and the
//                               squared responses of Immerkaer's noise operator on the model's pixels x and on the original pixels y
//   vvg_paste_grain_composite   vvt_paste_lut_composite with stateless noise, scaled by a per-frame, per-channel, per-value table, added to
//                               every pasted byte before the feather
// The ring bits are vv_ring_bits.h's, the statement vv_tone.hip uses; the same row pass gives "a mask pixel in the 3 x 3 neighbourhood" from
// the mask's own bits at radius 1.  A tile that holds a ring pixel stages x (resized, looked up) and y with a one-pixel halo in LDS, planar,
// so each byte is resized, looked up and read from memory once and the nine taps are LDS reads.  The sums go 32-bit registers -> 32-bit wave
// reduction -> 64-bit LDS atomics -> one set of 64-bit global integer atomics per block: integer adds, so the result does not depend on the
// order.  The band is selected by unrolled compares, every accumulator index is a constant.  The per-pixel arithmetic (resize, feather) is
// vv_image_px.h, the window's pixel and the noise vv_paste_px.h (shared with vv_blend.hip), so a zero amplitude gives vvt_paste_lut_composite's bytes.
#include "vv_paste_px.h"
#include "vv_ring_bits.h"
#include "vv_wave_bytes.h"
#include "../../include/vvgrain.h"
#pragma clang fp contract(off)

namespace {

using vvwave::wave_sum;
using vvring::TB;
using vvring::TW;
using vvring::TH;
using vvring::u64;
using vvpaste::window_px;
constexpr int NSUM = VVG_NSUM, BANDS = VVG_BANDS;
constexpr int SW = TW + 2, SH = TH + 2;          // the staged tile: a one-pixel halo
constexpr int SP = 68;                           // its row pitch in bytes
constexpr int ROWS_PER_THREAD = TH / (TB / 64);
static_assert(VVG_MAX_RING == vvring::MAX_RING, "the ring of vv_ring_bits.h");
static_assert(NSUM == 3 * BANDS * 3 && BANDS == 4, "n, Sx, Sy per channel and band; band = value >> 6");
static_assert(SP >= SW && SP % 4 == 0, "pitch");
// |L| <= 8 * 255 = 2040; a thread adds ROWS_PER_THREAD squares, a wave 64 threads: the 32-bit wave sum holds
static_assert(64ull * ROWS_PER_THREAD * 2040ull * 2040ull < (1ull << 32), "32-bit sums up to the wave");

// Immerkaer's operator, and max - min, on the 3 x 3 bytes round s (pitch SP)
__device__ __forceinline__ int noise_op(const uint8_t* s) {
    const int corners = s[-SP - 1] + s[-SP + 1] + s[SP - 1] + s[SP + 1];
    const int edges = s[-SP] + s[-1] + s[1] + s[SP];
    return corners - 2 * edges + 4 * s[0];
}
__device__ __forceinline__ int spread(const uint8_t* s) {
    int lo = 255, hi = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int v = s[dy * SP + dx];
            lo = min(lo, v); hi = max(hi, v);
        }
    return hi - lo;
}

// grid: tiles_x * tiles_y * T blocks, as ring_stats_kernel of vv_tone.hip.  Every read of the mask and of orig is bounds-checked against the
// frame, every read of patch lies inside frame t's Hm x Wm image (0 <= xx < w, 0 <= yy < h), whatever the offsets hold; the only writes to
// memory are the atomics into sums[t].
__global__ __launch_bounds__(TB) void ring_grain_stats_kernel(const uint8_t* __restrict__ patch, int Hm, int Wm, const uint8_t* __restrict__ orig,
                                                              const uint8_t* __restrict__ mask, const int* __restrict__ offsets,
                                                              const uint8_t* __restrict__ lut, int H, int W, int h, int w, int r, int flat, int tiles_x,
                                                              int tiles_y, u64* __restrict__ sums) {
    __shared__ u64 rowbits[vvring::HALO_ROWS];   // scratch of the row pass
    __shared__ u64 own[TH];                      // tile row y: bit px = the pixel's own mask
    __shared__ u64 ringbits[TH];                 // tile row y: bit px = the pixel belongs to the ring
    __shared__ u64 near[SH];                     // tile row j - 1: bit px = a mask pixel in columns px - 1 .. px + 1
    __shared__ u64 tot[NSUM];
    __shared__ uint8_t xs[3][SH][SP], ys[3][SH][SP];      // staged pixel (i, j) = window pixel (tx0 + i - 1, ty0 + j - 1)
    const int tile = (int)blockIdx.x % (tiles_x * tiles_y), t = (int)blockIdx.x / (tiles_x * tiles_y);
    const int tx0 = (tile % tiles_x) * TW, ty0 = (tile / tiles_x) * TH;        // the tile's origin in the window
    const int oy = offsets[t * 2 + 0], ox = offsets[t * 2 + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < NSUM) tot[threadIdx.x] = 0;
    vvring::ring_bits<true>(mask + (int64_t)t * H * W, H, W, oy, ox, tx0, ty0, h, w, r, rowbits, own, ringbits, near);

    u64 anyring = 0;
#pragma unroll 8
    for (int y = 0; y < TH; ++y) anyring |= ringbits[y];
    if (!anyring) return;                                                      // block-uniform: every thread read the same words

    const uint8_t* src = patch + (int64_t)t * Hm * Wm * 3;
    const uint8_t* tab = lut + (int64_t)t * 3 * 256;
    for (int k = threadIdx.x; k < SW * SH; k += TB) {
        const int j = k / SW, i = k - j * SW;
        const int xx = tx0 + i - 1, yy = ty0 + j - 1, X = ox + xx, Y = oy + yy;
        uint8_t p[3] = {0, 0, 0}, q[3] = {0, 0, 0};                            // outside the window or the frame: never a tap of a counted pixel
        if (xx >= 0 && xx < w && yy >= 0 && yy < h && X >= 0 && X < W && Y >= 0 && Y < H) {
            window_px(src, Hm, Wm, xx, yy, h, w, p);
            p[0] = tab[p[0]]; p[1] = tab[256 + p[1]]; p[2] = tab[512 + p[2]];
            const uint8_t* o = orig + (((int64_t)t * H + Y) * W + X) * 3;
            q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { xs[c][j][i] = p[c]; ys[c][j][i] = q[c]; }
    }
    __syncthreads();

    unsigned acc[NSUM];
#pragma unroll
    for (int i = 0; i < NSUM; ++i) acc[i] = 0;
    bool any = false;
    for (int y = wave; y < TH; y += TB / 64) {                                 // wave-uniform
        const u64 bits = ringbits[y] & ~(near[y] | near[y + 1] | near[y + 2]);
        if (!bits) continue;
        any = true;
        const int xx = tx0 + lane, yy = ty0 + y, X = ox + xx, Y = oy + yy;
        // (b): the 3 x 3 neighbourhood inside the window and the frame (unmasked: `near`)
        if (!((bits >> lane) & 1ull) || xx < 1 || xx + 1 >= w || yy < 1 || yy + 1 >= h || X < 1 || X + 1 >= W || Y < 1 || Y + 1 >= H) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint8_t* sx = &xs[c][y + 1][lane + 1];
            if (spread(sx) > flat) continue;
            const int lx = noise_op(sx), ly = noise_op(&ys[c][y + 1][lane + 1]);
            const unsigned band = sx[0] >> 6, lx2 = (unsigned)(lx * lx), ly2 = (unsigned)(ly * ly);
#pragma unroll
            for (int b = 0; b < BANDS; ++b) {
                const bool in = band == (unsigned)b;
                acc[(c * BANDS + b) * 3 + 0] += in ? 1u : 0u;
                acc[(c * BANDS + b) * 3 + 1] += in ? lx2 : 0u;
                acc[(c * BANDS + b) * 3 + 2] += in ? ly2 : 0u;
            }
        }
    }
    if (any) {                                                                 // wave-uniform: `any` was set from LDS words every lane read
#pragma unroll
        for (int i = 0; i < NSUM; ++i) {
            const unsigned s = wave_sum(acc[i]);
            if (lane == 0 && s) atomicAdd(&tot[i], (u64)s);
        }
    }
    __syncthreads();
    if (threadIdx.x < NSUM && tot[threadIdx.x]) atomicAdd(&sums[(int64_t)t * NSUM + threadIdx.x], tot[threadIdx.x]);
}

// pixel (x, y) of frame t, as paste_lut_kernel of vv_tone.hip; inside the window the looked-up bytes get their grain before the feather
__global__ __launch_bounds__(TB) void paste_grain_kernel(const uint8_t* __restrict__ patch, int Hm, int Wm, const uint8_t* __restrict__ orig,
                                                         const uint8_t* __restrict__ mask, const int* __restrict__ offsets, const uint8_t* __restrict__ lut,
                                                         const uint8_t* __restrict__ amp, const int* __restrict__ frame_ids, int seed, int mode, int T,
                                                         int H, int W, int h, int w, float feather, int R, uint8_t* __restrict__ out) {
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
    const uint8_t* a = amp + (int64_t)t * 3 * 256;
    const int av[3] = {a[p[0]], a[256 + p[1]], a[512 + p[2]]};
    int g[3];
    vvpaste::grain_px(vvpaste::noise_key(seed, frame_ids[t], H, W, x, y), mode, av, g);
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = (uint8_t)min(max((int)p[c] + g[c], 0), 255);
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

extern "C" int vvg_abi_version(void) { return VVG_ABI_VERSION; }
extern "C" const char* vvg_last_error(void) { return vv_last_error(); }

extern "C" int vvg_ring_grain_stats(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets,
                                    const uint8_t* lut, int T, int H0, int W0, int h, int w, int ring, int flat, int64_t* sums, void* stream) {
    if (!patch || !orig || !mask2d || !offsets || !lut || !sums || bad_sizes(Hm, Wm, T, H0, W0, h, w))
        VV_FAIL(VV_E_ARG, "vvg_ring_grain_stats: bad args (no null pointer, sizes > 0, h <= H0, w <= W0)");
    if (ring < 1 || ring > VVG_MAX_RING) VV_FAIL(VV_E_UNSUPPORTED, "vvg_ring_grain_stats: ring 1 .. %d is supported, not %d", VVG_MAX_RING, ring);
    if (flat < 0 || flat > 255) VV_FAIL(VV_E_UNSUPPORTED, "vvg_ring_grain_stats: flat 0 .. 255 is supported, not %d", flat);
    const int tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * T;
    if (blocks > 0x7fffffff) VV_FAIL(VV_E_UNSUPPORTED, "vvg_ring_grain_stats: %lld tiles are more than one launch holds", (long long)blocks);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, (size_t)T * NSUM * sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vvg_ring_grain_stats: memset failed");
    hipLaunchKernelGGL(ring_grain_stats_kernel, dim3((unsigned)blocks), dim3(TB), 0, st, patch, Hm, Wm, orig, mask2d, offsets, lut, H0, W0, h, w, ring, flat,
                       tiles_x, tiles_y, (u64*)sums);
    VV_CHECK_LAUNCH("vvg_ring_grain_stats");
    return VV_OK;
}

extern "C" int vvg_paste_grain_composite(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets,
                                         const uint8_t* lut, const uint8_t* amp, const int* frame_ids, int seed, int mode, int T, int H0, int W0, int h,
                                         int w, float feather_px, uint8_t* out, void* stream) {
    if (!patch || !orig || !offsets || !lut || !amp || !frame_ids || !out || bad_sizes(Hm, Wm, T, H0, W0, h, w))
        VV_FAIL(VV_E_ARG, "vvg_paste_grain_composite: bad args (no null pointer, sizes > 0, h <= H0, w <= W0)");
    if (seed < 0 || mode < 0 || mode > 1) VV_FAIL(VV_E_ARG, "vvg_paste_grain_composite: seed >= 0 and mode 0 (luma) or 1 (rgb), not seed %d, mode %d", seed, mode);
    if (feather_px >= 0.f && !mask2d) VV_FAIL(VV_E_ARG, "vvg_paste_grain_composite: the feathered composite needs mask2d");
    if (feather_px > 64.f) VV_FAIL(VV_E_UNSUPPORTED, "vvg_paste_grain_composite: feather_px %.1f > 64", feather_px);
    const int R = feather_px > 0.f ? (int)ceilf(feather_px) : 0;
    const int64_t n = (int64_t)T * H0 * W0;
    hipLaunchKernelGGL(paste_grain_kernel, dim3((unsigned)((n + TB - 1) / TB)), dim3(TB), 0, (hipStream_t)stream, patch, Hm, Wm, orig, mask2d, offsets, lut,
                       amp, frame_ids, seed, mode, T, H0, W0, h, w, feather_px, R, out);
    VV_CHECK_LAUNCH("vvg_paste_grain_composite");
    return VV_OK;
}
