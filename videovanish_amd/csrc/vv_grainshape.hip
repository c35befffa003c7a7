// Grain shape (videovanish_amd/grainshape.py): the companion of seam grain matching that fits the grain's size and adds
// shaped noise.  The rules are include/grainshape.h's; all arithmetic is integer.
//   vvn_ring_shape_stats         30 integer sums per frame over the pairs of horizontally and vertically adjacent counted pixels of the ring:
//                                per channel and axis the pairs, the lag-1 products and the squares of Immerkaer's operator on x and on y
//   vvn_paste_shaped_composite   vvb_paste_blend_composite (the membrane optional) whose noise went through [a_x, 1, a_x] (x) [a_y, 1, a_y]
// The statistic is vv_grain.hip's kernel on tiles that OVERLAP: the 64 x 32 tile of vv_ring_bits.h is stepped at a pitch of 63 x 31, a block owns
// the pixels of its first 63 columns and 31 rows, and the right and the lower neighbour of every owned pixel lie in the same tile with their
// ring bits, `near` bits and staged 3 x 3 -- no wider halo, and the rule does not know the tile.  L(x), L(y) and the "counts for c" bits of the
// tile go through LDS; the sums go 32-bit registers -> 32-bit wave reduction -> 64-bit LDS atomics -> one set of 64-bit global integer atomics
// per block, signed values as two's complement: integer adds modulo 2^64, so the result does not depend on the order.
// The paste tiles the FRAME (64 x 8 pixels per block): a block stages the white field s of its tile and a one-pixel halo in LDS (int16; 660
// hashes for 512 pixels in "luma", three planes in "rgb") and takes the nine taps from there; a block wholly outside the window copies orig.
#include <vector>
#include "vv_paste_px.h"
#include "vv_ring_bits.h"
#include "vv_wave_bytes.h"
#include "../../include/grainshape.h"
#pragma clang fp contract(off)

namespace {

using vvwave::wave_sum;
using vvring::TB;
using vvring::TW;
using vvring::TH;
using vvring::u64;
using vvpaste::window_px;
constexpr int NSUM = VVN_NSUM;
constexpr int PW = TW - 1, PH = TH - 1;          // the pitch of the tiles = the pixels a block owns
constexpr int SW = TW + 2, SH = TH + 2;          // the staged tile: a one-pixel halo
constexpr int SP = 68;                           // its row pitch in bytes
constexpr int ROWS_PER_THREAD = TH / (TB / 64);
static_assert(VVN_MAX_RING == vvring::MAX_RING, "the ring of vv_ring_bits.h");
static_assert(NSUM == 3 * 2 * 5, "n, Cx, Cy, Dx, Dy per channel and axis");
static_assert(SP >= SW && SP % 4 == 0, "pitch");
// |L| <= 8 * 255 = 2040.  A thread adds ROWS_PER_THREAD pairs per accumulator, a wave 64 threads: the signed products stay inside 31 bits,
// the sums of two squares inside 32 bits unsigned
static_assert(64ll * ROWS_PER_THREAD * 2040ll * 2040ll < (1ll << 31), "signed 32-bit pair sums up to the wave");
static_assert(64ull * ROWS_PER_THREAD * 2ull * 2040ull * 2040ull < (1ull << 32), "unsigned 32-bit square sums up to the wave");

// Immerkaer's operator, and max - min, on the 3 x 3 bytes round s (pitch SP): vv_grain.hip's
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

// grid: tiles_x * tiles_y * T blocks over tiles at the pitch PW x PH.  Every read of the mask and of orig is bounds-checked against the frame,
// every read of patch lies inside frame t's Hm x Wm image (0 <= xx < w, 0 <= yy < h), whatever the offsets hold; the only writes to memory are
// the atomics into sums[t].
__global__ __launch_bounds__(TB) void ring_shape_stats_kernel(const uint8_t* __restrict__ patch, int Hm, int Wm, const uint8_t* __restrict__ orig,
                                                              const uint8_t* __restrict__ mask, const int* __restrict__ offsets,
                                                              const uint8_t* __restrict__ lut, int H, int W, int h, int w, int r, int flat, int tiles_x,
                                                              int tiles_y, u64* __restrict__ sums) {
    __shared__ u64 rowbits[vvring::HALO_ROWS];   // scratch of the row pass
    __shared__ u64 own[TH];
    __shared__ u64 ringbits[TH];
    __shared__ u64 near[SH];
    __shared__ u64 tot[NSUM];
    __shared__ uint8_t xs[3][SH][SP], ys[3][SH][SP];      // staged pixel (i, j) = window pixel (tx0 + i - 1, ty0 + j - 1)
    __shared__ int16_t lxs[3][TH][TW], lys[3][TH][TW];    // L(x_c), L(y_c) of the tile's pixels that count for c
    __shared__ uint8_t cnt[TH][TW];                       // bit c: the pixel counts for channel c
    const int tile = (int)blockIdx.x % (tiles_x * tiles_y), t = (int)blockIdx.x / (tiles_x * tiles_y);
    const int tx0 = (tile % tiles_x) * PW, ty0 = (tile / tiles_x) * PH;        // the tile's origin in the window
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

    // every pixel of the tile: does it count for c (rules (a), (b), (c) of vvgrain.h), and its two responses
    for (int y = wave; y < TH; y += TB / 64) {                                 // wave-uniform
        const u64 bits = ringbits[y] & ~(near[y] | near[y + 1] | near[y + 2]);
        const int xx = tx0 + lane, yy = ty0 + y, X = ox + xx, Y = oy + yy;
        int counts = 0;
        if (((bits >> lane) & 1ull) && xx >= 1 && xx + 1 < w && yy >= 1 && yy + 1 < h && X >= 1 && X + 1 < W && Y >= 1 && Y + 1 < H) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint8_t* sx = &xs[c][y + 1][lane + 1];
                if (spread(sx) > flat) continue;
                counts |= 1 << c;
                lxs[c][y][lane] = (int16_t)noise_op(sx);
                lys[c][y][lane] = (int16_t)noise_op(&ys[c][y + 1][lane + 1]);
            }
        }
        cnt[y][lane] = (uint8_t)counts;
    }
    __syncthreads();

    // the pairs of the owned pixels: p = (lane, y), q = its right (axis 0) and its lower (axis 1) neighbour, both inside the tile
    int pairs[6], cx[6], cy[6];
    unsigned dx[6], dy[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) { pairs[i] = 0; cx[i] = 0; cy[i] = 0; dx[i] = 0; dy[i] = 0; }
    if (lane < PW) {
        for (int y = wave; y < PH; y += TB / 64) {
            const int mine = cnt[y][lane];
            if (!mine) continue;
            const int both[2] = {mine & cnt[y][lane + 1], mine & cnt[y + 1][lane]};
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    if (!((both[a] >> c) & 1)) continue;
                    const int qy = y + a, qx = lane + 1 - a;
                    const int lxp = lxs[c][y][lane], lyp = lys[c][y][lane], lxq = lxs[c][qy][qx], lyq = lys[c][qy][qx];
                    pairs[c * 2 + a] += 1;
                    cx[c * 2 + a] += lxp * lxq;
                    cy[c * 2 + a] += lyp * lyq;
                    dx[c * 2 + a] += (unsigned)(lxp * lxp + lxq * lxq);
                    dy[c * 2 + a] += (unsigned)(lyp * lyp + lyq * lyq);
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const unsigned n = wave_sum((unsigned)pairs[i]);
        if (!n) continue;                                                      // wave-uniform: every lane holds the sum
        // a signed sum that fits 32 bits is the two's complement of its wrapped unsigned sum; sign-extended it adds modulo 2^64
        const int scx = (int)wave_sum((unsigned)cx[i]), scy = (int)wave_sum((unsigned)cy[i]);
        const unsigned sdx = wave_sum(dx[i]), sdy = wave_sum(dy[i]);
        if (lane == 0) {
            atomicAdd(&tot[i * 5 + 0], (u64)n);
            atomicAdd(&tot[i * 5 + 1], (u64)(int64_t)scx);
            atomicAdd(&tot[i * 5 + 2], (u64)(int64_t)scy);
            atomicAdd(&tot[i * 5 + 3], (u64)sdx);
            atomicAdd(&tot[i * 5 + 4], (u64)sdy);
        }
    }
    __syncthreads();
    if (threadIdx.x < NSUM && tot[threadIdx.x]) atomicAdd(&sums[(int64_t)t * NSUM + threadIdx.x], tot[threadIdx.x]);
}

// ---- the paste ------------------------------------------------------------------------------------------------------------------------------
constexpr int QW = 64, QH = 8;                   // the paste's tile of the FRAME: one lane per column, QH / 4 rows per thread
constexpr int NW = QW + 2, NH = QH + 2;          // the staged white field: a one-pixel halo
constexpr int NP = NW + 1;                       // its row pitch in int16 (odd: rows start in different banks)
static_assert(QH % (TB / 64) == 0, "whole rows per wave");
static_assert(512ll * 512ll * 1020ll < (1ll << 31), "the nine taps in 32 bits");

// grid: tiles_x * tiles_y * T blocks over the H x W frame.  Every read and write of orig / out is at a pixel (x, y) of the frame, every read of
// patch / field at a pixel of the window (0 <= xx < w, 0 <= yy < h); the mask is read by feather_alpha, bounds-checked against the frame.
template <bool FIELD>
__global__ __launch_bounds__(TB) void paste_shaped_kernel(const uint8_t* __restrict__ patch, int Hm, int Wm, const uint8_t* __restrict__ orig,
                                                          const uint8_t* __restrict__ mask, const int* __restrict__ offsets, const uint8_t* __restrict__ lut,
                                                          const int16_t* __restrict__ field, int strength, const uint8_t* __restrict__ amp,
                                                          const int* __restrict__ taps, const int* __restrict__ frame_ids, int seed, int mode, int H, int W,
                                                          int h, int w, float feather, int R, int tiles_x, int tiles_y, uint8_t* __restrict__ out) {
    __shared__ int16_t ns[3][NH][NP];            // staged s (i, j) = frame pixel (x0 + i - 1, y0 + j - 1); plane c in "rgb", plane 0 in "luma"
    const int tile = (int)blockIdx.x % (tiles_x * tiles_y), t = (int)blockIdx.x / (tiles_x * tiles_y);
    const int x0 = (tile % tiles_x) * QW, y0 = (tile / tiles_x) * QH;
    const int oy = offsets[t * 2 + 0], ox = offsets[t * 2 + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = x0 + lane;
    const bool inside = x0 < ox + w && x0 + QW > ox && y0 < oy + h && y0 + QH > oy;       // block-uniform: the tile meets the window
    if (inside) {
        const int fid = frame_ids[t];
        for (int k = threadIdx.x; k < NW * NH; k += TB) {
            const int j = k / NW, i = k - j * NW;
            const u64 key = vvpaste::noise_key(seed, fid, H, W, x0 + i - 1, y0 + j - 1);          // signed coordinates, modulo 2^64
            if (mode) {
#pragma unroll
                for (int c = 0; c < 3; ++c) ns[c][j][i] = (int16_t)vvpaste::noise_sum(key * 3ull + (u64)c);
            } else {
                ns[0][j][i] = (int16_t)vvpaste::noise_sum(key);
            }
        }
        __syncthreads();
    }
    if (x >= W) return;
    const uint8_t* tab = lut + (int64_t)t * 3 * 256;
    const uint8_t* a = amp + (int64_t)t * 3 * 256;
    const int* tp = taps + t * 6;
    for (int ly = wave; ly < QH; ly += TB / 64) {
        const int y = y0 + ly;
        if (y >= H) break;
        const int64_t i = ((int64_t)t * H + y) * W + x;
        const uint8_t* o = orig + i * 3;
        uint8_t* d = out + i * 3;
        const int yy = y - oy, xx = x - ox;
        if (yy < 0 || yy >= h || xx < 0 || xx >= w) {
            d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
            continue;
        }
        uint8_t p[3];
        window_px(patch + (int64_t)t * Hm * Wm * 3, Hm, Wm, xx, yy, h, w, p);
        p[0] = tab[p[0]]; p[1] = tab[256 + p[1]]; p[2] = tab[512 + p[2]];
        const int av[3] = {a[p[0]], a[256 + p[1]], a[512 + p[2]]};             // the amplitude of the tabled value, as the grain statistic saw it
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int16_t* s = &ns[mode ? c : 0][ly + 1][lane + 1];
            const int ax = tp[c * 2 + 0], ay = tp[c * 2 + 1];
            const int up = ax * (s[-NP - 1] + s[-NP + 1]) + 256 * s[-NP];
            const int at = ax * (s[-1] + s[1]) + 256 * s[0];
            const int dn = ax * (s[NP - 1] + s[NP + 1]) + 256 * s[NP];
            const int u = (ay * (up + dn) + 256 * at + (1 << 15)) >> 16;
            const int g = (int)(((int64_t)av[c] * u * 5017 + (1 << 23)) >> 24);
            int v = p[c];
            if (FIELD) {
                const int m = field[(((int64_t)t * h + yy) * w + xx) * 3 + c];
                v = min(max(v + ((m * strength + (1 << 13)) >> 14), 0), 255);  // the membrane: vvblend.h's statement
            }
            p[c] = (uint8_t)min(max(v + g, 0), 255);
        }
        if (feather < 0.f) {
            d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
            continue;
        }
        const float alpha = vvpx::feather_alpha(mask + (int64_t)t * H * W, H, W, x, y, feather, R);
        vvpx::feather_blend(alpha, p, o, d);
    }
}

bool bad_sizes(int Hm, int Wm, int T, int H0, int W0, int h, int w) {
    return T <= 0 || H0 <= 0 || W0 <= 0 || Hm <= 0 || Wm <= 0 || h <= 0 || w <= 0 || h > H0 || w > W0;
}

}  // namespace

extern "C" int vvn_abi_version(void) { return VVN_ABI_VERSION; }
extern "C" const char* vvn_last_error(void) { return vv_last_error(); }

extern "C" int vvn_ring_shape_stats(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets,
                                    const uint8_t* lut, int T, int H0, int W0, int h, int w, int ring, int flat, int64_t* sums, void* stream) {
    if (!patch || !orig || !mask2d || !offsets || !lut || !sums || bad_sizes(Hm, Wm, T, H0, W0, h, w))
        VV_FAIL(VV_E_ARG, "vvn_ring_shape_stats: bad args (no null pointer, sizes > 0, h <= H0, w <= W0)");
    if (ring < 1 || ring > VVN_MAX_RING) VV_FAIL(VV_E_UNSUPPORTED, "vvn_ring_shape_stats: ring 1 .. %d is supported, not %d", VVN_MAX_RING, ring);
    if (flat < 0 || flat > 255) VV_FAIL(VV_E_UNSUPPORTED, "vvn_ring_shape_stats: flat 0 .. 255 is supported, not %d", flat);
    const int tiles_x = (w + PW - 1) / PW, tiles_y = (h + PH - 1) / PH;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * T;
    if (blocks > 0x7fffffff) VV_FAIL(VV_E_UNSUPPORTED, "vvn_ring_shape_stats: %lld tiles are more than one launch holds", (long long)blocks);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, (size_t)T * NSUM * sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vvn_ring_shape_stats: memset failed");
    hipLaunchKernelGGL(ring_shape_stats_kernel, dim3((unsigned)blocks), dim3(TB), 0, st, patch, Hm, Wm, orig, mask2d, offsets, lut, H0, W0, h, w, ring, flat,
                       tiles_x, tiles_y, (u64*)sums);
    VV_CHECK_LAUNCH("vvn_ring_shape_stats");
    return VV_OK;
}

extern "C" int vvn_paste_shaped_composite(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets,
                                          const uint8_t* lut, const int16_t* field, int strength_q8, const uint8_t* amp, const int* taps,
                                          const int* frame_ids, int seed, int mode, int T, int H0, int W0, int h, int w, float feather_px, uint8_t* out,
                                          void* stream) {
    if (!patch || !orig || !offsets || !lut || !amp || !taps || !frame_ids || !out || bad_sizes(Hm, Wm, T, H0, W0, h, w))
        VV_FAIL(VV_E_ARG, "vvn_paste_shaped_composite: bad args (no null pointer but field, sizes > 0, h <= H0, w <= W0)");
    if (seed < 0 || mode < 0 || mode > 1) VV_FAIL(VV_E_ARG, "vvn_paste_shaped_composite: seed >= 0 and mode 0 (luma) or 1 (rgb), not seed %d, mode %d", seed, mode);
    if (feather_px >= 0.f && !mask2d) VV_FAIL(VV_E_ARG, "vvn_paste_shaped_composite: the feathered composite needs mask2d");
    if (feather_px > 64.f) VV_FAIL(VV_E_UNSUPPORTED, "vvn_paste_shaped_composite: feather_px %.1f > 64", feather_px);
    if (strength_q8 < 0 || strength_q8 > 512) VV_FAIL(VV_E_UNSUPPORTED, "vvn_paste_shaped_composite: strength_q8 0 .. 512 is supported, not %d", strength_q8);
    const int tiles_x = (W0 + QW - 1) / QW, tiles_y = (H0 + QH - 1) / QH;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * T;
    if (blocks > 0x7fffffff) VV_FAIL(VV_E_UNSUPPORTED, "vvn_paste_shaped_composite: %lld tiles are more than one launch holds", (long long)blocks);
    hipStream_t st = (hipStream_t)stream;
    // the taps decide a refusal, so they are read before the launch: 24 T bytes, the one synchronisation
    std::vector<int> host((size_t)T * 6);
    if (hipMemcpyAsync(host.data(), taps, host.size() * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        VV_FAIL(VV_E_LAUNCH, "vvn_paste_shaped_composite: reading the taps failed");
    for (size_t i = 0; i < host.size(); ++i)
        if (host[i] < 0 || host[i] > VVN_MAX_TAP)
            VV_FAIL(VV_E_UNSUPPORTED, "vvn_paste_shaped_composite: a tap 0 .. %d is supported, not %d (frame %d)", VVN_MAX_TAP, host[i], (int)(i / 6));
    const int R = feather_px > 0.f ? (int)ceilf(feather_px) : 0;
    if (field)
        hipLaunchKernelGGL(paste_shaped_kernel<true>, dim3((unsigned)blocks), dim3(TB), 0, st, patch, Hm, Wm, orig, mask2d, offsets, lut, field, strength_q8, amp,
                           taps, frame_ids, seed, mode, H0, W0, h, w, feather_px, R, tiles_x, tiles_y, out);
    else
        hipLaunchKernelGGL(paste_shaped_kernel<false>, dim3((unsigned)blocks), dim3(TB), 0, st, patch, Hm, Wm, orig, mask2d, offsets, lut, field, strength_q8, amp,
                           taps, frame_ids, seed, mode, H0, W0, h, w, feather_px, R, tiles_x, tiles_y, out);
    VV_CHECK_LAUNCH("vvn_paste_shaped_composite");
    return VV_OK;
}
