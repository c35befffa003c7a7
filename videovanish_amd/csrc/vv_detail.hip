// Seam detail matching (videovanish_amd/detailmatch.py, infill.finish(detail=)): the two device steps around the host's
// per-frame fit.  The rules are include/detailmatch.h's; all arithmetic is integer.
//   vvd_ring_detail_stats   12 integer sums per frame over the structured part of the ring: per channel the count, sum D K, sum K K and
//                           sum D D, with D = H(y) - H(x), K = H(H(x)), H = 16 I - (the 3 x 3 binomial) * I
//   vvd_sharpen             out = the window's pixel plus amount / 256 of its high-pass, clamped to the 3 x 3 neighbourhood's range widened by
//                           `overshoot`; a frame with amount 0 is the window's pixel itself (a copy, or the resize)
// Both use the 64 x 32 tile of vv_grain.hip, 256 threads, one lane per column.  The ring bits are vv_ring_bits.h's; the 5 x 5 gate ("all 25
// pixels inside the window and the frame and unmasked") needs the mask at radius 2, which ring_bits<true>'s `near` (radius 1) does not give, so
// this unit makes its own row words over the tile plus a two-pixel halo.  A tile that holds a counted pixel stages x (resized) with a two-pixel
// halo and y with a one-pixel halo in LDS, planar, and H(x) of the tile plus one pixel as int16, so that K is nine LDS reads.  The sums go 64-bit
// registers -> wave_sum64 -> 64-bit LDS atomics -> one 64-bit global atomic per block and quantity: integer adds in any order.
#include "vv_paste_px.h"
#include "vv_ring_bits.h"
#include "vv_wave_bytes.h"
#include "../../include/detailmatch.h"
#pragma clang fp contract(off)

namespace {

using vvwave::store_px;
using vvwave::wave_sum64;
using vvring::TB;
using vvring::TW;
using vvring::TH;
using vvring::u64;
using vvpaste::window_px;
constexpr int NSUM = VVD_NSUM, NQ = VVD_NQ;
constexpr int XW = TW + 4, XH = TH + 4, XP = 72;     // x of the statistic: a two-pixel halo; its row pitch in bytes
constexpr int YW = TW + 2, YH = TH + 2, YP = 68;     // y, H(x), and x of the apply: a one-pixel halo; the pitch in elements
static_assert(VVD_MAX_RING == vvring::MAX_RING, "the ring of vv_ring_bits.h");
static_assert(NSUM == 3 * NQ && NQ == 4, "n, DK, KK, DD per channel");
static_assert(XP >= XW && XP % 4 == 0 && YP >= YW && YP % 4 == 0, "pitch");
static_assert(TW == 64 && TW % 4 == 0 && (TW / 4) * TH == 2 * TB, "one lane per column; two 4-pixel units per thread");
static_assert(255 * 12 == 3060 && 3060 < 32768 && 3060 * 24 == 73440, "|H| <= 3060 fits int16, |K| <= 73440");
static_assert((u64)VVD_MAX_PIXELS * 73440ull * 73440ull < (1ull << 63), "sum K K of a frame");
static_assert(4096 * 255 + VVD_MAX_AMOUNT * 3060 + 2048 < (1 << 23), "the apply in 32 bits");

// sum of B .* I over the 3 x 3 round s (pitch P); H(I) = 16 s[0] - binomial
template <typename E, int P> __device__ __forceinline__ int binomial(const E* s) {
    const int corners = s[-P - 1] + s[-P + 1] + s[P - 1] + s[P + 1];
    const int edges = s[-P] + s[-1] + s[1] + s[P];
    return corners + 2 * edges + 4 * s[0];
}
template <typename E, int P> __device__ __forceinline__ int highpass(const E* s) { return 16 * s[0] - binomial<E, P>(s); }
// min and max over the 3 x 3 bytes round s
template <int P> __device__ __forceinline__ void range3(const uint8_t* s, int& lo, int& hi) {
    lo = 255; hi = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int v = s[dy * P + dx];
            lo = min(lo, v); hi = max(hi, v);
        }
}

// grid: tiles_x * tiles_y * T blocks, as ring_grain_stats_kernel of vv_grain.hip.  Every read of the mask and of orig is bounds-checked against
// the frame, every read of patch lies inside frame t's Hm x Wm image (0 <= xx < w, 0 <= yy < h), whatever the offsets hold; the only writes to
// memory are the atomics into sums[t].
__global__ __launch_bounds__(TB) void ring_detail_stats_kernel(const uint8_t* __restrict__ patch, int Hm, int Wm, const uint8_t* __restrict__ orig,
                                                               const uint8_t* __restrict__ mask, const int* __restrict__ offsets, int H, int W, int h, int w,
                                                               int r, int edge, int tiles_x, int tiles_y, u64* __restrict__ sums) {
    __shared__ u64 rowbits[vvring::HALO_ROWS];   // scratch of the row pass
    __shared__ u64 own[TH];                      // tile row y: bit px = the pixel's own mask
    __shared__ u64 ringbits[TH];                 // tile row y: bit px = the pixel belongs to the ring
    __shared__ u64 wide[XH];                     // tile row j - 2: bit px = a pixel of columns px - 2 .. px + 2 is masked or outside the window or the frame
    __shared__ u64 tot[NSUM];
    __shared__ uint8_t xs[3][XH][XP];            // staged pixel (i, j) = window pixel (tx0 + i - 2, ty0 + j - 2)
    __shared__ uint8_t ys[3][YH][YP];            // staged pixel (i, j) = frame pixel of window pixel (tx0 + i - 1, ty0 + j - 1)
    __shared__ int16_t hx[3][YH][YP];            // H(x) at window pixel (tx0 + i - 1, ty0 + j - 1)
    const int tile = (int)blockIdx.x % (tiles_x * tiles_y), t = (int)blockIdx.x / (tiles_x * tiles_y);
    const int tx0 = (tile % tiles_x) * TW, ty0 = (tile / tiles_x) * TH;        // the tile's origin in the window
    const int oy = offsets[t * 2 + 0], ox = offsets[t * 2 + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t* m = mask + (int64_t)t * H * W;
    if (threadIdx.x < NSUM) tot[threadIdx.x] = 0;
    vvring::ring_bits<false>(m, H, W, oy, ox, tx0, ty0, h, w, r, rowbits, own, ringbits, nullptr);

    u64 anyring = 0;
#pragma unroll 8
    for (int y = 0; y < TH; ++y) anyring |= ringbits[y];
    if (!anyring) return;                                                      // block-uniform: every thread read the same words

    // the 5 x 5 gate's row words: halo row j is window row ty0 + j - 2, halo column i is window column tx0 + i - 2, i < TW + 4: two ballots
    for (int j = wave; j < XH; j += TB / 64) {                                 // wave-uniform
        const int yy = ty0 + j - 2, Y = oy + yy;
        const bool rowin = yy >= 0 && yy < h && Y >= 0 && Y < H;
        const int xa = tx0 + lane - 2, xb = xa + 64, Xa = ox + xa, Xb = ox + xb;
        const bool b0 = !(rowin && xa >= 0 && xa < w && Xa >= 0 && Xa < W) || m[(int64_t)Y * W + Xa] != 0;
        const bool b1 = lane < 4 && (!(rowin && xb >= 0 && xb < w && Xb >= 0 && Xb < W) || m[(int64_t)Y * W + Xb] != 0);
        const u64 lo = __ballot(b0), hi = __ballot(b1);
        u64 v = lo;
#pragma unroll
        for (int k = 1; k <= 4; ++k) v |= (lo >> k) | (hi << (64 - k));        // bit px: halo columns px .. px + 4
        if (lane == 0) wide[j] = v;
    }
    __syncthreads();
    u64 anygate = 0;
    for (int y = 0; y < TH; ++y) anygate |= ringbits[y] & ~(wide[y] | wide[y + 1] | wide[y + 2] | wide[y + 3] | wide[y + 4]);
    if (!anygate) return;                                                      // block-uniform

    const uint8_t* src = patch + (int64_t)t * Hm * Wm * 3;
    for (int k = threadIdx.x; k < XW * XH; k += TB) {
        const int j = k / XW, i = k - j * XW;
        const int xx = tx0 + i - 2, yy = ty0 + j - 2, X = ox + xx, Y = oy + yy;
        uint8_t p[3] = {0, 0, 0}, q[3] = {0, 0, 0};                            // outside the window or the frame: never a tap of a counted pixel
        const bool in = xx >= 0 && xx < w && yy >= 0 && yy < h && X >= 0 && X < W && Y >= 0 && Y < H;
        if (in) {
            window_px(src, Hm, Wm, xx, yy, h, w, p);
            const uint8_t* o = orig + (((int64_t)t * H + Y) * W + X) * 3;
            q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
        }
        const bool iny = i >= 1 && i <= YW && j >= 1 && j <= YH;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            xs[c][j][i] = p[c];
            if (iny) ys[c][j - 1][i - 1] = q[c];
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < YW * YH; k += TB) {
        const int j = k / YW, i = k - j * YW;
#pragma unroll
        for (int c = 0; c < 3; ++c) hx[c][j][i] = (int16_t)highpass<uint8_t, XP>(&xs[c][j + 1][i + 1]);
    }
    __syncthreads();

    u64 acc[NSUM];
#pragma unroll
    for (int i = 0; i < NSUM; ++i) acc[i] = 0;
    bool any = false;
    for (int y = wave; y < TH; y += TB / 64) {                                 // wave-uniform
        const u64 bits = ringbits[y] & ~(wide[y] | wide[y + 1] | wide[y + 2] | wide[y + 3] | wide[y + 4]);
        if (!bits) continue;
        any = true;
        if (!((bits >> lane) & 1ull)) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int lo, hi;
            range3<XP>(&xs[c][y + 2][lane + 2], lo, hi);
            if (hi - lo < edge) continue;
            const int16_t* g = &hx[c][y + 1][lane + 1];
            const int64_t K = highpass<int16_t, YP>(g);
            const int64_t D = highpass<uint8_t, YP>(&ys[c][y + 1][lane + 1]) - (int)g[0];
            acc[c * NQ + 0] += 1ull;
            acc[c * NQ + 1] += (u64)(D * K);                                   // signed, modulo 2^64: the sum is the two's complement of the signed sum
            acc[c * NQ + 2] += (u64)(K * K);
            acc[c * NQ + 3] += (u64)(D * D);
        }
    }
    if (any) {                                                                 // wave-uniform: `any` was set from LDS words every lane read
#pragma unroll
        for (int i = 0; i < NSUM; ++i) {
            const u64 s = wave_sum64(acc[i]);
            if (lane == 0 && s) atomicAdd(&tot[i], s);
        }
    }
    __syncthreads();
    if (threadIdx.x < NSUM && tot[threadIdx.x]) atomicAdd(&sums[(int64_t)t * NSUM + threadIdx.x], tot[threadIdx.x]);
}

// grid: tiles_x * tiles_y * T blocks.  VEC: a thread owns two units of 4 adjacent pixels (w % 4 == 0 and a 4-byte aligned out: one 12-byte store);
// otherwise its column in 8 rows.  Every read of patch lies inside frame t's image (the coordinates are clamped to the window), every write
// inside out[t]'s h x w.
template <bool VEC>
__global__ __launch_bounds__(TB) void sharpen_kernel(const uint8_t* __restrict__ patch, int Hm, int Wm, const int* __restrict__ amount, int h, int w,
                                                     int overshoot, int tiles_x, int tiles_y, uint8_t* __restrict__ out) {
    constexpr int P = VEC ? 4 : 1, UNITS = TW / P, PER = TW * TH / P / TB;
    __shared__ uint8_t xs[3][YH][YP];            // staged pixel (i, j) = window pixel (tx0 + i - 1, ty0 + j - 1), clamped to the window
    const int tile = (int)blockIdx.x % (tiles_x * tiles_y), t = (int)blockIdx.x / (tiles_x * tiles_y);
    const int tx0 = (tile % tiles_x) * TW, ty0 = (tile / tiles_x) * TH;
    const int a = min(max(amount[t], -VVD_MAX_AMOUNT), VVD_MAX_AMOUNT);        // block-uniform
    const uint8_t* src = patch + (int64_t)t * Hm * Wm * 3;
    uint8_t* dst = out + (int64_t)t * h * w * 3;
    if (a != 0) {
        for (int k = threadIdx.x; k < YW * YH; k += TB) {
            const int j = k / YW, i = k - j * YW;
            uint8_t p[3];
            window_px(src, Hm, Wm, min(max(tx0 + i - 1, 0), w - 1), min(max(ty0 + j - 1, 0), h - 1), h, w, p);
#pragma unroll
            for (int c = 0; c < 3; ++c) xs[c][j][i] = p[c];
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int k = u * TB + (int)threadIdx.x, py = k / UNITS, px = (k - py * UNITS) * P;
        const int xx = tx0 + px, yy = ty0 + py;
        if (xx >= w || yy >= h) continue;                                      // VEC: w % 4 == 0, a unit is inside or outside as a whole
        unsigned v[3 * P];
#pragma unroll
        for (int e = 0; e < P; ++e) {
            if (a == 0) {
                uint8_t p[3];
                window_px(src, Hm, Wm, xx + e, yy, h, w, p);
                v[3 * e] = p[0]; v[3 * e + 1] = p[1]; v[3 * e + 2] = p[2];
                continue;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint8_t* s = &xs[c][py + 1][px + e + 1];
                int lo, hi;
                range3<YP>(s, lo, hi);
                const int x = s[0], sharp = (4096 * x + a * highpass<uint8_t, YP>(s) + 2048) >> 12;
                v[3 * e + c] = (unsigned)min(max(min(max(sharp, lo - overshoot), hi + overshoot), 0), 255);
            }
        }
        store_px<VEC>(dst + ((int64_t)yy * w + xx) * 3, v);
    }
}

// 0 = fine; the tile counts of an h x w window over T frames
int tiles_of(const char* who, int T, int h, int w, int* tiles_x, int* tiles_y) {
    if ((int64_t)h * w > VVD_MAX_PIXELS) VV_FAIL(VV_E_UNSUPPORTED, "%s: h * w <= 2^24 is supported, not %d x %d", who, h, w);
    *tiles_x = (w + TW - 1) / TW; *tiles_y = (h + TH - 1) / TH;
    if ((int64_t)*tiles_x * *tiles_y * T > 0x7fffffff)
        VV_FAIL(VV_E_UNSUPPORTED, "%s: %lld tiles are more than one launch holds", who, (long long)((int64_t)*tiles_x * *tiles_y * T));
    return VV_OK;
}

}  // namespace

extern "C" int vvd_abi_version(void) { return VVD_ABI_VERSION; }
extern "C" const char* vvd_last_error(void) { return vv_last_error(); }

extern "C" int vvd_ring_detail_stats(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets, int T, int H0,
                                     int W0, int h, int w, int ring, int edge, int64_t* sums, void* stream) {
    if (!patch || !orig || !mask2d || !offsets || !sums || T <= 0 || H0 <= 0 || W0 <= 0 || Hm <= 0 || Wm <= 0 || h <= 0 || w <= 0 || h > H0 || w > W0)
        VV_FAIL(VV_E_ARG, "vvd_ring_detail_stats: bad args (no null pointer, sizes > 0, h <= H0, w <= W0)");
    if (ring < 1 || ring > VVD_MAX_RING) VV_FAIL(VV_E_UNSUPPORTED, "vvd_ring_detail_stats: ring 1 .. %d is supported, not %d", VVD_MAX_RING, ring);
    if (edge < 0 || edge > VVD_MAX_EDGE) VV_FAIL(VV_E_UNSUPPORTED, "vvd_ring_detail_stats: edge 0 .. %d is supported, not %d", VVD_MAX_EDGE, edge);
    int tiles_x, tiles_y;
    const int rc = tiles_of("vvd_ring_detail_stats", T, h, w, &tiles_x, &tiles_y);
    if (rc != VV_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, (size_t)T * NSUM * sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vvd_ring_detail_stats: memset failed");
    hipLaunchKernelGGL(ring_detail_stats_kernel, dim3((unsigned)(tiles_x * tiles_y * T)), dim3(TB), 0, st, patch, Hm, Wm, orig, mask2d, offsets, H0, W0, h, w,
                       ring, edge, tiles_x, tiles_y, (u64*)sums);
    VV_CHECK_LAUNCH("vvd_ring_detail_stats");
    return VV_OK;
}

extern "C" int vvd_sharpen(const uint8_t* patch, int Hm, int Wm, const int* amount, int T, int h, int w, int overshoot, uint8_t* out, void* stream) {
    if (!patch || !amount || !out || out == patch || T <= 0 || Hm <= 0 || Wm <= 0 || h <= 0 || w <= 0)
        VV_FAIL(VV_E_ARG, "vvd_sharpen: bad args (no null pointer, sizes > 0, out is not patch)");
    if (overshoot < 0 || overshoot > VVD_MAX_OVERSHOOT)
        VV_FAIL(VV_E_UNSUPPORTED, "vvd_sharpen: overshoot 0 .. %d is supported, not %d", VVD_MAX_OVERSHOOT, overshoot);
    int tiles_x, tiles_y;
    const int rc = tiles_of("vvd_sharpen", T, h, w, &tiles_x, &tiles_y);
    if (rc != VV_OK) return rc;
    const dim3 grid((unsigned)(tiles_x * tiles_y * T));
    if (w % 4 == 0 && (uintptr_t)out % 4 == 0)
        hipLaunchKernelGGL(sharpen_kernel<true>, grid, dim3(TB), 0, (hipStream_t)stream, patch, Hm, Wm, amount, h, w, overshoot, tiles_x, tiles_y, out);
    else
        hipLaunchKernelGGL(sharpen_kernel<false>, grid, dim3(TB), 0, (hipStream_t)stream, patch, Hm, Wm, amount, h, w, overshoot, tiles_x, tiles_y, out);
    VV_CHECK_LAUNCH("vvd_sharpen");
    return VV_OK;
}
