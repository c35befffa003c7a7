// The ring round the mask as bits, the one statement vv_tone.hip (seam tone matching) and vv_grain.hip (seam grain matching) share: a pixel of
// the window belongs to the ring when it lies inside the window and the frame, is unmasked and has a mask pixel of the frame within `r` pixels
// (a box; include/vvtone.h).  A block of TB threads owns a TW x TH tile of the window and reads the mask of the tile plus a halo of r pixels,
// one row per wave step: two ballots turn the row into 128 bits, a log-step shift-OR ORs every run of 2 r + 1 bits (the row pass: seven 128-bit
// shift-ORs whatever the ring), and TH threads OR the 2 r + 1 row words above and below their row (the column pass: 2 r + 1 LDS reads per tile
// ROW, not per pixel); the window and the frame then clip the tile.  Nothing is searched per pixel.
#pragma once
#include "vv_common.h"

namespace vvring {

constexpr int TB = 256;                          // threads per block: 4 waves
constexpr int TW = 64, TH = 32;                  // the tile: one lane per column, TH * TW / TB = 8 rows per thread
constexpr int MAX_RING = 32;                     // VVT_MAX_RING / VVG_MAX_RING
constexpr int HALO_ROWS = TH + 2 * MAX_RING;
static_assert(TW + 2 * MAX_RING <= 128, "a halo row is two ballots");
typedef unsigned long long u64;

// (hi:lo) >> k, 0 < k < 64
__device__ __forceinline__ void shr128(u64& hi, u64& lo, int k) {
    lo = (lo >> k) | (hi << (64 - k));
    hi >>= k;
}

// Called by every thread of the block; tile origin (tx0, ty0) in the h x w window at (oy, ox) of the H x W frame whose mask is m; 1 <= r <=
// MAX_RING.  LDS out: own[y] bit px = the pixel's own mask, ringbits[y] bit px = the pixel belongs to the ring (y < TH), and with NEAR
// near[j] bit px = some mask pixel in columns px - 1 .. px + 1 of tile row j - 1 (j < TH + 2; rows outside the frame: 0).  rowbits
// [HALO_ROWS] is scratch.  Ends with a barrier.  Every read of the mask is bounds-checked against the frame, whatever the offsets hold.
template <bool NEAR>
__device__ __forceinline__ void ring_bits(const uint8_t* __restrict__ m, int H, int W, int oy, int ox, int tx0, int ty0, int h, int w, int r, u64* rowbits,
                                          u64* own, u64* ringbits, u64* near) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // row pass.  Halo row j is frame row oy + ty0 + j - r, halo column i is frame column ox + tx0 + i - r; outside the frame: no mask
    const int rows = TH + 2 * r, n = 2 * r + 1;
    for (int j = wave; j < rows; j += TB / 64) {                               // wave-uniform
        const int Y = oy + ty0 + j - r;
        const int X0 = ox + tx0 + lane - r, X1 = X0 + 64;
        const bool rowin = Y >= 0 && Y < H;
        const bool b0 = rowin && X0 >= 0 && X0 < W && m[(int64_t)Y * W + X0] != 0;
        const bool b1 = rowin && lane < 2 * r && X1 >= 0 && X1 < W && m[(int64_t)Y * W + X1] != 0;
        u64 lo = __ballot(b0), hi = __ballot(b1);
        if (j >= r && j < r + TH) {
            u64 a = hi, b = lo;
            shr128(a, b, r);
            if (lane == 0) own[j - r] = b;
        }
        if (NEAR && j >= r - 1 && j <= r + TH) {                               // columns px - 1 .. px + 1: halo columns px + r - 1 .. px + r + 1
            u64 a = hi, b = lo, c = hi, d = lo;
            shr128(a, b, 1);
            shr128(c, d, 2);
            a |= c | hi; b |= d | lo;
            if (r > 1) shr128(a, b, r - 1);
            if (lane == 0) near[j - (r - 1)] = b;
        }
        // OR of the n bits from each position on: doubling steps while they fit, one last step for the rest
        int cover = 1;
        for (; cover * 2 <= n; cover *= 2) {
            u64 a = hi, b = lo;
            shr128(a, b, cover);
            hi |= a; lo |= b;
        }
        if (n > cover) {
            u64 a = hi, b = lo;
            shr128(a, b, n - cover);
            hi |= a; lo |= b;
        }
        if (lane == 0) rowbits[j] = lo;
    }
    __syncthreads();

    // column pass: tile row y is halo row y + r and sees halo rows y .. y + 2 r; then the window and the frame clip the tile
    if (threadIdx.x < TH) {
        const int y = threadIdx.x;
        u64 v = 0;
        for (int k = 0; k < n; ++k) v |= rowbits[y + k];
        const int yy = ty0 + y, Y = oy + yy;
        u64 cols = 0;
        if (yy < h && Y >= 0 && Y < H) {
            int lo_x = max(0, -(ox + tx0)), hi_x = min(TW, min(w - tx0, W - (ox + tx0)));          // tile columns [lo_x, hi_x) exist
            if (hi_x > lo_x) cols = (hi_x - lo_x >= 64 ? ~0ull : ((1ull << (hi_x - lo_x)) - 1ull)) << lo_x;
        }
        ringbits[y] = v & ~own[y] & cols;
    }
    __syncthreads();
}

}  // namespace vvring
