// Overlay masking (videovanish_amd/overlaymask.py, infill.overlay_mask): pixels whose luma gradient keeps its sign over
// the clip while the picture under them changes are a screen-fixed graphic and join the mask of every frame.  The rules are
// include/overlaymask.h's; all arithmetic is integer.
//   vvo_accumulate        per tile of 64 x 16 pixels along the batch's frames: luma once per pixel into LDS, Sobel from LDS, four sums a pixel
//   vvo_classify          per pixel: rule 2's compares, the edge map, the two counts
//   vvo_component_stats   per pixel: area and bounding box at the component's label, integer atomics
//   vvo_select            per pixel: the kept components' pixels; per component: its box
//   vvo_merge             per frame: dil | O, the added-pixel counts
// vvo_accumulate is the hot one: it reads every frame byte of the clip once (4 bytes a pixel and frame with the mask).  A thread owns four
// adjacent pixels of one row: one 12-byte image load and one 4-byte mask load a frame (vv_wave_bytes.h's 4-pixel loads; W % 4 == 0 and aligned
// bases, checked by the launcher; else byte loads), four lumas packed into one dword of LDS.  The tile's plane is 18 rows of 18 dwords: the
// 16 x 16 dwords of the tile inside a ring of which the left column's last byte and the right column's first byte are the halo; 32 threads of
// wave 0 load the rows above and below, 36 of wave 1 the two columns, with coordinates clamped to the frame (rule 1's replicated border; a
// tile that hangs over the frame's edge replicates the same way, and its outside pixels are not stored).  Two planes: frame t writes plane
// t & 1, one barrier, every thread reads its 3 x 3 dwords; a thread that writes plane t & 1 again for frame t + 2 has passed the barrier of
// frame t + 1, which every thread reaches after its reads of frame t.  The next frame's own bytes are requested before the barrier and
// land while the Sobel taps of this one are taken.  The arithmetic is packed: a luma is one byte dot product, the taps are 16-bit lanes,
// two pixels an instruction, widened to 32 bits only where they join the sums (worth 0 to 8 % measured: DESIGN.md section 27).  The sixteen sums stay in registers and reach acc once, as 16-byte read-modify-writes: a
// thread owns its pixels, no atomics.  A frame with fewer than SPLIT_TILES tiles splits the batch over blockIdx.z in runs of at least
// SPLIT_FRAMES frames and adds with integer atomics; integer adds commute, so acc is the same either way.
#include "vv_common.h"
#include "vv_wave_bytes.h"
#include "../../include/overlaymask.h"

namespace {

using vvwave::load_mask;
using vvwave::luma;
using vvwave::store_mask;
using vvwave::U3;
using vvwave::wave_max;
using vvwave::wave_min;
using vvwave::wave_sum;
constexpr int PB = 256;                     // threads per block
typedef unsigned long long u64;
typedef long long i64;
constexpr int TW = VVO_TILE_W, TH = VVO_TILE_H;
constexpr int LS = TW / 4 + 2;              // 18: dwords a row of the plane
constexpr int LR = TH + 2;                  // 18: its rows
constexpr int SPLIT_TILES = 512, SPLIT_FRAMES = 8;
static_assert(TW == 64 && TH * (TW / 4) == PB && 2 * (TW / 4) <= 64 && 2 * LR <= 64, "a thread owns four pixels; the halo fits waves 0 and 1");
static_assert((i64)VVO_MAX_T * 2040 < ((i64)1 << 31), "A in 32 bits");

// every non-zero byte of w -> 255
__device__ __forceinline__ unsigned norm4(unsigned w) {
    const unsigned t = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;
    return (t >> 7) * 255u;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// luma of the pixel of `frame` nearest to (y, x)
__device__ __forceinline__ unsigned luma_at(const uint8_t* frame, int y, int x, int H, int W) {
    const uint8_t* px = frame + ((int64_t)clampi(y, H - 1) * W + clampi(x, W - 1)) * 3;
    return luma(px[0], px[1], px[2]);
}

// the 12 image bytes of the four pixels at (y, x .. x + 3), each taken from the nearest pixel of the frame
template <bool VEC> __device__ __forceinline__ U3 load_raw(const uint8_t* frame, int y, int x, int H, int W) {
    const uint8_t* row = frame + (int64_t)clampi(y, H - 1) * W * 3;
    if (VEC && x >= 0 && x + 3 < W) return *reinterpret_cast<const U3*>(row + (int64_t)x * 3);
    unsigned w[3] = {0, 0, 0};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint8_t* px = row + (int64_t)clampi(x + p, W - 1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) w[(3 * p + c) >> 2] |= (unsigned)px[c] << (((3 * p + c) & 3) * 8);
    }
    return U3{w[0], w[1], w[2]};
}
// four lumas, pixel p in bits 8 p ..
// vvwave::luma as one byte dot product a pixel: the pixel's three bytes are moved to the bottom of a dword (the fourth byte meets weight 0)
__device__ __forceinline__ unsigned luma4(const U3& q) {
    constexpr unsigned WEIGHTS = 77u | (150u << 8) | (29u << 16);
    const unsigned px[4] = {q.a, __builtin_amdgcn_alignbyte(q.b, q.a, 3), __builtin_amdgcn_alignbyte(q.c, q.b, 2), q.c >> 8};
    unsigned o = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) o |= (__builtin_amdgcn_udot4(px[p], WEIGHTS, 128u, false) >> 8) << (8 * p);
    return o;
}
static_assert(255u * (77u + 150u + 29u) + 128u < (1u << 16), "a luma is a byte");

// two 16-bit lanes in a dword: the Sobel taps of two pixels at once (every value stays within 16 bits: |g| <= 1020, |gx| + |gy| <= 2040)
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 lanes(unsigned w) { return __builtin_bit_cast(s16x2, w); }
__device__ __forceinline__ unsigned word(s16x2 v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ s16x2 abs2(s16x2 v) { return __builtin_elementwise_max(v, -v); }
// the four mask bytes at (y, x .. x + 3) of mask [H][W]; 255 outside the frame
template <bool VEC> __device__ __forceinline__ unsigned load_m4(const uint8_t* mask, int y, int x, int H, int W) {
    if (y >= H) return 0xffffffffu;
    const uint8_t* row = mask + (int64_t)y * W;
    if (VEC && x + 3 < W) return load_mask<true>(row + x);
    unsigned m = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) m |= (x + p < W ? (unsigned)row[x + p] : 255u) << (8 * p);
    return m;
}

// grid (tiles, 1, nz): tile = blockIdx.x, frames [blockIdx.z * chunk, + chunk) of the batch
template <bool VEC>
__global__ __launch_bounds__(PB) void accumulate_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ dil, int Tb, int H, int W,
                                                        int tiles_x, int chunk, int atomic, int acc16, int* __restrict__ acc) {
    __shared__ unsigned plane[2][LR * LS];
    const int t0 = (int)blockIdx.z * chunk, t1 = min(Tb, t0 + chunk);
    if (t0 >= t1) return;
    const int tid = threadIdx.x, tx = tid & (TW / 4 - 1), ty = tid / (TW / 4);
    const int x0 = ((int)blockIdx.x % tiles_x) * TW, y0 = ((int)blockIdx.x / tiles_x) * TH;
    const int x = x0 + 4 * tx, y = y0 + ty;
    const int64_t N = (int64_t)H * W;
    int n[4], sx[4], sy[4], sa[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) n[p] = sx[p] = sy[p] = sa[p] = 0;
    U3 raw = load_raw<VEC>(frames + (int64_t)t0 * N * 3, y, x, H, W);
    unsigned mraw = load_m4<VEC>(dil + (int64_t)t0 * N, y, x, H, W);
    for (int t = t0; t < t1; ++t) {
        unsigned* L = plane[(t - t0) & 1];
        const uint8_t* frame = frames + (int64_t)t * N * 3;
        L[(ty + 1) * LS + tx + 1] = luma4(raw);
        const unsigned m = mraw;
        if (tid < 2 * (TW / 4)) {                                            // the rows above and below
            const int below = tid / (TW / 4), j = tid % (TW / 4);
            L[(below ? LR - 1 : 0) * LS + j + 1] = luma4(load_raw<VEC>(frame, below ? y0 + TH : y0 - 1, x0 + 4 * j, H, W));
        } else if (tid >= 64 && tid < 64 + 2 * LR) {                          // the columns left and right, corners included
            const int right = (tid - 64) / LR, r = (tid - 64) % LR;
            reinterpret_cast<uint8_t*>(L)[(r * LS + (right ? LS - 1 : 0)) * 4 + (right ? 0 : 3)] =
                (uint8_t)luma_at(frame, y0 - 1 + r, right ? x0 + TW : x0 - 1, H, W);
        }
        if (t + 1 < t1) {                                                    // in flight across the barrier
            raw = load_raw<VEC>(frame + N * 3, y, x, H, W);
            mraw = load_m4<VEC>(dil + (int64_t)(t + 1) * N, y, x, H, W);
        }
        __syncthreads();
        if (norm4(m) == 0xffffffffu) continue;                                // no pixel of mine counts in this frame (uniform per thread: no barrier below)
        // R[k][j]: row k's lumas at x - 1 + 2 j and x + 2 j, a 16-bit lane each (v_perm_b32: selectors 0 .. 3 take the second operand's bytes,
        // 4 .. 7 the first's, 0x0c is zero)
        s16x2 R[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned* row = L + (ty + k) * LS + tx;
            const unsigned a = row[0], b = row[1], c = row[2];
            R[k][0] = lanes(__builtin_amdgcn_perm(b, a, 0x0c040c03u));
            R[k][1] = lanes(__builtin_amdgcn_perm(b, b, 0x0c020c01u));
            R[k][2] = lanes(__builtin_amdgcn_perm(c, b, 0x0c040c03u));
        }
        s16x2 CS[3], D[3];                                                    // the columns' 1 2 1 sums, and row below - row above
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            CS[j] = R[0][j] + R[1][j] + R[1][j] + R[2][j];
            D[j] = R[2][j] - R[0][j];
        }
        const s16x2 S0 = lanes(__builtin_amdgcn_alignbyte(word(D[1]), word(D[0]), 2)), S1 = lanes(__builtin_amdgcn_alignbyte(word(D[2]), word(D[1]), 2));
        const s16x2 gx[2] = {CS[1] - CS[0], CS[2] - CS[1]};                     // pixels (0, 1) and (2, 3)
        const s16x2 gy[2] = {D[0] + S0 + S0 + D[1], D[1] + S1 + S1 + D[2]};
        const unsigned open = ~norm4(m);                                      // byte p = 255 where pixel p counts
        const unsigned K[2] = {__builtin_amdgcn_perm(0u, open, 0x01010000u), __builtin_amdgcn_perm(0u, open, 0x03030202u)};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned ux = word(gx[h]) & K[h], uy = word(gy[h]) & K[h], ua = word(abs2(gx[h]) + abs2(gy[h])) & K[h];
            n[2 * h] += (int)((open >> (16 * h)) & 1u);
            n[2 * h + 1] += (int)((open >> (16 * h + 8)) & 1u);
            sx[2 * h] += (int)(short)ux;
            sx[2 * h + 1] += (int)ux >> 16;
            sy[2 * h] += (int)(short)uy;
            sy[2 * h + 1] += (int)uy >> 16;
            sa[2 * h] += (int)(ua & 0xffffu);
            sa[2 * h + 1] += (int)(ua >> 16);
        }
    }
    if (y >= H) return;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        if (x + p >= W) break;
        int* a = acc + ((int64_t)y * W + x + p) * 4;
        if (atomic) {
            if (n[p]) { atomicAdd(a, n[p]); atomicAdd(a + 1, sx[p]); atomicAdd(a + 2, sy[p]); atomicAdd(a + 3, sa[p]); }
        } else if (acc16) {
            int4 v = *reinterpret_cast<int4*>(a);
            v.x += n[p]; v.y += sx[p]; v.z += sy[p]; v.w += sa[p];
            *reinterpret_cast<int4*>(a) = v;
        } else {
            a[0] += n[p]; a[1] += sx[p]; a[2] += sy[p]; a[3] += sa[p];
        }
    }
}

// a block's two counts -> one 64-bit global atomic each
__device__ __forceinline__ void block_counts(unsigned c0, unsigned c1, u64* out0, u64* out1) {
    __shared__ unsigned tot[2];
    if (threadIdx.x < 2) tot[threadIdx.x] = 0;
    __syncthreads();
    const unsigned w0 = wave_sum(c0), w1 = wave_sum(c1);
    if ((threadIdx.x & 63) == 0) {
        if (w0) atomicAdd(&tot[0], w0);
        if (w1) atomicAdd(&tot[1], w1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && tot[0]) atomicAdd(out0, (u64)tot[0]);
    if (threadIdx.x == 1 && tot[1] && out1) atomicAdd(out1, (u64)tot[1]);
}

__global__ __launch_bounds__(PB) void classify_kernel(const int* __restrict__ acc, int64_t N, int min_samples, int mag, int coh, uint8_t* __restrict__ edge,
                                                      u64* __restrict__ counts) {
    const int64_t p = (int64_t)blockIdx.x * PB + threadIdx.x;
    unsigned strong = 0, e = 0;
    if (p < N) {
        const i64 n = acc[p * 4], Sx = acc[p * 4 + 1], Sy = acc[p * 4 + 2], A = acc[p * 4 + 3];
        strong = n >= min_samples && A >= (i64)mag * n;
        e = strong && 100 * ((Sx < 0 ? -Sx : Sx) + (Sy < 0 ? -Sy : Sy)) >= (i64)coh * A;
        edge[p] = e ? 255 : 0;
    }
    block_counts(strong, e, counts, counts + 1);
}

__global__ __launch_bounds__(PB) void stats_clear_kernel(int64_t N, int H, int W, int* __restrict__ stats) {
    const int64_t p = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (p >= N) return;
    int* s = stats + p * 5;
    s[0] = 0; s[1] = W; s[2] = H; s[3] = 0; s[4] = 0;
}

// A wave whose 64 pixels carry one label (the inside of a component: nearly every wave) reduces first and adds once.
__global__ __launch_bounds__(PB) void stats_kernel(const int* __restrict__ labels, int64_t N, int W, int* __restrict__ stats) {
    const int64_t p = (int64_t)blockIdx.x * PB + threadIdx.x;
    int l = p < N ? labels[p] : -1;
    if (l >= N) l = -1;
    const int px = (int)(p % W), py = (int)(p / W);
    const int first = __builtin_amdgcn_readfirstlane(l);
    if (__all(l == first)) {
        if (first < 0) return;
        const int lo_x = wave_min(px), lo_y = wave_min(py), hi_x = wave_max(px), hi_y = wave_max(py);
        if ((threadIdx.x & 63) == 0) {
            int* s = stats + (int64_t)first * 5;
            atomicAdd(s, 64); atomicMin(s + 1, lo_x); atomicMin(s + 2, lo_y); atomicMax(s + 3, hi_x + 1); atomicMax(s + 4, hi_y + 1);
        }
    } else if (l >= 0) {
        int* s = stats + (int64_t)l * 5;
        atomicAdd(s, 1); atomicMin(s + 1, px); atomicMin(s + 2, py); atomicMax(s + 3, px + 1); atomicMax(s + 4, py + 1);
    }
}

struct Keep { int min_area, max_area_px, inside_only, H, W; };
__device__ __forceinline__ bool is_kept(const int* s, const Keep& k) {
    return s[0] > 0 && s[0] >= k.min_area && s[0] <= k.max_area_px && (!k.inside_only || (s[1] > 0 && s[2] > 0 && s[3] < k.W && s[4] < k.H));
}
__device__ __forceinline__ void write_box(int* box, int label, const int* s) {
    box[0] = label; box[1] = s[0]; box[2] = s[1]; box[3] = s[2]; box[4] = s[3]; box[5] = s[4];
}

__global__ __launch_bounds__(PB) void select_kernel(const int* __restrict__ labels, const int* __restrict__ stats, int64_t N, Keep k, uint8_t* __restrict__ out,
                                                    int* __restrict__ boxes, int* __restrict__ nboxes) {
    const int64_t p = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (p >= N) return;
    const int l = labels[p];
    bool keep = false;
    if (l >= 0 && l < N) {
        const int* s = stats + (int64_t)l * 5;
        keep = is_kept(s, k);
        if (keep && l == p) {                                               // the component's first pixel speaks for it
            const int at = atomicAdd(nboxes, 1);
            if (at < VVO_MAX_BOXES) write_box(boxes + at * 6, l, s);
        }
    }
    out[p] = keep ? 255 : 0;
}

// More kept components than rows: the rows are those of the smallest labels, whatever order select_kernel's atomics came in.  One block walks
// the pixels in order and stops at the last row.
constexpr int FB = 1024;
__global__ __launch_bounds__(FB) void select_first_kernel(const int* __restrict__ labels, const int* __restrict__ stats, int64_t N, Keep k,
                                                          int* __restrict__ boxes, const int* __restrict__ nboxes) {
    __shared__ int wcnt[FB / 64];
    if (*nboxes <= VVO_MAX_BOXES) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int have = 0;
    for (int64_t s0 = 0; s0 < N && have < VVO_MAX_BOXES; s0 += FB) {
        const int64_t p = s0 + threadIdx.x;
        const bool f = p < N && labels[p] == p && is_kept(stats + p * 5, k);
        const u64 bal = __ballot(f);
        if (lane == 0) wcnt[w] = __popcll(bal);
        __syncthreads();
        int off = have, total = have;
        for (int j = 0; j < FB / 64; ++j) { off += j < w ? wcnt[j] : 0; total += wcnt[j]; }
        const int at = off + __popcll(bal & ((1ull << lane) - 1));
        if (f && at < VVO_MAX_BOXES) write_box(boxes + at * 6, (int)p, stats + p * 5);
        have = total;
        __syncthreads();
    }
}

// grid (ceil(units / PB), T): frame = blockIdx.y; o is the same map for every frame
template <bool VEC>
__global__ __launch_bounds__(PB) void merge_kernel(const uint8_t* __restrict__ dil, const uint8_t* __restrict__ o, int64_t N, int64_t units,
                                                   uint8_t* __restrict__ out, u64* __restrict__ added) {
    constexpr int P = VEC ? 4 : 1;
    const int t = (int)blockIdx.y;
    const int64_t u = (int64_t)blockIdx.x * PB + threadIdx.x;
    unsigned more = 0;
    if (u < units) {
        const int64_t at = (int64_t)t * N + u * P;
        const unsigned md = norm4(load_mask<VEC>(dil + at)), mo = norm4(load_mask<VEC>(o + u * P));
        more = (unsigned)__popc(mo & ~md) >> 3;
        store_mask<VEC>(out + at, md | mo);
    }
    block_counts(more, 0, added + t, nullptr);
}

// the frame sizes every entry point shares; 0 = fine
int bad_frame(const char* who, int H, int W) {
    if (H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31)) VV_FAIL(VV_E_ARG, "%s: bad args (H >= 1, W >= 1, H * W < 2^31)", who);
    return VV_OK;
}
int bad_frames(const char* who, int T, int H, int W) {
    if (T < 1) VV_FAIL(VV_E_ARG, "%s: bad args (T >= 1)", who);
    const int rc = bad_frame(who, H, W);
    if (rc != VV_OK) return rc;
    if (T > VVO_MAX_T) VV_FAIL(VV_E_UNSUPPORTED, "%s: T <= %d is supported, not %d", who, VVO_MAX_T, T);
    return VV_OK;
}
bool aligned(const void* p, unsigned a) { return (uintptr_t)p % a == 0; }
unsigned blocks_of(int64_t n) { return (unsigned)((n + PB - 1) / PB); }

}  // namespace

extern "C" int vvo_abi_version(void) { return VVO_ABI_VERSION; }
extern "C" const char* vvo_last_error(void) { return vv_last_error(); }

extern "C" int vvo_accumulate(const uint8_t* frames, const uint8_t* dil, int Tb, int H, int W, int32_t* acc, void* stream) {
    if (!frames || !dil || !acc) VV_FAIL(VV_E_ARG, "vvo_accumulate: bad args (no null pointer)");
    const int rc = bad_frames("vvo_accumulate", Tb, H, W);
    if (rc != VV_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int tiles_x = (W + TW - 1) / TW;
    const int64_t tiles = (int64_t)tiles_x * ((H + TH - 1) / TH);             // < 2^31: H * W < 2^31
    // a small frame: the batch in runs of at least SPLIT_FRAMES frames over blockIdx.z, added with atomics
    int nz = 1;
    if (tiles < SPLIT_TILES) {
        const int by_tiles = (int)(SPLIT_TILES / tiles), by_frames = (Tb + SPLIT_FRAMES - 1) / SPLIT_FRAMES;
        nz = by_tiles < by_frames ? by_tiles : by_frames;
    }
    const int chunk = (Tb + nz - 1) / nz;
    nz = (Tb + chunk - 1) / chunk;
    const bool vec = W % 4 == 0 && aligned(frames, 4) && aligned(dil, 4);
    const dim3 grid((unsigned)tiles, 1, (unsigned)nz);
    const int atomic = nz > 1, acc16 = aligned(acc, 16);
    if (vec) hipLaunchKernelGGL(accumulate_kernel<true>, grid, dim3(PB), 0, st, frames, dil, Tb, H, W, tiles_x, chunk, atomic, acc16, acc);
    else hipLaunchKernelGGL(accumulate_kernel<false>, grid, dim3(PB), 0, st, frames, dil, Tb, H, W, tiles_x, chunk, atomic, acc16, acc);
    VV_CHECK_LAUNCH("vvo_accumulate");
    return VV_OK;
}

extern "C" int vvo_classify(const int32_t* acc, int H, int W, int min_samples, int mag, int coh, uint8_t* edge, int64_t* counts, void* stream) {
    if (!acc || !edge || !counts || min_samples < 1 || mag < 1 || coh < 1)
        VV_FAIL(VV_E_ARG, "vvo_classify: bad args (no null pointer, min_samples >= 1, mag >= 1, coh >= 1)");
    const int rc = bad_frame("vvo_classify", H, W);
    if (rc != VV_OK) return rc;
    if (min_samples > VVO_MAX_T || mag > VVO_MAX_MAG || coh > VVO_MAX_COH)
        VV_FAIL(VV_E_UNSUPPORTED, "vvo_classify: min_samples <= %d, mag <= %d and coh <= %d are supported, not min_samples %d, mag %d, coh %d", VVO_MAX_T,
                VVO_MAX_MAG, VVO_MAX_COH, min_samples, mag, coh);
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)H * W;
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vvo_classify: memset failed");
    hipLaunchKernelGGL(classify_kernel, dim3(blocks_of(N)), dim3(PB), 0, st, acc, N, min_samples, mag, coh, edge, (u64*)counts);
    VV_CHECK_LAUNCH("vvo_classify");
    return VV_OK;
}

extern "C" int vvo_component_stats(const int32_t* labels, int H, int W, int32_t* stats, void* stream) {
    if (!labels || !stats) VV_FAIL(VV_E_ARG, "vvo_component_stats: bad args (no null pointer)");
    const int rc = bad_frame("vvo_component_stats", H, W);
    if (rc != VV_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)H * W;
    hipLaunchKernelGGL(stats_clear_kernel, dim3(blocks_of(N)), dim3(PB), 0, st, N, H, W, stats);
    VV_CHECK_LAUNCH("vvo_component_stats");
    hipLaunchKernelGGL(stats_kernel, dim3(blocks_of(N)), dim3(PB), 0, st, labels, N, W, stats);
    VV_CHECK_LAUNCH("vvo_component_stats");
    return VV_OK;
}

extern "C" int vvo_select(const int32_t* labels, const int32_t* stats, int H, int W, int min_area, int max_area_px, int inside_only, uint8_t* out,
                          int32_t* boxes, int32_t* nboxes, void* stream) {
    if (!labels || !stats || !out || !boxes || !nboxes || min_area < 0 || max_area_px < 0)
        VV_FAIL(VV_E_ARG, "vvo_select: bad args (no null pointer, min_area >= 0, max_area_px >= 0)");
    const int rc = bad_frame("vvo_select", H, W);
    if (rc != VV_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)H * W;
    const Keep k{min_area, max_area_px, inside_only != 0, H, W};
    if (hipMemsetAsync(nboxes, 0, sizeof(int32_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vvo_select: memset failed");
    hipLaunchKernelGGL(select_kernel, dim3(blocks_of(N)), dim3(PB), 0, st, labels, stats, N, k, out, boxes, nboxes);
    VV_CHECK_LAUNCH("vvo_select");
    hipLaunchKernelGGL(select_first_kernel, dim3(1), dim3(FB), 0, st, labels, stats, N, k, boxes, nboxes);
    VV_CHECK_LAUNCH("vvo_select");
    return VV_OK;
}

extern "C" int vvo_merge(const uint8_t* dil, const uint8_t* o, int T, int H, int W, uint8_t* dil_out, int64_t* added, void* stream) {
    if (!dil || !o || !dil_out || !added || dil_out == dil) VV_FAIL(VV_E_ARG, "vvo_merge: bad args (no null pointer, dil_out is not dil)");
    const int rc = bad_frames("vvo_merge", T, H, W);
    if (rc != VV_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)H * W;
    if (hipMemsetAsync(added, 0, (size_t)T * sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vvo_merge: memset failed");
    const bool vec = W % 4 == 0 && aligned(dil, 4) && aligned(o, 4) && aligned(dil_out, 4);
    const int64_t units = vec ? N / 4 : N;
    const dim3 grid(blocks_of(units), (unsigned)T);
    if (vec) hipLaunchKernelGGL(merge_kernel<true>, grid, dim3(PB), 0, st, dil, o, N, units, dil_out, (u64*)added);
    else hipLaunchKernelGGL(merge_kernel<false>, grid, dim3(PB), 0, st, dil, o, N, units, dil_out, (u64*)added);
    VV_CHECK_LAUNCH("vvo_merge");
    return VV_OK;
}
