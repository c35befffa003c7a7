// Block-matched inpaint deflicker (videovanish_amd/deflickerlocal.py, infill.finish): one integer displacement per block
// and temporal neighbour, found by block matching on the window's own pixels, and vv_flicker.hip's sigma filter read along it.  The rules are
// include/flicklocal.h's; all arithmetic is integer.
//   vvk_search   per (frame t, slot k, block) the lexicographic minimum of (cost, dy^2 + dx^2, dy, dx) over the valid candidates -> mv, stats
//   vvk_hold     vvc_hold's gather body with the block's record read per neighbour -> out, 12 sums per frame
// vvk_search: a workgroup of 4 waves owns up to 256 adjacent blocks of one block row of one (t, k) and walks them in strips of 4 blocks, one
// wave per block.  Per strip the 4 reference blocks (BLOCK rows x 4 * 3 * BLOCK bytes) and the search area of frame s under them (BLOCK + 2 S
// rows x (4 BLOCK + 2 S) * 3 bytes, zero where frame s's window has no pixel) are staged in LDS as dwords; no candidate reads HBM.
// Interleaved RGB is bytes: a block row is 3 * BLOCK bytes = W dwords, a candidate's row is the W dwords that start 3 * (dx + S) bytes into
// the area's row, made by v_alignbyte_b32 of adjacent LDS dwords, and the cost is v_sad_u8 of those against the reference dwords.
// Lanes: an item is (dy, group of 4 adjacent dx, quarter of the block's rows).  4 dx are 12 bytes = 3 dwords, so a group starts on a dword of
// the area's row and its four candidates sit at the CONSTANT byte shifts 0, 3, 2, 1 of the dwords 0, 0, 1, 2: a lane reads W + 3 area dwords
// and W reference dwords of a row once and takes 4 W SADs from them (0.6 LDS dwords per SAD; one candidate per lane reads 2.2 and
// measured up to 1.7 times slower).  The 4 lanes of a quad hold one (dy, group) and add their quarters with xor shuffles.  (2 S + 1) dy x
// ceil((2 S + 1) / 4) groups x 4 quarters: 108 items = 2 passes at 84 % of the lanes for S = 4 with 9 of 12 dx slots used, 340 = 6 passes at
// 89 % with 17 of 20 for S = 8, 40 = 1 pass at 62 % with 5 of 8 for S = 2; 81 candidates alone would fill 2 passes at 63 %.  The slots past
// dx = S are computed on staged bytes and dropped.
// D(t, s), the tracked flags, the block's extent and the byte masks of a tail block depend on blockIdx and the wave only: scalar registers.
// The winner is an integer minimum of the packed 64-bit key (cost, dy^2 + dx^2, dy + 8, dx + 8) over the wave: no lane order enters.
#include "vv_wave_bytes.h"
#include "../../include/flicklocal.h"

namespace {

using vvwave::wave_sum;
using vvwave::wave_min64;
typedef unsigned long long u64;
typedef long long i64;
constexpr int FB = 256;                     // threads per block
constexpr int WAVES = FB / 64;              // blocks per strip
constexpr int STRIPS = 64;                  // strips per workgroup: 256 blocks of a block row
constexpr int NSUM = 12;
constexpr int MAXS = VVK_MAX_SEARCH;
constexpr int MAXC = (2 * MAXS + 1) * (2 * MAXS + 1);
static_assert(VVK_MAX_RADIUS == 4 && 2 * VVK_MAX_RADIUS + 1 <= 9, "n <= 9: the reciprocals, the packed sums");
static_assert(16ll * 16 * 3 * 255 + 2ll * MAXS * VVK_MAX_LAM < (1ll << 31), "a cost fits 31 bits");
static_assert(2 * MAXS * MAXS < 256 && 2 * MAXS + 1 < 256, "the key's fields");
static_assert(64 * 255 < (1 << 16) && 64 * 9 < (1 << 16), "a wave's sums of one pixel per lane fit the 16-bit halves");

// grid (T * K * nby * xchunks): blockIdx.x = ((t * K + k) * nby + by) * xchunks + xc.  Reads of win are bounds-checked against the window of
// the frame they come from (staging); the writes are the workgroup's own records of mv and the atomics into stats[t][k].
template <int BLOCK>
__global__ __launch_bounds__(FB) void search_kernel(const uint8_t* __restrict__ win, const int* __restrict__ offsets, const int32_t* __restrict__ track, int T,
                                                    int h, int w, int R, int S, int lam, int nby, int nbx, int xchunks, int32_t* __restrict__ mv,
                                                    u64* __restrict__ stats) {
    constexpr int W = 3 * BLOCK / 4;            // dwords of a block row
    constexpr int RPITCH = WAVES * W;           // dwords of a row of the reference strip
    constexpr int APITCH = WAVES * W + 15;      // dwords of a row of the area: (4 BLOCK + 2 S) * 3 bytes and what the last group reads past them, odd
    constexpr int AROWS = BLOCK + 2 * MAXS;
    constexpr int RPI = BLOCK / 4;              // rows per item
    constexpr int MAXG = (2 * MAXS + 1 + 3) / 4;
    static_assert(APITCH * 4 >= (WAVES * BLOCK + 2 * MAXS) * 3 + 4 && (WAVES - 1) * W + 3 * (MAXG - 1) + W + 2 <= APITCH - 1, "the area's row");
    __shared__ unsigned ref[BLOCK * RPITCH];
    __shared__ unsigned area[AROWS * APITCH];
    __shared__ unsigned cost[WAVES][MAXC];
    __shared__ u64 tot[VVK_NSTAT];
    const int K = 2 * R + 1;
    unsigned g = blockIdx.x;
    const int xc = (int)(g % (unsigned)xchunks); g /= (unsigned)xchunks;
    const int by = (int)(g % (unsigned)nby); g /= (unsigned)nby;
    const int k = (int)(g % (unsigned)K), t = (int)(g / (unsigned)K);
    const int s = t - R + k;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bxa = xc * (STRIPS * WAVES), bxe = min(nbx, bxa + STRIPS * WAVES);
    int32_t* rec0 = mv + ((((i64)t * K + k) * nby + by) * nbx) * VVK_MV_INTS;      // the block row's records

    // whether s gives samples at all, and D(t, s): blockIdx only, scalar loads, scalar registers
    bool any = s != t && s >= 0 && s < T && track[t * VVK_TRACK_INTS + 3] == 1;
    if (any) any = track[s * VVK_TRACK_INTS + 3] == 1;
    i64 Dy = 0, Dx = 0;
    if (any) {
        Dy = ((i64)offsets[t * 2 + 0] + track[t * VVK_TRACK_INTS + 1]) - ((i64)offsets[s * 2 + 0] + track[s * VVK_TRACK_INTS + 1]);
        Dx = ((i64)offsets[t * 2 + 1] + track[t * VVK_TRACK_INTS + 0]) - ((i64)offsets[s * 2 + 1] + track[s * VVK_TRACK_INTS + 0]);
        any = Dy > -((i64)h + S) && Dy < (i64)h + S && Dx > -((i64)w + S) && Dx < (i64)w + S;      // else no candidate of any block is valid
    }
    if (!any) {
        for (int i = tid; i < (bxe - bxa) * VVK_MV_INTS; i += FB) rec0[(i64)bxa * VVK_MV_INTS + i] = 0;
        return;
    }
    if (tid < VVK_NSTAT) tot[tid] = 0;
    const int n1 = 2 * S + 1, NC = n1 * n1, groups = (n1 + 3) >> 2, items = n1 * groups * 4, arows = BLOCK + 2 * S;
    const int y0 = by * BLOCK, bh = min(BLOCK, h - y0);
    const uint8_t* wt = win + (i64)t * h * w * 3;
    const uint8_t* ws = win + (i64)s * h * w * 3;
    unsigned cnt = 0, moved = 0, sabs = 0, far = 0;          // this wave's blocks: wave-uniform
    u64 scost = 0, szero = 0;

    for (int bx0 = bxa; bx0 < bxe; bx0 += WAVES) {
        // ---- stage: the area of frame s (zero outside its window), the reference strip of frame t (zero outside the window)
        const i64 ay = (i64)y0 + Dy - S, ax = (i64)bx0 * BLOCK + Dx - S;
        for (int i = tid; i < arows * APITCH; i += FB) {
            const int r = i / APITCH, cd = i - r * APITCH;
            const i64 ys = ay + r;
            unsigned v = 0;
            if (ys >= 0 && ys < h) {
                const uint8_t* row = ws + ys * w * 3;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int c = 4 * cd + b, px = c / 3, ch = c - 3 * px;
                    const i64 xs = ax + px;
                    if (xs >= 0 && xs < w) v |= (unsigned)row[xs * 3 + ch] << (8 * b);
                }
            }
            area[i] = v;
        }
        for (int i = tid; i < BLOCK * RPITCH; i += FB) {
            const int r = i / RPITCH, cd = i - r * RPITCH;
            unsigned v = 0;
            if (r < bh) {
                const uint8_t* row = wt + (i64)(y0 + r) * w * 3;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int c = 4 * cd + b, px = c / 3, ch = c - 3 * px;
                    const i64 xx = (i64)bx0 * BLOCK + px;
                    if (xx < w) v |= (unsigned)row[xx * 3 + ch] << (8 * b);
                }
            }
            ref[i] = v;
        }
        __syncthreads();
        const int bx = bx0 + wave;
        const bool active = bx < bxe;
        const int bw = active ? min(BLOCK, w - bx * BLOCK) : 0;
        // ---- the byte SADs: item = (dy, group of 4 dx, quarter of the rows)
        if (active) {
            unsigned m[W];                                   // the bytes of a block row that exist: all ones but in a tail block
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const int nv = min(max(3 * bw - 4 * j, 0), 4);
                m[j] = nv >= 4 ? ~0u : (1u << (8 * nv)) - 1u;
            }
            for (int i0 = 0; i0 < items; i0 += 64) {
                const int i = i0 + lane;
                const bool live = i < items;                 // a quad is live or not as a whole: items % 4 == 0
                const int q = live ? i >> 2 : 0, part = i & 3;
                const int dyi = (int)((unsigned)q / (unsigned)groups), g = q - dyi * groups;
                const int ad = wave * W + 3 * g;             // the group's first dx starts 12 g bytes into the block's part of the area's row
                unsigned acc[4] = {0u, 0u, 0u, 0u};
                if (live) {
#pragma unroll
                    for (int r = 0; r < RPI; ++r) {
                        const int row = part * RPI + r;
                        if (row < bh) {
                            const unsigned* a = area + (row + dyi) * APITCH + ad;
                            const unsigned* f = ref + row * RPITCH + wave * W;
                            unsigned av[W + 3];
#pragma unroll
                            for (int j = 0; j < W + 3; ++j) av[j] = a[j];
#pragma unroll
                            for (int j = 0; j < W; ++j) {    // dx slot c starts 3 c bytes on: dword (3 c) >> 2, byte (3 c) & 3
                                const unsigned fj = f[j];
                                acc[0] = __builtin_amdgcn_sad_u8(av[j] & m[j], fj, acc[0]);
                                acc[1] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(av[j + 1], av[j], 3u) & m[j], fj, acc[1]);
                                acc[2] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(av[j + 2], av[j + 1], 2u) & m[j], fj, acc[2]);
                                acc[3] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(av[j + 3], av[j + 2], 1u) & m[j], fj, acc[3]);
                            }
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    acc[c] += __shfl_xor(acc[c], 1, 64);
                    acc[c] += __shfl_xor(acc[c], 2, 64);
                    if (live && part == 0 && 4 * g + c < n1) cost[wave][dyi * n1 + 4 * g + c] = acc[c];
                }
            }
        }
        __syncthreads();
        // ---- the winner: the minimum of the packed key over the valid candidates
        if (active) {
            const i64 py = (i64)y0 + Dy, px = (i64)bx * BLOCK + Dx;
            u64 best = ~0ull;
            for (int c0 = 0; c0 < NC; c0 += 64) {
                const int c = c0 + lane;
                if (c < NC) {
                    const int dyi = (int)((unsigned)c / (unsigned)n1), dy = dyi - S, dx = c - dyi * n1 - S;
                    const bool valid = py + dy >= 0 && py + dy + bh <= h && px + dx >= 0 && px + dx + bw <= w;
                    const unsigned cst = cost[wave][c] + (unsigned)lam * (unsigned)(abs(dy) + abs(dx));
                    const u64 key = ((u64)cst << 32) | ((u64)(unsigned)(dy * dy + dx * dx) << 16) | ((u64)(unsigned)(dy + MAXS) << 8) | (u64)(unsigned)(dx + MAXS);
                    if (valid && key < best) best = key;
                }
            }
            best = wave_min64(best);
            const bool zero_ok = py >= 0 && py + bh <= h && px >= 0 && px + bw <= w;
            if (zero_ok) szero += cost[wave][S * n1 + S];
            const bool won = best != ~0ull;
            const int dy = won ? (int)((best >> 8) & 255u) - MAXS : 0, dx = won ? (int)(best & 255u) - MAXS : 0;
            const int cst = won ? (int)(best >> 32) : 0;
            if (won) {
                cnt += 1; moved += (dy | dx) ? 1u : 0u; sabs += (unsigned)(abs(dy) + abs(dx)); far = max(far, (unsigned)max(abs(dy), abs(dx)));
                scost += (u64)cst;
            }
            if (lane < VVK_MV_INTS) rec0[(i64)bx * VVK_MV_INTS + lane] = lane == 0 ? dy : lane == 1 ? dx : lane == 2 ? (won ? 1 : 0) : cst;
        }
    }
    if (lane == 0) {
        if (cnt) { atomicAdd(&tot[0], (u64)cnt); atomicAdd(&tot[4], scost); }
        if (moved) { atomicAdd(&tot[1], (u64)moved); atomicAdd(&tot[2], (u64)sabs); atomicMax(&tot[3], (u64)far); }
        if (szero) atomicAdd(&tot[5], szero);
    }
    __syncthreads();
    if (tid < VVK_NSTAT && tot[tid]) {
        u64* dst = stats + ((i64)t * K + k) * VVK_NSTAT + tid;
        if (tid == 3) atomicMax(dst, tot[tid]); else atomicAdd(dst, tot[tid]);
    }
}

// ---- the filter: vv_flicker.hip's gather body (its arithmetic, token for token) with the block's record per neighbour --------------------
// x / (2 n) == (x * recip(n)) >> 20 for every x <= 2 * 255 * n + n
constexpr unsigned recip(unsigned n) { return (1u << 20) / (2u * n) + 1u; }
constexpr bool recip_exact() {
    for (unsigned n = 1; n <= 9; ++n)
        for (unsigned x = 0; x <= 511u * n; ++x)
            if (((x * recip(n)) >> 20) != x / (2u * n)) return false;
    return true;
}
static_assert(recip_exact(), "the rounded mean by multiplication");

__device__ __forceinline__ unsigned absdiff(unsigned a, unsigned b) { return __sad(a, b, 0u); }      // |a - b| of two bytes

// what one thread adds to a frame's sums: every lane of the wave calls it.  lo = the quantities over the window, hi = over the masked pixels:
// [0] = pixels | changed << 16, [1] = sum n | sum d_0 << 16, [2] = sum d_1 | sum d_2 << 16
__device__ __forceinline__ void add_sums(unsigned* tot, const unsigned* lo, const unsigned* hi) {
    const bool lane0 = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const unsigned* v = half ? hi : lo;
        if (half && !__any((int)v[0])) return;                             // wave-uniform: no masked pixel in this wave's pixels
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k == 2 && !__any((int)v[2])) continue;                     // wave-uniform
            const unsigned s = wave_sum(v[k]);
            if (lane0) {
                if (s & 0xffffu) atomicAdd(&tot[half * 6 + (k == 0 ? 0 : k == 1 ? 2 : 4)], s & 0xffffu);
                if (s >> 16) atomicAdd(&tot[half * 6 + (k == 0 ? 1 : k == 1 ? 3 : 5)], s >> 16);
            }
        }
    }
}

// grid (ceil(h w / FB), T): frame = blockIdx.y.  Reads of win are bounds-checked against the window of the frame they come from (in 64 bits:
// mv is data), reads of the mask against the frame, reads of mv lie at the pixel's own block of slot s - t + R; the writes are the thread's
// own 3 bytes of out and the atomics into sums[t].  e_t - e_s and the tracked flags stay in scalar registers, as in vvc_hold's kernel.
__global__ __launch_bounds__(FB) void hold_local_kernel(const uint8_t* __restrict__ win, const int* __restrict__ offsets, const int32_t* __restrict__ track,
                                                        const int32_t* __restrict__ mv, const uint8_t* __restrict__ mask, int T, int H0, int W0, int h, int w,
                                                        int R, int bshift, int nby, int nbx, int tol, uint8_t* __restrict__ out, u64* __restrict__ sums) {
    __shared__ unsigned mg[10];
    __shared__ unsigned tot[NSUM];
    const int t = (int)blockIdx.y;
    if (threadIdx.x < NSUM) tot[threadIdx.x] = 0;
    if (threadIdx.x < 10) mg[threadIdx.x] = threadIdx.x ? recip(threadIdx.x) : 0u;
    __syncthreads();
    const int64_t N = (int64_t)h * w, i = (int64_t)blockIdx.x * FB + threadIdx.x;
    const bool active = i < N;
    unsigned lo[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u};
    if (active) {
        const int yy = (int)(i / w), xx = (int)(i % w);
        const int py = offsets[t * 2 + 0] + yy, px = offsets[t * 2 + 1] + xx;
        const uint8_t* c = win + ((int64_t)t * N + i) * 3;
        const unsigned x[3] = {c[0], c[1], c[2]};
        unsigned S[3] = {x[0], x[1], x[2]}, n = 1;
        const int s0 = max(t - R, 0), s1 = min(t + R, T - 1), K = 2 * R + 1;
        const bool t_tracked = track[t * VVK_TRACK_INTS + 3] == 1;
        const int64_t ety = (int64_t)offsets[t * 2 + 0] + track[t * VVK_TRACK_INTS + 1], etx = (int64_t)offsets[t * 2 + 1] + track[t * VVK_TRACK_INTS + 0];
        const int64_t blk = (int64_t)(yy >> bshift) * nbx + (xx >> bshift);                 // the pixel's block inside a slot
        for (int s = s0; s <= s1; ++s) {
            if (s == t || !t_tracked || track[s * VVK_TRACK_INTS + 3] != 1) continue;
            const int64_t dy = ety - ((int64_t)offsets[s * 2 + 0] + track[s * VVK_TRACK_INTS + 1]), dx = etx - ((int64_t)offsets[s * 2 + 1] + track[s * VVK_TRACK_INTS + 0]);
            const int32_t* rec = mv + ((((int64_t)t * K + (s - t + R)) * nby) * nbx + blk) * VVK_MV_INTS;
            if (rec[2] != 1) continue;
            const int64_t ys = yy + dy + rec[0], xs = xx + dx + rec[1];                     // |each term| < 2^34: no overflow
            if (ys < 0 || ys >= h || xs < 0 || xs >= w) continue;
            const uint8_t* q = win + (((int64_t)s * h + ys) * w + xs) * 3;
            const unsigned v[3] = {q[0], q[1], q[2]};
            const unsigned ok = max(max(absdiff(v[0], x[0]), absdiff(v[1], x[1])), absdiff(v[2], x[2])) <= (unsigned)tol ? 1u : 0u;
            n += ok;
#pragma unroll
            for (int k = 0; k < 3; ++k) S[k] += v[k] * ok;
        }
        const unsigned m = mg[n];
        unsigned d[3];
        uint8_t* dst = out + ((int64_t)t * N + i) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned o = ((2u * S[k] + n) * m) >> 20;
            d[k] = absdiff(o, x[k]);
            dst[k] = (uint8_t)o;
        }
        lo[0] = 1u | ((d[0] | d[1] | d[2]) ? 1u << 16 : 0u); lo[1] = n | (d[0] << 16); lo[2] = d[1] | (d[2] << 16);
        if (py >= 0 && py < H0 && px >= 0 && px < W0 && mask[((int64_t)t * H0 + py) * W0 + px]) { hi[0] = lo[0]; hi[1] = lo[1]; hi[2] = lo[2]; }
    }
    add_sums(tot, lo, hi);
    __syncthreads();
    if (threadIdx.x < NSUM && tot[threadIdx.x]) atomicAdd(&sums[(int64_t)t * NSUM + threadIdx.x], (u64)tot[threadIdx.x]);
}

}  // namespace

extern "C" int vvk_abi_version(void) { return VVK_ABI_VERSION; }
extern "C" const char* vvk_last_error(void) { return vv_last_error(); }

extern "C" int vvk_search(const uint8_t* win, const int* offsets, const int32_t* track, int T, int h, int w, int radius, int block, int search, int lam,
                          int32_t* mv, int64_t* stats, void* stream) {
    if (!win || !offsets || !track || !mv || !stats || T <= 0 || h <= 0 || w <= 0 || radius < 0 || block <= 0 || search < 0 || lam < 0)
        VV_FAIL(VV_E_ARG, "vvk_search: bad args (no null pointer, sizes > 0, radius >= 0, block > 0, search >= 0, lam >= 0)");
    if ((block != 8 && block != 16) || search > VVK_MAX_SEARCH || lam > VVK_MAX_LAM || radius > VVK_MAX_RADIUS || T > VVK_MAX_T ||
        (int64_t)h * w >= ((int64_t)1 << 31))
        VV_FAIL(VV_E_UNSUPPORTED, "vvk_search: block 8 or 16, search <= %d, lam <= %d, radius <= %d, T <= %d and h * w < 2^31 are supported, not block %d, "
                "search %d, lam %d, radius %d, T %d, %d x %d", VVK_MAX_SEARCH, VVK_MAX_LAM, VVK_MAX_RADIUS, VVK_MAX_T, block, search, lam, radius, T, h, w);
    const int K = 2 * radius + 1, nby = (h + block - 1) / block, nbx = (w + block - 1) / block, xchunks = (nbx + STRIPS * WAVES - 1) / (STRIPS * WAVES);
    const int64_t groups = (int64_t)T * K * nby * xchunks;
    if (groups >= ((int64_t)1 << 31)) VV_FAIL(VV_E_UNSUPPORTED, "vvk_search: fewer than 2^31 workgroups are supported, not %lld", (long long)groups);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(stats, 0, (size_t)T * K * VVK_NSTAT * sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vvk_search: memset failed");
    if (block == 8)
        hipLaunchKernelGGL(search_kernel<8>, dim3((unsigned)groups), dim3(FB), 0, st, win, offsets, track, T, h, w, radius, search, lam, nby, nbx, xchunks, mv,
                           (u64*)stats);
    else
        hipLaunchKernelGGL(search_kernel<16>, dim3((unsigned)groups), dim3(FB), 0, st, win, offsets, track, T, h, w, radius, search, lam, nby, nbx, xchunks, mv,
                           (u64*)stats);
    VV_CHECK_LAUNCH("vvk_search");
    return VV_OK;
}

extern "C" int vvk_hold(const uint8_t* win, const int* offsets, const int32_t* track, const int32_t* mv, const uint8_t* mask2d, int T, int H0, int W0, int h,
                        int w, int radius, int block, int tol, uint8_t* out, int64_t* sums, void* stream) {
    if (!win || !offsets || !track || !mv || !mask2d || !out || !sums || T <= 0 || H0 <= 0 || W0 <= 0 || h <= 0 || w <= 0 || h > H0 || w > W0 || radius < 0 ||
        block <= 0 || tol < 0 || out == win)
        VV_FAIL(VV_E_ARG, "vvk_hold: bad args (no null pointer, sizes > 0, h <= H0, w <= W0, radius >= 0, block > 0, tol >= 0, out is not win)");
    if ((block != 8 && block != 16) || radius > VVK_MAX_RADIUS || tol > 255 || T > VVK_MAX_T || (int64_t)h * w >= ((int64_t)1 << 31))
        VV_FAIL(VV_E_UNSUPPORTED, "vvk_hold: block 8 or 16, radius <= %d, tol <= 255, T <= %d and h * w < 2^31 are supported, not block %d, radius %d, tol %d, "
                "T %d, %d x %d", VVK_MAX_RADIUS, VVK_MAX_T, block, radius, tol, T, h, w);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, (size_t)T * NSUM * sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vvk_hold: memset failed");
    const int64_t N = (int64_t)h * w;
    const int nby = (h + block - 1) / block, nbx = (w + block - 1) / block;
    hipLaunchKernelGGL(hold_local_kernel, dim3((unsigned)((N + FB - 1) / FB), (unsigned)T), dim3(FB), 0, st, win, offsets, track, mv, mask2d, T, H0, W0, h, w,
                       radius, block == 8 ? 3 : 4, nby, nbx, tol, out, (u64*)sums);
    VV_CHECK_LAUNCH("vvk_hold");
    return VV_OK;
}
