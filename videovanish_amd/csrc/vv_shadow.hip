// Shadow masking (videovanish_amd/shadowmask.py, infill.shadow_mask): unmasked pixels that look like the shot's clean
// background uniformly darkened, and that hang on to the frame's mask, join the mask.  The rules are include/vvshadow.h's; all arithmetic is
// integer.
//   vvh_plate        per pixel along time, twice: n and the luma sum over the sample frames, then n2, T1, T2 over the lit ones, the plate flag
//   vvh_candidates   per frame: rule 4's compares against the plate, the candidate counts
//   vvh_grow         per frame and 64 x 64 tile: rule 5's geodesic growth in LDS, up to 8 sweeps a pass inside an 8-pixel halo
//   vvh_merge        per frame: dil | S', the added-pixel counts
// vvh_plate, vvh_candidates and vvh_merge are a streaming family as vv_plate.hip's: a thread owns P adjacent pixels of one row (VEC: P = 4, one
// 12-byte image load and 4-byte mask loads, lane after lane contiguous; W % 4 == 0 and aligned bases, checked by the launcher; else P = 1 with
// byte loads).  The counts go registers -> wave reduction -> LDS -> one 64-bit global atomic per block, as in vv_tone.hip.
// vvh_grow keeps A in two LDS planes (ping-pong: a sweep reads A_k and writes A_{k+1}, never in place) and cand in a third, one byte a pixel
// (0 / 255), four pixels a dword: the 3 x 3 dilation of a dword is nine dword reads, shifts and ORs.  A plane is 82 rows of 22 dwords: the 80 x 80
// pixels of tile plus halo inside a ring of zeros, so that no read needs a bounds test; 22 dwords keeps the row stride off the 32-dword period of
// the banks.  K sweeps inside a K-pixel halo equal K global sweeps on the interior: a pixel d pixels inside the loaded region is exact through
// sweep d (what lies outside the region reaches it after d + 1 sweeps at the earliest), and the interior has d >= K.
#include "vv_common.h"
#include "vv_wave_bytes.h"
#include "../../include/vvshadow.h"

namespace {

using vvwave::load_mask;
using vvwave::load_px;
using vvwave::store_mask;
using vvwave::wave_sum;
constexpr int PB = 256;                     // threads per block
typedef unsigned long long u64;
typedef long long i64;
static_assert((u64)VVH_MAX_T * 255 * 255 < (1ull << 32), "T2 in 32 bits");
static_assert((u64)VVH_MAX_T * 765 * 2 < (1ull << 32), "rule 2 in 32 bits");

// every non-zero byte of w -> 255
__device__ __forceinline__ unsigned norm4(unsigned w) {
    const unsigned t = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;
    return (t >> 7) * 255u;
}

template <bool VEC>
__global__ __launch_bounds__(PB) void plate_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ ns, int T, int64_t N, int64_t units,
                                                   int min_samples, int tol, uint8_t* __restrict__ ok, unsigned* __restrict__ n2_out,
                                                   unsigned* __restrict__ t1_out) {
    constexpr int P = VEC ? 4 : 1;
    const int64_t u = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (u >= units) return;
    const int64_t i0 = u * P;
    // rule 2's n and S
    unsigned n[P], S[P];
#pragma unroll
    for (int p = 0; p < P; ++p) n[p] = S[p] = 0;
    for (int t = 0; t < T; ++t) {
        const unsigned m = load_mask<VEC>(ns + (int64_t)t * N + i0);
        unsigned smp[P], any = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) { smp[p] = ((m >> (8 * p)) & 255u) == 0; any |= smp[p]; }
        if (!any) continue;
        unsigned v[3 * P];
        load_px<VEC>(frames + ((int64_t)t * N + i0) * 3, v);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            n[p] += smp[p];
            S[p] += smp[p] ? v[3 * p] + v[3 * p + 1] + v[3 * p + 2] : 0u;
        }
    }
    // rule 3's sums over the lit samples: n * L + 3 * tol * n >= S, each side below 2^32
    unsigned n2[P], t1[3 * P], t2[3 * P], slack[P];
#pragma unroll
    for (int p = 0; p < P; ++p) { n2[p] = 0; slack[p] = 3u * (unsigned)tol * n[p]; }
#pragma unroll
    for (int j = 0; j < 3 * P; ++j) t1[j] = t2[j] = 0;
    for (int t = 0; t < T; ++t) {
        const unsigned m = load_mask<VEC>(ns + (int64_t)t * N + i0);
        unsigned smp[P], any = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) { smp[p] = ((m >> (8 * p)) & 255u) == 0; any |= smp[p]; }
        if (!any) continue;
        unsigned v[3 * P];
        load_px<VEC>(frames + ((int64_t)t * N + i0) * 3, v);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const unsigned L = v[3 * p] + v[3 * p + 1] + v[3 * p + 2];
            const bool lit = smp[p] && n[p] * L + slack[p] >= S[p];
            n2[p] += lit ? 1u : 0u;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned x = lit ? v[3 * p + c] : 0u;
                t1[3 * p + c] += x;
                t2[3 * p + c] += x * x;
            }
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        bool st = n2[p] >= (unsigned)min_samples;
        const u64 bound = (u64)tol * tol * n2[p] * n2[p];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const u64 a = (u64)n2[p] * t2[3 * p + c], b = (u64)t1[3 * p + c] * t1[3 * p + c];      // a >= b (Cauchy-Schwarz)
            st = st && a - b <= bound;
            t1_out[(i0 + p) * 3 + c] = t1[3 * p + c];
        }
        ok[i0 + p] = st ? 1 : 0;
        n2_out[i0 + p] = n2[p];
    }
}

struct CandArgs { int lo, hi, drop, chroma, floor; };

// rule 4 for one unmasked pixel with a plate
__device__ __forceinline__ bool is_candidate(const unsigned* v, unsigned n2u, const unsigned* t1u, const CandArgs& a) {
    const i64 n2 = n2u;
    i64 t1[3], nv[3];
    bool c = true;
    i64 dark = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t1[k] = t1u[k];
        nv[k] = n2 * (i64)v[k];
        c = c && t1[k] >= a.floor * n2 && a.lo * t1[k] <= 100 * nv[k] && 100 * nv[k] <= a.hi * t1[k];
        dark += t1[k] - nv[k];
    }
    c = c && dark >= 3 * (i64)a.drop * n2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int x = k == 2 ? 0 : k, y = k == 2 ? 2 : k + 1;                // (0, 1), (1, 2), (0, 2)
        const i64 d = (i64)v[x] * t1[y] - (i64)v[y] * t1[x];
        c = c && (d < 0 ? -d : d) * 100 * n2 <= (i64)a.chroma * t1[x] * t1[y];
    }
    return c;
}

// grid (ceil(units / PB), T): frame = blockIdx.y
template <bool VEC>
__global__ __launch_bounds__(PB) void cand_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ dil, const uint8_t* __restrict__ ok,
                                                  const unsigned* __restrict__ n2, const unsigned* __restrict__ t1, int64_t N, int64_t units, CandArgs a,
                                                  uint8_t* __restrict__ cand, u64* __restrict__ counts) {
    constexpr int P = VEC ? 4 : 1;
    __shared__ unsigned tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    const int t = (int)blockIdx.y;
    const int64_t u = (int64_t)blockIdx.x * PB + threadIdx.x;
    unsigned found = 0;
    if (u < units) {
        const int64_t i0 = u * P, at = (int64_t)t * N + i0;
        const unsigned md = load_mask<VEC>(dil + at), mo = load_mask<VEC>(ok + i0);
        unsigned open = 0, o = 0;                                           // open: bit p = pixel p is unmasked and has a plate
#pragma unroll
        for (int p = 0; p < P; ++p) open |= (((md >> (8 * p)) & 255u) == 0 && ((mo >> (8 * p)) & 255u) != 0) ? 1u << p : 0u;
        if (open) {
            unsigned v[3 * P];
            load_px<VEC>(frames + at * 3, v);
#pragma unroll
            for (int p = 0; p < P; ++p) {
                if (!((open >> p) & 1u)) continue;
                const unsigned tt[3] = {t1[(i0 + p) * 3], t1[(i0 + p) * 3 + 1], t1[(i0 + p) * 3 + 2]};
                if (is_candidate(v + 3 * p, n2[i0 + p], tt, a)) {
                    o |= 1u << (8 * p);
                    ++found;
                }
            }
        }
        store_mask<VEC>(cand + at, o);
    }
    const unsigned w = wave_sum(found);                                     // <= 4 per lane
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(&tot, w);
    __syncthreads();
    if (threadIdx.x == 0 && tot) atomicAdd(&counts[(int64_t)t * 2], (u64)tot);
}

// grid (ceil(units / PB), T)
template <bool VEC>
__global__ __launch_bounds__(PB) void merge_kernel(const uint8_t* __restrict__ dil, const uint8_t* __restrict__ s, int64_t N, int64_t units,
                                                   uint8_t* __restrict__ out, u64* __restrict__ counts) {
    constexpr int P = VEC ? 4 : 1;
    __shared__ unsigned tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    const int t = (int)blockIdx.y;
    const int64_t u = (int64_t)blockIdx.x * PB + threadIdx.x;
    unsigned added = 0;
    if (u < units) {
        const int64_t at = (int64_t)t * N + u * P;
        const unsigned md = norm4(load_mask<VEC>(dil + at)), ms = norm4(load_mask<VEC>(s + at));
        added = (unsigned)__popc(ms & ~md) >> 3;
        store_mask<VEC>(out + at, md | ms);
    }
    const unsigned w = wave_sum(added);
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(&tot, w);
    __syncthreads();
    if (threadIdx.x == 0 && tot) atomicAdd(&counts[(int64_t)t * 2 + 1], (u64)tot);
}

// ---- rule 5 in LDS -----------------------------------------------------------------------------------------------------------------------------
constexpr int GT = VVH_GROW_TILE, GK = VVH_GROW_K;
constexpr int GR = GT + 2 * GK;              // 80: rows and columns of tile plus halo
constexpr int GD = GR / 4;                   // 20: its dwords a row
constexpr int GS = GD + 2;                   // 22: the row stride in dwords, a zero dword either side
constexpr int GP = (GR + 2) * GS;            // a plane: a zero row above and below
static_assert(GT % 4 == 0 && GK % 4 == 0 && GS % 32 != 0, "dword columns; the stride off the banks' period");

// 4 bytes of src [H][W] at (y, x .. x + 3), zero outside the frame, every non-zero byte 255
template <bool VEC> __device__ __forceinline__ unsigned load4(const uint8_t* src, int y, int x, int H, int W) {
    if (y < 0 || y >= H) return 0;
    if constexpr (VEC) {
        if (x < 0 || x >= W) return 0;                                      // W % 4 == 0 and x % 4 == 0: all four inside or none
        return norm4(*reinterpret_cast<const unsigned*>(src + (int64_t)y * W + x));
    } else {
        unsigned w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (x + b >= 0 && x + b < W && src[(int64_t)y * W + x + b]) w |= 255u << (8 * b);
        return w;
    }
}
// a dword's row dilated by one pixel either way: byte 0 is the smallest x
__device__ __forceinline__ unsigned hdil(unsigned prev, unsigned w, unsigned next) { return w | (w << 8) | (w >> 8) | (prev >> 24) | (next << 24); }

// grid (ceil(W / 64), ceil(H / 64), T).  a = A at the start of the pass (a0 itself in the first), out = A after `sweeps` sweeps, or with `last`
// S = that & ~a0.
template <bool VEC>
__global__ __launch_bounds__(PB) void grow_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ cand, const uint8_t* __restrict__ a0, int H,
                                                  int W, int sweeps, int last, uint8_t* __restrict__ out) {
    __shared__ unsigned plane[3][GP];       // A, A, cand
    const int64_t frame = (int64_t)blockIdx.z * H * W;
    const int y0 = (int)blockIdx.y * GT, x0 = (int)blockIdx.x * GT;
    a += frame; cand += frame; a0 += frame; out += frame;
    for (int i = threadIdx.x; i < GP; i += PB) plane[0][i] = plane[1][i] = 0;       // the rings of both A planes stay zero
    __syncthreads();
    int anyA = 0, anyC = 0;
    for (int i = threadIdx.x; i < GR * GD; i += PB) {
        const int r = i / GD, j = i % GD, at = (r + 1) * GS + j + 1;
        const int y = y0 - GK + r, x = x0 - GK + 4 * j;
        const unsigned wa = load4<VEC>(a, y, x, H, W), wc = load4<VEC>(cand, y, x, H, W);
        plane[0][at] = wa;
        plane[2][at] = wc;
        anyA |= wa != 0;
        anyC |= wc != 0 && r >= GK && r < GK + GT && j >= GK / 4 && j < (GK + GT) / 4;
    }
    // no candidate in the interior, or nothing to grow from in tile plus halo: the interior cannot change
    anyA = __syncthreads_or(anyA);
    anyC = __syncthreads_or(anyC);
    int cur = 0;
    if (anyA && anyC) {
        for (int k = 0; k < sweeps; ++k) {
            const unsigned* src = plane[cur];
            unsigned* dst = plane[cur ^ 1];
            int changed = 0;
            for (int i = threadIdx.x; i < GR * GD; i += PB) {
                const int at = (i / GD + 1) * GS + i % GD + 1;
                const unsigned w = src[at];
                const unsigned nb = hdil(src[at - GS - 1], src[at - GS], src[at - GS + 1]) | hdil(src[at - 1], w, src[at + 1]) |
                                      hdil(src[at + GS - 1], src[at + GS], src[at + GS + 1]);
                const unsigned nw = w | (plane[2][at] & nb);
                dst[at] = nw;
                changed |= nw != w;
            }
            cur ^= 1;
            if (!__syncthreads_or(changed)) break;                          // a fixed point: the sweeps left would change nothing either
        }
    }
    const unsigned* res = plane[cur];
    for (int i = threadIdx.x; i < GT * (GT / 4); i += PB) {
        const int r = i / (GT / 4), j = i % (GT / 4);
        const int y = y0 + r, x = x0 + 4 * j;
        if (y >= H || x >= W) continue;
        unsigned w = res[(r + GK + 1) * GS + j + GK / 4 + 1];
        if (last) w &= ~load4<VEC>(a0, y, x, H, W);
        if constexpr (VEC) {
            *reinterpret_cast<unsigned*>(out + (int64_t)y * W + x) = w;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (x + b < W) out[(int64_t)y * W + x + b] = (uint8_t)(w >> (8 * b));
        }
    }
}

// the arguments every entry point shares; 0 = fine
int bad_clip(const char* who, int T, int H, int W) {
    if (T < 1 || H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31)) VV_FAIL(VV_E_ARG, "%s: bad args (T >= 1, H * W < 2^31)", who);
    if (T > VVH_MAX_T) VV_FAIL(VV_E_UNSUPPORTED, "%s: T <= %d is supported, not %d", who, VVH_MAX_T, T);
    return VV_OK;
}
bool aligned(const void* p, unsigned a) { return (uintptr_t)p % a == 0; }

}  // namespace

extern "C" int vvh_abi_version(void) { return VVH_ABI_VERSION; }
extern "C" const char* vvh_last_error(void) { return vv_last_error(); }

extern "C" int vvh_plate(const uint8_t* frames, const uint8_t* notsample, int T, int H, int W, int min_samples, int tol, uint8_t* ok, uint32_t* n2,
                         uint32_t* t1, void* stream) {
    if (!frames || !notsample || !ok || !n2 || !t1 || min_samples < 1 || tol < 0)
        VV_FAIL(VV_E_ARG, "vvh_plate: bad args (no null pointer, min_samples >= 1, tol >= 0)");
    const int rc = bad_clip("vvh_plate", T, H, W);
    if (rc != VV_OK) return rc;
    if (min_samples > VVH_MAX_T || tol > VVH_MAX_TOL)
        VV_FAIL(VV_E_UNSUPPORTED, "vvh_plate: min_samples <= %d and tol <= %d are supported, not min_samples %d, tol %d", VVH_MAX_T, VVH_MAX_TOL,
                min_samples, tol);
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)H * W;
    const bool vec = W % 4 == 0 && aligned(frames, 4) && aligned(notsample, 4);
    const int64_t units = vec ? N / 4 : N;
    const dim3 grid((unsigned)((units + PB - 1) / PB));
    if (vec) hipLaunchKernelGGL(plate_kernel<true>, grid, dim3(PB), 0, st, frames, notsample, T, N, units, min_samples, tol, ok, n2, t1);
    else hipLaunchKernelGGL(plate_kernel<false>, grid, dim3(PB), 0, st, frames, notsample, T, N, units, min_samples, tol, ok, n2, t1);
    VV_CHECK_LAUNCH("vvh_plate");
    return VV_OK;
}

extern "C" int vvh_candidates(const uint8_t* frames, const uint8_t* dil, const uint8_t* ok, const uint32_t* n2, const uint32_t* t1, int T, int H, int W,
                              int lo, int hi, int drop, int chroma, int floor, uint8_t* cand, int64_t* counts, void* stream) {
    if (!frames || !dil || !ok || !n2 || !t1 || !cand || !counts || lo < 0 || hi < lo || drop < 0 || chroma < 0 || floor < 1)
        VV_FAIL(VV_E_ARG, "vvh_candidates: bad args (no null pointer, 0 <= lo <= hi, drop >= 0, chroma >= 0, floor >= 1)");
    const int rc = bad_clip("vvh_candidates", T, H, W);
    if (rc != VV_OK) return rc;
    if (hi > 100 || drop > VVH_MAX_DROP || chroma > VVH_MAX_CHROMA || floor > VVH_MAX_FLOOR)
        VV_FAIL(VV_E_UNSUPPORTED, "vvh_candidates: hi <= 100, drop <= %d, chroma <= %d and floor <= %d are supported, not hi %d, drop %d, chroma %d, floor %d",
                VVH_MAX_DROP, VVH_MAX_CHROMA, VVH_MAX_FLOOR, hi, drop, chroma, floor);
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)H * W;
    if (hipMemsetAsync(counts, 0, (size_t)T * 2 * sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vvh_candidates: memset failed");
    const bool vec = W % 4 == 0 && aligned(frames, 4) && aligned(dil, 4) && aligned(ok, 4) && aligned(cand, 4);
    const int64_t units = vec ? N / 4 : N;
    const dim3 grid((unsigned)((units + PB - 1) / PB), (unsigned)T);
    const CandArgs a{lo, hi, drop, chroma, floor};
    if (vec) hipLaunchKernelGGL(cand_kernel<true>, grid, dim3(PB), 0, st, frames, dil, ok, n2, t1, N, units, a, cand, (u64*)counts);
    else hipLaunchKernelGGL(cand_kernel<false>, grid, dim3(PB), 0, st, frames, dil, ok, n2, t1, N, units, a, cand, (u64*)counts);
    VV_CHECK_LAUNCH("vvh_candidates");
    return VV_OK;
}

extern "C" int vvh_grow(const uint8_t* a0, const uint8_t* cand, int T, int H, int W, int reach, uint8_t* ws, uint8_t* s, void* stream) {
    if (!a0 || !cand || !ws || !s || reach < 0 || ws == s || ws == a0 || ws == cand || s == a0 || s == cand)
        VV_FAIL(VV_E_ARG, "vvh_grow: bad args (no null pointer, reach >= 0, s and ws are neither each other nor an input)");
    const int rc = bad_clip("vvh_grow", T, H, W);
    if (rc != VV_OK) return rc;
    if (reach > VVH_MAX_REACH) VV_FAIL(VV_E_UNSUPPORTED, "vvh_grow: reach <= %d is supported, not %d", VVH_MAX_REACH, reach);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = W % 4 == 0 && aligned(a0, 4) && aligned(cand, 4) && aligned(ws, 4) && aligned(s, 4);
    const dim3 grid((unsigned)((W + GT - 1) / GT), (unsigned)((H + GT - 1) / GT), (unsigned)T);
    const int passes = reach == 0 ? 1 : (reach + GK - 1) / GK;
    const uint8_t* from = a0;
    for (int j = 0; j < passes; ++j) {
        const int last = j == passes - 1;
        const int sweeps = reach == 0 ? 0 : (last && reach % GK ? reach % GK : GK);
        uint8_t* to = (passes - 1 - j) % 2 == 0 ? s : ws;                    // the last pass writes s
        if (vec) hipLaunchKernelGGL(grow_kernel<true>, grid, dim3(PB), 0, st, from, cand, a0, H, W, sweeps, last, to);
        else hipLaunchKernelGGL(grow_kernel<false>, grid, dim3(PB), 0, st, from, cand, a0, H, W, sweeps, last, to);
        VV_CHECK_LAUNCH("vvh_grow");
        from = to;
    }
    return VV_OK;
}

extern "C" int vvh_merge(const uint8_t* dil, const uint8_t* s, int T, int H, int W, uint8_t* dil_out, int64_t* counts, void* stream) {
    if (!dil || !s || !dil_out || !counts || dil_out == dil) VV_FAIL(VV_E_ARG, "vvh_merge: bad args (no null pointer, dil_out is not dil)");
    const int rc = bad_clip("vvh_merge", T, H, W);
    if (rc != VV_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)H * W;
    const bool vec = W % 4 == 0 && aligned(dil, 4) && aligned(s, 4) && aligned(dil_out, 4);
    const int64_t units = vec ? N / 4 : N;
    const dim3 grid((unsigned)((units + PB - 1) / PB), (unsigned)T);
    if (vec) hipLaunchKernelGGL(merge_kernel<true>, grid, dim3(PB), 0, st, dil, s, N, units, dil_out, (u64*)counts);
    else hipLaunchKernelGGL(merge_kernel<false>, grid, dim3(PB), 0, st, dil, s, N, units, dil_out, (u64*)counts);
    VV_CHECK_LAUNCH("vvh_merge");
    return VV_OK;
}
