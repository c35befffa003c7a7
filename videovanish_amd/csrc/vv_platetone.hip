// Clean-plate exposure matching (videovanish_amd/platetone.py, infill.plate_fill(tcfg=)): the device steps round the host's
// per-frame fit.  The rules are include/platetone.h's; all arithmetic is integer.
//   vve_mean_plane   per pixel along time: the rounded mean R of all T frames, the support U (never a non-sample, no channel near clipping), n
//   vve_moments      per frame: Sv, Svr over U; the blocks of frame 0 also add Sr, Srr
//   vve_apply        per frame: out = G_t[f] through the frame's table in LDS; an identity frame is copied
//   vve_restore      per frame: out = B_t[f''] where the fill took the pixel out of the mask, else f
// A streaming family over [T][H][W][3] u8.  A unit is P adjacent pixels (VEC: P = 4, one 12-byte image load and one 4-byte mask load, lane after
// lane contiguous; W % 4 == 0 and 4-byte aligned bases, checked by the launcher; else P = 1 with byte loads).  Nothing here depends on a
// pixel's row or column.  vve_mean_plane gives a thread one unit and walks the frames in registers; the other three lay a capped grid over
// (units, T) and stride it, so that a block's 768-byte table and its atomics are paid once for many units.  The sums go registers -> wave
// reduction -> LDS -> one 64-bit global atomic per block and quantity, as in vv_tone.hip: integer adds in any order.
#include "vv_common.h"
#include "vv_wave_bytes.h"
#include "../../include/platetone.h"

namespace {

using vvwave::load_mask;
using vvwave::load_px;
using vvwave::store_px;
using vvwave::wave_sum;
using vvwave::wave_sum64;
using vvwave::U3;
constexpr int PB = 256;                     // threads per block
constexpr int MAX_PX = 8192;                // pixels a thread of vve_moments adds up in 32 bits
typedef unsigned long long u64;
static_assert((u64)VVE_MAX_T * 255 < (1ull << 32), "P in 32 bits");
static_assert((u64)MAX_PX * 255 * 255 < (1ull << 32), "a thread's Svr in 32 bits");
static_assert((u64)VVE_MAX_PIXELS * 255 * 255 < (1ull << 40), "Svr and Srr below 2^40");

// frame t's three 256-byte tables into LDS; the caller synchronises
__device__ __forceinline__ void stage_table(const uint8_t* __restrict__ tabs, int t, unsigned* lds) {
    const unsigned* src = reinterpret_cast<const unsigned*>(tabs + (int64_t)t * 768);       // [T][3][256] u8 from a 4-byte aligned base (the launcher)
    if (threadIdx.x < 192) lds[threadIdx.x] = src[threadIdx.x];
}

template <bool VEC>
__global__ __launch_bounds__(PB) void mean_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ ns, int T, int64_t N, int64_t units,
                                                  int floor, uint8_t* __restrict__ mean, uint8_t* __restrict__ support, u64* __restrict__ n_out) {
    constexpr int P = VEC ? 4 : 1;
    __shared__ unsigned tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    const int64_t u = (int64_t)blockIdx.x * PB + threadIdx.x;
    unsigned cnt = 0;
    if (u < units) {
        const int64_t i0 = u * P;
        unsigned sum[3 * P], seen = 0;          // seen: byte p != 0 when some frame is no sample of pixel p
#pragma unroll
        for (int j = 0; j < 3 * P; ++j) sum[j] = 0;
        for (int t = 0; t < T; ++t) {
            seen |= load_mask<VEC>(ns + (int64_t)t * N + i0);
            unsigned v[3 * P];
            load_px<VEC>(frames + ((int64_t)t * N + i0) * 3, v);
#pragma unroll
            for (int j = 0; j < 3 * P; ++j) sum[j] += v[j];
        }
        unsigned r[3 * P], um = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            bool in = ((seen >> (8 * p)) & 255u) == 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned q = sum[3 * p + c] / (unsigned)T, rem = sum[3 * p + c] % (unsigned)T;
                const unsigned m = q + (2u * rem >= (unsigned)T ? 1u : 0u);          // (2 P + T) // (2 T)
                r[3 * p + c] = m;
                in = in && (int)m >= floor && (int)m <= 255 - floor;
            }
            um |= (in ? 1u : 0u) << (8 * p);
            cnt += in ? 1u : 0u;
        }
        store_px<VEC>(mean + i0 * 3, r);
        vvwave::store_mask<VEC>(support + i0, um);
    }
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&tot, cnt);
    __syncthreads();
    if (threadIdx.x == 0 && tot) atomicAdd(n_out, (u64)tot);
}

// grid (bx, T): block (b, t) strides the units of frame t.  Frame 0's blocks add Sr and Srr as well.
template <bool VEC>
__global__ __launch_bounds__(PB) void moments_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ mean, const uint8_t* __restrict__ support,
                                                     int64_t N, int64_t units, u64* __restrict__ sums) {
    constexpr int P = VEC ? 4 : 1;
    __shared__ u64 tot[VVE_NSUM];
    const int t = (int)blockIdx.y;
    if (threadIdx.x < VVE_NSUM) tot[threadIdx.x] = 0;
    __syncthreads();
    unsigned acc[VVE_NSUM];
#pragma unroll
    for (int i = 0; i < VVE_NSUM; ++i) acc[i] = 0;
    const uint8_t* f = frames + (int64_t)t * N * 3;
    for (int64_t u = (int64_t)blockIdx.x * PB + threadIdx.x; u < units; u += (int64_t)gridDim.x * PB) {
        const int64_t i0 = u * P;
        const unsigned um = load_mask<VEC>(support + i0);
        if (!um) continue;
        unsigned v[3 * P], r[3 * P];
        load_px<VEC>(f + i0 * 3, v);
        load_px<VEC>(mean + i0 * 3, r);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const bool in = ((um >> (8 * p)) & 255u) != 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned x = in ? v[3 * p + c] : 0u, m = in ? r[3 * p + c] : 0u;
                acc[c] += x; acc[3 + c] += x * m;
                acc[6 + c] += m; acc[9 + c] += m * m;
            }
        }
    }
    const int nq = t == 0 ? VVE_NSUM : 6;       // block-uniform
#pragma unroll
    for (int i = 0; i < VVE_NSUM; ++i) {
        if (i >= nq) break;
        const u64 s = wave_sum64((u64)acc[i]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&tot[i], s);
    }
    __syncthreads();
    if ((int)threadIdx.x < nq && tot[threadIdx.x]) atomicAdd(&sums[(int64_t)t * VVE_NSUM + threadIdx.x], tot[threadIdx.x]);
}

template <bool VEC>
__global__ __launch_bounds__(PB) void apply_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ fwd, const uint8_t* __restrict__ identity,
                                                   int64_t N, int64_t units, uint8_t* __restrict__ out) {
    constexpr int P = VEC ? 4 : 1;
    __shared__ unsigned tabw[192];
    const int t = (int)blockIdx.y;
    const bool same = identity[t] != 0;          // block-uniform
    if (!same) stage_table(fwd, t, tabw);
    __syncthreads();
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tabw);
    const uint8_t* f = frames + (int64_t)t * N * 3;
    uint8_t* o = out + (int64_t)t * N * 3;
    for (int64_t u = (int64_t)blockIdx.x * PB + threadIdx.x; u < units; u += (int64_t)gridDim.x * PB) {
        const int64_t i0 = u * P;
        unsigned v[3 * P];
        load_px<VEC>(f + i0 * 3, v);
        if (!same) {
#pragma unroll
            for (int j = 0; j < 3 * P; ++j) v[j] = tab[(j % 3) * 256 + v[j]];
        }
        store_px<VEC>(o + i0 * 3, v);
    }
}

template <bool VEC>
__global__ __launch_bounds__(PB) void restore_kernel(const uint8_t* __restrict__ orig, const uint8_t* __restrict__ filled, const uint8_t* __restrict__ dil,
                                                     const uint8_t* __restrict__ dil2, const uint8_t* __restrict__ back, int64_t N, int64_t units,
                                                     uint8_t* __restrict__ out) {
    constexpr int P = VEC ? 4 : 1;
    __shared__ unsigned tabw[192];
    const int t = (int)blockIdx.y;
    stage_table(back, t, tabw);
    __syncthreads();
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tabw);
    const int64_t base = (int64_t)t * N;
    for (int64_t u = (int64_t)blockIdx.x * PB + threadIdx.x; u < units; u += (int64_t)gridDim.x * PB) {
        const int64_t at = base + u * P;
        unsigned v[3 * P];
        load_px<VEC>(orig + at * 3, v);
        const unsigned md = load_mask<VEC>(dil + at);
        if (md) {                                                                   // an unmasked unit reads neither dil2 nor the filled crop
            const unsigned m2 = load_mask<VEC>(dil2 + at);
            unsigned go = 0;
#pragma unroll
            for (int p = 0; p < P; ++p) go |= ((((md >> (8 * p)) & 255u) != 0 && ((m2 >> (8 * p)) & 255u) == 0) ? 1u : 0u) << p;
            if (go) {
                unsigned w[3 * P];
                load_px<VEC>(filled + at * 3, w);
#pragma unroll
                for (int j = 0; j < 3 * P; ++j)
                    if ((go >> (j / 3)) & 1u) v[j] = tab[(j % 3) * 256 + w[j]];
            }
        }
        store_px<VEC>(out + at * 3, v);
    }
}

// the arguments every entry point shares; 0 = fine
int bad_clip(const char* who, int T, int H, int W) {
    if (T < 1 || H < 1 || W < 1) VV_FAIL(VV_E_ARG, "%s: bad args (T >= 1, H >= 1, W >= 1)", who);
    if (T > VVE_MAX_T || (int64_t)H * W > VVE_MAX_PIXELS)
        VV_FAIL(VV_E_UNSUPPORTED, "%s: T <= %d and H * W <= 2^24 are supported, not T %d, H %d, W %d", who, VVE_MAX_T, T, H, W);
    return VV_OK;
}
bool aligned(const void* p) { return (uintptr_t)p % 4 == 0; }
// blocks along the units of one frame: at least 8 and about 4096 over the T frames, never more than the frame has, and few enough strides
unsigned blocks_x(int64_t units, int T) {
    const int64_t nb = (units + PB - 1) / PB;
    const int64_t want = (4096 + T - 1) / T < 8 ? 8 : (4096 + T - 1) / T;
    return (unsigned)(nb < want ? nb : want);
}
static_assert(((int64_t)VVE_MAX_PIXELS / PB + 7) / 8 <= MAX_PX, "at least 8 blocks stride a frame of more than 8 blocks: the pixels of one thread");

}  // namespace

extern "C" int vve_abi_version(void) { return VVE_ABI_VERSION; }
extern "C" const char* vve_last_error(void) { return vv_last_error(); }

extern "C" int vve_mean_plane(const uint8_t* frames, const uint8_t* notsample, int T, int H, int W, int floor, uint8_t* mean, uint8_t* support, int64_t* n,
                              void* stream) {
    if (!frames || !notsample || !mean || !support || !n || floor < 0) VV_FAIL(VV_E_ARG, "vve_mean_plane: bad args (no null pointer, floor >= 0)");
    const int rc = bad_clip("vve_mean_plane", T, H, W);
    if (rc != VV_OK) return rc;
    if (floor > VVE_MAX_FLOOR) VV_FAIL(VV_E_UNSUPPORTED, "vve_mean_plane: floor <= %d is supported, not %d", VVE_MAX_FLOOR, floor);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(n, 0, sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vve_mean_plane: memset failed");
    const int64_t N = (int64_t)H * W;
    const bool vec = W % 4 == 0 && aligned(frames) && aligned(notsample) && aligned(mean) && aligned(support);
    const int64_t units = vec ? N / 4 : N;
    const dim3 grid((unsigned)((units + PB - 1) / PB));
    if (vec) hipLaunchKernelGGL(mean_kernel<true>, grid, dim3(PB), 0, st, frames, notsample, T, N, units, floor, mean, support, (u64*)n);
    else hipLaunchKernelGGL(mean_kernel<false>, grid, dim3(PB), 0, st, frames, notsample, T, N, units, floor, mean, support, (u64*)n);
    VV_CHECK_LAUNCH("vve_mean_plane");
    return VV_OK;
}

extern "C" int vve_moments(const uint8_t* frames, const uint8_t* mean, const uint8_t* support, int T, int H, int W, int64_t* sums, void* stream) {
    if (!frames || !mean || !support || !sums) VV_FAIL(VV_E_ARG, "vve_moments: bad args (no null pointer)");
    const int rc = bad_clip("vve_moments", T, H, W);
    if (rc != VV_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, (size_t)T * VVE_NSUM * sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vve_moments: memset failed");
    const int64_t N = (int64_t)H * W;
    const bool vec = W % 4 == 0 && aligned(frames) && aligned(mean) && aligned(support);
    const int64_t units = vec ? N / 4 : N;
    const dim3 grid(blocks_x(units, T), (unsigned)T);
    if (vec) hipLaunchKernelGGL(moments_kernel<true>, grid, dim3(PB), 0, st, frames, mean, support, N, units, (u64*)sums);
    else hipLaunchKernelGGL(moments_kernel<false>, grid, dim3(PB), 0, st, frames, mean, support, N, units, (u64*)sums);
    VV_CHECK_LAUNCH("vve_moments");
    return VV_OK;
}

extern "C" int vve_apply(const uint8_t* frames, const uint8_t* fwd, const uint8_t* identity, int T, int H, int W, uint8_t* out, void* stream) {
    if (!frames || !fwd || !identity || !out || out == frames) VV_FAIL(VV_E_ARG, "vve_apply: bad args (no null pointer, out is not frames)");
    if (!aligned(fwd)) VV_FAIL(VV_E_ARG, "vve_apply: bad args (the tables start at a multiple of 4 bytes)");
    const int rc = bad_clip("vve_apply", T, H, W);
    if (rc != VV_OK) return rc;
    const int64_t N = (int64_t)H * W;
    const bool vec = W % 4 == 0 && aligned(frames) && aligned(out);
    const int64_t units = vec ? N / 4 : N;
    const dim3 grid(blocks_x(units, T), (unsigned)T);
    if (vec) hipLaunchKernelGGL(apply_kernel<true>, grid, dim3(PB), 0, (hipStream_t)stream, frames, fwd, identity, N, units, out);
    else hipLaunchKernelGGL(apply_kernel<false>, grid, dim3(PB), 0, (hipStream_t)stream, frames, fwd, identity, N, units, out);
    VV_CHECK_LAUNCH("vve_apply");
    return VV_OK;
}

extern "C" int vve_restore(const uint8_t* orig, const uint8_t* filled, const uint8_t* dil, const uint8_t* dil2, const uint8_t* back, int T, int H, int W,
                           uint8_t* out, void* stream) {
    if (!orig || !filled || !dil || !dil2 || !back || !out || out == orig || out == filled)
        VV_FAIL(VV_E_ARG, "vve_restore: bad args (no null pointer, out is neither orig nor filled)");
    if (!aligned(back)) VV_FAIL(VV_E_ARG, "vve_restore: bad args (the tables start at a multiple of 4 bytes)");
    const int rc = bad_clip("vve_restore", T, H, W);
    if (rc != VV_OK) return rc;
    const int64_t N = (int64_t)H * W;
    const bool vec = W % 4 == 0 && aligned(orig) && aligned(filled) && aligned(dil) && aligned(dil2) && aligned(out);
    const int64_t units = vec ? N / 4 : N;
    const dim3 grid(blocks_x(units, T), (unsigned)T);
    if (vec) hipLaunchKernelGGL(restore_kernel<true>, grid, dim3(PB), 0, (hipStream_t)stream, orig, filled, dil, dil2, back, N, units, out);
    else hipLaunchKernelGGL(restore_kernel<false>, grid, dim3(PB), 0, (hipStream_t)stream, orig, filled, dil, dil2, back, N, units, out);
    VV_CHECK_LAUNCH("vve_restore");
    return VV_OK;
}
