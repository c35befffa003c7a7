// Mask-span inference (videovanish_amd/spans.py): the cut statistics of a clip, for the hard-cut detector (spans.find_cuts).
//   vvs_frame_pair_stats   for every adjacent frame pair: pixel count, luma sum of absolute differences and the two 64-bin luma histograms, over the
//                          pixels that are unmasked in both frames (the object that is about to be removed must not vote for a cut)
// An HBM-bound streaming kernel: grid (blocks per pair, T - 1), each block owns a contiguous pixel range of its pair.  Where the frame size allows it
// (H * W a multiple of 16, so every frame starts on a 16-byte boundary) a thread takes 16 pixels per step with three 16-byte loads per frame and one per
// mask; otherwise one pixel per step.  Every accumulation is an integer add -- registers, then LDS atomics, then one set of global integer atomics
// per block -- so the result is independent of the order of threads and blocks and equals the numpy restatement bit for bit (as vv_mask_bbox's min / max).
#include "vv_common.h"
#include "vv_wave_bytes.h"
#include "../../include/vvspans.h"

namespace {

using vvwave::luma;
using vvwave::wave_sum;
constexpr int SB = 256;                    // threads per block
constexpr int BINS = VVS_HIST_BINS;
constexpr int REP = 16;                    // LDS copies of the block's two histograms: thread i adds into copy i % REP (fewer same-address adds)
constexpr int PX_PER_BLOCK = 32768;        // at most this many pixels per block (+ rounding): 255 * pixels stays far below 2^32 in the 32-bit partials

// a thread's partial sums; its histogram adds are run-length merged (neighbouring pixels mostly share a bin): (bin, count) pending per frame
struct Acc {
    unsigned n = 0, sad = 0;
    int bin[2] = {0, 0};
    unsigned cnt[2] = {0, 0};
};
__device__ __forceinline__ void flush(Acc& s, int f, unsigned* lh, int rep) {
    if (s.cnt[f]) atomicAdd(&lh[(f * BINS + s.bin[f]) * REP + rep], s.cnt[f]);
    s.cnt[f] = 0;
}
__device__ __forceinline__ void add_px(Acc& s, unsigned ya, unsigned yb, unsigned* lh, int rep) {
    s.n += 1;
    s.sad += ya > yb ? ya - yb : yb - ya;
    const int ba = (int)(ya >> 2), bb = (int)(yb >> 2);
    if (ba != s.bin[0]) { flush(s, 0, lh, rep); s.bin[0] = ba; }
    if (bb != s.bin[1]) { flush(s, 1, lh, rep); s.bin[1] = bb; }
    s.cnt[0] += 1; s.cnt[1] += 1;
}
__device__ __forceinline__ unsigned byte_of(const unsigned* w, int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 255u; }
__device__ __forceinline__ void load48(const uint8_t* p, unsigned* w) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint4 v = q[k];
        w[k * 4 + 0] = v.x; w[k * 4 + 1] = v.y; w[k * 4 + 2] = v.z; w[k * 4 + 3] = v.w;
    }
}

// grid (nblk, T - 1).  VEC: units of 16 pixels, N % 16 == 0 and 16-byte aligned bases (checked by the launcher); else units of one pixel.  Block b of
// pair p reads units [b * per, min(units, (b + 1) * per)) of frames p and p + 1 (and of their masks): every read lies inside those two frames.
template <bool VEC>
__global__ __launch_bounds__(SB) void pair_stats_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ mask, int64_t N, int64_t units,
                                                        int64_t per, unsigned long long* __restrict__ n_sad, unsigned* __restrict__ hist) {
    __shared__ unsigned lh[2 * BINS * REP];
    __shared__ unsigned tot[2];
    for (int i = threadIdx.x; i < 2 * BINS * REP; i += SB) lh[i] = 0;
    if (threadIdx.x < 2) tot[threadIdx.x] = 0;
    __syncthreads();
    const int p = blockIdx.y;
    const uint8_t* fa = frames + (int64_t)p * N * 3;
    const uint8_t* fb = fa + N * 3;
    const uint8_t* ma = mask ? mask + (int64_t)p * N : nullptr;
    const uint8_t* mb = mask ? ma + N : nullptr;
    const int rep = threadIdx.x % REP;
    const int64_t u0 = (int64_t)blockIdx.x * per;
    const int64_t u1 = min(units, u0 + per);
    Acc s;
    for (int64_t u = u0 + threadIdx.x; u < u1; u += SB) {
        if constexpr (VEC) {
            unsigned wa[12], wb[12], m[4] = {0, 0, 0, 0};
            load48(fa + u * 48, wa);
            load48(fb + u * 48, wb);
            if (mask) {
                const uint4 x = *reinterpret_cast<const uint4*>(ma + u * 16), y = *reinterpret_cast<const uint4*>(mb + u * 16);
                m[0] = x.x | y.x; m[1] = x.y | y.y; m[2] = x.z | y.z; m[3] = x.w | y.w;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (byte_of(m, i)) continue;
                add_px(s, luma(byte_of(wa, 3 * i), byte_of(wa, 3 * i + 1), byte_of(wa, 3 * i + 2)),
                       luma(byte_of(wb, 3 * i), byte_of(wb, 3 * i + 1), byte_of(wb, 3 * i + 2)), lh, rep);
            }
        } else {
            if (mask && (ma[u] | mb[u])) continue;
            const uint8_t* a = fa + u * 3;
            const uint8_t* b = fb + u * 3;
            add_px(s, luma(a[0], a[1], a[2]), luma(b[0], b[1], b[2]), lh, rep);
        }
    }
    flush(s, 0, lh, rep);
    flush(s, 1, lh, rep);
    const unsigned wn = wave_sum(s.n), ws = wave_sum(s.sad);
    if ((threadIdx.x & 63) == 0 && wn) { atomicAdd(&tot[0], wn); atomicAdd(&tot[1], ws); }
    __syncthreads();
    if (tot[0] == 0) return;                                       // nothing counted in this block: nothing to add
    if (threadIdx.x < 2) atomicAdd(&n_sad[(int64_t)p * 2 + threadIdx.x], (unsigned long long)tot[threadIdx.x]);
    if (threadIdx.x < 2 * BINS) {
        unsigned v = 0;
#pragma unroll
        for (int r = 0; r < REP; ++r) v += lh[threadIdx.x * REP + r];
        if (v) atomicAdd(&hist[(int64_t)p * 2 * BINS + threadIdx.x], v);
    }
}

}  // namespace

extern "C" int vvs_abi_version(void) { return VVS_ABI_VERSION; }
extern "C" const char* vvs_last_error(void) { return vv_last_error(); }

extern "C" int vvs_frame_pair_stats(const uint8_t* frames, const uint8_t* mask2d, int T, int H, int W, int64_t* n_sad, int32_t* hist, void* stream) {
    if (!frames || !n_sad || !hist || T < 2 || T > 65536 || H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31))
        VV_FAIL(VV_E_ARG, "vvs_frame_pair_stats: bad args");
    hipStream_t st = (hipStream_t)stream;
    const int pairs = T - 1;
    const int64_t N = (int64_t)H * W;
    if (hipMemsetAsync(n_sad, 0, (size_t)pairs * 2 * sizeof(int64_t), st) != hipSuccess ||
        hipMemsetAsync(hist, 0, (size_t)pairs * 2 * BINS * sizeof(int32_t), st) != hipSuccess)
        VV_FAIL(VV_E_LAUNCH, "vvs_frame_pair_stats: memset failed");
    // blocks per pair: PX_PER_BLOCK pixels each, more (down to one 16-pixel step per thread) while the grid has fewer than ~1024 blocks
    int64_t nblk = (N + PX_PER_BLOCK - 1) / PX_PER_BLOCK;
    const int64_t want = (1024 + pairs - 1) / pairs, cap = (N + SB * 16 - 1) / (SB * 16);
    if (nblk < want) nblk = want < cap ? want : cap;
    const bool vec = N % 16 == 0 && (uintptr_t)frames % 16 == 0 && (!mask2d || (uintptr_t)mask2d % 16 == 0);
    const int64_t units = vec ? N / 16 : N;
    const int64_t per = (units + nblk - 1) / nblk;
    const dim3 grid((unsigned)nblk, (unsigned)pairs);
    if (vec)
        hipLaunchKernelGGL(pair_stats_kernel<true>, grid, dim3(SB), 0, st, frames, mask2d, N, units, per, (unsigned long long*)n_sad, (unsigned*)hist);
    else
        hipLaunchKernelGGL(pair_stats_kernel<false>, grid, dim3(SB), 0, st, frames, mask2d, N, units, per, (unsigned long long*)n_sad, (unsigned*)hist);
    VV_CHECK_LAUNCH("vvs_frame_pair_stats");
    return VV_OK;
}
