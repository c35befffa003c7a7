// Clean-plate warp (videovanish_amd/platewarp.py, infill.plate_fill(wcfg=)): one affine map per frame, fitted on the host to
// block-matched vectors of the visible blocks, and the clean-plate canvas built and read back through it.  The rules are include/platewarp.h's; all
// arithmetic is integer.
//   vvw_search    per (frame t, block) the lexicographic minimum of (cost, dx^2 + dy^2, dy, dx) over the valid candidates -> rec, stats
//   vvw_place     frames, masks -> canvas bytes, canvas masks, the canvas' invalid plane, every pixel read through the frame's inverse map
//   vvw_unplace   canvas -> the patch of filled bytes and the frames' masks, every pixel sent through the frame's forward map
// vvw_search follows vvk_search (vv_flicklocal.hip): a workgroup of 4 waves owns 4 adjacent blocks of one frame, one wave per block.  Each wave
// stages its block of frame t's luma (BLOCK rows x BLOCK bytes) and the key's search area under it, moved by d0 (BLOCK + 2 S rows x BLOCK + 2 S
// bytes each of luma and valid, zero where the key's plane has no pixel), in LDS as dwords; no candidate reads HBM.  Luma is one byte a pixel:
// a block row is W = BLOCK / 4 dwords, a candidate's row is the W dwords that start dx + S bytes into the area's row, made by v_alignbyte_b32
// of adjacent LDS dwords, its cost v_sad_u8 of those against the block's dwords, and its validity the same packed SAD of the valid bytes
// against zero, compared with BLOCK^2.  Lanes: an item is (dy, group of 4 adjacent dx, quarter of the block's rows); the four candidates of a
// group sit at the byte shifts 0 .. 3 of the same dwords, so a lane reads W + 1 area dwords of each plane and W block dwords of a row once and
// takes 8 W SADs from them.  The 4 lanes of a quad hold one (dy, group) and add their quarters with xor shuffles.  (2 S + 1) dy x
// ceil((2 S + 1) / 4) groups x 4 quarters: 340 items = 6 passes for S = 8.  The slots past dx = S are computed on staged bytes and dropped.
// The frame's state, key and d0 depend on blockIdx only: scalar registers.  The winner is an integer minimum of the packed 64-bit key
// (cost, dx^2 + dy^2, dy + 8, dx + 8) over the wave: no lane order enters.
#include "vv_wave_bytes.h"
#include "../../include/platewarp.h"

namespace {

using vvwave::wave_sum;
using vvwave::wave_min64;
typedef unsigned long long u64;
typedef long long i64;
constexpr int FB = 256;                     // threads per block
constexpr int WAVES = FB / 64;              // blocks per workgroup
constexpr int MAXS = VVW_MAX_SEARCH;
constexpr int MAXG = (2 * MAXS + 1 + 3) / 4;
constexpr int REC = VVW_TRACK_INTS;
static_assert(32 * 32 * 255 < (1ll << 31) && 2 * 32 * 32 * 255 < (1ll << 31), "a cost and an activity fit 31 bits");
static_assert(2 * MAXS * MAXS < 65536 && 2 * MAXS + 1 < 256, "the key's fields");

// grid (ceil(nby * nbx / WAVES), T): frame = blockIdx.y.  Reads of the planes of frame t lie inside its whole blocks; reads of the key's planes are
// bounds-checked in 64 bits (track is data); the writes are the wave's own record and the atomics into stats[t].
template <int BLOCK>
__global__ __launch_bounds__(FB) void search_kernel(const uint8_t* __restrict__ pyr, i64 stride, const int32_t* __restrict__ track, int T, int H, int W, int S,
                                                    int min_texture, int max_residual, int nby, int nbx, int32_t* __restrict__ rec, u64* __restrict__ stats) {
    constexpr int BW = BLOCK / 4;               // dwords of a block row
    constexpr int APITCH = BW + MAXG;           // dwords of a row of the area: BLOCK + 2 S bytes and the dword the last group reads past them; odd
    constexpr int AROWS = BLOCK + 2 * MAXS;
    constexpr int RPI = BLOCK / 4;              // rows per item
    static_assert(APITCH % 2 == 1 && APITCH * 4 >= BLOCK + 2 * MAXS + 4 && (MAXG - 1) + BW < APITCH, "the area's row");
    __shared__ unsigned ref[WAVES][BLOCK * BW];
    __shared__ unsigned areaY[WAVES][AROWS * APITCH];
    __shared__ unsigned areaV[WAVES][AROWS * APITCH];
    const int t = (int)blockIdx.y;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nb = nby * nbx, blk = (int)blockIdx.x * WAVES + wave;
    const bool active = blk < nb;
    int32_t* out = rec + ((i64)t * nb + blk) * VVW_REC_INTS;

    // the frame's state, key and d0: blockIdx only, scalar loads
    const int32_t* tr = track + (i64)t * REC;
    const int key = tr[2];
    const bool frame_ok = tr[3] == 1 && key >= 0 && key < T && key != t;
    if (!frame_ok) {                            // uniform over the workgroup: no barrier is skipped by a part of it
        if (active && lane < VVW_REC_INTS) out[lane] = 0;
        return;
    }
    const i64 d0x = (i64)tr[0] - track[(i64)key * REC + 0], d0y = (i64)tr[1] - track[(i64)key * REC + 1];
    const i64 HW = (i64)H * W;
    const uint8_t* tY = pyr + (i64)t * stride;
    const uint8_t* kY = pyr + (i64)key * stride;
    const int by = active ? blk / nbx : 0, bx = active ? blk - by * nbx : 0;
    const int y0 = by * BLOCK, x0 = bx * BLOCK;
    const int arows = BLOCK + 2 * S;
    unsigned nvalid = 0;

    if (active) {
        // ---- stage: the block of frame t (whole blocks only: inside the plane), and how many of its pixels are valid
        for (int i = lane; i < BLOCK * BW; i += 64) {
            const int r = i / BW, cd = i - r * BW;
            const i64 at = (i64)(y0 + r) * W + x0 + 4 * cd;
            unsigned v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                v |= (unsigned)tY[at + b] << (8 * b);
                nvalid += tY[HW + at + b] ? 1u : 0u;
            }
            ref[wave][i] = v;
        }
        // ---- stage: the key's area, moved by d0, zero (and invalid) outside the key's plane and past the area's bytes
        const i64 ay = (i64)y0 + d0y - S, ax = (i64)x0 + d0x - S;
        for (int i = lane; i < arows * APITCH; i += 64) {
            const int r = i / APITCH, cd = i - r * APITCH;
            const i64 ys = ay + r;
            unsigned vy = 0, vv = 0;
            if (ys >= 0 && ys < H) {
                const uint8_t* row = kY + ys * W;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int c = 4 * cd + b;
                    const i64 xs = ax + c;
                    if (c < arows && xs >= 0 && xs < W) {
                        vy |= (unsigned)row[xs] << (8 * b);
                        vv |= (row[HW + xs] ? 1u : 0u) << (8 * b);
                    }
                }
            }
            areaY[wave][i] = vy;
            areaV[wave][i] = vv;
        }
    }
    __syncthreads();
    if (!active) return;
    nvalid = wave_sum(nvalid);

    // ---- the block's activity: neighbour differences inside the block, from the staged bytes
    unsigned act = 0;
    {
        const uint8_t* rb = reinterpret_cast<const uint8_t*>(ref[wave]);
        for (int i = lane; i < BLOCK * BLOCK; i += 64) {
            const int r = i / BLOCK, c = i - r * BLOCK;
            const unsigned v = rb[i];
            if (c + 1 < BLOCK) act += __sad(v, (unsigned)rb[i + 1], 0u);
            if (r + 1 < BLOCK) act += __sad(v, (unsigned)rb[i + BLOCK], 0u);
        }
        act = wave_sum(act);
    }
    const bool usable = nvalid == (unsigned)(BLOCK * BLOCK) && act >= (unsigned)min_texture * (unsigned)(BLOCK * BLOCK);

    // ---- the byte SADs: item = (dy, group of 4 dx, quarter of the rows); the winner's key is kept per lane
    u64 best = ~0ull;
    if (usable) {                               // wave-uniform
        const int n1 = 2 * S + 1, groups = (n1 + 3) >> 2, items = n1 * groups * 4;
        for (int i0 = 0; i0 < items; i0 += 64) {
            const int i = i0 + lane;
            const bool live = i < items;        // a quad is live or not as a whole: items % 4 == 0
            const int q = live ? i >> 2 : 0, part = i & 3;
            const int dyi = (int)((unsigned)q / (unsigned)groups), g = q - dyi * groups;
            unsigned acc[4] = {0u, 0u, 0u, 0u}, val[4] = {0u, 0u, 0u, 0u};
            if (live) {
#pragma unroll
                for (int r = 0; r < RPI; ++r) {
                    const int row = part * RPI + r;
                    const unsigned* a = areaY[wave] + (row + dyi) * APITCH + g;
                    const unsigned* m = areaV[wave] + (row + dyi) * APITCH + g;
                    const unsigned* f = ref[wave] + row * BW;
                    unsigned av[BW + 1], mv[BW + 1];
#pragma unroll
                    for (int j = 0; j < BW + 1; ++j) { av[j] = a[j]; mv[j] = m[j]; }
#pragma unroll
                    for (int j = 0; j < BW; ++j) {  // dx slot c starts c bytes on
                        const unsigned fj = f[j];
                        acc[0] = __builtin_amdgcn_sad_u8(av[j], fj, acc[0]);
                        acc[1] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(av[j + 1], av[j], 1u), fj, acc[1]);
                        acc[2] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(av[j + 1], av[j], 2u), fj, acc[2]);
                        acc[3] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(av[j + 1], av[j], 3u), fj, acc[3]);
                        val[0] = __builtin_amdgcn_sad_u8(mv[j], 0u, val[0]);
                        val[1] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(mv[j + 1], mv[j], 1u), 0u, val[1]);
                        val[2] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(mv[j + 1], mv[j], 2u), 0u, val[2]);
                        val[3] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(mv[j + 1], mv[j], 3u), 0u, val[3]);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc[c] += __shfl_xor(acc[c], 1, 64);
                acc[c] += __shfl_xor(acc[c], 2, 64);
                val[c] += __shfl_xor(val[c], 1, 64);
                val[c] += __shfl_xor(val[c], 2, 64);
                const int dxi = 4 * g + c;
                if (live && part == 0 && dxi < n1 && val[c] == (unsigned)(BLOCK * BLOCK)) {
                    const int dy = dyi - S, dx = dxi - S;
                    const u64 k = ((u64)acc[c] << 32) | ((u64)(unsigned)(dx * dx + dy * dy) << 16) | ((u64)(unsigned)(dy + MAXS) << 8) | (u64)(unsigned)(dx + MAXS);
                    if (k < best) best = k;
                }
            }
        }
        best = wave_min64(best);
    }
    const bool won = best != ~0ull;
    const int cst = won ? (int)(best >> 32) : 0;
    const bool used = won && (unsigned)cst <= (unsigned)max_residual * (unsigned)(BLOCK * BLOCK);
    const int dy = used ? (int)((best >> 8) & 255u) - MAXS : 0, dx = used ? (int)(best & 255u) - MAXS : 0;
    if (lane < VVW_REC_INTS) out[lane] = lane == 0 ? dx : lane == 1 ? dy : lane == 2 ? (used ? 1 : 0) : (used ? cst : 0);
    if (lane == 0) {
        u64* st = stats + (i64)t * VVW_NSTAT;
        if (usable) atomicAdd(&st[0], (u64)1);
        if (used) {
            atomicAdd(&st[1], (u64)1);
            if (cst) atomicAdd(&st[2], (u64)cst);
            if (dx | dy) atomicAdd(&st[3], (u64)(abs(dx) + abs(dy)));
        }
    }
}

// rule M: one component of a map at the integer point (x, y); sums modulo 2^64, arithmetic shift
__device__ __forceinline__ i64 map_at(const int64_t* m, i64 x, i64 y) {
    const u64 s = (u64)m[0] + (u64)m[1] * (u64)x + (u64)m[2] * (u64)y + ((u64)1 << (VVW_FRAC_BITS - 1));
    return (i64)s >> VVW_FRAC_BITS;
}

// grid (ceil(ch * cw / FB), B): frame = blockIdx.y.  The read of the frame is bounds-checked; the writes are the thread's own canvas pixel.
__global__ __launch_bounds__(FB) void place_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ dil, const int64_t* __restrict__ inv,
                                                   const uint8_t* __restrict__ tracked, int H, int W, int cy0, int cx0, int ch, int cw,
                                                   uint8_t* __restrict__ canvas, uint8_t* __restrict__ dil_c, uint8_t* __restrict__ inv_c) {
    const i64 i = (i64)blockIdx.x * FB + threadIdx.x, M = (i64)ch * cw;
    if (i >= M) return;
    const i64 b = blockIdx.y;
    const int64_t* m = inv + b * VVW_MAP_INTS;
    const i64 cy = (i64)cy0 + i / cw, cx = (i64)cx0 + i % cw;
    unsigned r = 0, g = 0, bl = 0;
    uint8_t d = 0, v = 255;
    if (tracked[b]) {
        const i64 fx = map_at(m, cx, cy), fy = map_at(m + 3, cx, cy);
        if (fy >= 0 && fy < H && fx >= 0 && fx < W) {
            const i64 at = (b * H + fy) * W + fx;
            const uint8_t* px = frames + at * 3;
            r = px[0]; g = px[1]; bl = px[2];
            d = dil[at];
            v = 0;
        }
    }
    uint8_t* o = canvas + (b * M + i) * 3;
    o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)bl;
    dil_c[b * M + i] = d;
    inv_c[b * M + i] = v;
}

// grid (ceil(H * W / FB), T): frame = blockIdx.y.  The reads of the canvas are bounds-checked; the writes are the thread's own mask byte and, inside
// the patch box, its own patch pixel.
__global__ __launch_bounds__(FB) void unplace_kernel(const uint8_t* __restrict__ canvas, const uint8_t* __restrict__ dil_c, const uint8_t* __restrict__ dil_out_c,
                                                     const uint8_t* __restrict__ dil, const int64_t* __restrict__ fwd, const uint8_t* __restrict__ tracked, int H,
                                                     int W, int cy0, int cx0, int ch, int cw, int py0, int px0, int ph, int pw, uint8_t* __restrict__ patch,
                                                     uint8_t* __restrict__ dil_out) {
    const i64 i = (i64)blockIdx.x * FB + threadIdx.x, N = (i64)H * W;
    if (i >= N) return;
    const i64 t = blockIdx.y;
    const int y = (int)(i / W), x = (int)(i % W);
    const uint8_t d = dil[t * N + i];
    unsigned r = 0, g = 0, bl = 0;
    bool filled = false;
    if (tracked[t] && d) {
        const int64_t* m = fwd + t * VVW_MAP_INTS;
        const i64 jx = map_at(m, x, y) - cx0, jy = map_at(m + 3, x, y) - cy0;
        if (jy >= 0 && jy < ch && jx >= 0 && jx < cw) {
            const i64 at = (t * ch + jy) * cw + jx;
            if (dil_c[at] && !dil_out_c[at]) {
                const uint8_t* px = canvas + at * 3;
                r = px[0]; g = px[1]; bl = px[2];
                filled = true;
            }
        }
    }
    dil_out[t * N + i] = filled ? 0 : d;
    const int qy = y - py0, qx = x - px0;
    if (qy >= 0 && qy < ph && qx >= 0 && qx < pw) {
        uint8_t* o = patch + ((t * ph + qy) * pw + qx) * 3;
        o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)bl;
    }
}

int bad_sizes(const char* who, int T, int H, int W, int ch, int cw) {
    if (T < 1 || H < 1 || W < 1 || ch < 1 || cw < 1) VV_FAIL(VV_E_ARG, "%s: bad args (T, H, W, ch, cw >= 1)", who);
    if (T > VVW_MAX_T || (int64_t)H * W > VVW_MAX_PIXELS || (int64_t)ch * cw >= ((int64_t)1 << 31))
        VV_FAIL(VV_E_UNSUPPORTED, "%s: T <= %d, H * W <= %d and ch * cw < 2^31 are supported, not T %d, %d x %d, canvas %d x %d", who, VVW_MAX_T, VVW_MAX_PIXELS,
                T, H, W, ch, cw);
    return VV_OK;
}

}  // namespace

extern "C" int vvw_abi_version(void) { return VVW_ABI_VERSION; }
extern "C" const char* vvw_last_error(void) { return vv_last_error(); }

extern "C" int vvw_search(const uint8_t* pyr, int64_t stride, const int32_t* track, int T, int H, int W, int block, int search, int min_texture, int max_residual,
                          int32_t* rec, int64_t* stats, void* stream) {
    if (!pyr || !track || !stats || T < 1 || H < 1 || W < 1 || block < 1 || search < 0 || min_texture < 0 || max_residual < 0 ||
        (!rec && H / block > 0 && W / block > 0))
        VV_FAIL(VV_E_ARG, "vvw_search: bad args (no null pointer but rec without a block, T, H, W, block >= 1, search, min_texture, max_residual >= 0)");
    if ((block != 16 && block != 32) || search > VVW_MAX_SEARCH || min_texture > 510 || max_residual > 255 || T > VVW_MAX_T ||
        (int64_t)H * W > VVW_MAX_PIXELS || stride < 2 * (int64_t)H * W)
        VV_FAIL(VV_E_UNSUPPORTED, "vvw_search: block 16 or 32, search <= %d, min_texture <= 510, max_residual <= 255, T <= %d, H * W <= %d and stride >= 2 H W "
                "are supported, not block %d, search %d, min_texture %d, max_residual %d, T %d, %d x %d, stride %lld", VVW_MAX_SEARCH, VVW_MAX_T, VVW_MAX_PIXELS,
                block, search, min_texture, max_residual, T, H, W, (long long)stride);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(stats, 0, (size_t)T * VVW_NSTAT * sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vvw_search: memset failed");
    const int nby = H / block, nbx = W / block, nb = nby * nbx;
    if (nb == 0) return VV_OK;
    const dim3 grid((unsigned)((nb + WAVES - 1) / WAVES), (unsigned)T);
    if (block == 16)
        hipLaunchKernelGGL(search_kernel<16>, grid, dim3(FB), 0, st, pyr, (i64)stride, track, T, H, W, search, min_texture, max_residual, nby, nbx, rec, (u64*)stats);
    else
        hipLaunchKernelGGL(search_kernel<32>, grid, dim3(FB), 0, st, pyr, (i64)stride, track, T, H, W, search, min_texture, max_residual, nby, nbx, rec, (u64*)stats);
    VV_CHECK_LAUNCH("vvw_search");
    return VV_OK;
}

extern "C" int vvw_place(const uint8_t* frames, const uint8_t* dil, const int64_t* inv, const uint8_t* tracked, int B, int H, int W, int cy0, int cx0, int ch,
                         int cw, uint8_t* canvas, uint8_t* dil_c, uint8_t* invalid_c, void* stream) {
    if (!frames || !dil || !inv || !tracked || !canvas || !dil_c || !invalid_c) VV_FAIL(VV_E_ARG, "vvw_place: bad args (no null pointer)");
    const int rc = bad_sizes("vvw_place", B, H, W, ch, cw);
    if (rc != VV_OK) return rc;
    const dim3 grid((unsigned)(((int64_t)ch * cw + FB - 1) / FB), (unsigned)B);
    hipLaunchKernelGGL(place_kernel, grid, dim3(FB), 0, (hipStream_t)stream, frames, dil, inv, tracked, H, W, cy0, cx0, ch, cw, canvas, dil_c, invalid_c);
    VV_CHECK_LAUNCH("vvw_place");
    return VV_OK;
}

extern "C" int vvw_unplace(const uint8_t* canvas, const uint8_t* dil_c, const uint8_t* dil_out_c, const uint8_t* dil, const int64_t* fwd, const uint8_t* tracked,
                           int T, int H, int W, int cy0, int cx0, int ch, int cw, int py0, int px0, int ph, int pw, uint8_t* patch, uint8_t* dil_out,
                           void* stream) {
    if (!canvas || !dil_c || !dil_out_c || !dil || !fwd || !tracked || !patch || !dil_out || dil_out == dil)
        VV_FAIL(VV_E_ARG, "vvw_unplace: bad args (no null pointer, dil_out is not dil)");
    int rc = bad_sizes("vvw_unplace", T, H, W, ch, cw);
    if (rc != VV_OK) return rc;
    if (ph < 1 || pw < 1 || py0 < 0 || px0 < 0 || (int64_t)py0 + ph > H || (int64_t)px0 + pw > W)
        VV_FAIL(VV_E_ARG, "vvw_unplace: bad args (the patch box %d, %d + %d x %d must be non-empty and inside the %d x %d frame)", py0, px0, ph, pw, H, W);
    const dim3 grid((unsigned)(((int64_t)H * W + FB - 1) / FB), (unsigned)T);
    hipLaunchKernelGGL(unplace_kernel, grid, dim3(FB), 0, (hipStream_t)stream, canvas, dil_c, dil_out_c, dil, fwd, tracked, H, W, cy0, cx0, ch, cw, py0, px0, ph,
                       pw, patch, dil_out);
    VV_CHECK_LAUNCH("vvw_unplace");
    return VV_OK;
}
