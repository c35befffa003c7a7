// Clean-plate alignment (videovanish_amd/platealign.py, infill.plate_fill(acfg=)): one integer translation per frame of a
// panning shot, and the frames' masks laid out on a common canvas on which vv_plate.hip runs unchanged.  The rules are include/vvalign.h's; all
// arithmetic is integer.
//   vva_pyramid        per frame: luma + valid at level 0 (4-pixel ownership, one 12-byte image load and one 4-byte mask load, as vv_plate.hip; a
//                      byte path for the rest), then one 2 x 2 reduction per level
//   vva_sad            per level of one frame pair: (sad, n) of every candidate.  A block owns a 16 x 64 tile of frame t's plane, stages the key's
//                      tile shifted by the centre with a halo of r in LDS, keeps its own 4 pixels per thread in registers and walks the candidates:
//                      registers -> wave reduction -> LDS -> one pair of 64-bit global atomics per candidate and block.  Integer adds in any order.
//   vva_pick           one wave: the total order of vvalign.h over the candidates, the record of frame t and the start of frame t + 1
//   vva_track          the launcher: every vva_sad / vva_pick of a segment on one stream; centre, key and state live in `track` on the device
//   vva_place_masks    frame masks -> canvas masks and the canvas' invalid plane
//   vva_unplace_mask   canvas masks -> frame masks
#include "vv_common.h"
#include "vv_wave_bytes.h"
#include "../../include/vvalign.h"

namespace {

using vvwave::U3;
using vvwave::luma;
using vvwave::wave_sum;
constexpr int PB = 256;                      // threads per block of the streaming kernels
constexpr int TW = 64, TH = 16;              // vva_sad: the tile of frame t's plane a block owns; 256 threads x 4 adjacent pixels
constexpr int MAXR = VVA_MAX_RADIUS;
constexpr int LW = TW + 2 * MAXR, LH = TH + 2 * MAXR;
constexpr int MAXC = (2 * MAXR + 1) * (2 * MAXR + 1);
constexpr int REC = VVA_TRACK_INTS;
constexpr int CLIM = 1 << 24;                // a centre further out than any plane is wide: the record is not this unit's
typedef unsigned long long u64;
static_assert(TW * TH == PB * 4, "4 pixels per thread");
static_assert(TW * TH * 255 < (1 << 20) && TW * TH < (1 << 11), "a block's sad and n share 32 bits");

struct Geo {
    int Hl[VVA_MAX_LEVELS + 1], Wl[VVA_MAX_LEVELS + 1];
    int64_t o[VVA_MAX_LEVELS + 1], S;
};

// grid (ceil(units / PB), B): frame = blockIdx.y
template <bool VEC>
__global__ __launch_bounds__(PB) void luma_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ dil, int64_t N, int64_t units, int64_t S,
                                                  uint8_t* __restrict__ pyr) {
    const int64_t u = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (u >= units) return;
    const int64_t b = blockIdx.y;
    uint8_t* rec = pyr + b * S;
    if constexpr (VEC) {
        const int64_t i0 = u * 4;
        const U3 q = *reinterpret_cast<const U3*>(frames + (b * N + i0) * 3);
        const unsigned m = *reinterpret_cast<const unsigned*>(dil + b * N + i0);
        const unsigned w[3] = {q.a, q.b, q.c};
        unsigned v[12], y = 0, ok = 0;
#pragma unroll
        for (int j = 0; j < 12; ++j) v[j] = (w[j >> 2] >> ((j & 3) * 8)) & 255u;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            y |= luma(v[3 * p], v[3 * p + 1], v[3 * p + 2]) << (8 * p);
            ok |= (((m >> (8 * p)) & 255u) == 0 ? 1u : 0u) << (8 * p);
        }
        *reinterpret_cast<unsigned*>(rec + i0) = y;
        *reinterpret_cast<unsigned*>(rec + N + i0) = ok;
    } else {
        const uint8_t* px = frames + (b * N + u) * 3;
        rec[u] = (uint8_t)luma(px[0], px[1], px[2]);
        rec[N + u] = dil[b * N + u] == 0 ? 1 : 0;
    }
}

// level l from level l - 1 (Hp x Wp at op): grid (ceil(Hl * Wl / PB), B)
__global__ __launch_bounds__(PB) void down_kernel(uint8_t* pyr, int64_t S, int64_t op, int Hp, int Wp, int64_t ol, int Hl, int Wl) {
    const int i = blockIdx.x * PB + threadIdx.x;
    if (i >= Hl * Wl) return;
    const int y = i / Wl, x = i % Wl;
    uint8_t* rec = pyr + (int64_t)blockIdx.y * S;
    const uint8_t* py = rec + op + (int64_t)(2 * y) * Wp + 2 * x;
    const uint8_t* pv = py + (int64_t)Hp * Wp;
    const unsigned s = (unsigned)py[0] + py[1] + py[Wp] + py[Wp + 1] + 2u;
    rec[ol + i] = (uint8_t)(s >> 2);
    rec[ol + (int64_t)Hl * Wl + i] = (pv[0] & pv[1] & pv[Wp] & pv[Wp + 1]) ? 1 : 0;
}

// grid (ceil(Wl / TW), ceil(Hl / TH)).  o = the level's place in a frame's record.
__global__ __launch_bounds__(PB) void sad_kernel(const uint8_t* __restrict__ pyr, const int* __restrict__ track, int T, int64_t S, int64_t o, int Hl, int Wl,
                                                 int t, int level, int r, u64* __restrict__ acc) {
    __shared__ uint8_t ky[LH * LW], kv[LH * LW];
    __shared__ unsigned tot[MAXC];
    const int* rec = track + (int64_t)t * REC;
    const int cx = rec[0], cy = rec[1], key = rec[2];
    if (rec[3] != VVA_IN_PROGRESS || rec[7] != level || key < 0 || key >= T || cx < -CLIM || cx > CLIM || cy < -CLIM || cy > CLIM) return;
    const int tid = threadIdx.x, side = 2 * r + 1, ncand = side * side;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int64_t HW = (int64_t)Hl * Wl;
    const uint8_t* kY = pyr + (int64_t)key * S + o;
    const uint8_t* tY = pyr + (int64_t)t * S + o;
    for (int c = tid; c < ncand; c += PB) tot[c] = 0;
    // the key's tile, moved by the centre, with a halo of r: LDS (ly, lx) = key pixel (y0 + cy - r + ly, x0 + cx - r + lx); outside the plane: invalid
    const int w = TW + 2 * r, h = TH + 2 * r;
    for (int i = tid; i < w * h; i += PB) {
        const int ly = i / w, lx = i % w;
        const int gy = y0 + cy - r + ly, gx = x0 + cx - r + lx;
        uint8_t yv = 0, vv = 0;
        if (gy >= 0 && gy < Hl && gx >= 0 && gx < Wl) {
            const int64_t at = (int64_t)gy * Wl + gx;
            yv = kY[at];
            vv = kY[HW + at];
        }
        ky[ly * LW + lx] = yv;
        kv[ly * LW + lx] = vv;
    }
    // this thread's 4 pixels of frame t
    const int ty = tid / (TW / 4), tx4 = (tid % (TW / 4)) * 4;
    int yt[4];
    unsigned vt[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int y = y0 + ty, x = x0 + tx4 + p;
        yt[p] = 0;
        vt[p] = 0;
        if (y < Hl && x < Wl) {
            const int64_t at = (int64_t)y * Wl + x;
            yt[p] = tY[at];
            vt[p] = tY[HW + at];
        }
    }
    __syncthreads();
    for (int j = 0; j < side; ++j) {
        const uint8_t* rowy = ky + (ty + j) * LW + tx4;
        const uint8_t* rowv = kv + (ty + j) * LW + tx4;
        for (int i = 0; i < side; ++i) {
            unsigned pk = 0;                                             // sad in bits 0 .. 19, n from bit 20
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int d = (int)rowy[i + p] - yt[p];
                if (vt[p] & rowv[i + p]) pk += (unsigned)(d < 0 ? -d : d) + (1u << 20);
            }
            pk = wave_sum(pk);                                           // <= 256 pixels: sad < 2^16, n <= 2^8
            if ((tid & 63) == 0 && pk) atomicAdd(&tot[j * side + i], pk);
        }
    }
    __syncthreads();
    for (int c = tid; c < ncand; c += PB) {
        const unsigned v = tot[c];
        if (v) {
            atomicAdd(&acc[2 * c], (u64)(v & 0xfffffu));
            atomicAdd(&acc[2 * c + 1], (u64)(v >> 20));
        }
    }
}

struct Cand {
    u64 sad;
    unsigned n;
    int d2, dy, dx, ok;
};
__device__ __forceinline__ bool better(const Cand& a, const Cand& b) {
    if (!a.ok || !b.ok) return a.ok && !b.ok;
    const u64 l = a.sad * b.n, rr = b.sad * a.n;                         // sad < 2^32, n <= 2^24
    if (l != rr) return l < rr;
    if (a.d2 != b.d2) return a.d2 < b.d2;
    if (a.dy != b.dy) return a.dy < b.dy;
    return a.dx < b.dx;
}
__device__ __forceinline__ Cand shfl_cand(const Cand& a, int o) {
    Cand b;
    const unsigned lo = __shfl_xor((unsigned)(a.sad & 0xffffffffu), o, 64), hi = __shfl_xor((unsigned)(a.sad >> 32), o, 64);
    b.sad = ((u64)hi << 32) | lo;
    b.n = __shfl_xor(a.n, o, 64);
    b.d2 = __shfl_xor(a.d2, o, 64);
    b.dy = __shfl_xor(a.dy, o, 64);
    b.dx = __shfl_xor(a.dx, o, 64);
    b.ok = __shfl_xor(a.ok, o, 64);
    return b;
}

// one wave
__global__ __launch_bounds__(64) void pick_kernel(const u64* __restrict__ acc, int* track, int T, int H, int W, int L, int Hl, int Wl, int t, int level, int r,
                                                  int min_overlap, int max_residual) {
    int* rec = track + (int64_t)t * REC;
    const int cx = rec[0], cy = rec[1], key = rec[2];
    if (rec[3] != VVA_IN_PROGRESS || rec[7] != level || key < 0 || key >= T || cx < -CLIM || cx > CLIM || cy < -CLIM || cy > CLIM) return;
    const int side = 2 * r + 1, ncand = side * side;
    const u64 need = (u64)min_overlap * (u64)Hl * (u64)Wl;
    Cand best = {0, 0, 0, 0, 0, 0};
    for (int c = threadIdx.x; c < ncand; c += 64) {
        Cand a;
        a.sad = acc[2 * c];
        a.n = (unsigned)acc[2 * c + 1];
        const int ox = c % side - r, oy = c / side - r;
        a.d2 = ox * ox + oy * oy;
        a.dx = cx + ox;
        a.dy = cy + oy;
        a.ok = 100ull * a.n >= need && a.n > 0;
        if (better(a, best)) best = a;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const Cand b = shfl_cand(best, o);
        if (better(b, best)) best = b;
    }
    if (threadIdx.x != 0) return;
    if (best.ok && level > 0) {                                          // the centre of the next finer level
        rec[0] = 2 * best.dx;
        rec[1] = 2 * best.dy;
        rec[7] = level - 1;
        return;
    }
    // frame t is finished: lost at this level, or judged at level 0
    const int tracked = best.ok && best.sad <= (u64)max_residual * best.n;
    int q = t - 1;
    while (q > 0 && track[(int64_t)q * REC + 3] != 1) --q;
    if (q < 0) q = 0;
    const int kx = track[(int64_t)key * REC], kyy = track[(int64_t)key * REC + 1];
    const int ox = tracked ? kx + best.dx : track[(int64_t)q * REC], oy = tracked ? kyy + best.dy : track[(int64_t)q * REC + 1];
    rec[0] = ox;
    rec[1] = oy;
    rec[3] = tracked;
    rec[4] = best.ok ? (int)(unsigned)(best.sad & 0xffffffffu) : 0;
    rec[5] = best.ok ? (int)(unsigned)(best.sad >> 32) : 0;
    rec[6] = best.ok ? (int)best.n : 0;
    if (t + 1 < T) {
        const int64_t ax = (int64_t)ox - kx, ay = (int64_t)oy - kyy;
        const bool far = 4 * (ax < 0 ? -ax : ax) > W || 4 * (ay < 0 ? -ay : ay) > H;
        const int nkey = tracked && far ? t : key, nq = tracked ? t : q;
        const int px = track[(int64_t)nq * REC] - track[(int64_t)nkey * REC], py = track[(int64_t)nq * REC + 1] - track[(int64_t)nkey * REC + 1];
        int* nx = rec + REC;
        nx[0] = px / (1 << L);                                           // C division: toward zero
        nx[1] = py / (1 << L);
        nx[2] = nkey;
        nx[3] = VVA_IN_PROGRESS;
        nx[4] = nx[5] = nx[6] = 0;
        nx[7] = L;
    }
}

__global__ void start_kernel(int* track, int T, int L) {
    if (threadIdx.x >= REC) return;
    const int k = threadIdx.x;
    track[k] = k == 3 ? 1 : 0;
    if (T > 1) track[REC + k] = k == 3 ? VVA_IN_PROGRESS : (k == 7 ? L : 0);
}

// grid (ceil(ch * cw / PB), T)
__global__ __launch_bounds__(PB) void place_kernel(const uint8_t* __restrict__ dil, const int* __restrict__ track, int H, int W, int cy0, int cx0, int ch, int cw,
                                                   uint8_t* __restrict__ dil_c, uint8_t* __restrict__ inv_c) {
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x, M = (int64_t)ch * cw;
    if (i >= M) return;
    const int64_t t = blockIdx.y;
    const int* rec = track + t * REC;
    const int64_t fy = (int64_t)cy0 + i / cw - rec[1], fx = (int64_t)cx0 + i % cw - rec[0];
    uint8_t d = 0, v = 255;
    if (rec[3] == 1 && fy >= 0 && fy < H && fx >= 0 && fx < W) {
        d = dil[(t * H + fy) * W + fx];
        v = 0;
    }
    dil_c[t * M + i] = d;
    inv_c[t * M + i] = v;
}

// grid (ceil(H * W / PB), T)
__global__ __launch_bounds__(PB) void unplace_kernel(const uint8_t* __restrict__ out_c, const uint8_t* __restrict__ dil, const int* __restrict__ track, int H,
                                                     int W, int cy0, int cx0, int ch, int cw, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x, N = (int64_t)H * W;
    if (i >= N) return;
    const int64_t t = blockIdx.y;
    const int* rec = track + t * REC;
    const int64_t jy = i / W + rec[1] - cy0, jx = i % W + rec[0] - cx0;
    uint8_t d = dil[t * N + i];
    if (rec[3] == 1 && jy >= 0 && jy < ch && jx >= 0 && jx < cw) d = out_c[(t * ch + jy) * cw + jx];
    out[t * N + i] = d;
}

// H, W, L of every entry point -> the level geometry; 0 = fine
int geometry(const char* who, int H, int W, int L, Geo* g) {
    if (H < 1 || W < 1 || L < 0) VV_FAIL(VV_E_ARG, "%s: bad args (H >= 1, W >= 1, L >= 0)", who);
    if ((int64_t)H * W > VVA_MAX_PIXELS || L > VVA_MAX_LEVELS || ((H < W ? H : W) >> L) < 1)
        VV_FAIL(VV_E_UNSUPPORTED, "%s: H * W <= %d, L <= %d and min(H, W) >> L >= 1 are supported, not %d x %d, L %d", who, VVA_MAX_PIXELS, VVA_MAX_LEVELS, H,
                W, L);
    int64_t o = 0;
    for (int l = 0; l <= L; ++l) {
        g->Hl[l] = H >> l;
        g->Wl[l] = W >> l;
        g->o[l] = o;
        o += 2 * (int64_t)g->Hl[l] * g->Wl[l];
    }
    g->S = o;
    return VV_OK;
}
// the arguments vva_sad, vva_pick and vva_track share
int bad_step(const char* who, int T, int t, int level, int L, int r) {
    if (T < 1 || t < 0 || t >= T || level < 0 || level > L || r < 0) VV_FAIL(VV_E_ARG, "%s: bad args (T >= 1, 0 <= t < T, 0 <= level <= L, r >= 0)", who);
    if (T > VVA_MAX_T || r > VVA_MAX_RADIUS) VV_FAIL(VV_E_UNSUPPORTED, "%s: T <= %d and r <= %d are supported, not T %d, r %d", who, VVA_MAX_T, VVA_MAX_RADIUS, T, r);
    return VV_OK;
}
int bad_rule(const char* who, int min_overlap, int max_residual) {
    if (min_overlap < 1 || min_overlap > 100 || max_residual < 0 || max_residual > 255)
        VV_FAIL(VV_E_ARG, "%s: bad args (1 <= min_overlap <= 100, 0 <= max_residual <= 255)", who);
    return VV_OK;
}
int bad_canvas(const char* who, int T, int H, int W, int ch, int cw) {
    if (T < 1 || H < 1 || W < 1 || ch < 1 || cw < 1) VV_FAIL(VV_E_ARG, "%s: bad args (T, H, W, ch, cw >= 1)", who);
    if (T > VVA_MAX_T || (int64_t)H * W > VVA_MAX_PIXELS || (int64_t)ch * cw >= ((int64_t)1 << 31))
        VV_FAIL(VV_E_UNSUPPORTED, "%s: T <= %d, H * W <= %d and ch * cw < 2^31 are supported, not T %d, %d x %d, canvas %d x %d", who, VVA_MAX_T, VVA_MAX_PIXELS,
                T, H, W, ch, cw);
    return VV_OK;
}
bool aligned4(const void* p) { return (uintptr_t)p % 4 == 0; }

int launch_sad(const uint8_t* pyr, const int* track, int T, const Geo& g, int t, int level, int r, u64* acc, hipStream_t st) {
    const int side = 2 * r + 1;
    if (hipMemsetAsync(acc, 0, (size_t)side * side * 2 * sizeof(u64), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vva_sad: memset failed");
    const dim3 grid((unsigned)((g.Wl[level] + TW - 1) / TW), (unsigned)((g.Hl[level] + TH - 1) / TH));
    hipLaunchKernelGGL(sad_kernel, grid, dim3(PB), 0, st, pyr, track, T, g.S, g.o[level], g.Hl[level], g.Wl[level], t, level, r, acc);
    VV_CHECK_LAUNCH("vva_sad");
    return VV_OK;
}
int launch_pick(const u64* acc, int* track, int T, int H, int W, int L, const Geo& g, int t, int level, int r, int min_overlap, int max_residual,
                hipStream_t st) {
    hipLaunchKernelGGL(pick_kernel, dim3(1), dim3(64), 0, st, acc, track, T, H, W, L, g.Hl[level], g.Wl[level], t, level, r, min_overlap, max_residual);
    VV_CHECK_LAUNCH("vva_pick");
    return VV_OK;
}

}  // namespace

extern "C" int vva_abi_version(void) { return VVA_ABI_VERSION; }
extern "C" const char* vva_last_error(void) { return vv_last_error(); }

extern "C" int64_t vva_frame_bytes(int H, int W, int L) {
    Geo g;
    const int rc = geometry("vva_frame_bytes", H, W, L, &g);
    return rc != VV_OK ? rc : g.S;
}

extern "C" int vva_pyramid(const uint8_t* frames, const uint8_t* dil, int B, int H, int W, int L, uint8_t* pyr, void* stream) {
    if (!frames || !dil || !pyr || B < 1) VV_FAIL(VV_E_ARG, "vva_pyramid: bad args (no null pointer, B >= 1)");
    Geo g;
    const int rc = geometry("vva_pyramid", H, W, L, &g);
    if (rc != VV_OK) return rc;
    if (B > VVA_MAX_T) VV_FAIL(VV_E_UNSUPPORTED, "vva_pyramid: B <= %d is supported, not %d", VVA_MAX_T, B);
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)H * W;
    const bool vec = W % 4 == 0 && g.S % 4 == 0 && aligned4(frames) && aligned4(dil) && aligned4(pyr);
    const int64_t units = vec ? N / 4 : N;
    const dim3 grid((unsigned)((units + PB - 1) / PB), (unsigned)B);
    if (vec) hipLaunchKernelGGL(luma_kernel<true>, grid, dim3(PB), 0, st, frames, dil, N, units, g.S, pyr);
    else hipLaunchKernelGGL(luma_kernel<false>, grid, dim3(PB), 0, st, frames, dil, N, units, g.S, pyr);
    VV_CHECK_LAUNCH("vva_pyramid");
    for (int l = 1; l <= L; ++l) {
        const dim3 gl((unsigned)(((int64_t)g.Hl[l] * g.Wl[l] + PB - 1) / PB), (unsigned)B);
        hipLaunchKernelGGL(down_kernel, gl, dim3(PB), 0, st, pyr, g.S, g.o[l - 1], g.Hl[l - 1], g.Wl[l - 1], g.o[l], g.Hl[l], g.Wl[l]);
        VV_CHECK_LAUNCH("vva_pyramid");
    }
    return VV_OK;
}

extern "C" int vva_sad(const uint8_t* pyr, const int32_t* track, int T, int H, int W, int L, int t, int level, int r, uint64_t* acc, void* stream) {
    if (!pyr || !track || !acc) VV_FAIL(VV_E_ARG, "vva_sad: bad args (no null pointer)");
    Geo g;
    int rc = geometry("vva_sad", H, W, L, &g);
    if (rc != VV_OK) return rc;
    rc = bad_step("vva_sad", T, t, level, L, r);
    if (rc != VV_OK) return rc;
    return launch_sad(pyr, track, T, g, t, level, r, (u64*)acc, (hipStream_t)stream);
}

extern "C" int vva_pick(const uint64_t* acc, int32_t* track, int T, int H, int W, int L, int t, int level, int r, int min_overlap, int max_residual,
                        void* stream) {
    if (!acc || !track) VV_FAIL(VV_E_ARG, "vva_pick: bad args (no null pointer)");
    Geo g;
    int rc = geometry("vva_pick", H, W, L, &g);
    if (rc != VV_OK) return rc;
    rc = bad_step("vva_pick", T, t, level, L, r);
    if (rc != VV_OK) return rc;
    rc = bad_rule("vva_pick", min_overlap, max_residual);
    if (rc != VV_OK) return rc;
    return launch_pick((const u64*)acc, track, T, H, W, L, g, t, level, r, min_overlap, max_residual, (hipStream_t)stream);
}

extern "C" int64_t vva_track_launches(int T, int L) {
    if (T < 1 || L < 0) return VV_E_ARG;
    return 1 + (int64_t)(T - 1) * (L + 1) * 3;
}

extern "C" int vva_track(const uint8_t* pyr, int32_t* track, uint64_t* acc, int T, int H, int W, int L, int radius, int min_overlap, int max_residual,
                         void* stream) {
    if (!pyr || !track || !acc || radius < 1) VV_FAIL(VV_E_ARG, "vva_track: bad args (no null pointer, radius >= 1)");
    Geo g;
    int rc = geometry("vva_track", H, W, L, &g);
    if (rc != VV_OK) return rc;
    rc = bad_step("vva_track", T, 0, 0, L, radius);
    if (rc != VV_OK) return rc;
    rc = bad_rule("vva_track", min_overlap, max_residual);
    if (rc != VV_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(start_kernel, dim3(1), dim3(64), 0, st, track, T, L);
    VV_CHECK_LAUNCH("vva_track");
    for (int t = 1; t < T; ++t)
        for (int level = L; level >= 0; --level) {
            const int r = level == L ? radius : 1;
            rc = launch_sad(pyr, track, T, g, t, level, r, (u64*)acc, st);
            if (rc != VV_OK) return rc;
            rc = launch_pick((const u64*)acc, track, T, H, W, L, g, t, level, r, min_overlap, max_residual, st);
            if (rc != VV_OK) return rc;
        }
    return VV_OK;
}

extern "C" int vva_place_masks(const uint8_t* dil, const int32_t* track, int T, int H, int W, int cy0, int cx0, int ch, int cw, uint8_t* dil_c,
                               uint8_t* invalid_c, void* stream) {
    if (!dil || !track || !dil_c || !invalid_c) VV_FAIL(VV_E_ARG, "vva_place_masks: bad args (no null pointer)");
    const int rc = bad_canvas("vva_place_masks", T, H, W, ch, cw);
    if (rc != VV_OK) return rc;
    const dim3 grid((unsigned)(((int64_t)ch * cw + PB - 1) / PB), (unsigned)T);
    hipLaunchKernelGGL(place_kernel, grid, dim3(PB), 0, (hipStream_t)stream, dil, track, H, W, cy0, cx0, ch, cw, dil_c, invalid_c);
    VV_CHECK_LAUNCH("vva_place_masks");
    return VV_OK;
}

extern "C" int vva_unplace_mask(const uint8_t* dil_out_c, const uint8_t* dil, const int32_t* track, int T, int H, int W, int cy0, int cx0, int ch, int cw,
                                uint8_t* dil_out, void* stream) {
    if (!dil_out_c || !dil || !track || !dil_out || dil_out == dil) VV_FAIL(VV_E_ARG, "vva_unplace_mask: bad args (no null pointer, dil_out is not dil)");
    const int rc = bad_canvas("vva_unplace_mask", T, H, W, ch, cw);
    if (rc != VV_OK) return rc;
    const dim3 grid((unsigned)(((int64_t)H * W + PB - 1) / PB), (unsigned)T);
    hipLaunchKernelGGL(unplace_kernel, grid, dim3(PB), 0, (hipStream_t)stream, dil_out_c, dil, track, H, W, cy0, cx0, ch, cw, dil_out);
    VV_CHECK_LAUNCH("vva_unplace_mask");
    return VV_OK;
}
