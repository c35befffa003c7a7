// Inpaint deflicker (videovanish_amd/deflicker.py, infill.finish): Lee's sigma filter along time on the model's pixels.
// The rules are include/vvflicker.h's; all arithmetic is integer.
//   vvf_window_pixels   the window's pixels as vv_roi_paste_composite reads them (vv_paste_px.h), materialised: patch [T][Hm][Wm][3] -> win [T][h][w][3]
//   vvf_hold            per pixel the rounded mean of the temporal neighbours within tol, out [T][h][w][3], and 12 integer sums per frame
//   vvc_hold            the same along a tracked camera translation (include/vvflickalign.h): the gather form's body
// vvf_hold has two forms, chosen by the launcher from its arguments alone.
//   fixed    the window stands at one place in every frame and w % 4 == 0.  A streaming kernel over [T][h][w][3] u8, as vv_plate.hip's family:
//            a thread owns 4 adjacent pixels of one row (12 bytes: one dwordx3 load per frame, lane after lane contiguous) and walks the frames
//            of its slab (grid z: VVF_SLAB frames) with the last 2 R + 1 frames packed in registers, so every input byte is read once per slab
//            (plus R frames of halo on each side).  The ring is a template on R, rotated by unrolled moves: every index is a constant, nothing
//            goes to scratch.  The frame after the newest one is in flight while a frame is computed.  A slab writes and counts its own frames only.
//   gather   everything else (a window that follows the mask, an odd width): one thread per output pixel, its up to 2 R + 1 neighbours read at
//            (x - ox_s, y - oy_s) with byte loads; neighbouring threads re-read the same lines, which come from L2.
// The sums go registers (packed in 16-bit halves) -> wave reduction -> LDS -> one group of 64-bit global atomics per block, as in vv_tone.hip:
// integer adds in any order.  out_c = (2 S_c + n) / (2 n) is a multiplication by a 20-bit reciprocal, exact for every S_c <= 255 n, n <= 9.
#include "vv_paste_px.h"
#include "vv_wave_bytes.h"
#include "../../include/vvflicker.h"
#include "../../include/vvflickalign.h"

namespace {

using vvwave::U3;
using vvwave::wave_sum;
constexpr int FB = 256;                     // threads per block
constexpr int NSUM = 12;
typedef unsigned long long u64;
static_assert(VVF_MAX_RADIUS == 4 && 2 * VVF_MAX_RADIUS + 1 <= 9, "n <= 9: the reciprocals, the packed sums");
static_assert(VVC_MAX_RADIUS == VVF_MAX_RADIUS && VVC_MAX_T == VVF_MAX_T, "vvc_hold shares vvf_hold's limits");
static_assert(64 * 4 * 255 < (1 << 16) && 64 * 4 * 9 < (1 << 16), "a wave's sums of 4 pixels per lane fit the 16-bit halves");

// x / (2 n) == (x * recip(n)) >> 20 for every x <= 2 * 255 * n + n
constexpr unsigned recip(unsigned n) { return (1u << 20) / (2u * n) + 1u; }
constexpr bool recip_exact() {
    for (unsigned n = 1; n <= 9; ++n)
        for (unsigned x = 0; x <= 511u * n; ++x)
            if (((x * recip(n)) >> 20) != x / (2u * n)) return false;
    return true;
}
static_assert(recip_exact(), "the rounded mean by multiplication");

__device__ __forceinline__ unsigned byte_of(const U3& q, int j) {       // byte j of the 12, j a constant
    const unsigned w = (j >> 2) == 0 ? q.a : (j >> 2) == 1 ? q.b : q.c;
    return (w >> ((j & 3) * 8)) & 255u;
}
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
            if (k == 2 && !__any((int)v[2]) ) continue;                    // wave-uniform
            const unsigned s = wave_sum(v[k]);
            if (lane0) {
                if (s & 0xffffu) atomicAdd(&tot[half * 6 + (k == 0 ? 0 : k == 1 ? 2 : 4)], s & 0xffffu);
                if (s >> 16) atomicAdd(&tot[half * 6 + (k == 0 ? 1 : k == 1 ? 3 : 5)], s >> 16);
            }
        }
    }
}

__global__ __launch_bounds__(FB) void window_pixels_kernel(const uint8_t* __restrict__ patch, int Hm, int Wm, int h, int w, uint8_t* __restrict__ win) {
    const int64_t N = (int64_t)h * w, i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i >= N) return;
    const int t = (int)blockIdx.y;
    uint8_t p[3];
    vvpaste::window_px(patch + (int64_t)t * Hm * Wm * 3, Hm, Wm, (int)(i % w), (int)(i / w), h, w, p);
    uint8_t* d = win + ((int64_t)t * N + i) * 3;
    d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
}

// grid (ceil(h w / 4 / FB), 1, ceil(T / VVF_SLAB)).  Reads of win lie inside frames 0 .. T - 1 at the thread's own 12 bytes (i0 + 3 < h w: w % 4 == 0),
// reads of the mask are bounds-checked against the frame, the writes are the thread's own 12 bytes of out in its slab's frames and the atomics.
template <int R>
__global__ __launch_bounds__(FB) void hold_fixed_kernel(const uint8_t* __restrict__ win, const int* __restrict__ offsets, const uint8_t* __restrict__ mask,
                                                        int mask_vec, int T, int H0, int W0, int h, int w, int tol, uint8_t* __restrict__ out,
                                                        u64* __restrict__ sums) {
    constexpr int K = 2 * R + 1;
    __shared__ unsigned mg[10];
    __shared__ unsigned tot[VVF_SLAB * NSUM];
    if (threadIdx.x < VVF_SLAB * NSUM) tot[threadIdx.x] = 0;
    if (threadIdx.x < 10) mg[threadIdx.x] = threadIdx.x ? recip(threadIdx.x) : 0u;
    __syncthreads();
    const int64_t N = (int64_t)h * w;
    const int64_t i0 = ((int64_t)blockIdx.x * FB + threadIdx.x) * 4;
    const bool active = i0 < N;
    const int tb = (int)blockIdx.z * VVF_SLAB, te = min(T, tb + VVF_SLAB);
    const int my = active ? offsets[0] + (int)(i0 / w) : -1, mx = active ? offsets[1] + (int)(i0 % w) : 0;      // the first pixel in the frame
    const bool row_in = my >= 0 && my < H0;
    const bool quad = row_in && mask_vec && mx >= 0 && mx + 3 < W0 && (mx & 3) == 0;                          // one aligned dword holds the 4 mask bytes
    const int64_t NM = (int64_t)H0 * W0, F = N * 3;                         // the strides of a frame: uniform, the pointers below walk by them
    const uint8_t* src = win + i0 * 3;                                      // the thread's 12 bytes of frame 0
    auto frame = [&](int t) -> U3 {
        U3 q = {0u, 0u, 0u};
        if (active && t >= 0 && t < T) q = *reinterpret_cast<const U3*>(src + t * F);
        return q;
    };
    U3 ring[K];                                  // at frame t: ring[j] = frame t - R + j
#pragma unroll
    for (int j = 1; j < K; ++j) ring[j] = frame(tb - R + j - 1);
    U3 next = frame(tb + R);
    const uint8_t* pm = mask + tb * NM + ((int64_t)my * W0 + mx);          // read where row_in only
    uint8_t* po = out + tb * F + i0 * 3;
    for (int t = tb; t < te; ++t, pm += NM, po += F) {
#pragma unroll
        for (int j = 0; j + 1 < K; ++j) ring[j] = ring[j + 1];
        ring[K - 1] = next;
        next = frame(t + 1 < te ? t + R + 1 : T);
        unsigned mk = 0;                                                       // byte p: pixel p's mask
        if (quad) {
            mk = *reinterpret_cast<const unsigned*>(pm);
        } else if (row_in) {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (mx + p >= 0 && mx + p < W0) mk |= (unsigned)pm[p] << (8 * p);
        }
        unsigned lo[3] = {active ? 4u : 0u, 0u, 0u}, hi[3] = {0u, 0u, 0u};
        unsigned q[3] = {0u, 0u, 0u};                                          // the 12 output bytes
#pragma unroll
        for (int p = 0; p < 4; ++p) {                                          // pixel after pixel: 7 live values, not 28
            const unsigned x[3] = {byte_of(ring[R], 3 * p), byte_of(ring[R], 3 * p + 1), byte_of(ring[R], 3 * p + 2)};
            unsigned S[3] = {x[0], x[1], x[2]}, n = 1;
#pragma unroll
            for (int j = 0; j < K; ++j) {                                      // straight-line code: no branch per sample
                if (j == R) continue;
                const int s = t - R + j;
                const int gate = (s >= 0 && s < T) ? tol : -1;                 // block-uniform; a frame outside the clip (zeros in the ring) passes no gate
                const unsigned v[3] = {byte_of(ring[j], 3 * p), byte_of(ring[j], 3 * p + 1), byte_of(ring[j], 3 * p + 2)};
                const unsigned far = max(max(absdiff(v[0], x[0]), absdiff(v[1], x[1])), absdiff(v[2], x[2]));
                const unsigned ok = (int)far <= gate ? 1u : 0u;
                n += ok;
#pragma unroll
                for (int c = 0; c < 3; ++c) S[c] += v[c] * ok;
            }
            const unsigned m = mg[n];
            unsigned d[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned o = ((2u * S[c] + n) * m) >> 20;
                d[c] = absdiff(o, x[c]);
                q[(3 * p + c) >> 2] |= o << (((3 * p + c) & 3) * 8);
            }
            const unsigned a[3] = {(d[0] | d[1] | d[2]) ? 1u << 16 : 0u, n | (d[0] << 16), d[1] | (d[2] << 16)};
            const bool masked = ((mk >> (8 * p)) & 255u) != 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (active) lo[k] += a[k];
                if (masked) hi[k] += a[k] + (k == 0 ? 1u : 0u);
            }
        }
        if (active) {
            const U3 o3 = {q[0], q[1], q[2]};
            *reinterpret_cast<U3*>(po) = o3;
        }
        add_sums(tot + (t - tb) * NSUM, lo, hi);
    }
    __syncthreads();
    if (threadIdx.x < VVF_SLAB * NSUM && tb + (int)threadIdx.x / NSUM < te && tot[threadIdx.x])
        atomicAdd(&sums[(int64_t)tb * NSUM + threadIdx.x], (u64)tot[threadIdx.x]);
}

// grid (ceil(h w / FB), T): frame = blockIdx.y.  Reads of win are bounds-checked against the window of the frame they come from, reads of the mask
// against the frame, whatever the offsets (and the track) hold; the writes are the thread's own 3 bytes of out and the atomics into sums[t].
// TRACKED (vvc_hold, include/vvflickalign.h): the neighbour s is read at the pixel's place moved by e_t - e_s, e = offsets + the tracked offset.
// That displacement (taken in 64 bits) and whether s gives a sample at all (not t, both frames tracked, the windows overlap) are the same for
// every pixel of the block: they come from scalar loads at addresses made of blockIdx and the loop counter and stay in scalar registers.
template <bool TRACKED>
__global__ __launch_bounds__(FB) void hold_gather_kernel(const uint8_t* __restrict__ win, const int* __restrict__ offsets, const int32_t* __restrict__ track,
                                                         const uint8_t* __restrict__ mask, int T, int H0, int W0, int h, int w, int R, int tol,
                                                         uint8_t* __restrict__ out, u64* __restrict__ sums) {
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
        const int s0 = max(t - R, 0), s1 = min(t + R, T - 1);
        // TRACKED: e_t, and below e_s and whether s gives samples at all, depend on blockIdx and the loop counter only: scalar loads, scalar registers
        const bool t_tracked = TRACKED && track[t * VVC_TRACK_INTS + 3] == 1;
        const int64_t ety = TRACKED ? (int64_t)offsets[t * 2 + 0] + track[t * VVC_TRACK_INTS + 1] : 0, etx = TRACKED ? (int64_t)offsets[t * 2 + 1] + track[t * VVC_TRACK_INTS + 0] : 0;
        for (int s = s0; s <= s1; ++s) {
            int ys, xs;
            if constexpr (TRACKED) {
                if (s == t || !t_tracked || track[s * VVC_TRACK_INTS + 3] != 1) continue;
                const int64_t dy = ety - ((int64_t)offsets[s * 2 + 0] + track[s * VVC_TRACK_INTS + 1]), dx = etx - ((int64_t)offsets[s * 2 + 1] + track[s * VVC_TRACK_INTS + 0]);
                if (dy <= -(int64_t)h || dy >= h || dx <= -(int64_t)w || dx >= w) continue;         // the windows share no pixel
                // |dy| < h, |dx| < w: the sums lie in (-2^31, 2^32), so one unsigned compare per axis tells inside from outside
                ys = (int)((unsigned)yy + (unsigned)(int)dy); xs = (int)((unsigned)xx + (unsigned)(int)dx);
                if ((unsigned)ys >= (unsigned)h || (unsigned)xs >= (unsigned)w) continue;
            } else {
                ys = py - offsets[s * 2 + 0]; xs = px - offsets[s * 2 + 1];
                if (s == t || ys < 0 || ys >= h || xs < 0 || xs >= w) continue;
            }
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

bool aligned(const void* p, unsigned a) { return (uintptr_t)p % a == 0; }

}  // namespace

extern "C" int vvf_abi_version(void) { return VVF_ABI_VERSION; }
extern "C" const char* vvf_last_error(void) { return vv_last_error(); }

extern "C" int vvf_window_pixels(const uint8_t* patch, int T, int Hm, int Wm, int h, int w, uint8_t* win, void* stream) {
    if (!patch || !win || T <= 0 || Hm <= 0 || Wm <= 0 || h <= 0 || w <= 0) VV_FAIL(VV_E_ARG, "vvf_window_pixels: bad args (no null pointer, sizes > 0)");
    if (T > VVF_MAX_T || (int64_t)h * w >= ((int64_t)1 << 31) || (int64_t)Hm * Wm >= ((int64_t)1 << 31))
        VV_FAIL(VV_E_UNSUPPORTED, "vvf_window_pixels: T <= %d and fewer than 2^31 pixels per frame are supported, not T %d, %d x %d from %d x %d", VVF_MAX_T, T,
                h, w, Hm, Wm);
    const int64_t N = (int64_t)h * w;
    hipLaunchKernelGGL(window_pixels_kernel, dim3((unsigned)((N + FB - 1) / FB), (unsigned)T), dim3(FB), 0, (hipStream_t)stream, patch, Hm, Wm, h, w, win);
    VV_CHECK_LAUNCH("vvf_window_pixels");
    return VV_OK;
}

extern "C" int vvf_hold(const uint8_t* win, const int* offsets, const uint8_t* mask2d, int T, int H0, int W0, int h, int w, int radius, int tol, int fixed,
                        uint8_t* out, int64_t* sums, void* stream) {
    if (!win || !offsets || !mask2d || !out || !sums || T <= 0 || H0 <= 0 || W0 <= 0 || h <= 0 || w <= 0 || h > H0 || w > W0 || radius < 0 || tol < 0 ||
        out == win)
        VV_FAIL(VV_E_ARG, "vvf_hold: bad args (no null pointer, sizes > 0, h <= H0, w <= W0, radius >= 0, tol >= 0, out is not win)");
    if (radius > VVF_MAX_RADIUS || tol > 255 || T > VVF_MAX_T || (int64_t)h * w >= ((int64_t)1 << 31))
        VV_FAIL(VV_E_UNSUPPORTED, "vvf_hold: radius <= %d, tol <= 255, T <= %d and h * w < 2^31 are supported, not radius %d, tol %d, T %d, %d x %d",
                VVF_MAX_RADIUS, VVF_MAX_T, radius, tol, T, h, w);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, (size_t)T * NSUM * sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vvf_hold: memset failed");
    const int64_t N = (int64_t)h * w;
    if (fixed && w % 4 == 0 && aligned(win, 4) && aligned(out, 4)) {
        const dim3 grid((unsigned)((N / 4 + FB - 1) / FB), 1, (unsigned)((T + VVF_SLAB - 1) / VVF_SLAB));
        const int mask_vec = W0 % 4 == 0 && aligned(mask2d, 4);
#define VVF_FIXED(R) hipLaunchKernelGGL(hold_fixed_kernel<R>, grid, dim3(FB), 0, st, win, offsets, mask2d, mask_vec, T, H0, W0, h, w, tol, out, (u64*)sums)
        switch (radius) {
            case 0: VVF_FIXED(0); break;
            case 1: VVF_FIXED(1); break;
            case 2: VVF_FIXED(2); break;
            case 3: VVF_FIXED(3); break;
            default: VVF_FIXED(4); break;
        }
#undef VVF_FIXED
    } else {
        hipLaunchKernelGGL(hold_gather_kernel<false>, dim3((unsigned)((N + FB - 1) / FB), (unsigned)T), dim3(FB), 0, st, win, offsets, (const int32_t*)nullptr,
                           mask2d, T, H0, W0, h, w, radius, tol, out, (u64*)sums);
    }
    VV_CHECK_LAUNCH("vvf_hold");
    return VV_OK;
}

extern "C" int vvc_abi_version(void) { return VVC_ABI_VERSION; }
extern "C" const char* vvc_last_error(void) { return vv_last_error(); }

extern "C" int vvc_hold(const uint8_t* win, const int* offsets, const int32_t* track, const uint8_t* mask2d, int T, int H0, int W0, int h, int w, int radius,
                        int tol, uint8_t* out, int64_t* sums, void* stream) {
    if (!win || !offsets || !track || !mask2d || !out || !sums || T <= 0 || H0 <= 0 || W0 <= 0 || h <= 0 || w <= 0 || h > H0 || w > W0 || radius < 0 ||
        tol < 0 || out == win)
        VV_FAIL(VV_E_ARG, "vvc_hold: bad args (no null pointer, sizes > 0, h <= H0, w <= W0, radius >= 0, tol >= 0, out is not win)");
    if (radius > VVC_MAX_RADIUS || tol > 255 || T > VVC_MAX_T || (int64_t)h * w >= ((int64_t)1 << 31))
        VV_FAIL(VV_E_UNSUPPORTED, "vvc_hold: radius <= %d, tol <= 255, T <= %d and h * w < 2^31 are supported, not radius %d, tol %d, T %d, %d x %d",
                VVC_MAX_RADIUS, VVC_MAX_T, radius, tol, T, h, w);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, (size_t)T * NSUM * sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vvc_hold: memset failed");
    const int64_t N = (int64_t)h * w;
    hipLaunchKernelGGL(hold_gather_kernel<true>, dim3((unsigned)((N + FB - 1) / FB), (unsigned)T), dim3(FB), 0, st, win, offsets, track, mask2d, T, H0, W0, h, w,
                       radius, tol, out, (u64*)sums);
    VV_CHECK_LAUNCH("vvc_hold");
    return VV_OK;
}
