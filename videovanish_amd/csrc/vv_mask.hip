// Mask clean-up (videovanish_amd/maskclean.py): the stage between the dilation and the planners.
//   vvm_label_components   8-connected components of every frame, labelled with the smallest linear index of the component
//   vvm_despeckle          label, weigh every component by the raw mask pixels inside it, clear the light ones
//   vvm_time_bridge_grow   per pixel along time: fill short zero runs between two set frames, then OR over +-grow frames
// Labelling is union-find in global memory, frame by frame: L[i] = the start of i's horizontal run inside its 64-pixel wave segment (one ballot:
// no atomics for most horizontal links), one merge pass that unites every pixel with the run to its left (first lane of a segment only) and with
// the row above (N, else NW and NE: with N set, NW and NE hang on N already), then a flatten pass.  A parent is always a smaller index than its
// child, so every walk ends, the root of a tree is its smallest index, and the labels do not depend on the order of the threads.  Inside the merge
// and flatten passes L is touched by agent-scope atomics only (other workgroups, on other XCDs, move it meanwhile).
// The time kernel keeps, per pixel, three small shift registers (input, dilated, closed) and reads every frame once: thread = 16 pixels with
// 16-byte loads where H * W is a multiple of 16, else one pixel.
#include "vv_common.h"
#include "vv_wave_bytes.h"
#include "../../include/vvmask.h"

namespace {

using vvwave::wave_sum;
constexpr int MB = 256;                     // threads per block; a multiple of 64, and block b starts at pixel b * MB: lane = pixel index & 63

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int find_root(const int* L, int i) {
    for (int p = ld_agent(L + i); p != i; p = ld_agent(L + i)) i = p;
    return i;
}
// hook the larger root under the smaller; a returned old value other than the root itself shows that root had moved: go on from where it went
__device__ __forceinline__ void unite(int* L, int a, int b) {
    for (;;) {
        a = find_root(L, a);
        b = find_root(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

// grid (ceil(N / MB), S) for the per-pixel kernels below: frame = blockIdx.y, pixel i = blockIdx.x * MB + threadIdx.x < N
__global__ __launch_bounds__(MB) void label_init_kernel(const uint8_t* __restrict__ mask, int N, int W, int* __restrict__ L) {
    const int64_t base = (int64_t)blockIdx.y * N;
    const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
    const bool in = i < N;
    const bool fg = in && mask[base + i] != 0;
    const unsigned long long F = __ballot(fg), R = __ballot(in && i % W == 0);
    if (!in) return;
    const int lane = threadIdx.x & 63;
    // lane j continues the run of lane j - 1: both set, same row.  s = the last lane at or below this one that does not continue: the run's start
    const unsigned long long cont = F & (F << 1) & ~R;
    const unsigned long long below = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    const int s = 63 - __clzll((long long)(~cont & below));
    L[base + i] = fg ? (int)i - (lane - s) : -1;
}

__global__ __launch_bounds__(MB) void label_merge_kernel(const uint8_t* __restrict__ mask, int N, int W, int* L) {
    const int64_t base = (int64_t)blockIdx.y * N;
    const int64_t i64 = (int64_t)blockIdx.x * MB + threadIdx.x;
    if (i64 >= N) return;
    const uint8_t* m = mask + base;
    const int i = (int)i64;
    if (!m[i]) return;
    int* Lf = L + base;
    const int x = i % W;
    if (x > 0 && (i & 63) == 0 && m[i - 1]) unite(Lf, i, i - 1);       // the other lanes were linked to their run by label_init_kernel
    if (i >= W) {
        if (m[i - W]) unite(Lf, i, i - W);
        else {
            if (x > 0 && m[i - W - 1]) unite(Lf, i, i - W - 1);
            if (x + 1 < W && m[i - W + 1]) unite(Lf, i, i - W + 1);
        }
    }
}

__global__ __launch_bounds__(MB) void label_flatten_kernel(int N, int* L) {
    const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
    if (i >= N) return;
    int* Lf = L + (int64_t)blockIdx.y * N;
    if (ld_agent(Lf + i) < 0) return;
    __hip_atomic_store(Lf + i, find_root(Lf, (int)i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // any value a walker meets here is an ancestor
}

// weight[label] += 1 for every labelled pixel whose raw mask is non-zero in any channel; the lanes of a wave that share a label add once
__global__ __launch_bounds__(MB) void weigh_kernel(const uint8_t* __restrict__ raw, int N, int ch, const int* __restrict__ L, int* __restrict__ weight) {
    const int64_t base = (int64_t)blockIdx.y * N;
    const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
    int r = -1;
    if (i < N) {
        const int lab = L[base + i];
        if (lab >= 0) {
            const uint8_t* p = raw + (base + i) * ch;
            unsigned any = 0;
            for (int c = 0; c < ch; ++c) any |= p[c];
            if (any) r = lab;
        }
    }
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(r >= 0);
    while (pending) {                                                   // wave-uniform
        const int lead = __ffsll((long long)pending) - 1;
        const int rl = __shfl(r, lead, 64);
        const unsigned long long same = __ballot(r == rl);
        if (lane == lead) atomicAdd(&weight[base + rl], (int)__popcll(same));
        pending &= ~same;
    }
}

__global__ __launch_bounds__(MB) void clear_kernel(const uint8_t* __restrict__ dil, int N, int min_area, const int* __restrict__ L, const int* __restrict__ weight,
                                                   uint8_t* __restrict__ out, unsigned long long* __restrict__ counts) {
    __shared__ unsigned tot[2];
    if (threadIdx.x < 2) tot[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.y * N;
    const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
    unsigned cleared = 0, removed = 0;
    if (i < N) {
        const uint8_t v = dil[base + i];
        if (v && min_area > 1) {
            const int lab = L[base + i];
            if (weight[base + lab] < min_area) { cleared = 1; removed = lab == (int)i; }      // a component is counted once, at its root pixel
        }
        out[base + i] = cleared ? (uint8_t)0 : v;
    }
    const unsigned pk = wave_sum(cleared | (removed << 16));           // <= 64 each
    if ((threadIdx.x & 63) == 0 && pk) { atomicAdd(&tot[0], pk >> 16); atomicAdd(&tot[1], pk & 0xffffu); }
    __syncthreads();
    if (threadIdx.x < 2 && tot[threadIdx.x]) atomicAdd(&counts[(int64_t)blockIdx.y * 2 + threadIdx.x], (unsigned long long)tot[threadIdx.x]);
}

// Thread = P pixels (VEC: 16, unit u = pixels 16 u .. 16 u + 15, N % 16 == 0 and 16-byte aligned bases, checked by the launcher; else 1), walking
// the frames once.  At step s the thread reads frame s (zero from T on) and holds, newest bit lowest:
//   w  the input                                  bit j = in[s - j]
//   d  its dilation by bridge + 1 frames          D[s] = OR in[s - g .. s]
//   c  the closing                                C[s - g] = AND D[s - g .. s]: the input with the bridged runs filled
// and writes out[s - g - k] = OR C[s - g - 2 k .. s - g].  Everything before frame 0 and from frame T on is zero in all three, so runs that touch
// an end stay open and the grow is clamped.
template <bool VEC>
__global__ __launch_bounds__(MB) void time_kernel(const uint8_t* __restrict__ in, int T, int64_t N, int64_t units, int g, int k, uint8_t* __restrict__ out,
                                                  unsigned long long* __restrict__ counts) {
    constexpr int P = VEC ? 16 : 1;
    const int64_t u = (int64_t)blockIdx.x * MB + threadIdx.x;
    const bool live = u < units;
    unsigned w[P], d[P], c[P];
#pragma unroll
    for (int p = 0; p < P; ++p) w[p] = d[p] = c[p] = 0;
    const unsigned Mg = (2u << g) - 1u, Mk = (2u << (2 * k)) - 1u;
    for (int s = 0; s < T + g + k; ++s) {
        unsigned v[4] = {0, 0, 0, 0};
        if (live && s < T) {
            if constexpr (VEC) {
                const uint4 q = *reinterpret_cast<const uint4*>(in + (int64_t)s * N + u * 16);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                v[0] = in[(int64_t)s * N + u];
            }
        }
        const int fs = s - g, ft = s - g - k;                           // the frame the closing reaches at this step, the frame written
        unsigned nb = 0, ng = 0, o4[4] = {0, 0, 0, 0};
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const unsigned bit = ((v[p >> 2] >> ((p & 3) * 8)) & 255u) != 0;
            w[p] = (w[p] << 1) | bit;
            d[p] = (d[p] << 1) | (unsigned)((w[p] & Mg) != 0);
            const unsigned e = (d[p] & Mg) == Mg;
            nb += e & ~(w[p] >> g) & 1u;                                // closed but not set in the input: bridged, in frame fs
            c[p] = (c[p] << 1) | e;
            const unsigned o = (c[p] & Mk) != 0;
            ng += o & ~(c[p] >> k) & 1u;                                // written but not in the closing: grown, in frame ft
            o4[p >> 2] |= o ? 255u << ((p & 3) * 8) : 0u;
        }
        if (live && ft >= 0) {
            if constexpr (VEC) *reinterpret_cast<uint4*>(out + (int64_t)ft * N + u * 16) = make_uint4(o4[0], o4[1], o4[2], o4[3]);
            else out[(int64_t)ft * N + u] = (uint8_t)o4[0];
        }
        if (fs < 0 || fs >= T) nb = 0;
        if (ft < 0) ng = 0;
        unsigned pk = nb | (ng << 16);                                  // <= 16 each per lane, <= 1024 per wave
        if (__ballot(pk != 0)) {                                        // wave-uniform
            pk = wave_sum(pk);
            if ((threadIdx.x & 63) == 0) {
                if (pk & 0xffffu) atomicAdd(&counts[(int64_t)fs * 2], (unsigned long long)(pk & 0xffffu));
                if (pk >> 16) atomicAdd(&counts[(int64_t)ft * 2 + 1], (unsigned long long)(pk >> 16));
            }
        }
    }
}

int label(const char* who, const uint8_t* mask, int S, int H, int W, int32_t* L, hipStream_t st) {
    const int N = H * W;
    const dim3 grid((unsigned)(((int64_t)N + MB - 1) / MB), (unsigned)S);
    hipLaunchKernelGGL(label_init_kernel, grid, dim3(MB), 0, st, mask, N, W, L);
    hipLaunchKernelGGL(label_merge_kernel, grid, dim3(MB), 0, st, mask, N, W, L);
    hipLaunchKernelGGL(label_flatten_kernel, grid, dim3(MB), 0, st, N, L);
    VV_CHECK_LAUNCH(who);
    return VV_OK;
}

bool bad_frames(int S, int H, int W) { return S < 1 || S > 65535 || H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31); }

}  // namespace

extern "C" int vvm_abi_version(void) { return VVM_ABI_VERSION; }
extern "C" const char* vvm_last_error(void) { return vv_last_error(); }

extern "C" int vvm_label_components(const uint8_t* mask2d, int S, int H, int W, int32_t* labels, void* stream) {
    if (!mask2d || !labels || bad_frames(S, H, W)) VV_FAIL(VV_E_ARG, "vvm_label_components: bad args (S in [1, 65535], H * W < 2^31)");
    return label("vvm_label_components", mask2d, S, H, W, labels, (hipStream_t)stream);
}

extern "C" int vvm_despeckle(const uint8_t* dil, const uint8_t* raw, int S, int H, int W, int ch, int min_area, int32_t* labels_ws, int32_t* weight_ws,
                             uint8_t* out, int64_t* counts, void* stream) {
    if (!dil || !raw || !labels_ws || !weight_ws || !out || !counts || ch < 1 || bad_frames(S, H, W))
        VV_FAIL(VV_E_ARG, "vvm_despeckle: bad args (S in [1, 65535], H * W < 2^31, ch >= 1)");
    hipStream_t st = (hipStream_t)stream;
    const int N = H * W;
    if (hipMemsetAsync(counts, 0, (size_t)S * 2 * sizeof(int64_t), st) != hipSuccess ||
        hipMemsetAsync(weight_ws, 0, (size_t)S * N * sizeof(int32_t), st) != hipSuccess)
        VV_FAIL(VV_E_LAUNCH, "vvm_despeckle: memset failed");
    const int rc = label("vvm_despeckle", dil, S, H, W, labels_ws, st);
    if (rc != VV_OK) return rc;
    const dim3 grid((unsigned)(((int64_t)N + MB - 1) / MB), (unsigned)S);
    hipLaunchKernelGGL(weigh_kernel, grid, dim3(MB), 0, st, raw, N, ch, labels_ws, weight_ws);
    hipLaunchKernelGGL(clear_kernel, grid, dim3(MB), 0, st, dil, N, min_area, labels_ws, weight_ws, out, (unsigned long long*)counts);
    VV_CHECK_LAUNCH("vvm_despeckle");
    return VV_OK;
}

extern "C" int vvm_time_bridge_grow(const uint8_t* in, int T, int H, int W, int bridge, int grow, uint8_t* out, int64_t* counts, void* stream) {
    if (!in || !out || !counts || T < 1 || H <= 0 || W <= 0 || bridge < 0 || grow < 0 || (int64_t)H * W >= ((int64_t)1 << 31))
        VV_FAIL(VV_E_ARG, "vvm_time_bridge_grow: bad args");
    if (bridge > VVM_MAX_BRIDGE || grow > VVM_MAX_GROW || T > VVM_MAX_T)
        VV_FAIL(VV_E_UNSUPPORTED, "vvm_time_bridge_grow: bridge <= %d, grow <= %d and T <= %d are supported, not bridge %d, grow %d, T %d", VVM_MAX_BRIDGE,
                VVM_MAX_GROW, VVM_MAX_T, bridge, grow, T);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)T * 2 * sizeof(int64_t), st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vvm_time_bridge_grow: memset failed");
    const int64_t N = (int64_t)H * W;
    const bool vec = N % 16 == 0 && (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0;
    const int64_t units = vec ? N / 16 : N;
    const dim3 grid((unsigned)((units + MB - 1) / MB));
    if (vec) hipLaunchKernelGGL(time_kernel<true>, grid, dim3(MB), 0, st, in, T, N, units, bridge, grow, out, (unsigned long long*)counts);
    else hipLaunchKernelGGL(time_kernel<false>, grid, dim3(MB), 0, st, in, T, N, units, bridge, grow, out, (unsigned long long*)counts);
    VV_CHECK_LAUNCH("vvm_time_bridge_grow");
    return VV_OK;
}
