// Mask-region inference (videovanish_amd/roi.py): the two device steps around a clip that was cropped to the masked area.
//   vv_mask_bbox            per-frame bounding box of the dilated masks (T*4 ints come back to the host, not the mask video)
//   vv_roi_paste_composite  model output of the window -> full frames: resize to the window, paste at the frame's offset, feather
//                           against the original with the full-frame mask; outside the window the original bytes
// HBM-bound byte kernels, one thread per pixel, coalesced along x.  The per-pixel arithmetic is vv_image_px.h, the same statement
// vv_resize_bilinear_u8 and vv_feather_composite use, so the fused paste equals that chain byte for byte.
#include "vv_image_px.h"
#pragma clang fp contract(off)

namespace {

constexpr int EB = 256;

// ---- bounding box -------------------------------------------------------------------------------------------
// identity of the (min y0, min x0, max y1, max x1) reduction: (H, W, 0, 0)
__global__ void bbox_init_kernel(int* bbox, int T, int H, int W) {
    const int t = blockIdx.x * EB + threadIdx.x;
    if (t >= T) return;
    bbox[t * 4 + 0] = H; bbox[t * 4 + 1] = W; bbox[t * 4 + 2] = 0; bbox[t * 4 + 3] = 0;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
// grid (row groups, T): block b of frame t scans rows b, b + gridDim.x, ...; each wave reduces its lanes' extents and, when it saw a mask
// pixel, folds them into the frame's box with four global integer atomics (min / max: order-independent, so the result is deterministic)
__global__ __launch_bounds__(EB) void bbox_kernel(const uint8_t* __restrict__ mask, int H, int W, int* bbox) {
    const int t = blockIdx.y;
    const uint8_t* img = mask + (int64_t)t * H * W;
    int y0 = H, x0 = W, y1 = 0, x1 = 0;
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        const uint8_t* row = img + (int64_t)y * W;
        for (int x = threadIdx.x; x < W; x += EB) {
            if (row[x] > 0) {
                y0 = min(y0, y); y1 = max(y1, y + 1);
                x0 = min(x0, x); x1 = max(x1, x + 1);
            }
        }
    }
    y0 = wave_min(y0); x0 = wave_min(x0);
    y1 = wave_max(y1); x1 = wave_max(x1);
    if ((threadIdx.x & 63) == 0 && y1 > 0) {
        int* b = bbox + t * 4;
        atomicMin(b + 0, y0); atomicMin(b + 1, x0);
        atomicMax(b + 2, y1); atomicMax(b + 3, x1);
    }
}
// frames without a mask pixel: (0, 0, 0, 0)
__global__ void bbox_finish_kernel(int* bbox, int T) {
    const int t = blockIdx.x * EB + threadIdx.x;
    if (t >= T) return;
    if (bbox[t * 4 + 2] == 0) { bbox[t * 4 + 0] = 0; bbox[t * 4 + 1] = 0; bbox[t * 4 + 3] = 0; }
}

// ---- paste + composite --------------------------------------------------------------------------------------
// pixel (x, y) of frame t: outside the window [oy, oy + h) x [ox, ox + w) the original; inside it the window pixel of the model output
// (Hm x Wm resized to h x w), feathered against the original with the full-frame mask (feather < 0: pasted as is).  Every read of
// `patch` stays inside frame t's Hm x Wm image whatever the offsets hold; every write is a pixel of the full frame.
__global__ __launch_bounds__(EB) void roi_paste_kernel(const uint8_t* __restrict__ patch, int Hm, int Wm, const uint8_t* __restrict__ orig,
                                                        const uint8_t* __restrict__ mask, const int* __restrict__ offsets, int T, int H, int W, int h,
                                                        int w, float feather, int R, uint8_t* __restrict__ out) {
    const int64_t n = (int64_t)T * H * W;
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % W); const int y = (int)((i / W) % H); const int t = (int)(i / ((int64_t)W * H));
    const int yy = y - offsets[t * 2 + 0], xx = x - offsets[t * 2 + 1];
    const uint8_t* o = orig + i * 3;
    uint8_t* d = out + i * 3;
    if (yy < 0 || yy >= h || xx < 0 || xx >= w) {
        d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
        return;
    }
    const uint8_t* src = patch + (int64_t)t * Hm * Wm * 3;
    uint8_t p[3];
    if (Hm == h && Wm == w) {
        const uint8_t* s = src + ((int64_t)yy * w + xx) * 3;
        p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
    } else {
        vvpx::bilinear_px(src, Hm, Wm, 3, xx, yy, h, w, p);
    }
    if (feather < 0.f) {
        d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
        return;
    }
    const float alpha = vvpx::feather_alpha(mask + (int64_t)t * H * W, H, W, x, y, feather, R);
    vvpx::feather_blend(alpha, p, o, d);
}

}  // namespace

extern "C" int vv_mask_bbox(const uint8_t* mask2d, int T, int H, int W, int* bbox, void* stream) {
    if (!mask2d || !bbox || T <= 0 || T > 65535 || H <= 0 || W <= 0) VV_FAIL(VV_E_ARG, "vv_mask_bbox: bad args");
    hipStream_t st = (hipStream_t)stream;
    const dim3 gt((unsigned)((T + EB - 1) / EB));
    hipLaunchKernelGGL(bbox_init_kernel, gt, dim3(EB), 0, st, bbox, T, H, W);
    // ~1024 blocks in all, at least one row per block
    int rows = 1024 / T;
    rows = rows < 1 ? 1 : (rows > H ? H : rows);
    hipLaunchKernelGGL(bbox_kernel, dim3((unsigned)rows, (unsigned)T), dim3(EB), 0, st, mask2d, H, W, bbox);
    hipLaunchKernelGGL(bbox_finish_kernel, gt, dim3(EB), 0, st, bbox, T);
    VV_CHECK_LAUNCH("vv_mask_bbox");
    return VV_OK;
}

extern "C" int vv_roi_paste_composite(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets, int T, int H0,
                                      int W0, int h, int w, float feather_px, uint8_t* out, void* stream) {
    if (!patch || !orig || !offsets || !out || T <= 0 || H0 <= 0 || W0 <= 0 || Hm <= 0 || Wm <= 0 || h <= 0 || w <= 0 || h > H0 || w > W0)
        VV_FAIL(VV_E_ARG, "vv_roi_paste_composite: bad args");
    if (feather_px >= 0.f && !mask2d) VV_FAIL(VV_E_ARG, "vv_roi_paste_composite: the feathered composite needs mask2d");
    if (feather_px > 64.f) VV_FAIL(VV_E_UNSUPPORTED, "vv_roi_paste_composite: feather_px %.1f > 64", feather_px);
    const int R = feather_px > 0.f ? (int)ceilf(feather_px) : 0;
    const int64_t n = (int64_t)T * H0 * W0;
    hipLaunchKernelGGL(roi_paste_kernel, dim3((unsigned)((n + EB - 1) / EB)), dim3(EB), 0, (hipStream_t)stream, patch, Hm, Wm, orig, mask2d, offsets, T, H0,
                       W0, h, w, feather_px, R, out);
    VV_CHECK_LAUNCH("vv_roi_paste_composite");
    return VV_OK;
}
