// Mask-region inference (videovanish_amd/roi.py): the two device steps around a clip that was cropped to the masked area.
//   vv_mask_bbox            per-frame bounding box of the dilated masks (T*4 ints come back to the host, not the mask video)
//   vv_mask_tile_union      occupancy of the clip's mask footprint on a grid of tile x tile cells (the host labels its components)
//   vv_mask_bbox_tiles      per-frame bounding box of each labelled component, reading only the occupied tiles
//   vv_roi_paste_composite  model output of the window -> full frames: resize to the window, paste at the frame's offset, feather
//                           against the original with the full-frame mask; outside the window the original bytes
// HBM-bound byte kernels, one thread per pixel, coalesced along x.  The per-pixel arithmetic is vv_image_px.h, the same statement
// vv_resize_bilinear_u8 and vv_feather_composite use, so the fused paste equals that chain byte for byte.
#include "vv_image_px.h"
#include "vv_wave_bytes.h"
#pragma clang fp contract(off)

namespace {

using vvwave::wave_max;
using vvwave::wave_min;
constexpr int EB = 256;

// ---- bounding box -------------------------------------------------------------------------------------------
// identity of the (min y0, min x0, max y1, max x1) reduction: (H, W, 0, 0)
__global__ void bbox_init_kernel(int* bbox, int T, int H, int W) {
    const int t = blockIdx.x * EB + threadIdx.x;
    if (t >= T) return;
    bbox[t * 4 + 0] = H; bbox[t * 4 + 1] = W; bbox[t * 4 + 2] = 0; bbox[t * 4 + 3] = 0;
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

// ---- tile occupancy ----------------------------------------------------------------------------------------
// grid (row bands, T): block b of frame t scans the contiguous rows [b * rows, (b + 1) * rows); a thread that sees a non-zero byte stores 1
// into its cell unless it stored into that cell last (the rows of one tile row follow each other).  Every writer stores the same byte, so
// the result does not depend on the order.  Cells are < ceil(H / tile) * ceil(W / tile) for every y < H, x < W.
__global__ __launch_bounds__(EB) void tile_union_kernel(const uint8_t* __restrict__ mask, int H, int W, int tile, int rows, int Wc, uint8_t* occ) {
    const uint8_t* img = mask + (int64_t)blockIdx.y * H * W;
    const int ya = blockIdx.x * rows;
    const int yb = min(H, ya + rows);
    for (int x = threadIdx.x; x < W; x += EB) {
        const int cx = x / tile;
        int64_t last = -1;
        for (int y = ya; y < yb; ++y) {
            const int64_t cell = (int64_t)(y / tile) * Wc + cx;
            if (cell != last && img[(int64_t)y * W + x] > 0) {
                occ[cell] = 1;
                last = cell;
            }
        }
    }
}

// ---- bounding box per labelled component --------------------------------------------------------------------
// identity of the reduction for each (frame, label)
__global__ void bbox_tiles_init_kernel(int* bbox, int64_t n, int H, int W) {
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= n) return;
    bbox[i * 4 + 0] = H; bbox[i * 4 + 1] = W; bbox[i * 4 + 2] = 0; bbox[i * 4 + 3] = 0;
}
// grid (n, T): block i scans tile tiles[i] = (ty, tx, label) of frame t, each wave reduces its lanes' extents and, when it saw a mask pixel,
// folds them into bbox[t][label] with four integer atomics.  An entry outside the grid or with a label outside [0, K) is skipped, so every
// read stays inside frame t and every write inside bbox whatever `tiles` holds.
__global__ __launch_bounds__(EB) void bbox_tiles_kernel(const uint8_t* __restrict__ mask, int H, int W, int tile, const int* __restrict__ tiles, int K,
                                                        int* bbox) {
    const int t = blockIdx.y;
    const int ty = tiles[(int64_t)blockIdx.x * 3 + 0], tx = tiles[(int64_t)blockIdx.x * 3 + 1], k = tiles[(int64_t)blockIdx.x * 3 + 2];
    if (ty < 0 || tx < 0 || ty > (H - 1) / tile || tx > (W - 1) / tile || k < 0 || k >= K) return;
    const int ya = ty * tile, xa = tx * tile;
    const int th = min(tile, H - ya), tw = min(tile, W - xa);
    const uint8_t* img = mask + (int64_t)t * H * W;
    int y0 = H, x0 = W, y1 = 0, x1 = 0;
    const int64_t np = (int64_t)th * tw;
    for (int64_t i = threadIdx.x; i < np; i += EB) {
        const int y = ya + (int)(i / tw), x = xa + (int)(i % tw);
        if (img[(int64_t)y * W + x] > 0) {
            y0 = min(y0, y); y1 = max(y1, y + 1);
            x0 = min(x0, x); x1 = max(x1, x + 1);
        }
    }
    y0 = wave_min(y0); x0 = wave_min(x0);
    y1 = wave_max(y1); x1 = wave_max(x1);
    if ((threadIdx.x & 63) == 0 && y1 > 0) {
        int* b = bbox + ((int64_t)t * K + k) * 4;
        atomicMin(b + 0, y0); atomicMin(b + 1, x0);
        atomicMax(b + 2, y1); atomicMax(b + 3, x1);
    }
}
// (frame, label) without a mask pixel: (0, 0, 0, 0)
__global__ void bbox_tiles_finish_kernel(int* bbox, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
    if (i >= n) return;
    if (bbox[i * 4 + 2] == 0) { bbox[i * 4 + 0] = 0; bbox[i * 4 + 1] = 0; bbox[i * 4 + 3] = 0; }
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

extern "C" int vv_mask_tile_union(const uint8_t* mask2d, int T, int H, int W, int tile, uint8_t* occ, void* stream) {
    if (!mask2d || !occ || T <= 0 || T > 65535 || tile <= 0 || H <= 0 || W <= 0) VV_FAIL(VV_E_ARG, "vv_mask_tile_union: bad args");
    hipStream_t st = (hipStream_t)stream;
    const int Hc = (H - 1) / tile + 1, Wc = (W - 1) / tile + 1;
    if (hipMemsetAsync(occ, 0, (size_t)Hc * Wc, st) != hipSuccess) VV_FAIL(VV_E_LAUNCH, "vv_mask_tile_union: memset failed");
    // ~1024 blocks in all, bands of whole tile rows where the frame allows it
    int bands = 1024 / T;
    bands = bands < 1 ? 1 : (bands > H ? H : bands);
    int rows = (H + bands - 1) / bands;
    if (rows > tile) rows = (rows + tile - 1) / tile * tile;
    bands = (H + rows - 1) / rows;
    hipLaunchKernelGGL(tile_union_kernel, dim3((unsigned)bands, (unsigned)T), dim3(EB), 0, st, mask2d, H, W, tile, rows, Wc, occ);
    VV_CHECK_LAUNCH("vv_mask_tile_union");
    return VV_OK;
}

extern "C" int vv_mask_bbox_tiles(const uint8_t* mask2d, int T, int H, int W, int tile, const int* tiles, int n, int K, int* bbox, void* stream) {
    if (!mask2d || !tiles || !bbox || T <= 0 || T > 65535 || tile <= 0 || H <= 0 || W <= 0 || n < 0 || K <= 0)
        VV_FAIL(VV_E_ARG, "vv_mask_bbox_tiles: bad args");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = (int64_t)T * K;
    const dim3 gb((unsigned)((nb + EB - 1) / EB));
    hipLaunchKernelGGL(bbox_tiles_init_kernel, gb, dim3(EB), 0, st, bbox, nb, H, W);
    if (n > 0) hipLaunchKernelGGL(bbox_tiles_kernel, dim3((unsigned)n, (unsigned)T), dim3(EB), 0, st, mask2d, H, W, tile, tiles, K, bbox);
    hipLaunchKernelGGL(bbox_tiles_finish_kernel, gb, dim3(EB), 0, st, bbox, nb);
    VV_CHECK_LAUNCH("vv_mask_bbox_tiles");
    return VV_OK;
}
