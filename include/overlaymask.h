/* overlaymask.h -- C ABI of the overlay-masking entry points of libvvhip.so (videovanish_amd/csrc/vv_overlay.hip; Python binding:
 * videovanish_amd/overlaymask_bind.py; host: videovanish_amd/overlaymask.py, infill.overlay_mask; rules: DESIGN.md section 27).
 *
 * Conventions are those of vvhip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void* (NULL = the null stream), the
 * return value is 0 = launched or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing launched), and vvo_last_error()
 * gives the message of the calling thread's last failure (the string vv_last_error() of vvhip.h returns).
 *
 * THE RULES.  A screen-fixed graphic (a station logo, a channel bug, the frame of a timestamp) keeps its edges at the same pixels in every
 * frame while the picture under them changes: where the gradient keeps its sign over the clip there is an overlay, where it averages out
 * there is scene.  Masks change, never a frame byte.  All arithmetic is integer, so the device result equals a host restatement bit for
 * bit.  One call works on the whole clip call; a cut is no boundary (it changes the background, which only helps).  frames [T][H][W][3] u8,
 * dil [T][H][W] u8 (the dilated and cleaned masks, non-zero = masked).  Per pixel p = (y, x):
 *
 *   1. Gradients.  Y = the rounded Rec. 601 luma (77 r + 150 g + 29 b + 128) >> 8.  With the frame's border replicated (Y at a coordinate
 *      outside the frame is Y at the nearest pixel inside):
 *        gx = Y(y-1, x+1) + 2 Y(y, x+1) + Y(y+1, x+1) - Y(y-1, x-1) - 2 Y(y, x-1) - Y(y+1, x-1)
 *        gy = Y(y+1, x-1) + 2 Y(y+1, x) + Y(y+1, x+1) - Y(y-1, x-1) - 2 Y(y-1, x) - Y(y-1, x+1)          (|g| <= 1020)
 *      Frame t counts at p when dil[t][p] == 0 (an object that passes over the graphic gives no sample there; the neighbours' bytes are read
 *      whatever their masks say).  Over the counted frames: n, Sx = sum gx, Sy = sum gy, A = sum (|gx| + |gy|), int32 each.  T <= 65535
 *      keeps A <= 65535 * 2040 < 2^31.  Every compare below is 64-bit.
 *   2. Persistent edges.  strong(p): n >= min_samples and A >= mag * n.  E(p): strong(p) and 100 * (|Sx| + |Sy|) >= coh * A.  Equality
 *      counts in both.  Counts: strong = |{p: strong(p)}|, edges = |E|.
 *   3. Guard.  strong == 0: verdict "none".  100 * edges > max_share * strong: verdict "static" (the scene does not move: every edge is
 *      persistent).  Both add nothing.  The host decides this from vvo_classify's counts.
 *   4. Closing.  C = E dilated `close` times with the 3 x 3 cross: vv_mask_collapse_dilate of vvhip.h, which the caller runs.
 *   5. Holes.  Of the 8-connected components of ~C (as vvm_label_components of vvmask.h labels them, which the caller runs), one joins when
 *      its bounding box touches no frame border and it holds at most max_hole pixels: F = C | holes.  A stroke's interior, a translucent
 *      plate's flat inside.
 *   6. Selection.  A component of F is kept when area >= min_area, 100 * area <= max_area * H * W and, unless border = 1, its bounding box
 *      touches no frame border.  Nothing kept: verdict "none"; else "found".
 *   7. Fringe.  O = the kept pixels dilated `grow` times with the cross.  dil'[t] = 255 where dil[t] != 0 or O, for every frame of the call.
 *   8. Counts.  added[t] = |O & (dil[t] == 0)|; the kept components as (label, area, x0, y0, x1, y1) with x1, y1 exclusive, at most
 *      VVO_MAX_BOXES of them (those of the smallest labels when there are more; in label order only then: the host sorts), the true count
 *      beside them.
 *
 * A bounding box (x0, y0, x1, y1) touches a frame border when x0 == 0, y0 == 0, x1 == W or y1 == H.
 *
 * Limits: min_samples 1..65535, mag 1..2040, coh 1..100, max_share 0..100, close 0..16, max_hole 0..2^31 - 1, min_area 0..2^31 - 1,
 * max_area 1..100, border 0 / 1, grow 0..16, T <= 65535, H * W < 2^31.  The defaults of the settings (videovanish_amd/overlaymask.py) are
 * build-defined: they come from synthetic clips; nobody has run real footage through this stage.
 */
#ifndef OVERLAYMASK_H
#define OVERLAYMASK_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVO_ABI_VERSION 1
#define VVO_MAX_T 65535
#define VVO_MAX_MAG 2040
#define VVO_MAX_COH 100
#define VVO_MAX_BOXES 256
#define VVO_TILE_W 64           /* vvo_accumulate: a block owns a tile of 64 x 16 pixels ... */
#define VVO_TILE_H 16           /* ... and stages its luma with a halo of one pixel */

int vvo_abi_version(void);
const char* vvo_last_error(void);

/* Rule 1 for a batch of Tb frames: frames [Tb][H][W][3] u8, dil [Tb][H][W] u8; the four sums (n, Sx, Sy, A) of the batch are ADDED to
 * acc [H][W][4] int32, which the caller cleared before the first batch.  Splitting a clip into batches in any way gives the same acc.
 * A null pointer, Tb < 1, H < 1, W < 1, H * W >= 2^31 -> -1; Tb > 65535 -> -2. */
int vvo_accumulate(const uint8_t* frames, const uint8_t* dil, int Tb, int H, int W, int32_t* acc, void* stream);

/* Rule 2 from acc [H][W][4] int32 (any sums: acc is an input).  edge [H][W] u8: 255 where E, else 0.  counts [2] int64, cleared first:
 * (strong, edges).  A null pointer, H < 1, W < 1, H * W >= 2^31, min_samples < 1, mag < 1, coh < 1 -> -1; min_samples > 65535,
 * mag > 2040, coh > 100 -> -2. */
int vvo_classify(const int32_t* acc, int H, int W, int min_samples, int mag, int coh, uint8_t* edge, int64_t* counts, void* stream);

/* Area and bounding box of every component of labels [H][W] int32 (vvm_label_components' output: the smallest linear index of the pixel's
 * component, -1 = none).  stats [H * W][5] int32, cleared by the call to (0, W, H, 0, 0); row l of a label l then holds (area, x0, y0, x1,
 * y1), x1 and y1 exclusive.  Integer add / min / max only: thread order cannot matter.  A label outside [-1, H * W) is ignored.  A null
 * pointer, H < 1, W < 1, H * W >= 2^31 -> -1. */
int vvo_component_stats(const int32_t* labels, int H, int W, int32_t* stats, void* stream);

/* out [H][W] u8 = 255 where the pixel's component is kept, else 0.  Kept: min_area <= area <= max_area_px and, with inside_only != 0, a
 * bounding box that touches no frame border.  boxes [VVO_MAX_BOXES][6] int32 = (label, area, x0, y0, x1, y1) of kept components (rule 8;
 * rows past the count are not written), nboxes [1] int32 = the true count, cleared first.  Rule 5: min_area = 0, max_area_px = max_hole,
 * inside_only = 1.  Rule 6: inside_only = !border, max_area_px = max_area * H * W / 100 rounded down.  A null pointer, H < 1, W < 1,
 * H * W >= 2^31, min_area < 0, max_area_px < 0 -> -1. */
int vvo_select(const int32_t* labels, const int32_t* stats, int H, int W, int min_area, int max_area_px, int inside_only, uint8_t* out,
               int32_t* boxes, int32_t* nboxes, void* stream);

/* Rule 7's union and rule 8's counts: dil [T][H][W] u8, o [H][W] u8 (non-zero = set; the same map for every frame) -> dil_out [T][H][W] u8
 * (not dil): 255 where dil != 0 or o != 0, else 0; added [T] int64, cleared first: the pixels with o != 0 and dil == 0 of frame t.  A null
 * pointer, dil_out == dil, T < 1, H < 1, W < 1, H * W >= 2^31 -> -1; T > 65535 -> -2. */
int vvo_merge(const uint8_t* dil, const uint8_t* o, int T, int H, int W, uint8_t* dil_out, int64_t* added, void* stream);

#ifdef __cplusplus
}
#endif
#endif
