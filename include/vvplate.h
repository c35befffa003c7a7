/* vvplate.h -- C ABI of the clean-plate fill entry points of libvvhip.so (videovanish_amd/csrc/vv_plate.hip; Python binding:
 * videovanish_amd/plate_hip.py; host: videovanish_amd/platefill.py, infill.plate_fill; rules: DESIGN.md section 16).
 *
 * Conventions are those of vvhip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void* (NULL = the null stream), the
 * return value is 0 = launched or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing launched), and vvp_last_error()
 * gives the message of the calling thread's last failure (the string vv_last_error() of vvhip.h returns).
 *
 * THE RULES.  A masked pixel whose background is visible, steadily, in other frames of the same shot at the same place is filled with the
 * nearest such frame's bytes and leaves the mask.  All arithmetic is integer, so the device result equals a host restatement bit for bit.
 * One call works on ONE segment (the frames between two cuts): frames [T][H][W][3] u8, dil [T][H][W] u8 (non-zero = masked).  Per pixel p:
 *
 *   1. Sample frames.  s is a sample frame of p when dil[s'][p] == 0 for every s' in [s - guard, s + guard] inside [0, T): the complement of
 *      vvm_time_bridge_grow(dil, 0, guard) of vvmask.h, which the caller runs; its output is `notsample` below (dil itself for guard = 0).
 *   2. Statistics.  Over the sample frames, per channel c: n, S1_c = sum v, S2_c = sum v * v (v = frames[s][p][c]).  Exact integers;
 *      T <= 65535 keeps n < 2^16, S1 < 2^24 and S2 < 2^32.
 *   3. Steady.  p is steady when n >= min_samples and n * S2_c - S1_c * S1_c <= tol * tol * n * n for every channel (a standard deviation of
 *      at most tol; equality counts), in 64 bits.
 *   4. Usable sample.  A sample frame s of a steady pixel is usable when |n * v_c - S1_c| <= outlier * tol * n for every channel.
 *   5. Source.  For dil[t][p] != 0 and p steady: src = the usable sample frame nearest to t in time, the smaller index at a tie; none when no
 *      usable frame exists, or when max_gap > 0 and |src - t| > max_gap.  src is a uint16, VVP_NO_SOURCE = none.
 *   6. Margin.  F = the masked pixels with a source, R0 = dil & ~F (vvp_sources writes it, 255 / 0).  The caller dilates R0 by `margin`
 *      iterations of the 3 x 3 cross (vv_mask_collapse_dilate of vvhip.h) into `keep`; dil' = keep & dil.
 *   7. Fill.  Where dil != 0 and dil' == 0: frames'[t][p] = frames[src][p].  A source pixel is unmasked and writes hit masked pixels only, so a
 *      source is never itself written and the fill runs in place.
 *   Counts [T][2] int64 per frame: (pixels filled, masked pixels left).
 *
 * TILES.  occ [ceil(H / tile)][ceil(W / tile)] u8 (vv_mask_tile_union of vvhip.h over dil) or NULL: a pixel whose tile has occ == 0 is masked in
 * no frame, needs nothing, and no kernel reads an image byte of it; its outputs are steady = n = S1 = 0, src = VVP_NO_SOURCE, R0 = dil' = 0.
 * NULL = every tile counts (the statistics of every pixel; same frames', dil' and counts).
 */
#ifndef VVPLATE_H
#define VVPLATE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVP_ABI_VERSION 1
#define VVP_MAX_T 65535
#define VVP_NO_SOURCE 65535
#define VVP_MAX_GUARD 8
#define VVP_MAX_TOL 255
#define VVP_MAX_OUTLIER 64
#define VVP_MAX_GAP 65535

int vvp_abi_version(void);
const char* vvp_last_error(void);

/* Rules 2 and 3.  steady [H][W] u8 (1 / 0), n [H][W] int32, s1 [H][W][3] int32.  T < 1, H * W >= 2^31, min_samples < 1, tol < 0, tile < 1 with
 * occ -> -1; T > 65535, tol > 255 -> -2. */
int vvp_stats(const uint8_t* frames, const uint8_t* notsample, const uint8_t* occ, int T, int H, int W, int tile, int min_samples, int tol,
              uint8_t* steady, int32_t* n, int32_t* s1, void* stream);

/* Rules 4 and 5, and R0 of rule 6, from vvp_stats' outputs.  src [T][H][W] uint16: the source frame where dil != 0 and one exists, else
 * VVP_NO_SOURCE.  r0 [T][H][W] u8: 255 where dil != 0 and there is no source, else 0.  outlier < 0, max_gap < 0 -> -1; outlier > 64,
 * max_gap > 65535 -> -2; the rest as vvp_stats. */
int vvp_sources(const uint8_t* frames, const uint8_t* dil, const uint8_t* notsample, const uint8_t* occ, const uint8_t* steady, const int32_t* n,
                const int32_t* s1, int T, int H, int W, int tile, int tol, int outlier, int max_gap, uint16_t* src, uint8_t* r0, void* stream);

/* Rule 7 and the counts, in place on frames.  keep [T][H][W] u8: the dilated R0.  dil_out [T][H][W] u8 (not dil): 255 where dil != 0 and
 * keep != 0, else 0.  A masked pixel outside keep whose src is not below T stays masked (a caller's error, never an access outside frames).
 * counts [T][2] int64, cleared first. */
int vvp_fill(uint8_t* frames, const uint8_t* dil, const uint8_t* keep, const uint8_t* occ, const uint16_t* src, int T, int H, int W, int tile,
             uint8_t* dil_out, int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
