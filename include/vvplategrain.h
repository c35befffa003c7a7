/* vvplategrain.h -- C ABI of the rotated clean-plate sources of libvvhip.so (videovanish_amd/csrc/vv_plate.hip; Python binding:
 * videovanish_amd/plategrain_hip.py; host: videovanish_amd/plategrain.py, infill.plate_fill(gcfg=); rules: DESIGN.md section 20).
 *
 * Conventions are those of vvplate.h, on which this header builds: device pointers, `stream` a hipStream_t as void*, 0 = launched or a negative
 * code (-1 bad argument, -2 unsupported, -3 launch failed; nothing launched), vvl_last_error() = the message of the calling thread's last
 * failure (the string vv_last_error() of vvhip.h returns).
 *
 * THE RULE.  The clean-plate fill of vvplate.h pastes, into every masked frame of a steady pixel, the bytes of the NEAREST usable sample frame:
 * one frame's grain then stands still inside the fill for as long as that frame stays the nearest.  Here the fill takes its bytes from a
 * small set of usable frames in turn.  Rules 1 - 6 of vvplate.h hold unchanged.  Two settings are new: depth (1 .. 8) and reach (1 .. 65535).
 * For a masked frame t of a steady pixel p whose rule-5 source src exists (after max_gap):
 *
 *   Side.        "before" when src < t, "after" when src > t.
 *   Candidates.  c_0 = src; c_1, c_2, ... = the next usable sample frames (rule 4) of p going away from t on that side: descending indices
 *                before, ascending after.
 *   Limits.      Of the first `depth` candidates, those with |c_i - c_0| <= reach and, when max_gap > 0, |c_i - t| <= max_gap are kept.
 *                Both distances grow with i, so the kept candidates are a prefix c_0 .. c_(m-1), m >= 1.
 *   Live source. live[t][p] = c_k with k = t mod m, t being the frame's index in this call's segment.  Where src is VVP_NO_SOURCE, live is too.
 *   Fill.        Rule 7 of vvplate.h with live in place of src (vvp_fill, handed live).
 *
 * So depth = 1 gives live == src; src and r0, and with them dil' and the counts, are vvp_sources' bit for bit; every live source is a usable
 * sample frame of its pixel on the side of src, within reach of it and within max_gap of t, hence unmasked: vvp_fill still runs in place; and
 * two consecutive masked frames of a pixel that take the same side share their candidates, so with the same m >= 2 they never take the same
 * frame.  Only max_gap can give them different m (it counts from t); with max_gap = 0 they never differ.
 */
#ifndef VVPLATEGRAIN_H
#define VVPLATEGRAIN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVL_ABI_VERSION 1
#define VVL_MAX_DEPTH 8
#define VVL_MAX_REACH 65535

int vvl_abi_version(void);
const char* vvl_last_error(void);

/* vvp_sources of vvplate.h (the same arguments, src and r0 the same bytes) plus the rule above: live [T][H][W] uint16.  A pixel of a tile
 * with occ == 0 gets live = VVP_NO_SOURCE.  Refused as vvp_sources refuses, and: live null, depth < 1, reach < 1 -> -1; depth > 8,
 * reach > 65535 -> -2. */
int vvl_sources(const uint8_t* frames, const uint8_t* dil, const uint8_t* notsample, const uint8_t* occ, const uint8_t* steady, const int32_t* n,
                const int32_t* s1, int T, int H, int W, int tile, int tol, int outlier, int max_gap, int depth, int reach, uint16_t* src,
                uint16_t* live, uint8_t* r0, void* stream);

#ifdef __cplusplus
}
#endif
#endif
