/* vvshadow.h -- C ABI of the shadow-masking entry points of libvvhip.so (videovanish_amd/csrc/vv_shadow.hip; Python binding:
 * videovanish_amd/shadow_hip.py; host: videovanish_amd/shadowmask.py, infill.shadow_mask; rules: DESIGN.md section 21).
 *
 * Conventions are those of vvhip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void* (NULL = the null stream), the
 * return value is 0 = launched or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing launched), and vvh_last_error()
 * gives the message of the calling thread's last failure (the string vv_last_error() of vvhip.h returns).
 *
 * THE RULES.  An unmasked pixel that looks like the shot's clean background uniformly darkened, and that hangs on to the frame's mask, joins the
 * mask: the cast shadow of the masked object.  Masks change, never a frame byte.  All arithmetic is integer, so the device result equals a host
 * restatement bit for bit.  One call works on ONE segment (the frames between two cuts): frames [T][H][W][3] u8, dil [T][H][W] u8 (non-zero =
 * masked).  Per pixel p:
 *
 *   1. Sample frames.  As rule 1 of vvplate.h: s is a sample frame of p when dil[s'][p] == 0 for every s' in [s - guard, s + guard] inside
 *      [0, T): the complement of vvm_time_bridge_grow(dil, 0, guard) of vvmask.h, which the caller runs; its output is `notsample` below (dil
 *      itself for guard = 0).
 *   2. Lit samples.  With L_s = v_r + v_g + v_b at frame s, n the number of samples and S = sum of L_s over them: a sample is lit when
 *      n * L_s + 3 * tol * n >= S.  A shadow only darkens, so this one-step trim removes the shadowed samples; the mean is pulled down by less
 *      than the shadow's own depth.
 *   3. Plate.  Over the lit samples, per channel c: n2, T1_c = sum v, T2_c = sum v * v.  p has a plate when n2 >= min_samples and
 *      n2 * T2_c - T1_c * T1_c <= tol * tol * n2 * n2 for every channel (equality counts).  T <= 65535 keeps T2 < 2^32: sums are 32-bit,
 *      compares 64-bit.
 *   4. Candidate.  cand[t][p] holds when all of these hold (64-bit; every product stays below 2^56):
 *        dil[t][p] == 0 and p has a plate;
 *        T1_c >= floor * n2 for every channel;
 *        lo * T1_c <= 100 * n2 * v_c <= hi * T1_c for every channel (v = frames[t][p]);
 *        sum over c of (T1_c - n2 * v_c) >= 3 * drop * n2 (signed): a mean darkening of at least `drop` levels, so noise on a dark plate is no
 *        shadow;
 *        for each channel pair (a, b): |v_a * T1_b - v_b * T1_a| * 100 * n2 <= chroma * T1_a * T1_b: the three darkening ratios agree to
 *        `chroma` percentage points.  A dark coloured object is not a shadow.
 *   5. Growth.  A_0 = (dil[t] != 0), A_{k+1} = A_k | (cand[t] & dilate3x3(A_k)) with the full 3 x 3 square, k < reach.  S = A_reach & ~A_0.
 *      Growth is per frame and stays inside the frame: a shadow must touch the frame's own mask and lie within `reach` steps of it.
 *   6. Small parts.  8-connected components of S with fewer than min_area pixels are dropped; min_area <= 1 drops nothing.  This is
 *      vvm_despeckle of vvmask.h with dil = raw = S, ch = 1, which the caller runs.
 *   7. Penumbra.  S' = dilate_cross(S, grow) & ~A_0 with the 3 x 3 cross of vv_mask_collapse_dilate of vvhip.h, which the caller runs.
 *      dil' = 255 where A_0 | S', else 0.
 *   8. Counts.  [T][2] int64 per frame: (candidate pixels, pixels added = |S'|).
 *
 * Limits: guard 0..8 (VVM_MAX_GROW of vvmask.h), min_samples 1..65535, tol 0..255, 0 <= lo <= hi <= 100, drop 0..255, chroma 0..100, floor 1..255,
 * reach 0..64, min_area 0..2^31 - 1, grow 0..16, T <= 65535.
 */
#ifndef VVSHADOW_H
#define VVSHADOW_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVH_ABI_VERSION 1
#define VVH_MAX_T 65535
#define VVH_MAX_GUARD 8
#define VVH_MAX_TOL 255
#define VVH_MAX_DROP 255
#define VVH_MAX_CHROMA 100
#define VVH_MAX_FLOOR 255
#define VVH_MAX_REACH 64
#define VVH_MAX_GROW 16
#define VVH_GROW_TILE 64        /* vvh_grow: a block owns a 64 x 64 interior ... */
#define VVH_GROW_K 8            /* ... with a halo of 8 pixels, and runs at most 8 sweeps of rule 5 a pass */

int vvh_abi_version(void);
const char* vvh_last_error(void);

/* Rules 2 and 3.  ok [H][W] u8 (1 = p has a plate, else 0), n2 [H][W] uint32, t1 [H][W][3] uint32.  A null pointer, T < 1, H * W >= 2^31,
 * min_samples < 1, tol < 0 -> -1; T > 65535, min_samples > 65535, tol > 255 -> -2. */
int vvh_plate(const uint8_t* frames, const uint8_t* notsample, int T, int H, int W, int min_samples, int tol, uint8_t* ok, uint32_t* n2,
              uint32_t* t1, void* stream);

/* Rule 4 from vvh_plate's outputs.  cand [T][H][W] u8 (1 / 0).  counts [T][2] int64, both columns cleared first: column 0 = the candidate
 * pixels of frame t.  A null pointer, lo < 0, hi < lo, drop < 0, chroma < 0, floor < 1 and vvh_plate's clip checks -> -1; hi > 100,
 * drop > 255, chroma > 100, floor > 255, T > 65535 -> -2. */
int vvh_candidates(const uint8_t* frames, const uint8_t* dil, const uint8_t* ok, const uint32_t* n2, const uint32_t* t1, int T, int H, int W,
                   int lo, int hi, int drop, int chroma, int floor, uint8_t* cand, int64_t* counts, void* stream);

/* Rule 5, frame by frame: a0 [T][H][W] u8 (non-zero = in A_0; dil), cand [T][H][W] u8 (non-zero = candidate) -> s [T][H][W] u8: 255 where
 * A_reach & ~A_0, else 0.  ceil(reach / VVH_GROW_K) passes of at most VVH_GROW_K sweeps each (one pass for reach = 0), ping-pong between s
 * and ws [T][H][W] u8 (contents undefined on entry and on return); nothing is read back between them.  s and ws are neither each other nor
 * an input.  A null pointer, reach < 0 and the clip checks -> -1; reach > 64, T > 65535 -> -2. */
int vvh_grow(const uint8_t* a0, const uint8_t* cand, int T, int H, int W, int reach, uint8_t* ws, uint8_t* s, void* stream);

/* Rule 7's union and the added-pixel counts: s [T][H][W] u8 = the dilated S of rule 7 (non-zero = set) -> dil_out [T][H][W] u8 (not dil): 255
 * where dil != 0 or s != 0, else 0; column 1 of counts [T][2] int64 (vvh_candidates cleared it) gains the pixels with s != 0 and dil == 0 of
 * frame t.  A null pointer, dil_out == dil and the clip checks -> -1; T > 65535 -> -2. */
int vvh_merge(const uint8_t* dil, const uint8_t* s, int T, int H, int W, uint8_t* dil_out, int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
