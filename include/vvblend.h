/* vvblend.h -- C ABI of the seam membrane blending entry points of libvvhip.so (videovanish_amd/csrc/vv_blend.hip; Python binding:
 * videovanish_amd/blend_hip.py; rules: DESIGN.md section 15).
 *
 * Conventions are those of vvhip.h, vvtone.h and vvgrain.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void* (NULL
 * = the null stream), the return value is 0 = launched or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing
 * launched), and vvb_last_error() gives the message of the calling thread's last failure (the string vv_last_error() of vvhip.h returns).  A
 * window is seen as vvt_ring_stats sees it: frame t's window is [oy, oy + h) x [ox, ox + w) of the H0 x W0 frame, (oy, ox) = offsets[t]; its
 * pixel x is the model's Hm x Wm output resized to h x w (cv2's fixed-point INTER_LINEAR; the bytes as they are when Hm x Wm is h x w) and then
 * sent through lut [T][3][256] u8; y is orig.  The full frame is the window (0, 0, H0, W0).
 *
 * THE FIELD.  All arithmetic is integer; "//" is the floor division, ">>" the arithmetic shift.  Values are Q6 (1/64 level) int16.
 *   cells    level 0 is the h x w window, level l + 1 has h' = (h_l + 1) / 2 rows and w' = (w_l + 1) / 2 columns; levels are added while
 *            max(h_l, w_l) > 2 (vvb_levels).  The children of cell (Y, X) are the cells (2Y + a, 2X + b), a, b in {0, 1}, that exist.
 *   classes  VVB_KNOWN at level 0: a ring pixel as vvtone.h defines it (inside the window and the frame, mask2d == 0, a mask pixel of the frame
 *            within `ring` pixels, a box); VVB_UNKNOWN: a pixel of the window with mask2d != 0; VVB_INACTIVE: every other one.  At level
 *            l + 1 a cell is known when a child is known, else unknown when a child is unknown, else inactive.
 *   known    level 0: with d_c = y_c - x_c, S_c = the sum of d_c and N = the number of the ring pixels of the window within `presmooth` pixels
 *            (a box) of p: v_c(p) = clamp((2 * 64 * S_c + N) // (2 N), -64 max_shift, 64 max_shift).  Level l + 1: with S_c the sum of the
 *            known children's values and N their number: v_c = (2 S_c + N) // (2 N).  Inactive cells hold 0.
 *   unknown  from the top level down: an unknown cell (Y, X) starts from the value of its parent (Y >> 1, X >> 1) (known or unknown, never
 *            inactive), at the top level from 0; then `sweeps` Jacobi sweeps over all unknown cells of the level at once, each reading only
 *            the sweep before: v_c <- (N_c + S_c + W_c + E_c + 2) >> 2, the four 4-neighbours' values, a neighbour that lies outside the level's
 *            grid or is inactive (a pixel outside the frame) replaced by the cell's own value.
 * The level-0 values m are the field: 0 on inactive cells, and x + m = y up to the presmoothing on the ring.
 *
 * SCRATCH of T frames of an h x w window: level after level, val_l [T][h_l][w_l][3] int16 then cls_l [T][h_l][w_l] u8, each level's block
 * rounded up to 16 bytes: vvb_scratch_bytes = sum over l of ((7 T h_l w_l + 15) & ~15).  The field is val_0, the first bytes.
 */
#ifndef VVBLEND_H
#define VVBLEND_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVB_ABI_VERSION 1
#define VVB_MAX_RING 32
#define VVB_MAX_PRESMOOTH 4
#define VVB_MAX_SWEEPS 16
#define VVB_MAX_SHIFT 255
#define VVB_MAX_STRENGTH_Q8 512
#define VVB_INACTIVE 0
#define VVB_KNOWN 1
#define VVB_UNKNOWN 2
/* per frame: [0] ring pixels, [1..3] the sum of d_c^2 over them (levels^2), [4] unknown pixels of the window, [5..7] the sum and [8..10] the
 * largest of |m_c| (Q6) over those */
#define VVB_NSUM 11

int vvb_abi_version(void);
const char* vvb_last_error(void);

/* The number of levels of an h x w window, and the bytes of scratch T frames of it need; -1 for a size <= 0. */
int vvb_levels(int h, int w);
int64_t vvb_scratch_bytes(int T, int h, int w);

/* Level 0 before the solve.  patch [T][Hm][Wm][3] u8, orig [T][H0][W0][3] u8, mask2d [T][H0][W0] u8, offsets [T][2] int32, lut [T][3][256] u8
 * -> cls [T][h][w] u8, val [T][h][w][3] int16 (the known cells' values, 0 elsewhere) and sums [T][VVB_NSUM] int64, cleared first, entries 0 .. 3.
 * A 64 x 32 tile without a ring pixel reads no image byte.  Null pointer, a size <= 0, h > H0, w > W0 -> -1; ring outside 1 .. VVB_MAX_RING,
 * presmooth outside 0 .. VVB_MAX_PRESMOOTH, max_shift outside 1 .. VVB_MAX_SHIFT, or more than 2^31 - 1 tiles -> -2. */
int vvb_ring_diff(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets, const uint8_t* lut, int T,
                  int H0, int W0, int h, int w, int ring, int presmooth, int max_shift, uint8_t* cls, int16_t* val, int64_t* sums, void* stream);

/* One pull step: cls / val of T frames of an hl x wl level -> cls_up / val_up of the ((hl + 1) / 2) x ((wl + 1) / 2) level above. */
int vvb_pull(const uint8_t* cls, const int16_t* val, int T, int hl, int wl, uint8_t* cls_up, int16_t* val_up, void* stream);

/* `sweeps` Jacobi sweeps on one hl x wl level in ONE launch (a block keeps its 64 x 32 tile and a halo of `sweeps` cells in LDS).  start 1: the
 * unknown cells start from `parent` (the values of the level above, NULL: from 0) and `val` is read on known cells only, so out may be val;
 * start 0: they start from `val`, and out must be another buffer.  out gets every cell of the level.  sums (or NULL) [T][VVB_NSUM], which the
 * caller has cleared, gets entries 4 .. 7 ADDED to and entries 8 .. 10 RAISED to (a maximum) from the unknown cells of out.  sweeps outside
 * 1 .. VVB_MAX_SWEEPS, or more than 2^31 - 1 tiles -> -2; start outside {0, 1}, start 0 with out == val -> -1. */
int vvb_relax(const uint8_t* cls, const int16_t* val, const int16_t* parent, int16_t* out, int T, int hl, int wl, int sweeps, int start,
              int64_t* sums, void* stream);

/* The whole field: vvb_ring_diff into level 0 of scratch, vvb_pull up to the top, vvb_relax (start 1, in place) from the top down; the field
 * and its classes are then val_0 and cls_0 of scratch, sums holds all VVB_NSUM entries.  scratch_bytes < vvb_scratch_bytes(T, h, w) -> -1;
 * the other refusals are those of the three steps. */
int vvb_solve(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets, const uint8_t* lut, int T,
              int H0, int W0, int h, int w, int ring, int presmooth, int sweeps, int max_shift, void* scratch, int64_t scratch_bytes,
              int64_t* sums, void* stream);

/* vvg_paste_grain_composite with one more step: inside the window, after the table and before the grain (whose amplitude is looked up at the
 * tabled value, before the membrane), channel c of the window's pixel p becomes
 *   p_c <- clip(lut(p_c) + ((m_c * strength_q8 + (1 << 13)) >> 14), 0, 255),     m = field [T][h][w][3] int16 (Q6), strength_q8 0 .. 512
 * and then gets its grain: clip(p_c + g_c), g_c the d_c of vvgrain.h from amp[t][c][lut(p_c)].  With a zero field (or strength_q8 0) the bytes
 * are vvg_paste_grain_composite's, with amp all zero as well vvt_paste_lut_composite's.  Refusals as vvg_paste_grain_composite, and
 * strength_q8 outside 0 .. VVB_MAX_STRENGTH_Q8 -> -2. */
int vvb_paste_blend_composite(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets,
                              const uint8_t* lut, const int16_t* field, int strength_q8, const uint8_t* amp, const int* frame_ids, int seed, int mode,
                              int T, int H0, int W0, int h, int w, float feather_px, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
