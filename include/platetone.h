/* platetone.h -- C ABI of the clean-plate exposure matching of libvvhip.so (videovanish_amd/csrc/vv_platetone.hip; Python binding:
 * videovanish_amd/platetone_bind.py; host: videovanish_amd/platetone.py, infill.plate_fill(tcfg=); rules: DESIGN.md section 23).
 *
 * Conventions are those of vvplate.h, on which this header builds: device pointers, `stream` a hipStream_t as void*, 0 = launched or a negative
 * code (-1 bad argument, -2 unsupported, -3 launch failed; nothing launched, nothing cleared), vve_last_error() = the message of the calling
 * thread's last failure (the string vv_last_error() of vvhip.h returns).
 *
 * THE RULES.  The clean-plate fill of vvplate.h calls a pixel steady only when its samples agree to `tol` levels across the whole segment, so
 * a clip whose exposure drifts or flickers fills nothing.  Here every frame of a segment is mapped to the segment's common exposure before
 * the fill samples it, and every filled pixel is mapped back to the exposure of the frame it lands in.  All arithmetic is integer; the host
 * side uses exact integers and no float decides a byte.  `//` is floor division.  One call works on ONE segment: v_t[p][c] =
 * frames[t][p][c], T frames of h x w pixels.  Settings: mode (affine | gain | offset), ring, floor, min_pixels, max_gain (percent), max_offset.
 *
 *   1. Crop and support.  The crop is platefill.crop_box widened by `ring` pixels on every side (shadowmask.widen_box): a crossing object's
 *      union box is otherwise all mask.  notsample is rule 1 of vvplate.h, the plane the fill itself samples by.  U0[p] = 1 when
 *      notsample[t][p] == 0 for every frame t of the segment: the pixels that are never masked, nor within `guard` frames of a mask.
 *   2. Mean image.  P[p][c] = sum over t of v_t[p][c], in a u32: T <= 65535 keeps it below 2^24 * 2^8 = 2^32.  R[p][c] = (2 P + T) // (2 T),
 *      a u8: the rounded mean.  U[p] = 1 when U0[p] = 1 and floor <= R[p][c] <= 255 - floor in all three channels (equality counts): pixels
 *      that clip give no evidence.  n = the number of pixels in U.  A segment with n < min_pixels is UNFIT: every frame's tables are the
 *      identity.
 *   3. Moments over U, 64-bit sums.  Per channel: Sr = sum R, Srr = sum R * R.  Per frame and channel: Sv = sum v, Svr = sum v * R.  With
 *      h * w <= 2^24: n <= 2^24, Sr and Sv < 2^32, Srr and Svr < 2^40.
 *   4. Fit, on the host, of v ~ a R + b per frame and channel with exact rationals a = an / ad (ad > 0) and b = bn / bd (bd > 0).
 *        affine   N = n Svr - Sv Sr, D = n Srr - Sr Sr; a = N / D, b = (Sv - a Sr) / n.  When D < 16 n n (the support's standard deviation
 *                 of R is under 4 levels: the slope means nothing) the frame and channel take `gain`.
 *        gain     a = Sv / Sr (a = 1 when Sr == 0), b = 0.
 *        offset   a = 1, b = (Sv - Sr) / n.
 *      Clamps, by integer comparison, in this order: (100 + max_gain) an < 100 ad -> a = 100 / (100 + max_gain); 100 an > (100 + max_gain) ad
 *      -> a = (100 + max_gain) / 100; then b is formed with the clamped a (in mode gain it stays 0): bn = Sv ad - an Sr, bd = ad n; then
 *      |bn| > max_offset bd -> b = +-max_offset.
 *   5. Tables [T][3][256] u8, both monotone, rounded to nearest with halves up as rule 2 does:
 *        forward  G_t[c][v] = clamp(round((v - b) / a)) = min(max((2 (v bd - bn) ad + bd an) // (2 bd an), 0), 255)
 *        back     B_t[c][u] = clamp(round(a u + b))     = min(max((2 (an u bd + bn ad) + ad bd) // (2 ad bd), 0), 255)
 *      A frame whose three G_t are the identity is flagged IDENTITY, and its B_t are made the identity too: it is at the common exposure.
 *   6. Segment paths.  If every frame of the segment is identity (an unfit segment is), nothing more runs: the fill of vvplate.h runs on its
 *      own crop and the bytes are those without this stage.  Otherwise f' = G_t[f] over the whole crop (vve_apply), the fill of vvplate.h
 *      (with the live sources of vvplategrain.h when they are asked for) runs on (f', d) and gives (f'', d2), and the crop that returns is
 *        out[t][p][c] = (d[t][p] != 0 && d2[t][p] == 0) ? B_t[c][f''[t][p][c]] : f[t][p][c]                                  (vve_restore)
 *      so a pixel that is not filled keeps its original bytes.  d2, the counts and the fill's report are the fill's.
 *   7. With the alignment of vvalign.h: a segment on its "static" path is treated as above; a segment filled on the canvas is not matched
 *      (under a pan the never-masked common set is empty).
 *
 * The limits and the defaults (ring 32, floor 16, min_pixels 1024, max_gain 25, max_offset 32) are build-defined: they come from reasoning and
 * synthetic clips; nobody has run real footage through this stage.
 */
#ifndef PLATETONE_H
#define PLATETONE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVE_ABI_VERSION 1
#define VVE_MAX_T 65535
#define VVE_MAX_PIXELS (1 << 24)
#define VVE_MAX_RING 64
#define VVE_MAX_FLOOR 127
#define VVE_MAX_GAIN 100
#define VVE_MAX_OFFSET 255
#define VVE_NSUM 12

int vve_abi_version(void);
const char* vve_last_error(void);

/* Rules 1 and 2.  frames [T][H][W][3] u8, notsample [T][H][W] u8 -> mean [H][W][3] u8 = R, support [H][W] u8 = U (1 / 0), n [1] int64 (cleared
 * first).  A null pointer, T < 1, H < 1, W < 1, floor < 0 -> -1; T > 65535, H * W > 2^24, floor > 127 -> -2. */
int vve_mean_plane(const uint8_t* frames, const uint8_t* notsample, int T, int H, int W, int floor, uint8_t* mean, uint8_t* support, int64_t* n,
                   void* stream);

/* Rule 3.  sums [T][12] int64, cleared first: row t = Sv[3], Svr[3] of frame t, then Sr[3], Srr[3] on row 0 and zeros on every other row (the
 * blocks of frame 0 add them in the same launch).  An image byte is read only where support is set.  Refused as vve_mean_plane refuses. */
int vve_moments(const uint8_t* frames, const uint8_t* mean, const uint8_t* support, int T, int H, int W, int64_t* sums, void* stream);

/* f' of rule 6: out[t][p][c] = fwd[t][c][frames[t][p][c]], fwd [T][3][256] u8; a frame with identity[t] != 0 ([T] u8) is copied as it is and
 * its tables are not read.  Never in place: out == frames -> -1.  The rest as vve_mean_plane. */
int vve_apply(const uint8_t* frames, const uint8_t* fwd, const uint8_t* identity, int T, int H, int W, uint8_t* out, void* stream);

/* out of rule 6: orig = f, filled = f'', dil = d, dil2 = d2, back [T][3][256] u8 = B.  A fresh buffer: out == orig or out == filled -> -1.  The
 * rest as vve_mean_plane. */
int vve_restore(const uint8_t* orig, const uint8_t* filled, const uint8_t* dil, const uint8_t* dil2, const uint8_t* back, int T, int H, int W,
                uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
