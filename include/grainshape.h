/* grainshape.h -- C ABI of the grain shape entry points of libvvhip.so (videovanish_amd/csrc/vv_grainshape.hip; Python binding:
 * videovanish_amd/grainshape_bind.py; host fit: videovanish_amd/grainshape.py; rules: DESIGN.md section 25).  The companion of seam grain
 * matching (vvgrain.h): that stage adds noise that is white at pixel scale, this one fits the grain's SIZE on the ring and adds shaped noise.
 *
 * Conventions are those of vvhip.h, vvgrain.h and vvblend.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void* (NULL
 * = the null stream), the return value is 0 = launched or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing
 * launched), and vvn_last_error() gives the message of the calling thread's last failure (the string vv_last_error() of vvhip.h returns).  A
 * window is seen as vvg_ring_grain_stats sees it: frame t's window is [oy, oy + h) x [ox, ox + w) of the H0 x W0 frame, (oy, ox) =
 * offsets[t]; its pixel x is the model's Hm x Wm output resized to h x w and then sent through lut [T][3][256] u8; y is orig.
 *
 * THE MODEL.  The added grain is white noise s (exactly vvgrain.h's stateless field) sent through the separable 3 x 3 kernel
 * [a_x, 1, a_x] (x) [a_y, 1, a_y], 0 <= a <= max_a <= 0.5: the family runs from white (a = 0) to the binomial blur (a = 0.5).  With k =
 * [1, -2, 1], the 1-D factor of Immerkaer's operator L of vvgrain.h, and unit white noise shaped by [a, 1, a] along one axis:
 *   P0(a) = 6 - 16 a + 14 a^2      the variance of the k-response
 *   P1(a) = -4 + 14 a - 12 a^2     its lag-1 covariance
 *   r0(a) = 1 + 2 a^2              the shaped noise's own variance
 *   rho(a) = P1 / P0               rises monotonically from -2/3 at a = 0 to 0 at a = 0.5 (and turns back beyond about 0.6: hence the cap)
 * In two dimensions L = k (x) k, the covariance of L's response at lag 1 along x is sigma^2 P1(a_x) P0(a_y) and its variance sigma^2 P0(a_x)
 * P0(a_y): the other axis cancels out of the lag-1 ratio, so each axis is fitted on its own.  The model's rendering x carries no grain but its
 * own structure, so the fit takes the differences y - x of the sums below: rho = 2 (C_y - C_x) / (D_y - D_x), sums [1] - [2] over [3] - [4].
 */
#ifndef GRAINSHAPE_H
#define GRAINSHAPE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVN_ABI_VERSION 1
#define VVN_MAX_RING 32
#define VVN_MAX_TAP 128
#define VVN_NSUM 30

int vvn_abi_version(void);
const char* vvn_last_error(void);

/* The shape statistic of the ring: vvg_ring_grain_stats' arguments.  A pixel "counts for channel c" exactly as rules (a), (b), (c) of
 * vvgrain.h say, with the same ring and flat.  Axis 0 pairs p with q = p + (1, 0) (the right neighbour), axis 1 with q = p + (0, 1) (the lower
 * one); a pair is counted when BOTH p and q count for c (so a pair whose q leaves the window or the frame is not counted).  sums
 * [T][3][2][5] int64 (VVN_NSUM per frame: channel, axis, entry), cleared first, gets per counted pair
 *   [0] += 1    [1] += L(x_c)(p) L(x_c)(q)    [2] += L(y_c)(p) L(y_c)(q)    [3] += L(x_c)(p)^2 + L(x_c)(q)^2    [4] += L(y_c)(p)^2 + L(y_c)(q)^2
 * The products are signed; every accumulation is an integer add, so the sums are exact, do not depend on the order of threads and blocks and
 * equal a host restatement bit for bit.  The rule does not know the implementation's tiles.  Null pointer, a size <= 0, h > H0, w > W0 -> -1;
 * ring outside 1 .. VVN_MAX_RING, flat outside 0 .. 255, or more than 2^31 - 1 tiles -> -2. */
int vvn_ring_shape_stats(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets, const uint8_t* lut,
                         int T, int H0, int W0, int h, int w, int ring, int flat, int64_t* sums, void* stream);

/* vvb_paste_blend_composite's arguments with two differences: field may be NULL (no membrane step), and taps [T][3][2] int32 gives aq =
 * rint(256 a) per frame, channel and axis (0 = x, 1 = y), 0 .. VVN_MAX_TAP.  Inside the window, in integers:
 *   s(X, Y[, c])   vvgrain.h's centred byte sum at FRAME coordinates; the key arithmetic is on signed X, Y widened to 64 bits and taken
 *                  modulo 2^64, so the taps at X = -1, X = W0, Y = -1 and Y = H0 are still a pure function of the key, and the full frame and
 *                  any window give a pixel the same value
 *   u_c = (sum_j wy_j sum_i wx_i s(X + i, Y + j) + 2^15) >> 16,   w = [aq, 256, aq], i, j = -1, 0, 1;   |sum| <= 512^2 * 1020 < 2^31
 *   d_c = (amp[t][c][lut(p_c)] * u_c * 5017 + 2^23) >> 24         a 64-BIT product, an arithmetic shift
 * in the order of vvb_paste_blend_composite: table, membrane (if field), grain looked up at the tabled value, clip, feather.  amp is the
 * WHITE amplitude in front of the shaping kernel (the shaped noise's sigma is amp / 16 * sqrt(r0(a_x) r0(a_y))).  With taps all zero u_c = s:
 * field NULL gives vvg_paste_grain_composite's bytes, a field vvb_paste_blend_composite's, amp all zero as well vvt_paste_lut_composite's.
 * Refusals are those of the two pastes (null pointer but field and, for feather_px < 0, mask2d; a size <= 0; h > H0; w > W0; seed < 0; mode
 * outside {0, 1} -> -1; feather_px > 64, strength_q8 outside 0 .. 512 -> -2), and a tap outside 0 .. VVN_MAX_TAP -> -2: the taps are copied
 * to the host and checked before the launch (24 T bytes; the one synchronisation of `stream`). */
int vvn_paste_shaped_composite(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets,
                               const uint8_t* lut, const int16_t* field, int strength_q8, const uint8_t* amp, const int* taps, const int* frame_ids,
                               int seed, int mode, int T, int H0, int W0, int h, int w, float feather_px, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
