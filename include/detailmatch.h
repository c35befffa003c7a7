/* detailmatch.h -- C ABI of the seam detail matching entry points of libvvhip.so (videovanish_amd/csrc/vv_detail.hip; Python binding:
 * videovanish_amd/detailmatch_bind.py; settings and fit: videovanish_amd/detailmatch.py; rules and reasons: DESIGN.md section 24).
 *
 * Conventions are those of vvhip.h, vvtone.h and vvgrain.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void*
 * (NULL = the null stream), the return value is 0 = launched or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing
 * launched and nothing cleared), and vvd_last_error() gives the message of the calling thread's last failure (the string vv_last_error() of
 * vvhip.h returns).  Frame t's window is [oy, oy + h) x [ox, ox + w) of the H0 x W0 frame, (oy, ox) = offsets[t]; its pixel x is the model's
 * Hm x Wm output resized to h x w (cv2's fixed-point INTER_LINEAR; the bytes as they are when Hm x Wm is h x w); y is orig, the running buffer,
 * which inside this window still holds the original's bytes.  The full frame is the window (0, 0, H0, W0).  All arithmetic is integer: the
 * sums do not depend on the order of threads and blocks, and sums and bytes equal a host restatement bit for bit.
 *
 * The rules.  B = [[1,2,1],[2,4,2],[1,2,1]] (a 3 x 3 binomial, sum 16) and H(I)(p) = 16 I(p) - sum over the 3 x 3 neighbourhood of B .* I: the
 * high-pass in 1/16 levels, zero on constants, |H| <= 16 * 255 * 12 / 16 = 3060 on bytes.
 *
 * 1. Statistic (vvd_ring_detail_stats).  Pixel p of frame t counts for channel c when
 *      (a) p belongs to the ring as vvtone.h defines it (inside the window and the frame, mask2d[t][p] == 0, a mask pixel of the frame within
 *          `ring` pixels, a box), ring 1 .. VVD_MAX_RING;
 *      (b) all 25 pixels of p's 5 x 5 neighbourhood lie inside the window and the frame and are unmasked;
 *      (c) max - min of x_c over p's 3 x 3 neighbourhood is >= edge (the structured part of the ring: the complement of vvgrain.h's flat part).
 *    With D = H(y_c)(p) - H(x_c)(p), |D| <= 6120, and K = H(H(x_c))(p), |K| <= 24 * 3060 = 73440 (H of the int plane H(x_c); the 5 x 5 of (b)
 *    is what it reads), sums [T][3][VVD_NQ] int64 (VVD_NSUM per frame) is cleared first and gets sums[t][c][0] += 1, [1] += D * K (signed),
 *    [2] += K * K, [3] += D * D.  K * K reaches 5.4e9 and does not fit 32 bits: every product is formed and added in 64 bits per pixel.  With
 *    h * w <= VVD_MAX_PIXELS = 2^24 every sum stays below 2^24 * 73440^2 < 2^57 < 2^63; a larger window is refused with -2.
 *
 * 2. Fit (videovanish_amd/detailmatch.py, Python integers).  Per frame, over the three channels and the frames within `smooth` of it inside
 *    the clip call: P = sum D K, Q = sum K K, n = (sum of the counts) // 3.  n < min_pixels or Q = 0: the amount is 0 ("unfit").  Otherwise
 *    a = (8192 P + Q) // (2 Q), a floor division: q8, the least-squares amount of H(y) ~ H(x) + a / 256 * H(H(x)) / 16 rounded half up; a is
 *    clamped to [-q(max_soften), q(max_sharpen)] with q(v) = floor(256 v + 1/2); |a| < q(dead): the amount is 0 ("dead"); then
 *    a = (a * q(strength) + 128) >> 8 (an arithmetic shift).  max_sharpen <= 4, max_soften <= 1 and strength <= 1, so |a| <= VVD_MAX_AMOUNT =
 *    1024 and the amount never exceeds the caps.
 *
 * 3. Apply (vvd_sharpen), for EVERY pixel p of the window and every channel, with lo_c, hi_c = min, max of x_c over p's 3 x 3 neighbourhood:
 *      out_c = clip(clamp((4096 x_c + a_t H(x_c)(p) + 2048) >> 12, lo_c - overshoot, hi_c + overshoot), 0, 255)
 *    (an arithmetic shift; a / 256 amounts of H / 16 levels: 4096 = 256 * 16).  A neighbour outside the window is the window's edge pixel
 *    (its coordinates clamped to the window).  a_t = amount[t] clamped to +-VVD_MAX_AMOUNT, so |4096 x + a H + 2048| < 2^23.  a_t = 0 gives the
 *    bytes of x: the resize alone.  The clamp is what keeps an unsharp mask from ringing at a strong edge: no byte leaves
 *    [lo - overshoot, hi + overshoot] of its own neighbourhood; with a < 0 and a >= -256 the value is a convex mix of x and its binomial mean
 *    and stays inside [lo, hi] by itself.
 */
#ifndef DETAILMATCH_H
#define DETAILMATCH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVD_ABI_VERSION 1
#define VVD_MAX_RING 32
#define VVD_MAX_EDGE 255
#define VVD_MAX_OVERSHOOT 255
#define VVD_MAX_AMOUNT 1024
#define VVD_MAX_PIXELS (1 << 24)
#define VVD_NQ 4
#define VVD_NSUM 12

int vvd_abi_version(void);
const char* vvd_last_error(void);

/* Rule 1.  patch [T][Hm][Wm][3] u8, orig [T][H0][W0][3] u8, mask2d [T][H0][W0] u8, offsets [T][2] int32, sums [T][3][VVD_NQ] int64.  Null
 * pointer, a size <= 0, h > H0, w > W0 -> -1; ring outside 1 .. VVD_MAX_RING, edge outside 0 .. VVD_MAX_EDGE, h * w > VVD_MAX_PIXELS, or more
 * than 2^31 - 1 tiles of 64 x 32 pixels -> -2. */
int vvd_ring_detail_stats(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets, int T, int H0, int W0,
                          int h, int w, int ring, int edge, int64_t* sums, void* stream);

/* Rule 3.  patch [T][Hm][Wm][3] u8, amount [T] int32 (q8), out [T][h][w][3] u8 in window coordinates, not patch; every byte of out is
 * written.  A frame with amount 0 is copied (resized when Hm x Wm is not h x w) without filter arithmetic.  Null pointer, a size <= 0, out ==
 * patch -> -1; overshoot outside 0 .. VVD_MAX_OVERSHOOT, h * w > VVD_MAX_PIXELS, or more than 2^31 - 1 tiles -> -2. */
int vvd_sharpen(const uint8_t* patch, int Hm, int Wm, const int* amount, int T, int h, int w, int overshoot, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
