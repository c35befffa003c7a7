/* vvtone.h -- C ABI of the seam tone matching entry points of libvvhip.so (videovanish_amd/csrc/vv_tone.hip; Python binding:
 * videovanish_amd/tone_hip.py; rules: DESIGN.md section 13).
 *
 * Conventions are those of vvhip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void* (NULL = the null stream), the
 * return value is 0 = launched or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing launched), and vvt_last_error()
 * gives the message of the calling thread's last failure (the string vv_last_error() of vvhip.h returns).  Both functions see a window as
 * vv_roi_paste_composite does: frame t's window is [oy, oy + h) x [ox, ox + w) of the H0 x W0 frame, (oy, ox) = offsets[t]; its pixel is the
 * model's Hm x Wm output resized to h x w (cv2's fixed-point INTER_LINEAR; the bytes as they are when Hm x Wm is h x w).  The full frame is
 * the window (0, 0, H0, W0).  Every accumulation is an integer add, so the sums do not depend on the order of threads and blocks and equal a
 * host restatement bit for bit.
 */
#ifndef VVTONE_H
#define VVTONE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVT_ABI_VERSION 1
#define VVT_MAX_RING 32

int vvt_abi_version(void);
const char* vvt_last_error(void);

/* The ring statistic.  patch [T][Hm][Wm][3] u8, orig [T][H0][W0][3] u8, mask2d [T][H0][W0] u8, offsets [T][2] int32.  A pixel p of frame t
 * belongs to the ring when it lies inside the window (and the frame), mask2d[t][p] == 0 and some pixel q of the frame with |qx - px| <= ring,
 * |qy - py| <= ring has mask2d[t][q] != 0 (q may lie outside the window, not outside the frame).  With x = the window's pixel at p and
 * y = orig[t][p], sums [T][16] int64, cleared first, gets per frame: [0] n, [1..3] sum x_c, [4..6] sum y_c, [7..9] sum x_c^2,
 * [10..12] sum x_c * y_c, [13..15] sum y_c^2.  Null pointer, a size <= 0, h > H0, w > W0 -> -1; ring outside 1 .. VVT_MAX_RING, or more than
 * 2^31 - 1 tiles of 64 x 32 pixels -> -2. */
int vvt_ring_stats(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets, int T, int H0, int W0, int h,
                   int w, int ring, int64_t* sums, void* stream);

/* vv_roi_paste_composite with one more step: inside the window each of the pixel's three bytes goes through lut [T][3][256] u8
 * (out_c = lut[t][c][in_c]) before it is feathered against orig with mask2d; outside the window the bytes of orig.  out [T][H0][W0][3] u8, not
 * orig.  feather_px < 0: the looked-up pixel is pasted as it is, and mask2d may be NULL.  With lut[t][c][v] == v the bytes are
 * vv_roi_paste_composite's.  Null pointer, a size <= 0, h > H0, w > W0 -> -1; feather_px > 64 -> -2. */
int vvt_paste_lut_composite(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets, const uint8_t* lut,
                            int T, int H0, int W0, int h, int w, float feather_px, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
