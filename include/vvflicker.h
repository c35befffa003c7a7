/* vvflicker.h -- C ABI of the inpaint deflicker entry points of libvvhip.so (videovanish_amd/csrc/vv_flicker.hip; Python binding:
 * videovanish_amd/flicker_hip.py; settings: videovanish_amd/deflicker.py; host restatement: tests/deflicker_ref.py).
 *
 * Conventions are those of vvhip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void* (NULL = the null stream), the
 * return value is 0 = launched or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing launched), and vvf_last_error()
 * gives the message of the calling thread's last failure (the string vv_last_error() of vvhip.h returns).  Nothing here reads the environment.
 *
 * The rule (it is the ABI) is Lee's sigma filter along time: a pixel of the model's output becomes the rounded mean of those temporal
 * neighbours that lie within `tol` levels of it.  A clip call covers the frames 0 .. T - 1; a window has the size h x w and frame t's window
 * is [oy_t, oy_t + h) x [ox_t, ox_t + w) of the H0 x W0 frame, (oy_t, ox_t) = offsets[t], as vv_roi_paste_composite sees it.  The full
 * frame is the window (0, 0, H0, W0).
 *   1. Window pixel.  x_t(p) is the window's pixel at frame coordinate p: the model's Hm x Wm output resized to h x w (cv2's fixed-point
 *      INTER_LINEAR, vv_resize_bilinear_u8's arithmetic; the bytes as they are when Hm x Wm is h x w).  It is defined when p lies inside
 *      frame t's window.  vvf_window_pixels materialises it: win[t][yy][xx] = x_t((oy_t + yy, ox_t + xx)).
 *   2. Samples.  For frame t and pixel p the candidates are the frames s with |s - t| <= radius and 0 <= s < T whose window contains p.
 *      s is accepted when |x_s(p)_c - x_t(p)_c| <= tol for all three channels c (jointly: nothing fringes in colour).  s = t is always
 *      accepted, so the number of accepted samples n is >= 1 (and <= 2 radius + 1 <= 9).
 *   3. Output.  Per channel out_c = (2 S_c + n) / (2 n) in integer division, S_c = the sum of x_s(p)_c over the accepted samples: the mean,
 *      rounded half up.  |out_c - x_t(p)_c| <= tol by construction.  radius = 0 or tol = 0 gives x_t(p).
 *   4. Result.  out [T][h][w][3] u8 in window coordinates: out[t][yy][xx] belongs to p = (oy_t + yy, ox_t + xx).
 *   5. Sums [T][12] int64, cleared first, per frame t over the h * w pixels of its window: [0] the pixels, [1] the pixels with any byte
 *      changed, [2] the sum of n, [3..5] the sum of |out_c - x_c|; [6..11] the same four quantities over the pixels with mask2d[t][p] != 0
 *      (a window pixel outside the H0 x W0 frame has no mask byte and counts as unmasked).  Integer adds only: the sums do not depend on the
 *      order of threads and blocks.
 * Nothing crosses the ends of the clip call.
 */
#ifndef VVFLICKER_H
#define VVFLICKER_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVF_ABI_VERSION 1
#define VVF_MAX_RADIUS 4
#define VVF_MAX_T 65535
#define VVF_SLAB 16   /* frames per block of the fixed form: the grid's z axis splits T into slabs of this many frames */

int vvf_abi_version(void);
const char* vvf_last_error(void);

/* Rule 1.  patch [T][Hm][Wm][3] u8 (the model's output of the window) -> win [T][h][w][3] u8.  Null pointer, a size <= 0 -> -1; T > VVF_MAX_T,
 * or h * w or Hm * Wm >= 2^31 -> -2. */
int vvf_window_pixels(const uint8_t* patch, int T, int Hm, int Wm, int h, int w, uint8_t* win, void* stream);

/* Rules 2 - 5.  win [T][h][w][3] u8, offsets [T][2] int32 (oy, ox), mask2d [T][H0][W0] u8, out [T][h][w][3] u8 (not win), sums [T][12] int64.
 * fixed != 0: the caller states that offsets[t] == offsets[0] for every t; then, with w % 4 == 0 and win / out aligned to 4 bytes, the fixed
 * form runs (a thread owns 4 adjacent pixels and walks the frames of a slab of VVF_SLAB frames with the last 2 radius + 1 frames in
 * registers: every input byte is read once per slab), else the gather form (one thread per output pixel).  Both give the bytes of the
 * rule.  Every byte of out and of sums is written, nothing else.  Null pointer, a size <= 0, h > H0, w > W0, radius < 0, tol < 0, out == win
 * -> -1; radius > VVF_MAX_RADIUS, tol > 255, T > VVF_MAX_T, h * w >= 2^31 -> -2. */
int vvf_hold(const uint8_t* win, const int* offsets, const uint8_t* mask2d, int T, int H0, int W0, int h, int w, int radius, int tol, int fixed,
             uint8_t* out, int64_t* sums, void* stream);

#ifdef __cplusplus
}
#endif
#endif
