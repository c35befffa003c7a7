/* vvflickalign.h -- C ABI of the aligned inpaint deflicker entry points of libvvhip.so (videovanish_amd/csrc/vv_flicker.hip; Python binding:
 * videovanish_amd/flickalign_hip.py; settings: videovanish_amd/deflickeralign.py; host restatement: tests/deflickeralign_ref.py; DESIGN.md
 * section 19).
 *
 * Conventions are those of vvhip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void* (NULL = the null stream), the
 * return value is 0 = launched or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing launched), and vvc_last_error()
 * gives the message of the calling thread's last failure (the string vv_last_error() of vvhip.h returns).  Nothing here reads the environment.
 *
 * The rule (it is the ABI) is vvflicker.h's sigma filter along time, read along a tracked camera translation: under a pan the background moves
 * through a fixed frame place, so the neighbours are taken where the same piece of background sits in the neighbour frame.  Everything of
 * vvflicker.h holds (the window of frame t, x_t(p), rules 3 and 4, the limits), with these changes.  track [T][8] int32 is vvalign.h's record
 * (dx, dy, key, tracked, sad_lo, sad_hi, n, level); off[t] = (track[t][0], track[t][1]) = (x, y): the content of frame t at (x, y) sits on the
 * canvas at (x + off[t].x, y + off[t].y).  Frame t is TRACKED when track[t][3] == 1.  Only these three ints of a record are read.
 *   2'. Samples.  For frame t and frame pixel p the candidates are the frames s with |s - t| <= radius, 0 <= s < T, s != t, with BOTH t and s
 *       tracked.  A candidate's place q = p + off[t] - off[s] (x with x, y with y) must lie inside frame s's window.  s is accepted when
 *       |x_s(q)_c - x_t(p)_c| <= tol for all three channels c.  s = t is always accepted, so n >= 1.
 *       In window coordinates: with e_t = offsets[t] + (off[t].y, off[t].x), the window's place on the canvas, the pixel (yy, xx) of frame t's
 *       window reads frame s's window at (yy, xx) + e_t - e_s; e_t - e_s is taken in 64 bits, so the rule holds for every int32 content of
 *       `offsets` and `track`.  With every frame tracked this is vvflicker.h's rule 2 with the windows placed at e_t.
 *   LOST FRAMES.  A frame that is not tracked takes no sample and gives none: its pixels come back as they are, with n = 1.
 *   5'. Sums [T][12] int64 as vvflicker.h's rule 5; the mask byte is still read at p in frame t: mask2d[t][offsets[t] + (yy, xx)].
 * |out_c - x_t(p)_c| <= tol still holds by construction: the failure mode stays "not smoothed", never "ghosted".  An all-zero, all-tracked
 * track gives vvf_hold's bytes and sums.  Nothing crosses the ends of the clip call.
 */
#ifndef VVFLICKALIGN_H
#define VVFLICKALIGN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVC_ABI_VERSION 1
#define VVC_MAX_RADIUS 4
#define VVC_MAX_T 65535
#define VVC_TRACK_INTS 8

int vvc_abi_version(void);
const char* vvc_last_error(void);

/* win [T][h][w][3] u8, offsets [T][2] int32 (oy, ox), track [T][8] int32, mask2d [T][H0][W0] u8, out [T][h][w][3] u8 (not win), sums [T][12]
 * int64.  One thread per output pixel, as vvf_hold's gather form; the neighbours' places are worked out once per block.  Reads of win are
 * bounds-checked against the window of the frame they come from and reads of the mask against the frame, whatever offsets and track hold.
 * Every byte of out and of sums is written, nothing else.  Null pointer, a size <= 0, h > H0, w > W0, radius < 0, tol < 0, out == win -> -1;
 * radius > VVC_MAX_RADIUS, tol > 255, T > VVC_MAX_T, h * w >= 2^31 -> -2. */
int vvc_hold(const uint8_t* win, const int* offsets, const int32_t* track, const uint8_t* mask2d, int T, int H0, int W0, int h, int w, int radius,
             int tol, uint8_t* out, int64_t* sums, void* stream);

#ifdef __cplusplus
}
#endif
#endif
