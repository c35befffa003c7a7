/* vvgrain.h -- C ABI of the seam grain matching entry points of libvvhip.so (videovanish_amd/csrc/vv_grain.hip; Python binding:
 * videovanish_amd/grain_hip.py; rules: DESIGN.md section 14).
 *
 * Conventions are those of vvhip.h and vvtone.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void* (NULL = the null
 * stream), the return value is 0 = launched or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing launched), and
 * vvg_last_error() gives the message of the calling thread's last failure (the string vv_last_error() of vvhip.h returns).  Both functions see
 * a window as vvt_ring_stats does: frame t's window is [oy, oy + h) x [ox, ox + w) of the H0 x W0 frame, (oy, ox) = offsets[t]; its pixel is
 * the model's Hm x Wm output resized to h x w (cv2's fixed-point INTER_LINEAR; the bytes as they are when Hm x Wm is h x w) and then sent
 * through lut [T][3][256] u8 (x_c = lut[t][c][resized_c]; the identity table when there is no tone matching).  The full frame is the window
 * (0, 0, H0, W0).  Every accumulation is an integer add, so the sums do not depend on the order of threads and blocks and equal a host
 * restatement bit for bit; the noise is a pure function of its key, so the composite does too.
 */
#ifndef VVGRAIN_H
#define VVGRAIN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVG_ABI_VERSION 1
#define VVG_MAX_RING 32
#define VVG_BANDS 4
#define VVG_NSUM 36

int vvg_abi_version(void);
const char* vvg_last_error(void);

/* The grain statistic of the ring.  patch [T][Hm][Wm][3] u8, orig [T][H0][W0][3] u8, mask2d [T][H0][W0] u8, offsets [T][2] int32, lut
 * [T][3][256] u8.  With x = the window's pixel after lut and y = orig, pixel p of frame t counts for channel c when (a) p belongs to the ring
 * as vvtone.h defines it (inside the window and the frame, mask2d[t][p] == 0, a mask pixel of the frame within `ring` pixels, a box), (b) all
 * nine pixels of p's 3 x 3 neighbourhood lie inside the window and the frame and are unmasked, and (c) max - min of x_c over that neighbourhood
 * is <= flat.  L(I) = the sum over the neighbourhood of K .* I with K = [[1,-2,1],[-2,4,-2],[1,-2,1]] (zero on planes, variance 36 sigma^2 on
 * white noise of variance sigma^2); the band is b = x_c(p) >> 6.  sums [T][3][VVG_BANDS][3] int64 (VVG_NSUM per frame), cleared first, gets
 * sums[t][c][b][0] += 1, [1] += L(x_c)^2, [2] += L(y_c)^2.  Null pointer, a size <= 0, h > H0, w > W0 -> -1; ring outside 1 .. VVG_MAX_RING,
 * flat outside 0 .. 255, or more than 2^31 - 1 tiles of 64 x 32 pixels -> -2. */
int vvg_ring_grain_stats(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets, const uint8_t* lut,
                         int T, int H0, int W0, int h, int w, int ring, int flat, int64_t* sums, void* stream);

/* vvt_paste_lut_composite with one more step: inside the window, after the table and before the feather, channel c of the pixel p at frame
 * coordinates (X, Y) of frame t becomes clip(p_c + d_c, 0, 255).  amp [T][3][256] u8 is the noise amplitude in 1/16 levels for every value,
 * frame_ids [T] int32 the frames' indices in the caller's clip, seed 0 .. 2^31 - 1, mode 0 = "luma" (one noise value per pixel), 1 = "rgb"
 * (one per channel).  The noise is stateless and keyed on FRAME coordinates, so the full frame and any window give a pixel the same value
 * (all arithmetic on key and z modulo 2^64):
 *   key = ((uint64)seed << 32) ^ (((uint64)frame_ids[t] * H0 + Y) * W0 + X);  mode 1: key = key * 3 + c
 *   z = key + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31
 *   s = (the sum of the eight bytes of z) - 1020          an Irwin-Hall variable, standard deviation 209.02
 *   d_c = (amp[t][c][p_c] * s * 5017 + (1 << 23)) >> 24   an arithmetic shift; 5017 / 2^24 = 1 / (16 * 209.02); |product| < 2^31
 * out [T][H0][W0][3] u8, not orig.  feather_px < 0: the pixel is pasted as it is, and mask2d may be NULL.  With amp all zero the bytes are
 * vvt_paste_lut_composite's.  Null pointer, a size <= 0, h > H0, w > W0, seed < 0, mode outside {0, 1} -> -1; feather_px > 64 -> -2. */
int vvg_paste_grain_composite(const uint8_t* patch, int Hm, int Wm, const uint8_t* orig, const uint8_t* mask2d, const int* offsets, const uint8_t* lut,
                              const uint8_t* amp, const int* frame_ids, int seed, int mode, int T, int H0, int W0, int h, int w, float feather_px,
                              uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
