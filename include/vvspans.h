/* vvspans.h -- C ABI of the mask-span entry points of libvvhip.so (videovanish_amd/csrc/vv_spans.hip; Python binding:
 * videovanish_amd/spans_hip.py; rules: DESIGN.md section 11).
 *
 * Conventions are those of vvhip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void* (NULL = the null stream), the
 * return value is 0 = launched or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing launched), and vvs_last_error()
 * gives the message of the calling thread's last failure (the string vv_last_error() of vvhip.h returns).
 */
#ifndef VVSPANS_H
#define VVSPANS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVS_ABI_VERSION 1
#define VVS_HIST_BINS 64

int vvs_abi_version(void);
const char* vvs_last_error(void);

/* Cut statistics of every adjacent frame pair (t - 1, t), t = 1 .. T - 1, of an RGB clip frames [T][H][W][3] u8, over the pixels that are zero in
 * BOTH frames' masks mask2d [T][H][W] u8 (mask2d == NULL: every pixel).  Integer luma Y = (77 R + 150 G + 29 B + 128) >> 8, bin Y >> 2.
 *   n_sad [T-1][2] int64: (number of pixels counted, sum over them of |Y_t - Y_{t-1}|)
 *   hist  [T-1][2][64] int32: luma histogram of frame t - 1 and of frame t over the same pixels
 * Both outputs are cleared first; every accumulation is an integer add, so the result does not depend on the order of the blocks and equals a
 * host restatement bit for bit.  T in [2, 65536], H * W < 2^31; anything else -> -1 before any device work. */
int vvs_frame_pair_stats(const uint8_t* frames, const uint8_t* mask2d, int T, int H, int W, int64_t* n_sad, int32_t* hist, void* stream);

#ifdef __cplusplus
}
#endif
#endif
