/* vvmask.h -- C ABI of the mask clean-up entry points of libvvhip.so (videovanish_amd/csrc/vv_mask.hip; Python binding:
 * videovanish_amd/mask_hip.py; rules: DESIGN.md section 12).
 *
 * Conventions are those of vvhip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void* (NULL = the null stream), the
 * return value is 0 = launched or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing launched), and vvm_last_error()
 * gives the message of the calling thread's last failure (the string vv_last_error() of vvhip.h returns).  Every accumulation is an integer
 * add and every label a minimum, so each result is independent of the order of threads and blocks and equals a host restatement bit for bit.
 */
#ifndef VVMASK_H
#define VVMASK_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVM_ABI_VERSION 1
#define VVM_MAX_BRIDGE 16
#define VVM_MAX_GROW 8
#define VVM_MAX_T 65535

int vvm_abi_version(void);
const char* vvm_last_error(void);

/* 8-connected components of mask2d [S][H][W] u8 != 0, frame by frame.  labels [S][H][W] int32: the smallest linear index y * W + x of the
 * pixel's component within its frame, -1 where the mask byte is zero.  S >= 1, H * W < 2^31; anything else -> -1 before any device work. */
int vvm_label_components(const uint8_t* mask2d, int S, int H, int W, int32_t* labels, void* stream);

/* Despeckle: the components of dil [S][H][W] u8 (as vvm_label_components labels them, into labels_ws), each weighed by the number of pixels of
 * raw [S][H][W][ch] u8 inside it that are non-zero in any channel (into weight_ws, at the component's label); out = dil where the component's
 * weight is >= min_area, else 0.  min_area <= 1 clears nothing.  counts [S][2] int64, cleared first: (components removed, pixels of dil cleared)
 * per frame.  labels_ws, weight_ws: int32 [S][H][W] each, contents undefined on entry.  S >= 1, ch >= 1, H * W < 2^31, else -1. */
int vvm_despeckle(const uint8_t* dil, const uint8_t* raw, int S, int H, int W, int ch, int min_area, int32_t* labels_ws, int32_t* weight_ws,
                  uint8_t* out, int64_t* counts, void* stream);

/* Per pixel along the T frames of in [T][H][W] u8 (one segment: nothing outside [0, T) is read, the outside counts as zero): first every run of
 * at most `bridge` zero frames with a non-zero frame on both sides is filled (a closing with a flat element of bridge + 1 frames), then
 * out[t] = OR of the filled frames t - grow .. t + grow.  out [T][H][W] u8: 255 where set, else 0.  counts [T][2] int64, cleared first: (pixels
 * filled by the bridge, pixels added by the grow) in frame t.  T < 1, bridge < 0, grow < 0 -> -1; bridge > 16, grow > 8, T > 65535 -> -2. */
int vvm_time_bridge_grow(const uint8_t* in, int T, int H, int W, int bridge, int grow, uint8_t* out, int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
