"""ctypes binding of the seam grain matching entry points of libvvhip.so (include/vvgrain.h; kernels: csrc/vv_grain.hip).

Built on hip.py: PART (a hip.Part) declares vvgrain.h's part of the library once, SIGNATURES is applied when the library is first used through this
module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_grainmatch_cpu.py checks the table against the header
(tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
MAX_RING = 32
BANDS = 4
NSUM = 36

# every function of include/vvgrain.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvg_abi_version": (I, ()),
    "vvg_last_error": (C.c_char_p, ()),
    "vvg_ring_grain_stats": (I, (P, I, I, P, P, P, P, I, I, I, I, I, I, I, P, P)),
    "vvg_paste_grain_composite": (I, (P, I, I, P, P, P, P, P, P, I, I, I, I, I, I, I, C.c_float, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("vvgrain.h", "vvg_", ABI_VERSION, "grain matching", SIGNATURES)
lib, _check = PART.lib, PART.check


def ring_grain_stats(patch, orig, mask2d, offsets, lut, h, w, ring, flat):
    """patch [T,Hm,Wm,3] u8 (model output of the window), orig [T,H0,W0,3] u8, mask2d [T,H0,W0] u8, offsets [T,2] int32 (oy, ox), lut [T,3,256]
    u8, on the device -> sums [T,36] int64 on the device (vvg_ring_grain_stats), [T][channel][band][n, Sx, Sy]: over the ring pixels of frame
    t's h x w window whose 3 x 3 neighbourhood is unmasked, inside the window and spans at most `flat` levels of x_c, with x = patch resized to
    the window and sent through lut and y = orig: the count and the squared responses of Immerkaer's operator on x_c and y_c, by x_c >> 6."""
    if mask2d is None:
        raise RuntimeError("ring_grain_stats: the ring needs mask2d")
    hip._need_cuda(lut)
    T, Hm, Wm, H0, W0 = hip._need_window("ring_grain_stats", patch, orig, mask2d, offsets)
    hip._need_table("ring_grain_stats", "lut", lut, T)
    sums = torch.empty((T, NSUM), dtype=torch.int64, device=orig.device)
    with hip._Prof("grain_ring_stats", 0.0, T * int(h) * int(w) + sums.numel() * 8):
        _check(lib().vvg_ring_grain_stats(hip._p(patch), Hm, Wm, hip._p(orig), hip._p(mask2d), hip._p(offsets), hip._p(lut), T, H0, W0, int(h), int(w),
                                          int(ring), int(flat), hip._p(sums), hip._stream()), "vvg_ring_grain_stats")
    return sums


def paste_grain_composite(patch, orig, mask2d, offsets, lut, amp, frame_ids, seed, mode, h, w, feather_px, out=None):
    """tone_hip.paste_lut_composite with grain: after lut [T,3,256] u8 and before the feathered composite, channel c of a pixel of the window
    gets the stateless noise of include/vvgrain.h at the amplitude amp[t, c, value] (u8, 1/16 levels), keyed on seed, frame_ids[t] (int32 [T])
    and the pixel's FRAME coordinates; mode 0 = one value per pixel ("luma"), 1 = one per channel ("rgb").  feather_px < 0: plain paste (mask2d
    may be None).  out: an optional [T,H0,W0,3] u8 buffer to write (not orig)."""
    hip._need_cuda(lut, amp, frame_ids, out)
    T, Hm, Wm, H0, W0 = hip._need_window("paste_grain_composite", patch, orig, mask2d, offsets)
    hip._need_table("paste_grain_composite", "lut", lut, T)
    hip._need_table("paste_grain_composite", "amp", amp, T)
    if frame_ids.dtype != torch.int32 or tuple(frame_ids.shape) != (T,):
        raise RuntimeError("paste_grain_composite: frame_ids must be a [T] int32 tensor")
    out = hip._out_like("paste_grain_composite", out, orig, "orig")
    with hip._Prof("grain_paste_composite", 0.0, T * H0 * W0 * (3 + 1 + 3) + patch.numel()):
        _check(lib().vvg_paste_grain_composite(hip._p(patch), Hm, Wm, hip._p(orig), hip._p(mask2d), hip._p(offsets), hip._p(lut), hip._p(amp),
                                               hip._p(frame_ids), int(seed), int(mode), T, H0, W0, int(h), int(w), float(feather_px), hip._p(out),
                                               hip._stream()), "vvg_paste_grain_composite")
    return out
