"""ctypes binding of the seam tone matching entry points of libvvhip.so (include/vvtone.h; kernels: csrc/vv_tone.hip).

Built on hip.py: PART (a hip.Part) declares vvtone.h's part of the library once, SIGNATURES is applied when the library is first used through this
module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_tonematch_cpu.py checks the table against the header
(tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
MAX_RING = 32

# every function of include/vvtone.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvt_abi_version": (I, ()),
    "vvt_last_error": (C.c_char_p, ()),
    "vvt_ring_stats": (I, (P, I, I, P, P, P, I, I, I, I, I, I, P, P)),
    "vvt_paste_lut_composite": (I, (P, I, I, P, P, P, P, I, I, I, I, I, C.c_float, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("vvtone.h", "vvt_", ABI_VERSION, "tone matching", SIGNATURES)
lib, _check = PART.lib, PART.check


def ring_stats(patch, orig, mask2d, offsets, h, w, ring):
    """patch [T,Hm,Wm,3] u8 (model output of the window), orig [T,H0,W0,3] u8, mask2d [T,H0,W0] u8, offsets [T,2] int32 (oy, ox), on the device
    -> sums [T,16] int64 on the device (vvt_ring_stats): over the unmasked pixels of frame t's h x w window that have a mask pixel within `ring`
    pixels (a box), with x = patch resized to the window and y = orig: n, sum x_c, sum y_c, sum x_c^2, sum x_c y_c, sum y_c^2."""
    if mask2d is None:
        raise RuntimeError("ring_stats: the ring needs mask2d")
    T, Hm, Wm, H0, W0 = hip._need_window("ring_stats", patch, orig, mask2d, offsets)
    sums = torch.empty((T, 16), dtype=torch.int64, device=orig.device)
    with hip._Prof("tone_ring_stats", 0.0, T * int(h) * int(w) + sums.numel() * 8):
        _check(lib().vvt_ring_stats(hip._p(patch), Hm, Wm, hip._p(orig), hip._p(mask2d), hip._p(offsets), T, H0, W0, int(h), int(w), int(ring),
                                    hip._p(sums), hip._stream()), "vvt_ring_stats")
    return sums


def paste_lut_composite(patch, orig, mask2d, offsets, lut, h, w, feather_px, out=None):
    """hip.roi_paste_composite with the window's bytes sent through lut [T,3,256] u8 (out_c = lut[t, c, in_c]) before the feathered composite
    (vvt_paste_lut_composite).  feather_px < 0: plain paste (mask2d may be None).  out: an optional [T,H0,W0,3] u8 buffer to write (not orig)."""
    hip._need_cuda(lut, out)
    T, Hm, Wm, H0, W0 = hip._need_window("paste_lut_composite", patch, orig, mask2d, offsets)
    hip._need_table("paste_lut_composite", "lut", lut, T)
    out = hip._out_like("paste_lut_composite", out, orig, "orig")
    with hip._Prof("tone_paste_lut_composite", 0.0, T * H0 * W0 * (3 + 1 + 3) + patch.numel()):
        _check(lib().vvt_paste_lut_composite(hip._p(patch), Hm, Wm, hip._p(orig), hip._p(mask2d), hip._p(offsets), hip._p(lut), T, H0, W0, int(h), int(w),
                                             float(feather_px), hip._p(out), hip._stream()), "vvt_paste_lut_composite")
    return out
