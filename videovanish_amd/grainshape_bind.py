"""ctypes binding of the grain shape entry points of libvvhip.so (include/grainshape.h; kernels: csrc/vv_grainshape.hip).

Built on hip.py: PART (a hip.Part) declares grainshape.h's part of the library once, SIGNATURES is applied when the library is first used through
this module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_grainshape_cpu.py checks the table against the
header (tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
MAX_RING, MAX_TAP, NSUM = 32, 128, 30

# every function of include/grainshape.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvn_abi_version": (I, ()),
    "vvn_last_error": (C.c_char_p, ()),
    "vvn_ring_shape_stats": (I, (P, I, I, P, P, P, P, I, I, I, I, I, I, I, P, P)),
    "vvn_paste_shaped_composite": (I, (P, I, I, P, P, P, P, P, I, P, P, P, I, I, I, I, I, I, I, C.c_float, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("grainshape.h", "vvn_", ABI_VERSION, "grain shape", SIGNATURES)
lib, _check = PART.lib, PART.check


def ring_shape_stats(patch, orig, mask2d, offsets, lut, h, w, ring, flat):
    """grain_hip.ring_grain_stats' arguments -> sums [T,30] int64 on the device (vvn_ring_shape_stats), [T][channel][axis][pairs, Cx, Cy, Dx,
    Dy]: over the pairs of horizontally (axis 0) and vertically (axis 1) adjacent pixels that both count for the channel as ring_grain_stats
    counts them, the signed products L(p) L(q) and the squares L(p)^2 + L(q)^2 of Immerkaer's operator on x = patch resized to the window and
    sent through lut, and on y = orig."""
    if mask2d is None:
        raise RuntimeError("ring_shape_stats: the ring needs mask2d")
    hip._need_cuda(lut)
    T, Hm, Wm, H0, W0 = hip._need_window("ring_shape_stats", patch, orig, mask2d, offsets)
    hip._need_table("ring_shape_stats", "lut", lut, T)
    sums = torch.empty((T, NSUM), dtype=torch.int64, device=orig.device)
    with hip._Prof("grainshape_ring_stats", 0.0, T * int(h) * int(w) + sums.numel() * 8):
        _check(lib().vvn_ring_shape_stats(hip._p(patch), Hm, Wm, hip._p(orig), hip._p(mask2d), hip._p(offsets), hip._p(lut), T, H0, W0, int(h), int(w),
                                          int(ring), int(flat), hip._p(sums), hip._stream()), "vvn_ring_shape_stats")
    return sums


def paste_shaped_composite(patch, orig, mask2d, offsets, lut, field, strength_q8, amp, taps, frame_ids, seed, mode, h, w, feather_px, out=None):
    """blend_hip.paste_blend_composite with shaped noise: the stateless field of include/vvgrain.h goes through [aq, 256, aq] / 256 along x and
    along y (taps [T,3,2] int32, aq = rint(256 a) per frame, channel and axis, 0 .. 128) before amp scales it.  field None: no membrane step
    (grain_hip.paste_grain_composite's order).  Zero taps give the bytes of those two calls."""
    hip._need_cuda(lut, field, amp, taps, frame_ids, out)
    T, Hm, Wm, H0, W0 = hip._need_window("paste_shaped_composite", patch, orig, mask2d, offsets)
    hip._need_table("paste_shaped_composite", "lut", lut, T)
    hip._need_table("paste_shaped_composite", "amp", amp, T)
    if field is not None and (field.dtype != torch.int16 or tuple(field.shape) != (T, int(h), int(w), 3)):
        raise RuntimeError("paste_shaped_composite: field must be a [T, h, w, 3] int16 tensor")
    if taps.dtype != torch.int32 or tuple(taps.shape) != (T, 3, 2):
        raise RuntimeError("paste_shaped_composite: taps must be a [T, 3, 2] int32 tensor")
    if frame_ids.dtype != torch.int32 or tuple(frame_ids.shape) != (T,):
        raise RuntimeError("paste_shaped_composite: frame_ids must be a [T] int32 tensor")
    out = hip._out_like("paste_shaped_composite", out, orig, "orig")
    with hip._Prof("grainshape_paste_composite", 0.0, T * H0 * W0 * (3 + 1 + 3) + patch.numel() + (0 if field is None else field.numel() * 2)):
        _check(lib().vvn_paste_shaped_composite(hip._p(patch), Hm, Wm, hip._p(orig), hip._p(mask2d), hip._p(offsets), hip._p(lut), hip._p(field),
                                                int(strength_q8), hip._p(amp), hip._p(taps), hip._p(frame_ids), int(seed), int(mode), T, H0, W0, int(h),
                                                int(w), float(feather_px), hip._p(out), hip._stream()), "vvn_paste_shaped_composite")
    return out
