"""ctypes binding of the seam detail matching entry points of libvvhip.so (include/detailmatch.h; kernels: csrc/vv_detail.hip).

Built on hip.py: PART (a hip.Part) declares detailmatch.h's part of the library once, SIGNATURES is applied when the library is first used through
this module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_detailmatch_cpu.py checks the table against the
header (tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
MAX_RING, MAX_EDGE, MAX_OVERSHOOT, MAX_AMOUNT, MAX_PIXELS = 32, 255, 255, 1024, 1 << 24
NQ, NSUM = 4, 12

# every function of include/detailmatch.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvd_abi_version": (I, ()),
    "vvd_last_error": (C.c_char_p, ()),
    "vvd_ring_detail_stats": (I, (P, I, I, P, P, P, I, I, I, I, I, I, I, P, P)),
    "vvd_sharpen": (I, (P, I, I, P, I, I, I, I, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("detailmatch.h", "vvd_", ABI_VERSION, "detail matching", SIGNATURES)
lib, _check = PART.lib, PART.check


def ring_detail_stats(patch, orig, mask2d, offsets, h, w, ring, edge):
    """patch [T,Hm,Wm,3] u8 (model output of the window), orig [T,H0,W0,3] u8, mask2d [T,H0,W0] u8, offsets [T,2] int32 (oy, ox), on the device
    -> sums [T,12] int64 on the device (vvd_ring_detail_stats), [T][channel][n, sum D K, sum K K, sum D D]: over the ring pixels of frame t's
    h x w window whose 5 x 5 neighbourhood is unmasked and inside the window and the frame and whose 3 x 3 neighbourhood spans at least `edge`
    levels of x_c, with x = patch resized to the window, y = orig, H the 3 x 3 binomial high-pass in 1/16 levels, D = H(y) - H(x), K = H(H(x))."""
    if mask2d is None:
        raise RuntimeError("ring_detail_stats: the ring needs mask2d")
    T, Hm, Wm, H0, W0 = hip._need_window("ring_detail_stats", patch, orig, mask2d, offsets)
    sums = torch.empty((T, NSUM), dtype=torch.int64, device=orig.device)
    with hip._Prof("detail_ring_stats", 0.0, T * int(h) * int(w) + sums.numel() * 8):
        _check(lib().vvd_ring_detail_stats(hip._p(patch), Hm, Wm, hip._p(orig), hip._p(mask2d), hip._p(offsets), T, H0, W0, int(h), int(w), int(ring),
                                           int(edge), hip._p(sums), hip._stream()), "vvd_ring_detail_stats")
    return sums


def sharpen(patch, amount, h, w, overshoot, out=None):
    """patch [T,Hm,Wm,3] u8, amount [T] int32 (q8: 256 = the whole high-pass added once), on the device -> the window's pixels [T,h,w,3] u8 on the
    device (vvd_sharpen): the resize, plus amount / 256 of the pixel's 3 x 3 binomial high-pass, clamped to the neighbourhood's range widened by
    `overshoot`; a frame with amount 0 is the resize alone.  out: an optional [T,h,w,3] u8 buffer to write (not patch)."""
    hip._need_cuda(patch, amount, out)
    if patch.dtype != torch.uint8 or patch.dim() != 4 or patch.shape[3] != 3 or patch.shape[0] < 1:
        raise RuntimeError("sharpen: patch must be a [T >= 1, Hm, Wm, 3] uint8 tensor")
    T, Hm, Wm, _ = patch.shape
    if amount.dtype != torch.int32 or tuple(amount.shape) != (T,):
        raise RuntimeError("sharpen: amount must be a [T] int32 tensor")
    shape = (T, int(h), int(w), 3)
    if tuple(patch.shape) == shape:
        out = hip._out_like("sharpen", out, patch, "patch")
    elif out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=patch.device)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8:
        raise RuntimeError("sharpen: out must be a contiguous [T, h, w, 3] u8 buffer")
    with hip._Prof("detail_sharpen", 0.0, patch.numel() + out.numel()):
        _check(lib().vvd_sharpen(hip._p(patch), Hm, Wm, hip._p(amount), T, int(h), int(w), int(overshoot), hip._p(out), hip._stream()), "vvd_sharpen")
    return out
