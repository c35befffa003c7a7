"""ctypes binding of the aligned inpaint deflicker entry points of libvvhip.so (include/vvflickalign.h; kernel: csrc/vv_flicker.hip).

Built on hip.py: PART (a hip.Part) declares vvflickalign.h's part of the library once, SIGNATURES is applied when the library is first used through
this module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_deflickeralign_cpu.py checks the table against the
header (tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
MAX_RADIUS, MAX_T, TRACK_INTS = 4, 65535, 8
NSUM = 12

# every function of include/vvflickalign.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvc_abi_version": (I, ()),
    "vvc_last_error": (C.c_char_p, ()),
    "vvc_hold": (I, (P, P, P, P, I, I, I, I, I, I, I, P, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("vvflickalign.h", "vvc_", ABI_VERSION, "aligned deflicker", SIGNATURES)
lib, _check = PART.lib, PART.check


def hold(win, offsets, track, mask2d, radius, tol, out=None):
    """win [T,h,w,3] u8 (flicker_hip.window_pixels), offsets [T,2] int32 (oy, ox), track [T,8] int32 (align_hip.track's records), mask2d
    [T,H0,W0] u8, on the device -> (out [T,h,w,3] u8, sums [T,12] int64) on the device (vvc_hold): flicker_hip.hold's filter with every
    temporal neighbour read where the track says the same piece of background sits in it; a frame the tracker lost takes no sample and gives
    none.  out: an optional buffer to write (not win)."""
    hip._need_cuda(win, offsets, track, mask2d, out)
    if win.dtype != torch.uint8 or win.dim() != 4 or win.shape[3] != 3 or win.shape[0] < 1:
        raise RuntimeError("hold: the pixels must be a [T >= 1, H, W, 3] uint8 tensor")
    T, h, w, _ = win.shape
    if offsets.dtype != torch.int32 or tuple(offsets.shape) != (T, 2) or mask2d.dtype != torch.uint8 or mask2d.dim() != 3 or mask2d.shape[0] != T:
        raise RuntimeError("hold: offsets must be [T, 2] int32 and mask2d [T, H0, W0] uint8")
    if track.dtype != torch.int32 or tuple(track.shape) != (T, TRACK_INTS):
        raise RuntimeError(f"hold: track must be [T, {TRACK_INTS}] int32")
    _, H0, W0 = mask2d.shape
    out = hip._out_like("hold", out, win, "win")
    sums = torch.empty((T, NSUM), dtype=torch.int64, device=win.device)
    with hip._Prof("flickalign_hold", 0.0, 2 * win.numel() + T * h * w):
        _check(lib().vvc_hold(hip._p(win), hip._p(offsets), hip._p(track), hip._p(mask2d), T, H0, W0, h, w, int(radius), int(tol), hip._p(out),
                              hip._p(sums), hip._stream()), "vvc_hold")
    return out, sums
