"""ctypes binding of the inpaint deflicker entry points of libvvhip.so (include/vvflicker.h; kernels: csrc/vv_flicker.hip).

Built on hip.py: PART (a hip.Part) declares vvflicker.h's part of the library once, SIGNATURES is applied when the library is first used through this
module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_deflicker_cpu.py checks the table against the header
(tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
MAX_RADIUS, MAX_T, SLAB = 4, 65535, 16
NSUM = 12

# every function of include/vvflicker.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvf_abi_version": (I, ()),
    "vvf_last_error": (C.c_char_p, ()),
    "vvf_window_pixels": (I, (P, I, I, I, I, I, P, P)),
    "vvf_hold": (I, (P, P, P, I, I, I, I, I, I, I, I, P, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("vvflicker.h", "vvf_", ABI_VERSION, "deflicker", SIGNATURES)
lib, _check = PART.lib, PART.check


def _need_clip(what, t):
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or t.shape[0] < 1:
        raise RuntimeError(f"{what}: the pixels must be a [T >= 1, H, W, 3] uint8 tensor")


def window_pixels(patch, h, w):
    """patch [T,Hm,Wm,3] u8 on the device (the model's output of a window) -> the window's pixels [T,h,w,3] u8 as roi_paste_composite reads them
    (vvf_window_pixels: the bilinear resize of hip.resize_u8).  At equal size nothing is launched: patch itself."""
    hip._need_cuda(patch)
    _need_clip("window_pixels", patch)
    T, Hm, Wm, _ = patch.shape
    if (Hm, Wm) == (int(h), int(w)):
        return patch
    win = torch.empty((T, int(h), int(w), 3), dtype=torch.uint8, device=patch.device)
    with hip._Prof("flicker_window_pixels", 0.0, patch.numel() + win.numel()):
        _check(lib().vvf_window_pixels(hip._p(patch), T, Hm, Wm, int(h), int(w), hip._p(win), hip._stream()), "vvf_window_pixels")
    return win


def hold(win, offsets, mask2d, radius, tol, fixed=None, out=None):
    """win [T,h,w,3] u8 (window_pixels), offsets [T,2] int32 (oy, ox), mask2d [T,H0,W0] u8, on the device -> (out [T,h,w,3] u8, sums [T,12] int64)
    on the device (vvf_hold): every pixel the rounded mean of its temporal neighbours within `radius` frames and `tol` levels, and per frame the
    pixels, the pixels changed, the sum of accepted samples and the sum of |out - in| per channel, over the window and over its masked pixels.
    fixed: whether the offsets are the same for every frame (the streaming form of the kernel); None = the caller has not looked, the gather
    form runs.  out: an optional buffer to write (not win)."""
    hip._need_cuda(win, offsets, mask2d, out)
    _need_clip("hold", win)
    T, h, w, _ = win.shape
    if offsets.dtype != torch.int32 or tuple(offsets.shape) != (T, 2) or mask2d.dtype != torch.uint8 or mask2d.dim() != 3 or mask2d.shape[0] != T:
        raise RuntimeError("hold: offsets must be [T, 2] int32 and mask2d [T, H0, W0] uint8")
    _, H0, W0 = mask2d.shape
    out = hip._out_like("hold", out, win, "win")
    sums = torch.empty((T, NSUM), dtype=torch.int64, device=win.device)
    with hip._Prof("flicker_hold", 0.0, 2 * win.numel() + T * h * w):
        _check(lib().vvf_hold(hip._p(win), hip._p(offsets), hip._p(mask2d), T, H0, W0, h, w, int(radius), int(tol), 1 if fixed else 0, hip._p(out),
                              hip._p(sums), hip._stream()), "vvf_hold")
    return out, sums
