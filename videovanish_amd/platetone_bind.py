"""ctypes binding of the clean-plate exposure matching entry points of libvvhip.so (include/platetone.h; kernels: csrc/vv_platetone.hip).

Built on hip.py: PART (a hip.Part) declares platetone.h's part of the library once, SIGNATURES is applied when the library is first used through
this module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_platetone_cpu.py checks the table against the
header (tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
MAX_T, MAX_PIXELS = 65535, 1 << 24
MAX_RING, MAX_FLOOR, MAX_GAIN, MAX_OFFSET = 64, 127, 100, 255
NSUM = 12

# every function of include/platetone.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vve_abi_version": (I, ()),
    "vve_last_error": (C.c_char_p, ()),
    "vve_mean_plane": (I, (P, P, I, I, I, I, P, P, P, P)),
    "vve_moments": (I, (P, P, P, I, I, I, P, P)),
    "vve_apply": (I, (P, P, P, I, I, I, P, P)),
    "vve_restore": (I, (P, P, P, P, P, I, I, I, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("platetone.h", "vve_", ABI_VERSION, "clean-plate exposure matching", SIGNATURES)
lib, _check = PART.lib, PART.check


def mean_plane(frames, notsample, floor):
    """Rules 1 and 2 of platetone.h -> (R [H,W,3] u8, U [H,W] u8 {0, 1}, n [1] int64) on the device (vve_mean_plane)."""
    T, H, W = hip._need_clip("mean_plane", frames, notsample)
    dev = frames.device
    mean = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    support = torch.empty((H, W), dtype=torch.uint8, device=dev)
    n = torch.empty((1,), dtype=torch.int64, device=dev)
    with hip._Prof("platetone_mean_plane", 0.0, T * H * W * 4 + H * W * 4):
        _check(lib().vve_mean_plane(hip._p(frames), hip._p(notsample), T, H, W, int(floor), hip._p(mean), hip._p(support), hip._p(n), hip._stream()),
               "vve_mean_plane")
    return mean, support, n


def moments(frames, mean, support):
    """Rule 3 of platetone.h -> sums [T,12] int64 on the device: Sv[3], Svr[3] per frame, Sr[3], Srr[3] on row 0 (vve_moments)."""
    T, H, W = hip._need_clip("moments", frames)
    hip._need_cuda(mean, support)
    if (mean.dtype, tuple(mean.shape)) != (torch.uint8, (H, W, 3)) or (support.dtype, tuple(support.shape)) != (torch.uint8, (H, W)):
        raise RuntimeError("moments: mean [H,W,3] u8 and support [H,W] u8 are mean_plane's outputs")
    sums = torch.empty((T, NSUM), dtype=torch.int64, device=frames.device)
    with hip._Prof("platetone_moments", 0.0, T * H * W * 4):
        _check(lib().vve_moments(hip._p(frames), hip._p(mean), hip._p(support), T, H, W, hip._p(sums), hip._stream()), "vve_moments")
    return sums


def _need_flags(what, identity, T):
    hip._need_cuda(identity)
    if identity.dtype != torch.uint8 or tuple(identity.shape) != (T,):
        raise RuntimeError(f"{what}: identity must be a [T] uint8 tensor")


def apply(frames, fwd, identity, out=None):
    """f' of rule 6: frames through the forward tables fwd [T,3,256] u8, the frames with identity[t] != 0 copied -> a fresh [T,H,W,3] u8 tensor (or
    out, which must not be frames) on the device (vve_apply)."""
    T, H, W = hip._need_clip("apply", frames)
    hip._need_cuda(fwd)
    hip._need_table("apply", "fwd", fwd, T)
    _need_flags("apply", identity, T)
    out = hip._out_like("apply", out, frames, "frames")
    with hip._Prof("platetone_apply", 0.0, T * H * W * 6):
        _check(lib().vve_apply(hip._p(frames), hip._p(fwd), hip._p(identity), T, H, W, hip._p(out), hip._stream()), "vve_apply")
    return out


def restore(orig, filled, dil, dil2, back):
    """out of rule 6: the back table of what the fill took out of the mask (dil != 0, dil2 == 0), the original bytes everywhere else -> a fresh
    [T,H,W,3] u8 tensor on the device (vve_restore)."""
    T, H, W = hip._need_clip("restore", orig, dil, dil2)
    hip._need_cuda(filled, back)
    if filled.dtype != torch.uint8 or filled.shape != orig.shape:
        raise RuntimeError("restore: filled must be a uint8 tensor of orig's shape")
    hip._need_table("restore", "back", back, T)
    out = torch.empty_like(orig)
    with hip._Prof("platetone_restore", 0.0, T * H * W * 8):
        _check(lib().vve_restore(hip._p(orig), hip._p(filled), hip._p(dil), hip._p(dil2), hip._p(back), T, H, W, hip._p(out), hip._stream()), "vve_restore")
    return out
