"""ctypes binding of the seam membrane blending entry points of libvvhip.so (include/vvblend.h; kernels: csrc/vv_blend.hip).

Built on hip.py: PART (a hip.Part) declares vvblend.h's part of the library once, SIGNATURES is applied when the library is first used through this
module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_seamblend_cpu.py checks the table against the header
(tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip, seamblend
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
NSUM = 11
L = C.c_int64

# every function of include/vvblend.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvb_abi_version": (I, ()),
    "vvb_last_error": (C.c_char_p, ()),
    "vvb_levels": (I, (I, I)),
    "vvb_scratch_bytes": (L, (I, I, I)),
    "vvb_ring_diff": (I, (P, I, I, P, P, P, P, I, I, I, I, I, I, I, I, P, P, P, P)),
    "vvb_pull": (I, (P, P, I, I, I, P, P, P)),
    "vvb_relax": (I, (P, P, P, P, I, I, I, I, I, P, P)),
    "vvb_solve": (I, (P, I, I, P, P, P, P, I, I, I, I, I, I, I, I, I, P, L, P, P)),
    "vvb_paste_blend_composite": (I, (P, I, I, P, P, P, P, P, I, P, P, I, I, I, I, I, I, I, C.c_float, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("vvblend.h", "vvb_", ABI_VERSION, "seam blending", SIGNATURES)
lib, _check = PART.lib, PART.check


def scratch_bytes(T, h, w):
    """vvb_scratch_bytes: the bytes of scratch solve needs for T frames of an h x w window (seamblend.scratch_bytes restates it)."""
    return int(lib().vvb_scratch_bytes(int(T), int(h), int(w)))


def _level(what, cls, val):
    hip._need_cuda(cls, val)
    if cls.dtype != torch.uint8 or cls.dim() != 3 or val.dtype != torch.int16 or tuple(val.shape) != (*cls.shape, 3):
        raise RuntimeError(f"{what}: cls must be a [T, h, w] uint8 and val a [T, h, w, 3] int16 tensor")
    return tuple(cls.shape)


def ring_diff(patch, orig, mask2d, offsets, lut, h, w, ring, presmooth, max_shift):
    """Level 0 before the solve (vvb_ring_diff) -> (cls [T,h,w] u8, val [T,h,w,3] int16, sums [T,11] int64), on the device: the classes of the
    window's cells, the presmoothed Q6 value of y - x on the ring pixels (0 elsewhere), and entries 0 .. 3 of the sums."""
    if mask2d is None:
        raise RuntimeError("ring_diff: the ring needs mask2d")
    hip._need_cuda(lut)
    T, Hm, Wm, H0, W0 = hip._need_window("ring_diff", patch, orig, mask2d, offsets)
    hip._need_table("ring_diff", "lut", lut, T)
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise RuntimeError("ring_diff: the window must hold a pixel")
    cls = torch.empty((T, h, w), dtype=torch.uint8, device=orig.device)
    val = torch.empty((T, h, w, 3), dtype=torch.int16, device=orig.device)
    sums = torch.empty((T, NSUM), dtype=torch.int64, device=orig.device)
    with hip._Prof("blend_ring_diff", 0.0, T * h * w * 8):
        _check(lib().vvb_ring_diff(hip._p(patch), Hm, Wm, hip._p(orig), hip._p(mask2d), hip._p(offsets), hip._p(lut), T, H0, W0, h, w, int(ring),
                                   int(presmooth), int(max_shift), hip._p(cls), hip._p(val), hip._p(sums), hip._stream()), "vvb_ring_diff")
    return cls, val, sums


def pull(cls, val):
    """One level up (vvb_pull) -> (cls_up, val_up) of the halved grid."""
    T, hl, wl = _level("pull", cls, val)
    cls_up = torch.empty((T, (hl + 1) // 2, (wl + 1) // 2), dtype=torch.uint8, device=cls.device)
    val_up = torch.empty((*cls_up.shape, 3), dtype=torch.int16, device=cls.device)
    with hip._Prof("blend_pull", 0.0, cls.numel() * 7):
        _check(lib().vvb_pull(hip._p(cls), hip._p(val), T, hl, wl, hip._p(cls_up), hip._p(val_up), hip._stream()), "vvb_pull")
    return cls_up, val_up


def relax(cls, val, sweeps, parent=None, start=True, out=None, sums=None):
    """`sweeps` Jacobi sweeps on one level in one launch (vvb_relax) -> out [T,hl,wl,3] int16.  start=True: the unknown cells start from parent
    (the level above; None: from 0) and out may be val; start=False: from val, into another buffer.  sums ([T,11] int64) gets entries 4 .. 10
    added."""
    T, hl, wl = _level("relax", cls, val)
    hip._need_cuda(parent, out, sums)
    if parent is not None and (parent.dtype != torch.int16 or tuple(parent.shape) != (T, (hl + 1) // 2, (wl + 1) // 2, 3)):
        raise RuntimeError("relax: parent must be the [T, ceil(hl / 2), ceil(wl / 2), 3] int16 level above")
    if out is None:
        out = torch.empty_like(val)
    elif out.shape != val.shape or out.dtype != torch.int16:
        raise RuntimeError("relax: out must be an int16 buffer of val's shape")
    if sums is not None and (sums.dtype != torch.int64 or tuple(sums.shape) != (T, NSUM)):
        raise RuntimeError("relax: sums must be a [T, 11] int64 tensor")
    with hip._Prof("blend_relax", 0.0, cls.numel() * 13):
        _check(lib().vvb_relax(hip._p(cls), hip._p(val), hip._p(parent), hip._p(out), T, hl, wl, int(sweeps), 1 if start else 0, hip._p(sums),
                               hip._stream()), "vvb_relax")
    return out


def solve(patch, orig, mask2d, offsets, lut, h, w, ring, presmooth, sweeps, max_shift, scratch=None):
    """The whole field of T frames of the window (vvb_solve) -> (field [T,h,w,3] int16, cls [T,h,w] u8, sums [T,11] int64): field and cls are
    views of scratch (a uint8 device tensor of at least scratch_bytes(T, h, w) bytes; allocated here when None)."""
    if mask2d is None:
        raise RuntimeError("solve: the ring needs mask2d")
    hip._need_cuda(lut, scratch)
    T, Hm, Wm, H0, W0 = hip._need_window("solve", patch, orig, mask2d, offsets)
    hip._need_table("solve", "lut", lut, T)
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise RuntimeError("solve: the window must hold a pixel")
    need = seamblend.scratch_bytes(T, h, w)
    if scratch is None:
        scratch = torch.empty((need,), dtype=torch.uint8, device=orig.device)
    elif scratch.dtype != torch.uint8 or scratch.dim() != 1 or scratch.numel() < need:
        raise RuntimeError(f"solve: scratch must be a uint8 tensor of at least {need} bytes")
    sums = torch.empty((T, NSUM), dtype=torch.int64, device=orig.device)
    with hip._Prof("blend_solve", 0.0, T * h * w * 30):
        _check(lib().vvb_solve(hip._p(patch), Hm, Wm, hip._p(orig), hip._p(mask2d), hip._p(offsets), hip._p(lut), T, H0, W0, h, w, int(ring),
                               int(presmooth), int(sweeps), int(max_shift), hip._p(scratch), scratch.numel(), hip._p(sums), hip._stream()), "vvb_solve")
    n = T * h * w
    return scratch[:6 * n].view(torch.int16).view(T, h, w, 3), scratch[6 * n:7 * n].view(T, h, w), sums


def paste_blend_composite(patch, orig, mask2d, offsets, lut, field, strength_q8, amp, frame_ids, seed, mode, h, w, feather_px, out=None):
    """grain_hip.paste_grain_composite with the membrane: after lut and before the grain, channel c of a pixel of the window gets
    (field * strength_q8 + 2^13) >> 14 added (field [T,h,w,3] int16, Q6).  A zero field gives paste_grain_composite's bytes."""
    hip._need_cuda(lut, field, amp, frame_ids, out)
    T, Hm, Wm, H0, W0 = hip._need_window("paste_blend_composite", patch, orig, mask2d, offsets)
    hip._need_table("paste_blend_composite", "lut", lut, T)
    hip._need_table("paste_blend_composite", "amp", amp, T)
    if field.dtype != torch.int16 or tuple(field.shape) != (T, int(h), int(w), 3):
        raise RuntimeError("paste_blend_composite: field must be a [T, h, w, 3] int16 tensor")
    if frame_ids.dtype != torch.int32 or tuple(frame_ids.shape) != (T,):
        raise RuntimeError("paste_blend_composite: frame_ids must be a [T] int32 tensor")
    out = hip._out_like("paste_blend_composite", out, orig, "orig")
    with hip._Prof("blend_paste_composite", 0.0, T * H0 * W0 * (3 + 1 + 3) + patch.numel() + field.numel() * 2):
        _check(lib().vvb_paste_blend_composite(hip._p(patch), Hm, Wm, hip._p(orig), hip._p(mask2d), hip._p(offsets), hip._p(lut), hip._p(field),
                                               int(strength_q8), hip._p(amp), hip._p(frame_ids), int(seed), int(mode), T, H0, W0, int(h), int(w),
                                               float(feather_px), hip._p(out), hip._stream()), "vvb_paste_blend_composite")
    return out
