"""ctypes binding of the mask clean-up entry points of libvvhip.so (include/vvmask.h; kernels: csrc/vv_mask.hip).

Built on hip.py: PART (a hip.Part) declares vvmask.h's part of the library once, SIGNATURES is applied when the library is first used through this
module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_maskclean_cpu.py checks the table against the header
(tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
MAX_BRIDGE, MAX_GROW, MAX_T = 16, 8, 65535
WS_BYTES = 256 << 20    # despeckle walks the clip in slabs whose two int32 workspaces stay at or below this, together

# every function of include/vvmask.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvm_abi_version": (I, ()),
    "vvm_last_error": (C.c_char_p, ()),
    "vvm_label_components": (I, (P, I, I, I, P, P)),
    "vvm_despeckle": (I, (P, P, I, I, I, I, I, P, P, P, P, P)),
    "vvm_time_bridge_grow": (I, (P, I, I, I, I, I, P, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("vvmask.h", "vvm_", ABI_VERSION, "mask clean-up", SIGNATURES)
lib, _check = PART.lib, PART.check


def _need_mask(mask2d, what):
    hip._need_cuda(mask2d)
    if mask2d.dtype != torch.uint8 or mask2d.dim() != 3 or mask2d.shape[0] < 1:
        raise RuntimeError(f"{what}: the masks must be a [T >= 1, H, W] uint8 tensor")


def label_components(mask2d):
    """mask2d [S,H,W] u8 on the device -> labels [S,H,W] int32 on the device: the smallest linear index y * W + x of the pixel's 8-connected
    component within its frame, -1 where the mask byte is zero (vvm_label_components)."""
    _need_mask(mask2d, "label_components")
    S, H, W = mask2d.shape
    labels = torch.empty((S, H, W), dtype=torch.int32, device=mask2d.device)
    with hip._Prof("mask_label", 0.0, S * H * W * 5):
        _check(lib().vvm_label_components(hip._p(mask2d), S, H, W, hip._p(labels), hip._stream()), "vvm_label_components")
    return labels


def slab_frames(H, W, ws_bytes=WS_BYTES):
    """Frames per despeckle slab: labels and weights, int32 each, within ws_bytes together (at least one frame)."""
    return max(1, ws_bytes // (8 * H * W))


def despeckle(dil, raw, min_area, slab=None):
    """dil [T,H,W] u8, raw [T,H,W,ch] (or [T,H,W]) u8, on the device -> (out [T,H,W] u8, counts [T,2] int64 = components removed, pixels
    cleared) on the device: the 8-connected components of dil that hold fewer than min_area non-zero raw pixels are cleared (vvm_despeckle).
    The clip is walked in slabs of `slab` frames (default: slab_frames); frames are independent, so the seams need no care."""
    _need_mask(dil, "despeckle")
    hip._need_cuda(raw)
    T, H, W = dil.shape
    if raw.dim() == 3:
        raw = raw[..., None]
    if raw.dtype != torch.uint8 or raw.dim() != 4 or tuple(raw.shape[:3]) != (T, H, W):
        raise RuntimeError("despeckle: raw must be a [T, H, W, ch] uint8 tensor of dil's size")
    ch = raw.shape[3]
    slab = min(T, slab_frames(H, W) if slab is None else int(slab))
    if slab < 1:
        raise ValueError("despeckle: a slab holds at least one frame")
    out = torch.empty_like(dil)
    counts = torch.empty((T, 2), dtype=torch.int64, device=dil.device)
    ws = torch.empty((2, slab, H, W), dtype=torch.int32, device=dil.device)
    for s in range(0, T, slab):
        n = min(slab, T - s)
        with hip._Prof("mask_despeckle", 0.0, n * H * W * (2 + ch + 6 * 4)):
            _check(lib().vvm_despeckle(hip._p(dil[s:]), hip._p(raw[s:]), n, H, W, ch, int(min_area), hip._p(ws[0]), hip._p(ws[1]), hip._p(out[s:]),
                                       hip._p(counts[s:]), hip._stream()), "vvm_despeckle")
    return out, counts


def time_bridge_grow(mask2d, bridge, grow, out=None, counts=None):
    """mask2d [T,H,W] u8 on the device, ONE segment -> (out [T,H,W] u8 {0, 255}, counts [T,2] int64 = pixels bridged, pixels grown) on the device:
    per pixel along time, runs of at most `bridge` zero frames between two set frames are filled, then every frame becomes the OR of the frames
    within `grow` of it (vvm_time_bridge_grow).  out / counts: contiguous views to write into (the segments of a clip)."""
    _need_mask(mask2d, "time_bridge_grow")
    T, H, W = mask2d.shape
    if out is None:
        out = torch.empty_like(mask2d)
    if counts is None:
        counts = torch.empty((T, 2), dtype=torch.int64, device=mask2d.device)
    hip._need_cuda(out, counts)
    if out.dtype != torch.uint8 or out.shape != mask2d.shape or counts.dtype != torch.int64 or tuple(counts.shape) != (T, 2):
        raise RuntimeError("time_bridge_grow: out must be a uint8 tensor of the masks' size and counts [T, 2] int64")
    with hip._Prof("mask_time", 0.0, 2 * T * H * W):
        _check(lib().vvm_time_bridge_grow(hip._p(mask2d), T, H, W, int(bridge), int(grow), hip._p(out), hip._p(counts), hip._stream()),
               "vvm_time_bridge_grow")
    return out, counts
