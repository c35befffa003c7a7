"""ctypes binding of the overlay-masking entry points of libvvhip.so (include/overlaymask.h; kernels: csrc/vv_overlay.hip).

Built on hip.py: PART (a hip.Part) declares overlaymask.h's part of the library once, SIGNATURES is applied when the library is first used
through this module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_overlaymask_cpu.py checks the table
against the header (tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
MAX_T, MAX_MAG, MAX_COH, MAX_BOXES = 65535, 2040, 100, 256
TILE_W, TILE_H = 64, 16         # vvo_accumulate: the pixels a block owns

# every function of include/overlaymask.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvo_abi_version": (I, ()),
    "vvo_last_error": (C.c_char_p, ()),
    "vvo_accumulate": (I, (P, P, I, I, I, P, P)),
    "vvo_classify": (I, (P, I, I, I, I, I, P, P, P)),
    "vvo_component_stats": (I, (P, I, I, P, P)),
    "vvo_select": (I, (P, P, I, I, I, I, I, P, P, P, P)),
    "vvo_merge": (I, (P, P, I, I, I, P, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("overlaymask.h", "vvo_", ABI_VERSION, "overlay masking", SIGNATURES)
lib, _check = PART.lib, PART.check


def _need_map(what, name, t, H, W, dtype=torch.uint8, last=()):
    if t.dtype != dtype or tuple(t.shape) != (H, W) + tuple(last):
        raise RuntimeError(f"{what}: {name} must be a {list((H, W) + tuple(last))} {str(dtype).replace('torch.', '')} tensor")


def new_acc(H, W, device):
    """The cleared sums [H,W,4] int32 = (n, Sx, Sy, A) a clip's batches are added into."""
    return torch.zeros((H, W, 4), dtype=torch.int32, device=device)


def accumulate(frames, dil, acc):
    """Rule 1 of overlaymask.h for one batch: frames [Tb,H,W,3] u8, dil [Tb,H,W] u8; the batch's four sums are added to acc [H,W,4] int32
    in place (vvo_accumulate).  -> acc."""
    T, H, W = hip._need_clip("accumulate", frames, dil)
    hip._need_cuda(acc)
    _need_map("accumulate", "acc", acc, H, W, torch.int32, (4,))
    with hip._Prof("overlay_accumulate", 0.0, T * H * W * 4 + H * W * 32):
        _check(lib().vvo_accumulate(hip._p(frames), hip._p(dil), T, H, W, hip._p(acc), hip._stream()), "vvo_accumulate")
    return acc


def classify(acc, min_samples, mag, coh):
    """Rule 2 of overlaymask.h: acc [H,W,4] int32 -> (edge [H,W] u8 {0, 255}, counts [2] int64 = (strong, edges)) on the device
    (vvo_classify)."""
    hip._need_cuda(acc)
    if acc.dtype != torch.int32 or acc.dim() != 3 or acc.shape[2] != 4:
        raise RuntimeError("classify: acc must be an [H, W, 4] int32 tensor")
    H, W, _ = acc.shape
    edge = torch.empty((H, W), dtype=torch.uint8, device=acc.device)
    counts = torch.empty((2,), dtype=torch.int64, device=acc.device)
    with hip._Prof("overlay_classify", 0.0, H * W * 17):
        _check(lib().vvo_classify(hip._p(acc), H, W, int(min_samples), int(mag), int(coh), hip._p(edge), hip._p(counts), hip._stream()), "vvo_classify")
    return edge, counts


def _need_labels(what, labels):
    hip._need_cuda(labels)
    if labels.dtype != torch.int32 or labels.dim() != 2 or labels.numel() < 1:
        raise RuntimeError(f"{what}: labels must be an [H, W] int32 tensor (one frame of label_components)")
    return tuple(labels.shape)


def component_stats(labels):
    """labels [H,W] int32 (mask_hip.label_components' output for one frame) -> stats [H*W,5] int32 on the device: row l of a label l holds
    (area, x0, y0, x1, y1), every other row (0, W, H, 0, 0) (vvo_component_stats)."""
    H, W = _need_labels("component_stats", labels)
    stats = torch.empty((H * W, 5), dtype=torch.int32, device=labels.device)
    with hip._Prof("overlay_stats", 0.0, H * W * 24):
        _check(lib().vvo_component_stats(hip._p(labels), H, W, hip._p(stats), hip._stream()), "vvo_component_stats")
    return stats


def select(labels, stats, min_area, max_area_px, inside_only):
    """The kept components of overlaymask.h's rules 5 and 6: labels [H,W] int32, stats = component_stats(labels) -> (out [H,W] u8 {0, 255},
    boxes [256,6] int32 = (label, area, x0, y0, x1, y1), rows past the count undefined, nboxes [1] int32 = the true count) on the device
    (vvo_select)."""
    H, W = _need_labels("select", labels)
    hip._need_cuda(stats)
    if stats.dtype != torch.int32 or tuple(stats.shape) != (H * W, 5):
        raise RuntimeError("select: stats must be component_stats' [H * W, 5] int32 tensor")
    dev = labels.device
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    boxes = torch.empty((MAX_BOXES, 6), dtype=torch.int32, device=dev)
    nboxes = torch.empty((1,), dtype=torch.int32, device=dev)
    with hip._Prof("overlay_select", 0.0, H * W * 9):
        _check(lib().vvo_select(hip._p(labels), hip._p(stats), H, W, int(min_area), int(max_area_px), int(bool(inside_only)), hip._p(out), hip._p(boxes),
                                hip._p(nboxes), hip._stream()), "vvo_select")
    return out, boxes, nboxes


def merge(dil, o):
    """Rules 7 and 8 of overlaymask.h: dil [T,H,W] u8, o [H,W] u8 -> (dil' [T,H,W] u8 {0, 255}, added [T] int64) on the device (vvo_merge)."""
    hip._need_cuda(dil, o)
    if dil.dtype != torch.uint8 or dil.dim() != 3 or dil.shape[0] < 1:
        raise RuntimeError("merge: dil must be a [T >= 1, H, W] uint8 tensor")
    T, H, W = dil.shape
    _need_map("merge", "o", o, H, W)
    out = torch.empty_like(dil)
    added = torch.empty((T,), dtype=torch.int64, device=dil.device)
    with hip._Prof("overlay_merge", 0.0, T * H * W * 2 + H * W):
        _check(lib().vvo_merge(hip._p(dil), hip._p(o), T, H, W, hip._p(out), hip._p(added), hip._stream()), "vvo_merge")
    return out, added
