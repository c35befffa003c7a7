"""ctypes binding of the clean-plate fill entry points of libvvhip.so (include/vvplate.h; kernels: csrc/vv_plate.hip).

Built on hip.py: PART (a hip.Part) declares vvplate.h's part of the library once, SIGNATURES is applied when the library is first used through this
module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_platefill_cpu.py checks the table against the header
(tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
MAX_T, NO_SOURCE = 65535, 65535
MAX_GUARD, MAX_TOL, MAX_OUTLIER, MAX_GAP = 8, 255, 64, 65535
TILE = 64               # px: the occupancy grid (hip.mask_tile_union) the kernels skip on; a multiple of 4 keeps the 4-pixel form

# every function of include/vvplate.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvp_abi_version": (I, ()),
    "vvp_last_error": (C.c_char_p, ()),
    "vvp_stats": (I, (P, P, P, I, I, I, I, I, I, P, P, P, P)),
    "vvp_sources": (I, (P, P, P, P, P, P, P, I, I, I, I, I, I, I, P, P, P)),
    "vvp_fill": (I, (P, P, P, P, P, I, I, I, I, P, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("vvplate.h", "vvp_", ABI_VERSION, "clean-plate fill", SIGNATURES)
lib, _check = PART.lib, PART.check


def _need_clip(what, frames, *masks, occ=None, tile=TILE):
    """hip._need_clip, and occ [ceil(H/tile), ceil(W/tile)] u8 or None on the device -> (T, H, W)."""
    T, H, W = hip._need_clip(what, frames, *masks)
    hip._need_cuda(occ)
    if occ is not None and (occ.dtype != torch.uint8 or tuple(occ.shape) != ((H + tile - 1) // tile, (W + tile - 1) // tile)):
        raise RuntimeError(f"{what}: occ must be the [ceil(H / tile), ceil(W / tile)] uint8 grid of hip.mask_tile_union")
    return T, H, W


def stats(frames, notsample, occ, min_samples, tol, tile=TILE):
    """Rules 2 and 3 of vvplate.h -> (steady [H,W] u8, n [H,W] int32, s1 [H,W,3] int32) on the device (vvp_stats)."""
    T, H, W = _need_clip("stats", frames, notsample, occ=occ, tile=tile)
    dev = frames.device
    steady = torch.empty((H, W), dtype=torch.uint8, device=dev)
    n = torch.empty((H, W), dtype=torch.int32, device=dev)
    s1 = torch.empty((H, W, 3), dtype=torch.int32, device=dev)
    with hip._Prof("plate_stats", 0.0, T * H * W * 4):
        _check(lib().vvp_stats(hip._p(frames), hip._p(notsample), hip._p(occ), T, H, W, int(tile), int(min_samples), int(tol), hip._p(steady), hip._p(n),
                               hip._p(s1), hip._stream()), "vvp_stats")
    return steady, n, s1


def sources(frames, dil, notsample, occ, steady, n, s1, tol, outlier, max_gap, tile=TILE):
    """Rules 4 and 5 of vvplate.h and R0 of rule 6 -> (src [T,H,W] int16 holding the header's uint16 bits: -1 is NO_SOURCE; r0 [T,H,W] u8) on the
    device (vvp_sources)."""
    T, H, W = _need_clip("sources", frames, dil, notsample, occ=occ, tile=tile)
    hip._need_cuda(steady, n, s1)
    if (steady.dtype, tuple(steady.shape)) != (torch.uint8, (H, W)) or (n.dtype, tuple(n.shape)) != (torch.int32, (H, W)) or \
            (s1.dtype, tuple(s1.shape)) != (torch.int32, (H, W, 3)):
        raise RuntimeError("sources: steady [H,W] u8, n [H,W] int32 and s1 [H,W,3] int32 are stats' outputs")
    src = torch.empty((T, H, W), dtype=torch.int16, device=frames.device)
    r0 = torch.empty((T, H, W), dtype=torch.uint8, device=frames.device)
    with hip._Prof("plate_sources", 0.0, T * H * W * 12):
        _check(lib().vvp_sources(hip._p(frames), hip._p(dil), hip._p(notsample), hip._p(occ), hip._p(steady), hip._p(n), hip._p(s1), T, H, W, int(tile),
                                 int(tol), int(outlier), int(max_gap), hip._p(src), hip._p(r0), hip._stream()), "vvp_sources")
    return src, r0


def fill(frames, dil, keep, occ, src, tile=TILE):
    """Rule 7 of vvplate.h, IN PLACE on frames -> (dil' [T,H,W] u8 {0, 255}, counts [T,2] int64 = pixels filled, masked pixels left) on the
    device (vvp_fill).  src: sources' int16 tensor."""
    T, H, W = _need_clip("fill", frames, dil, keep, occ=occ, tile=tile)
    hip._need_cuda(src)
    if src.dtype != torch.int16 or tuple(src.shape) != (T, H, W):
        raise RuntimeError("fill: src must be sources' [T, H, W] int16 tensor")
    out = torch.empty_like(dil)
    counts = torch.empty((T, 2), dtype=torch.int64, device=frames.device)
    with hip._Prof("plate_fill", 0.0, T * H * W * 3):
        _check(lib().vvp_fill(hip._p(frames), hip._p(dil), hip._p(keep), hip._p(occ), hip._p(src), T, H, W, int(tile), hip._p(out), hip._p(counts),
                              hip._stream()), "vvp_fill")
    return out, counts
