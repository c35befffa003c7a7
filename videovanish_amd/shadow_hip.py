"""ctypes binding of the shadow-masking entry points of libvvhip.so (include/vvshadow.h; kernels: csrc/vv_shadow.hip).

Built on hip.py: PART (a hip.Part) declares vvshadow.h's part of the library once, SIGNATURES is applied when the library is first used through this
module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_shadowmask_cpu.py checks the table against the header
(tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
MAX_T, MAX_GUARD, MAX_TOL, MAX_DROP, MAX_CHROMA, MAX_FLOOR, MAX_REACH, MAX_GROW = 65535, 8, 255, 255, 100, 255, 64, 16
GROW_TILE, GROW_K = 64, 8       # vvh_grow: the interior a block owns, and the halo / the sweeps of one pass

# every function of include/vvshadow.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvh_abi_version": (I, ()),
    "vvh_last_error": (C.c_char_p, ()),
    "vvh_plate": (I, (P, P, I, I, I, I, I, P, P, P, P)),
    "vvh_candidates": (I, (P, P, P, P, P, I, I, I, I, I, I, I, I, P, P, P)),
    "vvh_grow": (I, (P, P, I, I, I, I, P, P, P)),
    "vvh_merge": (I, (P, P, I, I, I, P, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("vvshadow.h", "vvh_", ABI_VERSION, "shadow masking", SIGNATURES)
lib, _check = PART.lib, PART.check


def _need_masks(what, *masks):
    """masks [T,H,W] u8 on the device, all of one size -> (T, H, W)."""
    hip._need_cuda(*masks)
    m0 = masks[0]
    if m0.dim() != 3 or m0.shape[0] < 1:
        raise RuntimeError(f"{what}: every mask must be a [T >= 1, H, W] uint8 tensor")
    for m in masks:
        if m.dtype != torch.uint8 or m.shape != m0.shape:
            raise RuntimeError(f"{what}: every mask must be a [T, H, W] uint8 tensor of one size")
    return tuple(m0.shape)


def _need_plate(what, H, W, ok, n2, t1):
    hip._need_cuda(ok, n2, t1)
    if (ok.dtype, tuple(ok.shape)) != (torch.uint8, (H, W)) or (n2.dtype, tuple(n2.shape)) != (torch.int32, (H, W)) or \
            (t1.dtype, tuple(t1.shape)) != (torch.int32, (H, W, 3)):
        raise RuntimeError(f"{what}: ok [H,W] u8, n2 [H,W] int32 and t1 [H,W,3] int32 are plate's outputs")


def plate(frames, notsample, min_samples, tol):
    """Rules 2 and 3 of vvshadow.h -> (ok [H,W] u8, n2 [H,W] int32, t1 [H,W,3] int32 holding the header's uint32 bits; both stay below 2^31) on
    the device (vvh_plate)."""
    T, H, W = hip._need_clip("plate", frames, notsample)
    dev = frames.device
    ok = torch.empty((H, W), dtype=torch.uint8, device=dev)
    n2 = torch.empty((H, W), dtype=torch.int32, device=dev)
    t1 = torch.empty((H, W, 3), dtype=torch.int32, device=dev)
    with hip._Prof("shadow_plate", 0.0, T * H * W * 8):
        _check(lib().vvh_plate(hip._p(frames), hip._p(notsample), T, H, W, int(min_samples), int(tol), hip._p(ok), hip._p(n2), hip._p(t1),
                               hip._stream()), "vvh_plate")
    return ok, n2, t1


def candidates(frames, dil, ok, n2, t1, lo, hi, drop, chroma, floor):
    """Rule 4 of vvshadow.h -> (cand [T,H,W] u8 {0, 1}, counts [T,2] int64: column 0 = the candidates, column 1 = 0 for merge) on the device
    (vvh_candidates)."""
    T, H, W = hip._need_clip("candidates", frames, dil)
    _need_plate("candidates", H, W, ok, n2, t1)
    cand = torch.empty((T, H, W), dtype=torch.uint8, device=frames.device)
    counts = torch.empty((T, 2), dtype=torch.int64, device=frames.device)
    with hip._Prof("shadow_candidates", 0.0, T * H * W * 5):
        _check(lib().vvh_candidates(hip._p(frames), hip._p(dil), hip._p(ok), hip._p(n2), hip._p(t1), T, H, W, int(lo), int(hi), int(drop), int(chroma),
                                    int(floor), hip._p(cand), hip._p(counts), hip._stream()), "vvh_candidates")
    return cand, counts


def grow(a0, cand, reach):
    """Rule 5 of vvshadow.h: a0, cand [T,H,W] u8 on the device -> S [T,H,W] u8 {0, 255} = A_reach without A_0 (vvh_grow)."""
    T, H, W = _need_masks("grow", a0, cand)
    s, ws = torch.empty_like(a0), torch.empty_like(a0)
    passes = max(1, -(-int(reach) // GROW_K))
    with hip._Prof("shadow_grow", 0.0, passes * T * H * W * 3):
        _check(lib().vvh_grow(hip._p(a0), hip._p(cand), T, H, W, int(reach), hip._p(ws), hip._p(s), hip._stream()), "vvh_grow")
    return s


def merge(dil, s, counts):
    """Rule 7's union of vvshadow.h: dil, s [T,H,W] u8, counts = candidates' [T,2] int64 (column 1 gains the added pixels, in place) -> dil'
    [T,H,W] u8 {0, 255} on the device (vvh_merge)."""
    T, H, W = _need_masks("merge", dil, s)
    hip._need_cuda(counts)
    if counts.dtype != torch.int64 or tuple(counts.shape) != (T, 2):
        raise RuntimeError("merge: counts must be candidates' [T, 2] int64 tensor")
    out = torch.empty_like(dil)
    with hip._Prof("shadow_merge", 0.0, T * H * W * 3):
        _check(lib().vvh_merge(hip._p(dil), hip._p(s), T, H, W, hip._p(out), hip._p(counts), hip._stream()), "vvh_merge")
    return out
