"""ctypes binding of the mask-span entry points of libvvhip.so (include/vvspans.h; kernels: csrc/vv_spans.hip).

Built on hip.py: PART (a hip.Part) declares vvspans.h's part of the library once, SIGNATURES is applied when the library is first used through this
module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_spans_cpu.py checks the table against the header
(tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import numpy as np
import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
HIST_BINS = 64
SLAB = 64       # frames on the device at a time (frame_pair_stats)

# every function of include/vvspans.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvs_abi_version": (I, ()),
    "vvs_last_error": (C.c_char_p, ()),
    "vvs_frame_pair_stats": (I, (P, P, I, I, I, P, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("vvspans.h", "vvs_", ABI_VERSION, "mask-span", SIGNATURES)
lib, _check = PART.lib, PART.check


def pair_stats(frames, mask2d=None):
    """frames [T,H,W,3] u8, mask2d [T,H,W] u8 or None, on the device -> (n_sad [T-1,2] int64, hist [T-1,2,64] int32) on the device: for every
    adjacent frame pair, over the pixels whose mask byte is zero in both frames, (pixel count, luma sum of absolute differences) and the two
    luma histograms (vvs_frame_pair_stats)."""
    hip._need_cuda(frames, mask2d)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 2:
        raise RuntimeError("pair_stats: frames must be a [T >= 2, H, W, 3] uint8 tensor")
    T, H, W, _ = frames.shape
    if mask2d is not None and (mask2d.dtype != torch.uint8 or tuple(mask2d.shape) != (T, H, W)):
        raise RuntimeError("pair_stats: mask2d must be a [T, H, W] uint8 tensor")
    n_sad = torch.empty((T - 1, 2), dtype=torch.int64, device=frames.device)
    hist = torch.empty((T - 1, 2, HIST_BINS), dtype=torch.int32, device=frames.device)
    with hip._Prof("frame_pair_stats", 0.0, 2 * (T - 1) * H * W * (3 + (mask2d is not None))):
        _check(lib().vvs_frame_pair_stats(hip._p(frames), hip._p(mask2d), T, H, W, hip._p(n_sad), hip._p(hist), hip._stream()), "vvs_frame_pair_stats")
    return n_sad, hist


def frame_pair_stats(frames_rgb, mask2d=None, slab=SLAB, device=None):
    """The cut statistics of a whole clip, for spans.find_cuts: frames_rgb = a list of [H,W,3] u8 host frames (or one [T,H,W,3] array), mask2d = the
    dilated masks [T,H,W] u8 on the device (or a host array, or None) -> (sad [T-1], n [T-1], hist [T-1,2,64]) as int64 host arrays.
    The clip is walked in slabs of at most `slab` frames, consecutive slabs sharing one frame, so device memory stays bounded for long clips and
    every frame crosses to the device once (the shared ones twice)."""
    T = len(frames_rgb)
    if slab < 2:
        raise ValueError("frame_pair_stats: a slab holds at least two frames")
    if device is None:
        device = mask2d.device if isinstance(mask2d, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    sad, n, hist = np.zeros(max(T - 1, 0), np.int64), np.zeros(max(T - 1, 0), np.int64), np.zeros((max(T - 1, 0), 2, HIST_BINS), np.int64)
    for s in range(0, T - 1, slab - 1):
        e = min(T, s + slab)
        f = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(x) for x in frames_rgb[s:e]]))).to(device)
        m = None
        if mask2d is not None:
            m = mask2d[s:e] if isinstance(mask2d, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask2d[s:e]))
            m = m.to(device).contiguous()
        ns, hh = pair_stats(f.contiguous(), m)
        ns = ns.cpu().numpy()
        n[s:e - 1], sad[s:e - 1], hist[s:e - 1] = ns[:, 0], ns[:, 1], hh.cpu().numpy()
    return sad, n, hist
