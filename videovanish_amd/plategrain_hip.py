"""ctypes binding of the rotated clean-plate sources of libvvhip.so (include/vvplategrain.h; kernel: csrc/vv_plate.hip).

Built on hip.py: PART (a hip.Part) declares vvplategrain.h's part of the library once, SIGNATURES is applied when the library is first used through
this module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_plategrain_cpu.py checks the table against the
header (tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip, plate_hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
MAX_DEPTH, MAX_REACH = 8, 65535

# every function of include/vvplategrain.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvl_abi_version": (I, ()),
    "vvl_last_error": (C.c_char_p, ()),
    "vvl_sources": (I, (P, P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, P, P, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("vvplategrain.h", "vvl_", ABI_VERSION, "clean-plate grain", SIGNATURES)
lib, _check = PART.lib, PART.check


def sources(frames, dil, notsample, occ, steady, n, s1, tol, outlier, max_gap, depth, reach, tile=plate_hip.TILE):
    """plate_hip.sources' arguments plus depth and reach -> (src, live, r0) on the device (vvl_sources): src [T,H,W] int16 and r0 [T,H,W] u8 are
    plate_hip.sources' bytes, live [T,H,W] int16 (the header's uint16 bits: -1 is NO_SOURCE) is the frame each masked pixel takes its bytes from
    under the rule of vvplategrain.h; plate_hip.fill takes it in place of src."""
    T, H, W = plate_hip._need_clip("sources", frames, dil, notsample, occ=occ, tile=tile)
    hip._need_cuda(steady, n, s1)
    if (steady.dtype, tuple(steady.shape)) != (torch.uint8, (H, W)) or (n.dtype, tuple(n.shape)) != (torch.int32, (H, W)) or \
            (s1.dtype, tuple(s1.shape)) != (torch.int32, (H, W, 3)):
        raise RuntimeError("sources: steady [H,W] u8, n [H,W] int32 and s1 [H,W,3] int32 are plate_hip.stats' outputs")
    src = torch.empty((T, H, W), dtype=torch.int16, device=frames.device)
    live = torch.empty((T, H, W), dtype=torch.int16, device=frames.device)
    r0 = torch.empty((T, H, W), dtype=torch.uint8, device=frames.device)
    with hip._Prof("plategrain_sources", 0.0, T * H * W * 16):
        _check(lib().vvl_sources(hip._p(frames), hip._p(dil), hip._p(notsample), hip._p(occ), hip._p(steady), hip._p(n), hip._p(s1), T, H, W, int(tile),
                                 int(tol), int(outlier), int(max_gap), int(depth), int(reach), hip._p(src), hip._p(live), hip._p(r0), hip._stream()),
               "vvl_sources")
    return src, live, r0
