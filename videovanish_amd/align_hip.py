"""ctypes binding of the clean-plate alignment entry points of libvvhip.so (include/vvalign.h; kernels: csrc/vv_align.hip).

Built on hip.py: PART (a hip.Part) declares vvalign.h's part of the library once, SIGNATURES is applied when the library is first used through this
module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_platealign_cpu.py checks the table against the header
(tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

L64 = C.c_int64
ABI_VERSION = 1
MAX_LEVELS, MAX_RADIUS, MAX_PIXELS, MAX_T = 6, 8, 1 << 24, 65535
IN_PROGRESS, TRACK_INTS = -1, 8

# every function of include/vvalign.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vva_abi_version": (I, ()),
    "vva_last_error": (C.c_char_p, ()),
    "vva_frame_bytes": (L64, (I, I, I)),
    "vva_pyramid": (I, (P, P, I, I, I, I, P, P)),
    "vva_sad": (I, (P, P, I, I, I, I, I, I, I, P, P)),
    "vva_pick": (I, (P, P, I, I, I, I, I, I, I, I, I, P)),
    "vva_track": (I, (P, P, P, I, I, I, I, I, I, I, P)),
    "vva_track_launches": (L64, (I, I)),
    "vva_place_masks": (I, (P, P, I, I, I, I, I, I, I, P, P, P)),
    "vva_unplace_mask": (I, (P, P, P, I, I, I, I, I, I, I, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("vvalign.h", "vva_", ABI_VERSION, "clean-plate alignment", SIGNATURES)
lib = PART.lib


def _check(rc, what):      # not PART.check: vva_frame_bytes and vva_track_launches answer with a count, so only rc < 0 is an error and rc is handed on
    if rc < 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib().vva_last_error().decode()}")
    return rc


def frame_bytes(H, W, L):
    """S of vvalign.h: the bytes of one frame's record in the packed pyramid buffer (levels 0 .. L)."""
    return int(_check(lib().vva_frame_bytes(int(H), int(W), int(L)), "vva_frame_bytes"))


def track_launches(T, L):
    return int(_check(lib().vva_track_launches(int(T), int(L)), "vva_track_launches"))


def _need_track(what, track, T):
    hip._need_cuda(track)
    if track.dtype != torch.int32 or tuple(track.shape) != (T, TRACK_INTS):
        raise RuntimeError(f"{what}: track must be a [T, {TRACK_INTS}] int32 tensor")


def _need_pyr(what, pyr, H, W, L):
    hip._need_cuda(pyr)
    if pyr.dtype != torch.uint8 or pyr.dim() != 2 or pyr.shape[0] < 1 or pyr.shape[1] != frame_bytes(H, W, L):
        raise RuntimeError(f"{what}: pyr must be a [T >= 1, frame_bytes(H, W, L)] uint8 tensor")
    return pyr.shape[0]


def pyramid(frames, dil, L, out=None):
    """Luma and pyramid of vvalign.h: frames [B,H,W,3] u8, dil [B,H,W] u8 -> pyr [B, S] u8 on the device (vva_pyramid); out = the rows of a
    segment's buffer to write instead of a new tensor."""
    hip._need_cuda(frames, dil, out)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise RuntimeError("pyramid: the frames must be a [B >= 1, H, W, 3] uint8 tensor")
    B, H, W, _ = frames.shape
    if dil.dtype != torch.uint8 or tuple(dil.shape) != (B, H, W):
        raise RuntimeError("pyramid: dil must be a [B, H, W] uint8 tensor of the frames' size")
    S = frame_bytes(H, W, L)
    if out is None:
        out = torch.empty((B, S), dtype=torch.uint8, device=frames.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, S):
        raise RuntimeError("pyramid: out must be a [B, frame_bytes(H, W, L)] uint8 tensor")
    with hip._Prof("align_pyramid", 0.0, B * H * W * 7):
        _check(lib().vva_pyramid(hip._p(frames), hip._p(dil), B, H, W, int(L), hip._p(out), hip._stream()), "vva_pyramid")
    return out


def sad(pyr, track, H, W, L, t, level, r):
    """(sad, n) of every candidate of one level of frame t against its key -> acc [(2r+1)^2, 2] int64 on the device (vva_sad)."""
    T = _need_pyr("sad", pyr, H, W, L)
    _need_track("sad", track, T)
    acc = torch.empty((max(2 * int(r) + 1, 1) ** 2, 2), dtype=torch.int64, device=pyr.device)
    _check(lib().vva_sad(hip._p(pyr), hip._p(track), T, int(H), int(W), int(L), int(t), int(level), int(r), hip._p(acc), hip._stream()), "vva_sad")
    return acc


def pick(acc, track, H, W, L, t, level, r, min_overlap, max_residual):
    """The order, eligibility, acceptance and key rules on sad's acc, IN PLACE on track (vva_pick)."""
    hip._need_cuda(acc)
    T = track.shape[0] if track.dim() == 2 else 0
    _need_track("pick", track, T)
    if acc.dtype != torch.int64 or tuple(acc.shape) != ((2 * int(r) + 1) ** 2, 2):
        raise RuntimeError("pick: acc must be sad's [(2r+1)^2, 2] int64 tensor")
    _check(lib().vva_pick(hip._p(acc), hip._p(track), T, int(H), int(W), int(L), int(t), int(level), int(r), int(min_overlap), int(max_residual),
                          hip._stream()), "vva_pick")
    return track


def track(pyr, H, W, L, radius, min_overlap, max_residual):
    """The whole segment -> track [T, 8] int32 on the device (vva_track): every launch is enqueued, nothing is waited for."""
    T = _need_pyr("track", pyr, H, W, L)
    out = torch.empty((T, TRACK_INTS), dtype=torch.int32, device=pyr.device)
    acc = torch.empty((max((2 * int(radius) + 1) ** 2, 9), 2), dtype=torch.int64, device=pyr.device)
    with hip._Prof("align_track", 0.0, 0):
        _check(lib().vva_track(hip._p(pyr), hip._p(out), hip._p(acc), T, int(H), int(W), int(L), int(radius), int(min_overlap), int(max_residual),
                               hip._stream()), "vva_track")
    return out


def _need_masks(what, dil, track):
    hip._need_cuda(dil)
    if dil.dtype != torch.uint8 or dil.dim() != 3 or dil.shape[0] < 1:
        raise RuntimeError(f"{what}: dil must be a [T >= 1, H, W] uint8 tensor")
    _need_track(what, track, dil.shape[0])
    return tuple(dil.shape)


def place_masks(dil, track, box):
    """dil [T,H,W] + track + the canvas box (y0, x0, y1, x1 in canvas coordinates) -> (dil_c, invalid_c) [T,ch,cw] u8 (vva_place_masks)."""
    T, H, W = _need_masks("place_masks", dil, track)
    y0, x0, y1, x1 = (int(v) for v in box)
    ch, cw = y1 - y0, x1 - x0
    if ch < 1 or cw < 1:
        raise RuntimeError("place_masks: the canvas box is empty")
    dil_c = torch.empty((T, ch, cw), dtype=torch.uint8, device=dil.device)
    inv_c = torch.empty_like(dil_c)
    _check(lib().vva_place_masks(hip._p(dil), hip._p(track), T, H, W, y0, x0, ch, cw, hip._p(dil_c), hip._p(inv_c), hip._stream()), "vva_place_masks")
    return dil_c, inv_c


def unplace_mask(dil_out_c, dil, track, box):
    """The canvas masks back in frame coordinates -> dil' [T,H,W] u8 (vva_unplace_mask); untracked frames keep their mask."""
    T, H, W = _need_masks("unplace_mask", dil, track)
    y0, x0, y1, x1 = (int(v) for v in box)
    hip._need_cuda(dil_out_c)
    if dil_out_c.dtype != torch.uint8 or tuple(dil_out_c.shape) != (T, y1 - y0, x1 - x0):
        raise RuntimeError("unplace_mask: dil_out_c must be a [T, ch, cw] uint8 tensor of the box's size")
    out = torch.empty_like(dil)
    _check(lib().vva_unplace_mask(hip._p(dil_out_c), hip._p(dil), hip._p(track), T, H, W, y0, x0, y1 - y0, x1 - x0, hip._p(out), hip._stream()),
           "vva_unplace_mask")
    return out
