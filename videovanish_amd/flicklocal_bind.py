"""ctypes binding of the block-matched inpaint deflicker entry points of libvvhip.so (include/flicklocal.h; kernels: csrc/vv_flicklocal.hip).

Built on hip.py: PART (a hip.Part) declares flicklocal.h's part of the library once, SIGNATURES is applied when the library is first used through
this module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_deflickerlocal_cpu.py checks the table against the
header (tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

ABI_VERSION = 1
MAX_RADIUS, MAX_T, TRACK_INTS = 4, 65535, 8
MAX_SEARCH, MAX_LAM, BLOCKS = 8, 65535, (8, 16)
MV_INTS, NSTAT, NSUM = 4, 6, 12

# every function of include/flicklocal.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvk_abi_version": (I, ()),
    "vvk_last_error": (C.c_char_p, ()),
    "vvk_search": (I, (P, P, P, I, I, I, I, I, I, I, P, P, P)),
    "vvk_hold": (I, (P, P, P, P, P, I, I, I, I, I, I, I, I, P, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("flicklocal.h", "vvk_", ABI_VERSION, "block-matched deflicker", SIGNATURES)
lib, _check = PART.lib, PART.check

_zero_tracks = {}       # (T, device) -> the all-zero, all-tracked track that stands for "no tracker"


def zero_track(T, device):
    """The [T,8] int32 track of a clip nobody tracked (every frame tracked at offset zero), one per (T, device)."""
    key = (int(T), str(device))
    if key not in _zero_tracks:
        track = torch.zeros((int(T), TRACK_INTS), dtype=torch.int32)
        track[:, 3] = 1
        _zero_tracks[key] = track.to(device)
    return _zero_tracks[key]


def blocks(h, w, block):
    """(nby, nbx) of an h x w window cut into block x block pixels."""
    return -(-int(h) // int(block)), -(-int(w) // int(block))


def _clip(what, win, offsets, track):
    if win.dtype != torch.uint8 or win.dim() != 4 or win.shape[3] != 3 or win.shape[0] < 1:
        raise RuntimeError(f"{what}: the pixels must be a [T >= 1, H, W, 3] uint8 tensor")
    T = win.shape[0]
    if offsets.dtype != torch.int32 or tuple(offsets.shape) != (T, 2):
        raise RuntimeError(f"{what}: offsets must be [T, 2] int32")
    if track.dtype != torch.int32 or tuple(track.shape) != (T, TRACK_INTS):
        raise RuntimeError(f"{what}: track must be [T, {TRACK_INTS}] int32")


def _buffer(what, name, buf, shape, dtype, device):
    if buf is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(buf.shape) != tuple(shape) or buf.dtype != dtype or not buf.is_contiguous():
        raise RuntimeError(f"{what}: {name} must be a contiguous {dtype} buffer of shape {tuple(shape)}")
    return buf


def search(win, offsets, track, radius, cfg, mv=None, stats=None):
    """win [T,h,w,3] u8 (flicker_hip.window_pixels), offsets [T,2] int32 (oy, ox), track [T,8] int32 (align_hip.track's records) or None (no
    tracker: the zero track), on the device; cfg: block, search, lam (a deflickerlocal.DeflickerLocalConfig) -> (mv [T,2 radius+1,nby,nbx,4]
    int32, stats [T,2 radius+1,6] int64) on the device (vvk_search): per frame, temporal neighbour and block the displacement whose byte SAD
    plus lam (|dy| + |dx|) is smallest among those that keep the whole block inside the neighbour's window.  mv, stats: optional buffers."""
    if track is None:
        track = zero_track(win.shape[0], win.device)
    hip._need_cuda(win, offsets, track, mv, stats)
    _clip("search", win, offsets, track)
    T, h, w, _ = win.shape
    K = 2 * int(radius) + 1
    if K < 1 or int(cfg.block) not in BLOCKS:
        raise RuntimeError(f"search: radius >= 0 and block in {BLOCKS} are supported, not radius {radius}, block {cfg.block}")
    nby, nbx = blocks(h, w, cfg.block)
    mv = _buffer("search", "mv", mv, (T, K, nby, nbx, MV_INTS), torch.int32, win.device)
    stats = _buffer("search", "stats", stats, (T, K, NSTAT), torch.int64, win.device)
    ncand = (2 * int(cfg.search) + 1) ** 2
    with hip._Prof("flicklocal_search", 3.0 * T * (K - 1) * h * w * ncand, (K + 1) * win.numel() + 4 * mv.numel()):
        _check(lib().vvk_search(hip._p(win), hip._p(offsets), hip._p(track), T, h, w, int(radius), int(cfg.block), int(cfg.search), int(cfg.lam),
                                hip._p(mv), hip._p(stats), hip._stream()), "vvk_search")
    return mv, stats


def hold(win, offsets, track, mv, mask2d, radius, block, tol, out=None, sums=None):
    """win, offsets, track (or None) as for search, mv [T,2 radius+1,nby,nbx,4] int32 (search's; any content is legal), mask2d [T,H0,W0] u8, on
    the device -> (out [T,h,w,3] u8, sums [T,12] int64) on the device (vvk_hold): flickalign_hip.hold's filter with every temporal neighbour
    read at the place its block's record gives, and only where the record's third int is 1.  out (not win), sums: optional buffers."""
    if track is None:
        track = zero_track(win.shape[0], win.device)
    hip._need_cuda(win, offsets, track, mv, mask2d, out, sums)
    _clip("hold", win, offsets, track)
    T, h, w, _ = win.shape
    if mask2d.dtype != torch.uint8 or mask2d.dim() != 3 or mask2d.shape[0] != T:
        raise RuntimeError("hold: mask2d must be [T, H0, W0] uint8")
    K = 2 * int(radius) + 1
    if K < 1 or int(block) not in BLOCKS:
        raise RuntimeError(f"hold: radius >= 0 and block in {BLOCKS} are supported, not radius {radius}, block {block}")
    if mv.dtype != torch.int32 or tuple(mv.shape) != (T, K) + blocks(h, w, block) + (MV_INTS,):
        raise RuntimeError(f"hold: mv must be [T, 2 radius + 1, nby, nbx, {MV_INTS}] int32 = {(T, K) + blocks(h, w, block) + (MV_INTS,)}, not {tuple(mv.shape)}")
    _, H0, W0 = mask2d.shape
    out = hip._out_like("hold", out, win, "win")
    sums = _buffer("hold", "sums", sums, (T, NSUM), torch.int64, win.device)
    with hip._Prof("flicklocal_hold", 0.0, 2 * win.numel() + T * h * w + 4 * mv.numel()):
        _check(lib().vvk_hold(hip._p(win), hip._p(offsets), hip._p(track), hip._p(mv), hip._p(mask2d), T, H0, W0, h, w, int(radius), int(block), int(tol),
                              hip._p(out), hip._p(sums), hip._stream()), "vvk_hold")
    return out, sums
