"""ctypes binding of the clean-plate warp entry points of libvvhip.so (include/platewarp.h; kernels: csrc/vv_platewarp.hip).

Built on hip.py: PART (a hip.Part) declares platewarp.h's part of the library once, SIGNATURES is applied when the library is first used through
this module, and the handle, the device / contiguity checks and the stream are hip's.  tests/test_platewarp_cpu.py checks the table against the
header (tests/abiref.py).  No fallback: a missing symbol or a launcher's error raises RuntimeError.
"""
import ctypes as C

import torch

from . import hip
from .hip import I, P      # the ctypes shorthands of hip.SIGNATURES

L64 = C.c_int64
ABI_VERSION = 1
FRAC_BITS, MAX_SEARCH, MAX_T, MAX_PIXELS = 20, 8, 65535, 1 << 24
TRACK_INTS, REC_INTS, NSTAT, MAP_INTS, BLOCKS = 8, 4, 4, 6, (16, 32)

# every function of include/platewarp.h: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "vvw_abi_version": (I, ()),
    "vvw_last_error": (C.c_char_p, ()),
    "vvw_search": (I, (P, L64, P, I, I, I, I, I, I, I, P, P, P)),
    "vvw_place": (I, (P, P, P, P, I, I, I, I, I, I, I, P, P, P, P)),
    "vvw_unplace": (I, (P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, P, P, P)),
}
EXPORTS = list(SIGNATURES)
PART = hip.Part("platewarp.h", "vvw_", ABI_VERSION, "clean-plate warp", SIGNATURES)
lib, _check = PART.lib, PART.check


def blocks(H, W, block):
    """(nby, nbx): the whole block x block blocks of an H x W plane."""
    return int(H) // int(block), int(W) // int(block)


def tables(maps, device):
    """[T][6] Python integers (platewarp.to_fixed) -> [T,6] int64 on the device."""
    return torch.tensor([[int(v) for v in m] for m in maps], dtype=torch.int64).reshape(-1, MAP_INTS).to(device)


def flags(tracked, device):
    """[T] booleans -> [T] u8 on the device."""
    return torch.tensor([1 if k else 0 for k in tracked], dtype=torch.uint8).to(device)


def _need_maps(what, name, maps, tracked, T):
    if maps.dtype != torch.int64 or tuple(maps.shape) != (T, MAP_INTS):
        raise RuntimeError(f"{what}: {name} must be a [T, {MAP_INTS}] int64 tensor")
    if tracked.dtype != torch.uint8 or tuple(tracked.shape) != (T,):
        raise RuntimeError(f"{what}: tracked must be a [T] uint8 tensor")


def _box(what, box):
    y0, x0, y1, x1 = (int(v) for v in box)
    if y1 - y0 < 1 or x1 - x0 < 1:
        raise RuntimeError(f"{what}: the box is empty")
    return y0, x0, y1 - y0, x1 - x0


def search(pyr, track, H, W, cfg, max_residual):
    """pyr [T, S >= 2 H W] u8 (align_hip.pyramid's packed buffer: the level-0 planes lead every record), track [T,8] int32 (align_hip.track's),
    on the device; cfg: block, search, min_texture (a platewarp.PlateWarpConfig); max_residual = plate_align's -> (rec [T,nby,nbx,4] int32,
    stats [T,4] int64) on the device (vvw_search): per tracked frame and whole block the displacement round off[t] - off[key] whose luma SAD
    against the key is smallest among those that keep the whole block on valid pixels of the key."""
    hip._need_cuda(pyr, track)
    if pyr.dtype != torch.uint8 or pyr.dim() != 2 or pyr.shape[0] < 1:
        raise RuntimeError("search: pyr must be a [T >= 1, S] uint8 tensor")
    T = pyr.shape[0]
    if track.dtype != torch.int32 or tuple(track.shape) != (T, TRACK_INTS):
        raise RuntimeError(f"search: track must be a [T, {TRACK_INTS}] int32 tensor")
    if int(cfg.block) not in BLOCKS:
        raise RuntimeError(f"search: block in {BLOCKS} is supported, not {cfg.block}")
    nby, nbx = blocks(H, W, cfg.block)
    rec = torch.empty((T, nby, nbx, REC_INTS), dtype=torch.int32, device=pyr.device)
    stats = torch.empty((T, NSTAT), dtype=torch.int64, device=pyr.device)
    ncand = (2 * int(cfg.search) + 1) ** 2
    with hip._Prof("platewarp_search", 2.0 * T * nby * nbx * int(cfg.block) ** 2 * ncand, 4 * T * int(H) * int(W)):
        _check(lib().vvw_search(hip._p(pyr), int(pyr.shape[1]), hip._p(track), T, int(H), int(W), int(cfg.block), int(cfg.search), int(cfg.min_texture),
                                int(max_residual), hip._p(rec), hip._p(stats), hip._stream()), "vvw_search")
    return rec, stats


def place(frames, dil, inv, tracked, box, out=None):
    """frames [B,H,W,3] u8, dil [B,H,W] u8, inv [B,6] int64 (canvas -> frame), tracked [B] u8, the canvas box (y0, x0, y1, x1 in canvas
    coordinates) -> (canvas [B,ch,cw,3], dil_c, invalid_c [B,ch,cw]) u8 (vvw_place); out = the rows of a segment's three buffers to write
    instead of new tensors."""
    hip._need_cuda(frames, dil, inv, tracked)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise RuntimeError("place: the frames must be a [B >= 1, H, W, 3] uint8 tensor")
    B, H, W, _ = frames.shape
    if dil.dtype != torch.uint8 or tuple(dil.shape) != (B, H, W):
        raise RuntimeError("place: dil must be a [B, H, W] uint8 tensor of the frames' size")
    _need_maps("place", "inv", inv, tracked, B)
    y0, x0, ch, cw = _box("place", box)
    if out is None:
        out = (torch.empty((B, ch, cw, 3), dtype=torch.uint8, device=frames.device), torch.empty((B, ch, cw), dtype=torch.uint8, device=frames.device),
               torch.empty((B, ch, cw), dtype=torch.uint8, device=frames.device))
    canvas, dil_c, inv_c = out
    hip._need_cuda(canvas, dil_c, inv_c)
    if any(o.dtype != torch.uint8 for o in out) or tuple(canvas.shape) != (B, ch, cw, 3) or tuple(dil_c.shape) != (B, ch, cw) or tuple(inv_c.shape) != (B, ch, cw):
        raise RuntimeError("place: out must be ([B, ch, cw, 3], [B, ch, cw], [B, ch, cw]) uint8 tensors of the box's size")
    with hip._Prof("platewarp_place", 0.0, 9 * B * ch * cw):
        _check(lib().vvw_place(hip._p(frames), hip._p(dil), hip._p(inv), hip._p(tracked), B, H, W, y0, x0, ch, cw, hip._p(canvas), hip._p(dil_c), hip._p(inv_c),
                               hip._stream()), "vvw_place")
    return canvas, dil_c, inv_c


def unplace(canvas, dil_c, dil_out_c, dil, fwd, tracked, box, patch_box):
    """canvas [T,ch,cw,3], dil_c and dil_out_c [T,ch,cw] (the canvas' masks before and after the fill), dil [T,H,W] u8, fwd [T,6] int64
    (frame -> canvas), tracked [T] u8, the canvas box, and patch_box = (y0, x0, y1, x1) inside the frame -> (patch [T,ph,pw,3]: the canvas'
    bytes at the filled pixels, zeros elsewhere; dil' [T,H,W]) (vvw_unplace)."""
    hip._need_cuda(canvas, dil_c, dil_out_c, dil, fwd, tracked)
    if dil.dtype != torch.uint8 or dil.dim() != 3 or dil.shape[0] < 1:
        raise RuntimeError("unplace: dil must be a [T >= 1, H, W] uint8 tensor")
    T, H, W = dil.shape
    y0, x0, ch, cw = _box("unplace", box)
    py0, px0, ph, pw = _box("unplace", patch_box)
    if canvas.dtype != torch.uint8 or tuple(canvas.shape) != (T, ch, cw, 3):
        raise RuntimeError("unplace: canvas must be a [T, ch, cw, 3] uint8 tensor of the box's size")
    for name, m in (("dil_c", dil_c), ("dil_out_c", dil_out_c)):
        if m.dtype != torch.uint8 or tuple(m.shape) != (T, ch, cw):
            raise RuntimeError(f"unplace: {name} must be a [T, ch, cw] uint8 tensor of the box's size")
    _need_maps("unplace", "fwd", fwd, tracked, T)
    patch = torch.empty((T, ph, pw, 3), dtype=torch.uint8, device=dil.device)
    out = torch.empty_like(dil)
    with hip._Prof("platewarp_unplace", 0.0, 2 * T * H * W + 3 * T * ph * pw):
        _check(lib().vvw_unplace(hip._p(canvas), hip._p(dil_c), hip._p(dil_out_c), hip._p(dil), hip._p(fwd), hip._p(tracked), T, H, W, y0, x0, ch, cw, py0, px0,
                                 ph, pw, hip._p(patch), hip._p(out), hip._stream()), "vvw_unplace")
    return patch, out
