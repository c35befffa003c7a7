"""Clean-plate grain on the GPU: vvl_sources of vv_plate.hip against the numpy restatement of include/vvplategrain.h (tests/plategrain_ref.py)
bit for bit -- src, live and r0, then the frames, dil' and the counts vvp_fill makes of live -- each call run twice with identical bytes;
src and r0 against vvp_sources; guard bands, unoccupied tiles and refusals; infill.plate_fill(gcfg=) on the crop and on the canvas; and the
drop-in's plate_grain= path against the same call handed the restatement's frames and masks.  Tiny architecture."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import platealign_ref as A  # noqa: E402
import platefill_ref as R  # noqa: E402
import plategrain_ref as G  # noqa: E402

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.platealign import PlateAlignConfig  # noqa: E402
from videovanish_amd.platefill import PlateFillConfig  # noqa: E402
from videovanish_amd.plategrain import PlateGrainConfig  # noqa: E402
from videovanish_amd.roi import RoiConfig  # noqa: E402
from videovanish_amd.spans import SpanConfig  # noqa: E402

TILE = 64
NONE = G.NONE


def _d(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _twice(fn):
    """fn() -> tensors; run twice, identical bytes; the first run's results as numpy arrays."""
    a, b = fn(), fn()
    a, b = [x.cpu().numpy() for x in a], [x.cpu().numpy() for x in b]
    assert all((x == y).all() for x, y in zip(a, b))
    return a


def _check(frames, dil, gpu, depth, reach, tiles=True, **cfg):
    """One segment through vvp_stats, vvl_sources (twice), the margin and vvp_fill handed live (twice): every output against the restatement,
    src and r0 against vvp_sources too.  Returns the restatement's (frames', dil', counts, detail)."""
    from videovanish_amd import hip, mask_hip, plate_hip, plategrain_hip
    cfg = dict(R.DEFAULTS, **cfg)
    T, H, W = dil.shape
    want_f, want_d, want_c, det = G.fill_segment(frames, dil, depth, reach, **cfg)
    d, f = _d(dil, gpu), _d(frames, gpu)
    occ = hip.mask_tile_union(d, TILE) if tiles else None
    ns = d if cfg["guard"] == 0 else mask_hip.time_bridge_grow(d, 0, cfg["guard"])[0]
    st, n, s1 = plate_hip.stats(f, ns, occ, cfg["min_samples"], cfg["tol"])
    src, live, r0 = _twice(lambda: plategrain_hip.sources(f, d, ns, occ, st, n, s1, cfg["tol"], cfg["outlier"], cfg["max_gap"], depth, reach))
    assert src.dtype == live.dtype == np.int16 and r0.dtype == np.uint8
    src, live = src.view(np.uint16), live.view(np.uint16)
    assert (src == det["src"]).all(), int((src != det["src"]).sum())
    assert (live == det["live"]).all(), int((live != det["live"]).sum())
    assert (r0 == det["r0"]).all()
    p_src, p_r0 = plate_hip.sources(f, d, ns, occ, st, n, s1, cfg["tol"], cfg["outlier"], cfg["max_gap"])
    assert (p_src.cpu().numpy().view(np.uint16) == src).all() and (p_r0.cpu().numpy() == r0).all()        # vvp_sources' bytes
    if depth == 1:
        assert (live == src).all()
    t_live, t_r0 = _d(live.view(np.int16), gpu), _d(r0, gpu)
    keep = t_r0 if cfg["margin"] == 0 else hip.mask_collapse_dilate(t_r0[..., None].contiguous(), cfg["margin"])

    def fill():
        g = f.clone()
        return (g,) + tuple(plate_hip.fill(g, d, keep, occ, t_live))                                  # in place: a live source is unmasked
    got_f, got_d, got_c = _twice(fill)
    assert (got_c == want_c).all() and (got_d == want_d).all() and (got_f == want_f).all()
    return want_f, want_d, want_c, det


def _grain_clip(T, H, W, seed):
    """Pixels of every kind along time: a still with per-pixel noise of amplitude 0 / 3 / 30 and spikes in 2 % of the samples; per pixel one of:
    never masked, masked in all frames but one, a run of T // 6 + 1 masked frames in the middle (more than eight usable frames either side at
    T = 33), masked in every frame, in and out of the mask at random; a box that crosses; any non-zero byte is masked."""
    rng = np.random.default_rng(seed)
    amp = rng.choice([0, 3, 3, 30], (H, W, 1))
    frames = R.background(H, W, seed)[None] + rng.integers(-1, 2, (T, H, W, 3)) * amp
    spike = rng.random((T, H, W, 1)) < 0.02
    frames = np.clip(frames + spike * rng.choice([-22, 22], (T, H, W, 1)), 0, 255).astype(np.uint8)
    kind = rng.integers(0, 5, (H, W))
    t = np.arange(T).reshape(T, 1, 1)
    m = np.zeros((T, H, W), bool)
    m |= (kind == 1)[None] & (t != rng.integers(0, T, (H, W))[None])
    m |= (kind == 2)[None] & (np.abs(2 * t - (T - 1)) <= T // 6)
    m |= (kind == 3)[None]
    m |= (kind == 4)[None] & (rng.random((T, H, W)) < 0.3)
    bw = max(W // 5, 2)
    for i in range(T):
        x0 = -bw // 2 + (i * (W + bw)) // max(T, 1)
        m[i, H // 8: H // 8 + H // 3, max(x0, 0): max(min(x0 + bw, W), 0)] = True
    frames[m] = 255 - frames[m] // 4
    return frames, (m * rng.integers(1, 256, m.shape)).astype(np.uint8)


# ---- the kernel -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(40, 56), (96, 130), (96, 132)])      # smaller than a tile; a remainder tile on the byte form; on the 4-pixel form
@pytest.mark.parametrize("tiles", [True, False])
def test_sources_on_the_locked_off_clip(gpu, H, W, tiles):
    scale = H // 40
    frames, masks, clean, boxm, logom = R.locked_off_clip(24, H, W, speed=2 * W // 56, box=(15 * scale, 16 * W // 56), box_y=4 * scale,
                                                          logo=(26 * scale, 4, 38 * scale, 8))
    out, dil, counts, det = _check(frames, masks, gpu, 4, 8, tiles=tiles)
    assert not dil[boxm].any() and counts[:, 0].sum() == boxm.sum() and (det["live"] != det["src"]).sum() > 1000
    assert np.abs(out[boxm].astype(np.int64) - clean[boxm]).max() <= 6 and (out != det["nearest"]).any()


# depth, reach, max_gap, guard, occ given: every value of the issue's lists, and each depth with a reach that cuts it and one that does not
SETTINGS = [(1, 8, 0, 1, True), (2, 1, 0, 0, True), (2, 65535, 3, 1, False), (4, 8, 0, 1, True), (4, 1, 3, 0, False), (4, 65535, 0, 0, False),
            (8, 8, 3, 1, True), (8, 65535, 0, 1, False), (8, 1, 0, 0, True), (1, 65535, 3, 0, False), (8, 65535, 3, 0, True)]


@pytest.mark.parametrize("T", [1, 2, 9, 33])
def test_sources_settings_on_pixels_of_every_kind(gpu, T):
    for (H, W), seed in (((40, 56), 3), ((33, 50), 4)):                # the 4-pixel form, the byte form
        frames, masks = _grain_clip(T, H, W, seed + T)
        seen = set()
        for depth, reach, max_gap, guard, tiles in SETTINGS:
            out, dil, counts, det = _check(frames, masks, gpu, depth, reach, tiles=tiles, max_gap=max_gap, guard=guard, min_samples=1, margin=0)
            if T == 33:
                cum, side = np.cumsum(det["usable"], 0), det["side"]
                total = cum[-1][None]
                mine, other = np.where(side == -1, cum, total - cum)[side != 0], np.where(side == -1, total - cum, cum)[side != 0]
                seen |= set(np.minimum(mine, 9).tolist()) | ({0} if (other == 0).any() else set())
                if depth > 1:
                    assert (det["live"] != det["src"]).sum() > 100 and det["m"].max() > 1
        if T == 33:
            assert {0, 1, 2, 8, 9} <= seen, seen                    # usable frames on a side: none, one, some, more than eight
    if T == 33:
        frames, masks = _grain_clip(T, 96, 130, 9)                     # several blocks, a remainder tile, the byte form
        _check(frames, masks, gpu, 8, 65535, max_gap=0, guard=0, min_samples=1)
        frames, masks = _grain_clip(T, 96, 132, 10)
        _check(frames, masks, gpu, 4, 8, max_gap=3, guard=1, min_samples=1)


def test_sources_on_the_hand_made_pixel_table(gpu):
    frames, masks, us = G.table_clip()
    for rep in (1, 2):                                                 # W = 10: the byte form; W = 20: the 4-pixel form
        f, m = np.tile(frames, (1, 1, rep, 1)), np.tile(masks, (1, 1, rep))
        for depth, reach, max_gap in ((4, 8, 0), (1, 8, 0), (4, 3, 0), (4, 8, 4), (8, 65535, 0), (2, 1, 2), (8, 65535, 7)):
            out, dil, counts, det = _check(f, m, gpu, depth, reach, tiles=rep == 1, **dict(G.TABLE_CFG, max_gap=max_gap))
            assert (det["usable"][:, :, :10] == us).all()


def test_guard_bands_unoccupied_tiles_and_unaligned_outputs(gpu):
    """The launcher's own buffers: src, live and r0 inside poisoned buffers with bands either side; a clip of 2 x 3 tiles with masks in one tile
    only (every other tile keeps the launcher's values and its image bytes are never read); outputs at an odd offset take the byte form."""
    from videovanish_amd import hip, mask_hip, plate_hip, plategrain_hip
    lib = plategrain_hip.lib()
    frames, masks, clean, boxm, logom = R.locked_off_clip(24, 100, 180, speed=5, box=(15, 16), box_y=20, logo=(50, 70, 60, 76))
    masks[:, :, :64] = 0
    masks[:, :, 128:] = 0
    masks[:, 64:] = 0
    T, H, W = masks.shape
    want_f, want_d, want_c, det = G.fill_segment(frames, masks, 4, 8)
    assert (det["live"] != det["src"]).sum() > 100
    up = frames.copy()
    up[:, :, :64] = up[:, :, 128:] = 77                                # no image byte outside the occupied tile is read
    up[:, 64:] = 99
    d, f = _d(masks, gpu), _d(up, gpu)
    occ = hip.mask_tile_union(d, TILE)
    assert occ.cpu().numpy().tolist() == [[0, 1, 0], [0, 0, 0]]
    ns = mask_hip.time_bridge_grow(d, 0, 1)[0]
    st, n, s1 = plate_hip.stats(f, ns, occ, 4, 6)
    N, BAND = T * H * W, 4096
    p = lambda t: t.data_ptr()
    for shift in (0, 1):                                               # 1: src and live at an address that is no multiple of 8
        bs = torch.full((N + 2 * BAND,), 0x5A5A, dtype=torch.int16, device=gpu)
        bl = torch.full((N + 2 * BAND,), 0x5A5A, dtype=torch.int16, device=gpu)
        br = torch.full((N + 2 * BAND,), 0x5A, dtype=torch.uint8, device=gpu)
        o = BAND + shift
        rc = lib.vvl_sources(p(f), p(d), p(ns), p(occ), p(st), p(n), p(s1), T, H, W, TILE, 6, 3, 0, 4, 8, p(bs[o:]), p(bl[o:]), p(br[o:]), None)
        assert rc == 0
        torch.cuda.synchronize()
        for buf, want, poison in ((bs, det["src"].view(np.int16), 0x5A5A), (bl, det["live"].view(np.int16), 0x5A5A), (br, det["r0"], 0x5A)):
            got = buf.cpu().numpy()
            assert (got[:o] == poison).all() and (got[o + N:] == poison).all()
            assert (got[o:o + N].reshape(T, H, W) == want).all()
        assert (bl.cpu().numpy()[o:o + N].reshape(T, H, W)[:, :, :64] == -1).all()                     # unoccupied: the launcher's NO_SOURCE


def test_refusals_launch_nothing(gpu):
    from videovanish_amd import plategrain_hip
    lib = plategrain_hip.lib()
    f = torch.full((2, 8, 8, 3), 7, dtype=torch.uint8, device=gpu)
    m = torch.full((2, 8, 8), 7, dtype=torch.uint8, device=gpu)
    w = torch.full((2, 8, 8, 3), 7, dtype=torch.int32, device=gpu)
    s = torch.full((2, 8, 8), 7, dtype=torch.int16, device=gpu)
    l = torch.full((2, 8, 8), 7, dtype=torch.int16, device=gpu)
    p = lambda t: t.data_ptr()
    call = lambda T=2, tol=6, outlier=3, max_gap=0, depth=4, reach=8, live=p(l), occ=None, tile=64: lib.vvl_sources(
        p(f), p(m), p(m), occ, p(m), p(w), p(w), T, 8, 8, tile, tol, outlier, max_gap, depth, reach, p(s), live, p(m), None)
    bad = [call(T=0), call(tol=-1), call(outlier=-1), call(max_gap=-1), call(depth=0), call(reach=0), call(live=None), call(occ=p(m), tile=0)]
    assert bad == [-1] * len(bad) and lib.vvl_last_error().startswith(b"vvl_sources:")
    unsupported = [call(T=65536), call(tol=256), call(outlier=65), call(max_gap=65536), call(reach=65536), call(depth=9)]
    assert unsupported == [-2] * len(unsupported) and lib.vvl_last_error().startswith(b"vvl_sources:") and b"depth 9" in lib.vvl_last_error()
    torch.cuda.synchronize()
    assert (f == 7).all() and (m == 7).all() and (w == 7).all() and (s == 7).all() and (l == 7).all()   # nothing was launched, nothing cleared
    with pytest.raises(RuntimeError, match="depth <= 8"):
        plategrain_hip.sources(f, m, m, None, m[0].contiguous(), w[0, :, :, 0].contiguous(), w[0].contiguous(), 6, 3, 0, 9, 8)
    with pytest.raises(RuntimeError):
        plategrain_hip.sources(f.cpu(), m.cpu(), m.cpu(), None, m[0].cpu(), w[0, :, :, 0].cpu(), w[0].cpu(), 6, 3, 0, 4, 8)      # no CPU fallback
    with pytest.raises(ctypes.ArgumentError):
        call(depth=2.0)


# ---- infill.plate_fill(gcfg=) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", [None, [9, 15]])
def test_plate_fill_with_grain_on_the_crop(gpu, cuts):
    from videovanish_amd import infill
    frames, masks, clean, boxm, logom = R.locked_off_clip(24, 96, 130, speed=4, box=(30, 37), box_y=8, logo=(52, 6, 76, 11))
    flist = [f.copy() for f in frames]
    d = _d(masks, gpu)
    for gcfg, pkw in ((PlateGrainConfig(), {}), (PlateGrainConfig(depth=8, reach=3), dict(guard=0, margin=0, max_gap=3))):
        got = []
        out, dil, rep = infill.plate_fill(flist, d, PlateFillConfig(**pkw), cuts, gcfg=gcfg, grain_out=got)
        want, wd, wc, wrot = G.plate_fill(frames, masks, cuts, gcfg.depth, gcfg.reach, **dict(R.DEFAULTS, **pkw))
        assert (np.stack(out) == want).all() and (dil.cpu().numpy() == wd).all()
        assert (rep.filled == wc[:, 0]).all() and (rep.left == wc[:, 1]).all() and (got[0].rotated == wrot).all() and (got[0].filled == wc[:, 0]).all()
        assert wrot.sum() > 0 and all((out[i] is flist[i]) == (wc[i, 0] == 0) for i in range(24))
        assert all((a == b).all() for a, b in zip(flist, frames)) and (d.cpu().numpy() == masks).all()      # the caller's arrays are never written
    base, bd, brep = infill.plate_fill(flist, d, PlateFillConfig(), cuts)
    got = []
    out, dil, rep = infill.plate_fill(flist, d, PlateFillConfig(), cuts, gcfg=PlateGrainConfig(depth=1), grain_out=got)
    assert (np.stack(out) == np.stack(base)).all() and (dil.cpu().numpy() == bd.cpu().numpy()).all() and not got[0].rotated.any()


def test_plate_fill_with_grain_on_the_canvas(gpu):
    from videovanish_amd import infill
    frames, masks, off, clean, boxm, logom = A.pan_clip(H=45, W=83, seed=1, noise=3, steps_x=(3, 3), steps_y=(0, 0), **A.STAGE_CLIPS[45, 83])
    flist = [f.copy() for f in frames]
    d, got, agot = _d(masks, gpu), [], []
    out, dil, rep = infill.plate_fill(flist, d, PlateFillConfig(), None, acfg=PlateAlignConfig(), align_out=agot, gcfg=PlateGrainConfig(), grain_out=got)
    want, wd, wc, wrot = G.fill_on_canvas(frames, masks)
    assert agot[0].path == ("canvas",) and (agot[0].off[0] == off).all()
    assert (np.stack(out) == want).all() and (dil.cpu().numpy() == wd).all() and (rep.filled == wc[:, 0]).all() and (got[0].rotated == wrot).all()
    near = A.plate_fill(frames, masks)
    assert wrot.sum() > 100 and (wd == near[1]).all() and (wc == near[2]).all() and (want != near[0]).any()


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=960, num_inference_steps=2, scheduler="ddim")
T, H, W = 14, 96, 160
SPANS = SpanConfig("masked", context=1, min_len=3, min_gap=2)
ROI = RoiConfig("follow", context=0.25, pad_min=8, min_side=32)
SCREEN = (64, 96, 88, 136)        # a screen-fixed region that shows something else in every frame: never steady
LOGO = (70, 104, 80, 124)         # a mask on it in frames 4 .. 8


def _finish(frames, masks):
    rng = np.random.default_rng(77)
    y0, x0, y1, x1 = SCREEN
    frames[:, y0:y1, x0:x1] = rng.integers(0, 256, (T, y1 - y0, x1 - x0, 3))
    masks[4:9, LOGO[0]:LOGO[2], LOGO[1]:LOGO[3]] = 255
    m3 = [np.repeat(m[..., None], 3, axis=2) for m in masks]
    prior = []
    for f, m in zip(frames, masks):
        p = f.copy()
        p[m > 0] = f.reshape(-1, 3).mean(0).astype(np.uint8)
        prior.append(p)
    return list(frames), m3, prior


@pytest.fixture(scope="module")
def still_clip():          # section 16's
    frames, masks, clean, boxm, _ = R.locked_off_clip(T, H, W, a=3, seed=5, speed=12, box=(22, 24), box_y=20, logo=None)
    return _finish(frames, masks)


@pytest.fixture(scope="module")
def pan_clip():            # section 17's, with grain
    frames, masks, off, clean, boxm, _ = A.pan_clip(T=T, H=H, W=W, seed=5, noise=3, steps_x=(3, 3), steps_y=(0, 0), box=(22, 24), box_speed=-12)
    return _finish(frames, masks)


def _run(frames, masks, prior, **kw):
    import diffuerase
    diffuerase.configure(RUN)
    try:
        out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, feather_px=3, **KW, **kw)
        return out, diffuerase.last_plate_fill, diffuerase.last_plate_grain
    finally:
        diffuerase.configure(None)


def _same(a, b):
    return len(a) == len(b) == T and (np.stack(a) == np.stack(b)).all()


def _by_hand(monkeypatch, gpu, want_f, want_d, frames, reports):
    """infill.plate_fill replaced by a stand-in that hands over the restatement's frames and masks."""
    from videovanish_amd import infill
    empty = infill.PlateFillReport(np.zeros(T, np.int64), np.zeros(T, np.int64), (0,), (False,), ((0, T),), ())

    def stand_in(f, d, cfg, cuts=None, acfg=None, align_out=None, gcfg=None, grain_out=None):
        assert gcfg == PlateGrainConfig()
        grain_out.append(reports[0])
        if align_out is not None:
            align_out.append(reports[1])
        return [want_f[i] if (want_f[i] != frames[i]).any() else frames[i] for i in range(T)], _d(want_d, gpu), empty
    monkeypatch.setattr(infill, "plate_fill", stand_in)


@pytest.mark.parametrize("more", [{}, dict(spans=SPANS, roi=ROI)], ids=["plain", "spans-roi"])
def test_drop_in_equals_the_call_on_the_restatement(gpu, still_clip, monkeypatch, more):
    from videovanish_amd import hip
    frames, masks, prior = still_clip
    dil = hip.mask_collapse_dilate(_d(np.stack(masks), gpu), KW["mask_dilation_iter"]).cpu().numpy()
    want_f, want_d, want_c, want_rot = G.plate_fill(np.stack(frames), dil)
    near = R.plate_fill(np.stack(frames), dil)
    assert want_rot.sum() > 1000 and (want_f != near[0]).any() and (want_d == near[1]).all()
    kept = [f.copy() for f in frames]
    out, rep, grep = _run(frames, masks, prior, plate_fill="on", plate_grain="on", **more)
    assert (rep.filled == want_c[:, 0]).all() and (rep.left == want_c[:, 1]).all() and rep.skipped == (False,)
    assert (grep.rotated == want_rot).all() and (grep.filled == want_c[:, 0]).all() and grep.segments == ((0, T),)
    assert all((a == b).all() for a, b in zip(frames, kept))
    _by_hand(monkeypatch, gpu, want_f, want_d, frames, (grep,))
    hand, _, _ = _run(frames, masks, prior, plate_fill="on", plate_grain="on", **more)
    assert _same(out, hand)
    monkeypatch.undo()
    if more:
        filled = (dil != 0) & (want_d == 0)
        assert all((out[t] == want_f[t]).all() for t in (0, 1, 11, 12, 13)) and not (out[6] == want_f[6]).all()
        assert all((out[t][filled[t]] == want_f[t][filled[t]]).all() for t in range(T))
    else:
        # depth = 1: the bytes of plate_fill alone, and plategrain_hip stays unresolved
        from videovanish_amd import plategrain_hip
        monkeypatch.setattr(plategrain_hip.PART, "dll", None)
        one, rep1, grep1 = _run(frames, masks, prior, plate_fill="on", plate_grain="depth=1")
        assert plategrain_hip.PART.dll is None and not grep1.rotated.any() and (grep1.filled == rep1.filled).all()
        alone, rep0, none = _run(frames, masks, prior, plate_fill="on")
        assert none is None and _same(one, alone) and not _same(out, alone)
        assert all((a == b).all() if isinstance(a, np.ndarray) else a == b for a, b in zip(rep0, rep1))
        with pytest.raises(ValueError, match="plate_grain="):
            _run(frames, masks, prior, plate_grain="on")


def test_drop_in_on_the_canvas_equals_the_call_on_the_restatement(gpu, pan_clip, monkeypatch):
    import diffuerase
    from videovanish_amd import hip
    frames, masks, prior = pan_clip
    dil = hip.mask_collapse_dilate(_d(np.stack(masks), gpu), KW["mask_dilation_iter"]).cpu().numpy()
    want_f, want_d, want_c, want_rot = G.fill_on_canvas(np.stack(frames), dil)
    near = A.plate_fill(np.stack(frames), dil)
    assert want_rot.sum() > 1000 and (want_f != near[0]).any() and (want_d == near[1]).all() and (want_c == near[2]).all()
    out, rep, grep = _run(frames, masks, prior, plate_fill="on", plate_align="on", plate_grain="on")
    arep = diffuerase.last_plate_align
    assert arep.path == ("canvas",) and arep.tracked[0].all()
    assert (rep.filled == want_c[:, 0]).all() and (rep.left == want_c[:, 1]).all() and (grep.rotated == want_rot).all()
    _by_hand(monkeypatch, gpu, want_f, want_d, frames, (grep, arep))
    hand, _, _ = _run(frames, masks, prior, plate_fill="on", plate_align="on", plate_grain="on")
    assert _same(out, hand)
