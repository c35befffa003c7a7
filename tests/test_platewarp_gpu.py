"""Clean-plate warp on the GPU: the entry points of vv_platewarp.hip against the numpy restatement of include/platewarp.h
(tests/platewarp_ref.py) bit for bit, each run twice with identical bytes; infill.plate_fill(acfg=, wcfg=) on the synthetic clip with pan, zoom
and roll; and the drop-in's plate_warp= path against the same call handed the restatement's frames and masks.  Tiny architecture."""
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
import platewarp_ref as WR  # noqa: E402

from videovanish_amd import platewarp as PW  # noqa: E402
from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.platealign import PlateAlignConfig  # noqa: E402
from videovanish_amd.platefill import PlateFillConfig  # noqa: E402
from videovanish_amd.plategrain import PlateGrainConfig  # noqa: E402
from videovanish_amd.platewarp import PlateWarpConfig  # noqa: E402
from videovanish_amd.roi import RoiConfig  # noqa: E402
from videovanish_amd.spans import SpanConfig  # noqa: E402

SIZES = [(40, 56), (45, 83), (96, 130), (96, 132), (12, 40)]    # few blocks; odd, dropped edge blocks; the pyramid's byte and 4-pixel paths; no block


def _d(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _twice(fn):
    """fn() -> tensors; run twice, identical bytes; the first run's results as numpy arrays."""
    a, b = fn(), fn()
    a, b = [x.cpu().numpy() for x in a], [x.cpu().numpy() for x in b]
    assert all((x == y).all() for x, y in zip(a, b))
    return a


# ---- vvw_search -----------------------------------------------------------------------------------------------------------------------------
def _search_clip(H, W, seed, T=7):
    """A smooth texture panning by integer steps plus +-2 levels of noise; a mask through blocks of every frame (the key's too) and speckles; and
    a track written by hand: offsets a few pixels off the true ones (so that winners are not zero), a key change at frame 4, an untracked
    frame, a d0 that pushes most candidates off the key's plane, and one that leaves it altogether."""
    rng = np.random.default_rng(seed)
    step = np.array([3, 1])
    wide = np.clip((A.smooth(rng.integers(0, 256, (H + 40, W + 60, 3)), 1) - 128) * 3 + 128, 0, 255)
    frames = np.stack([wide[8 + step[1] * t: 8 + step[1] * t + H, 8 + step[0] * t: 8 + step[0] * t + W] for t in range(T)]) + rng.integers(-2, 3, (T, H, W, 3))
    frames = np.clip(frames, 0, 255).astype(np.uint8)
    m = rng.random((T, H, W)) < 0.002
    m[:, H // 3: H // 3 + 9, W // 5: W // 5 + 11] = True
    masks = (m * rng.integers(1, 256, m.shape)).astype(np.uint8)
    track = np.zeros((T, 8), np.int32)
    track[:, 3] = 1
    for t in range(T):
        track[t, :2] = step * t + rng.integers(-3, 4, 2)
        track[t, 2] = 0 if t <= 4 else 4
        track[t, 4:] = rng.integers(-5, 6, 4)                                                         # the other ints of a record are not read
    track[0, :3] = 0
    track[2, 3] = 0                                                                                   # untracked
    track[3, :2] += (W - 20, 0)                                                                       # most candidates leave the key's plane
    track[6, :2] = (1 << 20, -(1 << 20))                                                              # all of them do
    return frames, masks, track


@pytest.mark.parametrize("H,W", SIZES)
def test_search(gpu, H, W):
    from videovanish_amd import align_hip, platewarp_bind as B
    frames, masks, track = _search_clip(H, W, H * 7 + W)
    f, d, tr = _d(frames, gpu), _d(masks, gpu), _d(track, gpu)
    L = 1 if min(H, W) >= 32 else 0                                                                   # L = 1: a record longer than its level 0
    pyr = align_hip.pyramid(f, d, L)
    Y, V = A.pyramid(frames, masks, 0)[0]
    some = 0
    for block in (16, 32):
        for search in (0, 1, 8):
            for min_texture, max_residual in ((2, 12), (0, 255)):
                cfg = PlateWarpConfig(block=block, search=search, min_texture=min_texture)
                want, wstats = WR.search(Y, V, track, block, search, min_texture, max_residual)
                rec, stats = _twice(lambda: B.search(pyr, tr, H, W, cfg, max_residual))
                assert rec.shape == want.shape == (7, H // block, W // block, 4) and rec.dtype == np.int32 and stats.dtype == np.int64
                assert (rec == want).all() and (stats == wstats).all(), (block, search, min_texture, int((rec != want).sum()))
                assert not rec[0].any() and not rec[2].any() and not rec[6].any()                     # its own key; untracked; off the key's plane
                some += int(rec[..., 2].sum())
    assert (some > 0) == (H >= 16)                                                                    # the cases are not vacuous; below one block nothing is written


def test_search_on_constant_grey_and_through_a_pyramid_in_batches(gpu):
    from videovanish_amd import align_hip, platewarp_bind as B
    H, W, T = 48, 80, 3
    frames, masks = np.full((T, H, W, 3), 90, np.uint8), np.zeros((T, H, W), np.uint8)
    track = np.zeros((T, 8), np.int32)
    track[:, 3] = 1
    pyr = torch.empty((T, align_hip.frame_bytes(H, W, 2)), dtype=torch.uint8, device=gpu)
    for b in range(T):                                                                                # in batches into the rows of one buffer, as the host does
        align_hip.pyramid(_d(frames[b:b + 1], gpu), _d(masks[b:b + 1], gpu), 2, out=pyr[b:b + 1])
    rec, stats = _twice(lambda: B.search(pyr, _d(track, gpu), H, W, PlateWarpConfig(min_texture=0), 12))
    assert (rec[1:] == [0, 0, 1, 0]).all() and not rec[0].any() and stats.tolist() == [[0] * 4, [15, 15, 0, 0], [15, 15, 0, 0]]     # the tie order gives (0, 0)
    rec, stats = _twice(lambda: B.search(pyr, _d(track, gpu), H, W, PlateWarpConfig(), 12))
    assert not rec.any() and not stats.any()                                                          # min_texture: a flat block is not matched at all


# ---- vvw_place / vvw_unplace ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def warp():
    frames, masks, truth, maps = WR.warp_clip()
    return frames, masks, truth, WR.fill_segment(frames, masks)


def _place_unplace(gpu, frames, masks, fwd, inv, tracked, box, pbox, d2_of):
    """Both kernels against the restatement; d2_of(dil_c) = the canvas' masks after a fill.  -> (canvas, dil_c, inv_c, patch, dil_out)."""
    from videovanish_amd import platewarp_bind as B
    f, d = _d(frames, gpu), _d(masks, gpu)
    it, ft, fl = B.tables(inv, gpu), B.tables(fwd, gpu), B.flags(tracked, gpu)
    want = WR.place(frames, masks, inv, tracked, box)
    got = _twice(lambda: B.place(f, d, it, fl, box))
    assert all(g.dtype == np.uint8 and g.shape == w.shape and (g == w).all() for g, w in zip(got, want))
    T = len(frames)
    out = tuple(torch.full_like(_d(w, gpu), 7) for w in want)                                         # in batches into the rows of the segment's buffers
    for b in range(0, T, 5):
        B.place(f[b:b + 5], d[b:b + 5], it[b:b + 5], fl[b:b + 5], box, out=tuple(o[b:b + 5] for o in out))
    assert all((o.cpu().numpy() == w).all() for o, w in zip(out, want))
    d2 = d2_of(want[1])
    wp, wd = WR.unplace(want[0], want[1], d2, masks, fwd, tracked, box, pbox)
    patch, dout = _twice(lambda: B.unplace(out[0], out[1], _d(d2, gpu), d, ft, fl, box, pbox))
    assert patch.shape == wp.shape and (patch == wp).all() and (dout == wd).all()
    return want + (wp, wd)


def test_place_and_unplace_with_the_fitted_tables(gpu, warp):
    frames, masks, truth, (_, _, _, info) = warp
    plan, box = info["plan"], info["wbox"]
    assert info["warp"] == "warp" and box[1] < 0                                                      # a canvas box with a negative origin
    pbox = WR.patch_box(WR.mask_boxes(masks), 96, 128)
    rng = np.random.default_rng(3)
    canvas, dil_c, inv_c, patch, dout = _place_unplace(gpu, frames, masks, plan.fwd, plan.inv, plan.tracked, box, pbox,
                                                       lambda dc: np.where(rng.random(dc.shape) < 0.5, 0, dc).astype(np.uint8))
    went = (masks != 0) & (dout == 0)
    assert went.any() and (inv_c == 255).any() and (inv_c == 0).any() and patch.any()


def test_integer_translation_tables_give_the_trackers_canvas(gpu):
    """vvw_place and vvw_unplace with integer-translation tables: the bytes of vva_place_masks, of the host's slices and of vva_unplace_mask."""
    from videovanish_amd import align_hip, platealign
    frames, masks, off, _, _, _ = A.stage_clip(45, 83)
    T = len(frames)
    track = np.zeros((T, 8), np.int32)
    track[:, 3] = 1
    track[:, 0], track[:, 1] = off[:, 0], off[:, 1] + np.arange(T) % 3 - 1
    track[5, 3] = 0                                                                                   # a lost frame
    ok = track[:, 3] == 1
    box = A.canvas_box(masks, track)
    fwd, inv = [PW.translation_table(r[0], r[1]) for r in track], [PW.translation_table(-r[0], -r[1]) for r in track]
    canvas, dil_c, inv_c, patch, dout = _place_unplace(gpu, frames, masks, fwd, inv, ok, box, (0, 0, 45, 83),
                                                       lambda dc: np.where(np.arange(dc.shape[1])[None, :, None] % 2 == 0, 0, dc).astype(np.uint8))
    d, tr = _d(masks, gpu), _d(track, gpu)
    ad, ai = align_hip.place_masks(d, tr, box)
    assert (ad.cpu().numpy() == dil_c).all() and (ai.cpu().numpy() == inv_c).all()
    host = np.zeros_like(canvas)
    for t in range(T):                                                                                # the host's slices of infill._fill_on_canvas
        sl = platealign.frame_slices(box, track[t, :2], 45, 83) if ok[t] else None
        if sl is not None:
            host[t][sl[0]] = frames[t][sl[1]]
    assert (host == canvas).all()
    d2 = np.where(np.arange(dil_c.shape[1])[None, :, None] % 2 == 0, 0, dil_c).astype(np.uint8)
    assert (align_hip.unplace_mask(_d(d2, gpu), d, tr, box).cpu().numpy() == dout).all()
    went = (masks != 0) & (dout == 0)
    assert went.any() and (patch[went] == frames[went]).all()


def test_tables_that_map_outside_read_nothing(gpu):
    """Maps are data: tables that lead wholly or partly outside the frame or the canvas, and products that leave 64 bits, only ever give
    invalid_c = 255 and zeros there; this exercises the bounds tests and must run clean."""
    rng = np.random.default_rng(9)
    T, H, W = 6, 40, 56
    frames = rng.integers(1, 256, (T, H, W, 3)).astype(np.uint8)
    masks = (rng.random((T, H, W)) < 0.4).astype(np.uint8) * 255
    one = 1 << 20
    tabs = [PW.translation_table(1000, -1000),                                                        # wholly outside
            PW.translation_table(-30, 20),                                                            # partly
            (5 * one, 3 * one, 0, -2 * one, 0, 3 * one),                                              # a zoom of 3: most of it outside
            (1 << 62, 1 << 62, 1 << 61, -(1 << 62), 1 << 63 - 1, 1 << 60),                            # sums that wrap
            (-(1 << 63), 0, 0, (1 << 63) - 1, 0, 0),                                                  # the extremes
            PW.translation_table(0, 0)]
    tracked = [True] * T
    box = (-7, -12, 41, 60)
    canvas, dil_c, inv_c, patch, dout = _place_unplace(gpu, frames, masks, tabs, tabs, tracked, box, (3, 4, 39, 52), lambda dc: np.zeros_like(dc))
    assert (inv_c[0] == 255).all() and not canvas[0].any() and not dil_c[0].any() and (dout[0] == masks[0]).all() and not patch[0].any()
    assert (inv_c[1] == 255).any() and (inv_c[1] == 0).any() and (inv_c[5, 7:47, 12:68] == 0).all()
    assert (canvas[inv_c == 255] == 0).all() and (dil_c[inv_c == 255] == 0).all()
    assert (dout[5] == 0).all() and (patch[5] == frames[5, 3:39, 4:52] * (masks[5, 3:39, 4:52, None] != 0)).all()


def test_refusals_launch_nothing(gpu):
    from videovanish_amd import platewarp_bind as B
    lib = B.lib()
    H = W = 32
    pyr = torch.full((2, 2 * H * W), 7, dtype=torch.uint8, device=gpu)
    tr = torch.full((2, 8), 7, dtype=torch.int32, device=gpu)
    rec = torch.full((2, 2, 2, 4), 7, dtype=torch.int32, device=gpu)
    st = torch.full((2, 4), 7, dtype=torch.int64, device=gpu)
    f = torch.full((2, H, W, 3), 7, dtype=torch.uint8, device=gpu)
    m = torch.full((2, H, W), 7, dtype=torch.uint8, device=gpu)
    m2 = torch.full((2, H, W), 7, dtype=torch.uint8, device=gpu)
    maps = torch.full((2, 6), 7, dtype=torch.int64, device=gpu)
    fl = torch.full((2,), 7, dtype=torch.uint8, device=gpu)
    p = lambda t: t.data_ptr()
    bad = [lib.vvw_search(p(pyr), 2 * H * W, p(tr), 0, H, W, 16, 4, 2, 12, p(rec), p(st), None), lib.vvw_search(p(pyr), 2 * H * W, None, 2, H, W, 16, 4, 2, 12, p(rec), p(st), None),
           lib.vvw_search(p(pyr), 2 * H * W, p(tr), 2, H, W, 16, -1, 2, 12, p(rec), p(st), None),
           lib.vvw_place(p(f), p(m), p(maps), p(fl), 2, H, W, 0, 0, 0, W, p(f), p(m2), p(m2), None), lib.vvw_place(p(f), None, p(maps), p(fl), 2, H, W, 0, 0, H, W, p(f), p(m2), p(m2), None),
           lib.vvw_unplace(p(f), p(m), p(m), p(m), p(maps), p(fl), 2, H, W, 0, 0, H, W, 0, 0, H, W, p(f), p(m), None),
           lib.vvw_unplace(p(f), p(m), p(m), p(m), p(maps), p(fl), 2, H, W, 0, 0, H, W, 1, 0, H, W, p(f), p(m2), None)]
    assert bad == [-1] * len(bad) and b"vvw_unplace" in lib.vvw_last_error()
    unsupported = [lib.vvw_search(p(pyr), 2 * H * W, p(tr), 2, H, W, 8, 4, 2, 12, p(rec), p(st), None), lib.vvw_search(p(pyr), 2 * H * W, p(tr), 2, H, W, 16, 9, 2, 12, p(rec), p(st), None),
                   lib.vvw_search(p(pyr), 2 * H * W - 1, p(tr), 2, H, W, 16, 4, 2, 12, p(rec), p(st), None),
                   lib.vvw_place(p(f), p(m), p(maps), p(fl), 65536, H, W, 0, 0, H, W, p(f), p(m2), p(m2), None),
                   lib.vvw_unplace(p(f), p(m), p(m), p(m), p(maps), p(fl), 65536, H, W, 0, 0, H, W, 0, 0, H, W, p(f), p(m2), None)]
    assert unsupported == [-2] * len(unsupported) and b"65536" in lib.vvw_last_error()
    torch.cuda.synchronize()
    for t in (pyr, tr, rec, st, f, m, m2, maps, fl):
        assert (t == 7).all()                                                                         # nothing was launched, nothing cleared
    with pytest.raises(RuntimeError, match="search <= 8"):
        lib_cfg = type("C", (), dict(block=16, search=9, min_texture=2))
        B.search(pyr, tr, H, W, lib_cfg, 12)
    with pytest.raises(RuntimeError):
        B.place(f.cpu(), m.cpu(), maps.cpu(), fl.cpu(), (0, 0, H, W))                                 # no CPU fallback
    with pytest.raises(ctypes.ArgumentError):
        lib.vvw_search(p(pyr), 2 * H * W, p(tr), 2.0, H, W, 16, 4, 2, 12, p(rec), p(st), None)


# ---- infill.plate_fill(acfg=, wcfg=) --------------------------------------------------------------------------------------------------------
def _stage(gpu, frames, masks, pcfg=PlateFillConfig(), acfg=PlateAlignConfig(), wcfg=PlateWarpConfig(), cuts=None, **more):
    from videovanish_amd import infill
    flist = [f.copy() for f in frames]
    d, got, gota = _d(masks, gpu), [], []
    kw = dict(wcfg=wcfg, warp_out=got) if wcfg is not None else {}
    out, dil, rep = infill.plate_fill(flist, d, pcfg, cuts, acfg=acfg, align_out=gota, **kw, **more)
    assert all((a == b).all() for a, b in zip(flist, frames)) and (d.cpu().numpy() == masks).all()          # the caller's arrays are never written
    return flist, d, out, dil, rep, gota[0], got[0] if got else None


def test_stage_on_the_synthetic_clip_equals_the_restatement(gpu, warp):
    frames, masks, truth, (want, wd, wc, info) = warp
    T = len(frames)
    flist, d, out, dil, rep, arep, wrep = _stage(gpu, frames, masks)
    assert arep.path == ("canvas",) and wrep.path == ("warp",) and wrep.box == (info["wbox"],) and wrep.segments == ((0, T),)
    assert (np.stack(out) == want).all() and (dil.cpu().numpy() == wd).all() and (rep.filled == wc[:, 0]).all() and (rep.left == wc[:, 1]).all()
    assert all((out[i] is flist[i]) == (wc[i, 0] == 0) for i in range(T)) and rep.filled.sum() > 0 and dil is not d
    plan = info["plan"]
    assert (wrep.usable[0] == info["stats"][:, 0]).all() and (wrep.used[0] == info["stats"][:, 1]).all()
    assert wrep.kept[0].tolist() == [len(f.kept) if f is not None else 0 for f in plan.fits] and not wrep.failed[0].any() and wrep.kept[0][1:].min() >= 12
    assert np.allclose(wrep.maps[0], [[float(v) for r in m for v in r] for m in plan.maps], rtol=0, atol=1e-12) and 0 < wrep.rms[0].max() < 1
    # more than plate_align alone, which is the call without the option
    _, _, out1, dil1, rep1, arep1, none = _stage(gpu, frames, masks, wcfg=None)
    want1, wd1, wc1, _ = A.plate_fill(frames, masks)
    assert none is None and (np.stack(out1) == want1).all() and (rep1.filled == wc1[:, 0]).all() and rep.filled.sum() > rep1.filled.sum()
    # plate_grain on the warp canvas fills the same pixels
    got = []
    _, _, outg, dilg, repg, _, wrepg = _stage(gpu, frames, masks, gcfg=PlateGrainConfig(), grain_out=got)
    assert wrepg.path == ("warp",) and (dilg.cpu().numpy() == wd).all() and (repg.filled == rep.filled).all() and (got[0].filled == rep.filled).all()
    assert got[0].rotated.sum() > 0 and not (np.stack(outg) == want).all() and (np.stack(outg)[wd != 0] == frames[wd != 0]).all()
    # a canvas over max_bytes falls back to plate_align's path and is flagged
    full = PW.canvas_bytes(T, info["wbox"])
    abox = A.canvas_box(masks, info["track"])
    assert PW.canvas_bytes(T, abox) < full
    _, _, outf, dilf, repf, arepf, wrepf = _stage(gpu, frames, masks, pcfg=PlateFillConfig(max_bytes=full - 1))
    assert arepf.path == ("canvas",) and wrepf.path == ("fallback",) and (np.stack(outf) == want1).all() and (repf.filled == rep1.filled).all()
    _, _, _, _, repo, _, wrepo = _stage(gpu, frames, masks, pcfg=PlateFillConfig(max_bytes=full))
    assert wrepo.path == ("warp",) and (repo.filled == rep.filled).all()
    # cuts: every segment on its own
    cuts = [5]
    _, _, outc, dilc, repc, _, wrepc = _stage(gpu, frames, masks, cuts=cuts)
    wantc, wdc, wcc, infos = WR.plate_fill(frames, masks, cuts=cuts)
    assert wrepc.path == tuple(i["warp"] for i in infos) and (np.stack(outc) == wantc).all() and (dilc.cpu().numpy() == wdc).all() and (repc.filled == wcc[:, 0]).all()


def test_locked_off_clip_and_pure_pan_are_the_call_with_plate_align_alone(gpu):
    clips = [(R.locked_off_clip()[:2], "static", "static"), (A.stage_clip(96, 132)[:2], "canvas", "translation")]
    for (frames, masks), apath, wpath in clips:
        flist, d, out, dil, rep, arep, wrep = _stage(gpu, frames, masks)
        _, _, base_out, base_dil, base, barep, _ = _stage(gpu, frames, masks, wcfg=None)
        assert arep.path == (apath,) and wrep.path == (wpath,) and wrep.box == (None,) and rep.filled.sum() > 0
        assert (np.stack(out) == np.stack(base_out)).all() and (dil.cpu().numpy() == base_dil.cpu().numpy()).all()
        assert all((a == b).all() if isinstance(a, np.ndarray) else a == b for a, b in zip(rep, base))       # the PlateFillReport, field by field
        assert all((out[i] is flist[i]) == (rep.filled[i] == 0) for i in range(len(flist)))
        if wpath == "translation":
            assert not wrep.failed[0].any() and wrep.kept[0][1:].min() >= 12 and (wrep.maps[0][:, [1, 2, 4, 5]] == [1, 0, 0, 1]).all()     # fitted, and exactly linear-free
            assert (wrep.maps[0][:, [0, 3]] == arep.off[0]).all()


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=960, num_inference_steps=2, scheduler="ddim")
T, H, W = 12, 96, 160
SPANS = SpanConfig("masked", context=1, min_len=3, min_gap=2)
ROI = RoiConfig("follow", context=0.25, pad_min=8, min_side=32)


@pytest.fixture(scope="module")
def clip():
    frames, masks, _, _ = WR.warp_clip(T=T, H=H, W=W, seed=4, dilate=0)
    masks[7:] = 0                                                                                     # the box leaves early: frames without a mask for spans
    m3 = [np.repeat(m[..., None], 3, axis=2) for m in masks]
    prior = []
    for f, m in zip(frames, masks):
        p = f.copy()
        p[m > 0] = f.reshape(-1, 3).mean(0).astype(np.uint8)
        prior.append(p)
    return list(frames), m3, prior


def _run(frames, masks, prior, **kw):
    import diffuerase
    diffuerase.configure(RUN)
    try:
        out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, feather_px=3, **KW, **kw)
        return out, diffuerase.last_plate_fill, diffuerase.last_plate_align, diffuerase.last_plate_warp
    finally:
        diffuerase.configure(None)


def _same(a, b):
    return len(a) == len(b) == T and (np.stack(a) == np.stack(b)).all()


@pytest.mark.parametrize("more", [{}, dict(spans=SPANS, roi=ROI)], ids=["plain", "spans-roi"])
def test_drop_in_equals_the_call_on_the_reference_stage(gpu, clip, monkeypatch, more):
    from videovanish_amd import hip, infill
    frames, masks, prior = clip
    dil = hip.mask_collapse_dilate(_d(np.stack(masks), gpu), KW["mask_dilation_iter"]).cpu().numpy()
    want_f, want_d, want_c, infos = WR.plate_fill(np.stack(frames), dil)
    assert infos[0]["warp"] == "warp" and (infos[0]["track"][:7, 3] == 1).all()                            # every masked frame is tracked (the tracker loses the last three)
    kept = [f.copy() for f in frames]
    out, rep, arep, wrep = _run(frames, masks, prior, plate_fill="on", plate_align="on", plate_warp="on", **more)
    assert rep is not None and (rep.filled == want_c[:, 0]).all() and (rep.left == want_c[:, 1]).all() and rep.skipped == (False,)
    assert arep is not None and arep.path == ("canvas",) and wrep is not None and wrep.path == ("warp",) and wrep.box == (infos[0]["wbox"],)
    assert rep.filled.sum() > 0 and all((a == b).all() for a, b in zip(frames, kept))
    empty = infill.PlateFillReport(np.zeros(T, np.int64), np.zeros(T, np.int64), (0,), (False,), ((0, T),), ())

    def by_hand(f, d, cfg, cuts=None, acfg=None, align_out=None, wcfg=None, warp_out=None):
        assert acfg == PlateAlignConfig() and wcfg == PlateWarpConfig()
        align_out.append(arep)
        warp_out.append(wrep)
        return [want_f[i] if (want_f[i] != frames[i]).any() else frames[i] for i in range(T)], _d(want_d, gpu), empty
    monkeypatch.setattr(infill, "plate_fill", by_hand)
    hand, _, _, _ = _run(frames, masks, prior, plate_fill="on", plate_align="on", plate_warp="on", **more)
    assert _same(out, hand)
    monkeypatch.undo()
    aligned, arep1, _, none = _run(frames, masks, prior, plate_fill="on", plate_align="on", **more)
    assert none is None and arep1.filled.sum() < rep.filled.sum() and not _same(out, aligned)               # without the option: the stage as it was
    with pytest.raises(ValueError, match="plate_warp="):
        _run(frames, masks, prior, plate_fill="on", plate_warp="on", **more)
