"""Clean-plate fill on the GPU: the three entry points of vv_plate.hip against the numpy restatement of include/vvplate.h (tests/platefill_ref.py)
byte for byte, each run twice with identical bytes; infill.plate_fill alone and with cuts; and the drop-in's plate_fill= path against the same
call handed the reference's frames and masks.  Tiny architecture."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import platefill_ref as R  # noqa: E402

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.platefill import PlateFillConfig  # noqa: E402
from videovanish_amd.roi import RoiConfig  # noqa: E402
from videovanish_amd.spans import SpanConfig  # noqa: E402

TILE = 64


def _d(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _twice(fn):
    """fn() -> tensors; run twice, identical bytes; the first run's results as numpy arrays."""
    a, b = fn(), fn()
    a, b = [x.cpu().numpy() for x in a], [x.cpu().numpy() for x in b]
    assert all((x == y).all() for x, y in zip(a, b))
    return a


def _tile_px(occ, H, W):
    """occ [th,tw] -> [H,W] bool: the pixel lies in an occupied tile."""
    return np.kron(occ, np.ones((TILE, TILE), np.uint8))[:H, :W] != 0


def _check(frames, dil, gpu, tiles=True, poison=False, **cfg):
    """One segment through vvp_stats, vvp_sources, the margin and vvp_fill, every kernel twice, every output against the restatement.
    tiles=False: no occupancy grid (every pixel's statistics).  poison=True: the image bytes of the device copy outside the occupied tiles are
    overwritten first; no output may change.  Returns the restatement's (frames', dil', counts, detail)."""
    from videovanish_amd import hip, mask_hip, plate_hip
    cfg = dict(R.DEFAULTS, **cfg)
    T, H, W = dil.shape
    want_f, want_d, want_c, det = R.fill_segment(frames, dil, detail=True, **cfg)
    d = _d(dil, gpu)
    occ = hip.mask_tile_union(d, TILE) if tiles else None
    live = _tile_px(occ.cpu().numpy(), H, W) if tiles else np.ones((H, W), bool)
    assert ((dil != 0).any(0) <= live).all()
    up = frames.copy()
    if poison:
        assert not live.all()
        up[:, ~live] = np.random.default_rng(1).integers(0, 256, up[:, ~live].shape)
    f = _d(up, gpu)
    ns = d if cfg["guard"] == 0 else mask_hip.time_bridge_grow(d, 0, cfg["guard"])[0]
    assert ((ns.cpu().numpy() != 0) == det["ns"]).all()
    st, n, s1 = _twice(lambda: plate_hip.stats(f, ns, occ, cfg["min_samples"], cfg["tol"]))
    assert st.dtype == np.uint8 and n.dtype == np.int32 and s1.dtype == np.int32
    assert (st == (det["steady"] & live)).all(), int((st != (det["steady"] & live)).sum())
    assert (n == det["n"] * live).all() and (s1 == det["S1"] * live[..., None]).all()
    t_st, t_n, t_s1 = _d(st, gpu), _d(n, gpu), _d(s1, gpu)
    src, r0 = _twice(lambda: plate_hip.sources(f, d, ns, occ, t_st, t_n, t_s1, cfg["tol"], cfg["outlier"], cfg["max_gap"]))
    src = src.view(np.uint16)
    assert (src == det["src"]).all(), int((src != det["src"]).sum())                  # outside the occupied tiles: no mask, NONE
    assert (r0 == det["r0"]).all()
    t_src, t_r0 = _d(src.view(np.int16), gpu), _d(r0, gpu)
    keep = t_r0 if cfg["margin"] == 0 else hip.mask_collapse_dilate(t_r0[..., None].contiguous(), cfg["margin"])

    def fill():
        g = f.clone()
        return (g,) + tuple(plate_hip.fill(g, d, keep, occ, t_src))
    got_f, got_d, got_c = _twice(fill)
    assert got_c.dtype == np.int64 and (got_c == want_c).all(), (got_c.tolist(), want_c.tolist())
    assert (got_d == want_d).all() and set(np.unique(got_d)) <= {0, 255}
    assert (got_f[:, live] == want_f[:, live]).all() and (got_f[:, ~live] == up[:, ~live]).all()
    assert (got_f[dil == 0] == up[dil == 0]).all()                                    # pixels with dil == 0 keep their bytes
    return want_f, want_d, want_c, det


def _mixed_clip(T, H, W, seed):
    """Pixels of every kind: a still with per-pixel noise of amplitude 0 / 3 / 6 / 9 / 30 (steady, on the edge, not steady), a spike in 2 % of
    the samples (outliers), a box that crosses, pixels that flicker in and out of the mask, and a block masked in every frame."""
    rng = np.random.default_rng(seed)
    amp = rng.choice([0, 3, 6, 9, 30], (H, W, 1))
    frames = R.background(H, W, seed)[None] + rng.integers(-1, 2, (T, H, W, 3)) * amp
    spike = rng.random((T, H, W, 1)) < 0.02
    frames = np.clip(frames + spike * rng.choice([-22, 22], (T, H, W, 1)), 0, 255).astype(np.uint8)
    m = np.zeros((T, H, W), bool)
    bw = max(W // 5, 2)
    for t in range(T):
        x0 = -bw // 2 + (t * (W + bw)) // max(T, 1)
        m[t, H // 8: H // 8 + H // 3, max(x0, 0): max(min(x0 + bw, W), 0)] = True
    flick = rng.random((H, W)) < 0.1
    m[:, flick] |= rng.random((T, int(flick.sum()))) < 0.3
    m[:, H - 6: H - 2, 2: 7] = True
    frames[m] = 255 - frames[m] // 4
    return frames, (m * rng.integers(1, 256, m.shape)).astype(np.uint8)             # any non-zero byte is masked


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(40, 56), (96, 130), (96, 132)])      # smaller than a tile; a remainder tile on the byte path; on the 4-pixel path
@pytest.mark.parametrize("tiles", [True, False])
def test_kernels_on_the_locked_off_clip(gpu, H, W, tiles):
    scale = H // 40
    frames, masks, clean, boxm, logom = R.locked_off_clip(24, H, W, speed=2 * W // 56, box=(15 * scale, 16 * W // 56), box_y=4 * scale,
                                                          logo=(26 * scale, 4, 38 * scale, 8))
    out, dil, counts, det = _check(frames, masks, gpu, tiles=tiles)
    assert not dil[boxm].any() and (dil[:, logom] == 255).all() and counts[:, 0].sum() == boxm.sum()
    assert np.abs(out[boxm].astype(np.int64) - clean[boxm]).max() <= 6


@pytest.mark.parametrize("guard", [0, 1, 4])
@pytest.mark.parametrize("margin", [0, 2])
@pytest.mark.parametrize("max_gap", [0, 3])
def test_kernels_parameters(gpu, guard, margin, max_gap):
    for (H, W), seed in (((40, 56), 3), ((33, 50), 4)):                # the 4-pixel path, the byte path
        frames, masks = _mixed_clip(24, H, W, seed)
        out, dil, counts, det = _check(frames, masks, gpu, guard=guard, margin=margin, max_gap=max_gap)
        assert counts[:, 1].sum() > 100 and (~det["steady"]).sum() > 50 and det["steady"].sum() > 50
        # a source lies at least guard + 1 frames from the frame it fills: guard 4 with max_gap 3 fills nothing
        assert (counts[:, 0].sum() > 0) == (not (guard == 4 and max_gap == 3))
        assert (~det["ns"] & det["steady"][None] & ~det["usable"]).sum() > 0                    # outliers among the samples of steady pixels


def test_kernels_short_clips_and_min_samples_above_n(gpu):
    for T in (1, 2):
        frames, masks = _mixed_clip(T, 40, 56, 10 + T)
        out, dil, counts, det = _check(frames, masks, gpu, guard=0, min_samples=1)
        assert counts.shape == (T, 2)
    frames, masks = _mixed_clip(2, 40, 56, 13)
    masks[0, 20:, :] = 0                                                   # T = 2, guard 0: frame 0 is the plate of frame 1
    out, dil, counts, det = _check(frames, masks, gpu, guard=0, min_samples=1, margin=0)
    assert counts[1, 0] > 0 and (det["src"][1][(masks[1] != 0) & (dil[1] == 0)] == 0).all()
    frames, masks, clean, boxm, logom = R.locked_off_clip()
    out, dil, counts, det = _check(frames, masks, gpu, min_samples=25)   # more than the clip has frames: nothing is steady
    assert not det["steady"].any() and not counts[:, 0].any() and (dil == masks).all() and (out == frames).all()
    n_box = det["n"][boxm.any(0)]
    out, dil, counts, det = _check(frames, masks, gpu, min_samples=int(n_box.min()) + 1)       # above the n of some pixels, not of others
    assert 0 < counts[:, 0].sum() < boxm.sum()


def test_kernels_pixel_cases(gpu):
    T, H, W = 24, 8, 8
    frames = np.full((T, H, W, 3), 100, np.uint8)
    masks = np.zeros((T, H, W), np.uint8)
    masks[:, 0, 0] = 255                                                   # masked in every frame: no sample, left
    masks[10:13, 1, 1] = 255                                               # an exact tie between 9 and 13 for t = 11 (guard 0): the earlier wins
    vals = np.array([10, 10, 22, 22])                                      # n S2 - S1^2 = 576 = tol^2 n^2: steady, exactly
    masks[4:, 2, 2] = 255
    frames[:4, 2, 2] = vals[:, None]
    masks[4:, 2, 3] = 255
    frames[:4, 2, 3] = (vals + [0, 0, 0, 1])[:, None]                      # 627 > 576: not steady
    masks[8:12, 3, 3] = 255                                                # an outlier next to the run: 20 samples, one at 125
    frames[7, 3, 3] = 125                                                  # std 5.4 <= 6, |125 - mean| = 23.75 > 18
    masks[8:12, 3, 4] = 255
    frames[7, 3, 4, 1] = 125                                               # in one channel only
    out, dil, counts, det = _check(frames, masks, gpu, guard=0, margin=0)
    assert det["n"][0, 0] == 0 and (dil[:, 0, 0] == 255).all()
    assert det["src"][10:13, 1, 1].tolist() == [9, 9, 13]
    assert det["steady"][2, 2] and not det["steady"][2, 3] and not dil[4:, 2, 2].any() and (dil[4:, 2, 3] == 255).all()
    assert det["src"][4:8, 2, 2].tolist() == [3, 3, 3, 3] and (out[4:, 2, 2] == 22).all()
    for x in (3, 4):
        assert det["steady"][3, x] and not det["usable"][7, 3, x] and det["src"][8:12, 3, x].tolist() == [6, 6, 12, 12]
        assert (out[8:12, 3, x] == 100).all()
    _check(frames, masks, gpu, guard=1, margin=2, max_gap=1)


def test_kernels_long_clip_needs_64_bits(gpu):
    """T = 300 on 8 x 8 with values 0 / 255: n S2 is about 5.6e9 and tol^2 n^2 3.0e6, S1^2 about 1.4e9: a 32-bit intermediate shows."""
    T = 300
    rng = np.random.default_rng(9)
    frames = (rng.random((T, 8, 8, 3)) < 0.5).astype(np.uint8) * 255
    frames[:, :, 4:] = 255                                                 # the right half is steady, at the top of the range
    frames[:, 4:, 4:, 1] = 0
    masks = np.zeros((T, 8, 8), np.uint8)
    masks[100:140] = 255
    masks[290:, 0] = 255
    out, dil, counts, det = _check(frames, masks, gpu, tiles=False)
    assert det["n"].max() > 250 and int((det["n"][..., None] * det["S2"]).max()) > 2 ** 32
    assert det["steady"][:, 4:].all() and not det["steady"][:, :4].any()
    assert not dil[:, :, 6:].any() and (dil[100:140, :, :4] == 255).all()


def test_tiles_without_a_mask_are_never_read(gpu):
    """The only mask lies in one tile of 3 x 3; the image bytes of every other tile are overwritten in the device copy."""
    frames, masks, clean, boxm, logom = R.locked_off_clip(24, 150, 180, speed=5, box=(15, 16), box_y=70, logo=(100, 70, 110, 76))
    masks[:, :, :64] = 0
    masks[:, :, 128:] = 0
    assert (masks[:, 64:128, 64:128] != 0).any() and not masks[:, :64].any() and not masks[:, 128:].any()
    want = _check(frames, masks, gpu)
    got = _check(frames, masks, gpu, poison=True)
    assert (want[1] == got[1]).all() and (want[2] == got[2]).all() and got[2][:, 0].sum() > 0


def test_refusals_launch_nothing(gpu):
    from videovanish_amd import plate_hip
    lib = plate_hip.lib()
    f = torch.full((2, 8, 8, 3), 7, dtype=torch.uint8, device=gpu)
    m = torch.full((2, 8, 8), 7, dtype=torch.uint8, device=gpu)
    w = torch.full((2, 8, 8, 3), 7, dtype=torch.int32, device=gpu)
    cnt = torch.full((2, 2), 7, dtype=torch.int64, device=gpu)
    p = lambda t: t.data_ptr()
    bad = [lib.vvp_stats(p(f), p(m), None, 0, 8, 8, 64, 4, 6, p(m), p(w), p(w), None), lib.vvp_stats(p(f), p(m), None, 2, 8, 8, 64, 0, 6, p(m), p(w), p(w), None),
           lib.vvp_stats(p(f), p(m), p(m), 2, 8, 8, 0, 4, 6, p(m), p(w), p(w), None),
           lib.vvp_sources(p(f), p(m), p(m), None, p(m), p(w), p(w), 2, 8, 8, 64, 6, -1, 0, p(w), p(m), None),
           lib.vvp_fill(p(f), p(m), p(m), None, p(w), 2, 8, 8, 64, p(m), p(cnt), None), lib.vvp_fill(p(f), p(m), p(m), None, p(w), 2, 8, 8, 64, None, p(cnt), None)]
    assert bad == [-1] * len(bad) and b"vvp_fill" in lib.vvp_last_error()
    unsupported = [lib.vvp_stats(p(f), p(m), None, 2, 8, 8, 64, 4, 256, p(m), p(w), p(w), None),
                   lib.vvp_sources(p(f), p(m), p(m), None, p(m), p(w), p(w), 2, 8, 8, 64, 6, 65, 0, p(w), p(m), None),
                   lib.vvp_fill(p(f), p(m), p(m), None, p(w), 65536, 8, 8, 64, p(w), p(cnt), None)]
    assert unsupported == [-2] * 3 and b"65536" in lib.vvp_last_error()
    torch.cuda.synchronize()
    assert (f == 7).all() and (m == 7).all() and (w == 7).all() and (cnt == 7).all()          # nothing was launched, nothing cleared
    with pytest.raises(RuntimeError, match="tol <= 255"):
        plate_hip.stats(f, m, None, 4, 256)
    with pytest.raises(RuntimeError):
        plate_hip.stats(f.cpu(), m.cpu(), None, 4, 6)                                         # no CPU fallback
    with pytest.raises(ctypes.ArgumentError):
        lib.vvp_stats(p(f), p(m), None, 2.0, 8, 8, 64, 4, 6, p(m), p(w), p(w), None)


# ---- infill.plate_fill --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", [None, [9, 15]])
@pytest.mark.parametrize("H,W", [(40, 56), (96, 130)])
def test_plate_fill_alone_and_with_cuts(gpu, cuts, H, W):
    from videovanish_amd import infill, plate_hip
    scale = H // 40
    frames, masks, clean, boxm, logom = R.locked_off_clip(24, H, W, speed=2 * W // 56, box=(15 * scale, 16 * W // 56), box_y=4 * scale,
                                                          logo=(26 * scale, 6, 38 * scale, 11))
    flist = [f.copy() for f in frames]
    d = _d(masks, gpu)
    want, wd, wc = R.plate_fill(frames, masks, cuts=cuts)
    for cfg in (PlateFillConfig(), PlateFillConfig(guard=0, margin=0, max_gap=3)):
        if cfg.guard == 0:
            want, wd, wc = R.plate_fill(frames, masks, cuts=cuts, **dict(R.DEFAULTS, guard=0, margin=0, max_gap=3))
        out, dil, rep = infill.plate_fill(flist, d, cfg, cuts)
        assert (np.stack(out) == want).all() and (dil.cpu().numpy() == wd).all()
        assert (rep.filled == wc[:, 0]).all() and (rep.left == wc[:, 1]).all() and rep.filled.sum() > 0
        assert rep.cuts == tuple(cuts or ()) and rep.skipped == (False,) * len(rep.segments)
        assert all((out[i] is flist[i]) == (wc[i, 0] == 0) for i in range(24))
        assert all((a == b).all() for a, b in zip(flist, frames)) and (d.cpu().numpy() == masks).all()      # the caller's arrays are never written
    out, dil, rep = infill.plate_fill(flist, d, PlateFillConfig(max_bytes=100), cuts)
    assert all(rep.skipped) and dil is d and all(a is b for a, b in zip(out, flist)) and (rep.left == (masks != 0).reshape(24, -1).sum(1)).all()
    pf, pm, _, _ = R.panning_clip()
    pd = _d(pm, gpu)
    plist = list(pf)
    out, dil, rep = infill.plate_fill(plist, pd, PlateFillConfig(), cuts)
    assert dil is pd and all(a is b for a, b in zip(out, plist)) and not rep.filled.any()
    assert plate_hip.PART.dll is not None


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=960, num_inference_steps=2, scheduler="ddim")
T, H, W = 14, 96, 160
SPANS = SpanConfig("masked", context=1, min_len=3, min_gap=2)
ROI = RoiConfig("follow", context=0.25, pad_min=8, min_side=32)
SCREEN = (64, 96, 88, 136)        # a region that shows something else in every frame: never steady
LOGO = (70, 104, 80, 124)         # a mask on it in frames 4 .. 8


def _clip(logo):
    frames, masks, clean, boxm, _ = R.locked_off_clip(T, H, W, a=3, seed=5, speed=12, box=(22, 24), box_y=20, logo=None)
    rng = np.random.default_rng(77)
    y0, x0, y1, x1 = SCREEN
    frames[:, y0:y1, x0:x1] = rng.integers(0, 256, (T, y1 - y0, x1 - x0, 3))
    if logo:
        masks[4:9, LOGO[0]:LOGO[2], LOGO[1]:LOGO[3]] = 255
    m3 = [np.repeat(m[..., None], 3, axis=2) for m in masks]
    prior = []
    for f, m in zip(frames, masks):
        p = f.copy()
        p[m > 0] = f.reshape(-1, 3).mean(0).astype(np.uint8)
        prior.append(p)
    return list(frames), m3, prior


@pytest.fixture(scope="module")
def clip():
    return _clip(True)


def _run(frames, masks, prior, **kw):
    import diffuerase
    diffuerase.configure(RUN)
    try:
        out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, feather_px=3, **KW, **kw)
        return out, diffuerase.last_plate_fill
    finally:
        diffuerase.configure(None)


def _reference_stage(gpu, frames, masks):
    """The reference's (frames', dil', counts) for the call's dilated masks."""
    from videovanish_amd import hip
    dil = hip.mask_collapse_dilate(_d(np.stack(masks), gpu), KW["mask_dilation_iter"]).cpu().numpy()
    return R.plate_fill(np.stack(frames), dil) + (dil,)


def _by_hand(monkeypatch, gpu, want_f, want_d, frames):
    """infill.plate_fill replaced by a stand-in that hands over the reference's frames and masks."""
    from videovanish_amd import infill
    rep = infill.PlateFillReport(np.zeros(T, np.int64), np.zeros(T, np.int64), (0,), (False,), ((0, T),), ())
    monkeypatch.setattr(infill, "plate_fill", lambda f, d, cfg, cuts=None: ([want_f[i] if (want_f[i] != frames[i]).any() else frames[i] for i in range(T)],
                                                                           _d(want_d, gpu), rep))


def _same(a, b):
    return len(a) == len(b) == T and (np.stack(a) == np.stack(b)).all()


@pytest.mark.parametrize("more", [{}, dict(spans=SPANS, roi=ROI)], ids=["plain", "spans-roi"])
def test_drop_in_equals_the_call_on_the_reference_stage(gpu, clip, monkeypatch, more):
    frames, masks, prior = clip
    want_f, want_d, want_c, dil = _reference_stage(gpu, frames, masks)
    kept = [f.copy() for f in frames]
    out, rep = _run(frames, masks, prior, plate_fill="on", **more)
    assert rep is not None and (rep.filled == want_c[:, 0]).all() and (rep.left == want_c[:, 1]).all() and rep.skipped == (False,)
    assert rep.filled.sum() > 0 and (rep.left > 0).tolist() == [4 <= t < 9 for t in range(T)]          # the box is filled, the logo is left
    assert all((a == b).all() for a, b in zip(frames, kept))
    _by_hand(monkeypatch, gpu, want_f, want_d, frames)
    hand, _ = _run(frames, masks, prior, plate_fill="on", **more)
    assert _same(out, hand)
    monkeypatch.undo()
    far = ~R.dilate(dil != 0, 5)                                        # further from the dilated mask than the feather (3 px) reaches
    for t in range(T):
        assert (out[t][far[t]] == frames[t][far[t]]).all()
    filled = (dil != 0) & (want_d == 0)
    if more:
        # spans: frames without a mask left are the stage's frames as they are; the logo's frames went through the model
        assert all((out[t] == want_f[t]).all() for t in (0, 1, 11, 12, 13)) and not (out[6] == want_f[6]).all()
        assert all((out[t][filled[t]] == want_f[t][filled[t]]).all() for t in range(T))               # roi: filled pixels outside the window stay
    base, none = _run(frames, masks, prior, **more)
    assert none is None and not _same(out, base)
    off, none = _run(frames, masks, prior, plate_fill="off", **more)
    assert none is None and _same(off, base)


def test_locked_off_clip_without_a_logo_loads_no_model(gpu, monkeypatch):
    import diffuerase
    frames, masks, prior = _clip(False)
    want_f, want_d, want_c, dil = _reference_stage(gpu, frames, masks)
    assert not want_d.any() and want_c[:, 0].sum() == (dil != 0).sum() > 0
    monkeypatch.setattr(diffuerase, "_load_model", lambda *a: (_ for _ in ()).throw(AssertionError("no model is needed")))
    out, rep = _run(frames, masks, None, plate_fill="on", spans="masked")
    assert _same(out, list(want_f)) and not rep.left.any() and rep.filled.sum() == (dil != 0).sum()
    assert all((out[t] is frames[t]) == (want_c[t, 0] == 0) for t in range(T))
