"""Mask-region inference with one window per separate masked region, on the GPU: the two new kernels of vv_roi.hip against numpy, and the
drop-in's region path against the same computation spelled out step by step (per region: crop -> prior -> model; then roi_paste_composite
chained over the regions), against the fp32 oracle on each region's crop, and against the single-window / full-frame paths where it falls
back to them.  Tiny architecture."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig
from videovanish_amd.roi import RoiConfig, label_tiles, plan_regions


def _np_bbox(m):
    out = np.zeros((m.shape[0], 4), np.int32)
    for t in range(m.shape[0]):
        ys, xs = np.nonzero(m[t])
        if len(ys):
            out[t] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
    return out


def _np_occ(m, tile):
    T, H, W = m.shape
    occ = np.zeros(((H + tile - 1) // tile, (W + tile - 1) // tile), np.uint8)
    ys, xs = np.nonzero(m.any(axis=0))
    occ[ys // tile, xs // tile] = 1
    return occ


def _masks(T, H, W, seed):
    """The frame kinds of test_roi_gpu.py: empty, a pixel in each corner, full, sparse, a random box."""
    rng = np.random.default_rng(seed)
    m = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        kind = t % 8
        if kind == 0:
            continue
        if kind in (1, 2, 3, 4):
            m[t, (H - 1) * (kind in (3, 4)), (W - 1) * (kind in (2, 4))] = rng.integers(1, 256)
        elif kind == 5:
            m[t] = 255
        elif kind == 6:
            m[t] = (rng.random((H, W)) > 0.999) * rng.integers(1, 256, (H, W))
        else:
            y0, x0 = rng.integers(0, H), rng.integers(0, W)
            m[t, y0: y0 + rng.integers(1, H + 1), x0: x0 + rng.integers(1, W + 1)] = 7
    return m


SHAPES = [(40, 37, 53), (3, 720, 1280), (1, 1, 1), (5, 64, 65)]


@pytest.mark.parametrize("tile", [8, 16, 32])
@pytest.mark.parametrize("T,H,W", SHAPES)
def test_mask_tile_union_matches_numpy(gpu, T, H, W, tile):
    from videovanish_amd import hip
    m = _masks(T, H, W, T * 1000 + H)
    for mm in (m, m[:1] * 0, m[:1] * 0 + 1, m[:2] * 0 + (np.arange(H * W).reshape(H, W) % 97 == 5)):   # + empty, full and sparse clips
        mm = np.ascontiguousarray(mm, dtype=np.uint8)
        got = hip.mask_tile_union(torch.from_numpy(mm).to(gpu), tile).cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == ((H + tile - 1) // tile, (W + tile - 1) // tile)
        assert (got == _np_occ(mm, tile)).all()


@pytest.mark.parametrize("tile", [8, 16, 32])
@pytest.mark.parametrize("T,H,W", SHAPES)
def test_mask_bbox_tiles_matches_numpy(gpu, T, H, W, tile):
    """Every occupied tile gets a random label in [0, K) (K up to 64): per (frame, label) the box of the pixels of that label's tiles; the union over
    labels is mask_bbox; entries outside the grid or with a label outside [0, K) change nothing."""
    from videovanish_amd import hip
    rng = np.random.default_rng(7 * T + W + tile)
    m = _masks(T, H, W, T * 1000 + H + 1)
    occ = _np_occ(m, tile)
    ty, tx = np.nonzero(occ)
    K = int(min(64, max(1, len(ty))))
    lab = rng.integers(0, K, len(ty))
    tiles = np.stack([ty, tx, lab], 1).astype(np.int32)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    got = hip.mask_bbox_tiles(d(m), tile, d(tiles), K).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (T, K, 4)
    px = np.full(occ.shape, -1, np.int64)
    px[ty, tx] = lab
    px = np.repeat(np.repeat(px, tile, 0), tile, 1)[:H, :W]
    for k in range(K):
        assert (got[:, k] == _np_bbox(m * (px == k))).all(), k
    union = np.zeros((T, 4), np.int32)
    for t in range(T):
        has = (got[t, :, 2] > got[t, :, 0]) & (got[t, :, 3] > got[t, :, 1])
        if has.any():
            union[t] = (got[t, has, 0].min(), got[t, has, 1].min(), got[t, has, 2].max(), got[t, has, 3].max())
    assert (union == hip.mask_bbox(d(m)).cpu().numpy()).all()
    Hc, Wc = occ.shape
    junk = np.array([[-1, 0, 0], [0, -1, 0], [Hc, 0, 0], [0, Wc, 0], [1 << 30, 1 << 30, 0], [0, 0, -1], [0, 0, K], [0, 0, 1 << 30]], np.int32)
    got2 = hip.mask_bbox_tiles(d(m), tile, d(np.concatenate([junk[:4], tiles, junk[4:]])), K).cpu().numpy()
    assert (got2 == got).all()
    none = hip.mask_bbox_tiles(d(m), tile, d(junk), K).cpu().numpy()
    assert (none == 0).all()


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=960, num_inference_steps=2, scheduler="ddim")
FEATHER = 3
T, H, W = 5, 96, 160


def _clip(boxes, seed):
    """Random frames; masks: boxes (y0, y1, x0, x1, vx) moving vx px per frame; prior: the frame with the masked pixels set to its mean colour."""
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(T)]
    masks, prior = [], []
    for t in range(T):
        m = np.zeros((H, W, 3), np.uint8)
        for y0, y1, x0, x1, vx in boxes:
            m[y0:y1, x0 + vx * t: x1 + vx * t] = 255
        masks.append(m)
        p = frames[t].copy()
        p[m[..., 0] > 0] = frames[t].reshape(-1, 3).mean(0).astype(np.uint8)
        prior.append(p)
    return frames, masks, prior


CORNERS = [(6, 18, 6, 30, 2), (70, 86, 124, 148, -2)]          # top left moving right, bottom right moving left


def _cfg(mode, **kw):
    return RoiConfig(mode, **dict(dict(context=0.25, pad_min=8, min_side=32, smooth=1, max_regions=8), **kw))


def _dilate(masks, gpu):
    from videovanish_amd import hip
    return hip.mask_collapse_dilate(torch.from_numpy(np.stack(masks)).to(gpu).contiguous(), KW["mask_dilation_iter"])


def _np_plans(dil, cfg):
    """The region plan from numpy: occupancy on 16-px tiles, label_tiles, per (frame, label) boxes, plan_regions."""
    labels, K, tile = label_tiles(_np_occ(dil, 16))
    px = np.repeat(np.repeat(labels, tile, 0), tile, 1)[:H, :W]
    bb = np.stack([_np_bbox(dil * (px == k)) for k in range(K)], 1) if K else np.zeros((T, 0, 4), np.int32)
    return plan_regions(bb, H, W, FEATHER, cfg), K


def _manual_chain(frames, masks, prior, cfg, gpu, feather=FEATHER):
    """The region path spelled out: plans, per region crop -> prior -> model, then roi_paste_composite chained over the regions."""
    import diffuerase
    from videovanish_amd import hip
    dil_t = _dilate(masks, gpu)
    dil = dil_t.cpu().numpy()
    plans, _ = _np_plans(dil, cfg)
    crops = [[p.crop(frames), p.crop(list(dil)), None if prior is None else p.crop(prior)] for p in plans]
    if prior is None:
        for c in crops:
            c[2] = diffuerase.propainter.forward(c[0], c[1], ref_stride=10, neighbor_length=10, subvideo_length=50, mask_dilation=0)
    outs = [diffuerase.video_inpainting_sd.forward(c[0], c[1], c[2], max_img_size=KW["max_img_size"], mask_dilation_iter=0, num_inference_steps=2,
                                                   scheduler="ddim") for c in crops]
    cur = torch.from_numpy(np.stack(frames)).to(gpu)
    for p, o in zip(plans, outs):
        h, w = p.size
        cur = hip.roi_paste_composite(torch.from_numpy(np.stack(o)).to(gpu), cur, dil_t, torch.from_numpy(p.offsets).to(gpu), h, w, float(feather))
    return cur.cpu().numpy(), plans, dil, crops


def _inside(plans):
    inside = np.zeros((T, H, W), bool)
    for p in plans:
        h, w = p.size
        for t, (oy, ox) in enumerate(p.offsets.tolist()):
            inside[t, oy:oy + h, ox:ox + w] = True
    return inside


@pytest.mark.parametrize("with_prior", [True, False])
@pytest.mark.parametrize("mode", ["static", "follow"])
def test_regions_equal_the_manual_chain_and_the_oracle(gpu, mode, with_prior):
    import diffuerase
    from oracle import pipeline_ref as R
    frames, masks, prior = _clip(CORNERS, seed=41)
    cfg = _cfg(mode)
    pr = prior if with_prior else None
    diffuerase.configure(RUN)
    try:
        progs = []
        out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=pr, feather_px=FEATHER, prog=lambda p, s: progs.append((p, s)), roi=cfg,
                                              **KW)
        want, plans, dil, crops = _manual_chain(frames, masks, pr, cfg, gpu)
        raw = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=pr, feather_px=FEATHER, roi=cfg, keep_unmasked_original=False, **KW)
        want_raw = _manual_chain(frames, masks, pr, cfg, gpu, feather=-1.0)[0]
    finally:
        diffuerase.configure(None)
    assert len(plans) == 2 and all(p.size[0] < H and p.size[1] < W for p in plans)              # two true sub-windows
    assert len(out) == T and all(o.shape == (H, W, 3) and o.dtype == np.uint8 for o in out)
    assert (np.stack(out) == want).all()
    assert (np.stack(raw) == want_raw).all()
    inside = _inside(plans)
    for o in (out, raw):
        assert (np.stack(o)[~inside] == np.stack(frames)[~inside]).all()                        # outside every window: the original bytes
    # the progress protocol: each milestone once, in order, values non-decreasing, every message non-empty
    vals = [p for p, _ in progs]
    seq = [5, 10, 50, 90] if with_prior else [5, 10, 20, 50, 90]
    assert [v for v in vals if v in (5, 10, 20, 50, 90)] == seq
    assert vals == sorted(vals) and all(isinstance(s, str) and s for _, s in progs)
    if not with_prior:
        assert any(20 < v < 50 for v in vals)
    assert any(50 < v < 90 for v in vals)
    # fp32 oracle on each region's crop (with that region's prior), pasted and feathered in numpy
    pasted = np.stack(frames).copy()
    for p, (cf, cm, cp) in zip(plans, crops):
        ref = R.diffueraser_forward(cf, cm, cp, max_img_size=KW["max_img_size"], steps=2, chunk=4, overlap=2, seed=3, ucfg=TINY_UNET, vcfg=TINY_VAE)
        h, w = p.size
        for t, (oy, ox) in enumerate(p.offsets.tolist()):
            pasted[t, oy:oy + h, ox:ox + w] = R.I.resize_bilinear_u8(ref[t], w, h)
    for t in range(T):
        r = R.I.composite(pasted[t], frames[t], R.I.feather_alpha(dil[t], FEATHER))
        du = np.abs(out[t].astype(int) - r.astype(int))
        assert du.max() <= 4, (t, int(du.max()))


def test_regions_fall_back_and_are_deterministic(gpu):
    import diffuerase
    diffuerase.configure(RUN)
    try:
        for mode in ("static", "follow"):
            # one object: the single-window path
            frames, masks, prior = _clip(CORNERS[:1], seed=42)
            a = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, roi=_cfg(mode), **KW)
            b = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, roi=_cfg(mode, max_regions=1), **KW)
            assert (np.stack(a) == np.stack(b)).all()
            # two separate objects whose windows collide: one window, the single-window path
            frames, masks, prior = _clip([(30, 40, 10, 30, 0), (30, 40, 70, 90, 0)], seed=43)
            plans, K = _np_plans(_dilate(masks, gpu).cpu().numpy(), _cfg(mode, min_side=64))
            assert K == 2 and len(plans) == 1
            a = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, roi=_cfg(mode, min_side=64), **KW)
            b = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, roi=_cfg(mode, min_side=64, max_regions=1), **KW)
            assert (np.stack(a) == np.stack(b)).all()
        # windows that fill the frame: the full-frame path
        frames, masks, prior = _clip(CORNERS, seed=44)
        assert _np_plans(_dilate(masks, gpu).cpu().numpy(), _cfg("static", min_side=4096)) == (None, 2)
        a = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, roi=_cfg("static", min_side=4096), **KW)
        b = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, roi="off", **KW)
        assert (np.stack(a) == np.stack(b)).all()
        # two identical calls
        a = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, roi=_cfg("follow"), **KW)
        b = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, roi=_cfg("follow"), **KW)
        assert (np.stack(a) == np.stack(b)).all()
        single = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, roi=_cfg("follow", max_regions=1), **KW)
        assert not (np.stack(a) == np.stack(single)).all()                                       # the two windows changed what the model saw
    finally:
        diffuerase.configure(None)
