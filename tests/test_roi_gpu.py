"""Mask-region inference on the GPU: the two kernels of vv_roi.hip against numpy and against the kernel chain they fuse, and the drop-in's
roi= path against the same computation spelled out step by step (plan -> crops -> the unchanged model on the crops -> resize + paste +
feathered composite), against the fp32 oracle on the same crops, and against roi=None where the plan falls back.  Tiny architecture."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig
from videovanish_amd.roi import RoiConfig, plan_roi


def _np_bbox(m):
    out = np.zeros((m.shape[0], 4), np.int32)
    for t in range(m.shape[0]):
        ys, xs = np.nonzero(m[t])
        if len(ys):
            out[t] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
    return out


@pytest.mark.parametrize("T,H,W", [(40, 37, 53), (3, 720, 1280), (1, 1, 1), (5, 64, 65)])
def test_mask_bbox_matches_numpy(gpu, T, H, W):
    from videovanish_amd import hip
    rng = np.random.default_rng(T * 1000 + H)
    m = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        kind = t % 8
        if kind == 0:
            continue                                                      # empty frame
        if kind in (1, 2, 3, 4):                                          # one pixel in each corner
            m[t, (H - 1) * (kind in (3, 4)), (W - 1) * (kind in (2, 4))] = rng.integers(1, 256)
        elif kind == 5:
            m[t] = 255                                                    # full frame
        elif kind == 6:
            m[t] = (rng.random((H, W)) > 0.999) * rng.integers(1, 256, (H, W))
        else:
            y0, x0 = rng.integers(0, H), rng.integers(0, W)
            m[t, y0: y0 + rng.integers(1, H + 1), x0: x0 + rng.integers(1, W + 1)] = 7
    got = hip.mask_bbox(torch.from_numpy(m).to(gpu)).cpu().numpy()
    assert got.dtype == np.int32 and (got == _np_bbox(m)).all()


@pytest.mark.parametrize("feather", [0.0, 3.0, 8.5, -1.0])
@pytest.mark.parametrize("shrink", [False, True])
def test_roi_paste_composite_equals_the_chain(gpu, feather, shrink):
    """Byte-equal to resize_u8(patch -> h, w) pasted into a copy of orig at the offset, then feather_composite(., orig, mask) (feather < 0: the
    paste alone).  The four frames' windows touch the four corners, i.e. every frame edge; masks are random blobs across the whole frame."""
    from videovanish_amd import hip
    T, H0, W0, h, w = 4, 50, 70, 24, 32
    Hm, Wm = (16, 24) if shrink else (h, w)
    rng = np.random.default_rng(5 + int(shrink))
    orig = rng.integers(0, 256, (T, H0, W0, 3), dtype=np.uint8)
    patch = rng.integers(0, 256, (T, Hm, Wm, 3), dtype=np.uint8)
    mask = ((rng.random((T, H0, W0)) > 0.93) * 255).astype(np.uint8)
    mask[:, 10:30, 20:40] = 255
    offs = np.array([[0, 0], [0, W0 - w], [H0 - h, 0], [H0 - h, W0 - w]], np.int32)
    d = lambda a: torch.from_numpy(a).to(gpu)
    got = hip.roi_paste_composite(d(patch), d(orig), d(mask), d(offs), h, w, feather).cpu().numpy()
    rs = hip.resize_u8(d(patch), h, w, mode="bilinear").cpu().numpy() if shrink else patch
    pasted = orig.copy()
    for t, (oy, ox) in enumerate(offs):
        pasted[t, oy:oy + h, ox:ox + w] = rs[t]
    want = pasted if feather < 0 else hip.feather_composite(d(pasted), d(orig), d(mask), feather).cpu().numpy()
    assert (got == want).all()
    if feather < 0:
        got2 = hip.roi_paste_composite(d(patch), d(orig), None, d(offs), h, w, feather).cpu().numpy()
        assert (got2 == want).all()


def _clip(T, H, W, seed):
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(T)]
    masks, prior = [], []
    for t in range(T):
        m = np.zeros((H, W, 3), np.uint8)
        m[H // 4: H // 2, W // 4 + 2 * t: W // 2 + 2 * t] = 255
        masks.append(m)
        p = frames[t].copy()
        p[m[..., 0] > 0] = frames[t].reshape(-1, 3).mean(0).astype(np.uint8)
        prior.append(p)
    return frames, masks, prior


RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=960, num_inference_steps=2, scheduler="ddim")
FEATHER = 3


def _manual_chain(frames, masks, prior, cfg, gpu):
    """The roi= path spelled out: plan, crops, the unchanged model (and prior) on the crops, resize + paste + feather_composite."""
    import diffuerase
    from videovanish_amd import hip
    H0, W0 = frames[0].shape[:2]
    dil_t = hip.mask_collapse_dilate(torch.from_numpy(np.stack(masks)).to(gpu).contiguous(), KW["mask_dilation_iter"])
    dil = dil_t.cpu().numpy()
    plan = plan_roi(_np_bbox(dil), H0, W0, FEATHER, cfg)
    cf, cm = plan.crop(frames), plan.crop(list(dil))
    if prior is None:
        cp = diffuerase.propainter.forward(cf, cm, ref_stride=10, neighbor_length=10, subvideo_length=50, mask_dilation=0)
    else:
        cp = plan.crop(prior)
    model_out = diffuerase.video_inpainting_sd.forward(cf, cm, cp, max_img_size=KW["max_img_size"], mask_dilation_iter=0,
                                                      num_inference_steps=2, scheduler="ddim")
    h, w = plan.size
    mo = torch.from_numpy(np.stack(model_out)).to(gpu)
    if mo.shape[1:3] != (h, w):
        mo = hip.resize_u8(mo.contiguous(), h, w)
    mo = mo.cpu().numpy()
    pasted = np.stack(frames).copy()
    for t, (oy, ox) in enumerate(plan.offsets.tolist()):
        pasted[t, oy:oy + h, ox:ox + w] = mo[t]
    orig = torch.from_numpy(np.stack(frames)).to(gpu)
    out = hip.feather_composite(torch.from_numpy(pasted).to(gpu), orig, dil_t, float(FEATHER)).cpu().numpy()
    return out, plan, dil, model_out, cf, cm, cp


@pytest.mark.parametrize("with_prior", [True, False])
@pytest.mark.parametrize("mode", ["static", "follow"])
def test_drop_in_roi_equals_the_manual_chain_and_the_oracle(gpu, mode, with_prior):
    import diffuerase
    from oracle import pipeline_ref as R
    T, H, W = 5, 96, 128
    frames, masks, prior = _clip(T, H, W, seed=31)
    cfg = RoiConfig(mode, context=0.25, pad_min=8, min_side=32, smooth=1)
    diffuerase.configure(RUN)
    try:
        progs = []
        out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior if with_prior else None, feather_px=FEATHER,
                                              prog=lambda p, s: progs.append(p), roi=cfg, **KW)
        want, plan, dil, model_out, cf, cm, cp = _manual_chain(frames, masks, prior if with_prior else None, cfg, gpu)
    finally:
        diffuerase.configure(None)
    h, w = plan.size
    assert h < H and w < W                                                   # a true sub-window
    assert len(out) == T and all(o.shape == (H, W, 3) and o.dtype == np.uint8 for o in out)
    assert (np.stack(out) == want).all()
    seq = [5, 10, 50, 90] if with_prior else [5, 10, 20, 50, 90]            # the drop-in's progress protocol, unchanged
    assert all(p in progs for p in seq) and [progs.index(p) for p in seq] == sorted(progs.index(p) for p in seq)
    inside = np.zeros((T, H, W), bool)
    for t, (oy, ox) in enumerate(plan.offsets.tolist()):
        inside[t, oy:oy + h, ox:ox + w] = True
    assert (np.stack(out)[~inside] == np.stack(frames)[~inside]).all()      # outside the window: the original bytes
    # fp32 oracle on the same crops (and the same prior), pasted and feathered in numpy
    ref = R.diffueraser_forward(cf, cm, cp, max_img_size=KW["max_img_size"], steps=2, chunk=4, overlap=2, seed=3, ucfg=TINY_UNET, vcfg=TINY_VAE)
    for t, (oy, ox) in enumerate(plan.offsets.tolist()):
        r = R.I.resize_bilinear_u8(ref[t], w, h)
        pasted = frames[t].copy()
        pasted[oy:oy + h, ox:ox + w] = r
        r = R.I.composite(pasted, frames[t], R.I.feather_alpha(dil[t], FEATHER))
        du = np.abs(out[t].astype(int) - r.astype(int))
        assert du.max() <= 4, (t, int(du.max()))


def test_drop_in_roi_falls_back_and_is_deterministic(gpu):
    import diffuerase
    T, H, W = 4, 96, 128
    frames, masks, prior = _clip(T, H, W, seed=32)
    diffuerase.configure(RUN)
    try:
        base = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, **KW)
        full = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, roi=RoiConfig("static", min_side=4096), **KW)
        assert (np.stack(full) == np.stack(base)).all()                      # the window would be the whole frame: today's path
        empty = [np.zeros_like(m) for m in masks]
        e0 = diffuerase.run_infill_on_frames(frames, empty, propainer_frames=prior, **KW)
        e1 = diffuerase.run_infill_on_frames(frames, empty, propainer_frames=prior, roi="follow", **KW)
        assert (np.stack(e0) == np.stack(e1)).all()                          # no mask pixel: today's path
        cfg = RoiConfig("follow", pad_min=8, min_side=32)
        a = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, roi=cfg, **KW)
        b = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, roi=cfg, **KW)
        assert (np.stack(a) == np.stack(b)).all()
        assert not (np.stack(a) == np.stack(base)).all()                     # the window really changed what the model saw
        # keep_unmasked_original=False: the window is pasted as the model left it, the rest stays the original
        k = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, roi=cfg, keep_unmasked_original=False, **KW)
        far = np.zeros((T, H, W), bool)                                      # windows: about rows 12-60, columns 20-82
        far[:, 72:, :] = True
        far[:, :, 100:] = True
        assert (np.stack(k)[far] == np.stack(frames)[far]).all()
    finally:
        diffuerase.configure(None)
