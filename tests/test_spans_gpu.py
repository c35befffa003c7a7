"""Mask-span inference on the GPU: the frame-pair statistics of vv_spans.hip against numpy bit for bit, and the drop-in's span path against the same
call made on each sub-clip (byte for byte), against the fp32 oracle on one sub-clip, and on its special paths.  Tiny architecture."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spans_ref as R  # noqa: E402

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.roi import RoiConfig  # noqa: E402
from videovanish_amd.spans import SpanConfig, find_cuts, plan_spans  # noqa: E402


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
def _stat_clip(T, H, W, seed):
    """Frames with every luma bin in use and smooth runs (so the run-length merged histogram adds are exercised), masks of every kind."""
    rng = np.random.default_rng(seed)
    ramp = (np.add.outer(np.arange(H), np.arange(W)) % 256).astype(np.int64)
    frames = np.stack([np.clip(ramp[..., None] * [1, 1, 1] + rng.integers(-3, 4, (H, W, 3)) + 17 * t, 0, 255).astype(np.uint8) for t in range(T)])
    frames[T // 2] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)                       # one white-noise frame
    frames[0, :, : W // 2] = 255                                                           # saturated: the largest differences
    masks = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        kind = t % 4
        if kind == 1:
            masks[t, H // 4: H // 2 + 1, W // 5: W // 2 + 3] = 255
        elif kind == 2:
            masks[t] = (rng.random((H, W)) > 0.7) * rng.integers(1, 256, (H, W))
        elif kind == 3:
            masks[t, -1, -1] = 1
    return frames, masks


@pytest.mark.parametrize("T,H,W", [(7, 37, 53), (5, 180, 322), (6, 96, 160), (3, 720, 1280)])
def test_frame_pair_stats_match_numpy_bit_for_bit(gpu, T, H, W):
    from videovanish_amd import spans_hip
    frames, masks = _stat_clip(T, H, W, 1000 * T + W)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    for mk in (None, masks):
        want = R.pair_stats(frames, mk)
        n_sad, hist = spans_hip.pair_stats(d(frames), None if mk is None else d(mk))       # one launch
        assert n_sad.dtype == torch.int64 and hist.dtype == torch.int32 and tuple(hist.shape) == (T - 1, 2, 64)
        got = (n_sad[:, 1].cpu().numpy(), n_sad[:, 0].cpu().numpy(), hist.cpu().numpy())
        for g, w, name in zip(got, want, ("sad", "n", "hist")):
            assert (g == w).all(), (name, mk is not None)
        for slab in (2, 3, 64):                                                            # slab seams are crossed; host frames as a list
            got = spans_hip.frame_pair_stats(list(frames), None if mk is None else d(mk), slab=slab)
            for g, w, name in zip(got, want, ("sad", "n", "hist")):
                assert g.dtype == np.int64 and (g == w).all(), (name, slab, mk is not None)
    assert want[1].min() < H * W and (want[2].sum(axis=2) == want[1][:, None]).all()
    # an all-masked pair: n = 0, nothing counted
    masks[1] = 255
    sad, n, hist = spans_hip.frame_pair_stats(list(frames), masks, slab=3, device=gpu)     # a host mask array is accepted too
    assert n[0] == 0 and n[1] == 0 and sad[0] == 0 and not hist[:2].any()
    want = R.pair_stats(frames, masks)
    assert (sad == want[0]).all() and (n == want[1]).all() and (hist == want[2]).all()


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=960, num_inference_steps=2, scheduler="ddim")
FEATHER = 3
T, H, W = 14, 96, 160
CUT = 7
SPANS = SpanConfig("masked", context=1, min_len=3, min_gap=2)
RUNS = ((2, 4), (8, 11))                                       # the masked frame runs -> spans (1, 5) and (7, 12): frames 0, 5, 6, 12, 13 are skipped


def _clip(seed=51):
    """Two panned shots (7 + 7 frames, a hard cut at frame 7); a box mask in two separate frame runs; prior: the frame with the masked pixels set to its
    mean colour."""
    frames, cuts = R.shots_clip(seed, (CUT, T - CUT), (3, 5), H, W)
    assert cuts == [CUT]
    masks, prior = [], []
    for t in range(T):
        m = np.zeros((H, W, 3), np.uint8)
        if any(a <= t < b for a, b in RUNS):
            m[30:52, 40 + 4 * t: 76 + 4 * t] = 255
        masks.append(m)
        p = frames[t].copy()
        p[m[..., 0] > 0] = frames[t].reshape(-1, 3).mean(0).astype(np.uint8)
        prior.append(p)
    return frames, masks, prior


def _masked(masks):
    return np.array([bool(m.any()) for m in masks])


def _protocol(progs, with_prior, n):
    """each milestone once, in order, values non-decreasing, every message non-empty, every span reported"""
    vals = [p for p, _ in progs]
    assert [v for v in vals if v in (5, 10, 20, 50, 90)] == ([5, 10, 50, 90] if with_prior else [5, 10, 20, 50, 90])
    assert vals == sorted(vals) and all(isinstance(s, str) and s for _, s in progs)
    for k in range(n):
        assert any(50 < v < 90 and s.startswith(f"span {k + 1}/{n}: ") for v, s in progs), k
    if not with_prior:
        assert any(20 < v < 50 and s.startswith(f"span 1/{n}: ") for v, s in progs)


def _check_spans(frames, masks, prior, plan, spans, progs=None, with_prior=True, **kw):
    """run_infill_on_frames(spans=...) == the same call on every sub-clip frames[a:b], byte for byte; every other frame is the input."""
    import diffuerase
    pr = prior if with_prior else None
    out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=pr, feather_px=FEATHER, spans=spans,
                                          prog=None if progs is None else (lambda p, s: progs.append((p, s))), **KW, **kw)
    assert len(out) == len(frames) and all(o.shape == (H, W, 3) and o.dtype == np.uint8 for o in out)
    inside = np.zeros(len(frames), bool)
    subs = []
    for a, b in plan:
        sub = diffuerase.run_infill_on_frames(frames[a:b], masks[a:b], propainer_frames=None if pr is None else pr[a:b], feather_px=FEATHER, spans="off",
                                              **KW, **kw)
        assert (np.stack(out[a:b]) == np.stack(sub)).all(), (a, b)
        inside[a:b] = True
        subs.append(sub)
    for t in np.nonzero(~inside)[0]:
        assert (out[t] == frames[t]).all(), t
    return out, subs


@pytest.mark.parametrize("with_prior", [True, False])
def test_two_spans_equal_the_sub_clip_calls(gpu, with_prior):
    import diffuerase
    frames, masks, prior = _clip()
    plan = plan_spans(_masked(masks), None, SPANS)
    assert plan == [(1, 5), (7, 12)]                                           # two spans, skipped frames between them and at both ends
    diffuerase.configure(RUN)
    try:
        progs = []
        out, subs = _check_spans(frames, masks, prior, plan, SPANS, progs, with_prior)
        _protocol(progs, with_prior, 2)
        assert all(not (out[t] == frames[t]).all() for a, b in RUNS for t in range(a, b))      # the masked frames were inpainted
        if with_prior:
            # frames outside the spans are the inputs with keep_unmasked_original=False too
            _check_spans(frames, masks, prior, plan, SPANS, keep_unmasked_original=False)
            # one span against the fp32 oracle on its sub-clip
            from oracle import pipeline_ref as O
            from videovanish_amd import hip
            a, b = plan[1]
            dil = hip.mask_collapse_dilate(torch.from_numpy(np.stack(masks[a:b])).to(gpu).contiguous(), KW["mask_dilation_iter"]).cpu().numpy()
            ref = O.diffueraser_forward(frames[a:b], list(dil), prior[a:b], max_img_size=KW["max_img_size"], steps=2, chunk=4, overlap=2, seed=3,
                                        ucfg=TINY_UNET, vcfg=TINY_VAE)
            for t in range(b - a):
                r = ref[t] if ref[t].shape[:2] == (H, W) else O.I.resize_bilinear_u8(ref[t], W, H)
                r = O.I.composite(r, frames[a + t], O.I.feather_alpha(dil[t], FEATHER))
                du = np.abs(out[a + t].astype(int) - r.astype(int))
                assert du.max() <= 4, (t, int(du.max()))
    finally:
        diffuerase.configure(None)


def test_spans_with_roi_cuts_detector_and_reference_windows(gpu):
    import dataclasses
    import diffuerase
    from videovanish_amd import hip, spans_hip
    frames, masks, prior = _clip()
    diffuerase.configure(RUN)
    try:
        # a window per span
        roi = RoiConfig("follow", context=0.25, pad_min=8, min_side=32, smooth=1)
        _check_spans(frames, masks, prior, [(1, 5), (7, 12)], SPANS, roi=roi)
        # explicit cuts=: a cut inside the second masked run; nothing crosses it
        plan = plan_spans(_masked(masks), [9], SPANS)
        assert len(plan) >= 2 and any(a == 9 for a, _ in plan) and any(b == 9 for _, b in plan)
        _check_spans(frames, masks, prior, plan, SPANS, cuts=[9])
        _check_spans(frames, masks, prior, plan, dataclasses.replace(SPANS, cuts="auto"), cuts=[9])      # explicit cuts override the detector
        # "cuts": every frame, split where the detector finds the cut on the device
        dil = hip.mask_collapse_dilate(torch.from_numpy(np.stack(masks)).to(gpu).contiguous(), KW["mask_dilation_iter"])
        sad, n, hist = spans_hip.frame_pair_stats(frames, dil)
        assert find_cuts(sad, n, hist, SpanConfig("all", cuts="auto"), npix=H * W) == [CUT]
        progs = []
        _check_spans(frames, masks, prior, [(0, CUT), (CUT, T)], "cuts", progs)
        _protocol(progs, True, 2)
        # "masked-cuts" with this clip's lengths: the same spans as "masked" (the cut lies between them)
        assert plan_spans(_masked(masks), [CUT], SPANS) == [(1, 5), (7, 12)]
    finally:
        diffuerase.configure(None)
    diffuerase.configure(dataclasses.replace(RUN, windowing="reference"))
    try:
        _check_spans(frames, masks, prior, [(1, 5), (7, 12)], SPANS)
    finally:
        diffuerase.configure(None)


def test_special_paths_and_determinism(gpu):
    import diffuerase
    frames, masks, prior = _clip()
    diffuerase.configure(RUN)
    try:
        # no mask pixel: the inputs come back, nothing is loaded, the milestones are still delivered
        diffuerase.video_inpainting_sd = None
        progs = []
        empty = [np.zeros_like(m) for m in masks]
        for spans in ("masked", "masked-cuts"):
            out = diffuerase.run_infill_on_frames(frames, empty, spans=spans, prog=lambda p, s: progs.append((p, s)), **KW)
            assert len(out) == T and all((o == f).all() for o, f in zip(out, frames))
            assert diffuerase.video_inpainting_sd is None
        assert [p for p, _ in progs] == [5, 10, 20, 50, 90] * 2 and all(s for _, s in progs)
        # a plan of one span that is the whole clip: the plain call, byte for byte
        plain = diffuerase.run_infill_on_frames(frames[:6], masks[:6], propainer_frames=prior[:6], **KW)
        assert plan_spans(_masked(masks[:6]), None, SpanConfig("masked", context=2, min_len=3, min_gap=2)) == [(0, 6)]
        for spans in (SpanConfig("masked", context=2, min_len=3, min_gap=2), SpanConfig("all"), "cuts"):
            one = diffuerase.run_infill_on_frames(frames[:6], masks[:6], propainer_frames=prior[:6], spans=spans, **KW)
            assert (np.stack(one) == np.stack(plain)).all()
        # two runs are identical
        a = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, spans=SPANS, **KW)
        b = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, spans=SPANS, **KW)
        assert (np.stack(a) == np.stack(b)).all()
        assert not (np.stack(a)[8:11] == np.stack(frames)[8:11]).all()
    finally:
        diffuerase.configure(None)
