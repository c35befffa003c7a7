"""Seam tone matching on the GPU: the two entry points of vv_tone.hip against the numpy / scipy restatement (tests/tonematch_ref.py) byte for byte,
each run twice with identical bytes; infill.finish with the stage on against the restatement and against the original it has to restore; and
the drop-in's tone_match= path on the tiny architecture against the restatement applied to the model's own frames.  No tolerances."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tonematch_ref as R  # noqa: E402
import spans_ref  # noqa: E402

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.roi import RoiConfig, RoiPlan, plan_roi  # noqa: E402
from videovanish_amd.spans import SpanConfig  # noqa: E402
from videovanish_amd.tonematch import ToneMatchConfig  # noqa: E402

IDENT = np.broadcast_to(np.arange(256, dtype=np.uint8), (3, 256))


def _d(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _twice(fn):
    """fn() -> a tensor; run twice, identical bytes; the first run's result as a numpy array."""
    a, b = fn().cpu().numpy(), fn().cpu().numpy()
    assert (a == b).all()
    return a


def _stats(patch, orig, mask, offs, h, w, ring, gpu):
    from videovanish_amd import tone_hip
    args = [_d(a, gpu) for a in (patch, orig, mask, np.asarray(offs, np.int32))]
    got = _twice(lambda: tone_hip.ring_stats(*args, h, w, ring))
    want = R.sums(patch, orig, mask, offs, h, w, ring)
    assert got.dtype == np.int64 and got.shape == (len(patch), 16)
    assert (got == want).all(), (ring, got[:, 0].tolist(), want[:, 0].tolist())
    return want


# ---- ring_stats ---------------------------------------------------------------------------------------------------------------------------
def _frame_masks(H, W, seed):
    """Nine masks [H,W]: empty, full, one pixel in two corners, a bar along each frame edge (two frames), two blobs whose ring leaves the frame,
    random at density 0.02."""
    rng = np.random.default_rng(seed)
    m = np.zeros((9, H, W), np.uint8)
    m[1] = 255
    m[2, 0, 0] = 1
    m[3, :2, :] = 255
    m[3, :, :3] = 7                                  # top and left
    m[4, H - 1:, :] = 255
    m[4, :, W - 2:] = 255                            # bottom and right
    m[5, H // 3: H // 3 + 9, W - 7:W - 2] = 200      # next to the right edge
    m[6] = (rng.random((H, W)) < 0.02) * rng.integers(1, 256, (H, W))
    m[7, H - 1, W - 1] = 255
    m[8, 1:6, W // 2: W // 2 + 11] = 255             # next to the top edge
    return m


@pytest.mark.parametrize("ring", [1, 12, 32])
@pytest.mark.parametrize("H,W", [(37, 53), (96, 130)])
def test_ring_stats_full_frame(gpu, H, W, ring):
    """The full frame is the window (0, 0, H, W) of a patch of the frame's size.  W is a multiple of neither 16 nor 64: tiles end inside the frame."""
    rng = np.random.default_rng(H * 100 + ring)
    masks = _frame_masks(H, W, H + ring)
    n = []
    for a in range(0, 9, 3):
        orig = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        patch = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        n += _stats(patch, orig, masks[a:a + 3], np.zeros((3, 2), np.int32), H, W, ring, gpu)[:, 0].tolist()
    print("ring pixels:", n)
    assert n[0] == 0 and n[1] == 0 and n[2] == (ring + 1) ** 2 - 1 and n[7] == (ring + 1) ** 2 - 1 and all(v > 0 for v in n[2:])


@pytest.mark.parametrize("ring", [1, 12, 32])
def test_ring_stats_window(gpu, ring):
    """A 40 x 56 model output resized to a 48 x 64 window of a 96 x 130 frame; per-frame offsets with (0, 0) and the bottom-right corner; a mask
    that ends 3 pixels from the window's edge (the ring is clipped by the window), a mask pixel outside the window within `ring` of pixels
    inside it, and a random mask over the whole frame."""
    H, W, h, w, Hm, Wm = 96, 130, 48, 64, 40, 56
    rng = np.random.default_rng(ring)
    orig = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    patch = rng.integers(0, 256, (3, Hm, Wm, 3), dtype=np.uint8)
    offs = np.array([[0, 0], [H - h, W - w], [20, 31]], np.int32)
    mask = np.zeros((3, H, W), np.uint8)
    mask[0, 10:30, 50:61] = 255
    mask[0, 50, 70] = 255                            # outside the window (rows < 48, columns < 64), 3 rows and 7 columns away
    mask[1, 60:80, 100:126] = 9
    mask[1, 45, 60] = 255                            # outside the window (rows >= 48, columns >= 66)
    mask[2] = (rng.random((H, W)) < 0.02) * 255
    want = _stats(patch, orig, mask, offs, h, w, ring, gpu)
    # the pixel outside the window counts for the ring, the pixels outside the window do not belong to it
    lone = mask.copy()
    lone[0, 10:30, 50:61] = 0
    n = _stats(patch, orig, lone, offs, h, w, ring, gpu)[0, 0]
    assert n == (max(0, ring - 2) * max(0, ring - 6) if ring > 6 else 0)
    inside = np.zeros((H, W), bool)
    inside[:h, :w] = True
    assert want[0, 0] == (R.ring(mask[0], (0, 0, H, W), ring) & inside).sum() < R.ring(mask[0], (0, 0, H, W), ring).sum()
    # the same window without the resize, and the whole frame as the window of a smaller patch
    _stats(rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8), orig, mask, offs, h, w, ring, gpu)
    _stats(patch, orig, mask, np.zeros((3, 2), np.int32), H, W, ring, gpu)


def test_ring_stats_sums_are_64_bit(gpu):
    """One 272 x 272 frame with x = y = 255 and mask pixels on a 33-pixel lattice: at ring 16 every other pixel belongs to the ring, and the sums
    of squares pass 2^32."""
    H = W = 272
    orig = np.full((1, H, W, 3), 255, np.uint8)
    mask = np.zeros((1, H, W), np.uint8)
    mask[0, ::33, ::33] = 255
    want = _stats(orig.copy(), orig, mask, np.zeros((1, 2), np.int32), H, W, 16, gpu)
    n = H * W - 81
    assert want[0].tolist() == [n] + [255 * n] * 6 + [65025 * n] * 9 and 65025 * n > 2 ** 32


# ---- paste_lut_composite ------------------------------------------------------------------------------------------------------------------
def _paste_inputs(seed, full, resize):
    T, H, W = 4, 50, 70
    h, w = (H, W) if full else (24, 32)
    Hm, Wm = ((40, 56) if full else (16, 24)) if resize else (h, w)
    rng = np.random.default_rng(seed)
    orig = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    patch = rng.integers(0, 256, (T, Hm, Wm, 3), dtype=np.uint8)
    mask = ((rng.random((T, H, W)) > 0.93) * 255).astype(np.uint8)
    mask[:, 10:30, 20:40] = 255
    offs = np.zeros((T, 2), np.int32) if full else np.array([[0, 0], [0, W - w], [H - h, 0], [H - h, W - w]], np.int32)
    return patch, orig, mask, offs, h, w


@pytest.mark.parametrize("feather", [3.0, 0.0, -1.0])
@pytest.mark.parametrize("resize", [False, True])
@pytest.mark.parametrize("full", [False, True])
def test_paste_lut_composite(gpu, full, resize, feather):
    from videovanish_amd import hip, tone_hip
    patch, orig, mask, offs, h, w = _paste_inputs(3 + 2 * full + resize, full, resize)
    T = len(patch)
    dp, do, dm, df = (_d(a, gpu) for a in (patch, orig, mask, offs))
    # the identity table: the bytes of roi_paste_composite
    ident = _d(np.broadcast_to(IDENT, (T, 3, 256)), gpu)
    got = _twice(lambda: tone_hip.paste_lut_composite(dp, do, dm, df, ident, h, w, feather))
    assert (got == hip.roi_paste_composite(dp, do, dm, df, h, w, feather).cpu().numpy()).all()
    # random tables: the reference
    lut = np.random.default_rng(9).integers(0, 256, (T, 3, 256), dtype=np.uint8)
    dl = _d(lut, gpu)
    got = _twice(lambda: tone_hip.paste_lut_composite(dp, do, dm, df, dl, h, w, feather))
    want = R.composite(patch, orig, mask, offs, lut, h, w, feather)
    assert (got == want).all() and not (got == hip.roi_paste_composite(dp, do, dm, df, h, w, feather).cpu().numpy()).all()
    if feather < 0:
        assert (tone_hip.paste_lut_composite(dp, do, None, df, dl, h, w, feather).cpu().numpy() == want).all()      # the plain paste needs no mask
    if full:                                                                                                         # the chain the full-frame path replaces
        rs = hip.resize_u8(dp, h, w).cpu().numpy() if resize else patch
        looked = np.stack([np.stack([lut[t, c][rs[t, ..., c]] for c in range(3)], -1) for t in range(T)])
        chain = looked if feather < 0 else hip.feather_composite(_d(looked, gpu), do, dm, feather).cpu().numpy()
        assert (got == chain).all()
    buf = torch.empty_like(do)
    assert tone_hip.paste_lut_composite(dp, do, dm, df, dl, h, w, feather, out=buf) is buf and (buf.cpu().numpy() == want).all()


def test_refusals_launch_nothing(gpu):
    from videovanish_amd import tone_hip
    lib = tone_hip.lib()
    u8 = lambda *shape: torch.full(shape, 7, dtype=torch.uint8, device=gpu)
    patch, orig, mask, lut, out = u8(2, 8, 8, 3), u8(2, 8, 8, 3), u8(2, 8, 8), u8(2, 3, 256), u8(2, 8, 8, 3)
    offs = torch.zeros((2, 2), dtype=torch.int32, device=gpu)
    sums = torch.full((2, 16), 7, dtype=torch.int64, device=gpu)
    p = lambda t: t.data_ptr()
    assert [lib.vvt_ring_stats(p(patch), 8, 8, p(orig), p(mask), p(offs), 2, 8, 8, 8, 8, ring, p(sums), None) for ring in (0, 33)] == [-2, -2]
    assert lib.vvt_ring_stats(p(patch), 8, 8, p(orig), None, p(offs), 2, 8, 8, 8, 8, 4, p(sums), None) == -1
    assert lib.vvt_ring_stats(p(patch), 8, 8, p(orig), p(mask), p(offs), 2, 8, 8, 9, 8, 4, p(sums), None) == -1
    assert lib.vvt_paste_lut_composite(p(patch), 8, 8, p(orig), p(mask), p(offs), p(lut), 2, 8, 8, 8, 8, 64.5, p(out), None) == -2
    assert lib.vvt_paste_lut_composite(p(patch), 8, 8, p(orig), None, p(offs), p(lut), 2, 8, 8, 8, 8, 3.0, p(out), None) == -1
    assert lib.vvt_paste_lut_composite(p(patch), 8, 8, p(orig), p(mask), p(offs), None, 2, 8, 8, 8, 8, 3.0, p(out), None) == -1
    torch.cuda.synchronize()
    assert (sums == 7).all() and (out == 7).all()                                                   # nothing was launched, nothing cleared
    with pytest.raises(RuntimeError, match="ring 1 .. 32"):
        tone_hip.ring_stats(patch, orig, mask, offs, 8, 8, 33)
    with pytest.raises(RuntimeError):
        tone_hip.ring_stats(patch.cpu(), orig, mask, offs, 8, 8, 4)                                 # no CPU fallback
    with pytest.raises(RuntimeError, match="not orig itself"):
        tone_hip.paste_lut_composite(patch, orig, mask, offs, lut, 8, 8, 3.0, out=orig)


# ---- infill.finish ------------------------------------------------------------------------------------------------------------------------
CFG = ToneMatchConfig()
FIT = dict(mode=CFG.mode, ring=CFG.ring, smooth=CFG.smooth, max_gain=CFG.max_gain, max_offset=CFG.max_offset, min_count=CFG.min_count, min_var=CFG.min_var)


def _report_equals(rep, k, s, gain, offset, a=0, b=None):
    b = a + len(s) if b is None else b
    rb, ra = R.rms(s, gain, offset)
    assert (rep.n[k, a:b] == s[:, 0]).all() and (rep.gain[k, a:b] == gain).all() and (rep.offset[k, a:b] == offset).all()
    assert np.allclose(rep.rms_before[k, a:b], rb, rtol=1e-9, atol=1e-6) and np.allclose(rep.rms_after[k, a:b], ra, rtol=1e-9, atol=1e-6)


@pytest.mark.parametrize("a,b", R.RESTORE_CASES)
def test_finish_restores_a_known_tone_shift(gpu, a, b):
    """The restoration inputs of the CPU test through infill.finish on the full frame: the composite is within one level of the original where
    the model's pixels show (ring and mask; elsewhere it IS the original), where the plain composite is at least 6 off."""
    from videovanish_amd import infill
    orig, x, mask = R.restoration_clip(a, b)
    T, H, W = mask.shape
    dil = _d(mask, gpu)
    plain = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu))
    rows = []
    out = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu, tone=CFG, tone_out=rows))
    want, s, gain, offset = R.apply(x, orig, mask, np.zeros((T, 2), np.int32), H, W, 3.0, **FIT)
    assert (out == want).all()
    err = lambda f: int(np.abs(f.astype(int) - orig.astype(int)).max())
    print(f"a = {a}, b = {b}: worst error of the composite {err(plain)} -> {err(out)}; gain {rows[0].gain[0, 0].round(4).tolist()}")
    assert err(plain) >= 6 and err(out) <= 1 and (err(out) == 0 or (a, b) != (1.0, 6))
    assert len(rows) == 1 and rows[0].n.shape == (1, T) and rows[0].gain.shape == (1, T, 3) and rows[0].n.dtype == np.int64
    _report_equals(rows[0], 0, s, gain, offset)
    assert (rows[0].rms_after < rows[0].rms_before).all() and (s[:, 0] > 2000).all()
    # keep_unmasked_original=False: every pixel of the frame goes through the table
    out = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, False, gpu, tone=CFG))
    assert (out == R.apply(x, orig, mask, np.zeros((T, 2), np.int32), H, W, -1.0, **FIT)[0]).all() and err(out) <= 1


def test_finish_two_windows_are_fitted_independently(gpu):
    """K = 2: two disjoint windows whose model frames carry different tone shifts; each is fitted on its own ring and restored."""
    from videovanish_amd import infill
    orig, _, _ = R.restoration_clip(1.0, 0)
    T, H, W = orig.shape[:3]
    wins = [((0, 0), (48, 64), (12, 15, 30, 40), (0.9, 10)), ((50, 70), (40, 56), (60, 85, 75, 110), (1.2, -25))]
    mask = np.zeros((T, H, W), np.uint8)
    plans, outs = [], []
    for (oy, ox), (h, w), (y0, x0, y1, x1), (a, b) in wins:
        mask[:, y0:y1, x0:x1] = 255
        offs = np.tile(np.array([[oy, ox]], np.int32), (T, 1))
        plans.append(RoiPlan("static", (h, w), offs, offs.astype(np.float64)))
        outs.append(list(np.clip(np.rint(a * orig[:, oy:oy + h, ox:ox + w].astype(np.float64) + b), 0, 255).astype(np.uint8)))
    rows = []
    out = np.stack(infill.finish(outs, list(orig), _d(mask, gpu), plans, 3, True, gpu, tone=CFG, tone_out=rows))
    want = orig
    assert len(rows) == 1 and rows[0].n.shape == (2, T)
    for k, (plan, o) in enumerate(zip(plans, outs)):
        want, s, gain, offset = R.apply(np.stack(o), want, mask, plan.offsets, *plan.size, 3.0, **FIT)
        _report_equals(rows[0], k, s, gain, offset)
    assert (out == want).all()
    assert np.abs(out.astype(int) - orig.astype(int)).max() <= 1
    assert np.abs(rows[0].gain[0] - 1 / 0.9).max() < 0.01 and np.abs(rows[0].gain[1] - 1 / 1.2).max() < 0.01
    assert (rows[0].rms_after < rows[0].rms_before).all()
    plain = np.stack(infill.finish(outs, list(orig), _d(mask, gpu), plans, 3, True, gpu))
    assert np.abs(plain.astype(int) - orig.astype(int)).max() >= 6


def test_finish_two_windows_without_a_stage_is_the_paste_by_hand(gpu):
    """No stage, K = 2: finish returns the bytes of hip.roi_paste_composite applied window after window, the feathered composite and the plain
    paste."""
    from videovanish_amd import hip, infill
    orig, _, _ = R.restoration_clip(1.0, 0)
    T, H, W = orig.shape[:3]
    mask = np.zeros((T, H, W), np.uint8)
    plans, outs = [], []
    for (oy, ox), (h, w), (y0, x0, y1, x1), (a, b) in [((0, 0), (48, 64), (12, 15, 30, 40), (0.9, 10)), ((50, 70), (40, 56), (60, 85, 75, 110), (1.2, -25))]:
        mask[:, y0:y1, x0:x1] = 255
        offs = np.tile(np.array([[oy, ox]], np.int32), (T, 1))
        plans.append(RoiPlan("static", (h, w), offs, offs.astype(np.float64)))
        outs.append(list(np.clip(np.rint(a * orig[:, oy:oy + h, ox:ox + w].astype(np.float64) + b), 0, 255).astype(np.uint8)))
    for keep, feather in ((True, 3.0), (False, -1.0)):
        out = np.stack(infill.finish(outs, list(orig), _d(mask, gpu), plans, 3, keep, gpu))
        want = _d(orig, gpu)
        for plan, o in zip(plans, outs):
            want = hip.roi_paste_composite(_d(np.stack(o), gpu), want, _d(mask, gpu), _d(plan.offsets, gpu), *plan.size, feather)
        assert (out == want.cpu().numpy()).all() and (out != orig).any()


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=960, num_inference_steps=2, scheduler="ddim")
T, H, W = 14, 96, 160
ROI = RoiConfig("static", context=0.25, pad_min=8, min_side=32)
SPANS = SpanConfig("masked", context=1, min_len=3, min_gap=2)


@pytest.fixture(scope="module")
def clip():
    """A static box in frames 2 .. 10 of a panning shot, and a prior."""
    frames, _ = spans_ref.shots_clip(61, (T,), (3,), H, W)
    masks = [np.zeros((H, W, 3), np.uint8) for _ in range(T)]
    for t in range(2, 11):
        masks[t][30:52, 40:76] = 255
    prior = []
    for f, m in zip(frames, masks):
        p = f.copy()
        p[m[..., 0] > 0] = f.reshape(-1, 3).mean(0).astype(np.uint8)
        prior.append(p)
    return frames, masks, prior


@pytest.fixture(scope="module")
def run(gpu, clip):
    """run(**kw) -> (output frames, last_tone_match, the model's frames of every stages.run_model call) of the drop-in on the tiny architecture;
    the results are kept, so every distinct call of this module runs once."""
    import diffuerase
    frames, masks, prior = clip
    seen = {}

    def call(**kw):
        key = repr(sorted(kw.items()))
        if key not in seen:
            model, inner = [], diffuerase._run_model

            def wrapped(*a, **k):
                frames_out = inner(*a, **k)
                model.append(list(frames_out))                      # a copy of the list: the full-frame finish() writes its frames into it
                return frames_out

            diffuerase.configure(RUN)
            diffuerase._run_model = wrapped
            try:
                out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, feather_px=3, **KW, **kw)
                seen[key] = (out, diffuerase.last_tone_match, [np.stack(m) for m in model])
            finally:
                diffuerase._run_model = inner
                diffuerase.configure(None)
        return seen[key]
    return call


@pytest.fixture(scope="module")
def dil(gpu, clip):
    from videovanish_amd import hip
    return hip.mask_collapse_dilate(_d(np.stack(clip[1]), gpu), KW["mask_dilation_iter"]).cpu().numpy()


def test_drop_in_full_frame_equals_the_reference_on_the_models_frames(gpu, clip, run, dil):
    from oracle import imageops_ref as I
    frames, masks, prior = clip
    base, none, _ = run()
    out, rep, model = run(tone_match="on")
    assert none is None and len(model) == 1 and len(out) == T
    want, s, gain, offset = R.apply(model[0], np.stack(frames), dil, np.zeros((T, 2), np.int32), H, W, 3.0, **FIT)
    assert (np.stack(out) == want).all()
    assert rep.n.shape == (1, T) and rep.gain.shape == rep.offset.shape == rep.rms_before.shape == rep.rms_after.shape == (1, T, 3)
    _report_equals(rep, 0, s, gain, offset)
    assert (rep.n[0, 2:11] > 500).all() and not rep.n[0, [0, 1, 11, 12, 13]].any() and (rep.gain[0, [0, 1, 11, 12, 13]] == 1.0).all()
    assert (rep.gain[0, 2:11] != 1.0).any() or (rep.offset[0, 2:11] != 0.0).any()                   # random weights do not reproduce the surroundings
    # the stage moves only pixels the composite takes from the model
    alpha = np.stack([I.feather_alpha(d, 3) for d in dil])
    differs = (np.stack(out) != np.stack(base)).any(-1)
    assert differs.any() and not differs[alpha == 0].any()


def test_drop_in_with_a_window(gpu, clip, run, dil):
    frames, masks, prior = clip
    out, rep, model = run(tone_match="on", roi=ROI)
    bb = np.zeros((T, 4), np.int32)
    for t in range(T):
        ys, xs = np.nonzero(dil[t])
        if len(ys):
            bb[t] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
    plan = plan_roi(bb, H, W, 3, ROI)
    h, w = plan.size
    assert h < H and w < W and len(model) == 1 and model[0].shape[0] == T
    want, s, gain, offset = R.apply(model[0], np.stack(frames), dil, plan.offsets, h, w, 3.0, **FIT)
    assert (np.stack(out) == want).all()
    _report_equals(rep, 0, s, gain, offset)
    inside = np.zeros((T, H, W), bool)
    for t, (oy, ox) in enumerate(plan.offsets.tolist()):
        inside[t, oy:oy + h, ox:ox + w] = True
    assert (np.stack(out)[~inside] == np.stack(frames)[~inside]).all() and (~inside).any()        # outside the window: the original bytes
    assert not (np.stack(out) == np.stack(run(roi=ROI)[0])).all()


def test_drop_in_with_spans(gpu, clip, run, dil):
    frames, masks, prior = clip
    out, rep, model = run(tone_match="on", spans=SPANS)
    outside = [0, 12, 13]
    assert all(out[t] is frames[t] for t in outside) and not any(out[t] is frames[t] for t in range(1, 12))
    assert rep.n.shape == (1, T) and not rep.n[0, outside].any() and (rep.gain[0, outside] == 1.0).all() and not rep.offset[0, outside].any()
    assert not rep.rms_before[0, outside].any() and not rep.rms_after[0, outside].any()
    assert len(model) == 1 and len(model[0]) == 11
    want, s, gain, offset = R.apply(model[0], np.stack(frames[1:12]), dil[1:12], np.zeros((11, 2), np.int32), H, W, 3.0, **FIT)
    assert (np.stack(out[1:12]) == want).all()
    _report_equals(rep, 0, s, gain, offset, a=1)


def test_drop_in_off_is_the_plain_call(gpu, clip, run):
    base, none, _ = run()
    off, rep, _ = run(tone_match="off")
    assert none is None and rep is None and (np.stack(off) == np.stack(base)).all()
