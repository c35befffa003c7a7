"""Inpaint deflicker on the GPU: the entry points of vv_flicker.hip against the numpy restatement (tests/deflicker_ref.py) byte for byte, each run
twice with identical bytes; and the drop-in's deflicker= path on the tiny architecture: radius=0 against the call without the option (the
materialised resize against the fused one), and the stage against the same call with the device functions replaced by the restatement.
No tolerances."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflicker_ref as R  # noqa: E402
import spans_ref  # noqa: E402

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.roi import RoiConfig  # noqa: E402
from videovanish_amd.spans import SpanConfig  # noqa: E402

TS = (1, 2, 15, 16, 17, 33)         # round the slab edge (VVF_SLAB = 16) and below 2 radius + 1
RADII = (0, 1, 2, 4)
TOLS = (0, 6, 255)


def _d(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _clip(seed, T, h, w, H0, W0, offsets):
    """One textured background fixed in the frame, seen through the windows, with +-5 levels of flicker, a block that changes for good half way
    (a real change: beyond tol = 6), flat runs (equal samples at tol = 0) and a mask of random bytes over a third of the frame."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H0, W0, 3))
    base[: H0 // 3] = base[: H0 // 3] // 64 * 64
    win = np.stack([base[oy:oy + h, ox:ox + w] for oy, ox in offsets]) + rng.integers(-5, 6, (T, h, w, 3)) * (rng.random((T, h, w, 1)) < 0.8)
    win[T // 2:, h // 4: h // 2, w // 3:] += 40
    mask = (rng.random((T, H0, W0)) < 0.33) * rng.integers(1, 256, (T, H0, W0))
    return np.clip(win, 0, 255).astype(np.uint8), mask.astype(np.uint8)


def _hold_twice(win, offs, mask, radius, tol, fixed, gpu):
    from videovanish_amd import flicker_hip
    args = (_d(win, gpu), _d(np.asarray(offs, np.int32), gpu), _d(mask, gpu))
    a, b = (flicker_hip.hold(*args, radius, tol, fixed=fixed) for _ in range(2))
    out, sums = a[0].cpu().numpy(), a[1].cpu().numpy()
    assert (out == b[0].cpu().numpy()).all() and (sums == b[1].cpu().numpy()).all()
    assert out.dtype == np.uint8 and out.shape == win.shape and sums.dtype == np.int64 and sums.shape == (len(win), 12)
    return out, sums


def _against_the_restatement(win, offs, mask, fixed, gpu, radii=RADII, tols=TOLS):
    for radius in radii:
        for tol in tols:
            out, sums = _hold_twice(win, offs, mask, radius, tol, fixed, gpu)
            want, wsums = R.hold(win, offs, mask, radius, tol)
            assert (out == want).all(), (radius, tol, int((out != want).sum()))
            assert (sums == wsums).all(), (radius, tol, sums[0].tolist(), wsums[0].tolist())
            if radius and tol:
                assert sums[:, 1].any() == (len(win) > 1)


# ---- vvf_hold, the fixed form -----------------------------------------------------------------------------------------------------------
# (h, w, H0, W0, oy, ox): the full frame below one tile of 256 x 4 pixels; several tiles with a row tail, as a window at an odd place (the mask
# bytes one by one), at an aligned place (one dword) and in a frame whose width is no multiple of 4
FIXED = [(40, 56, 40, 56, 0, 0), (96, 132, 96, 132, 0, 0), (96, 132, 101, 140, 3, 5), (40, 56, 64, 96, 12, 8), (40, 56, 50, 70, 10, 14)]


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("h,w,H0,W0,oy,ox", FIXED[:3])
def test_hold_fixed_form(gpu, h, w, H0, W0, oy, ox, T):
    offs = np.tile([[oy, ox]], (T, 1))
    win, mask = _clip(T * 1000 + h, T, h, w, H0, W0, offs)
    _against_the_restatement(win, offs, mask, True, gpu)


@pytest.mark.parametrize("h,w,H0,W0,oy,ox", FIXED[3:])
def test_hold_fixed_form_mask_paths(gpu, h, w, H0, W0, oy, ox):
    offs = np.tile([[oy, ox]], (17, 1))
    win, mask = _clip(3, 17, h, w, H0, W0, offs)
    _against_the_restatement(win, offs, mask, True, gpu, radii=(2,), tols=(6,))


# ---- vvf_hold, the gather form ----------------------------------------------------------------------------------------------------------
def _moving_offsets(T, h, w, H0, W0, seed):
    """Offsets that move by 0 .. 3 px per frame, bounce off the frame's edges and touch them."""
    rng = np.random.default_rng(seed)
    o = np.zeros((T, 2), np.int64)
    o[0] = (H0 - h, 0)                                                                              # bottom left corner
    d = np.array([-1, 1])
    for t in range(1, T):
        for a, lim in ((0, H0 - h), (1, W0 - w)):
            v = o[t - 1, a] + d[a] * rng.integers(0, 4)
            if v < 0 or v > lim:
                d[a] = -d[a]
                v = min(max(v, 0), lim)
            o[t, a] = v
    return o.astype(np.int32)


@pytest.mark.parametrize("T", TS)
def test_hold_gather_form_odd_width(gpu, T):
    offs = np.tile([[2, 3]], (T, 1))
    win, mask = _clip(T, T, 45, 83, 50, 90, offs)
    thin = dict(radii=RADII, tols=TOLS) if T == 17 else dict(radii=(2, 4) if T % 2 else (1, 4), tols=(6,))
    _against_the_restatement(win, offs, mask, True, gpu, **thin)                                    # "fixed" alone does not make the fixed form: w % 4 != 0


@pytest.mark.parametrize("T", TS)
def test_hold_gather_form_moving_windows(gpu, T):
    offs = _moving_offsets(T, 40, 56, 64, 96, T)
    assert offs[:, 0].max() == 24 and offs[:, 1].min() == 0 and (T < 33 or (offs[:, 0].min() == 0 and len(np.unique(offs, axis=0)) > T // 2))
    win, mask = _clip(T + 7, T, 40, 56, 64, 96, offs)
    thin = dict(radii=RADII, tols=TOLS) if T == 17 else dict(radii=(2, 4) if T % 2 else (1, 4), tols=(6,))
    _against_the_restatement(win, offs, mask, False, gpu, **thin)


def test_both_forms_agree(gpu):
    """On an input both accept, the C entry with the binding's "fixed" flag off (the gather form) gives the fixed form's bytes."""
    from videovanish_amd import flicker_hip, hip
    T, h, w, H0, W0 = 33, 96, 132, 101, 140
    offs = np.tile([[3, 4]], (T, 1)).astype(np.int32)
    win, mask = _clip(11, T, h, w, H0, W0, offs)
    win_t, offs_t, mask_t = _d(win, gpu), _d(offs, gpu), _d(mask, gpu)
    for radius, tol in ((1, 6), (2, 12), (4, 255)):
        fixed = flicker_hip.hold(win_t, offs_t, mask_t, radius, tol, fixed=True)
        out, sums = torch.empty_like(win_t), torch.empty((T, 12), dtype=torch.int64, device=gpu)
        rc = flicker_hip.lib().vvf_hold(hip._p(win_t), hip._p(offs_t), hip._p(mask_t), T, H0, W0, h, w, radius, tol, 0, hip._p(out), hip._p(sums),
                                        hip._stream())
        assert rc == 0
        assert (out == fixed[0]).all() and (sums == fixed[1]).all()
        assert (flicker_hip.hold(win_t, offs_t, mask_t, radius, tol)[0] == out).all()              # fixed=None: the caller has not looked


# ---- vvf_window_pixels ------------------------------------------------------------------------------------------------------------------
def test_window_pixels(gpu):
    from videovanish_amd import flicker_hip, hip
    rng = np.random.default_rng(4)
    patch = _d(rng.integers(0, 256, (5, 24, 40, 3), dtype=np.uint8), gpu)
    a, b = flicker_hip.window_pixels(patch, 40, 56), flicker_hip.window_pixels(patch, 40, 56)
    assert a.shape == (5, 40, 56, 3) and (a == b).all() and (a == hip.resize_u8(patch, 40, 56, mode="bilinear")).all()
    assert (a.cpu().numpy() == R.window_pixels(patch.cpu().numpy(), 40, 56)).all()
    assert flicker_hip.window_pixels(patch, 24, 40) is patch                                         # equal size: nothing is launched
    down = flicker_hip.window_pixels(patch, 13, 21)
    assert (down == hip.resize_u8(patch, 13, 21, mode="bilinear")).all()


# ---- every byte of out is written, nothing outside it -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fixed", "gather"])
def test_poisoned_out(gpu, form):
    from videovanish_amd import flicker_hip
    T, H0, W0 = 17, 64, 96
    h, w = (40, 56) if form == "fixed" else (41, 55)
    offs = np.tile([[5, 7]], (T, 1)) if form == "fixed" else _moving_offsets(T, h, w, H0, W0, 2)
    win, mask = _clip(9, T, h, w, H0, W0, offs)
    want, wsums = R.hold(win, offs, mask, 2, 6)
    n, G = win.size, 4096
    for poison in (0x00, 0xFF):
        buf = torch.full((n + 2 * G,), poison, dtype=torch.uint8, device=gpu)
        out, sums = flicker_hip.hold(_d(win, gpu), _d(np.asarray(offs, np.int32), gpu), _d(mask, gpu), 2, 6, fixed=form == "fixed",
                                     out=buf[G:G + n].view(win.shape))
        assert out.data_ptr() == buf.data_ptr() + G
        assert (out.cpu().numpy() == want).all() and (sums.cpu().numpy() == wsums).all()
        assert (buf[:G] == poison).all() and (buf[G + n:] == poison).all()


def test_refusals_launch_nothing(gpu):
    from videovanish_amd import flicker_hip
    win, offs, mask = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=gpu), torch.zeros((2, 2), dtype=torch.int32, device=gpu), \
        torch.zeros((2, 8, 8), dtype=torch.uint8, device=gpu)
    for bad in (lambda: flicker_hip.hold(win, offs, mask, 5, 12), lambda: flicker_hip.hold(win, offs, mask, 2, 256),
                lambda: flicker_hip.hold(win, offs, mask[:, :7].contiguous(), 2, 12), lambda: flicker_hip.hold(win, offs, mask, 2, 12, out=win),
                lambda: flicker_hip.hold(win, offs[:1], mask, 2, 12), lambda: flicker_hip.hold(win.cpu(), offs, mask, 2, 12)):
        with pytest.raises(RuntimeError):
            bad()
    torch.cuda.synchronize()


# ---- the drop-in on the tiny architecture ---------------------------------------------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=80, num_inference_steps=2, scheduler="ddim")         # the model runs at 48 x 80, the frame is 96 x 160
T, H, W = 9, 96, 160
FOLLOW = RoiConfig("follow", context=0.25, pad_min=8, min_side=32, smooth=1)
REGIONS = RoiConfig("follow", context=0.25, pad_min=8, min_side=32, smooth=1, max_regions=8)
SPANS = SpanConfig("masked", context=1, min_len=3, min_gap=2)
BOXES = [(6, 18, 6, 30, 2), (70, 86, 124, 148, -2)]          # top left moving right, bottom right moving left, in frames 2 .. 6


@pytest.fixture(scope="module")
def clip():
    frames, _ = spans_ref.shots_clip(61, (T,), (3,), H, W)
    masks, prior = [], []
    for t in range(T):
        m = np.zeros((H, W, 3), np.uint8)
        if 2 <= t <= 6:
            for y0, y1, x0, x1, vx in BOXES:
                m[y0:y1, x0 + vx * t: x1 + vx * t] = 255
        masks.append(m)
        p = frames[t].copy()
        p[m[..., 0] > 0] = frames[t].reshape(-1, 3).mean(0).astype(np.uint8)
        prior.append(p)
    return frames, masks, prior


@pytest.fixture(scope="module")
def run(gpu, clip):
    """run(**kw) -> (output frames, last_deflicker, whether flicker_hip resolved its symbols) of the drop-in on the tiny architecture; the results
    are kept, so every distinct call of this module runs once.  host=True: flicker_hip's two functions are the restatement."""
    import diffuerase
    from videovanish_amd import flicker_hip
    frames, masks, prior = clip
    seen = {}

    def call(host=False, **kw):
        key = repr((host, sorted(kw.items(), key=lambda i: i[0])))
        if key not in seen:
            device = flicker_hip.window_pixels, flicker_hip.hold
            diffuerase.configure(RUN)
            if host:
                flicker_hip.window_pixels, flicker_hip.hold = R.hip_window_pixels, R.hip_hold
            try:
                out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, feather_px=3, **KW, **kw)
                seen[key] = (np.stack(out), diffuerase.last_deflicker, flicker_hip.PART.dll is not None)
            finally:
                flicker_hip.window_pixels, flicker_hip.hold = device
                diffuerase.configure(None)
        return seen[key]
    return call


SEAMS = dict(tone_match="on", seam_blend="on", grain_match="on")
PLUMBING = [dict(), SEAMS, dict(spans=SPANS, roi=FOLLOW)]


def test_no_resolution_without_the_option(gpu, clip):
    """First of the drop-in tests: nothing has used flicker_hip in this process unless an earlier test of this module did; the plain call leaves
    it as it found it, and a fresh binding stays unresolved through a whole call."""
    import diffuerase
    from videovanish_amd import flicker_hip
    frames, masks, prior = clip
    kept, flicker_hip.PART.dll = flicker_hip.PART.dll, None
    diffuerase.configure(RUN)
    try:
        for kw in (dict(), dict(deflicker="off", tone_match="on"), dict(roi=FOLLOW, spans=SPANS)):
            diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, feather_px=3, **KW, **kw)
            assert flicker_hip.PART.dll is None and diffuerase.last_deflicker is None
    finally:
        diffuerase.configure(None)
        flicker_hip.PART.dll = kept


def test_seam_bindings_stay_unresolved_while_their_stage_is_off(gpu, clip):
    """The same for the seam stages of infill.finish: a call with no stage leaves fresh tone_hip, grain_hip and blend_hip unresolved, the
    tone-only call grain_hip and blend_hip."""
    import diffuerase
    from videovanish_amd import blend_hip, grain_hip, tone_hip
    frames, masks, prior = clip
    mods = (tone_hip, grain_hip, blend_hip)
    kept = [m.PART.dll for m in mods]
    diffuerase.configure(RUN)
    try:
        for kw, off in ((dict(), mods), (dict(roi=FOLLOW), mods), (dict(tone_match="on", roi=FOLLOW), mods[1:])):
            for m in mods:
                m.PART.dll = None
            diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, feather_px=3, **KW, **kw)
            assert all(m.PART.dll is None for m in off)
            assert (tone_hip.PART.dll is not None) == ("tone_match" in kw)
    finally:
        diffuerase.configure(None)
        for m, lib in zip(mods, kept):
            m.PART.dll = lib


@pytest.mark.parametrize("kw", PLUMBING, ids=["plain", "seams", "spans-follow"])
def test_drop_in_radius_0_is_the_call_without_the_option(gpu, clip, run, kw):
    """radius = 0 only materialises the resize that the paste kernels otherwise do on the fly: byte for byte the call without the option, at a
    max_img_size that makes the model run at another size than the frame."""
    base, none, _ = run(**kw)
    out, rep, _ = run(deflicker="radius=0", **kw)
    assert none is None and rep is not None and out.shape == base.shape == (T, H, W, 3)
    assert (out == base).all()
    assert not rep.changed.any() and not rep.shift.any() and rep.n.any() and (rep.samples[rep.n > 0] == 1.0).all()
    assert (out != np.stack(clip[0])).any()


@pytest.mark.parametrize("kw", [dict(), dict(spans=SPANS, roi=REGIONS)], ids=["plain", "spans-follow-regions"])
def test_drop_in_stage_equals_the_restatement(gpu, run, kw):
    out, rep, resolved = run(deflicker="on", **kw)
    want, wrep, _ = run(host=True, deflicker="on", **kw)
    assert resolved and (out == want).all()
    for a, b in zip(rep, wrep):
        assert a.shape == b.shape and (a == b).all()
    K = 2 if kw else 1
    assert rep.n.shape == rep.changed.shape == rep.samples.shape == rep.n_mask.shape == rep.changed_mask.shape == rep.samples_mask.shape == (K, T)
    assert rep.shift.shape == rep.shift_mask.shape == (K, T, 3) and rep.n.dtype == rep.changed_mask.dtype == np.int64
    print("deflicker report:", dict(n=rep.n.tolist(), changed=rep.changed.tolist(), n_mask=rep.n_mask.tolist(), changed_mask=rep.changed_mask.tolist(),
                                    samples_mask=np.round(rep.samples_mask, 2).tolist()))
    assert rep.changed_mask.sum() > 0 and (rep.changed_mask <= rep.n_mask).all() and (rep.n_mask <= rep.n).all()
    if kw:                                                                                          # frames outside the span: zero rows
        assert not any(v[:, [0, 8]].any() for v in rep) and rep.n[:, 1:8].all() and rep.n_mask[:, 2:7].all()
    else:
        assert (rep.n == H * W).all() and not rep.n_mask[0, [0, 1, 7, 8]].any() and rep.n_mask[0, 2:7].all()
    base, none, _ = run(**kw)
    assert none is None and (out != base).any()                                                     # and None after a call without the option
