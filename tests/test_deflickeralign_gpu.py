"""Aligned inpaint deflicker on the GPU: vvc_hold against the numpy restatement (tests/deflickeralign_ref.py) byte for byte, each call run twice
with identical bytes; the zero track against both forms of vvf_hold; and the drop-in's deflicker_align= path on the tiny architecture: a
locked-off clip against deflicker alone, a panned clip against the same call with the device functions replaced by the restatement.
No tolerances."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflicker_ref as R0  # noqa: E402
import deflickeralign_ref as R  # noqa: E402
import platealign_ref as A  # noqa: E402
import spans_ref  # noqa: E402

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.roi import RoiConfig  # noqa: E402
from videovanish_amd.spans import SpanConfig  # noqa: E402

TS = (1, 2, 9, 17)
RADII = (0, 1, 2, 4)
TOLS = (0, 6, 255)


def _d(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _clip(seed, T, h, w, H0, W0, offsets, off):
    """One textured background fixed on the canvas, seen through the windows of the panned frames: the window pixel (yy, xx) of frame t shows
    wide[offsets[t] + (yy, xx) + (off[t].y, off[t].x)]; +-5 levels of flicker, a block that changes for good half way (a real change: beyond
    tol = 6), flat runs (equal samples at tol = 0) and a mask of random bytes over a third of the frame."""
    rng = np.random.default_rng(seed)
    ey, ex = offsets[:, 0] + off[:, 1], offsets[:, 1] + off[:, 0]
    wide = rng.integers(0, 256, (int(ey.max() - ey.min()) + h, int(ex.max() - ex.min()) + w, 3))
    wide[: len(wide) // 3] = wide[: len(wide) // 3] // 64 * 64
    win = np.stack([wide[y - ey.min():y - ey.min() + h, x - ex.min():x - ex.min() + w] for y, x in zip(ey, ex)])
    win = win + rng.integers(-5, 6, (T, h, w, 3)) * (rng.random((T, h, w, 1)) < 0.8)
    win[T // 2:, h // 4: h // 2, w // 3:] += 40
    mask = (rng.random((T, H0, W0)) < 0.33) * rng.integers(1, 256, (T, H0, W0))
    return np.clip(win, 0, 255).astype(np.uint8), mask.astype(np.uint8)


def _moving_offsets(T, h, w, H0, W0, seed):
    """Offsets that move by 0 .. 3 px per frame, bounce off the frame's edges and touch them (test_deflicker_gpu's)."""
    rng = np.random.default_rng(seed)
    o = np.zeros((T, 2), np.int64)
    o[0] = (H0 - h, 0)
    d = np.array([-1, 1])
    for t in range(1, T):
        for a, lim in ((0, H0 - h), (1, W0 - w)):
            v = o[t - 1, a] + d[a] * rng.integers(0, 4)
            if v < 0 or v > lim:
                d[a] = -d[a]
                v = min(max(v, 0), lim)
            o[t, a] = v
    return o


def _hold_twice(win, offs, track, mask, radius, tol, gpu):
    from videovanish_amd import flickalign_hip
    args = (_d(win, gpu), _d(np.asarray(offs, np.int32), gpu), _d(np.asarray(track, np.int32), gpu), _d(mask, gpu))
    a, b = (flickalign_hip.hold(*args, radius, tol) for _ in range(2))
    out, sums = a[0].cpu().numpy(), a[1].cpu().numpy()
    assert (out == b[0].cpu().numpy()).all() and (sums == b[1].cpu().numpy()).all()
    assert out.dtype == np.uint8 and out.shape == win.shape and sums.dtype == np.int64 and sums.shape == (len(win), 12)
    return out, sums


def _against_the_restatement(win, offs, track, mask, gpu):
    """Every (radius, tol) -> the sums of the call at radius 2, tol 6."""
    kept = None
    for radius in RADII:
        for tol in TOLS:
            out, sums = _hold_twice(win, offs, track, mask, radius, tol, gpu)
            want, wsums = R.hold(win, offs, track, mask, radius, tol)
            assert (out == want).all(), (radius, tol, int((out != want).sum()))
            assert (sums == wsums).all(), (radius, tol, sums[0].tolist(), wsums[0].tolist())
            if (radius, tol) == (2, 6):
                kept = out, sums
    return kept


# ---- vvc_hold against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
def test_hold_window_fixed_in_the_frame_with_lost_frames(gpu, T):
    """A 40 x 56 window at (12, 8) of a 64 x 96 frame, a random-walk track (dx 0 .. 5, dy -2 .. 2), frames 3 and T - 1 lost."""
    h, w, H0, W0 = 40, 56, 64, 96
    offs, off = np.tile([[12, 8]], (T, 1)), R.walk(T, T, (0, 5), (-2, 2))
    track = R.make_track(off, lost=(3, T - 1))
    win, mask = _clip(T * 1000 + h, T, h, w, H0, W0, offs, off)
    out, sums = _against_the_restatement(win, offs, track, mask, gpu)
    for t in {3, T - 1} & set(range(T)):
        assert (out[t] == win[t]).all() and sums[t, 2] == h * w
    assert sums[:, 1].any() == (T > 2)                                                              # T = 2: frame 1 is lost, frame 0 stands alone


@pytest.mark.parametrize("T", TS)
def test_hold_full_frame_odd_width(gpu, T):
    """The full frame at 45 x 83: an odd width, a tail block."""
    h, w = 45, 83
    offs, off = np.zeros((T, 2), np.int64), R.walk(T, T + 50, (-3, 4), (-2, 2))
    win, mask = _clip(T, T, h, w, h, w, offs, off)
    out, sums = _against_the_restatement(win, offs, R.make_track(off), mask, gpu)
    assert sums[:, 1].any() == (T > 1) and (sums[:, 0] == h * w).all()


@pytest.mark.parametrize("T", TS)
def test_hold_moving_windows_under_a_track_with_negative_steps(gpu, T):
    """40 x 56 windows whose offsets move 0 .. 3 px per frame and touch the frame's edges, under a track that walks left and up as well."""
    h, w, H0, W0 = 40, 56, 64, 96
    offs, off = _moving_offsets(T, h, w, H0, W0, T), R.walk(T, T + 90, (-4, 1), (-2, 2))
    assert offs[:, 0].max() == 24 and offs[:, 1].min() == 0 and (T < 9 or off[:, 0].min() < 0)
    win, mask = _clip(T + 7, T, h, w, H0, W0, offs, off)
    out, sums = _against_the_restatement(win, offs, R.make_track(off), mask, gpu)
    assert sums[:, 1].any() == (T > 1)


@pytest.mark.parametrize("T", TS)
def test_hold_steps_beyond_the_window_give_no_sample(gpu, T):
    """A track whose steps exceed the window, and one whose values are far beyond any frame: no overlap exists, n = 1 everywhere."""
    h, w, H0, W0 = 40, 56, 64, 96
    offs = _moving_offsets(T, h, w, H0, W0, 3)
    win, mask = _clip(T + 3, T, h, w, H0, W0, offs, np.zeros((T, 2), np.int64))
    far, t = np.stack([np.arange(T) * (w + 4), np.arange(T) * -(h + 4)], 1), np.arange(T)
    wild = np.stack([np.where(t % 2, 2 ** 31 - 1 - 100 * t, -(2 ** 31) + 100 * t), np.where(t % 2, -(2 ** 31) + 100 * t, 2 ** 31 - 1 - 100 * t)], 1)     # the ends of int32
    for off in (far, far * (1 << 20), wild):
        out, sums = _against_the_restatement(win, offs, R.make_track(off), mask, gpu)
        assert (out == win).all() and (sums[:, 2] == h * w).all() and not sums[:, 1].any()


# ---- the zero track is vvf_hold -----------------------------------------------------------------------------------------------------------
def test_zero_track_equals_both_forms_of_the_unaligned_filter(gpu):
    from videovanish_amd import flickalign_hip, flicker_hip
    T, h, w, H0, W0 = 17, 40, 56, 64, 96
    zero = R.make_track(np.zeros((T, 2), np.int64))
    for fixed, offs in ((True, np.tile([[12, 8]], (T, 1))), (False, _moving_offsets(T, h, w, H0, W0, 5))):
        win, mask = _clip(21, T, h, w, H0, W0, offs, np.zeros((T, 2), np.int64))
        args = _d(win, gpu), _d(offs.astype(np.int32), gpu), _d(mask, gpu)
        for radius, tol in ((1, 6), (2, 12), (4, 255)):
            want = flicker_hip.hold(*args, radius, tol, fixed=fixed)                                 # w % 4 == 0, fixed offsets: the fixed form
            for _ in range(2):
                out, sums = flickalign_hip.hold(args[0], args[1], _d(zero, gpu), args[2], radius, tol)
                assert (out == want[0]).all() and (sums == want[1]).all()
            assert (out.cpu().numpy() != win).any()


# ---- every byte of out and of sums is written, nothing outside them ------------------------------------------------------------------------
def test_poisoned_out_and_sums(gpu):
    from videovanish_amd import flickalign_hip, hip
    T, h, w, H0, W0 = 17, 41, 55, 64, 96
    offs, off = _moving_offsets(T, h, w, H0, W0, 2), R.walk(T, 8, (-3, 4), (-2, 2))
    track = R.make_track(off, lost=(5,))
    win, mask = _clip(9, T, h, w, H0, W0, offs, off)
    want, wsums = R.hold(win, offs, track, mask, 2, 6)
    n, G = win.size, 4096
    win_t, offs_t, track_t, mask_t = _d(win, gpu), _d(offs.astype(np.int32), gpu), _d(track, gpu), _d(mask, gpu)
    for poison in (0x00, 0xFF):
        for _ in range(2):
            buf = torch.full((n + 2 * G,), poison, dtype=torch.uint8, device=gpu)
            sbuf = torch.full((T * 12 + 2 * 16,), -1 if poison else 0x0101010101010101, dtype=torch.int64, device=gpu)
            guard = int(sbuf[0].item())
            out, sums = buf[G:G + n].view(win.shape), sbuf[16:16 + T * 12].view(T, 12)
            rc = flickalign_hip.lib().vvc_hold(hip._p(win_t), hip._p(offs_t), hip._p(track_t), hip._p(mask_t), T, H0, W0, h, w, 2, 6, hip._p(out), hip._p(sums),
                                               hip._stream())
            assert rc == 0
            assert (out.cpu().numpy() == want).all() and (sums.cpu().numpy() == wsums).all()
            assert (buf[:G] == poison).all() and (buf[G + n:] == poison).all() and (sbuf[:16] == guard).all() and (sbuf[16 + T * 12:] == guard).all()
        got, _ = flickalign_hip.hold(win_t, offs_t, track_t, mask_t, 2, 6, out=buf[G:G + n].view(win.shape))
        assert got.data_ptr() == buf.data_ptr() + G and (got.cpu().numpy() == want).all()


def test_refusals_launch_nothing(gpu):
    from videovanish_amd import flickalign_hip
    win, offs, mask = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=gpu), torch.zeros((2, 2), dtype=torch.int32, device=gpu), \
        torch.zeros((2, 8, 8), dtype=torch.uint8, device=gpu)
    track = torch.zeros((2, 8), dtype=torch.int32, device=gpu)
    hold = flickalign_hip.hold
    for bad in (lambda: hold(win, offs, track, mask, 5, 12), lambda: hold(win, offs, track, mask, 2, 256),
                lambda: hold(win, offs, track, mask[:, :7].contiguous(), 2, 12), lambda: hold(win, offs, track, mask, 2, 12, out=win),
                lambda: hold(win, offs[:1], track, mask, 2, 12), lambda: hold(win, offs, track[:1], mask, 2, 12),
                lambda: hold(win, offs, track[:, :7].contiguous(), mask, 2, 12), lambda: hold(win, offs, track.to(torch.int64), mask, 2, 12),
                lambda: hold(win, offs, track.cpu(), mask, 2, 12), lambda: hold(win.cpu(), offs, track, mask, 2, 12)):
        with pytest.raises(RuntimeError):
            bad()
    torch.cuda.synchronize()


# ---- the drop-in on the tiny architecture (the fixtures of test_deflicker_gpu.py) -------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=80, num_inference_steps=2, scheduler="ddim")         # the model runs at 48 x 80, the frame is 96 x 160
T, H, W = 9, 96, 160
REGIONS = RoiConfig("follow", context=0.25, pad_min=8, min_side=32, smooth=1, max_regions=8)
SPANS = SpanConfig("masked", context=1, min_len=3, min_gap=2)
BOXES = [(6, 18, 6, 30, 2), (70, 86, 124, 148, -2)]          # top left moving right, bottom right moving left, in frames 2 .. 6
LOGO = (64, 104, 80, 134)                                    # screen-fixed, in frames 2 .. 6


def _with_prior(frames, masks):
    prior = []
    for f, m in zip(frames, masks):
        p = f.copy()
        p[m[..., 0] > 0] = f.reshape(-1, 3).mean(0).astype(np.uint8)
        prior.append(p)
    return prior


@pytest.fixture(scope="module")
def still_clip():
    """test_deflicker_gpu's clip with the camera locked off."""
    frames, _ = spans_ref.shots_clip(61, (T,), (0,), H, W)
    masks = []
    for t in range(T):
        m = np.zeros((H, W, 3), np.uint8)
        if 2 <= t <= 6:
            for y0, y1, x0, x1, vx in BOXES:
                m[y0:y1, x0 + vx * t: x1 + vx * t] = 255
        masks.append(m)
    return frames, masks, _with_prior(frames, masks)


@pytest.fixture(scope="module")
def pan_clip():
    """A pan of 2 .. 5 px in x and -2 .. 2 px in y per frame over an iid texture with +-3 levels of noise; in frames 2 .. 6 a box that crosses the
    screen and a screen-fixed logo, both masked."""
    frames, _, off, _, _, _ = A.pan_clip(T=T, H=H, W=W, seed=8, box=(0, 0))
    masks = []
    for t in range(T):
        m = np.zeros((H, W, 3), np.uint8)
        if 2 <= t <= 6:
            m[LOGO[0]:LOGO[2], LOGO[1]:LOGO[3]] = 255
            m[10:30, 6 + 9 * t: 30 + 9 * t] = 255
            frames[t][m[..., 0] > 0] = 20
        masks.append(m)
    frames = list(frames)
    return frames, masks, _with_prior(frames, masks), off


def _call(clip, host=False, **kw):
    """-> (output frames, last_deflicker, last_deflicker_align) of the drop-in on the tiny architecture.  host=True: flicker_hip.window_pixels
    and flickalign_hip.hold are the restatement."""
    import diffuerase
    from videovanish_amd import flickalign_hip, flicker_hip
    frames, masks, prior = clip[:3]
    device = flicker_hip.window_pixels, flickalign_hip.hold
    diffuerase.configure(RUN)
    if host:
        flicker_hip.window_pixels, flickalign_hip.hold = R0.hip_window_pixels, R.hip_hold
    try:
        out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, feather_px=3, **KW, **kw)
        return np.stack(out), diffuerase.last_deflicker, diffuerase.last_deflicker_align
    finally:
        flicker_hip.window_pixels, flickalign_hip.hold = device
        diffuerase.configure(None)


def test_drop_in_locked_off_is_deflicker_alone_and_resolves_nothing_without_the_option(gpu, still_clip):
    from videovanish_amd import flickalign_hip
    kept, flickalign_hip.PART.dll = flickalign_hip.PART.dll, None
    try:
        base, rep, none = _call(still_clip, deflicker="on")
        assert none is None and rep is not None and flickalign_hip.PART.dll is None                 # a full call without the option
        out, arep_rep, arep = _call(still_clip, deflicker="on", deflicker_align="on")
        assert flickalign_hip.PART.dll is None                                                      # "static": vvf_hold as it is
    finally:
        flickalign_hip.PART.dll = kept
    assert (out == base).all() and (out != np.stack(still_clip[0])).any()
    for a, b in zip(rep, arep_rep):
        assert (a == b).all()
    assert arep.path == ("static",) and arep.segments == ((0, T),) and not arep.off[0].any() and arep.tracked[0].all() and arep.off[0].shape == (T, 2)
    assert rep.changed_mask.sum() > 0


@pytest.mark.parametrize("kw", [dict(), dict(spans=SPANS, roi=REGIONS)], ids=["plain", "spans-follow-regions"])
def test_drop_in_on_a_pan_equals_the_restatement(gpu, pan_clip, kw):
    off = pan_clip[3]
    out, rep, arep = _call(pan_clip, deflicker="on", deflicker_align="on", **kw)
    want, wrep, warep = _call(pan_clip, host=True, deflicker="on", deflicker_align="on", **kw)
    assert (out == want).all()
    for a, b in zip(rep, wrep):
        assert a.shape == b.shape and (a == b).all()
    a, b = (1, 8) if kw else (0, T)                                                                 # the span: frames 2 .. 6 and one frame of context
    assert arep.path == warep.path == ("tracked",) and arep.segments == warep.segments == ((a, b),)
    assert (arep.off[0] == off[a:b] - off[a]).all() and arep.tracked[0].all() and (arep.key[0] == warep.key[0]).all()
    assert (arep.off[0] == warep.off[0]).all() and (arep.residual[0] == warep.residual[0]).all() and arep.residual[0][1:].all()
    K = 2 if kw else 1
    assert rep.n.shape == (K, T) and rep.changed_mask.sum() > 0 and (rep.changed_mask <= rep.n_mask).all()
    print("deflicker report:", dict(samples_mask=np.round(rep.samples_mask, 2).tolist(), changed_mask=rep.changed_mask.tolist()))
    alone, _, none = _call(pan_clip, deflicker="on", **kw)
    assert none is None and (out != alone).any()                                                    # and None after a call without the option
