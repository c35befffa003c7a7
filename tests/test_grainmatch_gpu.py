"""Seam grain matching on the GPU: the two entry points of vv_grain.hip against the numpy / scipy restatement (tests/grainmatch_ref.py) byte for
byte, each run twice with identical bytes; infill.finish with the stage on against the restatement, against the grain it has to give back and
against the call without it; and the drop-in's grain_match= path on the tiny architecture against the restatement applied to the model's own
frames.  No tolerances but the CPU-measured margin of the recovery."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grainmatch_ref as R  # noqa: E402
import tonematch_ref as TR  # noqa: E402
import spans_ref  # noqa: E402

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.grainmatch import GrainMatchConfig  # noqa: E402
from videovanish_amd.roi import RoiConfig, RoiPlan, plan_roi  # noqa: E402
from videovanish_amd.tonematch import ToneMatchConfig  # noqa: E402


def _d(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _twice(fn):
    """fn() -> a tensor; run twice, identical bytes; the first run's result as a numpy array."""
    a, b = fn().cpu().numpy(), fn().cpu().numpy()
    assert (a == b).all()
    return a


def _ident(T):
    return np.ascontiguousarray(np.broadcast_to(R.IDENT, (T, 3, 256)))


def _stats(patch, orig, mask, offs, lut, h, w, ring, flat, gpu):
    from videovanish_amd import grain_hip
    args = [_d(a, gpu) for a in (patch, orig, mask, np.asarray(offs, np.int32), lut)]
    got = _twice(lambda: grain_hip.ring_grain_stats(*args, h, w, ring, flat))
    want = R.sums(patch, orig, mask, offs, lut, h, w, ring, flat)
    assert got.dtype == np.int64 and got.shape == (len(patch), 36)
    assert (got == want).all(), (ring, flat, got.reshape(-1, 12, 3)[..., 0].sum(1).tolist(), want.reshape(-1, 12, 3)[..., 0].sum(1).tolist())
    return want.reshape(len(patch), 3, 4, 3)


# ---- ring_grain_stats ---------------------------------------------------------------------------------------------------------------------
def _frame_masks(H, W, seed):
    """The nine masks [H,W] of the tone test: empty, full, one pixel in two corners, a bar along each frame edge (two frames), two blobs whose
    ring leaves the frame, random at density 0.02."""
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


def _plateaus(rng, T, H, W):
    """Model frames [T,H,W,3] with every kind of neighbourhood: plateaus of 16 levels over all four bands (flat 0 counts their insides), +-3 of
    noise on the right half (flat 24 counts it, flat 0 does not), steps between the plateaus and a few bright specks (only flat 255 counts them)."""
    x = np.stack([TR.smooth_texture(int(rng.integers(1 << 30)), H, W, lo=0, hi=255) for _ in range(T)]).astype(np.int64) // 16 * 16
    x[:, :, W // 2:] += rng.integers(-3, 4, x[:, :, W // 2:].shape)
    speck = rng.random(x.shape[:3]) < 0.01
    x[speck] = 255 - x[speck]
    return np.clip(x, 0, 255).astype(np.uint8)


def _bent_tables(T):
    """[T,3,256]: a negative, a compressed and an identity table (smooth ones: they keep the flat places flat and move the bands)."""
    v = np.arange(256)
    return np.ascontiguousarray(np.broadcast_to(np.stack([255 - v, v * 3 // 4 + 20, v]).astype(np.uint8), (T, 3, 256)))


@pytest.mark.parametrize("ring", [1, 12, 32])
@pytest.mark.parametrize("H,W", [(37, 53), (96, 130)])
def test_ring_grain_stats_full_frame(gpu, H, W, ring):
    """The full frame is the window (0, 0, H, W) of a patch of the frame's size: 37 x 53 is smaller than a tile, 96 x 130 leaves a 2-column
    remainder tile.  Nine masks, flat 0 / 24 / 255, the identity table and one that is not."""
    rng = np.random.default_rng(H * 100 + ring)
    masks = _frame_masks(H, W, H + ring)
    n = {flat: [] for flat in (0, 24, 255)}
    for a in range(0, 9, 3):
        orig = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        patch = _plateaus(rng, 3, H, W)
        for flat in n:
            n[flat] += _stats(patch, orig, masks[a:a + 3], np.zeros((3, 2), np.int32), _ident(3), H, W, ring, flat, gpu)[..., 0].sum((1, 2)).tolist()
        if a == 6:
            bent = _stats(patch, orig, masks[a:a + 3], np.zeros((3, 2), np.int32), _bent_tables(3), H, W, ring, 24, gpu)
            plain = _stats(patch, orig, masks[a:a + 3], np.zeros((3, 2), np.int32), _ident(3), H, W, ring, 24, gpu)
            if ring > 1:
                assert (bent[:, 0, :, 0] == plain[:, 0, ::-1, 0]).all() and bent[:, 0, :, 0].any()      # the negative: the same pixels, the bands mirrored
                assert (bent[:, 0, ::-1, 1:] == plain[:, 0, :, 1:]).all()                               # |L| is the same, y untouched
                assert (bent[:, 2] == plain[:, 2]).all() and not (bent[:, 1] == plain[:, 1]).all()
    print("counted (pixel, channel) pairs:", n)
    for flat in n:
        assert n[flat][0] == 0 and n[flat][1] == 0                                                   # no mask: no ring; all mask: no unmasked pixel
    assert all(a <= b <= c for a, b, c in zip(n[0], n[24], n[255]))
    # one mask pixel in a corner: the ring is the (ring + 1)^2 - 1 pixels round it, 3 channels; without the frame's border row and column and
    # the three pixels that touch the mask pixel (ring 1: none is left)
    assert n[255][2] == n[255][7] == 3 * max(0, ring * ring - 1)
    if ring > 1:
        assert all(v > 0 for v in n[255][2:]) and sum(n[0]) > 0 and sum(n[24]) > sum(n[0])


@pytest.mark.parametrize("ring", [1, 12, 32])
def test_ring_grain_stats_window(gpu, ring):
    """A 40 x 56 model output resized to a 48 x 64 window of a 96 x 130 frame; per-frame offsets with (0, 0) and the bottom-right corner; a mask
    that ends 3 pixels from the window's edge (the ring is clipped by the window, and the window's border pixels have no neighbourhood), a mask
    pixel outside the window within `ring` of pixels inside it, and a random mask over the whole frame; then the same window without the resize
    and the whole frame as the window of a smaller patch."""
    H, W, h, w, Hm, Wm = 96, 130, 48, 64, 40, 56
    rng = np.random.default_rng(ring)
    orig = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    patch = _plateaus(rng, 3, Hm, Wm)
    offs = np.array([[0, 0], [H - h, W - w], [20, 31]], np.int32)
    mask = np.zeros((3, H, W), np.uint8)
    mask[0, 10:30, 50:61] = 255
    mask[0, 50, 70] = 255                            # outside the window (rows < 48, columns < 64), 3 rows and 7 columns away
    mask[1, 60:80, 100:126] = 9
    mask[1, 45, 60] = 255                            # outside the window (rows >= 48, columns >= 66)
    mask[2] = (rng.random((H, W)) < 0.02) * 255
    for flat, lut in ((24, _ident(3)), (255, _bent_tables(3))):
        _stats(patch, orig, mask, offs, lut, h, w, ring, flat, gpu)
    # the pixel outside the window counts for the ring; the window's last row and column are in the ring but have no neighbourhood in the window
    lone = mask.copy()
    lone[0, 10:30, 50:61] = 0
    got = _stats(patch, orig, lone, offs, _ident(3), h, w, ring, 255, gpu)[0, :, :, 0].sum(1)
    assert (got == (max(0, ring - 3) * max(0, ring - 7) if ring > 7 else 0)).all()
    _stats(_plateaus(rng, 3, h, w), orig, mask, offs, _ident(3), h, w, ring, 24, gpu)
    _stats(patch, orig, mask, np.zeros((3, 2), np.int32), _bent_tables(3), H, W, ring, 24, gpu)


def test_ring_grain_stats_sums_are_64_bit(gpu):
    """One 128 x 128 frame with x = 128 everywhere, y a 0 / 255 checkerboard (|L| = 2040 at every pixel) and a one-column mask: at ring 32 the
    62 x 126 pixels beside it count, all in band 2, and Sy passes 2^32."""
    H = W = 128
    patch = np.full((1, H, W, 3), 128, np.uint8)
    yy, xx = np.mgrid[:H, :W]
    orig = np.ascontiguousarray(np.broadcast_to((((yy + xx) % 2) * 255).astype(np.uint8)[None, :, :, None], (1, H, W, 3)))
    mask = np.zeros((1, H, W), np.uint8)
    mask[0, :, 64] = 255
    want = _stats(patch, orig, mask, np.zeros((1, 2), np.int32), _ident(1), H, W, 32, 0, gpu)
    n = 62 * 126
    assert want[0, :, 2].tolist() == [[n, 0, n * 2040 * 2040]] * 3 and n * 2040 * 2040 > 2 ** 32
    assert not want[0, :, [0, 1, 3]].any()


# ---- paste_grain_composite ----------------------------------------------------------------------------------------------------------------
FRAME_IDS = np.array([5, 0, 2 ** 31 - 1, 1000003], np.int32)


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
def test_paste_grain_composite(gpu, full, resize, feather):
    from videovanish_amd import grain_hip, tone_hip
    patch, orig, mask, offs, h, w = _paste_inputs(3 + 2 * full + resize, full, resize)
    T = len(patch)
    rng = np.random.default_rng(9)
    lut = rng.integers(0, 256, (T, 3, 256), dtype=np.uint8)
    amp = rng.integers(0, 256, (T, 3, 256), dtype=np.uint8)                                          # up to sigma 15.9: the clip to 0 .. 255 is at work
    dp, do, dm, df, dl, da, di = (_d(a, gpu) for a in (patch, orig, mask, offs, lut, amp, FRAME_IDS))
    toned = tone_hip.paste_lut_composite(dp, do, dm, df, dl, h, w, feather).cpu().numpy()
    zero = torch.zeros_like(da)
    for mode, name in enumerate(("luma", "rgb")):
        # no amplitude: the bytes of the tone paste
        assert (_twice(lambda: grain_hip.paste_grain_composite(dp, do, dm, df, dl, zero, di, 77, mode, h, w, feather)) == toned).all()
        got = _twice(lambda: grain_hip.paste_grain_composite(dp, do, dm, df, dl, da, di, 77, mode, h, w, feather))
        want = R.composite(patch, orig, mask, offs, lut, amp, FRAME_IDS, 77, name, h, w, feather)
        assert (got == want).all() and (got != toned).any()
        if feather < 0:                                                                              # the plain paste needs no mask
            assert (grain_hip.paste_grain_composite(dp, do, None, df, dl, da, di, 77, mode, h, w, feather).cpu().numpy() == want).all()
        buf = torch.empty_like(do)
        assert grain_hip.paste_grain_composite(dp, do, dm, df, dl, da, di, 77, mode, h, w, feather, out=buf) is buf and (buf.cpu().numpy() == want).all()
        other = grain_hip.paste_grain_composite(dp, do, dm, df, dl, da, di, 78, mode, h, w, feather).cpu().numpy()
        assert (other == R.composite(patch, orig, mask, offs, lut, amp, FRAME_IDS, 78, name, h, w, feather)).all() and (other != got).any()


@pytest.mark.parametrize("mode", [0, 1])
def test_a_pixel_gets_the_same_noise_through_a_window_and_the_full_frame(gpu, mode):
    """The plain paste of a full-frame patch, and of its crops at per-frame offsets: inside each window the same bytes."""
    from videovanish_amd import grain_hip
    T, H, W, h, w = 4, 50, 70, 24, 32
    rng = np.random.default_rng(21 + mode)
    orig = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    patch = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    lut = rng.integers(0, 256, (T, 3, 256), dtype=np.uint8)
    amp = rng.integers(1, 256, (T, 3, 256), dtype=np.uint8)
    offs = np.array([[0, 0], [0, W - w], [H - h, 0], [13, 29]], np.int32)
    crop = np.stack([patch[t, oy:oy + h, ox:ox + w] for t, (oy, ox) in enumerate(offs)])
    do, dl, da, di = (_d(a, gpu) for a in (orig, lut, amp, FRAME_IDS))
    whole = _twice(lambda: grain_hip.paste_grain_composite(_d(patch, gpu), do, None, _d(np.zeros((T, 2), np.int32), gpu), dl, da, di, 3, mode, H, W, -1.0))
    part = _twice(lambda: grain_hip.paste_grain_composite(_d(crop, gpu), do, None, _d(offs, gpu), dl, da, di, 3, mode, h, w, -1.0))
    assert (whole == R.composite(patch, orig, None, np.zeros((T, 2), np.int32), lut, amp, FRAME_IDS, 3, ("luma", "rgb")[mode], H, W, -1.0)).all()
    for t, (oy, ox) in enumerate(offs):
        assert (part[t, oy:oy + h, ox:ox + w] == whole[t, oy:oy + h, ox:ox + w]).all()
        outside = np.ones((H, W), bool)
        outside[oy:oy + h, ox:ox + w] = False
        assert (part[t][outside] == orig[t][outside]).all()
    assert (whole != np.stack([np.stack([lut[t, c][patch[t, ..., c]] for c in range(3)], -1) for t in range(T)])).mean() > 0.5


def test_refusals_launch_nothing(gpu):
    from videovanish_amd import grain_hip
    lib = grain_hip.lib()
    u8 = lambda *shape: torch.full(shape, 7, dtype=torch.uint8, device=gpu)
    patch, orig, mask, lut, amp, out = u8(2, 8, 8, 3), u8(2, 8, 8, 3), u8(2, 8, 8), u8(2, 3, 256), u8(2, 3, 256), u8(2, 8, 8, 3)
    offs = torch.zeros((2, 2), dtype=torch.int32, device=gpu)
    ids = torch.zeros(2, dtype=torch.int32, device=gpu)
    sums = torch.full((2, 36), 7, dtype=torch.int64, device=gpu)
    p = lambda t: t.data_ptr()
    stats = lambda ring=4, flat=24, m=mask, h=8: lib.vvg_ring_grain_stats(p(patch), 8, 8, p(orig), None if m is None else p(m), p(offs), p(lut), 2, 8, 8, h, 8,
                                                                            ring, flat, p(sums), None)
    paste = lambda mode=0, feather=3.0, m=mask, a=amp: lib.vvg_paste_grain_composite(p(patch), 8, 8, p(orig), None if m is None else p(m), p(offs), p(lut),
                                                                                     None if a is None else p(a), p(ids), 0, mode, 2, 8, 8, 8, 8, feather,
                                                                                     p(out), None)
    assert [stats(ring=0), stats(ring=33), stats(flat=256), stats(flat=-1)] == [-2, -2, -2, -2]
    assert stats(m=None) == -1 and stats(h=9) == -1
    assert [paste(mode=2), paste(mode=-1), paste(m=None), paste(a=None)] == [-1, -1, -1, -1] and paste(feather=64.5) == -2
    torch.cuda.synchronize()
    assert (sums == 7).all() and (out == 7).all()                                                   # nothing was launched, nothing cleared
    with pytest.raises(RuntimeError, match="ring 1 .. 32"):
        grain_hip.ring_grain_stats(patch, orig, mask, offs, lut, 8, 8, 33, 24)
    with pytest.raises(RuntimeError, match="flat 0 .. 255"):
        grain_hip.ring_grain_stats(patch, orig, mask, offs, lut, 8, 8, 4, 256)
    with pytest.raises(RuntimeError, match="mode 0"):
        grain_hip.paste_grain_composite(patch, orig, mask, offs, lut, amp, ids, 0, 2, 8, 8, 3.0)
    with pytest.raises(RuntimeError):
        grain_hip.ring_grain_stats(patch.cpu(), orig, mask, offs, lut, 8, 8, 4, 24)                  # no CPU fallback
    with pytest.raises(RuntimeError):
        grain_hip.paste_grain_composite(patch, orig, mask, offs, lut, amp.cpu(), ids, 0, 0, 8, 8, 3.0)
    with pytest.raises(RuntimeError, match="not orig itself"):
        grain_hip.paste_grain_composite(patch, orig, mask, offs, lut, amp, ids, 0, 0, 8, 8, 3.0, out=orig)
    assert (sums == 7).all() and (out == 7).all()


# ---- infill.finish ------------------------------------------------------------------------------------------------------------------------
CFG = GrainMatchConfig()
FIT = dict(mode=CFG.mode, ring=CFG.ring, flat=CFG.flat, seed=CFG.seed, smooth=CFG.smooth, strength=CFG.strength, max_sigma=CFG.max_sigma, min_count=CFG.min_count)
TONE = ToneMatchConfig()
TONE_FIT = dict(mode=TONE.mode, ring=TONE.ring, smooth=TONE.smooth, max_gain=TONE.max_gain, max_offset=TONE.max_offset, min_count=TONE.min_count,
                min_var=TONE.min_var)


def _report_equals(rep, k, s, so, sm, sa, a=0, b=None):
    b = a + len(s) if b is None else b
    assert (rep.n[k, a:b] == np.asarray(s).reshape(-1, 3, 4, 3)[..., 0]).all() and ((rep.sigma_added[k, a:b] == 0) == (sa == 0)).all()
    for got, want in ((rep.sigma_orig, so), (rep.sigma_model, sm), (rep.sigma_added, sa)):
        assert np.allclose(got[k, a:b], want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("sigma", R.RECOVERY_SIGMAS)
def test_finish_gives_a_known_grain_back(gpu, sigma):
    """The recovery clips of the CPU test (seeds 0 .. 3) through infill.finish on the full frame: the restatement's bytes, and Immerkaer's
    estimate deep inside the mask of the output within the CPU-measured margin of sigma, where the plain composite carries no grain at all."""
    from videovanish_amd import infill
    for s in range(4):
        orig, x, mask = R.recovery_clip(s, sigma)
        T, H, W = mask.shape
        dil = _d(mask, gpu)
        rows = []
        out = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu, grain=CFG, grain_out=rows, frame0=0))
        want, sums, so, sm, sa = R.apply(x, orig, mask, np.zeros((T, 2), np.int32), H, W, 3.0, [0], **FIT)
        assert (out == want).all()
        assert len(rows) == 1 and rows[0].n.shape == rows[0].sigma_added.shape == (1, T, 3, 4) and rows[0].n.dtype == np.int64
        _report_equals(rows[0], 0, sums, so, sm, sa)
        inside = R.inside_estimate(out[0], x[0], mask[0])
        plain = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu))
        print(f"sigma {sigma}, seed {s}: inside the mask {inside.round(3).tolist()}, added {sa.min():.3f} .. {sa.max():.3f}")
        assert (np.abs(inside / sigma - 1) <= 1.5 * R.MEASURED_DEVIATION["inside"][sigma]).all()
        assert (np.abs(sa / sigma - 1) <= 1.5 * R.MEASURED_DEVIATION["fit"][sigma]).all()
        assert not R.inside_estimate(plain[0], x[0], mask[0]).any()
    # another first frame: another field of the same size; keep_unmasked_original=False: every pixel of the frame gets grain
    later = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu, grain=CFG, frame0=7))
    assert (later == R.apply(x, orig, mask, np.zeros((T, 2), np.int32), H, W, 3.0, [7], **FIT)[0]).all() and (later != out).any()
    every = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, False, gpu, grain=CFG))
    assert (every == R.apply(x, orig, mask, np.zeros((T, 2), np.int32), H, W, -1.0, [0], **FIT)[0]).all() and (every != x).mean() > 0.5


def test_finish_with_tone_in_front(gpu):
    """Three frames whose model frames carry a tone shift and no grain: the tone table first, the grain statistics on what it gives; both reports."""
    from videovanish_amd import infill
    smooth, shifted, mask = TR.restoration_clip(0.9, 10)
    T, H, W = mask.shape
    orig = np.clip(np.rint(smooth + np.random.default_rng(5).normal(0, 4.0, smooth.shape)), 0, 255).astype(np.uint8)
    tones, grains = [], []
    out = np.stack(infill.finish([list(shifted)], list(orig), _d(mask, gpu), [], 3, True, gpu, tone=TONE, tone_out=tones, grain=CFG, grain_out=grains,
                                 frame0=3))
    want, sums, so, sm, sa = R.apply(shifted, orig, mask, np.zeros((T, 2), np.int32), H, W, 3.0, [3, 4, 5], tone=dict(TONE_FIT), **FIT)
    assert (out == want).all()
    _report_equals(grains[0], 0, sums, so, sm, sa)
    gain, offset = TR.fit(TR.sums(shifted, orig, mask, np.zeros((T, 2), np.int32), H, W, TONE.ring), **{k: v for k, v in TONE_FIT.items() if k != "ring"})
    assert len(tones) == len(grains) == 1 and (tones[0].gain[0] == gain).all() and (tones[0].offset[0] == offset).all()
    assert np.abs(gain - 1 / 0.9).max() < 0.02 and (np.abs(sa / 4.0 - 1) < 0.25).all()
    # the tone-only call is what it was, and differs; the grain-only call measures the grain on the unshifted pixels
    tone_only = np.stack(infill.finish([list(shifted)], list(orig), _d(mask, gpu), [], 3, True, gpu, tone=TONE))
    assert (tone_only == TR.apply(shifted, orig, mask, np.zeros((T, 2), np.int32), H, W, 3.0, **TONE_FIT)[0]).all() and (tone_only != out).any()


def test_finish_two_windows_are_fitted_independently(gpu):
    """K = 2: two disjoint windows on an original whose two halves carry different grain; each is fitted on its own ring."""
    from videovanish_amd import infill
    smooth, _, _ = TR.restoration_clip(1.0, 0)
    T, H, W = smooth.shape[:3]
    g = np.random.default_rng(11).normal(0, 1.0, smooth.shape)
    g[:, :, :67] *= 3.0
    g[:, :, 67:] *= 7.0
    orig = np.clip(np.rint(smooth + g), 0, 255).astype(np.uint8)
    wins = [((0, 0), (48, 64), (12, 15, 30, 40)), ((50, 70), (40, 56), (60, 85, 75, 110))]
    mask = np.zeros((T, H, W), np.uint8)
    plans, outs = [], []
    for (oy, ox), (h, w), (y0, x0, y1, x1) in wins:
        mask[:, y0:y1, x0:x1] = 255
        offs = np.tile(np.array([[oy, ox]], np.int32), (T, 1))
        plans.append(RoiPlan("static", (h, w), offs, offs.astype(np.float64)))
        outs.append(list(smooth[:, oy:oy + h, ox:ox + w].copy()))
    rows = []
    cfg = GrainMatchConfig(mode="rgb", seed=9)
    out = np.stack(infill.finish(outs, list(orig), _d(mask, gpu), plans, 3, True, gpu, grain=cfg, grain_out=rows, frame0=100))
    want = orig
    assert len(rows) == 1 and rows[0].n.shape == (2, T, 3, 4)
    for k, (plan, o) in enumerate(zip(plans, outs)):
        want, s, so, sm, sa = R.apply(np.stack(o), want, mask, plan.offsets, *plan.size, 3.0, [100, 101, 102], **dict(FIT, mode="rgb", seed=9))
        _report_equals(rows[0], k, s, so, sm, sa)
    assert (out == want).all()
    print("added:", rows[0].sigma_added[:, 0].round(2).tolist())
    assert (np.abs(rows[0].sigma_added[0] / 3.0 - 1) < 0.3).all() and (np.abs(rows[0].sigma_added[1] / 7.0 - 1) < 0.3).all()


def test_finish_without_missing_grain_is_the_plain_call(gpu):
    """The model's frame equals the original on the ring (and is something else inside the mask): Sx == Sy, nothing is added, the bytes of the
    call without the option, with and without tone matching."""
    from videovanish_amd import infill
    smooth, _, mask = TR.restoration_clip(1.0, 0)
    orig = np.clip(np.rint(smooth + np.random.default_rng(2).normal(0, 5.0, smooth.shape)), 0, 255).astype(np.uint8)
    x = orig.copy()
    x[mask > 0] = 255 - x[mask > 0]
    dil = _d(mask, gpu)
    rows = []
    out = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu, grain=CFG, grain_out=rows))
    assert (out == np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu))).all()
    assert (rows[0].n.sum((2, 3)) > 1000).all() and not rows[0].sigma_added.any() and (rows[0].sigma_orig == rows[0].sigma_model).all()
    assert (rows[0].sigma_orig > 3).any()
    both = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu, tone=TONE, grain=CFG))
    assert (both == out).all()


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=960, num_inference_steps=2, scheduler="ddim")
T, H, W = 14, 96, 160
CUT = 6
ROI = RoiConfig("static", context=0.25, pad_min=8, min_side=32)
DROP = GrainMatchConfig(flat=255, smooth=2, min_count=64, seed=5)       # random weights give no flat rendering of the surroundings: every ring pixel counts
DROP_FIT = dict(mode=DROP.mode, ring=DROP.ring, flat=DROP.flat, seed=DROP.seed, smooth=DROP.smooth, strength=DROP.strength, max_sigma=DROP.max_sigma,
                min_count=DROP.min_count)


@pytest.fixture(scope="module")
def clip():
    """A static box in frames 2 .. 10 of a panning shot with grain of sigma 16, and a prior."""
    frames, _ = spans_ref.shots_clip(61, (T,), (3,), H, W)
    rng = np.random.default_rng(62)
    frames = [np.clip(np.rint(f + rng.normal(0, 16.0, f.shape)), 0, 255).astype(np.uint8) for f in frames]
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
    """run(**kw) -> (output frames, last_grain_match, the model's frames of every stages.run_model call) of the drop-in on the tiny architecture;
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
                seen[key] = (out, diffuerase.last_grain_match, [np.stack(m) for m in model])
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
    out, rep, model = run(grain_match=DROP)
    assert none is None and len(model) == 1 and len(out) == T
    want, s, so, sm, sa = R.apply(model[0], np.stack(frames), dil, np.zeros((T, 2), np.int32), H, W, 3.0, np.arange(T), **DROP_FIT)
    assert (np.stack(out) == want).all()
    assert rep.n.shape == rep.sigma_orig.shape == rep.sigma_model.shape == rep.sigma_added.shape == (1, T, 3, 4)
    _report_equals(rep, 0, s, so, sm, sa)
    quiet = [0, 1, 11, 12, 13]
    print("sigma of the original / the model / added, frame 5:", rep.sigma_orig[0, 5].round(2).tolist(), rep.sigma_model[0, 5].round(2).tolist(),
          rep.sigma_added[0, 5].round(2).tolist())
    assert (rep.n[0, 2:11].sum((1, 2)) > 1500).all() and not rep.n[0, quiet].any() and not rep.sigma_added[0, quiet].any()
    assert (rep.sigma_added[0, 2:11] > 0).any()                                                      # the clip's grain is missing from the model's frames
    # the stage moves only pixels the composite takes from the model
    alpha = np.stack([I.feather_alpha(d, 3) for d in dil])
    differs = (np.stack(out) != np.stack(base)).any(-1)
    assert differs.any() and not differs[alpha == 0].any()


def test_drop_in_with_a_window(gpu, clip, run, dil):
    frames, masks, prior = clip
    out, rep, model = run(grain_match=DROP, roi=ROI)
    bb = np.zeros((T, 4), np.int32)
    for t in range(T):
        ys, xs = np.nonzero(dil[t])
        if len(ys):
            bb[t] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
    plan = plan_roi(bb, H, W, 3, ROI)
    h, w = plan.size
    assert h < H and w < W and len(model) == 1 and model[0].shape[0] == T
    want, s, so, sm, sa = R.apply(model[0], np.stack(frames), dil, plan.offsets, h, w, 3.0, np.arange(T), **DROP_FIT)
    assert (np.stack(out) == want).all()
    _report_equals(rep, 0, s, so, sm, sa)
    inside = np.zeros((T, H, W), bool)
    for t, (oy, ox) in enumerate(plan.offsets.tolist()):
        inside[t, oy:oy + h, ox:ox + w] = True
    assert (np.stack(out)[~inside] == np.stack(frames)[~inside]).all() and (~inside).any()        # outside the window: the original bytes
    assert (rep.sigma_added > 0).any() and not (np.stack(out) == np.stack(run(roi=ROI)[0])).all()


def test_drop_in_with_a_cut_keys_the_noise_on_the_calls_frames(gpu, clip, run, dil):
    """spans="cuts", cuts=[6]: two clip calls; each is the restatement on its own model frames, fitted inside the span, with the noise of the
    frames' indices in the CALL.  Counting the second span's frames from 0 gives other bytes."""
    frames, masks, prior = clip
    out, rep, model = run(grain_match=DROP, spans="cuts", cuts=[CUT])
    assert len(model) == 2 and len(model[0]) == CUT and len(model[1]) == T - CUT and rep.n.shape == (1, T, 3, 4)
    for m, (a, b) in zip(model, ((0, CUT), (CUT, T))):
        args = (m, np.stack(frames[a:b]), dil[a:b], np.zeros((b - a, 2), np.int32), H, W, 3.0)
        want, s, so, sm, sa = R.apply(*args, np.arange(a, b), **DROP_FIT)
        assert (np.stack(out[a:b]) == want).all()
        _report_equals(rep, 0, s, so, sm, sa, a=a)
        assert (sa > 0).any()
        if a:
            assert not (np.stack(out[a:b]) == R.apply(*args, np.arange(b - a), **DROP_FIT)[0]).all()


def test_drop_in_off_is_the_plain_call(gpu, clip, run):
    base, none, _ = run()
    off, rep, _ = run(grain_match="off")
    assert none is None and rep is None and (np.stack(off) == np.stack(base)).all()
