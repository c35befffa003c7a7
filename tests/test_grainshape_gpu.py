"""Grain shape on the GPU: the two entry points of vv_grainshape.hip against the numpy restatement (tests/grainshape_ref.py) bit for bit, each run
twice with identical bytes; the byte-equalities with the existing pastes at zero taps; infill.finish with the option on against the restatement,
against the shape and level it has to recover and against the call without it; and the drop-in's grain_shape= path on the tiny architecture
against the restatement applied to the model's own frames.  No tolerances but the CPU-measured margins of the recovery."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grainmatch_ref as GR  # noqa: E402
import grainshape_ref as R  # noqa: E402
import tonematch_ref as TR  # noqa: E402
import spans_ref  # noqa: E402

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.grainmatch import GrainMatchConfig  # noqa: E402
from videovanish_amd.grainshape import GrainShapeConfig  # noqa: E402
from videovanish_amd.roi import RoiConfig, RoiPlan, plan_roi  # noqa: E402
from videovanish_amd.seamblend import SeamBlendConfig  # noqa: E402
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
    from videovanish_amd import grainshape_bind
    args = [_d(a, gpu) for a in (patch, orig, mask, np.asarray(offs, np.int32), lut)]
    got = _twice(lambda: grainshape_bind.ring_shape_stats(*args, h, w, ring, flat))
    want = R.sums(patch, orig, mask, offs, lut, h, w, ring, flat)
    assert got.dtype == np.int64 and got.shape == (len(patch), 30)
    assert (got == want).all(), (ring, flat, got.reshape(-1, 6, 5)[..., 0].tolist(), want.reshape(-1, 6, 5)[..., 0].tolist())
    return want.reshape(len(patch), 3, 2, 5)


# ---- ring_shape_stats -----------------------------------------------------------------------------------------------------------------------
def _frame_masks(H, W, seed):
    """The nine masks [H,W] of the grain statistic's test, restated: empty, full, one pixel in two corners, a bar along each frame edge (two
    frames), two blobs whose ring leaves the frame, random at density 0.02."""
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
    """Model frames [T,H,W,3] with every kind of neighbourhood: plateaus of 16 levels, +-3 of noise on the right half (flat 24 counts it, flat 0
    does not), steps between the plateaus and a few bright specks (only flat 255 counts them)."""
    x = np.stack([TR.smooth_texture(int(rng.integers(1 << 30)), H, W, lo=0, hi=255) for _ in range(T)]).astype(np.int64) // 16 * 16
    x[:, :, W // 2:] += rng.integers(-3, 4, x[:, :, W // 2:].shape)
    speck = rng.random(x.shape[:3]) < 0.01
    x[speck] = 255 - x[speck]
    return np.clip(x, 0, 255).astype(np.uint8)


def _bent_tables(T):
    """[T,3,256]: a negative, a compressed and an identity table."""
    v = np.arange(256)
    return np.ascontiguousarray(np.broadcast_to(np.stack([255 - v, v * 3 // 4 + 20, v]).astype(np.uint8), (T, 3, 256)))


@pytest.mark.parametrize("ring", [1, 12, 32])
@pytest.mark.parametrize("H,W", [(37, 53), (96, 130)])
def test_ring_shape_stats_full_frame(gpu, H, W, ring):
    """The full frame is the window (0, 0, H, W): 37 x 53 is smaller than a tile, 96 x 130 has pairs across columns 62 / 63 and 63 / 64 and rows
    30 / 31 and 31 / 32 (the tile pitch and the tile size) and a remainder tile.  Nine masks, flat 0 / 24 / 255, the identity table and one that
    is not."""
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
                assert (bent[:, 0] == plain[:, 0]).all() and bent[:, 0, :, 0].any()                   # the negative: L changes sign, every product stays
                assert (bent[:, 2] == plain[:, 2]).all() and not (bent[:, 1] == plain[:, 1]).all()
    print("counted (pair, channel, axis) triples:", n)
    for flat in n:
        assert n[flat][0] == 0 and n[flat][1] == 0                                                   # no mask: no ring; all mask: no unmasked pixel
    assert all(a <= b <= c for a, b, c in zip(n[0], n[24], n[255]))
    # one mask pixel in a corner: the counted pixels are the ring x ring square beside the frame's border row and column, less the one pixel that
    # touches the mask pixel: 2 ring (ring - 1) pairs less that pixel's two, 3 channels
    if ring > 1:
        assert n[255][2] == n[255][7] == 3 * (2 * ring * (ring - 1) - 2)
        assert all(v > 0 for v in n[255][2:]) and sum(n[0]) > 0 and sum(n[24]) > sum(n[0])


@pytest.mark.parametrize("ring", [1, 12, 32])
def test_ring_shape_stats_window(gpu, ring):
    """A 40 x 56 model output resized to a 48 x 64 window of a 96 x 130 frame; per-frame offsets (0, 0), the bottom-right corner and (20, 31); a
    pair whose q leaves the window or the frame is not counted (the restatement's selection is empty there); then the same window without the
    resize and the whole frame as the window of a smaller patch."""
    H, W, h, w, Hm, Wm = 96, 130, 48, 64, 40, 56
    rng = np.random.default_rng(ring)
    orig = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    patch = _plateaus(rng, 3, Hm, Wm)
    offs = np.array([[0, 0], [H - h, W - w], [20, 31]], np.int32)
    mask = np.zeros((3, H, W), np.uint8)
    mask[0, 10:30, 50:61] = 255
    mask[0, 50, 70] = 255                            # outside the window, 3 rows and 7 columns away
    mask[1, 60:80, 100:126] = 9
    mask[1, 45, 60] = 255
    mask[2] = (rng.random((H, W)) < 0.02) * 255
    for flat, lut in ((24, _ident(3)), (255, _bent_tables(3))):
        _stats(patch, orig, mask, offs, lut, h, w, ring, flat, gpu)
    # a mask pixel outside the window alone: the counted pixels are a (ring - 3) x (ring - 7) block in the window's corner, less its border
    lone = mask.copy()
    lone[0, 10:30, 50:61] = 0
    got = _stats(patch, orig, lone, offs, _ident(3), h, w, ring, 255, gpu)[0, :, :, 0]
    a, b = max(0, ring - 3), max(0, ring - 7)
    assert (got == ([a * max(b - 1, 0), max(a - 1, 0) * b] if ring > 7 else [0, 0])).all()
    _stats(_plateaus(rng, 3, h, w), orig, mask, offs, _ident(3), h, w, ring, 24, gpu)
    _stats(patch, orig, mask, np.zeros((3, 2), np.int32), _bent_tables(3), H, W, ring, 24, gpu)


def test_ring_shape_stats_sums_are_signed_and_64_bit(gpu):
    """One 128 x 128 frame with x = 128 everywhere, y a 0 / 255 checkerboard (L = +-2040, the sign alternating) and a one-column mask: at ring 32
    every pair has L(y)(p) L(y)(q) = -2040^2; the pair sums pass -2^32 and the square sums +2^33."""
    H = W = 128
    patch = np.full((1, H, W, 3), 128, np.uint8)
    yy, xx = np.mgrid[:H, :W]
    orig = np.ascontiguousarray(np.broadcast_to((((yy + xx) % 2) * 255).astype(np.uint8)[None, :, :, None], (1, H, W, 3)))
    mask = np.zeros((1, H, W), np.uint8)
    mask[0, :, 64] = 255
    want = _stats(patch, orig, mask, np.zeros((1, 2), np.int32), _ident(1), H, W, 32, 0, gpu)
    nx, ny = 2 * 30 * 126, 62 * 125                  # two 31 x 126 blocks: 30 pairs per row along x, 125 per column along y
    sq = 2040 * 2040
    assert want[0].tolist() == [[[nx, 0, -nx * sq, 0, 2 * nx * sq], [ny, 0, -ny * sq, 0, 2 * ny * sq]]] * 3
    assert -nx * sq < -2 ** 32 and 2 * nx * sq > 2 ** 33


# ---- paste_shaped_composite -------------------------------------------------------------------------------------------------------------------
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
    offs = np.zeros((T, 2), np.int32) if full else np.array([[0, 0], [0, W - w], [H - h, 0], [H - h, W - w]], np.int32)      # taps reach X = -1, W0, Y = -1, H0
    return patch, orig, mask, offs, h, w


@pytest.mark.parametrize("feather", [3.0, 0.0, -1.0])
@pytest.mark.parametrize("resize", [False, True])
@pytest.mark.parametrize("full", [False, True])
def test_paste_shaped_composite(gpu, full, resize, feather):
    from videovanish_amd import blend_hip, grain_hip, grainshape_bind, tone_hip
    patch, orig, mask, offs, h, w = _paste_inputs(3 + 2 * full + resize, full, resize)
    T = len(patch)
    rng = np.random.default_rng(9)
    lut = rng.integers(0, 256, (T, 3, 256), dtype=np.uint8)
    amp = rng.integers(0, 256, (T, 3, 256), dtype=np.uint8)                                          # up to 255: the 64-bit product and the clip are at work
    field = rng.integers(-64 * 40, 64 * 40, (T, h, w, 3)).astype(np.int16)
    taps = {"zero": np.zeros((T, 3, 2), np.int32), "binomial": np.full((T, 3, 2), 128, np.int32), "random": rng.integers(0, 129, (T, 3, 2)).astype(np.int32)}
    dp, do, dm, df, dl, da, di, dfield = (_d(a, gpu) for a in (patch, orig, mask, offs, lut, amp, FRAME_IDS, field))
    dt = {k: _d(v, gpu) for k, v in taps.items()}
    zero = torch.zeros_like(da)
    toned = tone_hip.paste_lut_composite(dp, do, dm, df, dl, h, w, feather).cpu().numpy()
    for mode, name in enumerate(("luma", "rgb")):
        call = lambda f, a, t, seed=77: grainshape_bind.paste_shaped_composite(dp, do, dm, df, dl, f, 256, a, t, di, seed, mode, h, w, feather)
        # the three byte-equalities with the existing pastes
        white = _twice(lambda: call(None, da, dt["zero"]))
        assert (white == grain_hip.paste_grain_composite(dp, do, dm, df, dl, da, di, 77, mode, h, w, feather).cpu().numpy()).all()
        blent = _twice(lambda: call(dfield, da, dt["zero"]))
        assert (blent == blend_hip.paste_blend_composite(dp, do, dm, df, dl, dfield, 256, da, di, 77, mode, h, w, feather).cpu().numpy()).all()
        assert (_twice(lambda: call(None, zero, dt["binomial"])) == toned).all() and (white != toned).any() and (blent != white).any()
        seen = [white]
        for kind in ("binomial", "random"):
            for f, df_ in ((None, None), (field, dfield)):
                got = _twice(lambda: call(df_, da, dt[kind]))
                want = R.composite(patch, orig, mask, offs, lut, f, 256, amp, taps[kind], FRAME_IDS, 77, name, h, w, feather)
                assert (got == want).all() and all((got != s).any() for s in seen), (name, kind, f is None)
                seen.append(got)
        if feather < 0:                                                                              # the plain paste needs no mask
            got = grainshape_bind.paste_shaped_composite(dp, do, None, df, dl, None, 0, da, dt["random"], di, 77, mode, h, w, feather).cpu().numpy()
            assert (got == seen[3]).all()
        buf = torch.empty_like(do)
        assert grainshape_bind.paste_shaped_composite(dp, do, dm, df, dl, None, 0, da, dt["random"], di, 77, mode, h, w, feather, out=buf) is buf
        assert (buf.cpu().numpy() == seen[3]).all()
        other = call(None, da, dt["random"], seed=78).cpu().numpy()
        assert (other == R.composite(patch, orig, mask, offs, lut, None, 0, amp, taps["random"], FRAME_IDS, 78, name, h, w, feather)).all()
        assert (other != seen[3]).any()


@pytest.mark.parametrize("mode", [0, 1])
def test_a_pixel_gets_the_same_shaped_noise_through_a_window_and_the_full_frame(gpu, mode):
    """The plain paste of a full-frame patch, and of its crops at per-frame offsets, with non-zero taps: inside each window the same bytes,
    also in the window's first and last rows and columns, whose taps lie outside it (and, at the frame's corners, outside the frame)."""
    from videovanish_amd import grainshape_bind
    T, H, W, h, w = 4, 50, 70, 24, 32
    rng = np.random.default_rng(21 + mode)
    orig = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    patch = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    lut = rng.integers(0, 256, (T, 3, 256), dtype=np.uint8)
    amp = rng.integers(1, 256, (T, 3, 256), dtype=np.uint8)
    taps = rng.integers(1, 129, (T, 3, 2)).astype(np.int32)
    offs = np.array([[0, 0], [0, W - w], [H - h, 0], [13, 29]], np.int32)
    crop = np.stack([patch[t, oy:oy + h, ox:ox + w] for t, (oy, ox) in enumerate(offs)])
    do, dl, da, dt, di = (_d(a, gpu) for a in (orig, lut, amp, taps, FRAME_IDS))
    zeros = np.zeros((T, 2), np.int32)
    whole = _twice(lambda: grainshape_bind.paste_shaped_composite(_d(patch, gpu), do, None, _d(zeros, gpu), dl, None, 0, da, dt, di, 3, mode, H, W, -1.0))
    part = _twice(lambda: grainshape_bind.paste_shaped_composite(_d(crop, gpu), do, None, _d(offs, gpu), dl, None, 0, da, dt, di, 3, mode, h, w, -1.0))
    assert (whole == R.composite(patch, orig, None, zeros, lut, None, 0, amp, taps, FRAME_IDS, 3, ("luma", "rgb")[mode], H, W, -1.0)).all()
    for t, (oy, ox) in enumerate(offs):
        assert (part[t, oy:oy + h, ox:ox + w] == whole[t, oy:oy + h, ox:ox + w]).all()
        outside = np.ones((H, W), bool)
        outside[oy:oy + h, ox:ox + w] = False
        assert (part[t][outside] == orig[t][outside]).all()
    assert (whole != np.stack([np.stack([lut[t, c][patch[t, ..., c]] for c in range(3)], -1) for t in range(T)])).mean() > 0.5


def test_refusals_launch_nothing(gpu):
    from videovanish_amd import grainshape_bind
    lib = grainshape_bind.lib()
    u8 = lambda *shape: torch.full(shape, 7, dtype=torch.uint8, device=gpu)
    patch, orig, mask, lut, amp, out = u8(2, 8, 8, 3), u8(2, 8, 8, 3), u8(2, 8, 8), u8(2, 3, 256), u8(2, 3, 256), u8(2, 8, 8, 3)
    offs = torch.zeros((2, 2), dtype=torch.int32, device=gpu)
    ids = torch.zeros(2, dtype=torch.int32, device=gpu)
    field = torch.zeros((2, 8, 8, 3), dtype=torch.int16, device=gpu)
    good = torch.full((2, 3, 2), 64, dtype=torch.int32, device=gpu)
    high, low = good.clone(), good.clone()
    high[1, 2, 1], low[0, 0, 0] = 129, -1
    sums = torch.full((2, 30), 7, dtype=torch.int64, device=gpu)
    p = lambda t: None if t is None else t.data_ptr()
    stats = lambda ring=4, flat=24, m=mask, h=8: lib.vvn_ring_shape_stats(p(patch), 8, 8, p(orig), p(m), p(offs), p(lut), 2, 8, 8, h, 8, ring, flat, p(sums), None)
    paste = lambda mode=0, feather=3.0, m=mask, a=amp, t=good, f=None, q8=256, seed=0: lib.vvn_paste_shaped_composite(
        p(patch), 8, 8, p(orig), p(m), p(offs), p(lut), p(f), q8, p(a), p(t), p(ids), seed, mode, 2, 8, 8, 8, 8, feather, p(out), None)
    assert [stats(ring=0), stats(ring=33), stats(flat=256), stats(flat=-1)] == [-2, -2, -2, -2]
    assert stats(m=None) == -1 and stats(h=9) == -1
    assert [paste(mode=2), paste(mode=-1), paste(m=None), paste(a=None), paste(t=None), paste(seed=-1)] == [-1] * 6
    assert [paste(feather=64.5), paste(q8=513), paste(f=field, q8=-1), paste(t=high), paste(t=low), paste(t=high, f=field)] == [-2] * 6
    assert b"a tap 0 .. 128" in lib.vvn_last_error()
    torch.cuda.synchronize()
    assert (sums == 7).all() and (out == 7).all()                                                   # nothing was launched, nothing cleared
    with pytest.raises(RuntimeError, match="ring 1 .. 32"):
        grainshape_bind.ring_shape_stats(patch, orig, mask, offs, lut, 8, 8, 33, 24)
    with pytest.raises(RuntimeError, match="a tap 0 .. 128"):
        grainshape_bind.paste_shaped_composite(patch, orig, mask, offs, lut, None, 0, amp, high, ids, 0, 0, 8, 8, 3.0)
    with pytest.raises(RuntimeError):
        grainshape_bind.ring_shape_stats(patch.cpu(), orig, mask, offs, lut, 8, 8, 4, 24)           # no CPU fallback
    with pytest.raises(RuntimeError):
        grainshape_bind.paste_shaped_composite(patch, orig, mask, offs, lut, None, 0, amp, good.cpu(), ids, 0, 0, 8, 8, 3.0)
    with pytest.raises(RuntimeError, match="taps must be"):
        grainshape_bind.paste_shaped_composite(patch, orig, mask, offs, lut, None, 0, amp, good[:, :, :1].contiguous(), ids, 0, 0, 8, 8, 3.0)
    with pytest.raises(RuntimeError, match="not orig itself"):
        grainshape_bind.paste_shaped_composite(patch, orig, mask, offs, lut, None, 0, amp, good, ids, 0, 0, 8, 8, 3.0, out=orig)
    assert (sums == 7).all() and (out == 7).all()
    assert paste() == 0 and paste(f=field, t=torch.full_like(good, 128)) == 0                       # the limits themselves are accepted
    torch.cuda.synchronize()
    assert (out != 7).any()


# ---- infill.finish ------------------------------------------------------------------------------------------------------------------------
CFG, SHAPE = GrainMatchConfig(), GrainShapeConfig()
GRAIN_FIT = dict(smooth=CFG.smooth, strength=CFG.strength, max_sigma=CFG.max_sigma, min_count=CFG.min_count)
SHAPE_FIT = dict(max_a=SHAPE.max_a, dead=SHAPE.dead, min_pairs=SHAPE.min_pairs, smooth=SHAPE.smooth, max_gain=SHAPE.max_gain)
TONE = ToneMatchConfig()
TONE_FIT = dict(mode=TONE.mode, ring=TONE.ring, smooth=TONE.smooth, max_gain=TONE.max_gain, max_offset=TONE.max_offset, min_count=TONE.min_count,
                min_var=TONE.min_var)


def _report_equals(rep, k, ss, f, a=0, b=None):
    rh, taps, ks, sp, clamped, dead, _ = f
    b = a + len(ss) if b is None else b
    assert (rep.pairs[k, a:b] == np.asarray(ss).reshape(-1, 3, 2, 5)[..., 0]).all() and (rep.a[k, a:b] * 256 == taps).all()
    assert (rep.clamped[k, a:b] == clamped).all() and (rep.dead[k, a:b] == dead).all() and ((rep.sigma_pixel[k, a:b] == 0) == (sp == 0)).all()
    for got, want in ((rep.rho, rh), (rep.k, ks), (rep.sigma_pixel, sp)):
        assert np.allclose(got[k, a:b], want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("shape", R.RECOVERY_SHAPES)
def test_finish_recovers_a_known_shape_and_level(gpu, shape):
    """The recovery clips of the CPU test (seeds 0 .. 3) through infill.finish on the full frame: the restatement's bytes and report, a and
    sigma_pixel within 1.5 times the CPU-measured deviations, the shaped estimate deep inside the mask of the output within its margin of
    sigma, and, with the option off, grain matching alone short of the level by the CPU-measured factor."""
    from videovanish_amd import infill
    ax, ay = shape
    for sigma in R.RECOVERY_SIGMAS:
        m = R.MEASURED_DEVIATION[shape][sigma]
        for s in range(4):
            orig, x, mask = R.recovery_clip(s, sigma, ax, ay)
            T, H, W = mask.shape
            dil = _d(mask, gpu)
            rows, grows = [], []
            out = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu, grain=CFG, grain_out=grows, grain_shape=SHAPE, grain_shape_out=rows))
            want, ss, gs, f = R.apply(x, orig, mask, np.zeros((T, 2), np.int32), H, W, 3.0, [0])
            assert (out == want).all()
            assert len(rows) == 1 and rows[0].pairs.shape == (1, T, 3, 2) and rows[0].pairs.dtype == np.int64
            _report_equals(rows[0], 0, ss, f)
            inside = R.inside_estimate(out[0], x[0], mask[0])
            white = grows[0].sigma_added[0]
            print(f"a = {shape}, sigma {sigma}, seed {s}: fitted a {rows[0].a[0, 0, 0].tolist()}, k {rows[0].k[0, 0, 0]:.3f}, sigma_pixel "
                  f"{rows[0].sigma_pixel.min():.3f} .. {rows[0].sigma_pixel.max():.3f}, inside the mask {inside.round(3).tolist()}, white fit "
                  f"{white.min():.3f} .. {white.max():.3f}")
            assert (np.abs(rows[0].a[0] - np.array([ax, ay])) <= 1.5 * m["a"]).all()
            assert (np.abs(rows[0].sigma_pixel / sigma - 1) <= 1.5 * m["sigma"]).all()
            assert (np.abs(inside / sigma - 1) <= 1.5 * m["inside"]).all()
            # the option off: the same clip's plain grain_match, which the report above restates, under-adds
            plain = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu, grain=CFG))
            assert (plain == GR.apply(x, orig, mask, np.zeros((T, 2), np.int32), H, W, 3.0, [0])[0]).all()
            assert (np.abs(white / sigma - 1) <= 1.5 * m["white"]).all() and (np.abs(white / sigma - 1) >= m["white_least"] / 1.5).all()
            if shape == (0.0, 0.0):
                assert not rows[0].a.any() and (plain == out).all()                                  # white grain: the bytes of grain_match alone
            else:
                assert (white < sigma).all() and (plain != out).any()


def test_finish_without_missing_grain_is_the_plain_call(gpu):
    """The model's frame equals the original on the ring (and is something else inside the mask): Dy == Dx, no axis is live, nothing is added:
    the bytes of the call without the option, and of the call without any stage."""
    from videovanish_amd import infill
    orig, _, mask = R.recovery_clip(2, 5, 0.5, 0.5)
    x = orig.copy()
    x[mask > 0] = 255 - x[mask > 0]
    dil = _d(mask, gpu)
    rows = []
    out = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu, grain=CFG, grain_shape=SHAPE, grain_shape_out=rows))
    assert (out == np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu, grain=CFG))).all()
    assert (out == np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu))).all()
    assert (rows[0].pairs.sum((2, 3)) > 1000).all() and not rows[0].a.any() and not rows[0].sigma_pixel.any() and (rows[0].k == 1.0).all()


def test_finish_with_tone_in_front_and_with_blend(gpu):
    """Three frames whose model frames carry a tone shift and no grain: the table first, both statistics on what it gives; then with the
    membrane, over two groups of frames."""
    from videovanish_amd import infill, seamblend
    orig, x, mask = R.recovery_clip(3, 4, 0.5, 0.25, T=3)
    shifted = np.clip(np.rint(0.9 * x.astype(np.float64) + 10), 0, 255).astype(np.uint8)
    T, H, W = mask.shape
    offs = np.zeros((T, 2), np.int32)
    rows = []
    out = np.stack(infill.finish([list(shifted)], list(orig), _d(mask, gpu), [], 3, True, gpu, tone=TONE, grain=CFG, grain_shape=SHAPE, grain_shape_out=rows, frame0=3))
    want, ss, gs, f = R.apply(shifted, orig, mask, offs, H, W, 3.0, [3, 4, 5], tone=dict(TONE_FIT))
    assert (out == want).all()
    _report_equals(rows[0], 0, ss, f)
    assert (np.abs(rows[0].a[..., 0] - 0.5) < 0.08).all() and (np.abs(rows[0].a[..., 1] - 0.25) < 0.05).all()
    blend = SeamBlendConfig(strength=0.75)
    old = seamblend.groups
    seamblend.groups = lambda n, h, w: [(0, 2), (2, n)]
    try:
        rows = []
        both = np.stack(infill.finish([list(shifted)], list(orig), _d(mask, gpu), [], 3, True, gpu, tone=TONE, grain=CFG, grain_shape=SHAPE, grain_shape_out=rows,
                                      blend=blend, frame0=3))
    finally:
        seamblend.groups = old
    want, ss, gs, f = R.apply(shifted, orig, mask, offs, H, W, 3.0, [3, 4, 5], tone=dict(TONE_FIT),
                              blend=dict(strength=0.75, ring=blend.ring, presmooth=blend.presmooth, sweeps=blend.sweeps, max_shift=blend.max_shift))
    assert (both == want).all() and (both != out).any()
    _report_equals(rows[0], 0, ss, f)


def test_finish_two_windows_are_fitted_independently(gpu):
    """K = 2: two disjoint windows on an original whose left half carries binomial grain and whose right half white grain; each window is
    fitted on its own ring, in "rgb" mode per channel."""
    from videovanish_amd import infill
    T, H, W = 3, 96, 130
    soft, smooth, _ = R.recovery_clip(5, 5, 0.5, 0.5, T=T)
    white = R.recovery_clip(6, 5, 0.0, 0.0, T=T)[0]
    orig = np.concatenate([soft[:, :, :67], white[:, :, 67:]], axis=2)
    wins = [((0, 0), (60, 64), (14, 15, 40, 44)), ((30, 70), (60, 58), (46, 85, 74, 112))]
    mask = np.zeros((T, H, W), np.uint8)
    plans, outs = [], []
    for (oy, ox), (h, w), (y0, x0, y1, x1) in wins:
        mask[:, y0:y1, x0:x1] = 255
        offs = np.tile(np.array([[oy, ox]], np.int32), (T, 1))
        plans.append(RoiPlan("static", (h, w), offs, offs.astype(np.float64)))
        outs.append(list(smooth[:, oy:oy + h, ox:ox + w].copy()))
    rows = []
    cfg = GrainMatchConfig(mode="rgb", seed=9)
    out = np.stack(infill.finish(outs, list(orig), _d(mask, gpu), plans, 3, True, gpu, grain=cfg, grain_shape=SHAPE, grain_shape_out=rows, frame0=100))
    want = orig
    assert len(rows) == 1 and rows[0].pairs.shape == (2, T, 3, 2)
    for k, (plan, o) in enumerate(zip(plans, outs)):
        want, ss, gs, f = R.apply(np.stack(o), want, mask, plan.offsets, *plan.size, 3.0, [100, 101, 102], mode="rgb", seed=9)
        _report_equals(rows[0], k, ss, f)
    assert (out == want).all()
    print("fitted a:", rows[0].a[:, 0].tolist())
    assert (rows[0].a[0] > 0.35).all() and not rows[0].a[1].any() and (rows[0].k[0] > 3).all() and (rows[0].k[1] == 1.0).all()


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=960, num_inference_steps=2, scheduler="ddim")
T, H, W = 14, 96, 160
CUT = 6
ROI = RoiConfig("static", context=0.25, pad_min=8, min_side=32)
DROP = GrainMatchConfig(flat=255, smooth=2, min_count=64, seed=5)       # random weights give no flat rendering of the surroundings: every ring pixel counts
DROP_SHAPE = GrainShapeConfig(smooth=2, min_pairs=128, dead=0.0)      # the tiny model's frames are noisy themselves: every live fit counts
DROP_FIT = dict(mode=DROP.mode, ring=DROP.ring, flat=DROP.flat, seed=DROP.seed,
                grain=dict(smooth=DROP.smooth, strength=DROP.strength, max_sigma=DROP.max_sigma, min_count=DROP.min_count),
                max_a=DROP_SHAPE.max_a, dead=DROP_SHAPE.dead, min_pairs=DROP_SHAPE.min_pairs, smooth=DROP_SHAPE.smooth, max_gain=DROP_SHAPE.max_gain)


@pytest.fixture(scope="module")
def clip():
    """A static box in frames 2 .. 10 of a panning shot with grain of sigma 32 shaped by a = 0.25 on both axes, and a prior."""
    frames, _ = spans_ref.shots_clip(61, (T,), (3,), H, W)
    rng = np.random.default_rng(62)
    frames = [np.clip(np.rint(f + R.shape_noise(rng, 32.0, f.shape, 0.25, 0.25)), 0, 255).astype(np.uint8) for f in frames]
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
    """run(**kw) -> (output frames, last_grain_shape, the model's frames of every stages.run_model call) of the drop-in on the tiny architecture;
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
                seen[key] = (out, diffuerase.last_grain_shape, [np.stack(m) for m in model])
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
    frames, masks, prior = clip
    out, rep, model = run(grain_match=DROP, grain_shape=DROP_SHAPE)
    assert len(model) == 1 and len(out) == T
    want, ss, gs, f = R.apply(model[0], np.stack(frames), dil, np.zeros((T, 2), np.int32), H, W, 3.0, np.arange(T), **DROP_FIT)
    assert (np.stack(out) == want).all()
    assert rep.pairs.shape == rep.a.shape == (1, T, 3, 2) and rep.k.shape == (1, T, 3) and rep.sigma_pixel.shape == (1, T, 3, 4)
    _report_equals(rep, 0, ss, f)
    quiet = [0, 1, 11, 12, 13]
    print("fitted a / k / sigma_pixel, frame 5:", rep.a[0, 5].tolist(), rep.k[0, 5].round(2).tolist(), rep.sigma_pixel[0, 5].round(2).tolist())
    assert (rep.pairs[0, 2:11].sum((1, 2)) > 1500).all() and not rep.pairs[0, quiet].any() and not rep.sigma_pixel[0, quiet].any()
    assert (rep.sigma_pixel[0, 2:11] > 0).any() and rep.a[0, 2:11].any()                             # shaped noise is at work
    # the option off: the bytes of grain_match alone, which differ where the shape is fitted
    off, none, _ = run(grain_match=DROP, grain_shape="off")
    alone, none2, _ = run(grain_match=DROP)
    assert none is None and none2 is None and (np.stack(off) == np.stack(alone)).all()
    assert (np.stack(alone) != np.stack(out)).any() == bool(rep.a.any())


def test_drop_in_with_a_window(gpu, clip, run, dil):
    frames, masks, prior = clip
    out, rep, model = run(grain_match=DROP, grain_shape=DROP_SHAPE, roi=ROI)
    bb = np.zeros((T, 4), np.int32)
    for t in range(T):
        ys, xs = np.nonzero(dil[t])
        if len(ys):
            bb[t] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
    plan = plan_roi(bb, H, W, 3, ROI)
    h, w = plan.size
    assert h < H and w < W and len(model) == 1 and model[0].shape[0] == T
    want, ss, gs, f = R.apply(model[0], np.stack(frames), dil, plan.offsets, h, w, 3.0, np.arange(T), **DROP_FIT)
    assert (np.stack(out) == want).all()
    _report_equals(rep, 0, ss, f)
    inside = np.zeros((T, H, W), bool)
    for t, (oy, ox) in enumerate(plan.offsets.tolist()):
        inside[t, oy:oy + h, ox:ox + w] = True
    assert (np.stack(out)[~inside] == np.stack(frames)[~inside]).all() and (~inside).any()        # outside the window: the original bytes
    assert (rep.sigma_pixel > 0).any()


def test_drop_in_with_a_cut_fits_each_span_on_its_own(gpu, clip, run, dil):
    """spans="cuts", cuts=[6]: two clip calls; each is the restatement on its own model frames, pooled inside the span, with the noise of the
    frames' indices in the CALL."""
    frames, masks, prior = clip
    out, rep, model = run(grain_match=DROP, grain_shape=DROP_SHAPE, spans="cuts", cuts=[CUT])
    assert len(model) == 2 and len(model[0]) == CUT and len(model[1]) == T - CUT and rep.pairs.shape == (1, T, 3, 2)
    for m, (a, b) in zip(model, ((0, CUT), (CUT, T))):
        want, ss, gs, f = R.apply(m, np.stack(frames[a:b]), dil[a:b], np.zeros((b - a, 2), np.int32), H, W, 3.0, np.arange(a, b), **DROP_FIT)
        assert (np.stack(out[a:b]) == want).all()
        _report_equals(rep, 0, ss, f, a=a)
    assert (rep.sigma_pixel > 0).any() and rep.a.any()
