"""Seam membrane blending on the GPU: the entry points of vv_blend.hip against the numpy / scipy restatement (tests/seamblend_ref.py) byte for
byte, each run twice with identical bytes; the blocked relax against single sweeps; the paste against the grain and tone pastes; infill.finish
with the stage on against the restatement and against the call without it; and the drop-in's seam_blend= path on the tiny architecture against
the restatement applied to the model's own frames.  No tolerances."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grainmatch_ref as GR  # noqa: E402
import seamblend_ref as R  # noqa: E402
import spans_ref  # noqa: E402
import tonematch_ref as TR  # noqa: E402
from test_tonematch_gpu import _frame_masks  # noqa: E402

from videovanish_amd import seamblend as M  # noqa: E402
from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.grainmatch import GrainMatchConfig  # noqa: E402
from videovanish_amd.roi import RoiConfig, RoiPlan, plan_roi  # noqa: E402
from videovanish_amd.seamblend import SeamBlendConfig  # noqa: E402
from videovanish_amd.tonematch import ToneMatchConfig  # noqa: E402


def _d(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _n(t):
    return t.cpu().numpy()


def _ident(T):
    return np.ascontiguousarray(np.broadcast_to(R.IDENT, (T, 3, 256)))


def _bent_tables(T):
    """[T,3,256]: a compressed, a lifted and an identity table."""
    v = np.arange(256)
    return np.ascontiguousarray(np.broadcast_to(np.stack([v * 3 // 4 + 20, np.minimum(v + 9, 255), v]).astype(np.uint8), (T, 3, 256)))


def _pair(rng, T, H, W, hm=None, wm=None, grain=3.0):
    """(orig [T,H,W,3], patch [T,hm,wm,3]): smooth textures with grain, and a model rendering with a tone error that varies across the frame."""
    hm, wm = hm or H, wm or W
    orig = np.stack([TR.smooth_texture(int(rng.integers(1 << 30)), H, W) for _ in range(T)]).astype(np.float64)
    orig = np.clip(np.rint(orig + rng.normal(0, grain, orig.shape)), 0, 255).astype(np.uint8)
    patch = np.stack([TR.smooth_texture(int(rng.integers(1 << 30)), hm, wm, lo=40, hi=200) for _ in range(T)]).astype(np.uint8)
    return orig, patch


def _solve_both(patch, orig, mask, offs, lut, h, w, ring, presmooth, sweeps, max_shift, gpu):
    """vvb_ring_diff and vvb_solve, each twice, against the restatement; -> (field, cls, sums) of the restatement."""
    from videovanish_amd import blend_hip
    args = [_d(a, gpu) for a in (patch, orig, mask, np.asarray(offs, np.int32), lut)]
    T = len(patch)
    wc, wv, ws = R.level0(patch, orig, mask, offs, lut, h, w, ring, presmooth, max_shift)
    for _ in range(2):
        cls, val, sums = blend_hip.ring_diff(*args, h, w, ring, presmooth, max_shift)
        assert cls.shape == (T, h, w) and val.shape == (T, h, w, 3) and sums.shape == (T, 11) and sums.dtype == torch.int64
        assert (_n(cls) == wc).all() and (_n(val) == wv).all() and (_n(sums) == ws).all(), (ring, presmooth, max_shift)
    field, cls, sums = R.solve(patch, orig, mask, offs, lut, h, w, ring, presmooth, sweeps, max_shift)
    for _ in range(2):
        scratch = torch.full((blend_hip.scratch_bytes(T, h, w),), 0xA5, dtype=torch.uint8, device=gpu)      # nothing is read before it is written
        f, c, s = blend_hip.solve(*args, h, w, ring, presmooth, sweeps, max_shift, scratch=scratch)
        assert f.dtype == torch.int16 and f.shape == (T, h, w, 3) and f.data_ptr() == scratch.data_ptr()
        assert (_n(c) == cls).all() and (_n(s) == sums).all(), (_n(s).tolist(), sums.tolist())
        assert (_n(f) == field).all(), (ring, presmooth, sweeps, max_shift, int((_n(f) != field).sum()))
    return field, cls, sums


# ---- the field ----------------------------------------------------------------------------------------------------------------------------
PARAMS = [(1, 0, 1, 32), (12, 2, 8, 32), (32, 4, 16, 255), (12, 2, 8, 3)]          # ring, presmooth, sweeps, max_shift (3: small enough to clamp)


@pytest.mark.parametrize("ring,presmooth,sweeps,max_shift", PARAMS)
@pytest.mark.parametrize("H,W", [(37, 53), (96, 130)])
def test_solve_full_frame(gpu, H, W, ring, presmooth, sweeps, max_shift):
    """37 x 53 is smaller than a tile, 96 x 130 has a two-column remainder tile; the nine masks of the tone test: empty, full, corners, edge
    bars, blobs next to the frame edge, random specks."""
    from videovanish_amd import blend_hip
    rng = np.random.default_rng(H * 1000 + ring)
    mask = _frame_masks(H, W, 3)
    T = len(mask)
    orig, patch = _pair(rng, T, H, W)
    assert blend_hip.scratch_bytes(T, H, W) == M.scratch_bytes(T, H, W)
    field, cls, sums = _solve_both(patch, orig, mask, np.zeros((T, 2), np.int32), _bent_tables(T), H, W, ring, presmooth, sweeps, max_shift, gpu)
    assert not field[0].any() and not field[1].any() and (cls[0] == R.INACTIVE).all() and (cls[1] == R.UNKNOWN).all()      # no mask, no ring: zero
    assert sums[1].tolist() == [0, 0, 0, 0, H * W, 0, 0, 0, 0, 0, 0] and (sums[2:, 0] > 0).all() and field[2:].any()
    assert np.abs(field).max() <= 64 * max_shift and (max_shift != 3 or np.abs(field).max() == 64 * 3)


def _corner_blob(H=96, W=130):
    """A blob across the corner of the tiles at (x, y) = (64, 32), with a hole, and a second component in the remainder tile."""
    yy, xx = np.mgrid[:H, :W]
    m = ((yy - 32) ** 2 + (xx - 64) ** 2 <= 20 ** 2) & ((yy - 30) ** 2 + (xx - 60) ** 2 > 5 ** 2)
    m[70:90, 120:130] = True
    return (m * 255).astype(np.uint8)


def test_solve_in_a_window_with_a_resized_patch(gpu):
    """A window smaller than the frame, at its own place per frame, whose mask runs over the window's edge (the field replicates there), and a
    patch of another size than the window (the resize path)."""
    rng = np.random.default_rng(11)
    T, H, W, h, w = 3, 96, 130, 50, 70
    orig, patch = _pair(rng, T, H, W, 40, 56)
    mask = np.stack([_corner_blob()] * T)
    offs = np.array([[20, 50], [30, 60], [46, 60]], np.int32)
    field, cls, sums = _solve_both(patch, orig, mask, offs, _bent_tables(T), h, w, 12, 2, 8, 32, gpu)
    assert all((cls[t][[0, -1]] == R.UNKNOWN).any() or (cls[t][:, [0, -1]] == R.UNKNOWN).any() for t in range(T))       # the mask reaches the edge
    assert (sums[:, 4] < (mask[0] > 0).sum()).all() and field.any()


def test_solve_in_a_window_that_hangs_over_the_frame(gpu):
    """Offsets that put part of the window outside the frame (above and left, below and right, right): the cells there are inactive, hold 0
    and are never read; a masked pixel next to the frame's edge replicates its own value towards them."""
    rng = np.random.default_rng(12)
    T, H, W, h, w = 3, 96, 130, 50, 70
    orig, patch = _pair(rng, T, H, W, h, w)
    mask = np.stack([_frame_masks(H, W, 3)[3], _frame_masks(H, W, 3)[4], _corner_blob()])          # bars along the frame's edges; the blob
    offs = np.array([[-10, -20], [60, 80], [-5, 70]], np.int32)
    field, cls, sums = _solve_both(patch, orig, mask, offs, _bent_tables(T), h, w, 12, 2, 8, 32, gpu)
    assert (cls[0][:10] == R.INACTIVE).all() and (cls[0][:, :20] == R.INACTIVE).all() and (cls[1][36:] == R.INACTIVE).all()
    assert (cls[1][:, 50:] == R.INACTIVE).all() and (cls[2][:5] == R.INACTIVE).all() and (cls[2][:, 60:] == R.INACTIVE).all()
    assert not field[cls == R.INACTIVE].any() and (sums[:, 4] > 0).all() and (sums[:, 0] > 0).all() and field.any()
    assert (cls[0][10] == R.UNKNOWN).any() and (cls[1][35] == R.UNKNOWN).any()                      # masked pixels at the frame's edge


@pytest.mark.parametrize("s", [8, 16])
@pytest.mark.parametrize("level", [0, 1])
def test_one_blocked_launch_equals_single_sweeps(gpu, s, level):
    """The halo: one launch with sweeps = s equals s launches with sweeps = 1 on the same level (96 x 130: tiles meet inside the blob at
    (64, 32); level 1 is 48 x 65, two tiles), and both equal the restatement; the pull steps equal it too."""
    from videovanish_amd import blend_hip
    rng = np.random.default_rng(s)
    T, H, W = 2, 96, 130
    orig, patch = _pair(rng, T, H, W)
    mask = np.stack([_corner_blob(), _frame_masks(H, W, 5)[6]])
    args = [_d(a, gpu) for a in (patch, orig, mask, np.zeros((T, 2), np.int32), _ident(T))]
    cls, val, _ = blend_hip.ring_diff(*args, H, W, 12, 2, 32)
    wc, wv, _ = R.level0(patch, orig, mask, np.zeros((T, 2), np.int32), _ident(T), H, W)
    assert (_n(cls) == wc).all() and (_n(val) == wv).all()
    ref = [[(wc[t], wv[t].astype(np.int64)) for t in range(T)]]         # per level and frame: (classes, values)
    levels = [(cls, val)]
    for l in range(2):
        levels.append(blend_hip.pull(*levels[-1]))
        again = blend_hip.pull(*levels[-2])
        assert (_n(again[0]) == _n(levels[-1][0])).all() and (_n(again[1]) == _n(levels[-1][1])).all()
        ref.append([R.pull(*ref[-1][t]) for t in range(T)])
        assert (_n(levels[-1][0]) == np.stack([c for c, _ in ref[-1]])).all() and (_n(levels[-1][1]) == np.stack([v for _, v in ref[-1]])).all()
    cls, val = levels[level]
    parent = levels[level + 1][1]
    sums = [torch.zeros((T, 11), dtype=torch.int64, device=gpu) for _ in range(2)]
    one = blend_hip.relax(cls, val, s, parent=parent, sums=sums[0])
    again = blend_hip.relax(cls, val, s, parent=parent)
    def chain(acc=None):
        step = blend_hip.relax(cls, val, 1, parent=parent)
        for k in range(1, s):
            step = blend_hip.relax(cls, step, 1, start=False, sums=acc if k == s - 1 else None)
        return step

    step = chain(sums[1])
    assert (_n(chain()) == _n(step)).all()
    want = np.stack([R.relax(ref[level][t][0], ref[level][t][1], s, ref[level + 1][t][1]) for t in range(T)])
    assert (_n(one) == _n(again)).all() and (_n(one) == _n(step)).all() and (_n(one) == want).all()
    assert (_n(sums[0]) == _n(sums[1])).all() and (_n(sums[0]) == R.field_sums(_n(cls), want, np.zeros((T, 11), np.int64))).all()
    # in place, and from zero without a parent
    for _ in range(2):
        inplace = val.clone()
        assert blend_hip.relax(cls, inplace, s, parent=parent, out=inplace).data_ptr() == inplace.data_ptr() and (_n(inplace) == want).all()
    zero = blend_hip.relax(cls, val, s)
    assert (_n(blend_hip.relax(cls, val, s)) == _n(zero)).all()
    assert (_n(zero) == np.stack([R.relax(ref[level][t][0], ref[level][t][1], s) for t in range(T)])).all() and (_n(zero) != want).any()


# ---- the paste ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feather", [3.0, 0.0, -1.0])
@pytest.mark.parametrize("resize", [False, True])
def test_paste_blend_composite(gpu, resize, feather):
    from videovanish_amd import blend_hip, grain_hip, tone_hip
    rng = np.random.default_rng(21)
    T, H, W, h, w = 3, 96, 130, 50, 70
    orig, patch = _pair(rng, T, H, W, *((40, 56) if resize else (h, w)))
    mask = np.stack([_corner_blob()] * T)
    offs = np.array([[20, 50], [30, 60], [46, 60]], np.int32)
    lut, ids = _bent_tables(T), np.array([4, 5, 9], np.int32)
    amp = rng.integers(0, 200, (T, 3, 256)).astype(np.uint8)
    field = rng.integers(-64 * 40, 64 * 40, (T, h, w, 3)).astype(np.int16)
    args = [_d(a, gpu) for a in (patch, orig, mask, offs, lut)]
    for q8, mode in ((256, 0), (192, 1), (512, 0)):
        got = [_n(blend_hip.paste_blend_composite(*args, _d(field, gpu), q8, _d(amp, gpu), _d(ids, gpu), 7, mode, h, w, feather)) for _ in range(2)]
        want = R.composite(patch, orig, mask, offs, lut, field, q8, amp, ids, 7, GR_MODES[mode], h, w, feather)
        assert (got[0] == got[1]).all() and (got[0] == want).all(), (q8, mode)
    # a zero field, or no strength: the grain paste's bytes; zero amplitudes as well: the tone paste's
    grain = _n(grain_hip.paste_grain_composite(*args, _d(amp, gpu), _d(ids, gpu), 7, 1, h, w, feather))
    zero_f, zero_a = _d(np.zeros_like(field), gpu), _d(np.zeros_like(amp), gpu)
    assert (_n(blend_hip.paste_blend_composite(*args, zero_f, 256, _d(amp, gpu), _d(ids, gpu), 7, 1, h, w, feather)) == grain).all()
    assert (_n(blend_hip.paste_blend_composite(*args, _d(field, gpu), 0, _d(amp, gpu), _d(ids, gpu), 7, 1, h, w, feather)) == grain).all()
    tone = _n(tone_hip.paste_lut_composite(*args, h, w, feather))
    assert (_n(blend_hip.paste_blend_composite(*args, zero_f, 256, zero_a, _d(ids, gpu), 7, 0, h, w, feather)) == tone).all()
    assert (grain != tone).any() and (got[0] != grain).any()


GR_MODES = ("luma", "rgb")


def test_refusals_launch_nothing(gpu):
    """Each refusal returns its code with the function's name in vvb_last_error() and leaves the outputs as they were."""
    from videovanish_amd import blend_hip
    lib = blend_hip.lib()
    T, H, W = 1, 40, 48
    z = lambda *shape, dt=torch.uint8: torch.full(shape, 77, dtype=dt, device=gpu)
    patch, orig, mask, offs, lut = z(T, H, W, 3), z(T, H, W, 3), z(T, H, W), torch.zeros((T, 2), dtype=torch.int32, device=gpu), z(T, 3, 256)
    cls, val, sums, out = z(T, H, W), z(T, H, W, 3, dt=torch.int16), z(T, 11, dt=torch.int64), z(T, H, W, 3)
    scratch = z(M.scratch_bytes(T, H, W))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    diff = lambda ring=4, ps=2, ms=32, h=H: lib.vvb_ring_diff(p(patch), H, W, p(orig), p(mask), p(offs), p(lut), T, H, W, h, W, ring, ps, ms, p(cls), p(val),
                                                               p(sums), None)
    solve = lambda ring=4, ps=2, sw=8, ms=32, n=scratch.numel(): lib.vvb_solve(p(patch), H, W, p(orig), p(mask), p(offs), p(lut), T, H, W, H, W, ring, ps, sw,
                                                                                ms, p(scratch), n, p(sums), None)
    relax = lambda sw=8, start=1, o=val: lib.vvb_relax(p(cls), p(val), None, p(o), T, H, W, sw, start, None, None)
    paste = lambda q8=256, feather=3.0, mode=0: lib.vvb_paste_blend_composite(p(patch), H, W, p(orig), p(mask), p(offs), p(lut), p(val), q8, p(lut), p(offs),
                                                                              0, mode, T, H, W, H, W, feather, p(out), None)
    for call, name, code in ((lambda: diff(h=H + 1), b"vvb_ring_diff", -1), (lambda: diff(ring=0), b"vvb_ring_diff", -2), (lambda: diff(ring=33), b"vvb_ring_diff", -2),
                             (lambda: diff(ps=5), b"vvb_ring_diff", -2), (lambda: diff(ms=256), b"vvb_ring_diff", -2),
                             (lambda: solve(n=scratch.numel() - 1), b"vvb_solve", -1), (lambda: solve(sw=17), b"vvb_solve", -2), (lambda: solve(ps=-1), b"vvb_solve", -2),
                             (lambda: relax(sw=0), b"vvb_relax", -2), (lambda: relax(sw=17), b"vvb_relax", -2), (lambda: relax(start=0), b"vvb_relax", -1),
                             (lambda: paste(q8=513), b"vvb_paste_blend_composite", -2), (lambda: paste(feather=65.0), b"vvb_paste_blend_composite", -2),
                             (lambda: paste(mode=2), b"vvb_paste_blend_composite", -1)):
        assert call() == code and name in lib.vvb_last_error(), name
    torch.cuda.synchronize()
    for t in (cls, val, sums, out, scratch):
        assert (t == 77).all()
    with pytest.raises(RuntimeError, match="vvb_solve"):
        blend_hip.solve(patch, orig, mask, offs, lut, H, W, 4, 2, 17, 32)
    with pytest.raises(RuntimeError, match="scratch"):
        blend_hip.solve(patch, orig, mask, offs, lut, H, W, 4, 2, 8, 32, scratch=scratch[:-1])


# ---- infill.finish ------------------------------------------------------------------------------------------------------------------------
CFG = SeamBlendConfig()
TONE = ToneMatchConfig()
GRAIN = GrainMatchConfig(seed=5, min_count=64)
GRAIN_FIT = dict(seed=5, min_count=64)


def _report_equals(rep, k, sums, a=0):
    n, rms, nh, mx, mean = R.report(sums)
    b = a + len(sums)
    assert (rep.n[k, a:b] == n).all() and (rep.n_hole[k, a:b] == nh).all() and (rep.max_shift[k, a:b] == mx).all()
    assert np.allclose(rep.rms_diff[k, a:b], rms, rtol=1e-12, atol=0) and np.allclose(rep.mean_shift[k, a:b], mean, rtol=1e-12, atol=0)


@pytest.mark.parametrize("stages", ["alone", "tone", "tone+grain"])
def test_finish_full_frame(gpu, stages):
    """The full frame through infill.finish: the restatement's bytes and report; the ramp that the plain composite keeps is gone."""
    from videovanish_amd import infill
    T, H, W = 3, 96, 130
    rng = np.random.default_rng(31)
    smooth = np.stack([TR.smooth_texture(s, H, W) for s in range(T)]).astype(np.float64)
    orig = np.clip(np.rint(smooth + rng.normal(0, 3, smooth.shape)), 0, 255).astype(np.uint8)
    x = np.clip(np.rint(smooth + 2 * R.shift_field("ramp", H, W)[None]), 0, 255).astype(np.uint8)
    mask = np.stack([R.box_mask(), R.two_components(), np.zeros((H, W), np.uint8)])
    dil = _d(mask, gpu)
    kw, ref = {}, {}
    if "tone" in stages:
        kw.update(tone=TONE, tone_out=[])
        ref.update(tone=dict(ring=12))
    if "grain" in stages:
        kw.update(grain=GRAIN, grain_out=[], frame0=7)
        ref.update(grain=GRAIN_FIT)
    rows = []
    out = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu, blend=CFG, blend_out=rows, **kw))
    ids = [7, 8, 9] if "grain" in stages else [0, 1, 2]
    want, field, cls, sums = R.apply(x, orig, mask, np.zeros((T, 2), np.int32), H, W, 3.0, frame_ids=ids, **ref)
    assert (out == want).all() and field[:2].any() and not field[2].any() and (out[2] == orig[2]).all()
    assert len(rows) == 1 and rows[0].n.shape == (1, T) and rows[0].n.dtype == np.int64
    _report_equals(rows[0], 0, sums)
    if stages == "alone":
        plain = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu))
        err = lambda f: float(np.abs(f[:2].astype(int) - smooth[:2]).max())
        print(f"worst distance from the smooth original: plain {err(plain):.1f}, blended {err(out):.1f}")
        assert err(plain) >= 10 and (rows[0].max_shift[0, :2] > 6).all() and (rows[0].rms_diff[0, :2] > 3).all()
        out = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, False, gpu, blend=CFG))
        assert (out == R.apply(x, orig, mask, np.zeros((T, 2), np.int32), H, W, -1.0)[0]).all()


def test_finish_two_windows_take_their_own_shifts(gpu):
    from videovanish_amd import infill
    T, H, W = 3, 96, 130
    orig = np.stack([TR.smooth_texture(10 + s, H, W) for s in range(T)])
    wins = [((0, 0), (48, 64), (12, 15, 30, 40), "ramp"), ((50, 70), (40, 56), (60, 85, 75, 110), "vignette")]
    mask = np.zeros((T, H, W), np.uint8)
    plans, outs = [], []
    for (oy, ox), (h, w), (y0, x0, y1, x1), kind in wins:
        mask[:, y0:y1, x0:x1] = 255
        offs = np.tile(np.array([[oy, ox]], np.int32), (T, 1))
        plans.append(RoiPlan("static", (h, w), offs, offs.astype(np.float64)))
        outs.append(list(np.clip(np.rint(orig[:, oy:oy + h, ox:ox + w] + R.shift_field(kind, h, w)[None]), 0, 255).astype(np.uint8)))
    rows = []
    out = np.stack(infill.finish(outs, list(orig), _d(mask, gpu), plans, 3, True, gpu, blend=CFG, blend_out=rows))
    want = orig
    assert len(rows) == 1 and rows[0].n.shape == (2, T)
    for k, (plan, o) in enumerate(zip(plans, outs)):
        want, field, cls, sums = R.apply(np.stack(o), want, mask, plan.offsets, *plan.size, 3.0)
        _report_equals(rows[0], k, sums)
    assert (out == want).all()
    plain = np.stack(infill.finish(outs, list(orig), _d(mask, gpu), plans, 3, True, gpu))
    err = lambda f: int(np.abs(f.astype(int) - orig.astype(int)).max())
    print(f"worst error of the composite: plain {err(plain)}, blended {err(out)}")
    assert err(plain) >= 6 and err(out) <= 2


@pytest.mark.parametrize("stages", ["grain", "tone+grain"])
def test_finish_two_windows_with_the_other_stages(gpu, stages):
    """The two windows above, on originals with grain, with the membrane and grain (no tone: the identity table in front of both), and with all
    three stages: byte for byte the restatement chained over the windows, and one [2,T] report per stage."""
    from videovanish_amd import infill
    T, H, W = 3, 96, 130
    smooth = np.stack([TR.smooth_texture(10 + s, H, W) for s in range(T)]).astype(np.float64)
    orig = np.clip(np.rint(smooth + np.random.default_rng(41).normal(0, 3, smooth.shape)), 0, 255).astype(np.uint8)
    wins = [((0, 0), (48, 64), (12, 15, 30, 40), "ramp"), ((50, 70), (40, 56), (60, 85, 75, 110), "vignette")]
    mask = np.zeros((T, H, W), np.uint8)
    plans, outs = [], []
    for (oy, ox), (h, w), (y0, x0, y1, x1), kind in wins:
        mask[:, y0:y1, x0:x1] = 255
        offs = np.tile(np.array([[oy, ox]], np.int32), (T, 1))
        plans.append(RoiPlan("static", (h, w), offs, offs.astype(np.float64)))
        outs.append(list(np.clip(np.rint(smooth[:, oy:oy + h, ox:ox + w] * 0.95 + 4 + R.shift_field(kind, h, w)[None]), 0, 255).astype(np.uint8)))
    kw, ref = dict(grain=GRAIN, grain_out=[], frame0=7), dict(grain=GRAIN_FIT)
    if "tone" in stages:
        kw.update(tone=TONE, tone_out=[])
        ref.update(tone=dict(ring=12))
    rows = []
    out = np.stack(infill.finish(outs, list(orig), _d(mask, gpu), plans, 3, True, gpu, blend=CFG, blend_out=rows, **kw))
    want = orig
    assert len(rows) == 1 and rows[0].n.shape == (2, T)
    for k, (plan, o) in enumerate(zip(plans, outs)):
        want, field, cls, sums = R.apply(np.stack(o), want, mask, plan.offsets, *plan.size, 3.0, frame_ids=[7, 8, 9], **ref)
        _report_equals(rows[0], k, sums)
    assert (out == want).all()
    assert len(kw["grain_out"]) == 1 and kw["grain_out"][0].n.shape[:2] == (2, T) and kw["grain_out"][0].sigma_added.any()
    if "tone" in stages:
        assert len(kw["tone_out"]) == 1 and kw["tone_out"][0].n.shape == (2, T) and (kw["tone_out"][0].gain == 1.0).all()
        assert kw["tone_out"][0].offset.any()
        bare = np.stack(infill.finish(outs, list(orig), _d(mask, gpu), plans, 3, True, gpu, blend=CFG, grain=GRAIN, frame0=7))
        assert (bare != out).any()                                                                   # the table changes the bytes


def test_finish_without_a_difference_is_the_plain_call(gpu):
    """A model frame that equals the original on the ring, and strength 0: the bytes of the call without the option."""
    from videovanish_amd import infill
    orig, _, mask = TR.restoration_clip(1.0, 0, T=2)
    x = orig.copy()
    x[mask > 0] = 255 - x[mask > 0]
    dil = _d(mask, gpu)
    rows = []
    plain = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu))
    out = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, gpu, blend=CFG, blend_out=rows))
    assert (out == plain).all() and (rows[0].n > 2000).all() and not rows[0].rms_diff.any() and not rows[0].max_shift.any()
    x2 = np.clip(x.astype(int) + 9, 0, 255).astype(np.uint8)
    off = np.stack(infill.finish([list(x2)], list(orig), dil, [], 3, True, gpu, blend=SeamBlendConfig(strength=0.0), blend_out=rows))
    assert (off == np.stack(infill.finish([list(x2)], list(orig), dil, [], 3, True, gpu))).all() and (rows[1].max_shift > 8).all()


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=960, num_inference_steps=2, scheduler="ddim")
T, H, W = 14, 96, 160
CUT = 6
ROI = RoiConfig("static", context=0.25, pad_min=8, min_side=32)
DROP = SeamBlendConfig(sweeps=6, max_shift=64)
DROP_FIT = dict(ring=12, presmooth=2, sweeps=6, max_shift=64)
DROP_GRAIN = GrainMatchConfig(flat=255, smooth=2, min_count=64, seed=5)
DROP_GRAIN_FIT = dict(mode="luma", ring=12, flat=255, seed=5, smooth=2, strength=1.0, max_sigma=12.0, min_count=64)


@pytest.fixture(scope="module")
def clip():
    """A static box in frames 2 .. 10 of a panning shot with grain of sigma 8, and a prior."""
    frames, _ = spans_ref.shots_clip(61, (T,), (3,), H, W)
    rng = np.random.default_rng(62)
    frames = [np.clip(np.rint(f + rng.normal(0, 8.0, f.shape)), 0, 255).astype(np.uint8) for f in frames]
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
    """run(**kw) -> (output frames, last_seam_blend, the model's frames of every stages.run_model call) of the drop-in on the tiny architecture;
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
                seen[key] = (out, diffuerase.last_seam_blend, [np.stack(m) for m in model])
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
    out, rep, model = run(seam_blend=DROP)
    assert none is None and len(model) == 1 and len(out) == T
    want, field, cls, sums = R.apply(model[0], np.stack(frames), dil, np.zeros((T, 2), np.int32), H, W, 3.0, **DROP_FIT)
    assert (np.stack(out) == want).all()
    assert rep.n.shape == rep.n_hole.shape == (1, T) and rep.rms_diff.shape == rep.max_shift.shape == rep.mean_shift.shape == (1, T, 3)
    _report_equals(rep, 0, sums)
    quiet = [0, 1, 11, 12, 13]
    print("frame 5: ring pixels", int(rep.n[0, 5]), "rms", rep.rms_diff[0, 5].round(2).tolist(), "largest / mean |m|", rep.max_shift[0, 5].round(2).tolist(),
          rep.mean_shift[0, 5].round(2).tolist())
    assert (rep.n[0, 2:11] > 1500).all() and not rep.n[0, quiet].any() and not rep.max_shift[0, quiet].any() and (rep.max_shift[0, 2:11] > 0).any()
    # the stage moves only pixels the composite takes from the model
    alpha = np.stack([I.feather_alpha(d, 3) for d in dil])
    differs = (np.stack(out) != np.stack(base)).any(-1)
    assert differs.any() and not differs[alpha == 0].any()


def test_drop_in_with_tone_and_grain(gpu, clip, run, dil):
    frames, masks, prior = clip
    for kw, ref in ((dict(tone_match="on"), dict(tone=dict(ring=12))),
                    (dict(tone_match="on", grain_match=DROP_GRAIN), dict(tone=dict(ring=12), grain=DROP_GRAIN_FIT))):
        out, rep, model = run(seam_blend=DROP, **kw)
        want, field, cls, sums = R.apply(model[0], np.stack(frames), dil, np.zeros((T, 2), np.int32), H, W, 3.0, **ref, **DROP_FIT)
        assert (np.stack(out) == want).all(), sorted(kw)
        _report_equals(rep, 0, sums)
        assert not (np.stack(out) == np.stack(run(**kw)[0])).all()


def test_drop_in_with_a_window(gpu, clip, run, dil):
    frames, masks, prior = clip
    out, rep, model = run(seam_blend=DROP, roi=ROI)
    bb = np.zeros((T, 4), np.int32)
    for t in range(T):
        ys, xs = np.nonzero(dil[t])
        if len(ys):
            bb[t] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
    plan = plan_roi(bb, H, W, 3, ROI)
    h, w = plan.size
    assert h < H and w < W and len(model) == 1 and model[0].shape[0] == T
    want, field, cls, sums = R.apply(model[0], np.stack(frames), dil, plan.offsets, h, w, 3.0, **DROP_FIT)
    assert (np.stack(out) == want).all()
    _report_equals(rep, 0, sums)
    inside = np.zeros((T, H, W), bool)
    for t, (oy, ox) in enumerate(plan.offsets.tolist()):
        inside[t, oy:oy + h, ox:ox + w] = True
    assert (np.stack(out)[~inside] == np.stack(frames)[~inside]).all() and (~inside).any()        # outside the window: the original bytes
    assert (rep.max_shift > 0).any() and not (np.stack(out) == np.stack(run(roi=ROI)[0])).all()


def test_drop_in_with_a_cut(gpu, clip, run, dil):
    """spans="cuts", cuts=[6]: two clip calls; each is the restatement on its own model frames, the report assembled over the spans."""
    frames, masks, prior = clip
    out, rep, model = run(seam_blend=DROP, spans="cuts", cuts=[CUT])
    assert len(model) == 2 and len(model[0]) == CUT and len(model[1]) == T - CUT and rep.n.shape == (1, T)
    for m, (a, b) in zip(model, ((0, CUT), (CUT, T))):
        want, field, cls, sums = R.apply(m, np.stack(frames[a:b]), dil[a:b], np.zeros((b - a, 2), np.int32), H, W, 3.0, **DROP_FIT)
        assert (np.stack(out[a:b]) == want).all()
        _report_equals(rep, 0, sums, a=a)
        assert field.any()


def test_drop_in_off_is_the_plain_call(gpu, clip, run):
    base, none, _ = run()
    off, rep, _ = run(seam_blend="off")
    assert none is None and rep is None and (np.stack(off) == np.stack(base)).all()
