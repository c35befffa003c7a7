"""Shadow masking on the GPU: the four entry points of vv_shadow.hip against the numpy restatement of include/vvshadow.h
(tests/shadowmask_ref.py) byte for byte, each run twice with identical bytes; vvh_grow at its tile, halo and pass edges; vvh_plate and
vvh_candidates at their numeric edges; infill.shadow_mask alone and with cuts; and the drop-in's shadow_mask= path against the same call handed
the restatement's masks.  Tiny architecture."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import platefill_ref as P  # noqa: E402
import shadowmask_ref as R  # noqa: E402

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.roi import RoiConfig  # noqa: E402
from videovanish_amd.shadowmask import ShadowMaskConfig  # noqa: E402
from videovanish_amd.spans import SpanConfig  # noqa: E402

K = 8           # VVH_GROW_K: the halo, and the sweeps of one pass


def _d(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _twice(fn):
    """fn() -> tensors; run twice, identical bytes; the first run's results as numpy arrays."""
    a, b = fn(), fn()
    a, b = [x.cpu().numpy() for x in a], [x.cpu().numpy() for x in b]
    assert all((x == y).all() for x, y in zip(a, b))
    return a


def _check(frames, dil, gpu, **cfg):
    """One segment through the guard, vvh_plate, vvh_candidates, vvh_grow, the despeckle, the penumbra and vvh_merge, every kernel twice, every
    output against the restatement.  Returns the restatement's (dil', counts, detail)."""
    from videovanish_amd import hip, mask_hip, shadow_hip
    cfg = dict(R.DEFAULTS, **cfg)
    want_d, want_c, det = R.shadow_segment(frames, dil, detail=True, **cfg)
    f, d = _d(frames, gpu), _d(dil, gpu)
    ns = d if cfg["guard"] == 0 else mask_hip.time_bridge_grow(d, 0, cfg["guard"])[0]
    assert ((ns.cpu().numpy() != 0) == det["ns"]).all()
    ok, n2, t1 = _twice(lambda: shadow_hip.plate(f, ns, cfg["min_samples"], cfg["tol"]))
    assert ok.dtype == np.uint8 and n2.dtype == np.int32 and t1.dtype == np.int32
    assert (ok == det["ok"]).all(), int((ok != det["ok"]).sum())
    assert (n2 == det["n2"]).all() and (t1 == det["T1"]).all()
    t_ok, t_n2, t_t1 = _d(ok, gpu), _d(n2, gpu), _d(t1, gpu)
    cand, counts = _twice(lambda: shadow_hip.candidates(f, d, t_ok, t_n2, t_t1, cfg["lo"], cfg["hi"], cfg["drop"], cfg["chroma"], cfg["floor"]))
    assert set(np.unique(cand)) <= {0, 1} and ((cand != 0) == det["cand"]).all(), int(((cand != 0) != det["cand"]).sum())
    assert counts.dtype == np.int64 and (counts[:, 0] == want_c[:, 0]).all() and not counts[:, 1].any()
    t_cand = _d(cand, gpu)
    s, = _twice(lambda: (shadow_hip.grow(d, t_cand, cfg["reach"]),))
    assert set(np.unique(s)) <= {0, 255} and ((s != 0) == det["s"]).all(), int(((s != 0) != det["s"]).sum())
    t_s = _d(s, gpu)
    if cfg["min_area"] > 1:
        t_s = mask_hip.despeckle(t_s, t_s, cfg["min_area"])[0]
        assert ((t_s.cpu().numpy() != 0) == det["s6"]).all()
    if cfg["grow"]:
        t_s = hip.mask_collapse_dilate(t_s[..., None].contiguous(), cfg["grow"])

    def merge():
        c = _d(counts, gpu)
        return shadow_hip.merge(d, t_s, c), c
    got_d, got_c = _twice(merge)
    assert (got_d == want_d).all() and set(np.unique(got_d)) <= {0, 255}
    assert (got_c == want_c).all(), (got_c.tolist(), want_c.tolist())
    assert (f.cpu().numpy() == frames).all() and (d.cpu().numpy() == dil).all()               # masks change, never an input
    return want_d, want_c, det


# ---- the shared clip ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strength", [60, 85])
def test_kernels_on_the_shared_clip(gpu, strength):
    frames, dil, band, *_ = R.shadow_clip(0, strength)
    want_d, want_c, det = _check(frames, dil, gpu)
    true = band & (dil == 0)
    assert ((want_d != 0) & true).sum() == true.sum() > 0 and want_c[:, 1].sum() >= true.sum()


@pytest.mark.parametrize("cfg", [dict(guard=0, grow=0, min_area=0), dict(guard=4, reach=3, min_area=40), dict(tol=2, chroma=3, drop=40, grow=3)])
def test_kernels_parameters(gpu, cfg):
    frames, dil, *_ = R.shadow_clip(1, 75)
    _check(frames, dil, gpu, **cfg)


@pytest.mark.parametrize("cuts", [None, [9, 15]])
def test_shadow_mask_alone_and_with_cuts(gpu, cuts):
    from videovanish_amd import infill, shadow_hip
    frames, dil, band, *_ = R.shadow_clip(2, 60)
    flist = [f.copy() for f in frames]
    d = _d(dil, gpu)
    for cfg in (ShadowMaskConfig(), ShadowMaskConfig(guard=0, reach=5, grow=0, min_area=1)):
        kw = {k: getattr(cfg, k) for k in R.DEFAULTS}
        wd, wc = R.shadow_mask(frames, dil, cuts=cuts, **kw)
        got, rep = infill.shadow_mask(flist, d, cfg, cuts)
        assert got is not d and (got.cpu().numpy() == wd).all() and (rep.added == wc[:, 1]).all() and rep.added.sum() > 0
        # the candidates are counted inside the uploaded crop: never more than the full frame's, never fewer than what was added before the penumbra
        assert (rep.candidates <= wc[:, 0]).all() and rep.candidates.sum() > 0
        assert rep.cuts == tuple(cuts or ()) and rep.skipped == (False,) * len(rep.segments) and all(p > 0 for p in rep.plate)
        assert all((a == b).all() for a, b in zip(flist, frames)) and (d.cpu().numpy() == dil).all()      # the caller's arrays are never written
    got, rep = infill.shadow_mask(flist, d, ShadowMaskConfig(max_bytes=100), cuts)
    assert all(rep.skipped) and got is d and not rep.added.any()
    pf, pm, _, _ = P.panning_clip()
    pd = _d(pm, gpu)
    got, rep = infill.shadow_mask(list(pf), pd, ShadowMaskConfig(), cuts)
    assert got is pd and not rep.added.any()
    assert shadow_hip.PART.dll is not None


# ---- vvh_grow at its edges ----------------------------------------------------------------------------------------------------------------
GH = 70
REACHES = (0, 1, K - 1, K, K + 1, 2 * K, 3 * K - 1, 64)
SEEDS = ((58, 52), None, (40, 70))          # frame 0: the path's start; frame 1: a corner (set per width); frame 2: an interior pixel


def _serpentine(H, W):
    """A one-pixel path: down column x from row 58 to row 68, right along row 68 to x + 4, up column x + 4 to row 58, right along row 58, and so
    on from x = 52 to the frame's right edge.  It crosses the tile border y = 64 in every column it walks and x = 64, x = 128 along the rows."""
    c = np.zeros((H, W), bool)
    x, down = 52, True
    while x < W:
        c[58:69, x] = True
        c[68 if down else 58, x:min(x + 5, W)] = True
        x, down = x + 4, not down
    return c


@pytest.fixture(scope="module", params=[133, 136], ids=["W133-bytes", "W136-dwords"])
def grow_case(request):
    """a0, cand [3,70,W] bool and the restatement's S for every reach, computed once."""
    W = request.param
    a0, cand = np.zeros((3, GH, W), bool), np.ones((3, GH, W), bool)
    cand[0] = _serpentine(GH, W)
    seeds = [SEEDS[0], (GH - 1, W - 1), SEEDS[2]]
    for t, (y, x) in enumerate(seeds):
        a0[t, y, x] = True
    assert cand[0].sum() > 3 * 64 and cand[0, 58, 52]
    want = {r: R.geodesic(a0, cand, r) for r in REACHES}
    return W, a0, cand, seeds, want


@pytest.mark.parametrize("reach", REACHES)
def test_grow_path_and_balls_across_tiles(gpu, grow_case, reach):
    from videovanish_amd import shadow_hip
    W, a0, cand, seeds, want = grow_case
    ta, tc = _d(a0.astype(np.uint8) * 255, gpu), _d(cand.astype(np.uint8), gpu)
    s, = _twice(lambda: (shadow_hip.grow(ta, tc, reach),))
    assert set(np.unique(s)) <= {0, 255}
    assert ((s != 0) == want[reach]).all(), [int(((s[t] != 0) != want[reach][t]).sum()) for t in range(3)]
    # the restatement itself: with cand everywhere, the Chebyshev ball of radius reach round the seed, cut at the frame, without the seed
    yy, xx = np.mgrid[:GH, :W]
    for t in (1, 2):
        y, x = seeds[t]
        ball = (np.maximum(np.abs(yy - y), np.abs(xx - x)) <= reach) & ~a0[t]
        assert (want[reach][t] == ball).all()
    # the path is longer than any reach: it never fills, and it grows with every step
    grown = int(want[reach][0].sum())
    assert reach <= grown < cand[0].sum() - 1 and (reach == 0) == (grown == 0)
    if reach == 64:
        assert want[reach][0][:, 64:].any() and want[reach][0][64:].any() and want[reach][0][:64].any()      # across both borders


def test_grow_empty_candidates_and_unnormalised_bytes(gpu):
    from videovanish_amd import shadow_hip
    rng = np.random.default_rng(3)
    a0 = (rng.random((2, GH, 133)) < 0.01)
    bytes_a = np.where(a0, rng.integers(1, 256, a0.shape), 0).astype(np.uint8)      # any non-zero byte is in A_0
    none = np.zeros_like(bytes_a)
    s = shadow_hip.grow(_d(bytes_a, gpu), _d(none, gpu), 64).cpu().numpy()
    assert not s.any()                                                               # an empty cand copies through: S is empty
    cand = np.where(rng.random(a0.shape) < 0.5, rng.integers(1, 256, a0.shape), 0).astype(np.uint8)
    s = shadow_hip.grow(_d(bytes_a, gpu), _d(cand, gpu), 11).cpu().numpy()
    assert ((s != 0) == R.geodesic(a0, cand != 0, 11)).all() and set(np.unique(s)) == {0, 255}


# ---- vvh_plate and vvh_candidates at their numeric edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 3, 4, 5])
def test_plate_and_candidates_narrow_widths(gpu, W):
    rng = np.random.default_rng(10 + W)
    T, H = 12, 3
    base = rng.integers(60, 200, (1, H, W, 3))
    frames = np.clip(base + rng.integers(-3, 4, (T, H, W, 3)), 0, 255).astype(np.uint8)
    shade = rng.random((T, H, W)) < 0.3
    shade[3, 1, 0] = shade[6, 0, -1] = True                                         # a shaded pixel next to each mask
    frames[shade] = (frames[shade].astype(np.int64) * 60 // 100).astype(np.uint8)
    dil = np.zeros((T, H, W), np.uint8)
    dil[3:5, 0, 0] = 255
    dil[6, 1:, -1] = 255
    want_d, want_c, det = _check(frames, dil, gpu, min_area=0)
    assert det["ok"].any() and det["cand"].any() and want_c[:, 1].sum() > 0


def test_plate_sums_at_the_32_bit_bound(gpu):
    """T = 65535 all-255 frames of 1 x 4 pixels: n2 = 65535, T1 = 65535 * 255, T2 = 65535 * 255^2 = 2^32 - 34 301 441 in every channel, a
    variance of exactly 0."""
    from videovanish_amd import shadow_hip
    T = 65535
    f = torch.full((T, 1, 4, 3), 255, dtype=torch.uint8, device=gpu)
    ns = torch.zeros((T, 1, 4), dtype=torch.uint8, device=gpu)
    ns[7, 0, 2] = 255                                                               # one pixel loses one sample
    ok, n2, t1 = _twice(lambda: shadow_hip.plate(f, ns, 65535, 0))
    assert ok.tolist() == [[1, 1, 0, 1]] and n2.tolist() == [[T, T, T - 1, T]]       # min_samples = 65535 holds with equality, and fails one below
    assert (t1 == n2[..., None].astype(np.int64) * 255).all() and T * 255 * 255 < 2 ** 32
    # rule 4 with these sums: every product at its largest, against the restatement
    v = np.array([[[[255, 255, 255], [229, 229, 229], [229, 230, 229], [77, 77, 76]]],
                  [[[76, 76, 76], [230, 229, 229], [0, 0, 0], [128, 153, 128]]]], np.uint8)
    z = np.zeros((2, 1, 4), np.uint8)
    cfg = dict(lo=30, hi=90, drop=12, chroma=20, floor=255)
    want = R.candidates(v, z, ok != 0, n2.astype(np.int64), t1.astype(np.int64), **cfg)
    cand, counts = shadow_hip.candidates(_d(v, gpu), _d(z, gpu), _d(ok, gpu), _d(n2, gpu), _d(t1, gpu), **cfg)
    assert ((cand.cpu().numpy() != 0) == want).all() and want.any() and not want.all()
    assert counts.cpu().numpy()[:, 0].tolist() == want.reshape(2, -1).sum(1).tolist()


def test_rule_2_and_3_equalities(gpu):
    """Each pixel sits on a threshold of rule 2 or rule 3, or one step past it.  tol = 2, min_samples = 4, T = 5 with frame 4 no sample."""
    from videovanish_amd import shadow_hip
    px = {
        # rule 2: n = 4, three samples of L = 30 and one of L_s: n L_s + 3 tol n >= S is 4 L_s + 24 >= 90 + L_s, L_s >= 22
        "lit_eq": [(10, 10, 10)] * 3 + [(8, 7, 7)],             # L_s = 22: lit, n2 = 4
        "lit_past": [(10, 10, 10)] * 3 + [(7, 7, 7)],           # L_s = 21: not lit, n2 = 3 < min_samples
        # rule 3: {a, a, b, b} in one channel has the standard deviation (b - a) / 2
        "var_eq": [(10, 50, 90), (10, 50, 90), (14, 50, 90), (14, 50, 90)],        # 2 = tol: a plate
        "var_past": [(10, 50, 90), (10, 50, 90), (15, 50, 90), (15, 50, 90)],      # 2.5 > tol: none
        "var_eq_blue": [(10, 50, 90), (10, 50, 94), (10, 50, 90), (10, 50, 94)],
        "var_past_blue": [(10, 50, 89), (10, 50, 94), (10, 50, 89), (10, 50, 94)],
    }
    names = list(px)
    frames = np.zeros((5, 1, len(names), 3), np.uint8)
    for i, k in enumerate(names):
        frames[:4, 0, i] = px[k]
    frames[4] = 200
    ns = np.zeros((5, 1, len(names)), np.uint8)
    ns[4] = 255
    want_ok, want_n2, want_t1, lit = R.plate(frames, ns != 0, 4, 2)
    assert dict(zip(names, want_ok[0].tolist())) == dict(lit_eq=True, lit_past=False, var_eq=True, var_past=False, var_eq_blue=True, var_past_blue=False)
    assert want_n2[0].tolist() == [4, 3, 4, 4, 4, 4]
    for pad in (0, 2):                                                              # 6 pixels: the byte form; 8: the 4-pixel form
        f = np.concatenate([frames, frames[:, :, :pad]], 2)
        m = np.concatenate([ns, ns[:, :, :pad]], 2)
        ok, n2, t1 = shadow_hip.plate(_d(f, gpu), _d(m, gpu), 4, 2)
        assert (ok.cpu().numpy()[:, :6] != 0).tolist() == want_ok.tolist() and (n2.cpu().numpy()[:, :6] == want_n2).all()
        assert (t1.cpu().numpy()[:, :6] == want_t1).all()


def test_rule_4_equalities(gpu):
    """Every compare of rule 4 on its threshold and one step past it, the plate handed over directly: n2 = 2, T1 = 200 per channel unless stated."""
    from videovanish_amd import shadow_hip
    wide = dict(lo=0, hi=100, drop=0, chroma=100, floor=1)
    cases = [   # (settings, T1, v, candidate?)
        (dict(wide, floor=16), (32, 32, 32), (10, 10, 10), True), (dict(wide, floor=16), (32, 31, 32), (10, 10, 10), False),
        (dict(wide, lo=30), (200, 200, 200), (30, 50, 50), True), (dict(wide, lo=30), (200, 200, 200), (50, 29, 50), False),
        (dict(wide, hi=90), (200, 200, 200), (80, 80, 90), True), (dict(wide, hi=90), (200, 200, 200), (80, 80, 91), False),
        (dict(wide, drop=12), (200, 200, 200), (88, 88, 88), True), (dict(wide, drop=12), (200, 200, 200), (88, 88, 89), False),
        (dict(wide, drop=12), (200, 200, 200), (100, 100, 64), True),                                     # the sum, not each channel
        (dict(wide, chroma=20), (200, 200, 200), (80, 60, 70), True), (dict(wide, chroma=20), (200, 200, 200), (81, 60, 70), False),
        (dict(wide, chroma=20), (200, 200, 200), (70, 80, 60), True), (dict(wide, chroma=20), (200, 200, 200), (70, 81, 60), False),
        (dict(wide, chroma=20), (200, 200, 200), (80, 70, 60), True), (dict(wide, chroma=20), (200, 200, 200), (81, 70, 60), False),
        (dict(wide, chroma=20), (200, 100, 40), (80, 30, 14), True), (dict(wide, chroma=20), (200, 100, 40), (81, 30, 14), False),
        (dict(wide, chroma=0), (200, 100, 50), (80, 40, 20), True), (dict(wide, chroma=0), (200, 100, 50), (80, 40, 21), False),
        (dict(wide, hi=100), (200, 200, 200), (100, 100, 100), True),                                     # no darkening at all, drop = 0
        (dict(wide, drop=1), (200, 200, 200), (101, 100, 99), False),                                     # a signed sum of 0
        (dict(wide, hi=100), (200, 200, 200), (101, 100, 99), False),
    ]
    for pad in (0, 1):                                                              # width 1: the byte form; width 4: the 4-pixel form
        Wc = 4 if pad else 1
        for cfg, T1, v, want in cases:
            frames = np.zeros((2, 1, Wc, 3), np.uint8)
            frames[:, 0, :] = v
            dil = np.zeros((2, 1, Wc), np.uint8)
            dil[1] = 255                                                            # masked: never a candidate
            ok = np.ones((1, Wc), np.uint8)
            n2 = np.full((1, Wc), 2, np.int32)
            t1 = np.broadcast_to(np.array(T1, np.int32), (1, Wc, 3)).copy()
            if pad:
                ok[0, 3] = 0                                                        # no plate: never a candidate
            ref = R.candidates(frames, dil, ok != 0, n2.astype(np.int64), t1.astype(np.int64), **cfg)
            assert bool(ref[0, 0, 0]) is want and not ref[1].any(), (cfg, T1, v)
            cand, counts = shadow_hip.candidates(_d(frames, gpu), _d(dil, gpu), _d(ok, gpu), _d(n2, gpu), _d(t1, gpu), **cfg)
            assert ((cand.cpu().numpy() != 0) == ref).all(), (cfg, T1, v)
            assert counts.cpu().numpy().tolist() == [[int(ref[0].sum()), 0], [0, 0]]


def test_refusals_launch_nothing(gpu):
    from videovanish_amd import shadow_hip
    lib = shadow_hip.lib()
    f = torch.full((2, 8, 8, 3), 7, dtype=torch.uint8, device=gpu)
    m = torch.full((2, 8, 8), 7, dtype=torch.uint8, device=gpu)
    m2 = torch.full((2, 8, 8), 7, dtype=torch.uint8, device=gpu)
    w = torch.full((2, 8, 8, 3), 7, dtype=torch.int32, device=gpu)
    cnt = torch.full((2, 2), 7, dtype=torch.int64, device=gpu)
    p = lambda t: t.data_ptr()
    cand = lambda *v: lib.vvh_candidates(p(f), p(m), p(m), p(w), p(w), 2, 8, 8, *v, p(m2), p(cnt), None)      # lo, hi, drop, chroma, floor
    bad = [lib.vvh_plate(p(f), p(m), 0, 8, 8, 4, 6, p(m2), p(w), p(w), None), lib.vvh_plate(p(f), p(m), 2, 8, 8, 0, 6, p(m2), p(w), p(w), None),
           lib.vvh_plate(p(f), p(m), 2, 8, 8, 4, -1, p(m2), p(w), p(w), None), lib.vvh_plate(p(f), None, 2, 8, 8, 4, 6, p(m2), p(w), p(w), None),
           cand(-1, 90, 12, 20, 16), cand(91, 90, 12, 20, 16), cand(30, 90, -1, 20, 16), cand(30, 90, 12, -1, 16), cand(30, 90, 12, 20, 0),
           lib.vvh_grow(p(m), p(m2), 2, 8, 8, -1, p(f), p(w), None), lib.vvh_grow(p(m), p(m2), 2, 8, 8, 4, p(f), p(f), None),
           lib.vvh_grow(p(m), p(m2), 2, 8, 8, 4, p(m), p(f), None), lib.vvh_merge(p(m), p(m2), 2, 8, 8, p(m), p(cnt), None),
           lib.vvh_merge(p(m), p(m2), 0, 8, 8, p(f), p(cnt), None)]
    assert bad == [-1] * len(bad) and b"vvh_merge" in lib.vvh_last_error()
    unsupported = [lib.vvh_plate(p(f), p(m), 2, 8, 8, 4, 256, p(m2), p(w), p(w), None), lib.vvh_plate(p(f), p(m), 2, 8, 8, 65536, 6, p(m2), p(w), p(w), None),
                   cand(30, 101, 12, 20, 16), cand(30, 90, 256, 20, 16), cand(30, 90, 12, 101, 16), cand(30, 90, 12, 20, 256),
                   lib.vvh_grow(p(m), p(m2), 2, 8, 8, 65, p(f), p(w), None), lib.vvh_merge(p(m), p(m2), 65536, 8, 8, p(f), p(cnt), None)]
    assert unsupported == [-2] * len(unsupported) and b"65536" in lib.vvh_last_error()
    torch.cuda.synchronize()
    assert (f == 7).all() and (m == 7).all() and (m2 == 7).all() and (w == 7).all() and (cnt == 7).all()      # nothing was launched, nothing cleared
    with pytest.raises(RuntimeError, match="tol <= 255"):
        shadow_hip.plate(f, m, 4, 256)
    with pytest.raises(RuntimeError):
        shadow_hip.plate(f.cpu(), m.cpu(), 4, 6)                                                  # no CPU fallback
    with pytest.raises(ctypes.ArgumentError):
        lib.vvh_plate(p(f), p(m), 2.0, 8, 8, 4, 6, p(m2), p(w), p(w), None)


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------------
# mask_dilation_iter = 0 is no "hand the masks over as they are": as in the reference, it dilates to convergence, a whole frame as soon as one
# pixel is set, and then there is nothing left to add.  So the calls dilate by 2, and "the call without the option handed the restatement's dil'"
# is the call whose infill.shadow_mask is a stand-in that returns the restatement's dil' for the call's dilated masks, as
# tests/test_platefill_gpu.py does it for its stage.
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=960, num_inference_steps=2, scheduler="ddim")
T, H, W = 14, 96, 160
SPANS = SpanConfig("masked", context=1, min_len=3, min_gap=2)
ROI = RoiConfig("follow", context=0.25, pad_min=8, min_side=32)


@pytest.fixture(scope="module")
def clip():
    """A locked-off shot of T frames: a bright box crossing it with a shadow band under it at 60 %, and a logo masked in frames 4 .. 8 on a
    region that never holds still (so something is left to the model with plate_fill too).  -> (frames, masks as 3-channel frames, prior,
    the shadow band [T,H,W] bool)."""
    frames, masks, clean, boxm, _ = P.locked_off_clip(T, H, W, a=3, seed=5, speed=12, box=(22, 24), box_y=20, logo=None)
    band = np.zeros((T, H, W), bool)
    for t in range(T):
        x0 = -12 + 12 * t
        for r in range(10):
            band[t, 42 + r, max(x0 + 2 * r, 0):max(min(x0 + 2 * r + 30, W), 0)] = True
    band &= masks == 0
    frames[band] = (frames[band].astype(np.int64) * 60 // 100).astype(np.uint8)
    rng = np.random.default_rng(77)
    frames[:, 64:88, 96:136] = rng.integers(0, 256, (T, 24, 40, 3))
    masks[4:9, 70:80, 104:124] = 255
    prior = []
    for f, m in zip(frames, masks):
        p = f.copy()
        p[m > 0] = f.reshape(-1, 3).mean(0).astype(np.uint8)
        prior.append(p)
    return list(frames), [np.repeat(m[..., None], 3, axis=2) for m in masks], prior, band


def _run(frames, masks, prior, feather_px=3, **kw):
    import diffuerase
    diffuerase.configure(RUN)
    try:
        out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, feather_px=feather_px, **KW, **kw)
        return out, diffuerase.last_shadow_mask
    finally:
        diffuerase.configure(None)


def _restatement(gpu, frames, masks):
    """The restatement's (dil', counts) for the call's dilated masks, and those masks."""
    from videovanish_amd import hip
    dil = hip.mask_collapse_dilate(_d(np.stack(masks), gpu), KW["mask_dilation_iter"]).cpu().numpy()
    return R.shadow_mask(np.stack(frames), dil) + (dil,)


def _by_hand(monkeypatch, gpu, want_d):
    """infill.shadow_mask replaced by a stand-in that hands over the restatement's masks."""
    from videovanish_amd import infill
    z = np.zeros(T, np.int64)
    monkeypatch.setattr(infill, "shadow_mask", lambda f, d, cfg, cuts=None: (_d(want_d, gpu), infill.ShadowMaskReport(z, z, (0,), (False,), ((0, T),), ())))


def _same(a, b):
    return len(a) == len(b) == T and (np.stack(a) == np.stack(b)).all()


@pytest.mark.parametrize("more", [{}, dict(plate_fill="on"), dict(spans=SPANS, roi=ROI)], ids=["plain", "plate-fill", "spans-roi"])
def test_drop_in_equals_the_call_on_the_restatements_masks(gpu, clip, monkeypatch, more):
    frames, masks, prior, band = clip
    want_d, want_c, dil = _restatement(gpu, frames, masks)
    true = band & (dil == 0)
    assert ((want_d != 0) & true).sum() >= 0.95 * true.sum() > 0                    # the clip has a shadow, and the rules find it
    kept, kept_m = [f.copy() for f in frames], [m.copy() for m in masks]
    out, rep = _run(frames, masks, prior, shadow_mask="on", **more)
    assert rep is not None and (rep.added == want_c[:, 1]).all() and rep.added.sum() > 0 and rep.skipped == (False,)
    assert all((a == b).all() for a, b in zip(frames, kept)) and all((a == b).all() for a, b in zip(masks, kept_m))      # the caller's arrays are not written
    _by_hand(monkeypatch, gpu, want_d)
    hand, _ = _run(frames, masks, prior, shadow_mask="on", **more)
    assert _same(out, hand)
    monkeypatch.undo()
    base, none = _run(frames, masks, prior, **more)
    assert none is None and not _same(out, base)
    off, none = _run(frames, masks, prior, shadow_mask="off", **more)
    assert none is None and _same(off, base)
    far = ~P.dilate(want_d != 0, 5)                                     # further from dil' than the feather (3 px) reaches
    for t in range(T):
        assert (out[t][far[t]] == frames[t][far[t]]).all()
    if not more:
        hard, _ = _run(frames, masks, prior, feather_px=0, shadow_mask="on")
        for t in range(T):
            assert (hard[t][want_d[t] == 0] == frames[t][want_d[t] == 0]).all()      # without a feather: every pixel outside dil' keeps its bytes
        assert any((hard[t][band[t]] != frames[t][band[t]]).any() for t in range(T))  # and the shadow's pixels went to the model


def test_a_pan_adds_nothing_and_gives_the_bytes_of_the_call_without(gpu):
    pf, pm, _, _ = P.panning_clip(T=8, H=64, W=96)
    frames, masks = list(pf), [np.repeat(m[..., None], 3, axis=2) for m in pm]
    prior = [f.copy() for f in frames]
    out, rep = _run(frames, masks, prior, shadow_mask="on")
    assert rep is not None and not rep.added.any()
    base, _ = _run(frames, masks, prior)
    assert len(out) == len(base) and (np.stack(out) == np.stack(base)).all()
