"""Mask-region inference with one window per separate masked region, host side: the tile labelling (roi.label_tiles) against a brute-force flood
fill, the region planner (roi.plan_regions) as properties over random sets of box tracks, worked examples, the new spellings of the setting, the
one crop -> prior -> model sequence (infill.run_windows) for no, one and two windows with fake stages, and the argument checks of the two new
entry points.  No GPU."""
import ctypes
import math
import os
import sys
import types

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from videovanish_amd import roi
from videovanish_amd.roi import RoiConfig, as_config, label_tiles, plan_regions, plan_roi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "videovanish_amd", "csrc", "libvvhip.so")


# ---- labelling ------------------------------------------------------------------------------------------------------------------------
def _flood(g):
    """Brute force: repeated 8-neighbour propagation of the smallest cell index until nothing changes, as a partition {cell: root}."""
    H, W = g.shape
    lab = np.where(g, np.arange(H * W).reshape(H, W), -1)
    while True:
        p = np.pad(lab, 1, constant_values=-1)
        best = lab.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nb = p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
                best = np.where(g & (nb >= 0), np.minimum(best, np.where(nb >= 0, nb, best)), best)
        if (best == lab).all():
            return lab
        lab = best


def _canon(lab):
    """Labels renumbered by the raster order of each component's first cell (-1 stays -1)."""
    out = np.full(lab.shape, -1, np.int64)
    seen = {}
    for i, v in enumerate(lab.ravel().tolist()):
        if v >= 0:
            out.flat[i] = seen.setdefault(v, len(seen))
    return out


@settings(max_examples=150, deadline=None)
@given(st.integers(1, 24), st.integers(1, 24), st.sampled_from([0.05, 0.2, 0.4, 0.6]), st.integers(0, 2 ** 31))
def test_label_tiles_matches_flood_fill(H, W, p, seed):
    g = np.random.default_rng(seed).random((H, W)) < p
    lab, K, tile = label_tiles(g.astype(np.uint8), max_components=H * W + 1)
    assert tile == 16 and lab.dtype == np.int32 and lab.shape == (H, W)
    assert ((lab >= 0) == g).all()
    assert (_canon(lab) == _canon(_flood(g))).all()
    assert K == len(np.unique(lab[lab >= 0]))


@settings(max_examples=100, deadline=None)
@given(st.integers(1, 70), st.integers(1, 130), st.sampled_from([0.05, 0.3, 0.5]), st.sampled_from([1, 4, 16, 64]), st.integers(0, 2 ** 31))
def test_label_tiles_coarsening_bounds_k_and_only_merges(H, W, p, cap, seed):
    g = np.random.default_rng(seed).random((H, W)) < p
    fine, _, _ = label_tiles(g, max_components=H * W + 1)
    lab, K, tile = label_tiles(g, max_components=cap)
    assert K <= cap and tile >= 16
    f = tile // 16
    assert f & (f - 1) == 0 and lab.shape == (-(-H // f), -(-W // f))
    pooled = np.zeros(lab.shape, bool)                          # the coarse grid is the OR-pool of the fine one
    ys, xs = np.nonzero(g)
    pooled[ys // f, xs // f] = True
    assert ((lab >= 0) == pooled).all()
    for k in np.unique(fine[fine >= 0]):                        # a fine component lies in exactly one coarse component
        ys, xs = np.nonzero(fine == k)
        assert len(np.unique(lab[ys // f, xs // f])) == 1
    assert (_canon(lab) == _canon(_flood(lab >= 0))).all()


def test_label_tiles_salt_and_empty():
    salt = np.zeros((68, 120), np.uint8)
    salt[::2, ::2] = 1                                          # 2040 isolated tiles (a 1080p salt mask at 16 px)
    lab, K, tile = label_tiles(salt)
    assert K <= 64 and tile > 16
    lab, K, tile = label_tiles(np.zeros((5, 7), np.uint8))
    assert K == 0 and (lab == -1).all() and tile == 16


# ---- planner --------------------------------------------------------------------------------------------------------------------------
def _empty(b):
    return b[2] <= b[0] or b[3] <= b[1]


@st.composite
def region_tracks(draw):
    """(bboxes [T,K,4], H0, W0): 1-4 boxes, each drifting across the frame with size jitter and gaps (empty frames)."""
    H0 = draw(st.integers(16, 1100))
    W0 = draw(st.integers(16, 2000))
    T = draw(st.integers(1, 24))
    n = draw(st.integers(1, 4))
    rng = np.random.default_rng(draw(st.integers(0, 2 ** 31)))
    out = np.zeros((T, n, 4), np.int64)
    for k in range(n):
        bh = int(rng.integers(1, max(2, H0 // draw(st.sampled_from([1, 4, 12])))))
        bw = int(rng.integers(1, max(2, W0 // draw(st.sampled_from([1, 4, 12])))))
        y, x = int(rng.integers(0, H0 - bh + 1)), int(rng.integers(0, W0 - bw + 1))
        vy, vx = draw(st.integers(-12, 12)), draw(st.integers(-12, 12))
        gap_p = draw(st.sampled_from([0.0, 0.2, 0.6]))
        for t in range(T):
            h = int(np.clip(bh + rng.integers(-3, 4), 1, H0))
            w = int(np.clip(bw + rng.integers(-3, 4), 1, W0))
            y0 = int(np.clip(y + vy * t + rng.integers(-2, 3), 0, H0 - h))
            x0 = int(np.clip(x + vx * t + rng.integers(-2, 3), 0, W0 - w))
            if rng.random() >= gap_p:
                out[t, k] = (y0, x0, y0 + h, x0 + w)
    return out, H0, W0


cfgs = st.builds(RoiConfig, mode=st.sampled_from(["static", "follow"]), context=st.sampled_from([0.0, 0.25, 0.5, 1.0]),
                 pad_min=st.sampled_from([0, 8, 32]), min_side=st.sampled_from([1, 32, 256, 512]), smooth=st.sampled_from([0, 1, 8]),
                 max_regions=st.sampled_from([1, 2, 3, 8]))
feathers = st.sampled_from([-1.0, 0.0, 3.0, 8.5])


def _whole(b):
    """Per-frame bbox of the union of all boxes (what hip.mask_bbox gives for the whole mask)."""
    out = np.zeros((b.shape[0], 4), np.int64)
    for t in range(b.shape[0]):
        bs = [x for x in b[t] if not _empty(x)]
        if bs:
            bs = np.array(bs)
            out[t] = (bs[:, 0].min(), bs[:, 1].min(), bs[:, 2].max(), bs[:, 3].max())
    return out


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return len(a) == len(b) and all(p.mode == q.mode and p.size == q.size and np.array_equal(p.offsets, q.offsets) and np.array_equal(p.centers, q.centers)
                                    for p, q in zip(a, b))


def _check_plan_contract(p, T, H0, W0, cfg):
    h, w = p.size
    assert (h % 8 == 0 or h == H0) and (w % 8 == 0 or w == W0) and (h, w) != (H0, W0)
    assert h >= min(cfg.min_side, H0) and w >= min(cfg.min_side, W0)
    assert p.mode == cfg.mode and p.offsets.shape == (T, 2) and p.offsets.dtype == np.int32
    assert (p.offsets[:, 0] >= 0).all() and (p.offsets[:, 0] <= H0 - h).all() and (p.offsets[:, 1] >= 0).all() and (p.offsets[:, 1] <= W0 - w).all()
    if cfg.mode == "static":
        assert (p.offsets == p.offsets[0]).all()


@settings(max_examples=300, deadline=None)
@given(region_tracks(), cfgs, feathers, st.integers(0, 2 ** 31))
def test_plan_regions_properties(track, cfg, feather, seed):
    b, H0, W0 = track
    T, K = b.shape[:2]
    R = max(0, math.ceil(feather))
    plans = plan_regions(b, H0, W0, feather, cfg)
    whole = plan_roi(_whole(b), H0, W0, feather, cfg)
    if plans is None or len(plans) == 1 or cfg.max_regions == 1 or K == 1:
        assert _same(plans, None if whole is None else [whole])      # one region left: plan_roi on the whole mask
    if plans is None:
        return
    assert 1 <= len(plans) <= cfg.max_regions
    for p in plans:
        _check_plan_contract(p, T, H0, W0, cfg)
    wins = [np.concatenate([p.offsets, p.offsets + np.array(p.size)], 1) for p in plans]
    for i in range(len(plans)):                                   # pairwise disjoint in every frame
        for j in range(i + 1, len(plans)):
            a, c = wins[i], wins[j]
            meet = (np.maximum(a[:, 0], c[:, 0]) < np.minimum(a[:, 2], c[:, 2])) & (np.maximum(a[:, 1], c[:, 1]) < np.minimum(a[:, 3], c[:, 3]))
            assert not meet.any()
    for k in range(K):                                            # each box track lies, with its feather radius, in ONE window in every frame
        homes = []
        for i, wi in enumerate(wins):
            ok = True
            for t in range(T):
                if _empty(b[t, k]):
                    continue
                y0, x0, y1, x1 = b[t, k]
                oy, ox, ey, ex = wi[t]
                ok &= oy <= max(0, y0 - R) and min(H0, y1 + R) <= ey and ox <= max(0, x0 - R) and min(W0, x1 + R) <= ex
            homes.append(ok)
        assert all(_empty(x) for x in b[:, k]) or any(homes)
    perm = np.random.default_rng(seed).permutation(K)              # the numbering of the components does not matter
    assert _same(plan_regions(b[:, perm], H0, W0, feather, cfg), plans)


def test_two_logos_in_opposite_corners_get_two_windows():
    """1920 x 1080, default settings: 160 x 90 logos top right (as bench_roi.py's clip b) and bottom left."""
    T = 6
    b = np.array([[[40, 1700, 130, 1860], [950, 60, 1040, 220]]] * T)
    for mode in ("static", "follow"):
        cfg = as_config(f"{mode}-regions")
        assert plan_roi(_whole(b), 1080, 1920, 3, RoiConfig(mode)) is None           # the union window is the whole frame
        plans = plan_regions(b, 1080, 1920, 3, cfg)
        assert len(plans) == 2 and all(p.size == (512, 512) for p in plans)
        assert plans[0].offsets[0].tolist() == [0, 1408] and plans[1].offsets[0].tolist() == [568, 0]   # sorted by (y0, x0)


def test_nearby_logos_get_one_window():
    b = np.array([[[40, 1400, 130, 1560], [40, 1660, 130, 1820]]] * 4)              # 100 px apart
    plans = plan_regions(b, 1080, 1920, 3, as_config("static-regions"))
    assert _same(plans, [plan_roi(_whole(b), 1080, 1920, 3, RoiConfig("static"))])
    assert len(plans) == 1 and plans[0].size == (512, 840)                          # the two 512 x 512 windows would overlap


def test_plan_regions_empty_and_max_regions():
    cfg = RoiConfig("follow", context=0.0, min_side=32, pad_min=8, max_regions=8)
    assert plan_regions(np.zeros((3, 2, 4), int), 720, 1280, 3, cfg) is None
    assert plan_regions(np.zeros((0, 2, 4), int), 720, 1280, 3, cfg) is None
    b = np.array([[[100 * i, 100 * j, 100 * i + 10, 100 * j + 10] for i in range(3) for j in range(3)]] * 2)   # nine small separate boxes
    assert len(plan_regions(b, 720, 1280, 3, cfg)) == 8
    assert len(plan_regions(b, 720, 1280, 3, RoiConfig("follow", context=0.0, min_side=32, pad_min=8, max_regions=3))) <= 3
    assert len(plan_regions(b, 720, 1280, 3, RoiConfig("follow", min_side=32, pad_min=8, max_regions=8))) == 1     # merged windows grow into the rest


# ---- settings -------------------------------------------------------------------------------------------------------------------------
def test_region_spellings():
    assert roi.MODES == ("static", "follow")
    assert as_config("static-regions") == RoiConfig("static", max_regions=8)
    assert as_config(" Follow-Regions ") == RoiConfig("follow", max_regions=8)
    assert as_config("static") == RoiConfig("static") and RoiConfig("static").max_regions == 1
    for bad in ("everywhere", "sideways", "full", "regions", "static-region", 3, True):
        with pytest.raises(ValueError):
            as_config(bad)
    for bad in ("everywhere", "static-regions"):
        with pytest.raises(ValueError):
            RoiConfig(bad)
    with pytest.raises(ValueError):
        RoiConfig("static", max_regions=0)


def test_region_spellings_through_configure_and_environment(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_ROI", raising=False)
    try:
        monkeypatch.setenv("VV_ROI", "follow-regions")
        assert diffuerase.roi_config() == RoiConfig("follow", max_regions=8)
        diffuerase.configure(roi="static-regions")
        assert diffuerase.roi_config() == RoiConfig("static", max_regions=8)
        assert diffuerase.roi_config("follow-regions") == RoiConfig("follow", max_regions=8)
        assert diffuerase.roi_config("static") == RoiConfig("static")
        with pytest.raises(ValueError):
            diffuerase.configure(roi="sideways-regions")
    finally:
        diffuerase.configure()


def test_cli_accepts_region_spellings(monkeypatch, tmp_path):
    import diffuerase
    runs = []
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda p, s=0, n=-1: ([np.zeros((16, 24, 3), np.uint8)] * 2, 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    monkeypatch.setattr(diffuerase, "run_infill_on_frames", lambda fr, mk, **kw: (runs.append(kw), list(fr))[1])
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    base = ["diffuerase.py", "--color_video", str(color), "--mask_video", "m.mkv"]
    for r in ("static-regions", "follow-regions", "static"):
        monkeypatch.setattr(sys, "argv", base + ["--roi", r])
        diffuerase.main()
    assert [kw["roi"] for kw in runs] == ["static-regions", "follow-regions", "static"]
    for bad in ("everywhere", "full"):
        monkeypatch.setattr(sys, "argv", base + ["--roi", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()


# ---- orchestration ------------------------------------------------------------------------------------------------------------------
def _fake_clip(T=5, H=16, W=24):
    """Frames, masks and a prior whose every pixel tells frame and position, so a crop at a wrong offset or of a wrong frame differs."""
    y, x = np.mgrid[:H, :W]
    frames = [((7 * t + 3 * y + x)[..., None] + np.arange(3)).astype(np.uint8) for t in range(T)]
    for t, f in enumerate(frames):
        f[0, 0, 0] = t
    dil = [(100 + 5 * t + y + 2 * x).astype(np.uint8) for t in range(T)]
    prior = [255 - f for f in frames]
    return frames, dil, prior


def _fake_stages(log, prior_vals, model_vals):
    """An infill.Stages that records every call with its arguments and reports prior_vals / model_vals as progress (every other message empty)."""
    from videovanish_amd import infill

    def run(kind, vals, add):
        def stage(f, m, *rest):
            log.append((kind, f, m) + rest)
            if rest[-1] is not None:
                for i, v in enumerate(vals):
                    rest[-1](v, f"{kind} {i}" if i % 2 == 0 else "")
            return [x + add for x in f]
        return stage
    return infill.Stages(lambda: log.append(("load_model",)), lambda: log.append(("load_prior",)), run("prior", prior_vals, 1), run("model", model_vals, 2))


def _same_frames(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


@pytest.mark.parametrize("with_prior", [True, False])
def test_run_windows_full_frame_and_one_window(with_prior):
    from videovanish_amd import infill
    frames, dil, prior = _fake_clip()
    T = len(frames)
    plan = roi.RoiPlan("follow", (8, 16), np.array([[2 + t, 3 + t] for t in range(T)], np.int32), np.zeros((T, 2)))
    for plans in ([], [plan]):
        log, progs = [], []
        prog = lambda v, s: progs.append((v, s))
        outs = infill.run_windows(frames, dil, prior if with_prior else None, plans, _fake_stages(log, (25, 35), (60, 75)), prog)
        assert [c[0] for c in log] == (["load_model", "model"] if with_prior else ["load_model", "load_prior", "prior", "model"])
        calls = [c for c in log if len(c) > 1]
        model = calls[-1]
        if plans:                                                       # one window: the crops the plan makes
            for c in calls:
                assert _same_frames(c[1], plan.crop(frames)) and _same_frames(c[2], plan.crop(dil))
            if with_prior:
                assert _same_frames(model[3], plan.crop(prior))
        else:                                                           # the full frame: the very same list objects, no copy
            for c in calls:
                assert c[1] is frames and c[2] is dil
            if with_prior:
                assert model[3] is prior
        if not with_prior:                                              # the prior stage's result goes to the model as it is
            assert calls[0][0] == "prior" and _same_frames(model[3], [x + 1 for x in calls[0][1]]) and model[1] is calls[0][1] and model[2] is calls[0][2]
        assert all(c[-1] is prog for c in calls)                        # the caller's progress itself: no prefix, no remapping
        assert len(outs) == 1 and _same_frames(outs[0], [x + 2 for x in model[1]])
        want = [(10, "loading weights")] + ([] if with_prior else [(20, "running propainter prior"), (25, "prior 0"), (35, "")])
        assert progs == want + [(50, "running DiffuEraser"), (60, "model 0"), (75, ""), (90, "resizing and merging finished frames")]
        outs = infill.run_windows(frames, dil, prior if with_prior else None, plans, _fake_stages([], (25,), (60,)), None)      # no callback: nothing is called
        assert len(outs) == 1 and len(outs[0]) == T


@pytest.mark.parametrize("with_prior", [True, False])
def test_run_windows_two_windows(with_prior):
    from videovanish_amd import infill
    frames, dil, prior = _fake_clip()
    T = len(frames)
    plans = [roi.RoiPlan("static", (8, 8), np.tile(np.array([[0, 16]], np.int32), (T, 1)), np.zeros((T, 2))),
             roi.RoiPlan("follow", (8, 16), np.array([[8, t] for t in range(T)], np.int32), np.zeros((T, 2)))]
    log, progs = [], []
    # the sub-calls report their own end points too (20 / 50, 50 / 90): these must not land on a milestone
    outs = infill.run_windows(frames, dil, prior if with_prior else None, plans, _fake_stages(log, (20, 30, 40, 50), (50, 60, 80, 90)),
                              lambda v, s: progs.append((v, s)))
    kinds = [c[0] for c in log]
    assert kinds == (["load_model"] if with_prior else ["load_model", "load_prior", "prior", "prior"]) + ["model", "model"]    # every prior before any model
    for kind in ("model",) if with_prior else ("prior", "model"):
        for p, c in zip(plans, [c for c in log if c[0] == kind]):
            assert c[1][0].shape == p.size + (3,) and _same_frames(c[1], p.crop(frames)) and _same_frames(c[2], p.crop(dil))
            if kind == "model":
                assert _same_frames(c[3], p.crop(prior) if with_prior else [x + 1 for x in p.crop(frames)])
    assert len(outs) == 2 and all(_same_frames(o, [x + 2 for x in p.crop(frames)]) for o, p in zip(outs, plans))
    vals = [v for v, _ in progs]
    assert [v for v in vals if v in (5, 10, 20, 50, 90)] == ([10, 50, 90] if with_prior else [10, 20, 50, 90])      # each once; 5 is run_infill_on_frames'
    assert vals == sorted(vals) and all(isinstance(s, str) and s for _, s in progs)
    assert progs[0] == (10, "loading weights") and vals[-1] == 90 and (with_prior or vals[1] == 20)
    for a, b, kind in ((50, 90, "model"),) if with_prior else ((20, 50, "prior"), (50, 90, "model")):
        got = progs[vals.index(a) + 1:vals.index(b)]
        assert len(got) == 8 and all(a < v < b for v, _ in got)                               # four per region, strictly inside
        for k in (0, 1):                                                                      # the prefix, also where the sub-call's message is empty
            assert [s for _, s in got[4 * k:4 * k + 4]] == [f"region {k + 1}/2: {kind} 0", f"region {k + 1}/2", f"region {k + 1}/2: {kind} 2", f"region {k + 1}/2"]
    # no progress callback: nothing is called
    outs = infill.run_windows(frames, dil, None, plans, _fake_stages([], (30,), (60,)), None)
    assert len(outs) == 2 and _same_frames(outs[1], [x + 2 for x in plans[1].crop(frames)])


# ---- entry points -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(LIB)


def test_region_entry_points_reject_bad_arguments_without_gpu(lib):
    """Every case is invalid in one argument: the launchers return VV_E_ARG (-1) before touching the device."""
    lib.vv_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    tu = dict(mask2d=a, T=2, H=8, W=8, tile=16, occ=a)
    for k, v in (("mask2d", None), ("occ", None), ("T", 0), ("T", 65536), ("T", -1), ("tile", 0), ("tile", -16), ("H", 0), ("W", 0), ("W", -3)):
        args = dict(tu, **{k: v})
        rc = lib.vv_mask_tile_union(ctypes.c_void_p(args["mask2d"]), args["T"], args["H"], args["W"], args["tile"], ctypes.c_void_p(args["occ"]), None)
        assert rc == -1 and b"vv_mask_tile_union" in lib.vv_last_error(), (k, v)
    bt = dict(mask2d=a, T=2, H=8, W=8, tile=16, tiles=a, n=1, K=1, bbox=a)
    for k, v in (("mask2d", None), ("tiles", None), ("bbox", None), ("T", 0), ("T", 65536), ("tile", 0), ("H", 0), ("W", 0), ("n", -1), ("K", 0),
                 ("K", -2)):
        args = dict(bt, **{k: v})
        rc = lib.vv_mask_bbox_tiles(ctypes.c_void_p(args["mask2d"]), args["T"], args["H"], args["W"], args["tile"], ctypes.c_void_p(args["tiles"]),
                                    args["n"], args["K"], ctypes.c_void_p(args["bbox"]), None)
        assert rc == -1 and b"vv_mask_bbox_tiles" in lib.vv_last_error(), (k, v)
