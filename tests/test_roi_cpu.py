"""Mask-region inference, host side: the window planner (videovanish_amd/roi.py) as properties over random box tracks, and the drop-in's
settings (roi=, configure(roi=), $VV_ROI, --roi).  No GPU: the planner is pure numpy and the drop-in checks run before any device work."""
import ast
import math
import os
import sys
import types

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from videovanish_amd.roi import RoiConfig, as_config, plan_roi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _empty(b):
    return b[2] <= b[0] or b[3] <= b[1]


@st.composite
def tracks(draw):
    """(bboxes [T,4], H0, W0): a box drifting across the frame with random size jitter and gaps (empty frames)."""
    H0 = draw(st.integers(16, 1100))
    W0 = draw(st.integers(16, 2000))
    T = draw(st.integers(1, 40))
    bh = draw(st.integers(1, H0))
    bw = draw(st.integers(1, W0))
    y = draw(st.integers(0, H0 - bh))
    x = draw(st.integers(0, W0 - bw))
    vy = draw(st.integers(-12, 12))
    vx = draw(st.integers(-12, 12))
    gap_p = draw(st.sampled_from([0.0, 0.2, 0.6]))
    rng = np.random.default_rng(draw(st.integers(0, 2 ** 31)))
    out = np.zeros((T, 4), np.int64)
    for t in range(T):
        h = int(np.clip(bh + rng.integers(-3, 4), 1, H0))
        w = int(np.clip(bw + rng.integers(-3, 4), 1, W0))
        y0 = int(np.clip(y + vy * t + rng.integers(-2, 3), 0, H0 - h))
        x0 = int(np.clip(x + vx * t + rng.integers(-2, 3), 0, W0 - w))
        if rng.random() >= gap_p:
            out[t] = (y0, x0, y0 + h, x0 + w)
    return out, H0, W0


cfgs = st.builds(RoiConfig, mode=st.sampled_from(["static", "follow"]), context=st.sampled_from([0.0, 0.25, 0.5, 1.0]),
                 pad_min=st.sampled_from([0, 8, 32]), min_side=st.sampled_from([1, 32, 256, 512]), smooth=st.sampled_from([0, 1, 8]))
feathers = st.sampled_from([-1.0, 0.0, 3.0, 8.5])


def _expected_size(b, H0, W0, R, cfg):
    has = [k for k in range(len(b)) if not _empty(b[k])]
    if cfg.mode == "static":
        bh = max(b[k][2] for k in has) - min(b[k][0] for k in has)
        bw = max(b[k][3] for k in has) - min(b[k][1] for k in has)
    else:
        bh = max(b[k][2] - b[k][0] for k in has)
        bw = max(b[k][3] - b[k][1] for k in has)
    pad = max(cfg.pad_min, R + 2, math.ceil(cfg.context * max(bh, bw)))

    def side(e, F):
        s = max(e + 2 * pad, min(cfg.min_side, F))
        return min(F, (s + 7) // 8 * 8)
    return (side(bh, H0), side(bw, W0)), pad


@settings(max_examples=300, deadline=None)
@given(tracks(), cfgs, feathers)
def test_plan_properties(track, cfg, feather):
    b, H0, W0 = track
    R = max(0, math.ceil(feather))
    plan = plan_roi(b, H0, W0, feather, cfg)
    if all(_empty(x) for x in b):
        assert plan is None
        return
    (eh, ew), pad = _expected_size(b, H0, W0, R, cfg)
    if (eh, ew) == (H0, W0):
        assert plan is None                                  # the window would be the whole frame: today's path
        return
    assert plan is not None and plan.size == (eh, ew)
    h, w = plan.size
    assert (h % 8 == 0 or h == H0) and (w % 8 == 0 or w == W0)
    assert h >= min(cfg.min_side, H0) and w >= min(cfg.min_side, W0)
    assert plan.offsets.shape == (len(b), 2) and plan.offsets.dtype == np.int32
    for k, (oy, ox) in enumerate(plan.offsets.tolist()):
        assert 0 <= oy <= H0 - h and 0 <= ox <= W0 - w        # inside the frame
        if _empty(b[k]):
            continue
        y0, x0, y1, x1 = b[k]                                # the mask and its feather neighbourhood inside the window
        assert oy <= max(0, y0 - R) and min(H0, y1 + R) <= oy + h
        assert ox <= max(0, x0 - R) and min(W0, x1 + R) <= ox + w
    if cfg.mode == "static":
        assert (plan.offsets == plan.offsets[0]).all()
        has = ~np.array([_empty(x) for x in b])
        uy0, ux0, uy1, ux1 = b[has, 0].min(), b[has, 1].min(), b[has, 2].max(), b[has, 3].max()
        oy, ox = plan.offsets[0].tolist()
        # the padded union, shifted into the frame
        assert oy <= max(0, uy0 - pad) and min(H0, uy1 + pad) <= oy + h
        assert ox <= max(0, ux0 - pad) and min(W0, ux1 + pad) <= ox + w
        assert oy == min(max(uy0 - (h - (uy1 - uy0)) // 2, 0), H0 - h) and ox == min(max(ux0 - (w - (ux1 - ux0)) // 2, 0), W0 - w)


@settings(max_examples=200, deadline=None)
@given(tracks(), st.sampled_from([0, 1, 3, 8]), feathers)
def test_follow_centres_are_smoothed(track, smooth, feather):
    """The window centres are the box-centre track (gaps interpolated, ends held) smoothed: they never move faster than that track, and a window
    sits at its centre unless the frame border or its own box forces a shift."""
    b, H0, W0 = track
    cfg = RoiConfig("follow", pad_min=8, min_side=32, smooth=smooth)
    plan = plan_roi(b, H0, W0, feather, cfg)
    if plan is None:
        return
    has = np.array([not _empty(x) for x in b])
    idx = np.nonzero(has)[0]
    t = np.arange(len(b))
    raw = np.stack([np.interp(t, idx, (b[idx, 0] + b[idx, 2]) / 2.0), np.interp(t, idx, (b[idx, 1] + b[idx, 3]) / 2.0)], 1)
    if smooth == 0:
        assert np.allclose(plan.centers, raw)
    if len(b) > 1:
        assert (np.abs(np.diff(plan.centers, axis=0)) <= np.abs(np.diff(raw, axis=0)).max(axis=0) + 1e-9).all()
    h, w = plan.size
    R = max(0, math.ceil(feather))
    for k in range(len(b)):
        for a, (s, F) in enumerate(((h, H0), (w, W0))):
            want = int(math.floor(plan.centers[k, a] - s / 2.0 + 0.5))
            got = int(plan.offsets[k, a])
            if got != want:                        # a shift happened: the unshifted window left the frame or cut the box + guard
                lo, hi = (b[k, a], b[k, a + 2]) if has[k] else (0, 0)
                bad = want < 0 or want > F - s or (has[k] and (want > max(0, lo - R - 1) or want + s < min(F, hi + R + 1)))
                assert bad


def test_plan_fallbacks_and_examples():
    cfg = RoiConfig("follow")
    assert plan_roi(np.zeros((5, 4), int), 720, 1280, 3, cfg) is None                    # no mask pixel anywhere
    assert plan_roi(np.array([[0, 0, 720, 1280]]), 720, 1280, 3, cfg) is None             # the window is the whole frame
    # bench.py's synthetic clip at 1280 x 720: a 180 x 320 box moving 2 px per frame
    b = np.array([[240, 160 + 2 * t, 420, 480 + 2 * t] for t in range(32)])
    p = plan_roi(b, 720, 1280, 3, cfg)
    assert p.size == (512, 640) and p.mode == "follow"
    b8 = b + np.array([-8, -8, 8, 8])                                                      # dilated by 8
    p = plan_roi(b8, 720, 1280, 3, cfg)
    assert p.size == (536, 672)
    # a 160 x 90 logo at 1920 x 1080, static: min_side decides
    p = plan_roi(np.array([[40, 1700, 130, 1860]] * 4), 1080, 1920, 3, RoiConfig("static"))
    assert p.size == (512, 512) and p.offsets[0].tolist() == [0, 1408]


def test_roi_config_parsing():
    assert as_config(None) is None and as_config(False) is None and as_config("off") is None and as_config("") is None
    assert as_config("static") == RoiConfig("static") and as_config(" Follow ") == RoiConfig("follow")
    c = RoiConfig("follow", smooth=2)
    assert as_config(c) is c
    for bad in ("full", 3, True):
        with pytest.raises(ValueError):
            as_config(bad)
    with pytest.raises(ValueError):
        RoiConfig("everywhere")


def test_roi_precedence(monkeypatch):
    """Explicit roi= wins, then configure(roi=...), then $VV_ROI; configure() without roi resets."""
    import diffuerase
    monkeypatch.delenv("VV_ROI", raising=False)
    try:
        assert diffuerase.roi_config() is None
        monkeypatch.setenv("VV_ROI", "static")
        assert diffuerase.roi_config() == RoiConfig("static")
        diffuerase.configure(roi="follow")
        assert diffuerase.roi_config() == RoiConfig("follow")
        assert diffuerase.roi_config("static") == RoiConfig("static")
        assert diffuerase.roi_config("off") is None
        diffuerase.configure(roi="off")
        assert diffuerase.roi_config() is None                     # an explicit "off" is not overridden by the environment
        diffuerase.configure()
        assert diffuerase.roi_config() == RoiConfig("static")      # reset: the environment again
        monkeypatch.setenv("VV_ROI", "sideways")
        with pytest.raises(ValueError):
            diffuerase.roi_config()
        with pytest.raises(ValueError):
            diffuerase.configure(roi="sideways")
    finally:
        diffuerase.configure()


def test_roi_with_compat_early_return_raises(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_ROI", raising=False)
    fr = [np.zeros((16, 16, 3), np.uint8)]
    with pytest.raises(ValueError, match="compat_reference_early_return"):
        diffuerase.run_infill_on_frames(fr, fr, roi="static", compat_reference_early_return=True)
    try:
        diffuerase.configure(roi=RoiConfig("follow"))
        with pytest.raises(ValueError, match="compat_reference_early_return"):
            diffuerase.run_infill_on_frames(fr, fr, compat_reference_early_return=True)
    finally:
        diffuerase.configure()


def test_cli_forwards_roi_only_when_given(monkeypatch, tmp_path):
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
    monkeypatch.setattr(sys, "argv", base)
    diffuerase.main()
    monkeypatch.setattr(sys, "argv", base + ["--roi", "follow"])
    diffuerase.main()
    assert runs == [{"propainer_frames": None}, {"propainer_frames": None, "roi": "follow"}]
    monkeypatch.setattr(sys, "argv", base + ["--roi", "everywhere"])
    with pytest.raises(SystemExit):
        diffuerase.main()


def test_product_imports_nothing_from_oracle():
    files = [os.path.join(ROOT, "diffuerase.py")]
    pkg = os.path.join(ROOT, "videovanish_amd")
    files += [os.path.join(pkg, f) for f in sorted(os.listdir(pkg)) if f.endswith(".py")]
    assert os.path.join(pkg, "roi.py") in files
    for f in files:
        tree = ast.parse(open(f).read(), f)
        for node in ast.walk(tree):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""]
            assert not any(n == "oracle" or n.startswith("oracle.") for n in names), f"{f} imports {names}"
