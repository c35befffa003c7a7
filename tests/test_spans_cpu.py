"""Mask-span inference on the CPU: the planner's guarantees over seeded random inputs, the cut detector on synthetic clip families (numpy
restatement of the device statistics: tests/spans_ref.py), the drop-in's orchestration with a fake per-clip body, configuration, CLI and the
binding of include/vvspans.h."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abiref  # noqa: E402
import spans_ref as R  # noqa: E402

from videovanish_amd import spans as S  # noqa: E402
from videovanish_amd.spans import SpanConfig, find_cuts, plan_spans  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- planner ----------------------------------------------------------------------------------------------------------------------------
def _draw(rng, k):
    """One (masked, cuts, cfg): the kinds cycle through empty, full, single-frame, a few runs and salt masks; cuts fall anywhere (also inside masked
    runs, also next to each other so that segments are shorter than min_len)."""
    T = int(rng.integers(1, 90))
    kind = k % 6
    masked = np.zeros(T, bool)
    if kind == 1:
        masked[:] = True
    elif kind == 2:
        masked[rng.integers(0, T)] = True
    elif kind == 3:
        for _ in range(int(rng.integers(1, 4))):
            a = int(rng.integers(0, T))
            masked[a:a + int(rng.integers(1, 20))] = True
    elif kind >= 4:
        masked = rng.random(T) < (0.1 if kind == 4 else 0.5)
    ncut = int(rng.integers(0, 6))
    cuts = sorted({int(c) for c in rng.integers(1, max(T, 2), ncut)} - {T}) if T > 1 else []
    if kind == 3 and T > 2 and masked.any() and rng.random() < 0.7:           # a cut inside a masked run
        cuts = sorted(set(cuts) | {int(np.nonzero(masked)[0][len(np.nonzero(masked)[0]) // 2])} - {0})
    cfg = SpanConfig(mode="masked" if k % 3 else "all", context=int(rng.integers(0, 10)), min_len=int(rng.integers(1, 20)), min_gap=int(rng.integers(0, 10)))
    return masked, cuts, cfg


def _check_guarantees(masked, cuts, cfg, spans):
    T = len(masked)
    segs = S.segments(T, cuts)
    seg_of = lambda t: next((s, e) for s, e in segs if s <= t < e)
    assert spans == sorted(spans) and all(0 <= a < b <= T for a, b in spans)                         # sorted, non-empty, in range
    assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))                        # disjoint
    cover = np.zeros(T, int)
    for a, b in spans:
        cover[a:b] += 1
        assert not [c for c in cuts if a < c < b], (a, b, cuts)                                      # no cut in a span's interior
        s, e = seg_of(a)
        assert b <= e and b - a >= min(cfg.min_len, e - s)                                           # inside one segment, long enough for it
    assert (cover[masked] == 1).all()                                                                # every masked frame in exactly one span
    if cfg.mode == "all":
        assert spans == segs
        return
    assert not masked[cover == 0].any()                                                              # frames outside every span are unmasked
    for t in np.nonzero(masked)[0]:
        a, b = next((a, b) for a, b in spans if a <= t < b)
        s, e = seg_of(t)
        assert t - a >= min(cfg.context, t - s) and b - 1 - t >= min(cfg.context, e - 1 - t), (t, a, b, s, e)
    for (a0, b0), (a1, b1) in zip(spans, spans[1:]):
        if seg_of(a0) == seg_of(a1):
            assert a1 - b0 >= cfg.min_gap and a1 - b0 > 0, (spans, cfg)                              # no two spans of a segment closer than min_gap


def test_planner_guarantees_over_random_draws():
    rng = np.random.default_rng(20240611)
    seen = {"empty": 0, "full": 0, "single": 0, "short_seg": 0, "cut_in_run": 0, "several": 0}
    for k in range(900):
        masked, cuts, cfg = _draw(rng, k)
        spans = plan_spans(masked, cuts, cfg)
        _check_guarantees(masked, cuts, cfg, spans)
        assert plan_spans(masked.copy(), list(cuts), cfg) == spans                                    # nothing but the arguments decides
        seen["empty"] += not masked.any()
        seen["full"] += bool(masked.all())
        seen["single"] += masked.sum() == 1
        seen["short_seg"] += any(e - s < cfg.min_len for s, e in S.segments(len(masked), cuts))
        seen["cut_in_run"] += any(0 < c < len(masked) and masked[c - 1] and masked[c] for c in cuts)
        seen["several"] += cfg.mode == "masked" and len(spans) > 1
    assert all(v >= 30 for v in seen.values()), seen


def test_planner_hand_written_cases():
    full = np.ones(40, bool)
    assert plan_spans(full, None, SpanConfig("masked")) == [(0, 40)]
    assert plan_spans(full, [], SpanConfig("all")) == [(0, 40)]
    assert plan_spans(np.zeros(40, bool), None, SpanConfig("masked")) == []
    assert plan_spans(np.zeros(40, bool), [10, 25], SpanConfig("masked")) == []
    assert plan_spans(np.zeros(40, bool), [10, 25], SpanConfig("all")) == [(0, 10), (10, 25), (25, 40)]
    assert plan_spans(np.zeros(40, bool), None, SpanConfig("all", cuts=[25, 10])) == [(0, 10), (10, 25), (25, 40)]      # the config's own cuts
    assert plan_spans(np.zeros(40, bool), [0, 40, 99, -3], SpanConfig("all")) == [(0, 40)]                           # cuts that separate nothing
    m = np.zeros(100, bool)
    m[40:44] = True
    assert plan_spans(m, None, SpanConfig("masked")) == [(32, 52)]                                    # 4 + 2 * 8 = 20 >= 16
    assert plan_spans(m, None, SpanConfig("masked", context=2)) == [(34, 50)]                         # 8 frames raised to 16, left first, alternately
    assert plan_spans(m, [42], SpanConfig("masked")) == [(26, 42), (42, 58)]                          # a cut inside the run: two spans, each raised to 16
    assert plan_spans(m, [38, 46], SpanConfig("masked")) == [(38, 46)]                                # a segment shorter than min_len: the whole segment
    m[60:62] = True                                                                                   # second run: 52 .. 70, gap 0 -> one span
    assert plan_spans(m, None, SpanConfig("masked")) == [(32, 70)]
    m2 = np.zeros(100, bool)
    m2[[10, 50]] = True
    assert plan_spans(m2, None, SpanConfig("masked")) == [(2, 19), (42, 59)]
    assert plan_spans(m2, None, SpanConfig("masked", min_gap=24)) == [(2, 59)]                        # a 23-frame gap is run rather than split
    assert plan_spans(m2, None, SpanConfig("masked", context=1, min_len=3, min_gap=2)) == [(9, 12), (49, 52)]
    first = plan_spans(m2, [30], SpanConfig("masked"))
    assert all(plan_spans(m2, [30], SpanConfig("masked")) == first for _ in range(3))


# ---- detector ---------------------------------------------------------------------------------------------------------------------------
def _families():
    """name -> (frames, masks | None, true cuts): two and three shots under pans of 2 .. 12 px per frame, a dissolve, a flash, the moving masked
    box over a cut, white noise."""
    out = {}
    for seed in range(4):
        for v in (2, 6, 12):
            out[f"two shots, pan {v}, seed {seed}"] = (*R.shots_clip(100 + seed * 10 + v, (12, 12), (v, v)), None)
        out[f"three shots, seed {seed}"] = (*R.shots_clip(200 + seed, (10, 9, 11), (2, 12, 6)), None)
        out[f"pan only, seed {seed}"] = (*R.shots_clip(250 + seed, (20,), (2 + 5 * (seed % 3),)), None)
        out[f"dissolve, seed {seed}"] = (*R.dissolve_clip(300 + seed), None)
        out[f"flash, seed {seed}"] = (*R.flash_clip(400 + seed), None)
        out[f"noise, seed {seed}"] = (*R.noise_clip(500 + seed), None)
        frames, cuts = R.shots_clip(600 + seed, (12, 12), (6, 6))
        masks = R.moving_box(24)
        out[f"masked box, seed {seed}"] = (R.paint(frames, masks, seed), cuts, masks)
    return {k: (f, m, c) for k, (f, c, m) in out.items()}


@pytest.fixture(scope="module")
def family_stats():
    return {name: (R.pair_stats(np.stack(frames), masks), cuts, len(frames)) for name, (frames, masks, cuts) in _families().items()}


def test_cut_peaks_stand_clear_of_everything_else(family_stats):
    """On the statistics alone: the smallest histogram peak ratio at a true cut is at least twice the largest at any other pair of these clips, so a
    default between them does not sit on a knife edge.  (The ratio of m does not separate: under fast pan a cut is not even the largest m of its
    neighbourhood, which is why cut_m_ratio's default is below 1 and m carries a floor instead.)"""
    cfg = SpanConfig()
    at_cut, elsewhere, h_cut, m_cut, rm_cut = [], [], [], [], []
    for name, ((sad, n, hist), cuts, T) in family_stats.items():
        m, h = S.cut_statistics(sad, n, hist)
        rh, rm = S.peak_ratios(h, cfg.cut_window), S.peak_ratios(m, cfg.cut_window)
        for p in range(T - 1):
            (at_cut if p + 1 in cuts else elsewhere).append(rh[p])
            if p + 1 in cuts:
                h_cut.append(h[p]); m_cut.append(m[p]); rm_cut.append(rm[p])
    print("h peak ratio: min at cuts", min(at_cut), "max elsewhere", max(elsewhere), "| at cuts: min h", min(h_cut), "min m", min(m_cut), "min m ratio", min(rm_cut))
    assert len(at_cut) >= 20 and min(at_cut) >= 2 * max(elsewhere)
    assert max(elsewhere) < cfg.cut_h_ratio < min(at_cut)
    assert min(h_cut) >= 1.5 * cfg.cut_h_min and min(m_cut) >= 1.5 * cfg.cut_m_min and min(rm_cut) >= 1.5 * cfg.cut_m_ratio


def test_find_cuts_gives_exactly_the_true_cuts(family_stats):
    for name, ((sad, n, hist), cuts, T) in family_stats.items():
        assert find_cuts(sad, n, hist, SpanConfig(), npix=R.H * R.W) == cuts, name
    assert sum(bool(c) for _, c, _ in family_stats.values()) >= 20 and sum(not c for _, c, _ in family_stats.values()) >= 16


def test_find_cuts_special_cases():
    frames, cuts = R.shots_clip(700, (12, 12), (4, 4))
    assert cuts == [12]
    stats = R.pair_stats(np.stack(frames))
    assert find_cuts(*stats, SpanConfig()) == [12]
    # the cut hidden behind a full-frame mask (n = 0), and behind a mask that leaves less than cut_min_cover of the frame: no decision
    hidden = np.zeros((24, R.H, R.W), np.uint8)
    hidden[11:13] = 255
    s = R.pair_stats(np.stack(frames), hidden)
    assert s[1][11] == 0 and find_cuts(*s, SpanConfig(), npix=R.H * R.W) == []
    most = np.zeros((24, R.H, R.W), np.uint8)
    most[:, :, : int(R.W * 0.8)] = 255
    assert find_cuts(*R.pair_stats(np.stack(frames), most), SpanConfig(), npix=R.H * R.W) == []
    assert find_cuts(*R.pair_stats(np.stack(frames), most), SpanConfig(cut_min_cover=0.1), npix=R.H * R.W) == [12]
    # cuts that would leave a segment shorter than cut_min_seg are dropped together: two shots with a 2-frame insert
    a = R.shots_clip(701, (10, 2, 10), (4, 4, 4))[0]
    st = R.pair_stats(np.stack(a))
    assert find_cuts(*st, SpanConfig(cut_window=1)) == []
    assert find_cuts(*st, SpanConfig(cut_window=1, cut_min_seg=2)) == [10, 12]
    # a cut next to the clip's end leaves a short segment too
    assert find_cuts(*R.pair_stats(np.stack(R.shots_clip(702, (12, 2), (4, 4))[0])), SpanConfig()) == []
    assert find_cuts([], [], np.zeros((0, 2, 64)), SpanConfig()) == []


# ---- orchestration ----------------------------------------------------------------------------------------------------------------------
def _fake(T=14):
    frames = [np.full((4, 6, 3), t, np.uint8) for t in range(T)]
    dil = np.stack([np.full((4, 6), 100 + t, np.uint8) for t in range(T)])
    prior = [np.full((4, 6, 3), 200 + t, np.uint8) for t in range(T)]
    return frames, dil, prior


def test_run_spans_slices_reassembles_and_reports():
    from videovanish_amd import infill
    frames, dil, prior = _fake()
    for with_prior in (True, False):
        calls, loads, progs = [], [], []

        def body(f, d, p, prog):
            calls.append(([int(x[0, 0, 0]) for x in f], [int(x[0, 0]) for x in d], None if p is None else [int(x[0, 0, 0]) for x in p]))
            prog(10, "loading weights")
            if p is None:
                prog(20, "running propainter prior")
                prog(35, "flow 1/2")
            prog(50, "running DiffuEraser")
            prog(70, "step 1/2")
            prog(90, "resizing and merging finished frames")
            return [x + 50 for x in f]

        out = infill.run_spans(frames, dil, prior if with_prior else None, [(1, 4), (8, 12)], body, lambda v, s: progs.append((v, s)),
                               load=lambda: loads.append(1))
        want_p = (lambda a, b: list(range(200 + a, 200 + b))) if with_prior else (lambda a, b: None)
        assert calls == [([1, 2, 3], [101, 102, 103], want_p(1, 4)), ([8, 9, 10, 11], [108, 109, 110, 111], want_p(8, 12))]      # slices, in order
        assert loads == [1]
        assert len(out) == 14
        for t in range(14):
            if 1 <= t < 4 or 8 <= t < 12:
                assert int(out[t][0, 0, 0]) == t + 50
            else:
                assert out[t] is frames[t]                                                            # untouched frames: the input arrays
        vals = [v for v, _ in progs]
        assert [v for v in vals if v in (5, 10, 20, 50, 90)] == ([10, 50, 90] if with_prior else [10, 20, 50, 90])      # 5 is the caller's (dilation)
        assert vals == sorted(vals) and all(isinstance(s, str) and s for _, s in progs)
        assert any(50 < v < 90 and s.startswith("span 1/2: ") for v, s in progs) and any(50 < v < 90 and s.startswith("span 2/2: ") for v, s in progs)
        if not with_prior:
            assert any(20 < v < 50 and s.startswith("span 1/2: ") for v, s in progs)
    # no progress callback: nothing is called
    out = infill.run_spans(frames, dil, None, [(0, 2)], lambda f, d, p, prog: [x + 1 for x in f] if prog is None else None, None)
    assert int(out[1][0, 0, 0]) == 2 and out[2] is frames[2]


def test_run_spans_special_paths():
    from videovanish_amd import infill
    frames, dil, prior = _fake()
    loads, progs = [], []
    prog = lambda v, s: progs.append((v, s))
    # one span that is the whole clip: the body on the clip as it is, with the caller's progress and no extra load
    got = {}

    def body(f, d, p, pr):
        got["args"] = (f, d, p, pr)
        return "whole"

    assert infill.run_spans(frames, dil, prior, [(0, 14)], body, prog, load=lambda: loads.append(1)) == "whole"
    assert got["args"][0] is frames and got["args"][1] is dil and got["args"][2] is prior and got["args"][3] is prog and not loads and not progs
    # an empty plan: the inputs, no body, no load, the milestones still delivered
    def never(*a):
        raise AssertionError("the body must not run")
    out = infill.run_spans(frames, dil, prior, [], never, prog, load=lambda: loads.append(1))
    assert len(out) == 14 and all(o is f for o, f in zip(out, frames)) and not loads
    assert [v for v, _ in progs] == [10, 20, 50, 90] and all(s for _, s in progs)
    assert infill.run_spans(frames, dil, None, [], never, None) == frames


# ---- configuration, CLI, binding ----------------------------------------------------------------------------------------------------------
def test_spellings_and_config():
    assert S.SPELLINGS == ("masked", "cuts", "masked-cuts")
    assert S.as_config("masked") == SpanConfig("masked") and S.as_config(" Masked ") == SpanConfig("masked")
    assert S.as_config("cuts") == SpanConfig("all", cuts="auto") and S.as_config("masked-cuts") == SpanConfig("masked", cuts="auto")
    for off in (None, False, "off", "none", "", "OFF"):
        assert S.as_config(off) is None
    cfg = SpanConfig("all", cuts=[30, 10, 10])
    assert cfg.cuts == (10, 30) and S.as_config(cfg) is cfg
    assert (SpanConfig().context, SpanConfig().min_len, SpanConfig().min_gap, SpanConfig().mode, SpanConfig().cuts) == (8, 16, 8, "masked", None)
    for bad in ("follow", 3, "auto"):
        with pytest.raises(ValueError):
            S.as_config(bad)
    for kw in (dict(mode="some"), dict(cuts="detect"), dict(cuts=[-1]), dict(context=-1), dict(min_len=0), dict(min_gap=-1), dict(cut_window=0)):
        with pytest.raises(ValueError):
            SpanConfig(**kw)
    assert S.parse_cuts("120,431") == (120, 431) and S.parse_cuts("7") == (7,)


def test_precedence_argument_configure_environment(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_SPANS", raising=False)
    try:
        diffuerase.configure()
        assert diffuerase.spans_config() is None
        monkeypatch.setenv("VV_SPANS", "masked-cuts")
        assert diffuerase.spans_config() == SpanConfig("masked", cuts="auto")
        diffuerase.configure(spans="cuts")
        assert diffuerase.spans_config() == SpanConfig("all", cuts="auto")
        assert diffuerase.spans_config("masked") == SpanConfig("masked")
        assert diffuerase.spans_config("off") is None and diffuerase.spans_config(False) is None          # the full clip whatever else is set
        diffuerase.configure(spans="off")
        assert diffuerase.spans_config() is None                                                         # configure("off") beats the environment
        diffuerase.configure()
        assert diffuerase.spans_config() == SpanConfig("masked", cuts="auto")                            # configure() resets
        # explicit cuts override the detector; alone they mean every frame, split there
        assert diffuerase.spans_config("masked-cuts", cuts=[9, 4]) == SpanConfig("masked", cuts=(4, 9))
        monkeypatch.delenv("VV_SPANS")
        assert diffuerase.spans_config(None, cuts=[5]) == SpanConfig("all", cuts=(5,))
        assert diffuerase.spans_config("off", cuts=[5]) is None
        with pytest.raises(ValueError):
            diffuerase.configure(spans="sometimes")
    finally:
        diffuerase.configure()


def test_spans_refuse_the_reference_early_return(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_SPANS", raising=False)
    f = [np.zeros((8, 8, 3), np.uint8)] * 2
    for kw in (dict(spans="masked"), dict(cuts=[1]), dict(spans=SpanConfig("all"))):
        with pytest.raises(ValueError, match="spans="):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, **kw)
    monkeypatch.setenv("VV_SPANS", "masked")
    with pytest.raises(ValueError, match="spans="):
        diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)


@pytest.fixture()
def cli(monkeypatch, tmp_path):
    """tests/test_cli_cpu.py's stub: frame I/O and the hot path replaced."""
    import diffuerase
    calls = []
    videos = {"mask.mkv": [np.zeros((16, 24, 3), np.uint8)] * 3}
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda path, start=0, max_frames=-1: ([f.copy() for f in videos[path]], 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    monkeypatch.setattr(diffuerase, "run_infill_on_frames", lambda frames, masks, **kw: calls.append(kw) or [f.copy() for f in frames])
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 3
    return diffuerase, calls, ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"], monkeypatch


def test_cli_spans_and_cuts_reach_the_call(cli):
    d, calls, argv, mp = cli
    mp.setattr(sys, "argv", argv)
    d.main()
    assert calls[-1] == {"propainer_frames": None}                                                       # a default call passes neither keyword
    for name in S.SPELLINGS:
        mp.setattr(sys, "argv", argv + ["--spans", name])
        d.main()
        assert calls[-1] == {"propainer_frames": None, "spans": name}
    mp.setattr(sys, "argv", argv + ["--spans", "masked", "--cuts", "120,431", "--roi", "follow"])
    d.main()
    assert calls[-1] == {"propainer_frames": None, "spans": "masked", "cuts": (120, 431), "roi": "follow"}
    mp.setattr(sys, "argv", argv + ["--cuts", "7"])
    d.main()
    assert calls[-1] == {"propainer_frames": None, "cuts": (7,)}
    mp.setattr(sys, "argv", argv + ["--spans", "off"])
    with pytest.raises(SystemExit):
        d.main()


def test_binding_matches_vvspans_header():
    """spans_hip.SIGNATURES declares every function of include/vvspans.h with the header's types, spans_hip.lib() has applied it, the versions agree
    (abiref.check_binding; test_abi_cpu.py: no name could be taken for another part's), and arguments are refused before anything touches a device."""
    from videovanish_amd import spans_hip
    loaded, define = abiref.check_binding(spans_hip, 3)
    assert define("VVS_HIST_BINS") == spans_hip.HIST_BINS == R.BINS
    # arguments are validated before anything touches a device
    assert loaded.vvs_frame_pair_stats(None, None, 4, 8, 8, None, None, None) == -1 and b"vvs_frame_pair_stats" in loaded.vvs_last_error()
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    assert loaded.vvs_frame_pair_stats(a, None, 1, 8, 8, a, a, None) == -1 and loaded.vvs_frame_pair_stats(a, None, 4, 0, 8, a, a, None) == -1
    with pytest.raises(ctypes.ArgumentError):
        loaded.vvs_frame_pair_stats(a, None, 4.0, 8, 8, a, a, None)
    import torch
    with pytest.raises(RuntimeError):
        spans_hip.pair_stats(torch.zeros((2, 4, 4, 3), dtype=torch.uint8))                                # no CPU fallback


def test_product_sources_of_the_feature():
    """vv_spans is in the one build recipe and reads no environment; the planner imports no torch."""
    abiref.check_sources("vv_spans", "vvspans.h", "spans")
