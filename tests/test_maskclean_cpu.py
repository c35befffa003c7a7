"""Mask clean-up on the CPU: the settings, the binding of include/vvmask.h, the properties of the reference restatement (tests/maskclean_ref.py)
over seeded draws, the planners on noisy masks with and without the clean-up, the orchestration with the device functions replaced by the
reference, configuration and CLI."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abiref  # noqa: E402
import maskclean_ref as R  # noqa: E402

from videovanish_amd import maskclean as M  # noqa: E402
from videovanish_amd import roi, spans  # noqa: E402
from videovanish_amd.maskclean import MaskCleanConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_spellings_and_config():
    assert M.SPELLINGS == ("on",)
    for off in (None, False, "off", "none", "", " OFF "):
        assert M.as_config(off) is None
    assert M.as_config("on") == M.as_config(" On ") == MaskCleanConfig() == MaskCleanConfig(None, 2, 0)
    assert M.as_config("area=64,bridge=2,grow=1") == MaskCleanConfig(64, 2, 1)
    assert M.as_config("grow=3") == MaskCleanConfig(None, 2, 3) and M.as_config(" bridge = 0 , area = 5 ") == MaskCleanConfig(5, 0, 0)
    cfg = MaskCleanConfig(min_area=4, bridge=1)
    assert M.as_config(cfg) is cfg
    for bad in ("yes", "static", "area", "area=", "area=x", "area=-3", "area=1.5", "area=3,area=4", "size=3", "area=3;grow=1", "bridge=17", "grow=9", "on,grow=1",
                "area=3,", 3, 1.0, ("on",)):
        with pytest.raises(ValueError):
            M.as_config(bad)
    for kw in (dict(bridge=-1), dict(bridge=17), dict(grow=-1), dict(grow=9), dict(min_area=-1), dict(min_area=2 ** 31), dict(bridge=1.0), dict(grow=True),
               dict(min_area="4")):
        with pytest.raises(ValueError):
            MaskCleanConfig(**kw)
    assert MaskCleanConfig(bridge=16, grow=8, min_area=0).area_for(1080, 1920) == 0
    # the default threshold: four cells of a 256 x 256 grid at the clip's size
    d = MaskCleanConfig()
    assert (d.area_for(1080, 1920), d.area_for(720, 1280), d.area_for(256, 256), d.area_for(96, 160), d.area_for(8, 8)) == (127, 57, 4, 1, 1)


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_vvmask_header():
    """mask_hip.SIGNATURES declares every function of include/vvmask.h with the header's types, mask_hip.lib() has applied it, the versions and
    limits agree (abiref.check_binding; test_abi_cpu.py: no name could be taken for another part's)."""
    from videovanish_amd import mask_hip
    loaded, define = abiref.check_binding(mask_hip, 5)
    assert define("VVM_ABI_VERSION") == 1
    assert (define("VVM_MAX_BRIDGE"), define("VVM_MAX_GROW"), define("VVM_MAX_T")) == (mask_hip.MAX_BRIDGE, mask_hip.MAX_GROW, mask_hip.MAX_T) == (16, 8, 65535)
    assert (M.MAX_BRIDGE, M.MAX_GROW) == (mask_hip.MAX_BRIDGE, mask_hip.MAX_GROW)
    # arguments are validated before anything touches a device
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    assert loaded.vvm_label_components(None, 1, 8, 8, None, None) == -1 and b"vvm_label_components" in loaded.vvm_last_error()
    assert loaded.vvm_label_components(a, 0, 8, 8, a, None) == -1 and loaded.vvm_label_components(a, 1, 1 << 16, 1 << 15, a, None) == -1
    assert loaded.vvm_despeckle(a, a, 1, 8, 8, 0, 4, a, a, a, a, None) == -1 and b"vvm_despeckle" in loaded.vvm_last_error()
    assert loaded.vvm_time_bridge_grow(a, 0, 8, 8, 1, 1, a, a, None) == -1 and loaded.vvm_time_bridge_grow(a, 4, 8, 8, -1, 0, a, a, None) == -1
    for args in ((4, 8, 8, 17, 0), (4, 8, 8, 0, 9), (65536, 8, 8, 0, 0)):
        assert loaded.vvm_time_bridge_grow(a, *args, a, a, None) == -2 and b"vvm_time_bridge_grow" in loaded.vvm_last_error()
    with pytest.raises(ctypes.ArgumentError):
        loaded.vvm_time_bridge_grow(a, 4.0, 8, 8, 0, 0, a, a, None)
    import torch
    z = torch.zeros((2, 4, 4), dtype=torch.uint8)
    for call in (lambda: mask_hip.label_components(z), lambda: mask_hip.despeckle(z, z, 4), lambda: mask_hip.time_bridge_grow(z, 1, 0)):
        with pytest.raises(RuntimeError):
            call()                                                                                   # no CPU fallback


def test_product_sources_of_the_feature():
    """vv_mask is in the one build recipe with its header among the dependencies and reads no environment; the settings import no torch; importing
    the drop-in resolves no symbol of the feature."""
    abiref.check_sources("vv_mask", "vvmask.h", "maskclean")
    code = "import diffuerase; from videovanish_amd import mask_hip, hip; assert mask_hip.PART.dll is None and hip.CORE.dll is None"
    import subprocess
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ---- the reference's properties -----------------------------------------------------------------------------------------------------------
def _draw(rng, k):
    """One (x [T,P] bool, g, k, cuts): columns of every kind (empty, full, sparse, dense, dropouts, runs at the ends), cuts anywhere."""
    T = int(rng.integers(1, 48))
    P = 24
    p = rng.choice([0.0, 0.05, 0.3, 0.7, 0.95, 1.0], P)
    x = rng.random((T, P)) < p
    if T > 4:
        x[: T // 3, 0], x[T // 3:, 0] = True, False           # a run at the start only
        x[:, 1] = False
        x[[0, T - 1], 1] = True                               # the two ends only
    g, kk = int(rng.integers(0, 17)), int(rng.integers(0, 9))
    cuts = sorted({int(c) for c in rng.integers(1, max(T, 2), int(rng.integers(0, 4)))} - {T}) if (T > 1 and k % 2) else []
    return x, g, kk, cuts


def test_reference_properties_over_random_draws():
    rng = np.random.default_rng(20250117)
    seen = {"bridged": 0, "grown": 0, "cut_blocks": 0, "end_runs": 0}
    for k in range(200):
        x, g, kk, cuts = _draw(rng, k)
        T = len(x)
        b = R.bridge(x, g)
        # a closing with a flat element of g + 1 frames on the zero-padded sequence
        pad = np.zeros((g + 1, x.shape[1]), bool)
        closed = ndimage.binary_closing(np.concatenate([pad, x, pad]), structure=np.ones((g + 1, 1), bool))[g + 1: g + 1 + T]
        assert (b == closed).all(), (k, T, g)
        assert (b >= x).all() and (R.bridge(b, g) == b).all()                                          # a superset; idempotent
        o = R.grow(b, kk)
        assert (o >= b).all()
        want = np.zeros_like(b)
        for t in range(T):
            want[t] = b[max(0, t - kk): t + kk + 1].any(axis=0)
        assert (o == want).all()
        # with cuts: each segment is a clip of its own, and a column that is empty in a segment stays empty there
        out, counts = R.time_clean(x[:, :, None], g, kk, cuts)
        for s, e in R.segments(T, cuts):
            seg, c = R.time_clean(x[s:e, :, None], g, kk)
            assert (out[s:e] == seg).all() and (counts[s:e] == c).all()
            assert not out[s:e][:, ~x[s:e].any(axis=0)].any()
        assert R.segments(T, cuts) == spans.segments(T, cuts)
        assert set(np.unique(out)) <= {0, 255} and ((out[:, :, 0] > 0) >= x).all()
        assert counts[:, 0].sum() + counts[:, 1].sum() == (out[:, :, 0] > 0).sum() - x.sum()
        whole = R.time_clean(x[:, :, None], g, kk)[0]
        seen["bridged"] += bool(counts[:, 0].any())
        seen["grown"] += bool(counts[:, 1].any())
        seen["cut_blocks"] += bool(cuts) and not (whole == out).all()
        seen["end_runs"] += T > 4 and g >= T and not b[T // 3:, 0].any() and b[:, 1].all()
    assert all(v >= 10 for v in seen.values()), seen


def test_reference_despeckle_properties():
    rng = np.random.default_rng(5)
    for k in range(40):
        H, W = int(rng.integers(5, 40)), int(rng.integers(5, 40))
        raw = (rng.random((2, H, W, 3)) < rng.choice([0.02, 0.1, 0.3])) * rng.integers(1, 256, (2, H, W, 3))
        raw = raw.astype(np.uint8)
        dil = R.dilate(raw, int(rng.integers(1, 4)))
        lab = R.labels(dil)
        assert ((lab >= 0) == (dil > 0)).all()
        for t in range(2):
            roots = np.unique(lab[t][lab[t] >= 0])
            assert (lab[t].reshape(-1)[roots] == roots).all()                                      # a label is a pixel of its own component
            assert len(roots) == ndimage.label(dil[t] > 0, structure=np.ones((3, 3)))[1]
        prev = None
        for a in (0, 1, 2, 5, 30, 10 ** 9):
            out, counts = R.despeckle(dil, raw, a)
            assert ((out == dil) | (out == 0)).all() and (counts[:, 1] == ((dil > 0) & (out == 0)).reshape(2, -1).sum(1)).all()
            assert prev is None or ((out > 0) <= (prev > 0)).all()                                 # a larger threshold keeps less
            prev = out
            if a <= 1:
                assert (out == dil).all() and not counts.any()
        assert not out.any()
        # the threshold weighs raw pixels: it does not depend on the dilation
        a = 3
        kept = lambda it: {(t, int(y), int(x)) for t, y, x in zip(*np.nonzero((R.despeckle(R.dilate(raw, it), raw, a)[0] > 0) & (raw > 0).any(-1)[...]))}
        assert kept(1) <= kept(2) <= kept(3)                                                       # more dilation merges fragments, never drops raw pixels


# ---- the planners on noisy masks ----------------------------------------------------------------------------------------------------------
def _dilate8(m):
    """The 8-step cross dilation of boolean frames [T,H,W], on the window around each frame's pixels only (empty frames stay empty)."""
    out = np.zeros(m.shape, np.uint8)
    for t in range(len(m)):
        b = R.bbox(m[t])
        if b is not None:
            y0, y1, x0, x1 = max(b[0] - 8, 0), b[2] + 8, max(b[1] - 8, 0), b[3] + 8
            out[t, y0:y1, x0:x1] = R.dilate(m[t, y0:y1, x0:x1][None], 8)[0]
    return out


def _bboxes(dil):
    return np.array([R.bbox(f) or (0, 0, 0, 0) for f in dil], np.int64)


def _plans(dil):
    bb = _bboxes(dil)
    masked = (bb[:, 2] > bb[:, 0]) & (bb[:, 3] > bb[:, 1])
    windows = {mode: roi.plan_roi(bb, 1080, 1920, 3, roi.as_config(mode)) for mode in ("static", "follow")}
    return {k: None if p is None else p.size for k, p in windows.items()}, spans.plan_spans(masked, None, spans.as_config("masked"))


def test_planner_table_with_and_without_the_clean_up():
    """A 1920 x 1080 clip of 96 frames with a 160 x 90 logo in frames 28 .. 51: one stray pixel costs the window, three cost the span, and the
    reference clean-up with the default settings gives both back."""
    cfg = MaskCleanConfig()
    area = cfg.area_for(1080, 1920)
    clean = lambda m, d: R.clean(d, m.astype(np.uint8)[..., None], area, cfg.bridge, cfg.grow)
    m = R.logo_clip()
    dil = _dilate8(m)
    assert _plans(dil) == ({"static": (512, 512), "follow": (512, 512)}, [(20, 60)])
    out, counts = clean(m, dil)
    assert (out == dil).all() and not counts.any()                                                    # clean masks need nothing
    # one stray pixel in one frame, in the opposite corner
    m1 = m.copy()
    m1[40, 1000, 1800] = True
    d1 = _dilate8(m1)
    assert _plans(d1)[0] == {"static": None, "follow": None}                                          # the full frame
    out, counts = clean(m1, d1)
    assert (out == dil).all() and counts.sum(0).tolist() == [1, 145, 0, 0]
    # one stray pixel in each of frames 3, 70, 90
    m2 = m.copy()
    for t in (3, 70, 90):
        m2[t, 1000, 1800] = True
    d2 = _dilate8(m2)
    assert _plans(d2)[1] == [(0, 96)]                                                                 # the whole clip
    out, counts = clean(m2, d2)
    assert (out == dil).all() and counts[[3, 70, 90], 0].tolist() == [1, 1, 1]
    assert _plans(out) == ({"static": (512, 512), "follow": (512, 512)}, [(20, 60)])
    # a dropout: the plans do not notice, the frame does
    m3 = m.copy()
    m3[40] = False
    d3 = _dilate8(m3)
    assert _plans(d3)[1] == [(20, 60)] and not d3[40].any()
    out, counts = clean(m3, d3)
    assert (out == dil).all() and counts[40].tolist() == [0, 0, int((dil[40] > 0).sum()), 0]


# ---- orchestration ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def host_kernels(monkeypatch):
    """infill.clean_masks with the two device calls replaced by the reference on host tensors; the calls made are recorded."""
    import torch
    from videovanish_amd import infill, mask_hip
    calls = []
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))

    def despeckle(dil, raw, min_area):
        calls.append(("despeckle", int(min_area)))
        out, counts = R.despeckle(dil.numpy(), raw.numpy(), min_area)
        return t(out), t(counts)

    def time_bridge_grow(mask2d, bridge, grow, out=None, counts=None):
        calls.append(("time", len(mask2d), bridge, grow))
        o, c = R.time_clean(mask2d.numpy(), bridge, grow)
        out.copy_(t(o))
        counts.copy_(t(c))
        return out, counts

    monkeypatch.setattr(mask_hip, "despeckle", despeckle)
    monkeypatch.setattr(mask_hip, "time_bridge_grow", time_bridge_grow)
    return infill, calls, t


def test_clean_masks_order_segments_and_report(host_kernels):
    infill, calls, t = host_kernels
    T, H, W = 10, 12, 16
    raw = np.zeros((T, H, W, 1), np.uint8)
    raw[1:9, 3:7, 4:9] = 255
    raw[4] = 0                                  # a dropout
    raw[2, 10, 14] = 255                        # a speckle
    raw[6, 0, 0] = 255
    dil = R.dilate(raw, 1)
    cfg = MaskCleanConfig(min_area=3, bridge=1, grow=1)
    seen = []

    def find(despeckled):                       # the detector is handed the despeckled masks
        seen.append(despeckled.numpy().copy())
        return [5]

    for cuts, want_cuts in ((None, ()), ([5], (5,)), (find, (5,)), ([0, 99], (0, 99))):
        del calls[:]
        out, rep = infill.clean_masks(t(raw), t(dil), cfg, cuts)
        want, wc = R.clean(dil, raw, 3, 1, 1, want_cuts)
        assert (out.numpy() == want).all() and rep.cuts == want_cuts
        for got, k in ((rep.removed, 0), (rep.cleared, 1), (rep.bridged, 2), (rep.grown, 3)):
            assert got.dtype == np.int64 and got.shape == (T,) and (got == wc[:, k]).all()
        assert calls == [("despeckle", 3)] + [("time", e - s, 1, 1) for s, e in spans.segments(T, want_cuts)]
    assert len(seen) == 1 and (seen[0] == R.despeckle(dil, raw, 3)[0]).all() and not seen[0][2, 10, 14] and dil[2, 10, 14]
    assert rep.removed.sum() == 2 and rep.bridged[4] > 0 and rep.grown[0] > 0 and rep.grown[9] > 0
    assert infill.clean_masks(t(raw), t(dil), cfg, [4])[1].bridged.sum() == 0                     # the dropout touches a segment end
    # a step that is switched off launches nothing; everything off: the masks as they came
    del calls[:]
    d = t(dil)
    out, rep = infill.clean_masks(t(raw), d, MaskCleanConfig(min_area=1, bridge=0, grow=0), [5])
    assert out is d and calls == [] and not (rep.removed.any() or rep.cleared.any() or rep.bridged.any() or rep.grown.any())
    infill.clean_masks(t(raw), d, MaskCleanConfig(min_area=0, bridge=0, grow=2), None)
    infill.clean_masks(t(raw), d, MaskCleanConfig(min_area=None, bridge=0, grow=0), None)          # 12 x 16: the default threshold is 1
    infill.clean_masks(t(raw), d, MaskCleanConfig(min_area=7, bridge=0, grow=0), None)
    assert calls == [("time", T, 0, 2), ("despeckle", 7)]


def test_span_plan_keeps_its_behaviour(monkeypatch):
    """span_plan's cut finding moved into clip_cuts: explicit cuts as given, "auto" from the statistics, else none."""
    from videovanish_amd import infill
    frames = [np.zeros((8, 8, 3), np.uint8)] * 6
    monkeypatch.setattr(infill.spans_hip, "frame_pair_stats", lambda f, d: (_ for _ in ()).throw(AssertionError("no statistics without cuts='auto'")))
    assert infill.clip_cuts(frames, None, spans.SpanConfig("all")) is None
    assert infill.clip_cuts(frames, None, spans.SpanConfig("all", cuts=[4, 2])) == [2, 4]
    assert infill.clip_cuts(frames[:1], None, spans.SpanConfig("all", cuts="auto")) == []
    monkeypatch.setattr(infill.spans_hip, "frame_pair_stats", lambda f, d: ("sad", "n", "hist"))
    monkeypatch.setattr(infill.span_planner, "find_cuts", lambda sad, n, hist, cfg, npix: [3] if (sad, n, hist, npix) == ("sad", "n", "hist", 64) else None)
    assert infill.clip_cuts(frames, None, spans.SpanConfig("all", cuts="auto")) == [3]


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_precedence_argument_configure_environment(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_MASK_CLEAN", raising=False)
    try:
        diffuerase.configure()
        assert diffuerase.mask_clean_config() is None
        monkeypatch.setenv("VV_MASK_CLEAN", "area=9")
        assert diffuerase.mask_clean_config() == MaskCleanConfig(min_area=9)
        diffuerase.configure(mask_clean="grow=2")
        assert diffuerase.mask_clean_config() == MaskCleanConfig(grow=2)
        assert diffuerase.mask_clean_config("on") == MaskCleanConfig()
        assert diffuerase.mask_clean_config("off") is None and diffuerase.mask_clean_config(False) is None      # no clean-up whatever else is set
        diffuerase.configure(mask_clean="off")
        assert diffuerase.mask_clean_config() is None                                                      # configure("off") beats the environment
        diffuerase.configure()
        assert diffuerase.mask_clean_config() == MaskCleanConfig(min_area=9)                               # configure() resets
        cfg = MaskCleanConfig(min_area=4, bridge=1)
        diffuerase.configure(mask_clean=cfg)
        assert diffuerase.mask_clean_config() is cfg
        with pytest.raises(ValueError):
            diffuerase.configure(mask_clean="sometimes")
        monkeypatch.setenv("VV_MASK_CLEAN", "sometimes")
        diffuerase.configure()
        with pytest.raises(ValueError):
            diffuerase.mask_clean_config()
    finally:
        diffuerase.configure()


def test_mask_clean_refuses_the_reference_early_return(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_MASK_CLEAN", raising=False)
    f = [np.zeros((8, 8, 3), np.uint8)] * 2
    for value in ("on", "grow=1", MaskCleanConfig()):
        with pytest.raises(ValueError, match="mask_clean="):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, mask_clean=value)
    monkeypatch.setenv("VV_MASK_CLEAN", "on")
    with pytest.raises(ValueError, match="mask_clean="):
        diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)
    with pytest.raises(TypeError):
        diffuerase.run_infill_on_frames(f, f, mask_cleanup="on")


def test_cli_mask_clean_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
    """tests/test_cli_cpu.py's stub: frame I/O and the hot path replaced."""
    import diffuerase
    from videovanish_amd import infill
    calls = []
    videos = {"mask.mkv": [np.zeros((16, 24, 3), np.uint8)] * 3}
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda path, start=0, max_frames=-1: ([f.copy() for f in videos[path]], 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    z = np.zeros(3, np.int64)

    def fake(frames, masks, **kw):
        calls.append(kw)
        diffuerase.last_mask_clean = infill.MaskCleanReport(z + [1, 0, 2], z + [145, 0, 150], z + [0, 40, 0], z, ()) if "mask_clean" in kw else None
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 3
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    monkeypatch.setattr(sys, "argv", argv)
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None} and capsys.readouterr().out == ""                      # a default call passes no keyword, prints nothing
    for value in ("on", "area=64,bridge=2,grow=1"):
        monkeypatch.setattr(sys, "argv", argv + ["--mask-clean", value, "--roi", "static"])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "mask_clean": value, "roi": "static"}
        out = capsys.readouterr().out
        assert out.count("\n") == 1 and out.startswith("mask clean-up: 3 components (295 px) cleared in 2 frames, 40 px bridged in 1 frames, 0 px grown")
    for bad in ("off", "yes", "area=x"):
        monkeypatch.setattr(sys, "argv", argv + ["--mask-clean", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_mask_clean", None)
