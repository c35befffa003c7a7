"""Clean-plate fill on the CPU: the settings, the binding of include/vvplate.h, the reference restatement (tests/platefill_ref.py) on the
prototype's clips, the orchestration with the device functions replaced by the reference, configuration and CLI."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abiref  # noqa: E402
import platefill_ref as R  # noqa: E402

from videovanish_amd import platefill as PF  # noqa: E402
from videovanish_amd import spans  # noqa: E402
from videovanish_amd.platefill import PlateFillConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_spellings_and_config():
    assert PF.SPELLINGS == ("on",)
    for off in (None, False, "off", "none", "", " OFF "):
        assert PF.as_config(off) is None
    d = PlateFillConfig()
    assert PF.as_config("on") == PF.as_config(" On ") == PF.as_config(True) == d
    assert (d.guard, d.min_samples, d.tol, d.outlier, d.max_gap, d.margin) == (1, 4, 6, 3, 0, 2) == tuple(R.DEFAULTS[k] for k in
                                                                                                            ("guard", "min_samples", "tol", "outlier", "max_gap", "margin"))
    assert PF.as_config("guard=1,min_samples=4,tol=6,outlier=3,max_gap=0,margin=2") == d
    assert PF.as_config(" tol = 9 , guard = 0 ") == PlateFillConfig(guard=0, tol=9)
    assert PF.as_config("max_bytes=1000").max_bytes == 1000 and PF.as_config("max_gap=65535").max_gap == 65535
    cfg = PlateFillConfig(margin=0)
    assert PF.as_config(cfg) is cfg
    for bad in ("yes", "static", "tol", "tol=", "tol=x", "tol=-3", "tol=1.5", "tol=3,tol=4", "size=3", "tol=3;guard=1", "guard=9", "tol=256", "outlier=65",
                "max_gap=65536", "margin=17", "min_samples=0", "on,tol=1", "tol=3,", 3, 1.0, ("on",)):
        with pytest.raises(ValueError):
            PF.as_config(bad)
    for kw in (dict(guard=-1), dict(guard=9), dict(tol=-1), dict(tol=256), dict(outlier=-1), dict(outlier=65), dict(max_gap=-1), dict(max_gap=65536),
               dict(margin=-1), dict(margin=17), dict(min_samples=0), dict(min_samples=65536), dict(max_bytes=-1), dict(tol=6.0), dict(guard=True),
               dict(margin="2")):
        with pytest.raises(ValueError):
            PlateFillConfig(**kw)


def test_crop_box():
    e = (0, 0, 0, 0)
    assert PF.crop_box([e, e], 40, 56) is None
    assert PF.crop_box([e, (4, 5, 19, 11), (6, 9, 21, 30)], 40, 56) == (4, 4, 21, 32)          # the union, x to multiples of 4
    assert PF.crop_box([(0, 0, 40, 56)], 40, 56) == (0, 0, 40, 56)
    assert PF.crop_box([(1, 50, 2, 54)], 40, 54) == (1, 48, 2, 54)                             # x1 stops at the frame
    assert PF.crop_bytes(7, (4, 4, 21, 32)) == 7 * 17 * 28 * 3


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_vvplate_header():
    """plate_hip.SIGNATURES declares every function of include/vvplate.h with the header's types, plate_hip.lib() has applied it, the version and
    the range constants agree (abiref.check_binding; test_abi_cpu.py: no name could be taken for another part's), and arguments are refused
    before anything touches a device."""
    from videovanish_amd import mask_hip, plate_hip
    loaded, define = abiref.check_binding(plate_hip, 5)
    assert define("VVP_ABI_VERSION") == 1
    limits = (define("VVP_MAX_T"), define("VVP_NO_SOURCE"), define("VVP_MAX_GUARD"), define("VVP_MAX_TOL"), define("VVP_MAX_OUTLIER"), define("VVP_MAX_GAP"))
    assert limits == (plate_hip.MAX_T, plate_hip.NO_SOURCE, plate_hip.MAX_GUARD, plate_hip.MAX_TOL, plate_hip.MAX_OUTLIER, plate_hip.MAX_GAP)
    assert limits == (65535, R.NONE, 8, 255, 64, 65535)
    assert (PF.MAX_T, PF.MAX_GUARD, PF.MAX_TOL, PF.MAX_OUTLIER, PF.MAX_GAP) == (limits[0],) + limits[2:]
    assert plate_hip.MAX_GUARD == mask_hip.MAX_GROW and plate_hip.TILE % 4 == 0                       # the guard is vvm_time_bridge_grow's grow
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    st = lambda *v: loaded.vvp_stats(a, a, None, *v, a, a, a, None)                                    # T, H, W, tile, min_samples, tol
    so = lambda *v: loaded.vvp_sources(a, a, a, None, a, a, a, *v, a, a, None)                         # T, H, W, tile, tol, outlier, max_gap
    assert loaded.vvp_stats(None, a, None, 2, 8, 8, 64, 4, 6, a, a, a, None) == -1 and b"vvp_stats" in loaded.vvp_last_error()
    assert [st(0, 8, 8, 64, 4, 6), st(2, 0, 8, 64, 4, 6), st(2, 1 << 16, 1 << 15, 64, 4, 6), st(2, 8, 8, 64, 0, 6), st(2, 8, 8, 64, 4, -1)] == [-1] * 5
    assert loaded.vvp_stats(a, a, a, 2, 8, 8, 0, 4, 6, a, a, a, None) == -1                            # a tile grid needs a tile
    assert [st(65536, 8, 8, 64, 4, 6), st(2, 8, 8, 64, 4, 256)] == [-2] * 2 and b"vvp_stats" in loaded.vvp_last_error()
    assert [so(0, 8, 8, 64, 6, 3, 0), so(2, 8, 8, 64, -1, 3, 0), so(2, 8, 8, 64, 6, -1, 0), so(2, 8, 8, 64, 6, 3, -1)] == [-1] * 4
    assert b"vvp_sources" in loaded.vvp_last_error()
    assert [so(65536, 8, 8, 64, 6, 3, 0), so(2, 8, 8, 64, 256, 3, 0), so(2, 8, 8, 64, 6, 65, 0), so(2, 8, 8, 64, 6, 3, 65536)] == [-2] * 4
    assert loaded.vvp_fill(a, a, a, None, a, 0, 8, 8, 64, a + 8, a, None) == -1 and b"vvp_fill" in loaded.vvp_last_error()
    assert loaded.vvp_fill(a, a, a, None, a, 2, 8, 8, 64, a, a, None) == -1                            # dil_out is not dil
    assert loaded.vvp_fill(a, a, a, None, a, 65536, 8, 8, 64, a + 8, a, None) == -2
    with pytest.raises(ctypes.ArgumentError):
        loaded.vvp_stats(a, a, None, 2.0, 8, 8, 64, 4, 6, a, a, a, None)
    import torch
    f, z = torch.zeros((2, 4, 4, 3), dtype=torch.uint8), torch.zeros((2, 4, 4), dtype=torch.uint8)
    for call in (lambda: plate_hip.stats(f, z, None, 4, 6), lambda: plate_hip.fill(f, z, z, None, z.to(torch.int16))):
        with pytest.raises(RuntimeError):
            call()                                                                                   # no CPU fallback


def test_product_sources_of_the_feature():
    """vv_plate is in the one build recipe with its header among the dependencies and reads no environment; the settings import no torch; importing
    the drop-in resolves no symbol of the feature, and neither does a call's set-up without the option."""
    abiref.check_sources("vv_plate", "vvplate.h", "platefill")
    code = ("import diffuerase; from videovanish_amd import plate_hip, hip; assert plate_hip.PART.dll is None and hip.CORE.dll is None; "
            "assert diffuerase.plate_fill_config() is None and diffuerase.last_plate_fill is None")
    env = {k: v for k, v in os.environ.items() if k != "VV_PLATE_FILL"}
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)


# ---- the reference on the prototype's clips: a failure here means the rule is wrong, not the kernel ------------------------------------------
@pytest.mark.parametrize("a", [0, 3, 6])
def test_reference_fills_the_box_of_a_locked_off_clip_and_leaves_the_logo(a):
    frames, masks, clean, boxm, logom = R.locked_off_clip(a=a)
    out, dil, counts = R.plate_fill(frames, masks)
    hole = masks != 0
    assert boxm.sum() > 4000 and logom.sum() * len(frames) == 1152
    assert not dil[boxm].any()                                                                    # every box pixel is filled
    assert np.abs(out[boxm].astype(np.int64) - clean[boxm]).max() <= a                            # within the noise bound of the clean background
    assert (dil[:, logom] == 255).all() and (out[:, logom] == frames[:, logom]).all()             # every logo pixel is left
    assert (out[~hole] == frames[~hole]).all() and not dil[~hole].any()                           # outside the mask: the bytes
    assert counts[:, 0].sum() == boxm.sum() and (counts[:, 1] == logom.sum()).all() and (counts.sum(1) == hole.reshape(len(hole), -1).sum(1)).all()


def test_reference_fills_nothing_over_a_panning_texture():
    frames, masks, boxm, logom = R.panning_clip()
    out, dil, counts = R.plate_fill(frames, masks)
    assert (out == frames).all() and (dil == masks).all() and not counts[:, 0].any()


def test_reference_drift_segments_and_margin():
    # 1 level per frame: a standard deviation of about 7 over 24 frames: nothing is filled (a stated limit); 1/4 level per frame: most of it
    frames, masks, clean, boxm, logom = R.locked_off_clip(drift_q4=4)
    out, dil, counts = R.plate_fill(frames, masks)
    assert (out == frames).all() and (dil == masks).all()
    frames, masks, clean, boxm, logom = R.locked_off_clip(drift_q4=1)
    out, dil, counts = R.plate_fill(frames, masks)
    got = boxm & (dil == 0)
    assert got.sum() > 0.7 * boxm.sum() and np.abs(out[got].astype(np.int64) - clean[got]).max() <= 6 + 6
    hole = masks != 0
    assert (out[~hole] == frames[~hole]).all()
    # every segment is a clip of its own; nothing is taken from across a cut
    frames, masks, clean, boxm, logom = R.locked_off_clip()
    out, dil, counts = R.plate_fill(frames, masks, cuts=[9, 15])
    for s, e in R.segments(24, [9, 15]):
        o, d, c = R.fill_segment(frames[s:e], masks[s:e])
        assert (out[s:e] == o).all() and (dil[s:e] == d).all() and (counts[s:e] == c).all()
    assert counts[9:15, 0].sum() == 0 and counts[:9, 0].sum() > 0                                 # six frames give no pixel four samples
    # the margin keeps a band round what is left, inside the mask only
    o0, d0, c0 = R.plate_fill(frames, masks, **dict(R.DEFAULTS, margin=0, max_gap=3))
    o2, d2, c2 = R.plate_fill(frames, masks, **dict(R.DEFAULTS, margin=2, max_gap=3))
    assert ((d2 != 0) >= (d0 != 0)).all() and c2[:, 1].sum() > c0[:, 1].sum() > logom.sum() * 24 and ((d2 != 0) <= hole).all()


# ---- orchestration ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def host_kernels(monkeypatch):
    """infill.plate_fill with every device call replaced by the reference on host tensors; the calls made are recorded."""
    import torch
    from scipy import ndimage
    from videovanish_amd import hip, infill, mask_hip, plate_hip
    calls = []
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))

    def mask_bbox(m):
        calls.append(("bbox", tuple(m.shape)))
        out = np.zeros((len(m), 4), np.int32)
        for i, f in enumerate(m.numpy()):
            ys, xs = np.nonzero(f.any(1))[0], np.nonzero(f.any(0))[0]
            if len(ys):
                out[i] = ys[0], xs[0], ys[-1] + 1, xs[-1] + 1
        return t(out)

    def mask_tile_union(m, tile):
        calls.append(("occ", tuple(m.shape), tile))
        T, H, W = m.shape
        occ = np.zeros(((H + tile - 1) // tile, (W + tile - 1) // tile), np.uint8)
        for y, x in zip(*np.nonzero(m.numpy().any(0))):
            occ[y // tile, x // tile] = 1
        return t(occ)

    def time_bridge_grow(m, bridge, grow):
        calls.append(("guard", len(m), bridge, grow))
        return t(R.not_sample(m.numpy(), grow).astype(np.uint8) * 255), None

    def stats(f, ns, occ, min_samples, tol):
        calls.append(("stats", tuple(f.shape), min_samples, tol))
        assert f.is_contiguous() and ns.is_contiguous() and occ is not None
        n, S1, S2 = R.stats(f.numpy(), ns.numpy() != 0)
        return t(R.steady(n, S1, S2, min_samples, tol).astype(np.uint8)), t(n.astype(np.int32)), t(S1.astype(np.int32))

    def sources(f, d, ns, occ, st, n, s1, tol, outlier, max_gap):
        calls.append(("sources", tol, outlier, max_gap))
        us = R.usable(f.numpy(), ns.numpy() != 0, st.numpy() != 0, n.numpy().astype(np.int64), s1.numpy().astype(np.int64), tol, outlier)
        src = R.sources(d.numpy(), us, max_gap)
        return t(src.view(np.int16)), t(((d.numpy() != 0) & (src == R.NONE)).astype(np.uint8) * 255)

    def dilate(m, iters):
        calls.append(("margin", iters))
        return t(R.dilate(m.numpy()[..., 0] != 0, iters).astype(np.uint8) * 255)

    def fill(f, d, keep, occ, src):
        calls.append(("fill", tuple(f.shape)))
        dn, s = d.numpy() != 0, src.numpy().view(np.uint16)
        left = dn & (keep.numpy() != 0)
        go = dn & ~left
        tt, yy, xx = np.nonzero(go)
        f.numpy()[tt, yy, xx] = f.numpy()[s[tt, yy, xx].astype(np.int64), yy, xx]                    # in place, as the device does
        T = len(dn)
        return t(left.astype(np.uint8) * 255), t(np.stack([go.reshape(T, -1).sum(1), left.reshape(T, -1).sum(1)], 1).astype(np.int64))

    monkeypatch.setattr(hip, "mask_bbox", mask_bbox)
    monkeypatch.setattr(hip, "mask_tile_union", mask_tile_union)
    monkeypatch.setattr(hip, "mask_collapse_dilate", dilate)
    monkeypatch.setattr(mask_hip, "time_bridge_grow", time_bridge_grow)
    monkeypatch.setattr(plate_hip, "stats", stats)
    monkeypatch.setattr(plate_hip, "sources", sources)
    monkeypatch.setattr(plate_hip, "fill", fill)
    return infill, calls, t


def test_plate_fill_crop_segments_copy_on_write_and_report(host_kernels):
    infill, calls, t = host_kernels
    frames, masks, clean, boxm, logom = R.locked_off_clip()
    T = len(frames)
    flist = [f.copy() for f in frames]
    kept = [f.copy() for f in flist]
    d = t(masks)
    for cuts in (None, [9, 15], [12]):
        del calls[:]
        out, dil, rep = infill.plate_fill(flist, d, PlateFillConfig(), cuts)
        want, wd, wc = R.plate_fill(frames, masks, cuts=cuts)
        assert (np.stack(out) == want).all() and (dil.numpy() == wd).all()
        assert rep.filled.dtype == np.int64 and (rep.filled == wc[:, 0]).all() and (rep.left == wc[:, 1]).all()
        assert rep.cuts == tuple(cuts or ()) and list(rep.segments) == spans.segments(T, cuts) and rep.skipped == (False,) * len(rep.segments)
        assert all(s > 0 for s in rep.steady) and len(rep.steady) == len(rep.segments)
        # the caller's arrays are never written; a frame with nothing filled is the same object, a filled one a new array
        assert all((a == b).all() for a, b in zip(flist, kept)) and (d.numpy() == masks).all() and dil is not d
        for i in range(T):
            assert (out[i] is flist[i]) == (wc[i, 0] == 0), i
        # one upload per segment: the crop of the union box, x to multiples of 4 (the box leaves rows 4 .. 18, the logo rows 26 .. 37)
        shapes = [c[1] for c in calls if c[0] == "stats"]
        want_shapes = []
        for s, e in spans.segments(T, cuts):
            xs = np.nonzero(masks[s:e].any(axis=(0, 1)))[0]
            want_shapes.append((e - s, 34, min(56, -(-(xs[-1] + 1) // 4) * 4) - xs[0] // 4 * 4, 3))
        assert shapes == want_shapes and (cuts is not None or shapes == [(24, 34, 56, 3)])
        assert [c for c in calls if c[0] == "guard"] == [("guard", e - s, 0, 1) for s, e in spans.segments(T, cuts)]
        assert ("margin", 2) in calls and ("sources", 6, 3, 0) in calls
    # guard = 0 and margin = 0 launch nothing for them
    del calls[:]
    out, dil, rep = infill.plate_fill(flist, d, PlateFillConfig(guard=0, margin=0), None)
    want, wd, wc = R.plate_fill(frames, masks, **dict(R.DEFAULTS, guard=0, margin=0))
    assert (np.stack(out) == want).all() and (dil.numpy() == wd).all() and not [c for c in calls if c[0] in ("guard", "margin")]


def test_plate_fill_skips_and_nothing_to_do(host_kernels):
    infill, calls, t = host_kernels
    frames, masks, clean, boxm, logom = R.locked_off_clip()
    flist = list(frames)
    d = t(masks)
    # max_bytes: the crop of the whole clip is 24 * 34 * 56 * 3 bytes
    full = 24 * 34 * 56 * 3
    out, dil, rep = infill.plate_fill(flist, d, PlateFillConfig(max_bytes=full - 1), None)
    assert rep.skipped == (True,) and dil is d and all(a is b for a, b in zip(out, flist)) and not rep.filled.any()
    assert (rep.left == (masks != 0).reshape(24, -1).sum(1)).all() and not [c for c in calls if c[0] in ("stats", "occ", "fill")]
    out, dil, rep = infill.plate_fill(flist, d, PlateFillConfig(max_bytes=full), None)
    assert rep.skipped == (False,) and rep.filled.sum() == boxm.sum()
    # a segment without a mask pixel uploads nothing; one segment skipped, the others filled
    m2 = masks.copy()
    m2[:6] = 0
    del calls[:]
    out, dil, rep = infill.plate_fill(flist, t(m2), PlateFillConfig(max_bytes=8 * 34 * 56 * 3), [6, 14])      # 10 frames x 52 columns are more
    assert rep.skipped == (False, False, True) and rep.steady[0] == 0 and rep.steady[1] > 0 and rep.steady[2] == 0
    assert [c[1][0] for c in calls if c[0] == "stats"] == [8] and not rep.filled[:6].any() and not rep.left[:6].any() and rep.left[14:].all()
    want = R.plate_fill(frames, m2, cuts=[6, 14])
    assert (np.stack(out[:14]) == want[0][:14]).all() and all(out[i] is flist[i] for i in range(14, 24))
    assert (dil.numpy()[:14] == want[1][:14]).all() and (dil.numpy()[14:] == m2[14:]).all()
    # no mask at all: the arguments come back
    z = t(np.zeros_like(masks))
    out, dil, rep = infill.plate_fill(flist, z, PlateFillConfig(), None)
    assert dil is z and all(a is b for a, b in zip(out, flist)) and rep.steady == (0,) and not rep.left.any()
    # nothing can be filled (a panning texture): the same objects, so the call's bytes are those of the call without the option
    pf, pm, _, _ = R.panning_clip()
    plist, pd = list(pf), t(pm)
    out, dil, rep = infill.plate_fill(plist, pd, PlateFillConfig(), None)
    assert dil is pd and all(a is b for a, b in zip(out, plist)) and not rep.filled.any() and rep.left.sum() == (pm != 0).sum()


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_precedence_argument_configure_environment(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_PLATE_FILL", raising=False)
    try:
        diffuerase.configure()
        assert diffuerase.plate_fill_config() is None
        monkeypatch.setenv("VV_PLATE_FILL", "tol=9")
        assert diffuerase.plate_fill_config() == PlateFillConfig(tol=9)
        diffuerase.configure(plate_fill="guard=2")
        assert diffuerase.plate_fill_config() == PlateFillConfig(guard=2)
        assert diffuerase.plate_fill_config("on") == PlateFillConfig()
        assert diffuerase.plate_fill_config("off") is None and diffuerase.plate_fill_config(False) is None
        diffuerase.configure(plate_fill="off")
        assert diffuerase.plate_fill_config() is None                                                      # configure("off") beats the environment
        diffuerase.configure()
        assert diffuerase.plate_fill_config() == PlateFillConfig(tol=9)                                    # configure() resets
        with pytest.raises(ValueError):
            diffuerase.configure(plate_fill="sometimes")
        monkeypatch.setenv("VV_PLATE_FILL", "sometimes")
        diffuerase.configure()
        with pytest.raises(ValueError):
            diffuerase.plate_fill_config()
    finally:
        diffuerase.configure()


def test_plate_fill_refuses_the_reference_early_return_and_is_keyword_only(monkeypatch):
    import inspect

    import diffuerase
    monkeypatch.delenv("VV_PLATE_FILL", raising=False)
    f = [np.zeros((8, 8, 3), np.uint8)] * 2
    for value in ("on", "tol=1", PlateFillConfig()):
        with pytest.raises(ValueError, match="plate_fill="):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, plate_fill=value)
    monkeypatch.setenv("VV_PLATE_FILL", "on")
    with pytest.raises(ValueError, match="plate_fill="):
        diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)
    with pytest.raises(TypeError):
        diffuerase.run_infill_on_frames(f, f, platefill="on")
    params = list(inspect.signature(diffuerase.run_infill_on_frames).parameters.values())
    assert params[-1].name == "plate_fill" and params[-1].kind is inspect.Parameter.KEYWORD_ONLY and params[-1].default is None
    assert list(inspect.signature(diffuerase.configure).parameters)[-1] == "plate_fill"
    assert diffuerase.last_plate_fill is None                                                          # reset at the start of every call


def test_cli_plate_fill_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
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
        diffuerase.last_plate_fill = infill.PlateFillReport(z + [100, 0, 50], z + [7, 7, 0], (40,), (False,), ((0, 3),), ()) if "plate_fill" in kw else None
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 3
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    monkeypatch.setattr(sys, "argv", argv)
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None} and capsys.readouterr().out == ""                      # a default call passes no keyword, prints nothing
    for value in ("on", "guard=2,tol=8"):
        monkeypatch.setattr(sys, "argv", argv + ["--plate-fill", value, "--spans", "masked"])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "plate_fill": value, "spans": "masked"}
        out = capsys.readouterr().out
        assert out.count("\n") == 1 and out.startswith("plate fill: 150 px filled in 2 frames, 14 px left to the model in 2 of 3 frames, 0 of 1 segments skipped")
    for bad in ("off", "yes", "tol=x"):
        monkeypatch.setattr(sys, "argv", argv + ["--plate-fill", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_plate_fill", None)
