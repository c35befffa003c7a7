"""Aligned inpaint deflicker on the CPU: the binding of include/vvflickalign.h, the product sources, the invariants of the restatement
(tests/deflickeralign_ref.py) against the unaligned one (tests/deflicker_ref.py), the rule on a synthetic pan with the true offsets and with the
tracker's restatement in the loop, the report, configuration and CLI."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abiref  # noqa: E402
import deflicker_ref as R0  # noqa: E402
import deflickeralign_ref as R  # noqa: E402
import platealign_ref as A  # noqa: E402

from videovanish_amd import deflickeralign as DA  # noqa: E402
from videovanish_amd.deflicker import DeflickerConfig  # noqa: E402
from videovanish_amd.platealign import PlateAlignConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_settings_are_the_trackers():
    assert DA.DeflickerAlignConfig is PlateAlignConfig and DA.SPELLINGS == ("on",)
    for off in (None, False, "off", "none", "", " OFF "):
        assert DA.as_config(off) is None
    assert DA.as_config("on") == DA.as_config(True) == PlateAlignConfig() == PlateAlignConfig(**A.DEFAULTS)
    assert DA.as_config(" radius = 2 , levels=1 ") == PlateAlignConfig(levels=1, radius=2)
    cfg = PlateAlignConfig(max_residual=3)
    assert DA.as_config(cfg) is cfg
    for bad in ("yes", "radius", "radius=0", "levels=7", "tol=3", "radius=1,radius=2", 3, ("on",)):
        with pytest.raises(ValueError) as e:
            DA.as_config(bad)
        assert "plate_align" not in str(e.value) or "PlateAlignConfig" in str(e.value)
    with pytest.raises(ValueError, match="deflicker_align must be"):
        DA.as_config("sometimes")
    tr = DA.identity_track(4)
    assert tr.shape == (4, 8) and tr.dtype == np.int32 and (tr[:, 3] == 1).all() and not tr[:, :3].any() and DA.path_of(tr) == "static"
    tr[2, 0] = 1
    assert DA.path_of(tr) == "tracked"
    tr[2, 0], tr[3, 3] = 0, 0
    assert DA.path_of(tr) == "tracked"                                                             # a lost frame must stay unfiltered


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_vvflickalign_header():
    """flickalign_hip.SIGNATURES declares every function of include/vvflickalign.h with the header's types, flickalign_hip.lib() has applied it,
    the version and the limits agree in the header, the binding and vvflicker.h (abiref.check_binding; test_abi_cpu.py: no name could be taken
    for another part's), and arguments are refused before anything touches a device."""
    from videovanish_amd import align_hip, flickalign_hip, flicker_hip
    loaded, define = abiref.check_binding(flickalign_hip, 3)
    assert flickalign_hip.EXPORTS == ["vvc_abi_version", "vvc_last_error", "vvc_hold"] and define("VVC_ABI_VERSION") == 1
    limits = (define("VVC_MAX_RADIUS"), define("VVC_MAX_T"), define("VVC_TRACK_INTS"))
    assert limits == (flickalign_hip.MAX_RADIUS, flickalign_hip.MAX_T, flickalign_hip.TRACK_INTS) == (4, 65535, 8)
    assert limits == (flicker_hip.MAX_RADIUS, flicker_hip.MAX_T, align_hip.TRACK_INTS) and flickalign_hip.NSUM == flicker_hip.NSUM == R.NSUM == 12
    # refusals: nothing is launched, the message names the function
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    hold = lambda *v, out=a + 32: loaded.vvc_hold(a, a, a, a, *v, out, a, None)                       # T, H0, W0, h, w, radius, tol
    nulls = [loaded.vvc_hold(*(None if k == j else a for k in range(4)), 2, 8, 8, 8, 8, 1, 1, a + 32, a, None) for j in range(4)]
    assert nulls + [loaded.vvc_hold(a, a, a, a, 2, 8, 8, 8, 8, 1, 1, a + 32, None, None), hold(0, 8, 8, 8, 8, 1, 1), hold(2, 0, 8, 8, 8, 1, 1),
                    hold(2, 8, 8, 9, 8, 1, 1), hold(2, 8, 8, 8, 9, 1, 1), hold(2, 8, 8, 8, 8, -1, 1), hold(2, 8, 8, 8, 8, 1, -1),
                    hold(2, 8, 8, 8, 8, 1, 1, out=a), hold(2, 8, 8, 8, 8, 1, 1, out=None)] == [-1] * 13
    assert b"vvc_hold" in loaded.vvc_last_error()
    assert [hold(2, 8, 8, 8, 8, 5, 1), hold(2, 8, 8, 8, 8, 1, 256), hold(65536, 8, 8, 8, 8, 1, 1), hold(2, 1 << 16, 1 << 15, 1 << 16, 1 << 15, 1, 1)] == [-2] * 4
    assert b"vvc_hold" in loaded.vvc_last_error() and loaded.vvc_last_error() == flicker_hip.lib().vvf_last_error()
    with pytest.raises(ctypes.ArgumentError):
        loaded.vvc_hold(a, a, a, a, 2.0, 8, 8, 8, 8, 1, 1, a + 32, a, None)
    import torch
    f, z = torch.zeros((2, 8, 8, 3), dtype=torch.uint8), torch.zeros((2, 8, 8), dtype=torch.uint8)
    o, tr = torch.zeros((2, 2), dtype=torch.int32), torch.zeros((2, 8), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        flickalign_hip.hold(f, o, tr, z, 2, 12)                                                      # no CPU fallback


def test_product_sources_of_the_feature():
    """The kernel lives in vv_flicker.hip beside the gather form, as one body; the header is among the recipe's dependencies; the settings
    import no torch and no oracle; importing the drop-in resolves no vvc_ symbol; vvflicker.h keeps its four functions."""
    hipsrc, txt = abiref.check_sources("vv_flicker", "vvflickalign.h", "deflickeralign")
    assert "include/vvflicker.h" in open(os.path.join(abiref.CSRC, "build.sh")).read()
    assert len(re.findall(r"void hold_gather_kernel\(", hipsrc)) == 1 and "hold_gather_kernel<true>" in hipsrc and "hold_gather_kernel<false>" in hipsrc
    assert len(re.findall(r'extern "C" [^(]*\bvvc_', hipsrc)) == 3
    assert "vvc_" not in open(os.path.join(ROOT, "include", "vvflicker.h")).read()
    assert "class " not in txt
    code = ("import sys, diffuerase; from videovanish_amd import flickalign_hip, flicker_hip, align_hip, hip; "
            "assert flickalign_hip.PART.dll is None and flicker_hip.PART.dll is None and align_hip.PART.dll is None and hip.CORE.dll is None; "
            "assert diffuerase.deflicker_align_config() is None and diffuerase.last_deflicker_align is None")
    env = {k: v for k, v in os.environ.items() if k not in ("VV_DEFLICKER", "VV_DEFLICKER_ALIGN")}
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)
    code = "import sys, videovanish_amd.deflickeralign as d; assert 'torch' not in sys.modules and d.as_config('on').radius == 4"
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)


# ---- invariants of the restatement --------------------------------------------------------------------------------------------------------
def _random_clip(seed, T=9, h=12, w=16, H0=20, W0=24, moving=True):
    """test_deflicker_cpu's clip: one background fixed in the frame seen through windows, +-9 levels of noise, a real change, a random mask."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H0, W0, 3))
    offsets = np.stack([rng.integers(0, H0 - h + 1, T), rng.integers(0, W0 - w + 1, T)], 1) if moving else np.tile([[3, 5]], (T, 1))
    win = np.stack([base[oy:oy + h, ox:ox + w] for oy, ox in offsets]) + rng.integers(-9, 10, (T, h, w, 3))
    win[T // 2:, :, w // 2:] += 60
    mask = (rng.random((T, H0, W0)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (T, H0, W0)).astype(np.uint8)
    return np.clip(win, 0, 255).astype(np.uint8), offsets.astype(np.int32), mask


def _panned_clip(seed, off, T=9, h=12, w=16, H0=20, W0=24, moving=True):
    """One background fixed on the CANVAS: the window pixel (yy, xx) of frame t shows wide[offsets[t] + (yy, xx) + off[t]]; +-5 levels of noise."""
    rng = np.random.default_rng(seed)
    offsets = np.stack([rng.integers(0, H0 - h + 1, T), rng.integers(0, W0 - w + 1, T)], 1) if moving else np.tile([[3, 5]], (T, 1))
    ey, ex = offsets[:, 0] + off[:, 1], offsets[:, 1] + off[:, 0]
    wide = rng.integers(0, 256, (ey.max() - ey.min() + h, ex.max() - ex.min() + w, 3))
    win = np.stack([wide[y - ey.min():y - ey.min() + h, x - ex.min():x - ex.min() + w] for y, x in zip(ey, ex)]) + rng.integers(-5, 6, (T, h, w, 3))
    mask = (rng.random((T, H0, W0)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (T, H0, W0)).astype(np.uint8)
    return np.clip(win, 0, 255).astype(np.uint8), offsets.astype(np.int32), mask


@pytest.mark.parametrize("moving", [False, True])
def test_zero_track_is_the_unaligned_rule(moving):
    win, offs, mask = _random_clip(5, moving=moving)
    for radius, tol in ((1, 4), (2, 12), (4, 255), (0, 12), (2, 0)):
        out, sums = R.hold(win, offs, R.make_track(np.zeros((len(win), 2), int)), mask, radius, tol)
        want, wsums = R0.hold(win, offs, mask, radius, tol)
        assert (out == want).all() and (sums == wsums).all()


@pytest.mark.parametrize("moving", [False, True])
def test_all_tracked_is_the_unaligned_rule_on_the_canvas(moving):
    """With every frame tracked the rule is vvflicker.h's with the windows placed at offsets + off: an independent statement of the same thing.
    The mask half of the sums is not compared: the unaligned rule reads the mask at the canvas place, this one at p in frame t."""
    T = 9
    off = R.walk(T, 11, (-3, 4), (-2, 2))
    win, offs, mask = _panned_clip(6, off, moving=moving)
    changed = 0
    for radius, tol in ((1, 4), (2, 12), (4, 255)):
        out, sums = R.hold(win, offs, R.make_track(off), mask, radius, tol)
        want, wsums = R0.hold(win, offs + off[:, ::-1], mask, radius, tol)
        assert (out == want).all() and (sums[:, :6] == wsums[:, :6]).all()
        d = np.abs(out.astype(int) - win.astype(int))
        assert d.max() <= tol                                                                       # no byte moves more than tol
        assert (sums[:, 0] == win.shape[1] * win.shape[2]).all() and (sums[:, 3:6] == d.reshape(T, -1, 3).sum(1)).all()
        assert (sums[:, 6:] <= sums[:, :6]).all() and sums[:, 6].any()
        # the mask half against the mask moved to the canvas by hand
        for t in range(T):
            yy, xx = np.mgrid[0:win.shape[1], 0:win.shape[2]]
            sel = mask[t][offs[t, 0] + yy, offs[t, 1] + xx] != 0
            assert sums[t, 6] == sel.sum() and (sums[t, 9:12] == d[t][sel].sum(0)).all()
        changed += int(sums[:, 1].sum())
        fixed, fsums = R0.hold(win, offs, mask, radius, tol)                                        # the fixed-place filter sees another background
        assert tol == 255 or fsums[:, 2].sum() < sums[:, 2].sum()
    assert changed


def test_lost_frames_take_no_sample_and_give_none():
    T, L = 9, 4
    off = R.walk(T, 3, (-2, 3), (-1, 1))
    win, offs, mask = _panned_clip(8, off)
    h, w = win.shape[1:3]
    out, sums = R.hold(win, offs, R.make_track(off, lost=(L,)), mask, 2, 12)
    assert (out[L] == win[L]).all() and sums[L, 2] == h * w and not sums[L, [1, 3, 4, 5, 7, 9, 10, 11]].any()      # as it is, n = 1
    full, _ = R.hold(win, offs, R.make_track(off), mask, 2, 12)
    assert (full[L] != win[L]).any() and (out[[L - 1, L + 1]] != full[[L - 1, L + 1]]).any()       # tracked, it would have taken and given
    # taking it out of the others' neighbours: as a tracked frame whose window lies nowhere near (no place q inside it) ...
    away = off.copy()
    away[L] += (1000, -1000)
    gone, gsums = R.hold(win, offs, R.make_track(away), mask, 2, 12)
    others = [t for t in range(T) if t != L]
    assert (gone[others] == out[others]).all() and (gsums[others] == sums[others]).all() and (gone[L] == win[L]).all()
    # ... or as a frame of other content (nothing of it is read)
    other = win.copy()
    other[L] = 255 - other[L]
    out2, sums2 = R.hold(other, offs, R.make_track(off, lost=(L,)), mask, 2, 12)
    assert (out2[others] == out[others]).all() and (sums2[others] == sums[others]).all() and (out2[L] == other[L]).all()
    # every frame lost: the identity
    none, nsums = R.hold(win, offs, R.make_track(off, lost=range(T)), mask, 4, 255)
    assert (none == win).all() and (nsums[:, 2] == h * w).all()


def test_identity_settings_and_a_track_beyond_the_window():
    off = R.walk(9, 2)
    win, offs, mask = _panned_clip(9, off)
    T, h, w, _ = win.shape
    for radius, tol in ((0, 12), (2, 0), (0, 0)):
        out, sums = R.hold(win, offs, R.make_track(off), mask, radius, tol)
        assert (out == win).all() and not sums[:, [1, 3, 4, 5, 7, 9, 10, 11]].any()
        assert (sums[:, 2] == h * w).all() or tol == 0 and radius > 0                               # tol = 0 still accepts equal samples
    far = np.stack([np.arange(T) * (w + 1), np.arange(T) * -(h + 1)], 1)                            # steps that exceed the window: no overlap
    out, sums = R.hold(win, np.tile([[3, 5]], (T, 1)), R.make_track(far), mask, 4, 255)
    assert (out == win).all() and (sums[:, 2] == h * w).all()
    wild = R.make_track(far * (1 << 23))                                                            # any int32 content is data
    out, sums = R.hold(win, offs, wild, mask, 4, 255)
    assert (out == win).all()


# ---- the rule on the synthetic pan: a failure here means the rule is wrong, not the kernel -------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rule_removes_flicker_along_the_pan(seed):
    """The statistics of test_deflicker_cpu.test_rule_removes_flicker under a pan of 2 .. 5 px in x and -2 .. 2 px in y per frame, radius 2,
    tol 16, the full frame as the window.  Measured: DESIGN.md section 19."""
    x, off = R.pan_flicker_clip(seed)
    assert x.min() >= 33 and x.max() <= 223 and x.shape == (R.T, R.H, R.W, 3)
    assert (np.diff(off[:, 0]) >= 2).all() and (np.diff(off[:, 0]) <= 5).all() and (np.abs(np.diff(off[:, 1])) <= 2).all()
    zero, mask = np.zeros((R.T, 2), np.int32), np.zeros((R.T, R.H, R.W), np.uint8)
    out, sums = R.hold(x.astype(np.uint8), zero, R.make_track(off), mask, 2, 16)
    fixed, fsums = R0.hold(x.astype(np.uint8), zero, mask, 2, 16)
    before, after = R.difference_along(x, off), R.difference_along(out, off)
    n, n_fixed = R.samples_per_pixel(sums), R.samples_per_pixel(fsums)
    print(f"seed {seed}: mean |frame difference| along the motion {before:.3f} -> {after:.3f}, a factor of {before / after:.2f}; accepted samples "
          f"per pixel {n:.3f} tracked, {n_fixed:.3f} at a fixed place ({100 * fsums[:, 1].sum() / fsums[:, 0].sum():.1f} % of the pixels changed)")
    assert before / after >= 3.0
    assert n >= 3.5
    assert n_fixed <= 1.1
    assert np.abs(out.astype(int) - x).max() <= 16


def test_rule_with_the_tracker_in_the_loop():
    """The same three assertions with the track taken from the tracker's restatement on a pan with a crossing box and a screen-fixed logo,
    whose offsets it recovers exactly.  The clip's masks (box and logo) go in as mask2d and the statistics are taken over the unmasked pixels:
    the logo is the same byte at a fixed place in every frame, so at a fixed place every sample of it is accepted and along the motion none
    is; neither says anything about the background the stage is for."""
    frames, masks, off, clean, boxm, logom = A.pan_clip(T=12, H=96, W=128, logo=(40, 50, 60, 90))
    track = A.track_segment(frames, masks)
    assert (track[:, :2] == off).all() and (track[:, 3] == 1).all()
    T = len(frames)
    zero = np.zeros((T, 2), np.int32)
    out, sums = R.hold(frames, zero, track, masks, 2, 16)
    fixed, fsums = R0.hold(frames, zero, masks, 2, 16)
    free = masks == 0

    def along(x):                                                                                   # over the pixels unmasked in both frames
        total = count = 0
        for t in range(T - 1):
            dx, dy = int(off[t][0] - off[t + 1][0]), int(off[t][1] - off[t + 1][1])
            y0, y1, x0, x1 = max(0, -dy), min(96, 96 - dy), max(0, -dx), min(128, 128 - dx)
            both = free[t, y0:y1, x0:x1] & free[t + 1, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            d = np.abs(x[t + 1, y0 + dy:y1 + dy, x0 + dx:x1 + dx].astype(int) - x[t, y0:y1, x0:x1])[both]
            total, count = total + int(d.sum()), count + d.size
        return total / count

    per_pixel = lambda s: float((s[:, 2] - s[:, 8]).sum() / (s[:, 0] - s[:, 6]).sum())
    before, after = along(frames), along(out)
    print(f"tracker in the loop: mean |frame difference| along the motion {before:.3f} -> {after:.3f}, a factor of {before / after:.2f}; accepted "
          f"samples per unmasked pixel {per_pixel(sums):.3f} tracked, {per_pixel(fsums):.3f} at a fixed place")
    assert before / after >= 3.0
    assert per_pixel(sums) >= 3.5
    assert per_pixel(fsums) <= 1.1
    assert np.abs(out.astype(int) - frames).max() <= 16


# ---- the report ---------------------------------------------------------------------------------------------------------------------------
def test_report_over_spans():
    from videovanish_amd import infill
    a, b = R.make_track(R.walk(5, 1), lost=(3,)), DA.identity_track(4)
    a[:, 4:] = 0
    a[1, 4:7] = 300, 0, 100
    rep = infill.deflicker_align_report([(a, "tracked"), (b, "static")], [(2, 7), (9, 13)])
    assert infill.DeflickerAlignReport._fields == ("off", "key", "tracked", "residual", "path", "segments")
    assert rep.path == ("tracked", "static") and rep.segments == ((2, 7), (9, 13))
    assert (rep.off[0] == a[:, :2]).all() and rep.off[1].shape == (4, 2) and rep.tracked[0].tolist() == [True, True, True, False, True]
    assert rep.residual[0].tolist() == [0.0, 3.0, 0.0, 0.0, 0.0] and rep.key[1].tolist() == [0] * 4
    empty = infill.deflicker_align_report([], [])
    assert empty.path == () and empty.off == () and empty.segments == ()


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_precedence_and_the_need_for_deflicker(monkeypatch):
    import inspect

    import diffuerase
    monkeypatch.delenv("VV_DEFLICKER", raising=False)
    monkeypatch.delenv("VV_DEFLICKER_ALIGN", raising=False)
    try:
        diffuerase.configure()
        assert diffuerase.deflicker_align_config() is None
        monkeypatch.setenv("VV_DEFLICKER_ALIGN", "radius=1")
        assert diffuerase.deflicker_align_config() == PlateAlignConfig(radius=1)
        diffuerase.configure(deflicker_align="levels=2")
        assert diffuerase.deflicker_align_config() == PlateAlignConfig(levels=2) and diffuerase.deflicker_align_config("on") == PlateAlignConfig()
        assert diffuerase.deflicker_align_config("off") is None and diffuerase.deflicker_align_config(False) is None
        diffuerase.configure(deflicker_align="off")
        assert diffuerase.deflicker_align_config() is None                                         # configure("off") beats the environment
        diffuerase.configure()
        assert diffuerase.deflicker_align_config() == PlateAlignConfig(radius=1)
        with pytest.raises(ValueError, match="deflicker_align must be"):
            diffuerase.configure(deflicker_align="sometimes")
        f = [np.zeros((8, 8, 3), np.uint8)] * 2
        need = r"deflicker_align= \(aligned inpaint deflicker\) needs deflicker= \(inpaint deflicker\)"
        for kw in (dict(deflicker_align="on"), dict(), dict(deflicker_align="on", deflicker="off")):    # the second: from the environment
            with pytest.raises(ValueError, match=need):
                diffuerase.run_infill_on_frames(f, f, **kw)
        monkeypatch.setenv("VV_DEFLICKER", "on")
        with pytest.raises(ValueError, match=need):
            diffuerase.run_infill_on_frames(f, f, deflicker=False)                                  # "off" wins over the environment
        with pytest.raises(ValueError, match="cannot be combined with compat_reference_early_return=True"):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)               # past that check: deflicker comes from the environment
        with pytest.raises(ValueError, match="1 <= radius <= 8"):
            diffuerase.run_infill_on_frames(f, f, deflicker_align="radius=9")
        diffuerase.last_deflicker_align = "stale"
        with pytest.raises(ValueError):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)
        assert diffuerase.last_deflicker_align is None                                              # reset at the start of every call
    finally:
        diffuerase.configure()
    for fn in (diffuerase.run_infill_on_frames, diffuerase.configure):
        names = list(inspect.signature(fn).parameters)
        p = inspect.signature(fn).parameters["deflicker_align"]
        assert names[names.index("deflicker") + 1] == "deflicker_align" and names[-1] == "plate_fill"
        assert p.default is None and (fn is diffuerase.configure or p.kind is inspect.Parameter.KEYWORD_ONLY)


def test_cli_deflicker_align_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
    import diffuerase
    from videovanish_amd import infill
    calls = []
    videos = {"mask.mkv": [np.zeros((16, 24, 3), np.uint8)] * 7}
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda path, start=0, max_frames=-1: ([f.copy() for f in videos[path]], 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    walked = R.make_track(np.array([[0, 0], [3, -1], [7, -2], [7, -2]]), lost=(3,))
    report = infill.deflicker_align_report([(walked, "tracked"), (DA.identity_track(3), "static")], [(0, 4), (4, 7)])

    def fake(frames, masks, **kw):
        calls.append(kw)
        diffuerase.last_deflicker = None
        diffuerase.last_deflicker_align = report if "deflicker_align" in kw else None
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 7
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    for value in ("on", "levels=2,radius=8"):
        monkeypatch.setattr(sys, "argv", argv + ["--deflicker", "on", "--deflicker-align", value])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "deflicker": "on", "deflicker_align": value}
        assert capsys.readouterr().out == "deflicker align: 2 clip calls (1 tracked, 1 static), 1 of 7 frames lost, largest |offset| 7 px\n"
    monkeypatch.setattr(sys, "argv", argv + ["--deflicker", "on"])
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None, "deflicker": "on"} and capsys.readouterr().out == ""
    for bad in ("off", "yes", "radius=9", "tol=3"):
        monkeypatch.setattr(sys, "argv", argv + ["--deflicker-align", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_deflicker_align", None)
    assert DeflickerConfig() is not None
