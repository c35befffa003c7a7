"""Inpaint deflicker on the CPU: the settings, the binding of include/vvflicker.h, the product sources, the arithmetic and the invariants of the
restatement (tests/deflicker_ref.py), the rule on synthetic clips, the report, configuration and CLI."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abiref  # noqa: E402
import deflicker_ref as R  # noqa: E402

from videovanish_amd import deflicker as D  # noqa: E402
from videovanish_amd.deflicker import DeflickerConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_spellings_and_config():
    assert D.SPELLINGS == ("on",)
    for off in (None, False, "off", "none", "", " OFF "):
        assert D.as_config(off) is None
    d = DeflickerConfig()
    assert D.as_config("on") == D.as_config(" On ") == D.as_config(True) == d
    assert (d.radius, d.tol) == (2, 12) == (R.DEFAULTS["radius"], R.DEFAULTS["tol"])
    assert D.as_config("radius=2,tol=12") == d
    assert D.as_config(" tol = 0 , radius = 4 ") == DeflickerConfig(radius=4, tol=0) and D.as_config("radius=0") == DeflickerConfig(radius=0)
    assert D.as_config("tol=255") == DeflickerConfig(tol=255)
    cfg = DeflickerConfig(radius=1)
    assert D.as_config(cfg) is cfg
    for bad in ("yes", "median", "radius", "radius=", "radius=x", "radius=-1", "radius=1.5", "radius=1,radius=2", "size=3", "radius=1;tol=2", "radius=5",
                "tol=256", "on,radius=1", "radius=1,", 3, 1.0, ("on",)):
        with pytest.raises(ValueError):
            D.as_config(bad)
    for kw in (dict(radius=-1), dict(radius=5), dict(tol=-1), dict(tol=256), dict(radius=2.0), dict(tol=True), dict(radius="2")):
        with pytest.raises(ValueError):
            DeflickerConfig(**kw)


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_vvflicker_header():
    """flicker_hip.SIGNATURES declares every function of include/vvflicker.h with the header's types, flicker_hip.lib() has applied it, the version
    and the limits agree in the header, the binding and the settings (abiref.check_binding; test_abi_cpu.py: no name could be taken for
    another part's), and arguments are refused before anything touches a device."""
    from videovanish_amd import flicker_hip
    loaded, define = abiref.check_binding(flicker_hip, 4)
    assert define("VVF_ABI_VERSION") == 1
    limits = (define("VVF_MAX_RADIUS"), define("VVF_MAX_T"), define("VVF_SLAB"))
    assert limits == (flicker_hip.MAX_RADIUS, flicker_hip.MAX_T, flicker_hip.SLAB) == (4, 65535, 16)
    assert (D.MAX_RADIUS, D.MAX_T, D.MAX_TOL, D.NSUM) == (4, 65535, 255, 12) == (flicker_hip.MAX_RADIUS, flicker_hip.MAX_T, 255, flicker_hip.NSUM)
    assert R.NSUM == D.NSUM
    # refusals: nothing is launched, the message names the function
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    wp = lambda *v: loaded.vvf_window_pixels(a, *v, a + 32, None)                                     # T, Hm, Wm, h, w
    assert [loaded.vvf_window_pixels(None, 2, 8, 8, 8, 8, a, None), loaded.vvf_window_pixels(a, 2, 8, 8, 8, 8, None, None), wp(0, 8, 8, 8, 8),
            wp(2, 0, 8, 8, 8), wp(2, 8, 8, 8, -1)] == [-1] * 5
    assert b"vvf_window_pixels" in loaded.vvf_last_error()
    assert [wp(65536, 8, 8, 8, 8), wp(2, 8, 8, 1 << 16, 1 << 15), wp(2, 1 << 16, 1 << 15, 8, 8)] == [-2] * 3 and b"vvf_window_pixels" in loaded.vvf_last_error()
    hold = lambda *v, out=a + 32: loaded.vvf_hold(a, a, a, *v, out, a, None)                          # T, H0, W0, h, w, radius, tol, fixed
    assert [loaded.vvf_hold(None, a, a, 2, 8, 8, 8, 8, 1, 1, 1, a + 32, a, None), loaded.vvf_hold(a, None, a, 2, 8, 8, 8, 8, 1, 1, 1, a + 32, a, None),
            loaded.vvf_hold(a, a, None, 2, 8, 8, 8, 8, 1, 1, 1, a + 32, a, None), loaded.vvf_hold(a, a, a, 2, 8, 8, 8, 8, 1, 1, 1, a + 32, None, None),
            hold(0, 8, 8, 8, 8, 1, 1, 1), hold(2, 8, 8, 9, 8, 1, 1, 1), hold(2, 8, 8, 8, 9, 1, 1, 0), hold(2, 8, 8, 8, 8, -1, 1, 1),
            hold(2, 8, 8, 8, 8, 1, -1, 1), hold(2, 8, 8, 8, 8, 1, 1, 1, out=a), hold(2, 8, 8, 8, 8, 1, 1, 1, out=None)] == [-1] * 11
    assert b"vvf_hold" in loaded.vvf_last_error()
    assert [hold(2, 8, 8, 8, 8, 5, 1, 1), hold(2, 8, 8, 8, 8, 1, 256, 0), hold(65536, 8, 8, 8, 8, 1, 1, 1), hold(2, 1 << 16, 1 << 15, 1 << 16, 1 << 15, 1, 1, 1)] == [-2] * 4
    assert b"vvf_hold" in loaded.vvf_last_error()
    with pytest.raises(ctypes.ArgumentError):
        loaded.vvf_hold(a, a, a, 2.0, 8, 8, 8, 8, 1, 1, 1, a + 32, a, None)
    import torch
    f, z = torch.zeros((2, 8, 8, 3), dtype=torch.uint8), torch.zeros((2, 8, 8), dtype=torch.uint8)
    o = torch.zeros((2, 2), dtype=torch.int32)
    for call in (lambda: flicker_hip.window_pixels(f, 16, 16), lambda: flicker_hip.window_pixels(f, 8, 8), lambda: flicker_hip.hold(f, o, z, 2, 12, fixed=True)):
        with pytest.raises(RuntimeError):
            call()                                                                                   # no CPU fallback


def test_product_sources_of_the_feature():
    """vv_flicker is in the one build recipe with its header among the dependencies and reads no environment; the settings import no torch and no
    oracle; importing the drop-in resolves no vvf_ symbol."""
    abiref.check_sources("vv_flicker", "vvflicker.h", "deflicker")
    code = ("import sys, diffuerase; from videovanish_amd import flicker_hip, hip, infill; assert flicker_hip.PART.dll is None and hip.CORE.dll is None; "
            "assert diffuerase.deflicker_config() is None and diffuerase.last_deflicker is None")
    env = {k: v for k, v in os.environ.items() if k != "VV_DEFLICKER"}
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)
    code = "import sys, videovanish_amd.deflicker as d; assert 'torch' not in sys.modules and d.as_config('on').tol == 12"
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------------
def test_integer_division_is_the_rounded_mean():
    """(2 S + n) / (2 n) == floor(S / n + 0.5) for every n <= 9 and S <= 255 n; and the 20-bit reciprocal the kernels multiply by is exact there."""
    from fractions import Fraction
    for n in range(1, 10):
        S = np.arange(0, 255 * n + 1, dtype=np.int64)
        got = (2 * S + n) // (2 * n)
        want = np.array([(Fraction(int(s), n) + Fraction(1, 2)).__floor__() for s in S])
        assert (got == want).all(), n
        assert (((2 * S + n) * ((1 << 20) // (2 * n) + 1)) >> 20 == got).all() and int((2 * S[-1] + n) * ((1 << 20) // (2 * n) + 1)) < 1 << 32, n


# ---- invariants of the restatement --------------------------------------------------------------------------------------------------------
def _random_clip(seed, T=9, h=12, w=16, H0=20, W0=24, moving=True):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H0, W0, 3))                                                        # one background, fixed in the frame
    offsets = np.stack([rng.integers(0, H0 - h + 1, T), rng.integers(0, W0 - w + 1, T)], 1) if moving else np.tile([[3, 5]], (T, 1))
    win = np.stack([base[oy:oy + h, ox:ox + w] for oy, ox in offsets]) + rng.integers(-9, 10, (T, h, w, 3))
    win[T // 2:, :, w // 2:] += 60                                                                  # a real change
    mask = (rng.random((T, H0, W0)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (T, H0, W0)).astype(np.uint8)
    return np.clip(win, 0, 255).astype(np.uint8), offsets.astype(np.int32), mask


@pytest.mark.parametrize("moving", [False, True])
def test_restatement_invariants(moving):
    win, offs, mask = _random_clip(5, moving=moving)
    T, h, w, _ = win.shape
    for radius, tol in ((1, 4), (2, 12), (4, 255)):
        out, sums = R.hold(win, offs, mask, radius, tol)
        d = np.abs(out.astype(int) - win.astype(int))
        assert d.max() <= tol and d.any()                                                          # no byte moves more than tol
        assert (sums[:, 0] == h * w).all() and (sums[:, 1] == d.any(-1).reshape(T, -1).sum(1)).all() and (sums[:, 3:6] == d.reshape(T, -1, 3).sum(1)).all()
        assert (sums[:, 2] >= h * w).all() and (sums[:, 2] <= h * w * (2 * radius + 1)).all()
        assert (sums[:, 6:] <= sums[:, :6]).all() and sums[:, 6].any() and (sums[:, 6] < h * w).all()
    for radius, tol in ((0, 12), (2, 0), (0, 0)):                                                   # the identity
        out, sums = R.hold(win, offs, mask, radius, tol)
        assert (out == win).all() and not sums[:, [1, 3, 4, 5, 7, 9, 10, 11]].any()
        assert (sums[:, 2] == h * w).all() or tol == 0 and radius > 0                                # tol = 0 still accepts equal samples
    still = np.repeat(win[:1], T, 0)
    out, sums = R.hold(still, np.repeat(offs[:1], T, 0), mask, 2, 12)                               # constant in time: unchanged, every sample accepted
    assert (out == still).all() and sums[2, 2] == 5 * h * w and sums[0, 2] == 3 * h * w
    # nothing crosses the ends of a clip call: two clips filtered apart are the two halves filtered one by one
    a, b = R.hold(win[:4], offs[:4], mask[:4], 2, 12), R.hold(win[4:], offs[4:], mask[4:], 2, 12)
    whole = R.hold(win, offs, mask, 2, 12)
    assert (np.concatenate([a[0], b[0]])[[0, 1, 6, 7, 8]] == whole[0][[0, 1, 6, 7, 8]]).all()      # frames more than `radius` from the joint agree
    assert (np.concatenate([a[0], b[0]]) != whole[0]).any()                                         # and the joint itself is a border
    both = R.hold(np.concatenate([win[:4], win[:4]]), np.concatenate([offs[:4], offs[:4]]), np.concatenate([mask[:4], mask[:4]]), 0, 12)
    assert (both[1][:4] == both[1][4:]).all() and (np.concatenate([a[1], b[1]])[[0, 1, 6, 7, 8]] == whole[1][[0, 1, 6, 7, 8]]).all()


def test_a_window_that_moves_reads_its_neighbours_at_the_frames_place():
    """follow windows: the sample of frame s is taken at the same FRAME pixel, and a frame whose window does not hold that pixel gives none."""
    T, h, w = 3, 4, 4
    win = np.zeros((T, h, w, 3), np.uint8)
    win[0], win[1], win[2] = 100, 104, 108
    offs = np.array([[0, 0], [0, 2], [4, 4]], np.int32)                                             # frame 2's window shares no pixel with the others
    out, sums = R.hold(win, offs, np.zeros((T, 8, 8), np.uint8), 2, 12)
    assert (out[0][:, 2:] == 102).all() and (out[0][:, :2] == 100).all()                            # columns 2, 3 of frame 0 are columns 0, 1 of frame 1
    assert (out[1][:, :2] == 102).all() and (out[1][:, 2:] == 104).all() and (out[2] == 108).all()
    assert sums[:, 2].tolist() == [16 + 8, 16 + 8, 16]


# ---- the rule on synthetic clips: a failure here means the rule is wrong, not the kernel --------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rule_removes_flicker(seed):
    x = R.flicker_clip(seed)
    assert x.min() >= 33 and x.max() <= 223 and x.shape == (R.T, R.H, R.W, 3)
    out, sums = R.hold(x.astype(np.uint8), np.zeros((R.T, 2), np.int32), np.zeros((R.T, R.H, R.W), np.uint8), 2, 16)
    before, after = R.temporal_difference(x), R.temporal_difference(out)
    print(f"seed {seed}: mean |frame difference| {before:.3f} -> {after:.3f}, a factor of {before / after:.2f}")
    assert before / after >= 3.0
    assert (sums[2:-2, 2] == 5 * R.H * R.W).all()                                                   # |noise| + |pump| differences <= 14 < 16: every interior sample is accepted
    assert np.abs(out.astype(int) - x).max() <= 16


def test_rule_leaves_a_moving_edge():
    x, clean = R.edge_clip(0)
    out, _ = R.hold(x.astype(np.uint8), np.zeros((R.T, 2), np.int32), np.zeros((R.T, R.H, R.W), np.uint8), 2, 16)
    err_in, err_out = np.abs(x - clean), np.abs(out.astype(int) - clean)
    print(f"moving edge: max |out - clean| {err_out.max()}, mean {err_out.mean():.3f} against {err_in.mean():.3f} of the input")
    assert err_out.max() <= 3                                                                       # the noise bound: no ghost of the edge
    assert err_out.mean() < err_in.mean()


# ---- the report ---------------------------------------------------------------------------------------------------------------------------
def test_fit_and_report():
    from videovanish_amd import infill
    win, offs, mask = _random_clip(7)
    T, h, w, _ = win.shape
    _, sums = R.hold(win, offs, mask, 2, 12)
    f = D.fit(sums)
    assert f.n.tolist() == [h * w] * T and (f.changed == sums[:, 1]).all() and (f.n_mask == sums[:, 6]).all() and (f.changed_mask == sums[:, 7]).all()
    assert np.allclose(f.samples, sums[:, 2] / (h * w)) and np.allclose(f.shift, sums[:, 3:6] / (h * w)) and f.shift.shape == (T, 3)
    assert np.allclose(f.samples_mask, sums[:, 8] / sums[:, 6]) and np.allclose(f.shift_mask, sums[:, 9:12] / sums[:, 6:7])
    z = D.fit(np.zeros((3, 12), np.int64))
    assert all(not v.any() for v in z) and z.samples.dtype == np.float64
    part = infill.DeflickerReport(*(v[None] for v in f))
    rep = infill.deflicker_report([part], [(2, 2 + T)], T + 5, K=2)
    assert infill.DeflickerReport._fields == D.DeflickerFit._fields
    assert rep.n.shape == rep.changed.shape == rep.samples.shape == rep.n_mask.shape == rep.changed_mask.shape == rep.samples_mask.shape == (2, T + 5)
    assert rep.shift.shape == rep.shift_mask.shape == (2, T + 5, 3) and rep.n.dtype == np.int64 and rep.samples.dtype == np.float64
    for whole, piece in zip(rep, f):
        assert (whole[0, 2:2 + T] == piece).all() and not whole[1].any() and not whole[0, :2].any() and not whole[0, 2 + T:].any()
    empty = infill.deflicker_report([], [], 4)
    assert empty.n.shape == (1, 4) and all(not v.any() for v in empty)


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_precedence_and_exclusion(monkeypatch):
    import inspect

    import diffuerase
    monkeypatch.delenv("VV_DEFLICKER", raising=False)
    try:
        diffuerase.configure()
        assert diffuerase.deflicker_config() is None
        monkeypatch.setenv("VV_DEFLICKER", "radius=1")
        assert diffuerase.deflicker_config() == DeflickerConfig(radius=1)
        diffuerase.configure(deflicker="tol=6")
        assert diffuerase.deflicker_config() == DeflickerConfig(tol=6) and diffuerase.deflicker_config("on") == DeflickerConfig()
        assert diffuerase.deflicker_config("off") is None and diffuerase.deflicker_config(False) is None
        diffuerase.configure(deflicker="off")
        assert diffuerase.deflicker_config() is None                                               # configure("off") beats the environment
        diffuerase.configure()
        assert diffuerase.deflicker_config() == DeflickerConfig(radius=1)
        with pytest.raises(ValueError):
            diffuerase.configure(deflicker="sometimes")
        f = [np.zeros((8, 8, 3), np.uint8)] * 2
        for kw in (dict(deflicker="on"), dict(deflicker=DeflickerConfig(radius=0)), dict()):      # the last: from the environment
            with pytest.raises(ValueError, match=r"deflicker= \(inpaint deflicker\) cannot be combined with compat_reference_early_return=True"):
                diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, **kw)
        with pytest.raises(ValueError, match="0 <= radius <= 4"):
            diffuerase.run_infill_on_frames(f, f, deflicker="radius=7")
        assert diffuerase.last_deflicker is None
    finally:
        diffuerase.configure()
    for fn in (diffuerase.run_infill_on_frames, diffuerase.configure):
        p = inspect.signature(fn).parameters["deflicker"]
        assert p.default is None and (fn is diffuerase.configure or p.kind is inspect.Parameter.KEYWORD_ONLY)


def test_cli_deflicker_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
    import diffuerase
    from videovanish_amd import infill
    calls = []
    videos = {"mask.mkv": [np.zeros((16, 24, 3), np.uint8)] * 3}
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda path, start=0, max_frames=-1: ([f.copy() for f in videos[path]], 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    sums = np.zeros((3, 12), np.int64)
    sums[0] = [384, 100, 1200, 96, 48, 192, 50, 40, 200, 50, 25, 100]
    sums[2] = [384, 10, 400, 10, 0, 0, 150, 0, 150, 0, 0, 0]

    def fake(frames, masks, **kw):
        calls.append(kw)
        diffuerase.last_deflicker = infill.DeflickerReport(*(v[None] for v in D.fit(sums))) if "deflicker" in kw else None
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 3
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    for value in ("on", "radius=4,tol=3"):
        monkeypatch.setattr(sys, "argv", argv + ["--deflicker", value])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "deflicker": value}
        assert capsys.readouterr().out == "deflicker: 2 of 3 frames changed, mean accepted samples inside the mask 1.75, largest mean |shift| 0.50\n"
    monkeypatch.setattr(sys, "argv", argv)
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None} and capsys.readouterr().out == ""
    for bad in ("off", "yes", "radius=5"):
        monkeypatch.setattr(sys, "argv", argv + ["--deflicker", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_deflicker", None)
