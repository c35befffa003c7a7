"""Seam tone matching on the CPU: the settings, the binding of include/vvtone.h, the properties of the fit over seeded draws of sums (the product's
host code against the restatement of tests/tonematch_ref.py, bit for bit in the tables), the restoration of known tone shifts on the reference
alone, configuration and CLI."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abiref  # noqa: E402
import tonematch_ref as R  # noqa: E402

from videovanish_amd import tonematch as M  # noqa: E402
from videovanish_amd.tonematch import ToneMatchConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_spellings_and_config():
    assert M.SPELLINGS == ("on", "affine", "offset")
    for off in (None, False, "off", "none", "", " OFF "):
        assert M.as_config(off) is None
    d = ToneMatchConfig()
    assert (d.mode, d.ring, d.smooth, d.max_gain, d.max_offset, d.min_count, d.min_var) == ("affine", 12, 2, 1.25, 32.0, 64, 4.0)
    assert M.as_config("on") == M.as_config(" On ") == M.as_config(True) == M.as_config("affine") == d
    assert M.as_config("offset") == M.as_config(" OFFSET ") == ToneMatchConfig(mode="offset")
    assert M.as_config("mode=offset,ring=8,smooth=0") == ToneMatchConfig(mode="offset", ring=8, smooth=0)
    assert M.as_config(" max_gain = 1.5 , min_var=0,max_offset=8,min_count=1 ") == ToneMatchConfig(max_gain=1.5, min_var=0.0, max_offset=8.0, min_count=1)
    assert M.as_config("ring=32,smooth=16,max_gain=2,max_offset=128") == ToneMatchConfig(ring=32, smooth=16, max_gain=2.0, max_offset=128.0)
    cfg = ToneMatchConfig(ring=4)
    assert M.as_config(cfg) is cfg
    with pytest.raises(Exception):
        cfg.ring = 5                                                                                 # frozen
    for bad in ("yes", "static", "ring", "ring=", "ring=x", "ring=-3", "ring=1.5", "ring=3,ring=4", "size=3", "ring=3;smooth=1", "ring=0", "ring=33",
                "smooth=17", "max_gain=0.9", "max_gain=2.5", "max_offset=-1", "max_offset=129", "min_count=0", "min_var=-1", "min_var=nan", "mode=gamma",
                "mode=", "on,ring=3", "ring=3,", "max_gain=inf", 3, 1.0, ("on",)):
        with pytest.raises(ValueError):
            M.as_config(bad)
    for kw in (dict(mode="gamma"), dict(mode=None), dict(ring=0), dict(ring=33), dict(ring=4.0), dict(ring=True), dict(smooth=-1), dict(smooth=17),
               dict(smooth="2"), dict(max_gain=0.99), dict(max_gain=2.01), dict(max_gain="1"), dict(max_offset=-0.5), dict(max_offset=128.5),
               dict(min_count=0), dict(min_count=1.5), dict(min_var=-0.1), dict(min_var=float("nan")), dict(max_offset=None)):
        with pytest.raises(ValueError):
            ToneMatchConfig(**kw)
    ToneMatchConfig(ring=1, smooth=0, max_gain=1.0, max_offset=0, min_count=1, min_var=0)             # the limits themselves are inside
    assert "build-defined" in ToneMatchConfig.__doc__


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_vvtone_header():
    """tone_hip.SIGNATURES declares every function of include/vvtone.h with the header's types, tone_hip.lib() has applied it, the version and the
    limit agree (abiref.check_binding; test_abi_cpu.py: no name could be taken for another part's), and the arguments are validated before any
    device work."""
    from videovanish_amd import tone_hip
    loaded, define = abiref.check_binding(tone_hip, 4)
    assert define("VVT_ABI_VERSION") == 1
    assert define("VVT_MAX_RING") == tone_hip.MAX_RING == M.MAX_RING == 32
    # arguments are validated before anything touches a device: -1 null pointers and sizes, -2 the ring and the feather
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    stats = lambda patch=a, orig=a, mask=a, offs=a, sums=a, Hm=4, Wm=4, T=1, H0=8, W0=8, h=4, w=4, ring=4: loaded.vvt_ring_stats(
        patch, Hm, Wm, orig, mask, offs, T, H0, W0, h, w, ring, sums, None)
    paste = lambda patch=a, orig=a, mask=a, offs=a, lut=a, out=a, Hm=4, Wm=4, T=1, H0=8, W0=8, h=4, w=4, feather=3.0: loaded.vvt_paste_lut_composite(
        patch, Hm, Wm, orig, mask, offs, lut, T, H0, W0, h, w, feather, out, None)
    for kw in (dict(patch=None), dict(orig=None), dict(mask=None), dict(offs=None), dict(sums=None), dict(Hm=0), dict(Wm=-1), dict(T=0), dict(H0=0),
               dict(W0=0), dict(h=0), dict(w=0), dict(h=9), dict(w=9)):
        assert stats(**kw) == -1 and b"vvt_ring_stats" in loaded.vvt_last_error(), kw
    for ring in (0, -1, 33, 1000):
        assert stats(ring=ring) == -2 and b"vvt_ring_stats" in loaded.vvt_last_error(), ring
    assert stats(ring=0, T=0) == -1                                                                  # a bad argument before an unsupported one
    for kw in (dict(patch=None), dict(orig=None), dict(mask=None), dict(offs=None), dict(lut=None), dict(out=None), dict(Hm=0), dict(T=-2), dict(H0=0),
               dict(h=0), dict(w=9), dict(mask=None, feather=0.0)):
        assert paste(**kw) == -1 and b"vvt_paste_lut_composite" in loaded.vvt_last_error(), kw
    assert paste(feather=64.5) == -2 and b"vvt_paste_lut_composite" in loaded.vvt_last_error()
    with pytest.raises(ctypes.ArgumentError):
        loaded.vvt_ring_stats(a, 4.0, 4, a, a, a, 1, 8, 8, 4, 4, 4, a, None)
    import torch
    z = torch.zeros((2, 4, 4, 3), dtype=torch.uint8)
    offs, lut = torch.zeros((2, 2), dtype=torch.int32), torch.zeros((2, 3, 256), dtype=torch.uint8)
    for call in (lambda: tone_hip.ring_stats(z, z, z[..., 0].contiguous(), offs, 4, 4, 2),
                 lambda: tone_hip.paste_lut_composite(z, z, z[..., 0].contiguous(), offs, lut, 4, 4, 3.0)):
        with pytest.raises(RuntimeError):
            call()                                                                                   # no CPU fallback


def test_product_sources_of_the_feature():
    """vv_tone is in the one build recipe with its header among the dependencies and reads no environment; the settings import no torch; importing
    the drop-in resolves no symbol of the feature."""
    abiref.check_sources("vv_tone", "vvtone.h", "tonematch")
    code = ("import diffuerase; from videovanish_amd import tone_hip, hip, tonematch; assert tone_hip.PART.dll is None and hip.CORE.dll is None; "
            "assert diffuerase.last_tone_match is None")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ---- the fit ------------------------------------------------------------------------------------------------------------------------------
def _sums_of(x, y):
    x, y = x.astype(np.int64).reshape(-1, 3), y.astype(np.int64).reshape(-1, 3)
    return np.array([len(x), *x.sum(0), *y.sum(0), *(x * x).sum(0), *(x * y).sum(0), *(y * y).sum(0)], np.int64) if len(x) else np.zeros(16, np.int64)


def _draw(rng, k):
    """One (sums [T,16], config, kind): rings of every size (empty, below min_count, large), x flat or spread, y equal to x, an affine image of x
    inside or outside the clamps, or unrelated."""
    T = int(rng.integers(1, 9))
    kind = ("equal", "affine", "steep", "far", "flat", "noise")[k % 6]
    cfg = ToneMatchConfig(mode="offset" if k % 5 == 4 else "affine", ring=12, smooth=int(rng.choice([0, 0, 1, 2, 5])),
                          max_gain=float(rng.choice([1.0, 1.1, 1.25, 2.0])), max_offset=float(rng.choice([0, 4, 32, 128])),
                          min_count=int(rng.choice([1, 64, 300])), min_var=float(rng.choice([0, 4, 100])))
    rows = []
    for t in range(T):
        n = int(rng.choice([0, 0, 1, 20, 70, 400, 3000]))
        x = rng.integers(0, 256, (n, 3)) if kind != "flat" else rng.integers(100, 103, (n, 3))
        if kind == "equal":
            y = x
        elif kind == "affine":
            y = np.clip(np.rint(rng.uniform(0.9, 1.1) * x + rng.uniform(-10, 10)), 0, 255)
        elif kind == "steep":
            y = np.clip(np.rint(rng.choice([0.3, 2.5]) * x + rng.uniform(-5, 5)), 0, 255)
        elif kind == "far":
            y = np.clip(x + rng.choice([-150, 150]), 0, 255)
        elif kind == "flat":
            y = x + int(rng.integers(-8, 9))
        else:
            y = rng.integers(0, 256, (n, 3))
        rows.append(_sums_of(x, y))
    return np.stack(rows), cfg, kind


def test_fit_properties_over_random_draws():
    rng = np.random.default_rng(20251018)
    seen = dict.fromkeys(("identity_equal", "low_count", "own_empty", "fitted", "gain_clamped", "offset_clamped", "offset_mode", "low_var", "pooled",
                          "smooth0", "changed_table"), 0)
    ident = np.broadcast_to(np.arange(256, dtype=np.uint8), (3, 256))
    for k in range(360):
        s, cfg, kind = _draw(rng, k)
        T = len(s)
        f = M.fit(s, cfg)
        lut = M.tables(f.gain, f.offset)
        assert f.n.dtype == np.int64 and (f.n == s[:, 0]).all() and f.gain.shape == f.offset.shape == f.rms_before.shape == f.rms_after.shape == (T, 3)
        assert lut.dtype == np.uint8 and lut.shape == (T, 3, 256)
        # the product's fit equals the reference's: gains and offsets as numbers, the tables bit for bit, the residuals closely
        kw = dict(mode=cfg.mode, smooth=cfg.smooth, max_gain=cfg.max_gain, max_offset=cfg.max_offset, min_count=cfg.min_count, min_var=cfg.min_var)
        g, o = R.fit(s, **kw)
        assert (f.gain == g).all() and (f.offset == o).all() and (lut == R.tables(g, o)).all(), k
        rb, ra = R.rms(s, g, o)
        assert np.allclose(f.rms_before, rb, rtol=1e-9, atol=1e-6) and np.allclose(f.rms_after, ra, rtol=1e-9, atol=1e-6)
        assert (f.rms_before[s[:, 0] == 0] == 0).all() and (f.rms_after[s[:, 0] == 0] == 0).all()
        # the clamps, the monotone tables
        assert (f.gain >= 1 / cfg.max_gain).all() and (f.gain <= cfg.max_gain).all() and (np.abs(f.offset) <= cfg.max_offset).all()
        assert (np.diff(lut.astype(int), axis=-1) >= 0).all()
        pooled = M.pool(s, cfg.smooth)
        assert (pooled == np.stack([s[max(0, t - cfg.smooth):t + cfg.smooth + 1].sum(0) for t in range(T)])).all()
        skip = (s[:, 0] == 0) | (pooled[:, 0] < cfg.min_count)
        assert (f.gain[skip] == 1.0).all() and (f.offset[skip] == 0.0).all() and (lut[skip] == ident).all()
        seen["own_empty"] += bool((s[:, 0] == 0).any() and (pooled[s[:, 0] == 0, 0] >= cfg.min_count).any())
        seen["low_count"] += bool(((s[:, 0] > 0) & (pooled[:, 0] < cfg.min_count)).any())
        if kind == "equal":                                                                          # x == y on the ring: exactly the identity
            assert (f.gain == 1.0).all() and (f.offset == 0.0).all() and (lut == ident).all() and (f.rms_before == 0).all()
            seen["identity_equal"] += bool((~skip).any())
        if cfg.mode == "offset":
            assert (f.gain == 1.0).all()
            seen["offset_mode"] += bool((~skip).any() and (f.offset != 0).any())
        # pooling equals fitting the summed sums: frame t's row is the fit of one frame holding the pooled sums
        for t in np.nonzero(~skip)[0]:
            one = M.fit(pooled[t:t + 1], ToneMatchConfig(**{**kw, "smooth": 0}))
            assert (one.gain[0] == f.gain[t]).all() and (one.offset[0] == f.offset[t]).all()
        if cfg.smooth == 0:                                                                          # only the own frame: each row fitted alone
            for t in range(T):
                one = M.fit(s[t:t + 1], cfg)
                assert (one.gain[0] == f.gain[t]).all() and (one.offset[0] == f.offset[t]).all() and (one.rms_after[0] == f.rms_after[t]).all()
            seen["smooth0"] += bool((~skip).any())
        else:
            seen["pooled"] += bool((~skip).any() and T > 1 and (pooled[~skip] != s[~skip]).any())
        live = ~skip
        if live.any() and cfg.mode == "affine":
            n = pooled[live, :1].astype(float)
            vx = pooled[live, 7:10] / n - (pooled[live, 1:4] / n) ** 2
            seen["low_var"] += bool((vx < cfg.min_var).any())
            assert (f.gain[live][vx < cfg.min_var] == 1.0).all()
            seen["gain_clamped"] += bool(((f.gain[live] == cfg.max_gain) | (f.gain[live] == 1 / cfg.max_gain))[vx >= cfg.min_var].any() and cfg.max_gain > 1)
            seen["fitted"] += bool(((f.gain[live] > 1 / cfg.max_gain) & (f.gain[live] < cfg.max_gain) & (f.gain[live] != 1.0)).any())
        seen["offset_clamped"] += bool(live.any() and (np.abs(f.offset[live]) == cfg.max_offset).any() and cfg.max_offset > 0)
        seen["changed_table"] += bool((lut != ident).any())
    assert all(v >= 10 for v in seen.values()), seen


def test_tables_round_half_to_even_and_clip():
    lut = M.tables(np.array([[1.0, 0.5, 2.0]]), np.array([[0.5, 0.0, -100.0]]))
    assert lut[0, 0, :4].tolist() == [0, 2, 2, 4] and lut[0, 0, 255] == 255                           # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4
    assert lut[0, 1, :6].tolist() == [0, 0, 1, 2, 2, 2] and lut[0, 2, 50] == 0 and lut[0, 2, 51] == 2 and lut[0, 2, 200] == 255
    assert (M.tables(np.ones((2, 3)), np.zeros((2, 3))) == np.arange(256)).all()


# ---- restoration, on the reference alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", R.RESTORE_CASES)
def test_reference_restores_a_known_tone_shift(a, b):
    """x = clip(rint(a orig + b)) on smooth textures: the table fitted on the ring takes x back to within one level of orig everywhere, exactly
    for the pure offset; before the table the error is at least 6 levels."""
    orig, x, mask = R.restoration_clip(a, b)
    T, H, W = mask.shape
    assert orig.min() >= 20 and orig.max() <= 220 and mask[0].sum() == 255 * 30 * 50
    offs = np.zeros((T, 2), np.int32)
    s = R.sums(x, orig, mask, offs, H, W, 12)
    print("ring pixels per frame:", s[:, 0].tolist())
    assert (s[:, 0] > 2000).all()
    gain, offset = R.fit(s, mode="affine", smooth=2, max_gain=1.25, max_offset=32.0)
    lut = R.tables(gain, offset)
    out = np.stack([np.stack([lut[t, c][x[t, ..., c]] for c in range(3)], -1) for t in range(T)])
    before = np.abs(x.astype(int) - orig.astype(int)).max()
    after = np.abs(out.astype(int) - orig.astype(int)).max()
    print(f"a = {a}, b = {b}: gain {gain[0].round(4).tolist()}, offset {offset[0].round(3).tolist()}, worst error {before} -> {after}")
    assert before >= 6
    assert after <= 1 and (after == 0 or (a, b) != (1.0, 6))
    # the product's host code gives the same tables from the same sums
    f = M.fit(s, ToneMatchConfig())
    assert (M.tables(f.gain, f.offset) == lut).all() and (f.rms_after < f.rms_before).all() and (f.rms_after < 0.6).all()


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_precedence_argument_configure_environment(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_TONE_MATCH", raising=False)
    try:
        diffuerase.configure()
        assert diffuerase.tone_match_config() is None
        monkeypatch.setenv("VV_TONE_MATCH", "ring=9")
        assert diffuerase.tone_match_config() == ToneMatchConfig(ring=9)
        diffuerase.configure(tone_match="offset")
        assert diffuerase.tone_match_config() == ToneMatchConfig(mode="offset")
        assert diffuerase.tone_match_config("on") == ToneMatchConfig()
        assert diffuerase.tone_match_config("off") is None and diffuerase.tone_match_config(False) is None      # none whatever else is set
        diffuerase.configure(tone_match="off")
        assert diffuerase.tone_match_config() is None                                                      # configure("off") beats the environment
        diffuerase.configure()
        assert diffuerase.tone_match_config() == ToneMatchConfig(ring=9)                                   # configure() resets
        cfg = ToneMatchConfig(smooth=0)
        diffuerase.configure(tone_match=cfg)
        assert diffuerase.tone_match_config() is cfg
        with pytest.raises(ValueError):
            diffuerase.configure(tone_match="sometimes")
        monkeypatch.setenv("VV_TONE_MATCH", "sometimes")
        diffuerase.configure()
        with pytest.raises(ValueError):
            diffuerase.tone_match_config()
    finally:
        diffuerase.configure()


def test_tone_match_refuses_the_reference_early_return(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_TONE_MATCH", raising=False)
    f = [np.zeros((8, 8, 3), np.uint8)] * 2
    for value in ("on", "offset", "ring=4", ToneMatchConfig(), True):
        with pytest.raises(ValueError, match="tone_match="):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, tone_match=value)
    monkeypatch.setenv("VV_TONE_MATCH", "on")
    with pytest.raises(ValueError, match="tone_match="):
        diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)
    with pytest.raises(TypeError):
        diffuerase.run_infill_on_frames(f, f, tonematch="on")
    assert diffuerase.last_tone_match is None


def test_tone_report_assembles_spans_and_windows():
    from videovanish_amd import infill
    one = lambda K, T, v: infill.ToneMatchReport(np.full((K, T), v, np.int64), *(np.full((K, T, 3), float(v)) for _ in range(4)))
    rep = infill.tone_report([one(1, 3, 5), one(2, 2, 7)], [(1, 4), (6, 8)], 9)
    assert rep.n.shape == (2, 9) and rep.n.dtype == np.int64 and rep.gain.shape == rep.offset.shape == rep.rms_before.shape == rep.rms_after.shape == (2, 9, 3)
    assert rep.n.tolist() == [[0, 5, 5, 5, 0, 0, 7, 7, 0], [0, 0, 0, 0, 0, 0, 7, 7, 0]]
    assert (rep.gain[0, [0, 4, 5, 8]] == 1.0).all() and (rep.gain[1, :6] == 1.0).all() and (rep.gain[0, 1:4] == 5.0).all() and (rep.gain[1, 6:8] == 7.0).all()
    assert (rep.offset[0, [0, 4, 5, 8]] == 0.0).all() and (rep.rms_before[1, :6] == 0.0).all() and (rep.rms_after[0, 6:8] == 7.0).all()
    empty = infill.tone_report([], [], 4)
    assert empty.n.shape == (1, 4) and not empty.n.any() and (empty.gain == 1.0).all() and not empty.offset.any()


def test_cli_tone_match_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
    """tests/test_cli_cpu.py's stub: frame I/O and the hot path replaced."""
    import diffuerase
    from videovanish_amd import infill
    calls = []
    videos = {"mask.mkv": [np.zeros((16, 24, 3), np.uint8)] * 3}
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda path, start=0, max_frames=-1: ([f.copy() for f in videos[path]], 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    rep = infill.tone_report([], [], 3)
    rep.gain[0, 1] = (1.0, 0.9, 1.05)
    rep.offset[0, 2, 0] = -7.25

    def fake(frames, masks, **kw):
        calls.append(kw)
        diffuerase.last_tone_match = rep if "tone_match" in kw else None
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 3
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    monkeypatch.setattr(sys, "argv", argv)
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None} and capsys.readouterr().out == ""                      # a default call passes no keyword, prints nothing
    for value in ("on", "offset", "mode=offset,ring=8,smooth=0"):
        monkeypatch.setattr(sys, "argv", argv + ["--tone-match", value, "--roi", "static"])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "tone_match": value, "roi": "static"}
        out = capsys.readouterr().out
        assert out.count("\n") == 1 and out == "tone match: 2 of 3 frames corrected, largest |gain - 1| 0.1000, largest |offset| 7.25\n"
    for bad in ("off", "yes", "ring=x", "ring=40"):
        monkeypatch.setattr(sys, "argv", argv + ["--tone-match", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_tone_match", None)
