"""Grain shape on the CPU: the settings, the binding of include/grainshape.h, the product's fit against the restatement's Python numbers, the
model's closed forms, recovery of a known shape and level on the restatement (tests/grainshape_ref.py), infill.finish with the device functions
replaced by the restatements, configuration and CLI."""
import ctypes
import dataclasses
import inspect
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abiref  # noqa: E402
import grainmatch_ref as GR  # noqa: E402
import grainshape_ref as R  # noqa: E402
import seamblend_ref as BR  # noqa: E402
import tonematch_ref as TR  # noqa: E402

from videovanish_amd import grainmatch as GM  # noqa: E402
from videovanish_amd import grainshape as M  # noqa: E402
from videovanish_amd.grainmatch import GrainMatchConfig  # noqa: E402
from videovanish_amd.grainshape import GrainShapeConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_spellings_and_config():
    assert M.SPELLINGS == ("on",)
    for off in (None, False, "off", "none", "", " OFF "):
        assert M.as_config(off) is None
    d = GrainShapeConfig()
    assert dataclasses.asdict(d) == R.DEFAULTS
    assert M.as_config("on") == M.as_config(" On ") == M.as_config(True) == d
    assert M.as_config("max_a=0.5,dead=0.05,min_pairs=512,smooth=4,max_gain=6") == d
    assert M.as_config(" max_a = 0.25 , dead=0,min_pairs=1,smooth=16,max_gain=1 ") == GrainShapeConfig(0.25, 0.0, 1, 16, 1.0)
    assert M.as_config("dead=0.1").dead == 0.1 and M.as_config("smooth=0") == GrainShapeConfig(smooth=0)
    cfg = GrainShapeConfig(max_a=0.3)
    assert M.as_config(cfg) is cfg
    with pytest.raises(Exception):
        cfg.max_a = 0.4                                                                              # frozen
    for bad in ("yes", "luma", "max_a", "max_a=", "max_a=x", "max_a=0.6", "max_a=-0.1", "max_a=0.2,max_a=0.3", "size=3", "max_a=0.2;dead=0", "dead=0.6",
                "dead=-1", "min_pairs=0", "min_pairs=1.5", "min_pairs=2147483648", "smooth=17", "smooth=-1", "max_gain=0.5", "max_gain=6.5", "max_gain=nan",
                "max_gain=inf", "on,dead=0", "dead=0,", "mode=rgb", 3, 1.0, ("on",)):
        with pytest.raises(ValueError):
            M.as_config(bad)
    with pytest.raises(ValueError, match="'on', 'off', 'max_a=X,dead=X,min_pairs=N,smooth=N,max_gain=X'"):
        M.as_config("sometimes")
    for kw in (dict(max_a=0.51), dict(max_a=-0.01), dict(max_a="0.5"), dict(max_a=True), dict(dead=0.51), dict(dead=float("nan")), dict(min_pairs=0),
               dict(min_pairs=2 ** 31), dict(min_pairs=512.0), dict(smooth=-1), dict(smooth=17), dict(smooth=True), dict(max_gain=0.99), dict(max_gain=6.01),
               dict(max_gain=None)):
        with pytest.raises(ValueError):
            GrainShapeConfig(**kw)
    assert "build-defined" in GrainShapeConfig.__doc__ and "nobody has measured the grain" in GrainShapeConfig.__doc__
    assert int(np.rint(256 * 0.5)) == M.MAX_TAP == 128 and M.NSUM == 30


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_grainshape_header():
    """grainshape_bind.SIGNATURES declares every function of include/grainshape.h with the header's types and in its order, lib() has applied it,
    the version and the limits agree (abiref.check_binding); the arguments are refused before any device work, each refusal naming its
    function; the vvn_ prefix and every name belong to no other part (what test_abi_cpu.py's walk does for the parts of its table)."""
    from videovanish_amd import grainshape_bind as B
    loaded, define = abiref.check_binding(B, 4)
    assert B.EXPORTS == ["vvn_abi_version", "vvn_last_error", "vvn_ring_shape_stats", "vvn_paste_shaped_composite"] and define("VVN_ABI_VERSION") == 1
    assert (define("VVN_MAX_RING"), define("VVN_MAX_TAP"), define("VVN_NSUM")) == (B.MAX_RING, B.MAX_TAP, B.NSUM) == (GM.MAX_RING, M.MAX_TAP, M.NSUM) == (32, 128, 30)
    raw = open(os.path.join(ROOT, "include", "grainshape.h")).read()
    for formula in ("P0(a) = 6 - 16 a + 14 a^2", "P1(a) = -4 + 14 a - 12 a^2", "r0(a) = 1 + 2 a^2", "rho = 2 (C_y - C_x) / (D_y - D_x)",
                    "u_c = (sum_j wy_j sum_i wx_i s(X + i, Y + j) + 2^15) >> 16", "d_c = (amp[t][c][lut(p_c)] * u_c * 5017 + 2^23) >> 24", "64-BIT product",
                    "512^2 * 1020 < 2^31", "modulo 2^64"):
        assert formula in raw, formula                                                               # the rules are part of the ABI
    # Nothing can be launched here: every pointer is host memory and every call below is refused before the first device call.
    buf = (ctypes.c_char * 64)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 32
    stats = lambda patch=a, orig=a, mask=a, offs=a, lut=a, sums=a, Hm=4, Wm=4, T=1, H0=8, W0=8, h=4, w=4, ring=4, flat=24: \
        loaded.vvn_ring_shape_stats(patch, Hm, Wm, orig, mask, offs, lut, T, H0, W0, h, w, ring, flat, sums, None)
    paste = lambda patch=a, orig=a, mask=a, offs=a, lut=a, field=None, q8=256, amp=a, taps=a, ids=a, seed=0, mode=0, out=b, Hm=4, Wm=4, T=1, H0=8, W0=8, h=4, w=4, \
        feather=3.0: loaded.vvn_paste_shaped_composite(patch, Hm, Wm, orig, mask, offs, lut, field, q8, amp, taps, ids, seed, mode, T, H0, W0, h, w, feather, out, None)
    for kw in (dict(patch=None), dict(orig=None), dict(mask=None), dict(offs=None), dict(lut=None), dict(sums=None), dict(Hm=0), dict(Wm=-1), dict(T=0), dict(H0=0),
               dict(W0=0), dict(h=0), dict(w=0), dict(h=9), dict(w=9)):
        assert stats(**kw) == -1 and loaded.vvn_last_error().startswith(b"vvn_ring_shape_stats:"), kw
    for kw in (dict(ring=0), dict(ring=33), dict(flat=-1), dict(flat=256), dict(T=1 << 20, H0=1 << 15, W0=1 << 15, h=1 << 15, w=1 << 15)):
        assert stats(**kw) == -2 and loaded.vvn_last_error().startswith(b"vvn_ring_shape_stats:"), kw
    assert stats(ring=0, T=0) == -1                                                                  # a bad argument before an unsupported one
    for kw in (dict(patch=None), dict(orig=None), dict(offs=None), dict(lut=None), dict(amp=None), dict(taps=None), dict(ids=None), dict(out=None), dict(mask=None),
               dict(Hm=0), dict(T=0), dict(H0=0), dict(h=9), dict(w=9), dict(seed=-1), dict(mode=2), dict(mode=-1)):
        assert paste(**kw) == -1 and loaded.vvn_last_error().startswith(b"vvn_paste_shaped_composite:"), kw
    for kw in (dict(feather=64.5), dict(q8=-1), dict(q8=513), dict(field=a, q8=513)):
        assert paste(**kw) == -2 and loaded.vvn_last_error().startswith(b"vvn_paste_shaped_composite:"), kw
    with pytest.raises(ctypes.ArgumentError):
        paste(seed=2.0)
    with pytest.raises(ctypes.ArgumentError):
        stats(flat=1.5)
    import torch
    z, m = torch.zeros((2, 4, 4, 3), dtype=torch.uint8), torch.zeros((2, 4, 4), dtype=torch.uint8)
    offs, tab = torch.zeros((2, 2), dtype=torch.int32), torch.zeros((2, 3, 256), dtype=torch.uint8)
    taps, ids = torch.zeros((2, 3, 2), dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for call in (lambda: B.ring_shape_stats(z, z, m, offs, tab, 4, 4, 8, 24), lambda: B.ring_shape_stats(z, z, None, offs, tab, 4, 4, 8, 24),
                 lambda: B.paste_shaped_composite(z, z, m, offs, tab, None, 0, tab, taps, ids, 0, 0, 4, 4, 3.0)):
        with pytest.raises(RuntimeError):                                                            # no CPU fallback
            call()
    # the part stands outside abiref.PARTS: its prefix, header and names are checked against every part here
    assert "grainshape_bind" not in abiref.PARTS and abiref.part_of(B) is B.PART and B.PART.header == "grainshape.h"
    assert re.fullmatch(r"vv[a-z]_", B.PART.prefix)
    from videovanish_amd import detailmatch_bind, platetone_bind
    names = set(B.SIGNATURES)
    for module, part in abiref.parts() + [(platetone_bind, platetone_bind.PART), (detailmatch_bind, detailmatch_bind.PART)]:
        assert part.prefix != B.PART.prefix and part.header != B.PART.header, module.__name__
        assert not names & set(module.SIGNATURES), module.__name__
        assert not [n for n in module.SIGNATURES if n.startswith(B.PART.prefix)], module.__name__
    assert all(n.startswith("vvn_") for n in names)


def test_product_sources_of_the_feature():
    """The kernels live in a unit of their own, in the one recipe with the header among the dependencies; no environment; the ring, the window's
    pixel and the noise are the shared statements; the 32-bit partial sums are bounded by static_asserts; the settings import no torch;
    importing the drop-in and asking for the setting resolves no vvn_ symbol."""
    kernel, txt = abiref.check_sources("vv_grainshape", "grainshape.h", "grainshape")
    for fn in ("vvn_ring_shape_stats", "vvn_paste_shaped_composite"):
        assert f'extern "C" int {fn}(' in kernel
    for shared in ('#include "vv_ring_bits.h"', '#include "vv_paste_px.h"', '#include "vv_wave_bytes.h"', "vvring::ring_bits<true>(", "window_px(", "vvpaste::noise_key(",
                   "vvpaste::noise_sum(", "wave_sum(", "2040ll * 2040ll < (1ll << 31)", "2ull * 2040ull * 2040ull < (1ull << 32)", "512ll * 512ll * 1020ll < (1ll << 31)"):
        assert shared in kernel, shared
    assert "import ctypes" not in txt
    code = ("import diffuerase; from videovanish_amd import grainshape_bind, grain_hip, hip; "
            "assert grainshape_bind.PART.dll is None and grain_hip.PART.dll is None and hip.CORE.dll is None; "
            "assert diffuerase.grain_shape_config() is None and diffuerase.last_grain_shape is None")
    env = {k: v for k, v in os.environ.items() if k != "VV_GRAIN_SHAPE"}
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)


# ---- the model and the fit ------------------------------------------------------------------------------------------------------------------
def test_the_model_closed_forms():
    """P0, P1 and r0 are the autocorrelations of [a, 1, a] * [1, -2, 1] and of [a, 1, a]; rho rises from -2/3 to 0 on [0, 0.5] and turns back
    beyond 0.6; the closed-form inverse returns the grid it came from, and clamps."""
    for a in np.linspace(0.0, 0.5, 11):
        g = np.convolve([a, 1.0, a], [1.0, -2.0, 1.0])
        assert np.isclose(M.P0(a), (g * g).sum(), rtol=1e-13) and np.isclose(M.P1(a), (g[:-1] * g[1:]).sum(), rtol=1e-13, atol=1e-13)
        assert np.isclose(M.r0(a), 1 + 2 * a * a) and M.P0(a) == R.P0(a) and M.P1(a) == R.P1(a) and M.r0(a) == R.r0(a)
    assert M.rho(0.0) == -2.0 / 3.0 and M.rho(0.5) == 0.0 and M.P0(0.0) ** 2 == GM.OP_GAIN
    grid = np.linspace(0.0, 0.5, 513)
    assert (np.diff(M.rho(grid)) > 0).all() and M.rho(0.75) < M.rho(0.6)
    assert np.abs(M.a_of(M.rho(grid)) - grid).max() < 1e-12                                          # inverted on the grid
    assert np.abs(np.array([R.a_of(r) for r in M.rho(grid)]) - grid).max() < 1e-12                   # and by the restatement's bisection
    assert M.a_of(-0.9) == 0.0 and M.a_of(-2.0 / 3.0) == 0.0 and M.a_of(0.3) == 0.5 and M.a_of(0.0) == 0.5
    assert M.a_of(M.rho(0.4), max_a=0.3) == 0.3 and M.a_of([-1.0, M.rho(0.25), 1.0]).tolist() == [0.0, M.a_of(M.rho(0.25)), 0.5]


def _shape_row(n, a, scale=1000, base=(0, 0)):
    """One channel-axis entry [pairs, Cx, Cy, Dx, Dy] whose rho is rho(a): Dy - Dx = 2 scale P0, Cy - Cx = scale P1, on top of `base` = (Cx, Dx)."""
    cx, dx = base
    return [n, cx, cx + int(round(scale * 1e6 * M.P1(a))), dx, dx + int(round(2 * scale * 1e6 * M.P0(a)))]


def _rows(T, entry):
    """[T,30] with entry(t, c, axis) in every place."""
    return np.array([[v for c in range(3) for axis in range(2) for v in entry(t, c, axis)] for t in range(T)], np.int64)


def _grain_rows(T, n=1000, var=9.0):
    """[T,36]: every band n pixels, Sx = 0, Sy = 36 n var."""
    return np.tile(np.array([n, 0, int(36 * n * var)] * 12, np.int64), (T, 1))


def test_the_fit_clamps_dead_zone_support_and_level():
    g, rgb = GrainMatchConfig(), GrainMatchConfig(mode="rgb")
    cfg = GrainShapeConfig(smooth=0, min_pairs=100)
    one = lambda entry, gc=rgb, gs=None, **kw: M.fit(_rows(1, lambda t, c, axis: entry(c, axis)), _grain_rows(1) if gs is None else gs, gc, dataclasses.replace(cfg, **kw))
    # rho is inverted and quantised; each channel and axis on its own in "rgb"
    want = {(0, 0): 0.125, (0, 1): 0.25, (1, 0): 0.375, (1, 1): 0.5, (2, 0): 0.0, (2, 1): 0.0625}
    f = one(lambda c, axis: _shape_row(100, want[c, axis], base=(-5000, 700000)))
    assert f.taps.dtype == np.int32 and f.taps[0].tolist() == [[32, 64], [96, 128], [0, 16]] and (f.a == f.taps / 256.0).all()
    assert np.allclose(f.rho[0], [[M.rho(want[c, k]) for k in range(2)] for c in range(3)], atol=1e-6) and not f.clamped.any()
    assert f.dead[0].tolist() == [[False, False], [False, False], [True, False]] and (f.pairs == 100).all() and f.pairs.dtype == np.int64
    # the level: k = 6 sqrt(r0x r0y / (P0x P0y)), exactly 1 at a = 0 and 6 at the binomial on both axes; sigma_pixel = k sigma_white, capped
    k = [6 * np.sqrt(M.r0(want[c, 0]) * M.r0(want[c, 1]) / (M.P0(want[c, 0]) * M.P0(want[c, 1]))) for c in range(3)]
    assert np.allclose(f.k[0], k, rtol=1e-12) and np.allclose(f.sigma_pixel[0], np.minimum(3.0 * np.array(k)[:, None], 12.0), rtol=1e-12)
    assert one(lambda c, axis: _shape_row(100, 0.5)).k.tolist() == [[6.0] * 3] and one(lambda c, axis: _shape_row(100, 0.0)).k.tolist() == [[1.0] * 3]
    assert one(lambda c, axis: _shape_row(100, 0.5), max_gain=2.5).k.tolist() == [[2.5] * 3]
    assert np.allclose(one(lambda c, axis: _shape_row(100, 0.5), gc=GrainMatchConfig(mode="rgb", strength=0.5, max_sigma=15.9), max_gain=4).sigma_pixel, 0.5 * 4 * 3.0)
    # the amplitude is the white sigma in front of the kernel
    f = one(lambda c, axis: _shape_row(100, 0.25), gs=_grain_rows(1, var=0.25))
    kk = 6 * M.r0(0.25) / M.P0(0.25)
    assert np.allclose(f.sigma_pixel, 0.5 * kk) and (f.amp == GM.tables(np.full((1, 3, 4), 0.5 * kk / M.r0(0.25)))).all()
    # the clamps at both ends, the cap below the family's end, the dead zone
    f = one(lambda c, axis: [100, 0, -3 * 10 ** 9, 0, 6 * 10 ** 9] if axis == 0 else [100, 0, 10 ** 9, 0, 6 * 10 ** 9])                # rho = -1 and rho = +1/3
    assert f.taps[0].tolist() == [[0, 128]] * 3 and f.clamped[0].tolist() == [[True, True]] * 3 and f.rho[0, 0].tolist() == [-1.0, 1.0 / 3.0]
    f = one(lambda c, axis: _shape_row(100, 0.4), max_a=0.25)
    assert f.taps[0].tolist() == [[64, 64]] * 3 and f.clamped.all() and not f.dead.any()
    assert one(lambda c, axis: _shape_row(100, 0.04)).taps.tolist() == [[[0, 0]] * 3] and one(lambda c, axis: _shape_row(100, 0.04)).dead.all()
    assert one(lambda c, axis: _shape_row(100, 0.04), dead=0.0).taps.tolist() == [[[10, 10]] * 3]
    assert one(lambda c, axis: _shape_row(100, 0.06)).taps.tolist() == [[[15, 15]] * 3]
    # support: min_pairs, and Dy - Dx <= 0 gives 0 on that axis alone
    f = one(lambda c, axis: _shape_row(99 if axis == 0 else 100, 0.25))
    assert f.taps[0].tolist() == [[0, 64]] * 3 and f.rho[0, :, 0].tolist() == [0.0] * 3 and not f.dead[0, :, 0].any() and not f.clamped.any()
    f = one(lambda c, axis: [100, 0, 5, 10, 10] if axis == 1 else _shape_row(100, 0.25))
    assert f.taps[0].tolist() == [[64, 0]] * 3
    assert one(lambda c, axis: [100, 0, 5, 10, 9]).taps.tolist() == [[[0, 0]] * 3] and one(lambda c, axis: [100, 0, 5, 10, 9]).k.tolist() == [[1.0] * 3]
    # "luma" sums the channels: 34 + 33 + 33 pairs make the pool live, and the shape is one per frame
    f = one(lambda c, axis: _shape_row(34 if c == 0 else 33, (0.1, 0.25, 0.4)[c]), gc=g)
    assert (f.taps[0] == f.taps[0, 0]).all() and 0 < f.taps[0, 0, 0] < 128 and f.pairs[0, :, 0].tolist() == [34, 33, 33]
    assert one(lambda c, axis: _shape_row(34 if c == 0 else 33, 0.25)).taps.tolist() == [[[0, 0]] * 3]                                   # "rgb": each short
    # zero taps give grainmatch.tables' table unchanged, whatever the sums
    rng = np.random.default_rng(5)
    gs = rng.integers(0, 4000, (6, 36)).astype(np.int64) * np.tile([1, 1000, 3000], 12)
    for gc in (g, rgb, GrainMatchConfig(strength=0.7, max_sigma=3.0, smooth=1)):
        f = M.fit(np.zeros((6, 30), np.int64), gs, gc, GrainShapeConfig())
        own = GM.fit(gs, gc)
        assert not f.taps.any() and (f.k == 1.0).all() and (f.amp == GM.tables(own.sigma_added)).all() and (f.sigma_pixel == own.sigma_added).all()
        assert f.amp.dtype == np.uint8 and f.amp.shape == (6, 3, 256) and f.amp.any()


def test_the_fit_pools_frames_and_equals_the_restatement():
    # pooling: frames 0 and 2 hold 60 pairs each, frame 1 none; smooth 1 pools 120 >= 100 at frame 1 only
    s = _rows(3, lambda t, c, axis: _shape_row(60, 0.25) if t != 1 else [0] * 5)
    f = M.fit(s, _grain_rows(3), GrainMatchConfig(mode="rgb"), GrainShapeConfig(smooth=1, min_pairs=100))
    assert f.taps[:, 0, 0].tolist() == [0, 64, 0] and f.pairs[:, 0, 0].tolist() == [60, 0, 60]
    assert M.fit(s, _grain_rows(3), GrainMatchConfig(mode="rgb"), GrainShapeConfig(smooth=2, min_pairs=100)).taps[:, 0, 0].tolist() == [64, 64, 64]
    assert M.fit(np.zeros((0, 30), np.int64), np.zeros((0, 36), np.int64), GrainMatchConfig(), GrainShapeConfig()).taps.shape == (0, 3, 2)
    # the product against the restatement's Python numbers on random sums
    rng = np.random.default_rng(9)
    T = 24
    n = rng.integers(0, 400, (T, 3, 2))
    s = np.zeros((T, 3, 2, 5), np.int64)
    s[..., 0] = n
    s[..., 3] = rng.integers(0, 10 ** 6, (T, 3, 2)) * n
    s[..., 4] = s[..., 3] + rng.integers(-10 ** 5, 10 ** 7, (T, 3, 2)) * n
    s[..., 1] = rng.integers(-10 ** 5, 10 ** 5, (T, 3, 2)) * n
    s[..., 2] = s[..., 1] + rng.integers(-4 * 10 ** 6, 10 ** 6, (T, 3, 2)) * n
    s[7] = 0
    gs = rng.integers(0, 600, (T, 36)).astype(np.int64) * np.tile([1, 500, 4000], 12)
    seen = set()
    for mode in ("luma", "rgb"):
        for kw in ({}, dict(smooth=0), dict(min_pairs=2000, smooth=6), dict(dead=0.0, max_a=0.3), dict(max_gain=2.0, dead=0.2)):
            for gkw in ({}, dict(smooth=1, strength=1.5, max_sigma=6.0, min_count=900)):
                f = M.fit(s.reshape(T, 30), gs, GrainMatchConfig(mode=mode, **gkw), GrainShapeConfig(**kw))
                rh, taps, ks, sp, clamped, dead, amp = R.fit(s.reshape(T, 30), gs, mode=mode, grain_smooth=gkw.get("smooth", 4), strength=gkw.get("strength", 1.0),
                                                              max_sigma=gkw.get("max_sigma", 12.0), min_count=gkw.get("min_count", 256), **dict(R.DEFAULTS, **kw))
                assert (f.taps == taps).all() and (f.amp == amp).all() and (f.clamped == clamped).all() and (f.dead == dead).all(), (mode, kw, gkw)
                assert np.allclose(f.rho, rh, rtol=1e-13, atol=0) and np.allclose(f.k, ks, rtol=1e-13) and np.allclose(f.sigma_pixel, sp, rtol=1e-12), (mode, kw, gkw)
                seen |= set(f.taps.ravel().tolist())
    assert len(seen) > 30 and 0 in seen and 128 in seen


# ---- the restated rules ---------------------------------------------------------------------------------------------------------------------
def test_restatement_invariants():
    """The extended white field is grainmatch_ref.noise inside the frame; zero taps give grainmatch_ref's and seamblend_ref's composites; taps
    move bytes; the shaped field's variance is r0x r0y times the white one's; the pair sums of x = y carry equal x and y entries."""
    H, W = 21, 34
    for mode in ("luma", "rgb"):
        s = R.field(3, 5, H, W, mode)
        assert s.shape == (H + 2, W + 2, 3) and (s[1:-1, 1:-1] == GR.noise(3, 5, H, W, mode)).all()
        assert (R.shaped(3, 5, H, W, mode, np.zeros((3, 2), np.int64)) == s[1:-1, 1:-1]).all()
    s = R.field(1, 0, 200, 300, "rgb")[1:-1, 1:-1].astype(np.float64)
    u = R.shaped(1, 0, 200, 300, "rgb", [[128, 128], [64, 0], [0, 32]]).astype(np.float64)
    for c, (ax, ay) in enumerate(((0.5, 0.5), (0.25, 0.0), (0.0, 0.125))):
        assert abs(u[..., c].var() / (s[..., c].var() * M.r0(ax) * M.r0(ay)) - 1) < 0.03
    rng = np.random.default_rng(2)
    T, H0, W0, h, w = 2, 30, 40, 12, 16
    patch, orig = rng.integers(0, 256, (T, 9, 11, 3)).astype(np.uint8), rng.integers(0, 256, (T, H0, W0, 3)).astype(np.uint8)
    mask = np.zeros((T, H0, W0), np.uint8)
    mask[:, 8:20, 10:30] = 255
    offs = np.array([[0, 0], [H0 - h, W0 - w]], np.int32)
    lut, amp = rng.integers(0, 256, (T, 3, 256)).astype(np.uint8), rng.integers(0, 256, (T, 3, 256)).astype(np.uint8)
    membrane = rng.integers(-2000, 2000, (T, h, w, 3)).astype(np.int16)
    ids, zero = np.array([4, 9], np.int32), np.zeros((T, 3, 2), np.int32)
    for mode in ("luma", "rgb"):
        for feather in (3.0, -1.0):
            a = R.composite(patch, orig, mask, offs, lut, None, 0, amp, zero, ids, 7, mode, h, w, feather)
            assert (a == GR.composite(patch, orig, mask, offs, lut, amp, ids, 7, mode, h, w, feather)).all()
            b = R.composite(patch, orig, mask, offs, lut, membrane, 256, amp, zero, ids, 7, mode, h, w, feather)
            assert (b == BR.composite(patch, orig, mask, offs, lut, membrane, 256, amp, ids, 7, mode, h, w, feather)).all() and (a != b).any()
            assert (R.composite(patch, orig, mask, offs, lut, None, 0, amp, zero + 128, ids, 7, mode, h, w, feather) != a).any()
            assert (R.composite(patch, orig, mask, offs, lut, None, 0, 0 * amp, zero + 128, ids, 7, mode, h, w, feather) ==
                    TR.composite(patch, orig, mask, offs, lut, h, w, feather)).all()
    orig, x, mask = R.recovery_clip(0, 4, 0.25, 0.25)
    offs1, ident = np.zeros((1, 2), np.int32), np.broadcast_to(R.IDENT, (1, 3, 256))
    s = R.sums(orig, orig, mask, offs1, ident, 96, 130, 12, 255).reshape(3, 2, 5)
    assert (s[..., 0] > 1000).all() and (s[..., 1] == s[..., 2]).all() and (s[..., 3] == s[..., 4]).all()
    assert not R.sums(orig, orig, 0 * mask, offs1, ident, 96, 130, 12, 255).any()


# ---- recovery, on the restatement alone -------------------------------------------------------------------------------------------------------
def _recover(ax, ay, sigma, seeds):
    """(worst |a_fit - a|, worst |sigma_pixel / sigma - 1|, the worst and the smallest of the same of the white fit, the smallest pooled pair
    count, the seeds whose white case missed a = 0) at the default settings."""
    offs, ident = np.zeros((R.RECOVERY_T, 2), np.int32), np.broadcast_to(R.IDENT, (R.RECOVERY_T, 3, 256))
    wa = ws = ww = 0.0
    wb = 1.0
    pairs, missed = 10 ** 9, 0
    for s in seeds:
        orig, x, mask = R.recovery_clip(s, sigma, ax, ay)
        gs, ss = GR.sums(x, orig, mask, offs, ident, 96, 130, 12, 24), R.sums(x, orig, mask, offs, ident, 96, 130, 12, 24)
        rh, taps, ks, sp, clamped, dead, amp = R.fit(ss, gs)
        pairs = min(pairs, int(ss.reshape(-1, 3, 2, 5)[..., 0].sum(axis=(0, 1)).min()))
        wa = max(wa, float(np.abs(taps / 256.0 - np.array([ax, ay])).max()))
        ws = max(ws, float(np.abs(sp / sigma - 1).max()))
        ww = max(ww, float(np.abs(GR.fit(gs)[2] / sigma - 1).max()))
        wb = min(wb, float(np.abs(GR.fit(gs)[2] / sigma - 1).min()))
        missed += bool(taps.any()) if (ax, ay) == (0.0, 0.0) else 0
        f = M.fit(ss, gs, GrainMatchConfig(), GrainShapeConfig())                                    # the product's fit of the same sums
        assert (f.taps == taps).all() and (f.amp == amp).all()
    return wa, ws, ww, wb, pairs, missed


@pytest.mark.parametrize("shape", R.RECOVERY_SHAPES)
def test_reference_recovers_shape_and_level(shape):
    """recovery_clip's ring at T = 1 holds ten times min_pairs on both axes (asserted: a condition, not a measurement).  The figures printed here
    are grainshape_ref.MEASURED_DEVIATION; the shaped fit stays within 1.5 times them (the GPU tests assert the same bound on the product)."""
    ax, ay = shape
    for sigma in R.RECOVERY_SIGMAS:
        wa, ws, ww, wb, pairs, missed = _recover(ax, ay, sigma, R.RECOVERY_SEEDS)
        print(f"a = ({ax}, {ay}), sigma {sigma}: worst |a_fit - a| {wa:.4f}, worst |sigma_pixel / sigma - 1| {ws:.4f}, white fit {wb:.4f} .. {ww:.4f}, "
              f"smallest pooled pairs {pairs}, white cases off zero {missed}")
        assert pairs >= R.DEFAULTS["min_pairs"]
        m = R.MEASURED_DEVIATION[shape][sigma]
        assert wa <= 1.5 * m["a"] and ws <= 1.5 * m["sigma"] and ww <= 1.5 * m["white"] and wb >= m["white_least"] / 1.5
        if shape == (0.0, 0.0):
            assert missed <= 1                                                                       # the dead zone takes white grain for white
        else:
            assert ww > 1.5 * ws                                                                     # what the option is for


@pytest.mark.parametrize("shape", R.RECOVERY_SHAPES)
def test_reference_adds_the_level_inside_the_mask(shape):
    """The whole stage on the restatement: the shaped estimator on the composite's pixels deep inside the mask reads the level of the original's
    grain (the "inside" figures of grainshape_ref.MEASURED_DEVIATION, printed here)."""
    offs = np.zeros((R.RECOVERY_T, 2), np.int32)
    for sigma in R.RECOVERY_SIGMAS:
        worst = 0.0
        for s in R.RECOVERY_SEEDS:
            orig, x, mask = R.recovery_clip(s, sigma, *shape)
            out = R.apply(x, orig, mask, offs, 96, 130, 3.0)[0]
            worst = max(worst, float(np.abs(R.inside_estimate(out[0], x[0], mask[0]) / sigma - 1).max()))
        print(f"a = {shape}, sigma {sigma}: worst |inside estimate / sigma - 1| {worst:.4f}")
        assert worst <= 1.5 * R.MEASURED_DEVIATION[shape][sigma]["inside"]


# ---- infill.finish with the kernels replaced by the restatements ----------------------------------------------------------------------------
def _stand_ins(monkeypatch, calls, on, shaped=True):
    """tests/test_seamblend_cpu.py's stand-ins of the paste and seam entry points (a stage that is not in `on` raises), plus this feature's;
    calls gets (name, frames) per call."""
    import test_seamblend_cpu as SB
    from videovanish_amd import grainshape_bind
    SB._all_stand_ins(monkeypatch, calls, on)

    def said(name, fn):
        def f(patch, *a, **k):
            calls.append((name, len(patch)))
            return fn(patch, *a, **k)
        return f

    if shaped:
        monkeypatch.setattr(grainshape_bind, "ring_shape_stats", said("ring_shape_stats", R.hip_ring_shape_stats))
        monkeypatch.setattr(grainshape_bind, "paste_shaped_composite", said("paste_shaped_composite", R.hip_paste_shaped_composite))
    else:
        boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("a grain shape call without grain_shape="))
        for name in ("ring_shape_stats", "paste_shaped_composite", "lib"):
            monkeypatch.setattr(grainshape_bind, name, boom)


def _clip(T=3, sigma=4, a=0.5):
    """(orig, x, mask) [T,96,130]: the recovery clip's smooth frame with fresh shaped grain per frame; the last frame has no mask."""
    orig, x, mask = R.recovery_clip(1, sigma, a, a, T=T)
    mask[-1] = 0
    return orig, x, mask


def test_finish_runs_the_shape_next_to_the_grain_statistic(monkeypatch):
    """The full frame with grain and its shape, alone, behind tone and with blend: the calls in order and the bytes and report of the restatement."""
    import torch
    from videovanish_amd import infill
    from videovanish_amd.seamblend import SeamBlendConfig
    from videovanish_amd.tonematch import ToneMatchConfig
    calls = []
    _stand_ins(monkeypatch, calls, ("tone", "grain", "blend"))
    monkeypatch.setattr("videovanish_amd.seamblend.groups", lambda T, h, w: [(0, 2), (2, T)])
    orig, x, mask = _clip()
    T, H, W = mask.shape
    offs = np.zeros((T, 2), np.int32)
    g = GrainMatchConfig(seed=5, min_count=64, smooth=1)
    gkw = dict(smooth=1, min_count=64)
    for extra, want_calls, ref in (
            ({}, ["ring_grain_stats", "ring_shape_stats", "paste_shaped_composite"], {}),
            (dict(tone=ToneMatchConfig()), ["ring_stats", "ring_grain_stats", "ring_shape_stats", "paste_shaped_composite"], dict(tone=dict(ring=12))),
            (dict(tone=ToneMatchConfig(), blend=SeamBlendConfig(strength=0.75)),
             ["ring_stats", "ring_grain_stats", "ring_shape_stats", "solve", "paste_shaped_composite", "solve", "paste_shaped_composite"],
             dict(tone=dict(ring=12), blend=dict(strength=0.75)))):
        del calls[:]
        rows, grows = [], []
        out = np.stack(infill.finish([list(x)], list(orig), torch.from_numpy(mask), [], 3, True, "cpu", grain=g, grain_out=grows, frame0=7,
                                     grain_shape=GrainShapeConfig(smooth=1), grain_shape_out=rows, **extra))
        assert [c[0] for c in calls] == want_calls
        want, ss, gs, f = R.apply(x, orig, mask, offs, H, W, 3.0, frame_ids=[7, 8, 9], seed=5, grain=gkw, smooth=1, **ref)
        assert (out == want).all() and f[1][:2].any() and (out != orig).any()
        rep, = rows
        assert isinstance(rep, infill.GrainShapeReport) and rep._fields == ("pairs", "rho", "a", "k", "sigma_pixel", "clamped", "dead")
        assert rep.pairs.shape == rep.rho.shape == rep.a.shape == rep.clamped.shape == rep.dead.shape == (1, T, 3, 2) and rep.k.shape == (1, T, 3)
        assert rep.sigma_pixel.shape == (1, T, 3, 4) and rep.pairs.dtype == np.int64 and rep.clamped.dtype == rep.dead.dtype == bool
        assert (rep.a[0] * 256 == f[1]).all() and np.allclose(rep.rho[0], f[0], rtol=1e-13) and np.allclose(rep.k[0], f[2], rtol=1e-13)
        assert np.allclose(rep.sigma_pixel[0], f[3], rtol=1e-12) and (rep.pairs[0] == ss.reshape(T, 3, 2, 5)[..., 0]).all() and not rep.pairs[0, 2].any()
        assert (rep.clamped[0] == f[4]).all() and (rep.dead[0] == f[5]).all()
        assert len(grows) == 1 and (grows[0].n[0] == gs.reshape(T, 3, 4, 3)[..., 0]).all()              # grain matching's own report stays
    with pytest.raises(ValueError, match="grain_shape"):
        infill.finish([list(x)], list(orig), torch.from_numpy(mask), [], 3, True, "cpu", grain_shape=GrainShapeConfig())


def test_finish_two_windows_and_a_frame_of_another_rank(monkeypatch):
    import torch
    from videovanish_amd import infill
    calls = []
    _stand_ins(monkeypatch, calls, ("grain",))
    T, H, W = 4, 96, 130
    orig = np.concatenate([R.recovery_clip(2, 4, 0.5, 0.5, T=T)[0][:, :, :65], R.recovery_clip(2, 4, 0.0, 0.0, T=T)[0][:, :, 65:]], axis=2)
    smooth = R.recovery_clip(2, 4, 0.5, 0.5, T=T)[1]
    wins = [((10, 0), (70, 60)), ((12, 68), (72, 60))]
    mask = np.zeros((T, H, W), np.uint8)
    mask[:, 30:55, 18:40] = 255
    mask[:, 34:60, 86:110] = 255
    plans, outs = [], []
    for (oy, ox), (h, w) in wins:
        plans.append(types.SimpleNamespace(size=(h, w), offsets=np.tile(np.array([[oy, ox]], np.int32), (T, 1))))
        outs.append(list(smooth[:, oy:oy + h, ox:ox + w]))
    idx = [0, 1, 3]
    for o in outs:
        o[2] = None
    g, n = GrainMatchConfig(min_count=64, smooth=4), GrainShapeConfig(min_pairs=256)
    rows = []
    got = infill.finish(outs, list(orig), torch.from_numpy(mask), plans, 3, True, "cpu", grain=g, grain_shape=n, grain_shape_out=rows)
    assert got[2] is None and [c[0] for c in calls] == ["ring_grain_stats", "ring_shape_stats", "paste_shaped_composite"] * 2 and all(c[1] == 3 for c in calls)
    want, ident = orig[idx], np.broadcast_to(R.IDENT, (3, 3, 256))
    rep, = rows
    assert rep.pairs.shape == (2, T, 3, 2)
    for k, (plan, o) in enumerate(zip(plans, outs)):
        h, w = plan.size
        patch = np.stack([o[i] for i in idx])
        gs, ss = np.zeros((T, 36), np.int64), np.zeros((T, 30), np.int64)
        gs[idx] = GR.sums(patch, want, mask[idx], plan.offsets[idx], ident, h, w, 12, 24)
        ss[idx] = R.sums(patch, want, mask[idx], plan.offsets[idx], ident, h, w, 12, 24)
        f = R.fit(ss, gs, min_count=64, **dict(R.DEFAULTS, min_pairs=256))
        want = R.composite(patch, want, mask[idx], plan.offsets[idx], ident, None, 0, f[6][idx], f[1][idx], np.array(idx, np.int32), 0, "luma", h, w, 3.0)
        assert (rep.a[k] * 256 == f[1]).all() and not rep.pairs[k, 2].any() and (rep.pairs[k, idx] > 0).all()
    assert (np.stack([got[i] for i in idx]) == want).all()
    assert rep.a[0, 0].min() > 0.3 and not rep.a[1].any()                                             # the two windows are fitted independently
    rows = []
    none = infill.finish([[None] * T, [None] * T], list(orig), torch.from_numpy(mask), plans, 3, True, "cpu", grain=g, grain_shape=n, grain_shape_out=rows)
    assert none == [None] * T and rows[0].pairs.shape == (2, T, 3, 2) and not rows[0].a.any() and (rows[0].k == 1.0).all()


def test_grain_shape_report_assembles_spans_and_windows_and_finish_keeps_its_signature():
    from videovanish_amd import infill
    one = lambda K, T, v: infill.GrainShapeReport(np.full((K, T, 3, 2), v, np.int64), np.full((K, T, 3, 2), -v / 100.0), np.full((K, T, 3, 2), v / 256.0),
                                                  np.full((K, T, 3), float(v)), np.full((K, T, 3, 4), float(v)), np.ones((K, T, 3, 2), bool), np.zeros((K, T, 3, 2), bool))
    rep = infill.grain_shape_report([one(1, 3, 5), one(2, 2, 7)], [(1, 4), (6, 8)], 9)
    assert rep.pairs[..., 0, 0].tolist() == [[0, 5, 5, 5, 0, 0, 7, 7, 0], [0, 0, 0, 0, 0, 0, 7, 7, 0]] and (rep.a * 256 == rep.pairs).all()
    assert (rep.k[..., 0] == np.where(rep.pairs[..., 0, 0] > 0, rep.pairs[..., 0, 0], 1)).all() and (rep.clamped == (rep.pairs > 0)).all() and not rep.dead.any()
    empty = infill.grain_shape_report([], [], 4)
    assert empty.pairs.shape == (1, 4, 3, 2) and not empty.a.any() and (empty.k == 1.0).all() and infill.grain_shape_report([], [], 4, K=3).k.shape == (3, 4, 3)
    names = list(inspect.signature(infill.finish).parameters)
    assert names[names.index("grain_out") + 1:names.index("grain_out") + 3] == ["grain_shape", "grain_shape_out"] and names[-2:] == ["detail", "detail_out"]
    assert all(inspect.signature(infill.finish).parameters[k].default is None for k in ("grain_shape", "grain_shape_out"))


def test_finish_without_the_option_calls_nothing_of_the_feature(monkeypatch):
    import torch
    from videovanish_amd import infill
    calls = []
    _stand_ins(monkeypatch, calls, ("grain",), shaped=False)
    orig, x, mask = _clip()
    out = np.stack(infill.finish([list(x)], list(orig), torch.from_numpy(mask), [], 3, True, "cpu", grain=GrainMatchConfig(min_count=64)))
    assert (out == GR.apply(x, orig, mask, np.zeros((3, 2), np.int32), 96, 130, 3.0, [0, 1, 2], min_count=64)[0]).all()
    assert [c[0] for c in calls] == ["ring_grain_stats", "paste_grain_composite"]


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_the_call_passes_the_keywords_only_when_the_option_is_set(monkeypatch):
    import torch

    import diffuerase
    from videovanish_amd import hip, infill
    for o in diffuerase.ALL_OPTIONS:
        monkeypatch.delenv(o.env, raising=False)
    T = 3
    frames = [np.zeros((8, 8, 3), np.uint8) for _ in range(T)]
    log = []
    part = infill.grain_shape_report([], [], T)
    part.a[0, 1] = 0.5

    def run_clip(f, d, *a, **kw):
        log.append(kw)
        if "grain_shape_out" in kw:
            kw["grain_shape_out"].append(part)
        if "grain_out" in kw:
            kw["grain_out"].append(infill.grain_report([], [], T))
        return list(f)

    monkeypatch.setattr(diffuerase, "get_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(hip, "mask_collapse_dilate", lambda m, it: torch.zeros((T, 8, 8), dtype=torch.uint8))
    monkeypatch.setattr(infill, "run_clip", run_clip)
    diffuerase.configure()
    diffuerase.last_grain_shape = "stale"
    diffuerase.run_infill_on_frames(frames, frames)
    assert log == [{}] and diffuerase.last_grain_shape is None
    diffuerase.run_infill_on_frames(frames, frames, grain_match="on")
    assert set(log[-1]) == {"grain", "grain_out"} and diffuerase.last_grain_shape is None
    diffuerase.run_infill_on_frames(frames, frames, grain_match="rgb", grain_shape="max_a=0.3")
    assert set(log[-1]) == {"grain", "grain_out", "grain_shape", "grain_shape_out"} and log[-1]["grain_shape"] == GrainShapeConfig(max_a=0.3)
    rep = diffuerase.last_grain_shape
    assert isinstance(rep, infill.GrainShapeReport) and rep.a[0, :, 0, 0].tolist() == [0.0, 0.5, 0.0] and diffuerase.last_grain_match is not None
    diffuerase.run_infill_on_frames(frames, frames, grain_match="on", grain_shape="off")
    assert set(log[-1]) == {"grain", "grain_out"} and diffuerase.last_grain_shape is None


def test_precedence_argument_configure_environment_and_exclusions(monkeypatch):
    import diffuerase
    for name in ("VV_GRAIN_SHAPE", "VV_GRAIN_MATCH"):
        monkeypatch.delenv(name, raising=False)
    row = diffuerase._OPTION["grain_shape"]
    assert row in diffuerase.MORE_OPTIONS and row not in diffuerase.OPTIONS and len(diffuerase.OPTIONS) == 10
    assert row.env == "VV_GRAIN_SHAPE" and row.settings is M and row.phrase == "grain shape"
    assert [M.as_config(x) for x in row.metavar.split("|")] == [GrainShapeConfig()] * 2
    try:
        diffuerase.configure()
        assert diffuerase.grain_shape_config() is None
        monkeypatch.setenv("VV_GRAIN_SHAPE", "dead=0.1")
        assert diffuerase.grain_shape_config() == GrainShapeConfig(dead=0.1)
        diffuerase.configure(grain_shape="max_a=0.25")
        assert diffuerase.grain_shape_config() == GrainShapeConfig(max_a=0.25) and diffuerase.grain_shape_config("on") == GrainShapeConfig()
        assert diffuerase.grain_shape_config("off") is None and diffuerase.grain_shape_config(False) is None
        diffuerase.configure(grain_shape="off")
        assert diffuerase.grain_shape_config() is None                                                     # configure("off") beats the environment
        mine = GrainShapeConfig(smooth=0)
        assert diffuerase.grain_shape_config(mine) is mine
        diffuerase.configure()
        assert diffuerase.grain_shape_config() == GrainShapeConfig(dead=0.1)                               # configure() resets
        with pytest.raises(ValueError):
            diffuerase.configure(grain_shape="sometimes")
        f = [np.zeros((8, 8, 3), np.uint8)] * 2
        with pytest.raises(ValueError, match=r"grain_shape= \(grain shape\) needs grain_match= \(seam grain matching\)"):
            diffuerase.run_infill_on_frames(f, f)                                                          # from the environment, no grain_match
        with pytest.raises(ValueError, match=r"grain_shape= \(grain shape\) needs grain_match="):
            diffuerase.run_infill_on_frames(f, f, grain_match="off")
        monkeypatch.delenv("VV_GRAIN_SHAPE")
        for value in ("on", "dead=0.1", GrainShapeConfig(), True):
            with pytest.raises(ValueError, match="needs grain_match="):
                diffuerase.run_infill_on_frames(f, f, grain_shape=value)
            with pytest.raises(ValueError, match="compat_reference_early_return=True"):
                diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, grain_match="on", grain_shape=value)
        with pytest.raises(ValueError, match="0 <= max_a <= 0.5"):
            diffuerase.run_infill_on_frames(f, f, grain_match="on", grain_shape="max_a=0.7")
        with pytest.raises(TypeError):
            diffuerase.run_infill_on_frames(f, f, grainshape="on")
        diffuerase.last_grain_shape = "stale"
        with pytest.raises(ValueError):
            diffuerase.run_infill_on_frames(f, f, grain_shape="on")
        assert diffuerase.last_grain_shape is None                                                         # reset at the start of every call
        monkeypatch.setenv("VV_GRAIN_SHAPE", "sometimes")
        with pytest.raises(ValueError):
            diffuerase.grain_shape_config()
    finally:
        diffuerase.configure()
    for fn in (diffuerase.run_infill_on_frames, diffuerase.configure):
        names = list(inspect.signature(fn).parameters)
        p = inspect.signature(fn).parameters["grain_shape"]
        assert names[names.index("grain_match") + 1] == "grain_shape" and names[names.index("grain_shape") + 1] == "seam_blend"
        assert names[names.index("seam_blend") + 1] == "detail_match" and names[-3:] == ["plate_grain", "plate_align", "plate_fill"]
        assert p.default is None and (fn is diffuerase.configure or p.kind is inspect.Parameter.KEYWORD_ONLY)


def test_cli_grain_shape_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
    import diffuerase
    from videovanish_amd import infill
    calls = []
    videos = {"mask.mkv": [np.zeros((16, 24, 3), np.uint8)] * 4}
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda path, start=0, max_frames=-1: ([f.copy() for f in videos[path]], 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    rep = infill.grain_shape_report([], [], 4, K=2)
    rep.a[0, 0] = 0.25
    rep.a[1, 2, 1, 0] = 0.4375
    rep.k[1, 2] = 3.5
    rep.sigma_pixel[0, 0] = 6.25

    def fake(frames, masks, **kw):
        calls.append(kw)
        diffuerase.last_grain_shape = rep if "grain_shape" in kw else None
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 4
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    monkeypatch.setattr(sys, "argv", argv)
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None} and capsys.readouterr().out == ""                      # a default call passes no keyword, prints nothing
    for value in ("on", "max_a=0.4,dead=0.1"):
        monkeypatch.setattr(sys, "argv", argv + ["--grain-match", "rgb", "--grain-shape", value])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "grain_match": "rgb", "grain_shape": value}
        assert capsys.readouterr().out == "grain shape: grain shaped in 2 of 4 frames, largest a 0.438, largest level gain 3.50, largest sigma 6.25\n"
    for bad in ("off", "yes", "max_a=x", "max_a=0.6", "luma"):
        monkeypatch.setattr(sys, "argv", argv + ["--grain-shape", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_grain_shape", None)
