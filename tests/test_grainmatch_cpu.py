"""Seam grain matching on the CPU: the settings, the binding of include/vvgrain.h, the properties of the fit over seeded draws of sums (the
product's host code against the restatement of tests/grainmatch_ref.py, bit for bit in the tables), the recovery of a known grain and the
properties of the noise on the restatement alone, configuration and CLI."""
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
import grainmatch_ref as R  # noqa: E402

from videovanish_amd import grainmatch as M  # noqa: E402
from videovanish_amd.grainmatch import GrainMatchConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_spellings_and_config():
    assert M.SPELLINGS == ("on", "luma", "rgb")
    for off in (None, False, "off", "none", "", " OFF "):
        assert M.as_config(off) is None
    d = GrainMatchConfig()
    assert (d.mode, d.ring, d.smooth, d.strength, d.max_sigma, d.flat, d.min_count, d.seed) == ("luma", 12, 4, 1.0, 12.0, 24, 256, 0)
    assert M.as_config("on") == M.as_config(" On ") == M.as_config(True) == M.as_config("luma") == d
    assert M.as_config("rgb") == M.as_config(" RGB ") == GrainMatchConfig(mode="rgb")
    assert M.as_config("mode=rgb,ring=8,strength=0.8,seed=3") == GrainMatchConfig(mode="rgb", ring=8, strength=0.8, seed=3)
    assert M.as_config(" max_sigma = 15.9 , flat=0,min_count=1,smooth=16 ") == GrainMatchConfig(max_sigma=15.9, flat=0, min_count=1, smooth=16)
    assert M.as_config("ring=32,strength=2,flat=255,seed=2147483647") == GrainMatchConfig(ring=32, strength=2.0, flat=255, seed=2 ** 31 - 1)
    cfg = GrainMatchConfig(ring=4)
    assert M.as_config(cfg) is cfg
    with pytest.raises(Exception):
        cfg.ring = 5                                                                                 # frozen
    for bad in ("yes", "static", "affine", "ring", "ring=", "ring=x", "ring=-3", "ring=1.5", "ring=3,ring=4", "size=3", "ring=3;smooth=1", "ring=0",
                "ring=33", "smooth=17", "strength=-0.1", "strength=2.5", "max_sigma=-1", "max_sigma=16", "flat=256", "flat=-1", "min_count=0",
                "seed=-1", "seed=2147483648", "seed=1.5", "strength=nan", "mode=chroma", "mode=", "on,ring=3", "ring=3,", "max_sigma=inf", 3, 1.0,
                ("on",)):
        with pytest.raises(ValueError):
            M.as_config(bad)
    with pytest.raises(ValueError, match="'on', 'off', 'luma', 'rgb', 'mode="):
        M.as_config("sometimes")
    for kw in (dict(mode="chroma"), dict(mode=None), dict(ring=0), dict(ring=33), dict(ring=4.0), dict(ring=True), dict(smooth=-1), dict(smooth=17),
               dict(smooth="2"), dict(strength=-0.01), dict(strength=2.01), dict(strength="1"), dict(max_sigma=-0.5), dict(max_sigma=15.95),
               dict(max_sigma=None), dict(flat=-1), dict(flat=256), dict(flat=2.0), dict(min_count=0), dict(min_count=1.5), dict(seed=-1),
               dict(seed=2 ** 31), dict(seed=0.0), dict(strength=float("nan"))):
        with pytest.raises(ValueError):
            GrainMatchConfig(**kw)
    GrainMatchConfig(ring=1, smooth=0, strength=0, max_sigma=0, flat=0, min_count=1, seed=0)           # the limits themselves are inside
    GrainMatchConfig(ring=32, smooth=16, strength=2, max_sigma=15.9, flat=255, seed=2 ** 31 - 1)
    assert "build-defined" in GrainMatchConfig.__doc__


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_vvgrain_header():
    """grain_hip.SIGNATURES declares every function of include/vvgrain.h with the header's types and in its order, grain_hip.lib() has applied it,
    the version and the limits agree (abiref.check_binding; test_abi_cpu.py: no name could be taken for another part's), and the arguments are
    validated before any device work."""
    from videovanish_amd import grain_hip
    loaded, define = abiref.check_binding(grain_hip, 4)
    raw = open(os.path.join(ROOT, "include", "vvgrain.h")).read()
    assert define("VVG_ABI_VERSION") == 1
    assert define("VVG_MAX_RING") == grain_hip.MAX_RING == M.MAX_RING == 32
    assert define("VVG_BANDS") == grain_hip.BANDS == M.BANDS == 4 and define("VVG_NSUM") == grain_hip.NSUM == M.NSUM == 36
    for formula in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "* 5017 + (1 << 23)) >> 24", "- 1020"):
        assert formula in raw, formula                                                               # the noise is part of the ABI
    # vvtone.h is as it was: four functions, version 1
    tone = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vvtone.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(vvt_[a-z0-9_]+)\s*\(", tone))) == 4 and "#define VVT_ABI_VERSION 1" in tone
    # arguments are validated before anything touches a device: -1 null pointers, sizes, seed and mode, -2 the ring, flat and the feather
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    stats = lambda patch=a, orig=a, mask=a, offs=a, lut=a, sums=a, Hm=4, Wm=4, T=1, H0=8, W0=8, h=4, w=4, ring=4, flat=24: loaded.vvg_ring_grain_stats(
        patch, Hm, Wm, orig, mask, offs, lut, T, H0, W0, h, w, ring, flat, sums, None)
    paste = lambda patch=a, orig=a, mask=a, offs=a, lut=a, amp=a, ids=a, out=a, seed=0, mode=0, Hm=4, Wm=4, T=1, H0=8, W0=8, h=4, w=4, feather=3.0: \
        loaded.vvg_paste_grain_composite(patch, Hm, Wm, orig, mask, offs, lut, amp, ids, seed, mode, T, H0, W0, h, w, feather, out, None)
    for kw in (dict(patch=None), dict(orig=None), dict(mask=None), dict(offs=None), dict(lut=None), dict(sums=None), dict(Hm=0), dict(Wm=-1), dict(T=0),
               dict(H0=0), dict(W0=0), dict(h=0), dict(w=0), dict(h=9), dict(w=9)):
        assert stats(**kw) == -1 and b"vvg_ring_grain_stats" in loaded.vvg_last_error(), kw
    for kw in (dict(ring=0), dict(ring=-1), dict(ring=33), dict(ring=1000), dict(flat=-1), dict(flat=256)):
        assert stats(**kw) == -2 and b"vvg_ring_grain_stats" in loaded.vvg_last_error(), kw
    assert stats(ring=0, T=0) == -1                                                                  # a bad argument before an unsupported one
    for kw in (dict(patch=None), dict(orig=None), dict(mask=None), dict(offs=None), dict(lut=None), dict(amp=None), dict(ids=None), dict(out=None),
               dict(Hm=0), dict(T=-2), dict(H0=0), dict(h=0), dict(w=9), dict(mask=None, feather=0.0), dict(mode=2), dict(mode=-1), dict(seed=-1)):
        assert paste(**kw) == -1 and b"vvg_paste_grain_composite" in loaded.vvg_last_error(), kw
    assert paste(feather=64.5) == -2 and b"vvg_paste_grain_composite" in loaded.vvg_last_error()
    with pytest.raises(ctypes.ArgumentError):
        loaded.vvg_ring_grain_stats(a, 4.0, 4, a, a, a, a, 1, 8, 8, 4, 4, 4, 24, a, None)
    import torch
    z = torch.zeros((2, 4, 4, 3), dtype=torch.uint8)
    offs, lut, ids = torch.zeros((2, 2), dtype=torch.int32), torch.zeros((2, 3, 256), dtype=torch.uint8), torch.zeros(2, dtype=torch.int32)
    for call in (lambda: grain_hip.ring_grain_stats(z, z, z[..., 0].contiguous(), offs, lut, 4, 4, 2, 24),
                 lambda: grain_hip.paste_grain_composite(z, z, z[..., 0].contiguous(), offs, lut, lut, ids, 0, 0, 4, 4, 3.0)):
        with pytest.raises(RuntimeError):
            call()                                                                                   # no CPU fallback


def test_product_sources_of_the_feature():
    """vv_grain is in the one build recipe with its header among the dependencies and reads no environment; the ring has one statement, which
    both users include; the settings import no torch; importing the drop-in resolves no symbol of the feature."""
    grain, _ = abiref.check_sources("vv_grain", "vvgrain.h", "grainmatch")
    tone, shared = (open(os.path.join(abiref.CSRC, f)).read() for f in ("vv_tone.hip", "vv_ring_bits.h"))
    assert "getenv" not in shared
    for user in (grain, tone):
        assert '#include "vv_ring_bits.h"' in user and "vvring::ring_bits<" in user and "__ballot" not in user
    assert shared.count("__ballot(") == 2
    code = ("import diffuerase; from videovanish_amd import grain_hip, tone_hip, hip, grainmatch; "
            "assert grain_hip.PART.dll is None and tone_hip.PART.dll is None and hip.CORE.dll is None; assert diffuerase.last_grain_match is None")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ---- the fit ------------------------------------------------------------------------------------------------------------------------------
def _draw(rng, k):
    """One (sums [T,36], config, kind): counts of every size per band (empty, below min_count, large), Sy equal to Sx, above it (inside or
    beyond the cap) or below it."""
    T = int(rng.integers(1, 9))
    kind = ("equal", "grain", "heavy", "less", "mixed")[k % 5]
    cfg = GrainMatchConfig(mode="rgb" if k % 2 else "luma", smooth=int(rng.choice([0, 0, 1, 4, 9])), strength=float(rng.choice([0.0, 0.5, 1.0, 2.0])),
                           max_sigma=float(rng.choice([0.0, 3.0, 12.0, 15.9])), min_count=int(rng.choice([1, 256, 1000])), seed=k)
    s = np.zeros((T, 3, 4, 3), np.int64)
    for t in range(T):
        if rng.random() < 0.2:
            continue                                                                                 # a frame without a ring
        n = rng.choice([0, 0, 3, 100, 300, 2000, 50000], size=(3, 4))
        sx = (n * rng.uniform(0.0, 40.0, (3, 4))).astype(np.int64)
        grain = {"equal": 0.0, "grain": rng.uniform(0.5, 10.0), "heavy": rng.uniform(14.0, 40.0), "less": 0.0, "mixed": rng.uniform(0.0, 6.0)}[kind]
        sy = sx + (36.0 * n * grain ** 2 * rng.uniform(0.8, 1.2, (3, 4))).astype(np.int64)
        if kind == "less":
            sy = (sx * rng.uniform(0.0, 1.0, (3, 4))).astype(np.int64)
        s[t] = np.stack([n, sx, sy], axis=-1)
    return s.reshape(T, 36), cfg, kind


def test_fit_properties_over_random_draws():
    rng = np.random.default_rng(20261018)
    seen = dict.fromkeys(("equal_zero", "less_zero", "capped", "fitted", "band_fallback", "channel_short", "own_empty", "pooled", "smooth0",
                          "strength0", "table_nonzero", "table_varies"), 0)
    for k in range(300):
        s, cfg, kind = _draw(rng, k)
        T = len(s)
        f = M.fit(s, cfg)
        amp = M.tables(f.sigma_added)
        s4 = s.reshape(T, 3, 4, 3)
        assert f.n.dtype == np.int64 and (f.n == s4[..., 0]).all()
        assert f.n.shape == f.sigma_orig.shape == f.sigma_model.shape == f.sigma_added.shape == (T, 3, 4)
        assert amp.dtype == np.uint8 and amp.shape == (T, 3, 256) and amp.flags["C_CONTIGUOUS"] and M.tables(f.sigma_added[::2]).flags["C_CONTIGUOUS"]
        # the product's fit equals the restatement's: the sigmas closely, the tables bit for bit
        so, sm, sa = R.fit(s, smooth=cfg.smooth, strength=cfg.strength, max_sigma=cfg.max_sigma, min_count=cfg.min_count)
        assert np.allclose(f.sigma_added, sa, rtol=1e-12, atol=0) and np.allclose(f.sigma_orig, so, rtol=1e-12, atol=0)
        assert np.allclose(f.sigma_model, sm, rtol=1e-12, atol=0) and ((f.sigma_added == 0) == (sa == 0)).all()
        assert (amp == R.tables(sa)).all() and (amp == R.tables(f.sigma_added)).all(), k
        # the clamps
        assert (f.sigma_added >= 0).all() and (f.sigma_added <= cfg.max_sigma).all() and (amp <= np.rint(16 * cfg.max_sigma)).all()
        pooled = M.pool(s, cfg.smooth).reshape(T, 3, 4, 3)
        assert (pooled == np.stack([s4[max(0, t - cfg.smooth):t + cfg.smooth + 1].sum(0) for t in range(T)])).all()
        own_empty = s4[..., 0].sum(axis=(1, 2)) == 0
        assert (f.sigma_added[own_empty] == 0).all() and (f.sigma_orig[own_empty] == 0).all() and (amp[own_empty] == 0).all()
        seen["own_empty"] += bool((own_empty & (pooled[..., 0].sum(axis=(1, 2)) > 0)).any())
        chan_n = pooled[..., 0].sum(axis=2)
        short = np.broadcast_to((chan_n < cfg.min_count)[..., None], (T, 3, 4)) & (pooled[..., 0] < cfg.min_count)
        assert (f.sigma_added[short] == 0).all() and (f.sigma_orig[short] == 0).all()
        seen["channel_short"] += bool(short[~own_empty].any())
        # the fallback: a band short of min_count carries its channel's value
        fell = (pooled[..., 0] < cfg.min_count) & ~short & ~own_empty[:, None, None]
        for t, c, b in zip(*np.nonzero(fell)):
            n, sx, sy = (int(v) for v in pooled[t, c].sum(axis=0))
            want = min(cfg.strength * np.sqrt(max(sy - sx, 0) / (36.0 * n)), cfg.max_sigma)
            assert np.isclose(f.sigma_added[t, c, b], want, rtol=1e-12, atol=0) and (f.sigma_added[t, c][fell[t, c]] == f.sigma_added[t, c, b]).all()
        seen["band_fallback"] += bool(fell.any())
        if kind == "equal":                                                                          # Sx == Sy: exactly nothing
            assert (f.sigma_added == 0.0).all() and (amp == 0).all() and (f.sigma_orig == f.sigma_model).all()
            seen["equal_zero"] += bool((f.sigma_orig > 0).any())
        if kind == "less":                                                                           # the model noisier than the original: nothing
            assert (f.sigma_added == 0.0).all() and (amp == 0).all()
            seen["less_zero"] += bool((f.sigma_model > f.sigma_orig).any())
        if cfg.strength == 0:
            assert (f.sigma_added == 0.0).all()
            seen["strength0"] += 1
        live = f.sigma_added > 0
        seen["capped"] += bool(cfg.max_sigma > 0 and (f.sigma_added == cfg.max_sigma).any())
        seen["fitted"] += bool((live & (f.sigma_added < cfg.max_sigma)).any())
        # pooling equals fitting the summed sums: frame t's row is the fit of one frame holding the pooled sums
        one_cfg = GrainMatchConfig(smooth=0, strength=cfg.strength, max_sigma=cfg.max_sigma, min_count=cfg.min_count)
        for t in np.nonzero(~own_empty)[0]:
            one = M.fit(pooled[t].reshape(1, 36), one_cfg)
            assert (one.sigma_added[0] == f.sigma_added[t]).all() and (one.sigma_orig[0] == f.sigma_orig[t]).all()
        if cfg.smooth == 0:
            seen["smooth0"] += bool(live.any())
        else:
            seen["pooled"] += bool(live.any() and T > 1 and (pooled != s4).any())
        seen["table_nonzero"] += bool(amp.any())
        seen["table_varies"] += bool((amp.max(axis=-1) != amp.min(axis=-1)).any())
    assert all(v >= 10 for v in seen.values()), seen


def test_tables_interpolate_between_the_band_centres():
    sig = np.array([[[1.0, 3.0, 3.0, 0.0], [0.0, 0.0, 0.0, 0.0], [15.9, 15.9, 15.9, 15.9]]])
    amp = M.tables(sig)
    assert amp.shape == (1, 3, 256) and (amp == R.tables(sig)).all()
    assert (amp[0, 0, :33] == 16).all() and amp[0, 0, 64] == 32 and (amp[0, 0, 96:161] == 48).all() and amp[0, 0, 192] == 24 and (amp[0, 0, 224:] == 0).all()
    assert amp[0, 0, 34] == 17 and amp[0, 0, 33] == 16                                               # 16 * (1 + 2 / 64) = 16.5 -> 16, halves to even
    assert (np.diff(amp[0, 0, :97].astype(int)) >= 0).all() and (np.diff(amp[0, 0, 160:].astype(int)) <= 0).all()
    assert not amp[0, 1].any() and (amp[0, 2] == 254).all()
    assert not M.tables(np.zeros((2, 3, 4))).any()


# ---- recovery, on the restatement alone ---------------------------------------------------------------------------------------------------
def test_reference_recovers_a_known_grain():
    """The model's frame is the smooth restoration clip, the original that clip plus Gaussian noise of sigma 2, 4, 8 (12 seeds each): the fitted
    sigma_added of every channel and band comes back to sigma, and so does Immerkaer's estimate deep inside the mask of the composite, within
    1.5 times the worst relative deviation recorded in grainmatch_ref.MEASURED_DEVIATION; sigma 0 gives exactly 0 and the plain composite.
    The product's fit gives the same numbers from the restatement's sums."""
    cfg = GrainMatchConfig()
    offs = np.zeros((1, 2), np.int32)
    for sigma in (0,) + R.RECOVERY_SIGMAS:
        worst = {"fit": 0.0, "inside": 0.0}
        lo, hi = np.inf, -np.inf
        for s in R.RECOVERY_SEEDS:
            orig, x, mask = R.recovery_clip(s, sigma)
            _, H, W = mask.shape
            out, sums, so, sm, sa = R.apply(x, orig, mask, offs, H, W, 3.0, [0])
            n = sums.reshape(3, 4, 3)[..., 0]
            assert (n.sum(axis=1) > 1500).all()
            f = M.fit(sums, cfg)
            assert np.allclose(f.sigma_added, sa, rtol=1e-12, atol=0) and (M.tables(f.sigma_added) == R.tables(sa)).all()
            if sigma == 0:
                assert (orig == x).all() and (sa == 0.0).all() and (f.sigma_added == 0.0).all() and (so == sm).all()
                assert (out == x).all()
                continue
            inside = R.inside_estimate(out[0], x[0], mask[0])
            lo, hi = min(lo, sa.min()), max(hi, sa.max())
            worst["fit"] = max(worst["fit"], float(np.abs(sa / sigma - 1).max()))
            worst["inside"] = max(worst["inside"], float(np.abs(inside / sigma - 1).max()))
        if sigma:
            rec = {k: R.MEASURED_DEVIATION[k][sigma] for k in worst}
            print(f"sigma {sigma}: sigma_added {lo:.3f} .. {hi:.3f}; worst relative deviation: fit {worst['fit']:.4f} (recorded {rec['fit']}), "
                  f"inside the mask {worst['inside']:.4f} (recorded {rec['inside']})")
            for k in worst:
                assert worst[k] <= 1.5 * rec[k], (sigma, k, worst[k])


# ---- the noise, on the restatement (the GPU equals it byte for byte) ----------------------------------------------------------------------
def _noise_fields(mode, seed=0, frames=range(8)):
    """d [8,128,128,3] on a flat frame of 128 with amplitude 64 (sigma 4)."""
    img = np.full((128, 128, 3), 128, np.uint8)
    amp = np.full((3, 256), 64, np.uint8)
    return np.stack([R.grain(img, amp, R.noise(seed, t, 128, 128, mode))[1] for t in frames])


@pytest.mark.parametrize("mode", ["luma", "rgb"])
def test_noise_is_white_and_of_the_asked_size(mode):
    d = _noise_fields(mode).astype(np.float64)
    sd = np.sqrt(16 + 1 / 12)
    for c in range(3):
        v = d[..., c]
        N = v.size
        assert abs(v.mean()) <= 4 * sd / np.sqrt(N), (c, v.mean())
        assert abs(v.std() / sd - 1) < 0.02, (c, v.std())
        z = (v - v.mean()) / v.std()
        for name, a, b in (("x", z[:, :, 1:], z[:, :, :-1]), ("y", z[:, 1:], z[:, :-1]), ("t", z[1:], z[:-1])):
            r = float((a * b).mean())
            assert abs(r) < 4 / np.sqrt(a.size), (c, name, r)
    if mode == "luma":
        assert (d[..., 0] == d[..., 1]).all() and (d[..., 0] == d[..., 2]).all()
    else:
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert (d[..., a] != d[..., b]).mean() > 0.8
            za, zb = d[..., a] - d[..., a].mean(), d[..., b] - d[..., b].mean()
            assert abs((za * zb).mean() / (za.std() * zb.std())) < 4 / np.sqrt(za.size)


def test_noise_depends_on_seed_and_frame_and_on_nothing_else():
    base = _noise_fields("luma", frames=[0, 1])
    assert (base[0] != base[1]).mean() > 0.8                                                         # another frame id
    assert (_noise_fields("luma", seed=1, frames=[0])[0] != base[0]).mean() > 0.8                      # another seed
    assert (_noise_fields("luma", frames=[1])[0] == base[1]).all()                                   # stateless
    s = R.noise(5, 3, 40, 50, "rgb")
    assert s.min() >= -1020 and s.max() <= 1020 and (R.noise(5, 3, 40, 50, "rgb") == s).all()
    # the frame position is the key: a frame of another width is another field, the same frame is the same field whatever is cut from it
    assert (R.noise(5, 3, 40, 51, "rgb")[:, :50] != s).mean() > 0.8
    # splitmix64's first output for the state 0 is a published value: the key 0 must hash to it
    z = 0x9E3779B97F4A7C15
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    z ^= z >> 31
    assert z == 0xE220A8397B1DCDAF and R.noise(0, 0, 1, 1, "luma")[0, 0, 0] == sum(z.to_bytes(8, "little")) - 1020
    # an amplitude of zero adds nothing; the shift is a floor, so the rounding is to nearest with halves up
    img = np.full((4, 4, 3), 7, np.uint8)
    assert (R.grain(img, np.zeros((3, 256), np.uint8), R.noise(0, 0, 4, 4, "luma"))[0] == img).all()
    assert 255 * 1020 * 5017 + (1 << 23) < 2 ** 31


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_precedence_argument_configure_environment(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_GRAIN_MATCH", raising=False)
    try:
        diffuerase.configure()
        assert diffuerase.grain_match_config() is None
        monkeypatch.setenv("VV_GRAIN_MATCH", "ring=9")
        assert diffuerase.grain_match_config() == GrainMatchConfig(ring=9)
        diffuerase.configure(grain_match="rgb")
        assert diffuerase.grain_match_config() == GrainMatchConfig(mode="rgb")
        assert diffuerase.grain_match_config("on") == GrainMatchConfig()
        assert diffuerase.grain_match_config("off") is None and diffuerase.grain_match_config(False) is None    # none whatever else is set
        diffuerase.configure(grain_match="off")
        assert diffuerase.grain_match_config() is None                                                     # configure("off") beats the environment
        diffuerase.configure()
        assert diffuerase.grain_match_config() == GrainMatchConfig(ring=9)                                 # configure() resets
        cfg = GrainMatchConfig(smooth=0)
        diffuerase.configure(grain_match=cfg)
        assert diffuerase.grain_match_config() is cfg
        with pytest.raises(ValueError):
            diffuerase.configure(grain_match="sometimes")
        assert diffuerase.grain_match_config() is cfg                                                      # a refused value changes nothing
        monkeypatch.setenv("VV_GRAIN_MATCH", "sometimes")
        diffuerase.configure()
        with pytest.raises(ValueError):
            diffuerase.grain_match_config()
    finally:
        diffuerase.configure()


def test_grain_match_refuses_the_reference_early_return(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_GRAIN_MATCH", raising=False)
    f = [np.zeros((8, 8, 3), np.uint8)] * 2
    for value in ("on", "rgb", "ring=4", GrainMatchConfig(), True):
        with pytest.raises(ValueError, match="grain_match="):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, grain_match=value)
    monkeypatch.setenv("VV_GRAIN_MATCH", "on")
    with pytest.raises(ValueError, match="grain_match="):
        diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)
    with pytest.raises(TypeError):
        diffuerase.run_infill_on_frames(f, f, grainmatch="on")
    assert diffuerase.last_grain_match is None


def test_grain_report_assembles_spans_and_windows():
    from videovanish_amd import infill
    one = lambda K, T, v: infill.GrainMatchReport(np.full((K, T, 3, 4), v, np.int64), *(np.full((K, T, 3, 4), float(v)) for _ in range(3)))
    rep = infill.grain_report([one(1, 3, 5), one(2, 2, 7)], [(1, 4), (6, 8)], 9)
    assert rep.n.shape == rep.sigma_orig.shape == rep.sigma_model.shape == rep.sigma_added.shape == (2, 9, 3, 4) and rep.n.dtype == np.int64
    assert rep.n[:, :, 0, 0].tolist() == [[0, 5, 5, 5, 0, 0, 7, 7, 0], [0, 0, 0, 0, 0, 0, 7, 7, 0]] and (rep.n == rep.n[:, :, :1, :1]).all()
    for field in rep[1:]:
        assert field.dtype == np.float64 and (field == rep.n).all()
    empty = infill.grain_report([], [], 4)
    assert empty.n.shape == (1, 4, 3, 4) and not any(f.any() for f in empty)
    assert infill.grain_report([], [], 4, K=3).sigma_added.shape == (3, 4, 3, 4)


def test_run_spans_hands_each_clip_its_first_frame():
    """frame0 is what keys the noise of a span's frames on their index in the call; without the flag body is called as before."""
    from videovanish_amd import infill
    frames = [np.full((2, 2, 3), t, np.uint8) for t in range(9)]
    seen = []

    def body(f, d, prior, prog, **kw):
        seen.append((len(f), kw))
        return list(f)

    infill.run_spans(frames, frames, None, [(1, 4), (6, 9)], body, None, frame0=True)
    infill.run_spans(frames, frames, None, [(0, 9)], body, None, frame0=True)
    infill.run_spans(frames, frames, None, [(1, 4)], body, None)
    assert seen == [(3, {"frame0": 1}), (3, {"frame0": 6}), (9, {"frame0": 0}), (3, {})]


def test_cli_grain_match_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
    """tests/test_cli_cpu.py's stub: frame I/O and the hot path replaced."""
    import diffuerase
    from videovanish_amd import infill
    calls = []
    videos = {"mask.mkv": [np.zeros((16, 24, 3), np.uint8)] * 3}
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda path, start=0, max_frames=-1: ([f.copy() for f in videos[path]], 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    rep = infill.grain_report([], [], 3)
    rep.sigma_added[0, 1, 0] = (0.0, 2.5, 0.0, 0.0)
    rep.sigma_added[0, 2, 2, 3] = 3.257

    def fake(frames, masks, **kw):
        calls.append(kw)
        diffuerase.last_grain_match = rep if "grain_match" in kw else None
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 3
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    monkeypatch.setattr(sys, "argv", argv)
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None} and capsys.readouterr().out == ""                      # a default call passes no keyword, prints nothing
    for value in ("on", "rgb", "mode=rgb,ring=8,strength=0.8,seed=3"):
        monkeypatch.setattr(sys, "argv", argv + ["--grain-match", value, "--roi", "static"])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "grain_match": value, "roi": "static"}
        out = capsys.readouterr().out
        assert out.count("\n") == 1 and out == "grain match: grain added in 2 of 3 frames, largest sigma 3.26\n"
    monkeypatch.setattr(sys, "argv", argv + ["--grain-match", "luma", "--tone-match", "on"])
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None, "grain_match": "luma", "tone_match": "on"}
    capsys.readouterr()
    for bad in ("off", "yes", "ring=x", "ring=40", "flat=300"):
        monkeypatch.setattr(sys, "argv", argv + ["--grain-match", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_grain_match", None)
