"""Clean-plate exposure matching on the CPU: the settings, the binding of include/platetone.h, the rules' restatement (tests/platetone_ref.py) on
the synthetic drift and flicker clips, the product's integer fit against the restatement's fractions, the orchestration with the device
functions replaced by the restatement, configuration and CLI."""
import ctypes
import inspect
import os
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abiref  # noqa: E402
import platefill_ref as R  # noqa: E402
import platetone_ref as E  # noqa: E402

from videovanish_amd import platetone as PT  # noqa: E402
from videovanish_amd.platefill import PlateFillConfig  # noqa: E402
from videovanish_amd.plategrain import PlateGrainConfig  # noqa: E402
from videovanish_amd.platetone import PlateToneConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIPS = {"drift": dict(drift_q4=4), "flicker": dict(flicker_pct=8), "both": dict(drift_q4=4, flicker_pct=8)}
# What the four seeds fill with the option, as a share of what the same clip fills without drift: drift 100 % each,
# flicker 100, 100, 98.8, 100 %, both 100 % each.  The floors stand 10 points under the smallest.
SHARE_FLOOR = {"drift": 0.90, "flicker": 0.887, "both": 0.90}


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_spellings_and_config():
    assert PT.SPELLINGS == ("on",) and PT.MODES == ("affine", "gain", "offset")
    for off in (None, False, "off", "none", "", " OFF "):
        assert PT.as_config(off) is None
    d = PlateToneConfig()
    assert PT.as_config("on") == PT.as_config(" On ") == PT.as_config(True) == d
    assert dict(mode=d.mode, ring=d.ring, floor=d.floor, min_pixels=d.min_pixels, max_gain=d.max_gain, max_offset=d.max_offset) == E.DEFAULTS
    assert PT.as_config("mode=affine,ring=32,floor=16,min_pixels=1024,max_gain=25,max_offset=32") == d
    assert PT.as_config(" ring = 3 ") == PlateToneConfig(ring=3) and PT.as_config("mode=gain") == PlateToneConfig(mode="gain")
    assert PT.as_config("max_offset=255,max_gain=100,floor=127,ring=64,min_pixels=2147483647,mode=offset") == PlateToneConfig("offset", 64, 127, 2 ** 31 - 1, 100, 255)
    assert PT.as_config("ring=0,floor=0,max_gain=0,max_offset=0,min_pixels=1") == PlateToneConfig("affine", 0, 0, 1, 0, 0)
    cfg = PlateToneConfig(ring=2)
    assert PT.as_config(cfg) is cfg
    for bad in ("yes", "ring", "ring=", "ring=x", "ring=-1", "ring=1.5", "ring=2,ring=3", "size=3", "ring=2;floor=1", "ring=65", "floor=128", "min_pixels=0",
                "min_pixels=2147483648", "max_gain=101", "max_offset=256", "mode=linear", "mode=", "on,ring=2", "ring=2,", "affine", 3, 1.0, ("on",)):
        with pytest.raises(ValueError):
            PT.as_config(bad)
    for kw in (dict(ring=-1), dict(ring=65), dict(floor=128), dict(min_pixels=0), dict(max_gain=101), dict(max_offset=256), dict(ring=2.0), dict(floor=True),
               dict(max_gain="25"), dict(mode="histogram"), dict(mode=None)):
        with pytest.raises(ValueError):
            PlateToneConfig(**kw)


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_platetone_header():
    """platetone_bind.SIGNATURES declares every function of include/platetone.h with the header's types and in its order, lib() has applied it,
    the version and the limits agree (abiref.check_binding); the limits refuse before any device work; the vve_ prefix and every name belong to
    no part of abiref.parts() (what test_abi_cpu.py's walk does for the parts of its table)."""
    from videovanish_amd import platetone_bind as B
    loaded, define = abiref.check_binding(B, 6)
    assert B.EXPORTS == ["vve_abi_version", "vve_last_error", "vve_mean_plane", "vve_moments", "vve_apply", "vve_restore"] and define("VVE_ABI_VERSION") == 1
    assert (define("VVE_MAX_T"), define("VVE_MAX_PIXELS"), define("VVE_MAX_RING"), define("VVE_MAX_FLOOR"), define("VVE_MAX_GAIN"), define("VVE_MAX_OFFSET"),
            define("VVE_NSUM")) == (B.MAX_T, B.MAX_PIXELS, B.MAX_RING, B.MAX_FLOOR, B.MAX_GAIN, B.MAX_OFFSET, B.NSUM) == \
        (PT.MAX_T, PT.MAX_PIXELS, PT.MAX_RING, PT.MAX_FLOOR, PT.MAX_GAIN, PT.MAX_OFFSET, PT.NSUM) == (65535, 1 << 24, 64, 127, 100, 255, 12)
    # Nothing can be launched here: every pointer is host memory and every call below is refused before the first device call.
    buf = (ctypes.c_char * 64)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 16
    mean = lambda T=2, H=8, W=8, floor=16, f=a, n=a: loaded.vve_mean_plane(f, a, T, H, W, floor, a, a, n, None)
    mom = lambda T=2, H=8, W=8, s=a: loaded.vve_moments(a, a, a, T, H, W, s, None)
    app = lambda T=2, H=8, W=8, out=b, tab=a: loaded.vve_apply(a, tab, a, T, H, W, out, None)
    res = lambda T=2, H=8, W=8, out=b, tab=a: loaded.vve_restore(a, a + 32, a, a, tab, T, H, W, out, None)
    for fn, name in ((mean, b"vve_mean_plane:"), (mom, b"vve_moments:"), (app, b"vve_apply:"), (res, b"vve_restore:")):
        for bad in (dict(T=0), dict(T=-1), dict(H=0), dict(W=0)):
            assert fn(**bad) == -1 and loaded.vve_last_error().startswith(name), (name, bad)
        for bad in (dict(T=65536), dict(H=4097, W=4096), dict(H=1 << 15, W=1 << 15)):
            assert fn(**bad) == -2 and loaded.vve_last_error().startswith(name), (name, bad)
    assert mean(floor=-1) == -1 and mean(f=None) == -1 and mean(n=None) == -1 and mean(floor=128) == -2 and b"floor" in loaded.vve_last_error()
    assert mom(s=None) == -1 and app(out=None) == -1 and res(out=None) == -1 and app(tab=None) == -1 and res(tab=None) == -1
    assert app(out=a) == -1 and b"out is not frames" in loaded.vve_last_error()                        # never in place
    assert res(out=a) == -1 and res(out=a + 32) == -1 and b"neither orig nor filled" in loaded.vve_last_error()
    assert app(tab=a + 1) == -1 and res(tab=a + 2) == -1                                               # the tables are read as words
    with pytest.raises(ctypes.ArgumentError):
        mean(floor=2.0)
    import torch
    f, z = torch.zeros((2, 4, 4, 3), dtype=torch.uint8), torch.zeros((2, 4, 4), dtype=torch.uint8)
    tab = torch.zeros((2, 3, 256), dtype=torch.uint8)
    for call in (lambda: B.mean_plane(f, z, 16), lambda: B.moments(f, f[0], z[0]), lambda: B.apply(f, tab, z[:, 0, 0]), lambda: B.restore(f, f, z, z, tab)):
        with pytest.raises(RuntimeError):                                                               # no CPU fallback
            call()
    # the part stands outside abiref.PARTS: its prefix and names are checked against every part here
    assert "platetone_bind" not in abiref.PARTS and abiref.part_of(B) is B.PART and B.PART.header == "platetone.h"
    import re
    assert re.fullmatch(r"vv[a-z]_", B.PART.prefix)
    names = set(B.SIGNATURES)
    for module, part in abiref.parts():
        assert part.prefix != B.PART.prefix and part.header != B.PART.header, module.__name__
        assert not names & set(module.SIGNATURES), module.__name__
        assert not [n for n in module.SIGNATURES if n.startswith(B.PART.prefix)], module.__name__
    assert all(n.startswith("vve_") for n in names)


def test_product_sources_of_the_feature():
    """The kernels live in a unit of their own, in the one recipe with the header among the dependencies; no environment, no scratch array indexed
    at run time; the settings import neither torch nor numpy; importing the drop-in resolves no vve_ symbol."""
    kernel, txt = abiref.check_sources("vv_platetone", "platetone.h", "platetone")
    for fn in ("vve_mean_plane", "vve_moments", "vve_apply", "vve_restore"):
        assert f'extern "C" int {fn}(' in kernel
    assert '#include "vv_wave_bytes.h"' in kernel and "wave_sum64" in kernel and "load_px<VEC>" in kernel
    assert "numpy" not in txt and "import ctypes" not in txt
    header = open(os.path.join(ROOT, "include", "platetone.h")).read()
    for rule in ("1. Crop and support", "2. Mean image", "3. Moments over U", "4. Fit", "5. Tables", "6. Segment paths", "7. With the alignment"):
        assert rule in header
    code = ("import diffuerase; from videovanish_amd import platetone_bind, plate_hip, hip; "
            "assert platetone_bind.PART.dll is None and plate_hip.PART.dll is None and hip.CORE.dll is None; "
            "assert diffuerase.plate_tone_config() is None and diffuerase.last_plate_tone is None")
    env = {k: v for k, v in os.environ.items() if k not in ("VV_PLATE_TONE", "VV_PLATE_FILL")}
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)


# ---- the rules on synthetic clips -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("kind", list(CLIPS))
def test_drift_and_flicker_fill_again(kind, seed):
    """1 level per frame of drift, +-8 % of flicker, both: the plain fill fills nothing (DESIGN.md section 16's stated limit); with the option
    the clip fills what it fills without drift, and every filled byte lies near the noise-free background of its own frame: the source's noise
    (at most NOISE levels) scaled by the ratio of the two frames' gains, 1 level for the fit and the clip's own rounding, 2 for the rounding in
    G, then B."""
    frames, masks, clean, boxm, logom = E.exposure_clip(seed=seed, **CLIPS[kind])
    plain, pd, pc = R.plate_fill(frames, masks)
    assert (plain == frames).all() and (pd == masks).all() and not pc[:, 0].any()                      # nothing is filled: the stated limit
    still, smasks, sclean, _, _ = E.exposure_clip(seed=seed)
    base = int(R.plate_fill(still, smasks)[2][:, 0].sum())
    out, d2, counts, infos = E.plate_fill(frames, masks)
    info, = infos
    went = (masks != 0) & (d2 == 0)
    filled = int(counts[:, 0].sum())
    err = float(np.abs(out.astype(np.float64) - clean)[went].max())
    pct = CLIPS[kind].get("flicker_pct", 0)
    bound = E.NOISE * (100 + pct) / (100 - pct) + 1 + 2
    print(f"{kind} clip, seed {seed}: support {info['n']}, {filled} px filled of {base} without drift ({100.0 * filled / base:.1f} %), "
          f"largest |filled - clean| {err:.2f} (bound {bound:.2f})")
    assert info["path"] == "matched" and info["n"] >= 1024 and base > 5000
    assert filled > 0 and filled == went.sum() and filled >= SHARE_FLOOR[kind] * base
    assert err <= bound
    assert (out[~went] == frames[~went]).all()                                                         # a pixel that is not filled keeps its bytes
    assert (counts[:, 1] == (d2 != 0).reshape(len(d2), -1).sum(1)).all()
    # both tables of every frame and channel are monotone
    assert (np.diff(info["G"].astype(np.int64), axis=-1) >= 0).all() and (np.diff(info["B"].astype(np.int64), axis=-1) >= 0).all()


def test_gain_mode_on_the_additive_clip_is_recorded():
    """A drift that adds is no gain: mode=gain on the additive clip fills less than affine (recorded, not asserted: DESIGN.md section 23), and
    mode=offset fills the flicker clip worse still."""
    for kind in ("drift", "flicker"):
        for mode in PT.MODES:
            got = [int(E.plate_fill(*E.exposure_clip(seed=seed, **CLIPS[kind])[:2], tone=dict(mode=mode))[2][:, 0].sum()) for seed in range(2)]
            print(f"{kind} clip, mode={mode}: {got} px filled at seeds 0, 1")


def test_a_still_clip_is_identity_and_an_unfit_segment_is_left_alone():
    frames, masks, clean, _, _ = E.exposure_clip(seed=0, a=0)                                           # no drift, no grain: R is every frame
    out, d2, counts, (info,) = E.plate_fill(frames, masks)
    want = R.plate_fill(frames, masks)
    assert info["path"] == "identity" and info["identity"].all() and (info["G"] == E.IDENT).all() and (info["B"] == E.IDENT).all()
    assert all(f == (1, 0) for fs in info["fits"] for f in fs)
    assert (out == want[0]).all() and (d2 == want[1]).all() and (counts == want[2]).all() and counts[:, 0].sum() > 5000
    # fewer than min_pixels of support: unfit, the plain fill (which fills nothing under the drift)
    frames, masks, clean, _, _ = E.exposure_clip(seed=0, drift_q4=4)
    n = E.plate_fill(frames, masks)[3][0]["n"]
    for min_pixels, path in ((n, "matched"), (n + 1, "unfit")):
        out, d2, counts, (info,) = E.plate_fill(frames, masks, tone=dict(min_pixels=min_pixels))
        assert info["path"] == path and info["n"] == n
        assert (path == "unfit") == (out == frames).all() == (not counts[:, 0].any())
    assert info["identity"].all() and (info["G"] == E.IDENT).all()
    # the floor gate: equality counts
    f = np.full((4, 2, 4, 3), 100, np.uint8)
    f[:, 0, 0], f[:, 0, 1], f[:, 0, 2], f[:, 0, 3] = 16, 15, 239, 240
    Rm, U, n = E.mean_plane(f, np.zeros((4, 2, 4), bool), 16)
    assert U.tolist() == [[True, False, True, False], [True] * 4] and n == 6
    f[1, 1, 0, 1] = 103                                                                                 # the mean of 100, 103, 100, 100 rounds up to 101
    assert E.mean_plane(f, np.zeros((4, 2, 4), bool), 16)[0][1, 0].tolist() == [100, 101, 100]
    f[1, 1, 0, 1] = 101                                                                                 # 100.25 rounds down
    assert E.mean_plane(f, np.zeros((4, 2, 4), bool), 16)[0][1, 0].tolist() == [100, 100, 100]


def _same_tables(fit, Gt, Bt, ident):
    T = len(ident)
    return (np.frombuffer(fit.fwd, np.uint8).reshape(T, 3, 256) == Gt).all() and (np.frombuffer(fit.back, np.uint8).reshape(T, 3, 256) == Bt).all() and \
        (np.frombuffer(fit.identity, np.uint8) != 0).tolist() == ident.tolist()


def test_the_integer_fit_is_the_restatement_in_fractions():
    """platetone.fit_segment (integers) against platetone_ref.fit_tables (fractions.Fraction): the clips' sums in every mode, sums that clamp the
    gain both ways and the offset both ways, tables that clamp at 0 and at 255, the fall-back to gain on a flat support, Sr == 0."""
    from fractions import Fraction
    for kind in CLIPS:
        frames, masks, _, _, _ = E.exposure_clip(seed=1, **CLIPS[kind])
        info = E.plate_fill(frames, masks)[3][0]
        for mode in PT.MODES:
            for more in ({}, dict(max_gain=3, max_offset=2), dict(max_gain=0), dict(max_offset=0)):
                cfg = PlateToneConfig(mode=mode, **more)
                fit = PT.fit_segment(info["n"], np.array(info["sums"], np.int64), cfg)
                Gt, Bt, ident, fits, ok = E.fit_tables(info["n"], info["sums"], mode=mode, **more)
                assert ok and fit.fit and fit.n == info["n"] and _same_tables(fit, Gt, Bt, ident), (kind, mode, more)
                assert all((Fraction(p.an, p.ad), Fraction(p.bn, p.bd)) == q for ps, qs in zip(fit.fits, fits) for p, q in zip(ps, qs))
    # hand-made sums: n = 4 pixels with R = 10, 20, 30, 40 (Sr = 100, Srr = 3000, D = 2000 >= 16 n n = 256) and v = a R + b exactly
    n, Sr, Srr = 4, 100, 3000
    rows = []
    for a_num, a_den, b in ((1, 1, 0), (2, 1, 0), (1, 2, 0), (1, 1, 40), (1, 1, -40), (5, 4, 32), (4, 5, -32), (5, 4, 33), (9, 8, -3)):
        v = [Fraction(a_num * r, a_den) + b for r in (10, 20, 30, 40)]
        rows.append([int(sum(v))] * 3 + [int(sum(x * r for x, r in zip(v, (10, 20, 30, 40))))] * 3 + [Sr] * 3 + [Srr] * 3)
    for mode in PT.MODES:
        for more in ({}, dict(max_gain=100, max_offset=255)):
            fit = PT.fit_segment(n, rows, PlateToneConfig(mode=mode, min_pixels=1, **more))
            Gt, Bt, ident, fits, ok = E.fit_tables(n, rows, mode=mode, min_pixels=1, **more)
            assert _same_tables(fit, Gt, Bt, ident), (mode, more)
            if mode == "affine":
                assert ident.tolist() == [True] + [False] * 8
                if more:                                                                                # a = 2: the forward table halves, the back table clamps at 255
                    assert fits[1][0] == (2, 0) and Bt[1, 0, 127] == 254 and Bt[1, 0, 128:].tolist() == [255] * 128 and Gt[1, 0, 255] == 128
                    assert fits[3][0] == (1, 40) and Gt[3, 0, :41].tolist() == [0] * 41 and Bt[3, 0, 215:].tolist() == [255] * 41       # clamps at 0 and at 255
                    assert fits[4][0] == (1, -40) and Bt[4, 0, :41].tolist() == [0] * 41 and Gt[4, 0, 215:].tolist() == [255] * 41
                else:                                                                                   # the clamps: gain to 5/4 and 4/5, the offset to +-32
                    assert fits[1][0][0] == Fraction(5, 4) and fits[2][0][0] == Fraction(4, 5) and fits[3][0] == (1, 32) and fits[4][0] == (1, -32)
                    assert fits[5][0] == (Fraction(5, 4), 32) and fits[6][0] == (Fraction(4, 5), -32) and fits[7][0][1] == 32
    # a flat support (D < 16 n n) takes the gain; Sr == 0 is gain 1
    flat = [[440, 440, 440, 11000 + 2, 11000 + 2, 11000 + 2, 100, 100, 100, 2500 + 2, 2500 + 2, 2500 + 2]]
    fit = PT.fit_segment(4, flat, PlateToneConfig(min_pixels=1))
    assert fit.fits[0][0] == PT.Fit(125, 100, 0, 1) and _same_tables(fit, *E.fit_tables(4, flat, min_pixels=1)[:3])
    fit = PT.fit_segment(4, [[0] * 12], PlateToneConfig(min_pixels=1, floor=0))
    assert fit.all_identity and fit.fits[0][0] == PT.Fit(1, 1, 0, 1) and _same_tables(fit, *E.fit_tables(4, [[0] * 12], min_pixels=1)[:3])
    unfit = PT.fit_segment(3, [()] * 5, PlateToneConfig(min_pixels=4))
    assert not unfit.fit and unfit.all_identity and unfit.fwd == unfit.back == PT.IDENTITY * 15 and unfit.n == 3


# ---- orchestration ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def host_kernels(monkeypatch):
    """infill.plate_fill with every device call replaced by the restatements on host tensors; the calls made are recorded."""
    import torch

    import plategrain_ref as G
    from videovanish_amd import hip, infill, mask_hip, plate_hip, plategrain_hip, platetone_bind
    calls = []
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))

    def mask_bbox(m):
        out = np.zeros((len(m), 4), np.int32)
        for i, f in enumerate(m.numpy()):
            ys, xs = np.nonzero(f.any(1))[0], np.nonzero(f.any(0))[0]
            if len(ys):
                out[i] = ys[0], xs[0], ys[-1] + 1, xs[-1] + 1
        return t(out)

    def stats(f, ns, occ, min_samples, tol):
        calls.append(("stats", tuple(f.shape)))
        n, S1, S2 = R.stats(f.numpy(), ns.numpy() != 0)
        return t(R.steady(n, S1, S2, min_samples, tol).astype(np.uint8)), t(n.astype(np.int32)), t(S1.astype(np.int32))

    def _sources(f, d, ns, st, n, s1, tol, outlier, max_gap):
        us = R.usable(f.numpy(), ns.numpy() != 0, st.numpy() != 0, n.numpy().astype(np.int64), s1.numpy().astype(np.int64), tol, outlier)
        src = R.sources(d.numpy(), us, max_gap)
        return us, src, t(((d.numpy() != 0) & (src == R.NONE)).astype(np.uint8) * 255)

    def sources(f, d, ns, occ, st, n, s1, tol, outlier, max_gap):
        us, src, r0 = _sources(f, d, ns, st, n, s1, tol, outlier, max_gap)
        return t(src.view(np.int16)), r0

    def live_sources(f, d, ns, occ, st, n, s1, tol, outlier, max_gap, depth, reach):
        calls.append(("vvl_sources", depth, reach))
        us, src, r0 = _sources(f, d, ns, st, n, s1, tol, outlier, max_gap)
        return t(src.view(np.int16)), t(G.live_sources(src, us, depth, reach, max_gap)[0].view(np.int16)), r0

    def fill(f, d, keep, occ, src):
        dn, s = d.numpy() != 0, src.numpy().view(np.uint16)
        left = dn & (keep.numpy() != 0)
        go = dn & ~left
        tt, yy, xx = np.nonzero(go)
        f.numpy()[tt, yy, xx] = f.numpy()[s[tt, yy, xx].astype(np.int64), yy, xx]
        T = len(dn)
        return t(left.astype(np.uint8) * 255), t(np.stack([go.reshape(T, -1).sum(1), left.reshape(T, -1).sum(1)], 1).astype(np.int64))

    def mean_plane(f, ns, floor):
        calls.append(("mean_plane", tuple(f.shape), floor))
        Rm, U, n = E.mean_plane(f.numpy(), ns.numpy() != 0, floor)
        return t(Rm), t(U.astype(np.uint8)), torch.tensor([n], dtype=torch.int64)

    def moments(f, mean, support):
        calls.append(("moments",))
        return t(np.array(E.moments(f.numpy(), mean.numpy(), support.numpy() != 0), np.int64))

    def apply(f, fwd, identity, out=None):
        calls.append(("apply", identity.numpy().tolist()))
        return t(E.lut(f.numpy(), fwd.numpy()))

    def restore(orig, filled, d, d2, back):
        calls.append(("restore",))
        went = (d.numpy() != 0) & (d2.numpy() == 0)
        out = orig.numpy().copy()
        out[went] = E.lut(filled.numpy(), back.numpy())[went]
        return t(out)

    monkeypatch.setattr(hip, "mask_bbox", mask_bbox)
    monkeypatch.setattr(hip, "mask_tile_union", lambda m, tile: t(np.ones((1, 1), np.uint8)))
    monkeypatch.setattr(hip, "mask_collapse_dilate", lambda m, iters: t(R.dilate(m.numpy()[..., 0] != 0, iters).astype(np.uint8) * 255))
    monkeypatch.setattr(mask_hip, "time_bridge_grow", lambda m, bridge, grow: (t(R.not_sample(m.numpy(), grow).astype(np.uint8) * 255), None))
    monkeypatch.setattr(plate_hip, "stats", stats)
    monkeypatch.setattr(plate_hip, "sources", sources)
    monkeypatch.setattr(plate_hip, "fill", fill)
    monkeypatch.setattr(plategrain_hip, "sources", live_sources)
    for name, fn in (("mean_plane", mean_plane), ("moments", moments), ("apply", apply), ("restore", restore)):
        monkeypatch.setattr(platetone_bind, name, fn)
    return infill, calls, t


def test_plate_fill_with_tone_crops_segments_grain_and_report(host_kernels):
    infill, calls, t = host_kernels
    frames, masks, clean, boxm, logom = E.exposure_clip(seed=2, drift_q4=4, flicker_pct=8)
    T = len(frames)
    flist = [f.copy() for f in frames]
    d = t(masks)
    keep = masks.copy()
    for cuts in (None, [9, 15]):
        for tkw, gcfg in ((dict(min_pixels=256), None), (dict(min_pixels=256, mode="gain", floor=40), None), (dict(min_pixels=256), PlateGrainConfig(depth=3, reach=4))):
            del calls[:]
            got, more = [], {} if gcfg is None else dict(gcfg=gcfg)
            out, dil, rep = infill.plate_fill(flist, d, PlateFillConfig(), cuts, tcfg=PlateToneConfig(**tkw), tone_out=got, **more)
            want, wd, wc, infos = E.plate_fill(frames, masks, cuts, tone=tkw, grain=None if gcfg is None else (gcfg.depth, gcfg.reach))
            assert (np.stack(out) == want).all() and (dil.numpy() == wd).all() and (rep.filled == wc[:, 0]).all() and (rep.left == wc[:, 1]).all()
            assert rep.filled.sum() > (1000 if cuts is None else 100) and all((out[i] is flist[i]) == (wc[i, 0] == 0) for i in range(T))
            went = (masks != 0) & (wd == 0)
            assert (np.stack(out)[~went] == frames[~went]).all()                                        # only filled pixels change
            assert all((a == b).all() for a, b in zip(flist, frames)) and (d.numpy() == keep).all()     # the caller's arrays are never written
            trep, = got
            assert isinstance(trep, infill.PlateToneReport) and trep._fields == ("gain", "offset", "identity", "n", "path", "segments")
            assert trep.segments == rep.segments and trep.path == tuple(i["path"] for i in infos) == ("matched",) * len(infos)
            assert trep.n == tuple(i["n"] for i in infos) and trep.gain.shape == (T, 3) and trep.identity.dtype == bool
            assert trep.identity.tolist() == np.concatenate([i["identity"] for i in infos]).tolist()
            fits = [f for i in infos for f in i["fits"]]
            assert np.allclose(trep.gain, [[float(a) for a, b in fs] for fs in fits], rtol=0, atol=1e-12)
            assert np.allclose(trep.offset, [[float(b) for a, b in fs] for fs in fits], rtol=0, atol=1e-12)
            segs = len(rep.segments)
            steps = [["mean_plane", "moments", "apply", "stats"] + ["restore"] * bool(wc[s:e, 0].any()) for s, e in rep.segments]     # nothing filled: nothing to map back
            assert [c[0] for c in calls if c[0] != "vvl_sources"] == sum(steps, [])
            assert len([c for c in calls if c[0] == "vvl_sources"]) == (0 if gcfg is None else segs)
            # the widened crop: every device step of the stage and the fill itself work on it
            boxes = [i["box"] for i in infos]
            shapes = [(e - s, b[2] - b[0], b[3] - b[1], 3) for (s, e), b in zip(rep.segments, boxes)]
            assert [c[1] for c in calls if c[0] == "mean_plane"] == shapes == [c[1] for c in calls if c[0] == "stats"]
    # a smaller ring on a taller frame: the crop is the union box widened by the ring, not the frame
    tall, tm, _, _, _ = E.exposure_clip(seed=0, drift_q4=4, H=64, logo=None)
    del calls[:]
    got = []
    out, dil, rep = infill.plate_fill(list(tall), t(tm), PlateFillConfig(), None, tcfg=PlateToneConfig(ring=8, min_pixels=256), tone_out=got)
    want, wd, wc, (info,) = E.plate_fill(tall, tm, None, tone=dict(ring=8, min_pixels=256))
    assert info["box"] == (0, 0, 27, 56) and calls[0] == ("mean_plane", (24, 27, 56, 3), 16) and got[0].path == ("matched",)
    assert (np.stack(out) == want).all() and (dil.numpy() == wd).all() and rep.filled.sum() > 1000
    # ring 0: the union box is all mask at some time but for the two columns the box never reaches (15 rows of them): too little support,
    # unfit, the plain call
    del calls[:]
    got = []
    tlist = list(tall)
    out, dil, rep = infill.plate_fill(tlist, t(tm), PlateFillConfig(), None, tcfg=PlateToneConfig(ring=0), tone_out=got)
    assert got[0].path == ("unfit",) and got[0].n == (30,) and got[0].identity.all() and (got[0].gain == 1).all() and not got[0].offset.any()
    assert [c[0] for c in calls] == ["mean_plane", "stats"] and calls[1][1] == (24, 15, 56, 3) and not rep.filled.any() and all(a is b for a, b in zip(out, tlist))


def test_identity_unfit_skipped_empty_and_canvas_segments(host_kernels, monkeypatch):
    infill, calls, t = host_kernels
    # no drift, no grain: identity tables, the fill as without the option: its bytes, the same list entries where nothing is filled
    frames, masks, _, _, _ = E.exposure_clip(seed=0, a=0)
    flist, d, got = list(frames), t(masks), []
    out, dil, rep = infill.plate_fill(flist, d, PlateFillConfig(), None, tcfg=PlateToneConfig(), tone_out=got)
    base, bd, brep = infill.plate_fill(flist, d, PlateFillConfig(), None)
    assert got[0].path == ("identity",) and got[0].identity.all() and (got[0].gain == 1).all() and not got[0].offset.any() and got[0].n[0] > 1024
    assert (np.stack(out) == np.stack(base)).all() and (dil.numpy() == bd.numpy()).all() and rep.filled.sum() > 5000
    assert all((a == b).all() if isinstance(a, np.ndarray) else a == b for a, b in zip(rep, brep))
    assert [(o is f) for o, f in zip(out, flist)] == [(o is f) for o, f in zip(base, flist)]
    assert "apply" not in [c[0] for c in calls] and "restore" not in [c[0] for c in calls]
    # nothing filled at all: the same list entries and the same tensor object
    pf, pm, _, _ = R.panning_clip()
    plist, pd, got = list(pf), t(pm), []
    out, dil, rep = infill.plate_fill(plist, pd, PlateFillConfig(), None, tcfg=PlateToneConfig(min_pixels=64), tone_out=got)
    assert dil is pd and all(a is b for a, b in zip(out, plist)) and not rep.filled.any() and got[0].path[0] in ("matched", "identity")
    # skipped by max_bytes (the fill itself, then the widened crop alone), no mask pixel
    drift, dm, _, _, _ = E.exposure_clip(seed=0, drift_q4=4, H=64, logo=None)
    dlist, dd = list(drift), t(dm)
    for max_bytes, skipped in ((100, True), (24 * 15 * 56 * 3, False)):
        del calls[:]
        got = []
        out, dil, rep = infill.plate_fill(dlist, dd, PlateFillConfig(max_bytes=max_bytes), None, tcfg=PlateToneConfig(ring=8, min_pixels=256), tone_out=got)
        assert rep.skipped == (skipped,) and got[0].path == ("skipped",) and dil is dd and all(a is b for a, b in zip(out, dlist))
        assert "mean_plane" not in [c[0] for c in calls] and ("stats" in [c[0] for c in calls]) == (not skipped)
    z, got = t(np.zeros_like(masks)), []
    out, dil, rep = infill.plate_fill(flist, z, PlateFillConfig(), None, tcfg=PlateToneConfig(), tone_out=got)
    assert dil is z and all(a is b for a, b in zip(out, flist)) and got[0].path == ("skipped",) and got[0].n == (0,)
    infill.plate_fill(flist, d, PlateFillConfig(), None, tcfg=PlateToneConfig())                        # no list to report into: fine
    # a segment on plate_align's canvas is not matched: no step of the stage runs for it
    del calls[:]
    track = np.zeros((len(frames), 8), np.int32)
    track[:, 3] = 1
    monkeypatch.setattr(infill, "_plan_alignment", lambda f, dseg, boxes, pcfg, acfg: (None, track, (0, 0, 40, 60), "canvas"))
    monkeypatch.setattr(infill, "_fill_on_canvas", lambda f, dseg, tt, tr, box, pcfg, gcfg=None: ({}, None, np.zeros((len(f), 3), np.int64), 0))
    got = []
    out, dil, rep = infill.plate_fill(dlist, dd, PlateFillConfig(), None, acfg=object(), tcfg=PlateToneConfig(), tone_out=got)
    assert got[0].path == ("canvas",) and got[0].identity.all() and calls == [] and all(a is b for a, b in zip(out, dlist))


def test_the_call_passes_the_keywords_only_when_the_option_is_set(monkeypatch):
    import torch

    import diffuerase
    from videovanish_amd import hip, infill
    for name in ("VV_PLATE_TONE", "VV_PLATE_FILL", "VV_PLATE_GRAIN", "VV_PLATE_ALIGN", "VV_SPANS", "VV_SHADOW_MASK", "VV_MASK_CLEAN"):
        monkeypatch.delenv(name, raising=False)
    T = 3
    frames = [np.zeros((8, 8, 3), np.uint8) for _ in range(T)]
    log = []
    report = infill.PlateToneReport(np.ones((T, 3)), np.zeros((T, 3)), np.ones(T, bool), (0,), ("skipped",), ((0, T),))

    def plate_fill(f, d, cfg, cuts=None, **more):
        log.append(more)
        if "tone_out" in more:
            more["tone_out"].append(report)
        if "grain_out" in more:
            more["grain_out"].append("grain report")
        return f, d, "fill report"

    monkeypatch.setattr(diffuerase, "get_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(hip, "mask_collapse_dilate", lambda m, it: torch.zeros((T, 8, 8), dtype=torch.uint8))
    monkeypatch.setattr(infill, "plate_fill", plate_fill)
    monkeypatch.setattr(infill, "run_clip", lambda f, d, *a, **kw: list(f))
    diffuerase.last_plate_tone = "stale"
    diffuerase.run_infill_on_frames(frames, frames, plate_fill="on")
    assert log == [{}] and diffuerase.last_plate_tone is None                                           # a stand-in that knows no tcfg= still works
    diffuerase.run_infill_on_frames(frames, frames, plate_fill="on", plate_tone="ring=4")
    assert set(log[-1]) == {"tcfg", "tone_out"} and log[-1]["tcfg"] == PlateToneConfig(ring=4) and diffuerase.last_plate_tone is report
    diffuerase.run_infill_on_frames(frames, frames, plate_fill="on", plate_tone="on", plate_grain="on")
    assert set(log[-1]) == {"tcfg", "tone_out", "gcfg", "grain_out"}
    diffuerase.run_infill_on_frames(frames, frames, plate_fill="on", plate_tone="off")
    assert log[-1] == {} and diffuerase.last_plate_tone is None


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_precedence_argument_configure_environment_and_the_need_for_plate_fill(monkeypatch):
    import diffuerase
    for name in ("VV_PLATE_TONE", "VV_PLATE_FILL", "VV_PLATE_GRAIN", "VV_PLATE_ALIGN"):
        monkeypatch.delenv(name, raising=False)
    row = diffuerase._OPTION["plate_tone"]
    assert row in diffuerase.MORE_OPTIONS and row not in diffuerase.OPTIONS and len(diffuerase.OPTIONS) == 10
    assert row.env == "VV_PLATE_TONE" and row.settings is PT and row.phrase == "clean-plate exposure matching"
    assert [PT.as_config(x) for x in row.metavar.split("|")] == [PlateToneConfig()] * 2
    try:
        diffuerase.configure()
        assert diffuerase.plate_tone_config() is None
        monkeypatch.setenv("VV_PLATE_TONE", "ring=5")
        assert diffuerase.plate_tone_config() == PlateToneConfig(ring=5)
        diffuerase.configure(plate_tone="mode=gain")
        assert diffuerase.plate_tone_config() == PlateToneConfig(mode="gain") and diffuerase.plate_tone_config("on") == PlateToneConfig()
        assert diffuerase.plate_tone_config("off") is None and diffuerase.plate_tone_config(False) is None
        diffuerase.configure(plate_tone="off")
        assert diffuerase.plate_tone_config() is None                                                      # configure("off") beats the environment
        mine = PlateToneConfig(floor=3)
        assert diffuerase.plate_tone_config(mine) is mine
        diffuerase.configure()
        assert diffuerase.plate_tone_config() == PlateToneConfig(ring=5)                                   # configure() resets
        with pytest.raises(ValueError):
            diffuerase.configure(plate_tone="sometimes")
        f = [np.zeros((8, 8, 3), np.uint8)] * 2
        need = r"plate_tone= \(clean-plate exposure matching\) needs plate_fill= \(clean-plate fill\)"
        for kw in (dict(plate_tone="on"), dict(), dict(plate_tone="on", plate_fill="off")):                # the second: from the environment
            with pytest.raises(ValueError, match=need):
                diffuerase.run_infill_on_frames(f, f, **kw)
        monkeypatch.setenv("VV_PLATE_FILL", "on")
        with pytest.raises(ValueError, match=need):
            diffuerase.run_infill_on_frames(f, f, plate_fill=False)                                        # "off" wins over the environment
        with pytest.raises(ValueError, match="cannot be combined with compat_reference_early_return=True"):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)
        with pytest.raises(ValueError, match="0 <= ring <= 64"):
            diffuerase.run_infill_on_frames(f, f, plate_tone="ring=65")
        monkeypatch.delenv("VV_PLATE_FILL")
        monkeypatch.delenv("VV_PLATE_TONE")
        with pytest.raises(ValueError, match="cannot be combined with compat_reference_early_return=True"):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, plate_fill="on", plate_tone="on")
        diffuerase.last_plate_tone = "stale"
        with pytest.raises(ValueError):
            diffuerase.run_infill_on_frames(f, f, plate_tone="on")
        assert diffuerase.last_plate_tone is None                                                          # reset at the start of every call
        monkeypatch.setenv("VV_PLATE_TONE", "sometimes")
        with pytest.raises(ValueError):
            diffuerase.plate_tone_config()
    finally:
        diffuerase.configure()
    for fn in (diffuerase.run_infill_on_frames, diffuerase.configure):
        names = list(inspect.signature(fn).parameters)
        p = inspect.signature(fn).parameters["plate_tone"]
        assert names[names.index("shadow_mask") + 1] == "plate_tone" and names[-3:] == ["plate_grain", "plate_align", "plate_fill"]
        assert p.default is None and (fn is diffuerase.configure or p.kind is inspect.Parameter.KEYWORD_ONLY)
    from videovanish_amd import infill
    names = list(inspect.signature(infill.plate_fill).parameters)
    assert names[-2:] == ["tcfg", "tone_out"] and all(inspect.signature(infill.plate_fill).parameters[k].default is None for k in names[-2:])


def test_cli_plate_tone_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
    import diffuerase
    from videovanish_amd import infill
    calls = []
    videos = {"mask.mkv": [np.zeros((16, 24, 3), np.uint8)] * 3}
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda path, start=0, max_frames=-1: ([f.copy() for f in videos[path]], 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    gain = np.array([[1.0, 1.0, 1.0], [1.05, 0.9, 1.0], [1.0, 1.0, 1.02]])
    offset = np.array([[0.0, 0.0, 0.0], [2.5, -7.25, 0.0], [0.0, 1.0, 0.0]])

    def fake(frames, masks, **kw):
        calls.append(kw)
        diffuerase.last_plate_fill = None
        diffuerase.last_plate_tone = None
        if "plate_tone" in kw:
            diffuerase.last_plate_tone = infill.PlateToneReport(gain, offset, np.array([True, False, False]), (2000, 10, 0), ("matched", "unfit", "canvas"),
                                                                ((0, 1), (1, 2), (2, 3)))
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 3
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    monkeypatch.setattr(sys, "argv", argv)
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None} and capsys.readouterr().out == ""                      # a default call passes no keyword, prints nothing
    for value in ("on", "mode=gain,ring=3"):
        monkeypatch.setattr(sys, "argv", argv + ["--plate-fill", "on", "--plate-tone", value])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "plate_fill": "on", "plate_tone": value}
        out = capsys.readouterr().out
        assert out == "plate tone: 2 of 3 frames matched, largest |gain - 1| 0.1000, largest |offset| 7.25, 1 segments unfit, 1 on the canvas, of 3\n"
    for bad in ("off", "yes", "ring=x", "ring=65", "mode=linear"):
        monkeypatch.setattr(sys, "argv", argv + ["--plate-tone", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_plate_tone", None)
