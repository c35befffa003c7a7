"""Clean-plate warp on the CPU: the settings, the binding of include/platewarp.h, the product sources, the exact fit (recovery within the
rounding's bound, trimming, the pure pan, the failures, compose and invert), the restatement (tests/platewarp_ref.py) against the tracker's
restatement for integer translations, the rule on the synthetic clip with pan, zoom and roll, configuration and CLI."""
import ctypes
import inspect
import os
import re
import subprocess
import sys
import types
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abiref  # noqa: E402
import platealign_ref as A  # noqa: E402
import platewarp_ref as WR  # noqa: E402

from videovanish_amd import platewarp as PW  # noqa: E402
from videovanish_amd.platewarp import PlateWarpConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measured with the restatement on warp_clip() (seed 0, defaults), which is the reference for the device: the share of the masked pixels that
# plate_align + plate_warp fills, and the mean absolute error of the filled bytes against the sampling without the box
MEASURED_SHARE, MEASURED_MAE = 0.5485, 2.495


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_settings_parser():
    assert PW.SPELLINGS == ("on",) and (PW.BLOCKS, PW.MAX_SEARCH, PW.FRAC_BITS) == ((16, 32), 8, 20)
    for off in (None, False, "off", "none", "", " OFF "):
        assert PW.as_config(off) is None
    assert PW.as_config("on") == PW.as_config(True) == PlateWarpConfig() == PlateWarpConfig(**WR.DEFAULTS)
    assert PW.as_config("block=16,search=8,min_texture=2,min_blocks=12,trim=10,rounds=3,max_linear=50") == PlateWarpConfig()
    assert PW.as_config(" search = 2 , block=32 ") == PlateWarpConfig(block=32, search=2)
    assert PW.as_config("search=0,rounds=0,max_linear=0") == PlateWarpConfig(search=0, rounds=0, max_linear=0)
    cfg = PlateWarpConfig(trim=5)
    assert PW.as_config(cfg) is cfg
    for bad in ("yes", "search", "search=9", "block=8", "block=24", "min_blocks=2", "trim=0", "rounds=17", "max_linear=251", "min_texture=511", "radius=2",
                "search=1,search=2", "search=1.5", "trim=-1", 3, ("on",)):
        with pytest.raises(ValueError):
            PW.as_config(bad)
    with pytest.raises(ValueError, match="plate_warp must be"):
        PW.as_config("sometimes")
    for kw in (dict(block=True), dict(search=2.0), dict(trim="3")):
        with pytest.raises(ValueError, match="must be an integer"):
            PlateWarpConfig(**kw)


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_platewarp_header():
    """platewarp_bind.SIGNATURES declares every function of include/platewarp.h with the header's types and in its order, lib() has applied it,
    the version and the limits agree (abiref.check_binding); arguments are refused before anything touches a device, each refusal naming its
    function; the vvw_ prefix, the header and every name belong to no other part (what test_abi_cpu.py's walk does for the parts of its table)."""
    from videovanish_amd import align_hip, platewarp_bind as B
    loaded, define = abiref.check_binding(B, 5)
    assert B.EXPORTS == ["vvw_abi_version", "vvw_last_error", "vvw_search", "vvw_place", "vvw_unplace"] and define("VVW_ABI_VERSION") == 1
    limits = (define("VVW_FRAC_BITS"), define("VVW_MAX_SEARCH"), define("VVW_MAX_T"), define("VVW_MAX_PIXELS"), define("VVW_TRACK_INTS"), define("VVW_REC_INTS"),
              define("VVW_NSTAT"), define("VVW_MAP_INTS"))
    assert limits == (B.FRAC_BITS, B.MAX_SEARCH, B.MAX_T, B.MAX_PIXELS, B.TRACK_INTS, B.REC_INTS, B.NSTAT, B.MAP_INTS) == (20, 8, 65535, 1 << 24, 8, 4, 4, 6)
    assert limits[:4] == (PW.FRAC_BITS, PW.MAX_SEARCH, PW.MAX_T, PW.MAX_PIXELS) and B.BLOCKS == PW.BLOCKS and B.TRACK_INTS == align_hip.TRACK_INTS
    raw = open(os.path.join(ROOT, "include", "platewarp.h")).read()
    for rule in ("nby = H / block", "lexicographic minimum of (cost, dx^2 + dy^2, dy, dx)", "(dx, dy, 1, cost)", "(0, 0, 0, 0)", "Every int is written",
                 "max_residual * block^2", "min_texture * block^2", "+ 2^19) >> 20", "Maps are data", "invalid_c = 255", "dil_out_c[t][c] == 0",
                 "vva_place_masks", "launches nothing"):
        assert rule in raw, rule                                                                     # the rules are part of the ABI
    # Nothing can be launched here: every pointer is host memory and every call below is refused before the first device call.
    buf = (ctypes.c_char * 64)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 32
    search = lambda pyr=a, stride=2 * 32 * 32, track=a, T=2, H=32, W=32, block=16, s=4, tex=2, res=12, rec=a, stats=a: \
        loaded.vvw_search(pyr, stride, track, T, H, W, block, s, tex, res, rec, stats, None)
    place = lambda frames=a, dil=a, inv=a, tracked=a, B_=2, H=8, W=8, cy0=-1, cx0=-4, ch=8, cw=8, canvas=a, dil_c=a, inv_c=a: \
        loaded.vvw_place(frames, dil, inv, tracked, B_, H, W, cy0, cx0, ch, cw, canvas, dil_c, inv_c, None)
    unplace = lambda canvas=a, dil_c=a, dil_out_c=a, dil=a, fwd=a, tracked=a, T=2, H=8, W=8, cy0=-1, cx0=-4, ch=8, cw=8, py0=0, px0=0, ph=8, pw=8, patch=a, out=b: \
        loaded.vvw_unplace(canvas, dil_c, dil_out_c, dil, fwd, tracked, T, H, W, cy0, cx0, ch, cw, py0, px0, ph, pw, patch, out, None)
    for kw in (dict(pyr=None), dict(track=None), dict(rec=None), dict(stats=None), dict(T=0), dict(H=0), dict(W=-1), dict(block=0), dict(block=-16), dict(s=-1),
               dict(tex=-1), dict(res=-1)):
        assert search(**kw) == -1 and loaded.vvw_last_error().startswith(b"vvw_search:"), kw
    for kw in (dict(block=8), dict(block=24), dict(block=64), dict(s=9), dict(tex=511), dict(res=256), dict(T=65536), dict(H=1 << 13, W=(1 << 11) + 1, stride=1 << 40),
               dict(stride=2 * 32 * 32 - 1)):
        assert search(**kw) == -2 and loaded.vvw_last_error().startswith(b"vvw_search:"), kw
    assert search(s=9, T=0) == -1                                                                    # a bad argument before an unsupported one
    for kw in (dict(frames=None), dict(dil=None), dict(inv=None), dict(tracked=None), dict(canvas=None), dict(dil_c=None), dict(inv_c=None), dict(B_=0), dict(H=0),
               dict(W=0), dict(ch=0), dict(cw=-4)):
        assert place(**kw) == -1 and loaded.vvw_last_error().startswith(b"vvw_place:"), kw
    for kw in (dict(B_=65536), dict(H=1 << 13, W=(1 << 11) + 1), dict(ch=1 << 16, cw=1 << 15)):
        assert place(**kw) == -2 and loaded.vvw_last_error().startswith(b"vvw_place:"), kw
    for kw in (dict(canvas=None), dict(dil_c=None), dict(dil_out_c=None), dict(dil=None), dict(fwd=None), dict(tracked=None), dict(patch=None), dict(out=None),
               dict(out=a), dict(T=0), dict(H=0), dict(W=0), dict(ch=0), dict(cw=0), dict(ph=0), dict(pw=0), dict(py0=-1), dict(px0=-1), dict(py0=1), dict(pw=9)):
        assert unplace(**kw) == -1 and loaded.vvw_last_error().startswith(b"vvw_unplace:"), kw
    for kw in (dict(T=65536), dict(H=1 << 13, W=(1 << 11) + 1, ph=8, pw=8), dict(ch=1 << 16, cw=1 << 15)):
        assert unplace(**kw) == -2 and loaded.vvw_last_error().startswith(b"vvw_unplace:"), kw
    assert loaded.vvw_last_error() == align_hip.lib().vva_last_error()                               # one message per thread, whatever the part
    with pytest.raises(ctypes.ArgumentError):
        search(s=2.0)
    with pytest.raises(ctypes.ArgumentError):
        place(cw=8.0)
    import torch
    pyr, tr = torch.zeros((2, 2 * 32 * 32), dtype=torch.uint8), torch.zeros((2, 8), dtype=torch.int32)
    f, z = torch.zeros((2, 8, 8, 3), dtype=torch.uint8), torch.zeros((2, 8, 8), dtype=torch.uint8)
    maps, flags = torch.zeros((2, 6), dtype=torch.int64), torch.ones(2, dtype=torch.uint8)
    for call in (lambda: B.search(pyr, tr, 32, 32, PlateWarpConfig(), 12), lambda: B.place(f, z, maps, flags, (0, 0, 8, 8)),
                 lambda: B.unplace(f, z, z, z, maps, flags, (0, 0, 8, 8), (0, 0, 8, 8))):
        with pytest.raises(RuntimeError):                                                            # no CPU fallback
            call()
    assert B.blocks(40, 56, 16) == (2, 3) and B.blocks(45, 83, 16) == (2, 5) and B.blocks(96, 130, 32) == (3, 4) and B.blocks(15, 40, 16) == (0, 2)
    # the part stands outside abiref.PARTS: its prefix, header and names are checked against every part here
    assert "platewarp_bind" not in abiref.PARTS and abiref.part_of(B) is B.PART and B.PART.header == "platewarp.h"
    assert re.fullmatch(r"vv[a-z]_", B.PART.prefix)
    from videovanish_amd import detailmatch_bind, flicklocal_bind, grainshape_bind, overlaymask_bind, platetone_bind
    names = set(B.SIGNATURES)
    outside = [(m, m.PART) for m in (platetone_bind, detailmatch_bind, grainshape_bind, flicklocal_bind, overlaymask_bind)]
    for module, part in abiref.parts() + outside:
        assert part.prefix != B.PART.prefix and part.header != B.PART.header, module.__name__
        assert not names & set(module.SIGNATURES), module.__name__
        assert not [n for n in module.SIGNATURES if n.startswith(B.PART.prefix)], module.__name__
    assert all(n.startswith("vvw_") for n in names)
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != "platewarp.h":
            assert "vvw_" not in open(os.path.join(ROOT, "include", header)).read().lower(), header  # no header used the prefix before


def test_product_sources_of_the_feature():
    """The kernels live in a unit of their own, in the one recipe with the header among the dependencies; no environment; the reductions come
    from the shared header (the 64-bit minimum is the one vv_flicklocal.hip uses, moved there); the search uses the packed-byte SAD on
    byte-aligned LDS dwords and a 64-bit key; the settings import no torch; vvalign.h and vvplate.h keep their versions; importing the drop-in
    and asking for the setting resolves no vvw_ symbol."""
    kernel, txt = abiref.check_sources("vv_platewarp", "platewarp.h", "platewarp")
    for fn in ("vvw_search", "vvw_place", "vvw_unplace"):
        assert f'extern "C" int {fn}(' in kernel
    for used in ('#include "vv_wave_bytes.h"', "using vvwave::wave_sum;", "using vvwave::wave_min64;", "__builtin_amdgcn_sad_u8(", "__builtin_amdgcn_alignbyte(",
                 "__shared__ unsigned areaY[", "__shared__ unsigned areaV[", "__shared__ unsigned ref[", "wave_min64(best)"):
        assert used in kernel, used
    shared = open(os.path.join(abiref.CSRC, "vv_wave_bytes.h")).read()
    local = open(os.path.join(abiref.CSRC, "vv_flicklocal.hip")).read()
    assert "u64 wave_min64(u64 v)" in shared and "u64 wave_min64(u64 v)" not in local and "using vvwave::wave_min64;" in local
    assert "vv_platewarp" not in open(os.path.join(abiref.CSRC, "vv_align.hip")).read() + open(os.path.join(abiref.CSRC, "vv_plate.hip")).read()
    for header, version in (("vvalign.h", "VVA_ABI_VERSION 1"), ("vvplate.h", "VVP_ABI_VERSION 1")):
        assert "#define " + version in open(os.path.join(ROOT, "include", header)).read()
    assert "import ctypes" not in txt and "float(" not in txt and "import numpy" not in txt
    code = ("import sys, diffuerase; from videovanish_amd import platewarp_bind, align_hip, plate_hip, hip; "
            "assert platewarp_bind.PART.dll is None and align_hip.PART.dll is None and plate_hip.PART.dll is None and hip.CORE.dll is None; "
            "assert diffuerase.plate_warp_config() is None and diffuerase.last_plate_warp is None")
    env = {k: v for k, v in os.environ.items() if k not in ("VV_PLATE_FILL", "VV_PLATE_ALIGN", "VV_PLATE_WARP")}
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)
    code = "import sys, videovanish_amd.platewarp as d; assert 'torch' not in sys.modules and 'numpy' not in sys.modules and d.as_config('on').search == 8"
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)


# ---- the fit --------------------------------------------------------------------------------------------------------------------------------
def _grid(nby=6, nbx=8):
    return [(bx, by) for by in range(nby) for bx in range(nbx)]


def _centre(bx, by, B=16):
    return bx * B + (B - 1) / 2.0, by * B + (B - 1) / 2.0


def _field_at(field, x, y):
    return tuple(float(f[0] + f[1] * Fraction(x) + f[2] * Fraction(y)) for f in field)


def _bound(blocks, x, y, B=16):
    """Least squares is linear in the targets: the fitted value at (x, y) is sum_i w_i(x, y) u_i with w = (1, x, y) (D^T D)^-1 D^T over the
    design matrix D of the blocks' centres.  Targets rounded to integers are off by at most 1/2 each, so the fitted value is off from the
    field's by at most sum_i |w_i(x, y)| / 2 per component."""
    D = np.array([(1.0,) + _centre(bx, by, B) for bx, by in blocks])
    w = np.array([1.0, x, y]) @ np.linalg.inv(D.T @ D) @ D.T
    return float(np.abs(w).sum()) / 2 + 1e-9


def test_fit_recovers_a_rounded_affine_field_within_the_roundings_bound():
    """Vectors made by rounding a known affine field to integers: without trimming the fit is the least squares of all of them, so at the blocks'
    centres and at the frame's corners it lies within _bound of the field; exact arithmetic adds nothing to it."""
    true = ((3.3, 0.021, -0.013), (-1.6, 0.017, 0.030))
    blocks = _grid()
    vec = [(bx, by) + tuple(int(np.floor(t[0] + t[1] * x + t[2] * y + 0.5)) for t in true) for bx, by in blocks for x, y in [_centre(bx, by)]]
    fit = PW.fit_frame(vec, (0, 0), PlateWarpConfig(rounds=0))
    assert fit.ok and fit.kept == tuple(range(48)) and all(isinstance(v, Fraction) for f in fit.field for v in f)
    worst = 0.0
    for x, y in [_centre(bx, by) for bx, by in blocks] + [(0, 0), (127, 0), (0, 95), (127, 95)]:
        got, lim = _field_at(fit.field, x, y), _bound(blocks, x, y)
        for g, t in zip(got, true):
            worst = max(worst, abs(g - (t[0] + t[1] * x + t[2] * y)) / lim)
    assert worst <= 1.0, worst
    assert _bound(blocks, 63.5, 47.5) < 0.51 and 1.0 < _bound(blocks, 0, 0) < 1.1                   # the bound itself: half a pixel at the centre, 1.08 px at a corner of 6 x 8 blocks
    # d0 only moves the targets: the same vectors round d0 give the same field
    moved = PW.fit_frame([(bx, by, dx - 4, dy + 2) for bx, by, dx, dy in vec], (4, -2), PlateWarpConfig(rounds=0))
    assert moved.field == fit.field
    # with the default trimming nothing is dropped either (a rounding is at most 0.71 px from the field, the fit at most _bound more ... under 1 px here)
    assert PW.fit_frame(vec, (0, 0), PlateWarpConfig()).field == fit.field


def test_fit_trims_a_fifth_of_outliers_and_pure_pan_is_exactly_linear_free():
    rng = np.random.default_rng(5)
    true = ((-2.4, -0.018, 0.011), (0.7, -0.009, -0.025))
    blocks = _grid()
    vec = [[bx, by] + [int(np.floor(t[0] + t[1] * x + t[2] * y + 0.5)) for t in true] for bx, by in blocks for x, y in [_centre(bx, by)]]
    bad = sorted(int(i) for i in rng.choice(48, 10, replace=False))                                  # a fifth of the blocks
    for i in bad:
        ang = rng.uniform(0, 2 * np.pi)
        vec[i][2] += int(round(7 * np.cos(ang))) or 6
        vec[i][3] += int(round(7 * np.sin(ang))) or -6
    fit = PW.fit_frame([tuple(v) for v in vec], (0, 0), PlateWarpConfig())
    assert fit.ok and not set(fit.kept) & set(bad) and len(fit.kept) >= 30
    kept = [blocks[i] for i in fit.kept]
    for x, y in [(0, 0), (127, 0), (0, 95), (127, 95), (63.5, 47.5)]:
        for g, t in zip(_field_at(fit.field, x, y), true):
            assert abs(g - (t[0] + t[1] * x + t[2] * y)) <= _bound(kept, x, y)                       # the bound of the kept set
    assert not PW.fit_frame([tuple(v) for v in vec], (0, 0), PlateWarpConfig(rounds=0)).field == fit.field
    # equal vectors: exact least squares gives a linear part of exactly zero and the vector itself
    pan = PW.fit_frame([(bx, by, 1, -2) for bx, by in blocks], (7, 3), PlateWarpConfig())
    assert pan.ok and pan.field == ((8, 0, 0), (1, 0, 0)) and pan.mse == 0
    track = np.zeros((3, 8), np.int32)
    track[:, 3] = 1
    track[1, :2], track[2, :2] = (7, 3), (13, 5)
    rec = np.zeros((3, 6, 8, 4), np.int32)
    rec[..., 2] = 1
    plan = PW.plan_segment(track, rec, PlateWarpConfig(), 96, 128)
    assert plan.translation and plan.fwd[2] == PW.translation_table(13, 5) and plan.inv[2] == PW.translation_table(-13, -5)
    rec[1, ..., 0] = 1                                                                               # one more pixel everywhere: an integer translation, not the tracker's
    assert not PW.plan_segment(track, rec, PlateWarpConfig(), 96, 128).translation


def test_fit_failures_keep_the_translation():
    cfg = PlateWarpConfig()
    d0 = (5, -3)
    keep = ((5, 0, 0), (-3, 0, 0))
    few = PW.fit_frame([(bx, 0, 0, 0) for bx in range(11)] , d0, cfg)
    line = PW.fit_frame([(bx, 2, 0, 0) for bx in range(16)], d0, cfg)                                # collinear: the normal matrix is singular
    steep = PW.fit_frame([(bx, by, bx, 0) for bx, by in _grid()], d0, cfg)                           # 1 px per 16 px = 62.5 thousandths
    for fit in (few, line, steep, PW.fit_frame([], d0, cfg)):
        assert not fit.ok and fit.field == keep and fit.kept == () and fit.mse == 0
    assert PW.fit_frame([(bx, by, bx, 0) for bx, by in _grid()], d0, PlateWarpConfig(max_linear=63)).ok
    # in a plan a failed frame is the tracker's translation, exactly
    track = np.zeros((2, 8), np.int32)
    track[:, 3] = 1
    track[1, :2] = d0
    rec = np.zeros((2, 6, 8, 4), np.int32)
    plan = PW.plan_segment(track, rec, cfg, 96, 128)
    assert plan.fits[0] is None and not plan.fits[1].ok and plan.translation and plan.fwd[1] == PW.translation_table(5, -3)
    track[1, 3] = 0                                                                                  # an untracked frame has no map
    plan = PW.plan_segment(track, rec, cfg, 96, 128)
    assert plan.maps[1] is None and plan.tracked == [True, False] and plan.fwd[1] == PW.translation_table(0, 0)


def test_border_winners_are_not_fitted():
    cfg = PlateWarpConfig()
    assert PW.on_border(0, 0, 0, 0, 0, 0, 96, 128, cfg) and PW.on_border(7, 5, 0, 0, 0, 0, 96, 128, cfg) and not PW.on_border(1, 1, 0, 0, 0, 0, 96, 128, cfg)
    assert PW.on_border(1, 1, -16, 0, 0, 0, 96, 128, cfg) and not PW.on_border(1, 1, -15, 0, 0, 0, 96, 128, cfg)
    assert PW.on_border(3, 3, 8, 0, 8, 0, 96, 128, cfg) and PW.on_border(3, 3, 0, -8, 0, -8, 96, 128, cfg) and not PW.on_border(3, 3, 7, 7, 7, 7, 96, 128, cfg)
    assert not PW.on_border(3, 3, 0, 0, 0, 0, 96, 128, PlateWarpConfig(search=0))
    assert PW.on_border(3, 3, 0, 0, 0, 0, 96, 128, cfg, (40, 64, 50, 70)) and not PW.on_border(3, 3, 0, 0, 0, 0, 96, 128, cfg, (40, 65, 50, 70))
    assert not PW.on_border(3, 3, 0, 0, 0, 0, 96, 128, cfg, (0, 0, 0, 0))


def test_compose_invert_and_tables_round_trip():
    a = ((Fraction(7, 3), Fraction(1043, 1000), Fraction(-3, 100)), (Fraction(-11, 7), Fraction(29, 1000), Fraction(104, 100)))
    b = ((Fraction(-5), Fraction(99, 100), Fraction(1, 50)), (Fraction(2), Fraction(-1, 40), Fraction(101, 100)))
    ident = ((0, 1, 0), (0, 0, 1))
    assert PW.compose(a, PW.invert(a)) == ident == PW.compose(PW.invert(a), a) and PW.compose(a, ident) == a
    m = PW.compose(a, b)
    for x, y in ((0, 0), (5, 9), (-3, 120)):
        inner = tuple(r[0] + r[1] * x + r[2] * y for r in b)
        assert tuple(r[0] + r[1] * inner[0] + r[2] * inner[1] for r in a) == tuple(r[0] + r[1] * x + r[2] * y for r in m)
    with pytest.raises(ValueError):
        PW.invert(((0, 1, 2), (0, 2, 4)))
    fwd, inv = PW.to_fixed(m), PW.to_fixed(PW.invert(m))
    assert all(isinstance(v, int) for v in fwd + inv)
    assert PW.to_fixed(((Fraction(1, 2 ** 21), 1, 0), (Fraction(-1, 2 ** 21), 0, 1))) == (1, 1 << 20, 0, 0, 0, 1 << 20)        # half up, once
    worst = 0
    for y in range(-8, 120, 7):
        for x in range(-8, 160, 7):
            cx, cy = PW.apply_fixed(fwd, x, y)
            bx, by = PW.apply_fixed(inv, cx, cy)
            worst = max(worst, abs(bx - x), abs(by - y))
            gx, gy = WR.map_points(fwd, x, y)
            assert (int(gx), int(gy)) == (cx, cy)                                                    # the restatement's int64 form is rule M
    assert worst <= 1
    assert PW.apply_fixed(PW.translation_table(-3, 4), 10, 20) == (7, 24)
    # maps are data: products that leave 64 bits wrap, as the rule says
    gx, gy = WR.map_points((1 << 62, 1 << 62, 0, 0, 0, 1 << 20), 4, 5)
    assert int(gx) == ((((1 << 62) * 5 + (1 << 19)) % (1 << 64)) >> 20) and int(gy) == 5
    boxes = np.array([[10, 20, 30, 44], [0, 0, 0, 0], [12, 22, 28, 40]])
    tabs = [PW.translation_table(0, 0), PW.translation_table(100, 100), PW.translation_table(-30, 5)]
    assert PW.canvas_box(boxes, tabs, [True, True, True]) == (9, -12, 34, 48)
    assert PW.canvas_box(boxes, tabs, [True, True, False]) == (9, 16, 31, 48) and PW.canvas_box(boxes, tabs, [False, True, False]) is None
    assert PW.canvas_bytes(3, (9, -12, 34, 48)) == 3 * 25 * 60 * 3


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_restatement_with_integer_translations_is_the_trackers_canvas():
    """With integer-translation tables place and unplace give the bytes of platealign_ref's place, place_masks and unplace_mask."""
    frames, masks, off, _, _, _ = A.stage_clip(40, 56)
    T = len(frames)
    track = np.zeros((T, 8), np.int32)
    track[:, 3] = 1
    track[:, 0], track[:, 1] = off[:, 0], off[:, 1] + np.arange(T) % 3 - 1
    track[5, 3] = 0                                                                                  # a lost frame
    box = A.canvas_box(masks, track)
    fwd = [PW.translation_table(r[0], r[1]) for r in track]
    inv = [PW.translation_table(-r[0], -r[1]) for r in track]
    ok = track[:, 3] == 1
    canvas, dil_c, inv_c = WR.place(frames, masks, inv, ok, box)
    want, _ = A.place(frames, track, box)
    wd, wi = A.place_masks(masks, track, box)
    assert np.array_equal(canvas, want) and np.array_equal(dil_c, wd) and np.array_equal(inv_c, wi) and box[1] < 0 or box[3] > 56
    d2 = dil_c.copy()
    d2[:, ::2] = 0                                                                                   # "filled" rows
    patch, dout = WR.unplace(canvas, dil_c, d2, masks, fwd, ok, box, (0, 0, 40, 56))
    assert np.array_equal(dout, A.unplace_mask(d2, masks, track, box))
    went = (masks != 0) & (dout == 0)
    assert went.any() and not went[5].any() and np.array_equal(patch[went], frames[went]) and not patch[~went].any()


def test_search_restatement_finds_planted_vectors_and_keeps_the_order():
    rng = np.random.default_rng(11)
    wide = A.smooth(rng.integers(0, 256, (80, 110)) * 8, 1) // 8
    Y = np.stack([wide[8:56, 8:88], wide[8 + 2:56 + 2, 8 - 3:88 - 3], np.full((48, 80), 90), np.full((48, 80), 90)])
    V = np.ones(Y.shape, bool)
    track = np.zeros((4, 8), np.int32)
    track[:, 3] = 1
    track[3, 2] = 2                                                                                               # a flat frame against a flat key
    rec, stats = WR.search(Y, V, track, 16, 4, 1, 12)
    assert not rec[0].any() and (rec[1, 1, 1:4, :3] == [-3, 2, 1]).all() and (rec[1, 1, 1:4, 3] == 0).all()      # frame 0 is its own key; interior blocks find the plant
    assert not rec[2:].any() and stats[2:].tolist() == [[0, 0, 0, 0]] * 2                                         # flat: no texture
    flat, st = WR.search(Y, V, track, 16, 4, 0, 255)
    assert (flat[3] == [0, 0, 1, 0]).all() and st[3].tolist() == [15, 15, 0, 0]                                   # every candidate ties: the order gives (0, 0)
    V[0, 20:30, 30:44] = False
    masked, _ = WR.search(Y, V, track, 16, 4, 1, 12)
    assert (masked[1] != rec[1]).any()                                                                            # the key's mask takes candidates away
    assert WR.search(Y[:, :15], V[:, :15], track, 16, 4, 1, 12)[0].shape == (4, 0, 5, 4)


# ---- the rule on the synthetic clip ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip():
    frames, masks, truth, maps = WR.warp_clip()
    return frames, masks, truth, maps, A.fill_segment(frames, masks), WR.fill_segment(frames, masks)


def test_fitted_maps_predict_the_true_corner_displacements(clip):
    frames, masks, truth, maps, _, (_, _, _, info) = clip
    T, H, W = masks.shape
    assert (T, H, W) == (12, 96, 128) and info["path"] == "canvas" and info["warp"] == "warp" and (info["track"][:, 3] == 1).all()
    plan = info["plan"]
    assert all(f.ok for f in plan.fits[1:]) and plan.fits[0] is None and not plan.translation
    worst = 0.0
    for t in range(T):
        for x in (0, W - 1):
            for y in (0, H - 1):
                got = tuple(float(r[0] + r[1] * x + r[2] * y) for r in plan.maps[t])
                want = tuple(r[0] + r[1] * x + r[2] * y for r in maps[t])
                worst = max(worst, abs(got[0] - want[0]), abs(got[1] - want[1]))
    print(f"largest corner error {worst:.3f} px")
    assert worst < 1.0, worst
    # what a translation leaves at a corner of the last frame is several pixels: the case the stage is for
    t = T - 1
    left = max(abs(maps[t][0][0] + maps[t][0][1] * x + maps[t][0][2] * y - x - info["track"][t][0]) for x in (0, W - 1) for y in (0, H - 1))
    assert left > 3.0


def test_plate_warp_fills_more_than_plate_align_alone_and_close_to_the_truth(clip):
    frames, masks, truth, maps, (o1, d1, c1, i1), (o2, d2, c2, i2) = clip
    masked = masks != 0
    went1, went2 = masked & (d1 == 0), masked & (d2 == 0)
    assert i1["path"] == "canvas" and int(went2.sum()) > int(went1.sum()) and c2[:, 0].sum() == went2.sum() and c2[:, 1].sum() == (d2 != 0).sum()
    share = went2.sum() / masked.sum()
    mae = np.abs(o2[went2].astype(np.int64) - truth[went2].astype(np.int64)).mean()
    print(f"share of the masked pixels filled: warp {share:.4f}, align alone {went1.sum() / masked.sum():.4f}; mean absolute error of the filled bytes {mae:.3f}")
    assert share >= MEASURED_SHARE - 0.1 and mae <= MEASURED_MAE + 0.25
    # the guarantees of the fill: nothing outside the mask changes, an unfilled masked pixel keeps its bytes and its mask, dil' only clears
    assert np.array_equal(o2[~went2], frames[~went2]) and np.array_equal(d2[~went2], masks[~went2]) and not d2[went2].any()
    # every filled byte is a byte of the clip: of some frame at some place
    vals = {tuple(v) for v in frames.reshape(-1, 3)}
    assert all(tuple(v) in vals for v in o2[went2][::37])


# ---- configuration and CLI ------------------------------------------------------------------------------------------------------------------
def test_precedence_and_plate_warp_needs_plate_fill_and_plate_align(monkeypatch):
    import diffuerase
    from videovanish_amd import infill
    for name in ("VV_PLATE_FILL", "VV_PLATE_ALIGN", "VV_PLATE_WARP"):
        monkeypatch.delenv(name, raising=False)
    diffuerase.configure()
    try:
        assert diffuerase.plate_warp_config() is None
        monkeypatch.setenv("VV_PLATE_WARP", "search=6")
        assert diffuerase.plate_warp_config() == PlateWarpConfig(search=6)
        diffuerase.configure(plate_warp="block=32")
        assert diffuerase.plate_warp_config() == PlateWarpConfig(block=32) and diffuerase.plate_warp_config("on") == PlateWarpConfig()
        assert diffuerase.plate_warp_config("off") is None
        diffuerase.configure(plate_warp="off")
        assert diffuerase.plate_warp_config() is None                                                # configure("off") beats the environment
        diffuerase.configure()
        assert diffuerase.plate_warp_config() == PlateWarpConfig(search=6)
        with pytest.raises(ValueError):
            diffuerase.configure(plate_warp="sometimes")
        f = [np.zeros((8, 8, 3), np.uint8)] * 2
        needs = r"plate_warp= \(clean-plate warp\) needs plate_fill= \(clean-plate fill\) and plate_align= \(clean-plate alignment\)"
        for kw in (dict(), dict(plate_warp="on"), dict(plate_fill="on"), dict(plate_align="on", plate_fill="off"), dict(plate_fill="on", plate_align="off")):
            with pytest.raises(ValueError, match=needs if "plate_align" not in kw or kw["plate_align"] == "off" or "plate_fill" not in kw else "plate_align="):
                diffuerase.run_infill_on_frames(f, f, **kw)
        monkeypatch.delenv("VV_PLATE_WARP")
        diffuerase.last_plate_warp = "stale"
        with pytest.raises(ValueError, match=needs):
            diffuerase.run_infill_on_frames(f, f, plate_fill="on", plate_warp=PlateWarpConfig())
        assert diffuerase.last_plate_warp is None                                                    # reset at the start of every call
        with pytest.raises(ValueError, match="compat_reference_early_return=True"):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, plate_fill="on", plate_align="on", plate_warp="on")
        with pytest.raises(ValueError, match="wcfg"):
            infill.plate_fill(f, None, None, wcfg=PlateWarpConfig())
    finally:
        diffuerase.configure()
    for fn in (diffuerase.run_infill_on_frames, diffuerase.configure):
        names = list(inspect.signature(fn).parameters)
        p = inspect.signature(fn).parameters["plate_warp"]
        assert names[names.index("plate_tone") + 1] == "plate_warp" and names[-3:] == ["plate_grain", "plate_align", "plate_fill"]
        assert p.default is None and (fn is diffuerase.configure or p.kind is inspect.Parameter.KEYWORD_ONLY)
    names = list(inspect.signature(infill.plate_fill).parameters)
    assert names[names.index("acfg") + 1:names.index("acfg") + 4] == ["align_out", "wcfg", "warp_out"]                # next to acfg=, align_out=
    assert all(inspect.signature(infill.plate_fill).parameters[k].default is None for k in ("wcfg", "warp_out"))
    assert [o.name for o in diffuerase.ALL_OPTIONS][-1] == "plate_warp" and diffuerase.ALL_OPTIONS[-1].env == "VV_PLATE_WARP"
    assert diffuerase.ALL_OPTIONS[-1].metavar == "on|block=16,search=8,min_texture=2,min_blocks=12,trim=10,rounds=3,max_linear=50"


def test_cli_plate_warp_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
    import diffuerase
    from videovanish_amd import infill
    calls = []
    videos = {"mask.mkv": [np.zeros((16, 24, 3), np.uint8)] * 3}
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda path, start=0, max_frames=-1: ([f.copy() for f in videos[path]], 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    maps = np.array([[0, 1, 0, 0, 0, 1], [2.5, 1.01, -0.02, 0.25, 0.0125, 1.0], [np.nan] * 6])
    rep = infill.PlateWarpReport((maps,), (np.array([0, 40, 0]),), (np.array([0, 33, 0]),), (np.array([0, 25, 0]),), (np.array([0.0, 0.375, 0.0]),),
                                 (np.array([False, False, False]),), ((0, 0, 8, 8),), ("warp",), ((0, 3),))

    def fake(frames, masks, **kw):
        calls.append(kw)
        diffuerase.last_plate_warp = rep if "plate_warp" in kw else None
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 3
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    monkeypatch.setattr(sys, "argv", argv)
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None} and capsys.readouterr().out == ""                # a default call passes no keyword, prints nothing
    for value in ("on", "block=32,search=4"):
        monkeypatch.setattr(sys, "argv", argv + ["--plate-fill", "on", "--plate-align", "on", "--plate-warp", value])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "plate_fill": "on", "plate_align": "on", "plate_warp": value}
        assert capsys.readouterr().out == ("plate warp: 1 of 3 frames fitted, 0 fits failed, largest linear coefficient 0.0200, largest rms 0.38 px, "
                                           "1 of 1 segments filled on a warped canvas\n")
    for bad in ("off", "yes", "search=x", "search=9", "block=8"):
        monkeypatch.setattr(sys, "argv", argv + ["--plate-warp", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_plate_warp", None)
