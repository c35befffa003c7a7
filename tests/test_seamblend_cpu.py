"""Seam membrane blending on the CPU: the settings, the binding of include/vvblend.h, the level plan, the report, the accuracy of the
restatement of tests/seamblend_ref.py against a direct sparse solve, restoration and exactness on the restatement, infill.finish with the
kernels replaced by the restatement, configuration and CLI."""
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
import grainmatch_ref as GR  # noqa: E402
import seamblend_ref as R  # noqa: E402
import tonematch_ref as TR  # noqa: E402

from videovanish_amd import seamblend as M  # noqa: E402
from videovanish_amd.seamblend import SeamBlendConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_spellings_and_config():
    for off in (None, False, "off", "none", "", " OFF "):
        assert M.as_config(off) is None and M.as_config(off, 3) is None
    d = SeamBlendConfig()
    assert (d.ring, d.presmooth, d.sweeps, d.max_shift, d.strength, d.strength_q8) == (12, 2, 8, 32, 1.0, 256)
    assert M.as_config("on") == M.as_config(" On ") == M.as_config(True) == d
    assert M.as_config("ring=12,presmooth=2,sweeps=8,max_shift=32,strength=1.0") == d
    assert M.as_config(" ring = 32 , presmooth=4,sweeps=16,max_shift=255,strength=2 ") == SeamBlendConfig(32, 4, 16, 255, 2.0)
    assert M.as_config("ring=1,presmooth=0,sweeps=1,max_shift=1,strength=0") == SeamBlendConfig(1, 0, 1, 1, 0.0)
    assert M.as_config("strength=0.5").strength_q8 == 128 and M.as_config("strength=2").strength_q8 == 512
    cfg = SeamBlendConfig(ring=4)
    assert M.as_config(cfg) is cfg
    with pytest.raises(Exception):
        cfg.ring = 5                                                                                 # frozen
    for bad in ("yes", "static", "luma", "ring", "ring=", "ring=x", "ring=-3", "ring=1.5", "ring=3,ring=4", "size=3", "ring=3;sweeps=1", "ring=0",
                "ring=33", "presmooth=5", "presmooth=-1", "sweeps=0", "sweeps=17", "max_shift=0", "max_shift=256", "max_shift=1.5", "strength=-0.1",
                "strength=2.5", "strength=nan", "strength=inf", "on,ring=3", "ring=3,", "mode=luma", 3, 1.0, ("on",)):
        with pytest.raises(ValueError):
            M.as_config(bad)
    with pytest.raises(ValueError, match="'on', 'off', 'ring=N,presmooth=N,sweeps=N,max_shift=N,strength=X'"):
        M.as_config("sometimes")
    for kw in (dict(ring=0), dict(ring=33), dict(ring=4.0), dict(ring=True), dict(presmooth=-1), dict(presmooth=5), dict(presmooth="2"), dict(sweeps=0),
               dict(sweeps=17), dict(sweeps=8.0), dict(max_shift=0), dict(max_shift=256), dict(max_shift=32.0), dict(strength=-0.01), dict(strength=2.01),
               dict(strength="1"), dict(strength=None), dict(strength=float("nan"))):
        with pytest.raises(ValueError):
            SeamBlendConfig(**kw)
    assert "build-defined" in SeamBlendConfig.__doc__
    # every pixel the feather takes from the model has to be a cell of the field: the ring is wider than ceil(feather_px)
    assert M.as_config("on", 3) == d and M.as_config("ring=4", 3.0).ring == 4 and M.as_config("ring=4", 2.5).ring == 4 and M.as_config("ring=1", 0).ring == 1
    for ring, feather in ((3, 3), (3, 2.5), (1, 1), (12, 12), (2, 64)):
        with pytest.raises(ValueError, match="feather_px"):
            M.as_config(f"ring={ring}", feather)
    assert M.as_config("ring=1").ring == 1                                                           # no feather given: not checked


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_vvblend_header():
    """blend_hip.SIGNATURES declares every function of include/vvblend.h with the header's types and in its order, blend_hip.lib() has applied it,
    the version and the limits agree (abiref.check_binding; test_abi_cpu.py: no name could be taken for another part's), the formulas of the
    field stand in the header, and the arguments are validated before any device work, each refusal naming its function."""
    from videovanish_amd import blend_hip
    loaded, define = abiref.check_binding(blend_hip, 9)
    raw = open(os.path.join(ROOT, "include", "vvblend.h")).read()
    assert define("VVB_ABI_VERSION") == 1
    assert define("VVB_MAX_RING") == M.MAX_RING == 32 and define("VVB_MAX_PRESMOOTH") == M.MAX_PRESMOOTH == 4
    assert define("VVB_MAX_SWEEPS") == M.MAX_SWEEPS == 16 and define("VVB_MAX_SHIFT") == M.MAX_SHIFT == 255
    assert define("VVB_NSUM") == blend_hip.NSUM == M.NSUM == 11 and define("VVB_MAX_STRENGTH_Q8") == SeamBlendConfig(strength=2).strength_q8
    assert (define("VVB_INACTIVE"), define("VVB_KNOWN"), define("VVB_UNKNOWN")) == (R.INACTIVE, R.KNOWN, R.UNKNOWN)
    for formula in ("(2 * 64 * S_c + N) // (2 N)", "(2 S_c + N) // (2 N)", "(N_c + S_c + W_c + E_c + 2) >> 2", "(m_c * strength_q8 + (1 << 13)) >> 14",
                    "((7 T h_l w_l + 15) & ~15)", "max(h_l, w_l) > 2"):
        assert formula in raw, formula                                                               # the field is part of the ABI
    # the other headers are as they were
    for header, prefix, count in (("vvtone.h", "vvt", 4), ("vvgrain.h", "vvg", 4)):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        assert len(set(re.findall(rf"\b({prefix}_[a-z0-9_]+)\s*\(", txt))) == count and f"#define {prefix.upper()}_ABI_VERSION 1" in txt
    # the host-side functions, against the restated plan
    for T, h, w in ((1, 1, 1), (1, 2, 2), (3, 37, 53), (9, 96, 130), (32, 720, 1280), (2, 1080, 1920), (5, 1, 700), (1, 3, 2)):
        assert loaded.vvb_levels(h, w) == len(M.level_sizes(h, w)) and loaded.vvb_scratch_bytes(T, h, w) == M.scratch_bytes(T, h, w), (T, h, w)
    assert loaded.vvb_levels(0, 4) == -1 and loaded.vvb_scratch_bytes(0, 4, 4) == -1 and loaded.vvb_scratch_bytes(1, 4, -1) == -1
    # arguments are validated before anything touches a device: -1 null pointers and sizes, -2 the ranges
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    b = a + 32
    diff = lambda patch=a, orig=a, mask=a, offs=a, lut=a, cls=a, val=a, sums=a, Hm=4, Wm=4, T=1, H0=8, W0=8, h=4, w=4, ring=4, ps=2, ms=32: \
        loaded.vvb_ring_diff(patch, Hm, Wm, orig, mask, offs, lut, T, H0, W0, h, w, ring, ps, ms, cls, val, sums, None)
    solve = lambda patch=a, orig=a, mask=a, offs=a, lut=a, scratch=a, nbytes=1 << 20, sums=a, Hm=4, Wm=4, T=1, H0=8, W0=8, h=4, w=4, ring=4, ps=2, \
        sweeps=8, ms=32: loaded.vvb_solve(patch, Hm, Wm, orig, mask, offs, lut, T, H0, W0, h, w, ring, ps, sweeps, ms, scratch, nbytes, sums, None)
    pull = lambda cls=a, val=a, up=a, vup=a, T=1, hl=4, wl=4: loaded.vvb_pull(cls, val, T, hl, wl, up, vup, None)
    relax = lambda cls=a, val=a, parent=None, out=b, T=1, hl=4, wl=4, sweeps=8, start=0, sums=None: \
        loaded.vvb_relax(cls, val, parent, out, T, hl, wl, sweeps, start, sums, None)
    paste = lambda patch=a, orig=a, mask=a, offs=a, lut=a, field=a, q8=256, amp=a, ids=a, out=a, seed=0, mode=0, Hm=4, Wm=4, T=1, H0=8, W0=8, h=4, w=4, \
        feather=3.0: loaded.vvb_paste_blend_composite(patch, Hm, Wm, orig, mask, offs, lut, field, q8, amp, ids, seed, mode, T, H0, W0, h, w, feather, out, None)
    sizes = (dict(Hm=0), dict(Wm=-1), dict(T=0), dict(H0=0), dict(W0=0), dict(h=0), dict(w=0), dict(h=9), dict(w=9))
    for kw in (dict(patch=None), dict(orig=None), dict(mask=None), dict(offs=None), dict(lut=None), dict(cls=None), dict(val=None), dict(sums=None)) + sizes:
        assert diff(**kw) == -1 and b"vvb_ring_diff" in loaded.vvb_last_error(), kw
    for kw in (dict(ring=0), dict(ring=33), dict(ps=-1), dict(ps=5), dict(ms=0), dict(ms=256)):
        assert diff(**kw) == -2 and b"vvb_ring_diff" in loaded.vvb_last_error(), kw
        assert solve(**kw) == -2 and b"vvb_solve" in loaded.vvb_last_error(), kw
    assert diff(ring=0, T=0) == -1                                                                   # a bad argument before an unsupported one
    for kw in (dict(patch=None), dict(orig=None), dict(mask=None), dict(offs=None), dict(lut=None), dict(scratch=None), dict(sums=None),
               dict(nbytes=M.scratch_bytes(1, 4, 4) - 1), dict(nbytes=0)) + sizes:
        assert solve(**kw) == -1 and b"vvb_solve" in loaded.vvb_last_error(), kw
    for kw in (dict(sweeps=0), dict(sweeps=17), dict(sweeps=-1)):
        assert solve(**kw) == -2 and b"vvb_solve" in loaded.vvb_last_error(), kw
        assert relax(**kw) == -2 and b"vvb_relax" in loaded.vvb_last_error(), kw
    for kw in (dict(cls=None), dict(val=None), dict(up=None), dict(vup=None), dict(T=0), dict(hl=0), dict(wl=-1)):
        assert pull(**kw) == -1 and b"vvb_pull" in loaded.vvb_last_error(), kw
    for kw in (dict(cls=None), dict(val=None), dict(out=None), dict(T=0), dict(hl=0), dict(wl=0), dict(start=2), dict(start=-1), dict(out=a, start=0)):
        assert relax(**kw) == -1 and b"vvb_relax" in loaded.vvb_last_error(), kw
    for kw in (dict(patch=None), dict(orig=None), dict(offs=None), dict(lut=None), dict(field=None), dict(amp=None), dict(ids=None), dict(out=None),
               dict(Hm=0), dict(T=-2), dict(H0=0), dict(h=0), dict(w=9), dict(mask=None, feather=0.0), dict(mode=2), dict(mode=-1), dict(seed=-1)):
        assert paste(**kw) == -1 and b"vvb_paste_blend_composite" in loaded.vvb_last_error(), kw
    for kw in (dict(feather=64.5), dict(q8=-1), dict(q8=513)):
        assert paste(**kw) == -2 and b"vvb_paste_blend_composite" in loaded.vvb_last_error(), kw
    with pytest.raises(ctypes.ArgumentError):
        loaded.vvb_pull(a, a, 1.0, 4, 4, a, a, None)
    import torch
    z = torch.zeros((2, 4, 4, 3), dtype=torch.uint8)
    offs, lut, ids = torch.zeros((2, 2), dtype=torch.int32), torch.zeros((2, 3, 256), dtype=torch.uint8), torch.zeros(2, dtype=torch.int32)
    m, f = z[..., 0].contiguous(), torch.zeros((2, 4, 4, 3), dtype=torch.int16)
    for call in (lambda: blend_hip.ring_diff(z, z, m, offs, lut, 4, 4, 2, 2, 32), lambda: blend_hip.solve(z, z, m, offs, lut, 4, 4, 2, 2, 8, 32),
                 lambda: blend_hip.pull(m, f), lambda: blend_hip.relax(m, f, 8),
                 lambda: blend_hip.paste_blend_composite(z, z, m, offs, lut, f, 256, lut, ids, 0, 0, 4, 4, 3.0)):
        with pytest.raises(RuntimeError):
            call()                                                                                   # no CPU fallback


def test_product_sources_of_the_feature():
    """vv_blend is in the one build recipe with its header among the dependencies and reads no environment; the ring and the noise have one
    statement each, which their users include; the settings import no torch; importing the drop-in resolves no symbol of the feature."""
    blend, _ = abiref.check_sources("vv_blend", "vvblend.h", "seamblend")
    grain, paste = (open(os.path.join(abiref.CSRC, f)).read() for f in ("vv_grain.hip", "vv_paste_px.h"))
    assert "getenv" not in paste
    assert '#include "vv_ring_bits.h"' in blend and "vvring::ring_bits<" in blend and "__ballot" not in blend
    for user in (blend, grain):
        assert '#include "vv_paste_px.h"' in user and "vvpaste::grain_px(" in user and "0x9E3779B97F4A7C15" not in user and "5017" not in user
    assert paste.count("0x9E3779B97F4A7C15") == 1 and paste.count("5017 + (1 << 23)) >> 24") == 1
    code = ("import diffuerase; from videovanish_amd import blend_hip, grain_hip, tone_hip, hip, seamblend; "
            "assert blend_hip.PART.dll is None and grain_hip.PART.dll is None and tone_hip.PART.dll is None and hip.CORE.dll is None; "
            "assert diffuerase.last_seam_blend is None")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ---- the level plan -------------------------------------------------------------------------------------------------------------------------
def test_level_plan_and_groups():
    assert M.level_sizes(1, 1) == [(1, 1)] and M.level_sizes(2, 2) == [(2, 2)] and M.level_sizes(3, 2) == [(3, 2), (2, 1)]
    assert M.level_sizes(37, 53) == [(37, 53), (19, 27), (10, 14), (5, 7), (3, 4), (2, 2)]
    assert M.level_sizes(1080, 1920)[-1] == (2, 2) and len(M.level_sizes(1080, 1920)) == 11
    plan, total = M.level_plan(3, 37, 53)
    at = 0
    for (val, cls, hl, wl), size in zip(plan, M.level_sizes(37, 53)):
        assert (hl, wl) == size and val == at and cls == at + 6 * 3 * hl * wl and val % 16 == 0
        at += -(-7 * 3 * hl * wl // 16) * 16
    assert total == at == M.scratch_bytes(3, 37, 53)
    # the scratch of a group stays at or below four times the bytes of the window's frames (both sides >= 2), and the groups tile the clip
    for T, h, w in ((1, 96, 130), (32, 720, 1280), (32, 512, 512), (7, 37, 53), (1, 2, 300), (3, 16, 16)):
        g = M.groups(T, h, w)
        assert g[0][0] == 0 and g[-1][1] == T and all(a[1] == b[0] for a, b in zip(g, g[1:])) and all(b > a for a, b in g)
        assert max(M.scratch_bytes(b - a, h, w) for a, b in g) <= M.SCRATCH_FACTOR * 3 * T * h * w, (T, h, w)
    assert M.groups(4, 1, 700) == [(0, 3), (3, 4)] and M.scratch_bytes(4, 1, 700) > 12 * 4 * 700     # one pixel high: 14 bytes a cell, two groups
    assert M.groups(1, 1, 700) == [(0, 1)]                                                            # never less than a frame


# ---- the report -----------------------------------------------------------------------------------------------------------------------------
def test_fit_is_the_closed_form_of_the_sums():
    rng = np.random.default_rng(5)
    s = rng.integers(0, 10 ** 6, (6, 11)).astype(np.int64)
    s[1] = 0
    s[2, 0] = 0
    s[3, 4] = 0
    f = M.fit(s)
    n, rms, nh, mx, mean = R.report(s)
    assert f.n.dtype == f.n_hole.dtype == np.int64 and (f.n == n).all() and (f.n_hole == nh).all()
    assert np.allclose(f.rms_diff, rms, rtol=1e-12, atol=0) and (f.max_shift == mx).all() and np.allclose(f.mean_shift, mean, rtol=1e-12, atol=0)
    assert not any(v[1].any() for v in f)
    assert M.fit(np.zeros((0, 11), np.int64)).rms_diff.shape == (0, 3)


def test_seam_blend_report_assembles_spans_and_windows():
    from videovanish_amd import infill
    one = lambda K, T, v: infill.SeamBlendReport(np.full((K, T), v, np.int64), np.full((K, T, 3), float(v)), np.full((K, T), v, np.int64),
                                                 np.full((K, T, 3), float(v)), np.full((K, T, 3), float(v)))
    rep = infill.seam_blend_report([one(1, 3, 5), one(2, 2, 7)], [(1, 4), (6, 8)], 9)
    assert rep.n.shape == rep.n_hole.shape == (2, 9) and rep.rms_diff.shape == rep.max_shift.shape == rep.mean_shift.shape == (2, 9, 3)
    assert rep.n.dtype == rep.n_hole.dtype == np.int64
    assert rep.n.tolist() == [[0, 5, 5, 5, 0, 0, 7, 7, 0], [0, 0, 0, 0, 0, 0, 7, 7, 0]] and (rep.n_hole == rep.n).all()
    for field in (rep.rms_diff, rep.max_shift, rep.mean_shift):
        assert field.dtype == np.float64 and (field == rep.n[..., None]).all()
    empty = infill.seam_blend_report([], [], 4)
    assert empty.n.shape == (1, 4) and not any(f.any() for f in empty)
    assert infill.seam_blend_report([], [], 4, K=3).max_shift.shape == (3, 4, 3)


# ---- accuracy, on the restatement alone -----------------------------------------------------------------------------------------------------
_fields = {}


def _case_fields(name, kind, sigma):
    """(cls, val Q6, field Q6, direct fp64 levels, orig, x, mask, shift) of one case with the default settings, computed once."""
    key = (name, kind, sigma)
    if key not in _fields:
        orig, x, mask, shift = R.case(name, kind, sigma)
        H, W = mask.shape
        cls = R.classes(mask, (0, 0, H, W), 12)
        val, _ = R.boundary(x, orig, cls, 2, 32)
        _fields[key] = (cls, val, R.solve_levels(cls, val, 8), R.direct_solve(cls, val / 64.0), orig, x, mask, shift)
    return _fields[key]


@pytest.mark.parametrize("name,kind,sigma", R.CASES)
def test_cascade_against_the_direct_solve(name, kind, sigma):
    """The integer cascade (Q6, 8 sweeps a level, parents copied down) against scipy's sparse solve of the same Dirichlet problem in fp64, on
    the unknown cells: within 1.5 times the deviation recorded in seamblend_ref.MEASURED_DEVIATION, and within one level on the clean cases
    (the default `sweeps` is chosen for that).  The direct solve itself restores the linear ramp, which is harmonic."""
    cls, val, field, direct, orig, x, mask, shift = _case_fields(name, kind, sigma)
    unk = cls == R.UNKNOWN
    assert unk.sum() == (mask > 0).sum() > 1000 and (cls == R.KNOWN).sum() > 1000
    dev = float(np.abs(field / 64.0 - direct)[unk].max())
    rec = R.MEASURED_DEVIATION[(name, kind, sigma)]
    print(f"{name} {kind} sigma {sigma}: worst deviation from the direct solve {dev:.4f} levels (recorded {rec}); direct solve against the shift "
          f"{np.abs(direct - shift)[unk].max():.3f}; largest |field| {np.abs(field).max() / 64.0:.2f}")
    assert dev <= 1.5 * rec
    if sigma == 0:
        assert dev < 1.0
        # the boundary values are the shift up to the rounding of x (half a level) and the one-sided box of the presmooth (two pixels of slope)
        slope = np.abs(np.diff(shift, axis=0)).max() + np.abs(np.diff(shift, axis=1)).max()
        known = cls == R.KNOWN
        assert np.abs(val / 64.0 - shift)[known].max() <= 0.5 + 2 * slope + 1 / 64 + (0.05 if kind == "vignette" else 0)
        if kind == "ramp":                                                                           # the maximum principle
            assert np.abs(direct - shift)[unk].max() <= 0.5 + 2 * slope + 1 / 64
    assert np.abs(field).max() <= 64 * 32                                                            # max_shift holds inside too


def test_separate_components_take_their_own_outlines():
    """Two masks in one window in different light: each component's field is its own outline's constant, which one offset for the window
    (section 13) cannot give."""
    mask = R.two_components()
    H, W = mask.shape
    orig = TR.smooth_texture(3, H, W, lo=60, hi=190)
    shift = np.zeros((H, W, 3))
    shift[:, :60] = 9
    shift[:, 60:] = -7
    x = (orig.astype(np.int64) - shift.astype(np.int64)).astype(np.uint8)
    cls = R.classes(mask, (0, 0, H, W), 12)
    val, _ = R.boundary(x, orig, cls, 2, 32)
    field = R.solve_levels(cls, val, 8)
    unk = cls == R.UNKNOWN
    assert (field[unk & (np.arange(W) < 60)[None, :]] == 9 * 64).all() and (field[unk & (np.arange(W) >= 60)[None, :]] == -7 * 64).all()


# ---- restoration and exactness, on the restatement alone ----------------------------------------------------------------------------------
def _restoration(seed):
    """(orig, x, mask, shift) [1,96,130]: section 13's smooth texture, x = clip(rint(orig + shift)) with twice the linear ramp (up to 24 levels
    across the frame, which one offset leaves half of), the box mask."""
    orig = TR.smooth_texture(seed, 96, 130)[None]
    shift = 2 * R.shift_field("ramp", 96, 130)
    x = np.clip(np.rint(orig + shift[None]), 0, 255).astype(np.uint8)
    return orig, x, R.box_mask()[None], shift


@pytest.mark.parametrize("tone", [None, "offset", "on"])
def test_reference_restores_a_shift_that_varies_across_the_hole(tone):
    """The composite with the stage comes back to the original: the error is at most 1.5 times the recorded deviation of the cascade, plus the
    boundary values' own error (the presmooth box is one-sided next to the mask: two pixels of the ramp's slope), plus half a level for
    rounding the membrane to a byte; these are integers, so that is one level.  The composite without the stage does not come back: it keeps
    the ramp, also behind tone matching, which in its "offset" mode takes only the ramp's mean and in its "affine" mode ("on") is misled by it
    (gains of 0.91 .. 1.11 for a true 1.0).  In front of the membrane the tone stage fits the offset alone, so "on" gives the bytes of "offset"
    with the stage and is held to the same bound."""
    offs = np.zeros((1, 2), np.int32)
    for seed in range(4):
        orig, x, mask, shift = _restoration(seed)
        mode = {None: None, "offset": "offset", "on": "affine"}[tone]
        out, field, cls, sums = R.apply(x, orig, mask, offs, 96, 130, 3.0, tone=None if tone is None else dict(ring=12, mode=mode))
        plain = TR.composite(x, orig, mask, offs, np.broadcast_to(R.IDENT, (1, 3, 256)), 96, 130, 3.0)
        if tone is not None:
            gain, offset = TR.fit(TR.sums(x, orig, mask, offs, 96, 130, 12), mode=mode)
            plain = TR.composite(x, orig, mask, offs, TR.tables(gain, offset), 96, 130, 3.0)
        slope = np.abs(np.diff(shift, axis=0)).max() + np.abs(np.diff(shift, axis=1)).max()
        bound = 1.5 * R.MEASURED_DEVIATION[("box", "ramp", 0)] + 2 * slope + 1 / 64 + 0.5
        err = lambda f: int(np.abs(f.astype(int) - orig.astype(int)).max())
        print(f"seed {seed}, tone {tone}: worst error of the composite {err(plain)} -> {err(out)} (bound {bound:.2f})")
        assert bound < 2 and err(out) <= bound
        assert err(plain) >= 6 and err(plain) > 2 * bound
        if tone == "on":
            assert (out == R.apply(x, orig, mask, offs, 96, 130, 3.0, tone=dict(ring=12, mode="offset"))[0]).all()
        n, rms, nh, mx, mean = R.report(sums)
        assert n[0] == (cls == R.KNOWN).sum() > 2000 and nh[0] == 30 * 50 and (mx >= mean).all() and (mean[0] > 0).all()
        f = M.fit(sums)
        assert (f.n == n).all() and np.allclose(f.rms_diff, rms) and (f.max_shift == mx).all() and np.allclose(f.mean_shift, mean)


def test_reference_without_a_difference_is_the_plain_composite():
    """A model frame that equals the original on the ring: d = 0, a zero field, the bytes of the composite without the stage; strength 0 gives
    those bytes whatever the field is."""
    offs = np.zeros((2, 2), np.int32)
    orig, _, mask = TR.restoration_clip(1.0, 0, T=2)
    x = orig.copy()
    x[mask > 0] = 255 - x[mask > 0]                                                                  # anything inside the hole
    ident = np.broadcast_to(R.IDENT, (2, 3, 256))
    plain = TR.composite(x, orig, mask, offs, ident, 96, 130, 3.0)
    out, field, cls, sums = R.apply(x, orig, mask, offs, 96, 130, 3.0)
    assert not field.any() and (out == plain).all() and (sums[:, 0] > 2000).all() and not sums[:, 1:4].any() and not sums[:, 5:].any()
    assert (sums[:, 4] == 30 * 50).all()
    orig, x, mask, _ = _restoration(1)
    out, field, cls, sums = R.apply(x, orig, mask, offs[:1], 96, 130, 3.0, strength=0.0)
    assert field.any() and (out == TR.composite(x, orig, mask, offs[:1], ident[:1], 96, 130, 3.0)).all()
    # a window the mask fills and a frame without a mask: the zero field
    full = np.full((1, 40, 40), 255, np.uint8)
    o = TR.smooth_texture(0, 40, 40)[None]
    field, cls, sums = R.solve(255 - o, o, full, offs[:1], ident[:1], 40, 40)
    assert (cls == R.UNKNOWN).all() and not field.any() and sums[0].tolist() == [0, 0, 0, 0, 1600, 0, 0, 0, 0, 0, 0]
    field, cls, sums = R.solve(255 - o, o, 0 * full, offs[:1], ident[:1], 40, 40)
    assert (cls == R.INACTIVE).all() and not field.any() and not sums.any()


# ---- infill.finish with the kernels replaced by the restatement ---------------------------------------------------------------------------
def _stand_ins(monkeypatch, calls):
    """The device entry points finish uses, as the restatement on CPU tensors."""
    import torch
    from videovanish_amd import blend_hip, grain_hip, tone_hip
    n = lambda t: t.numpy()
    th = lambda a: torch.from_numpy(np.ascontiguousarray(a))

    def solve(patch, orig, mask2d, offsets, lut, h, w, ring, presmooth, sweeps, max_shift, scratch=None):
        calls.append(("solve", len(patch), None if scratch is None else scratch.numel()))
        assert scratch is None or scratch.numel() >= M.scratch_bytes(len(patch), h, w)
        field, cls, sums = R.solve(n(patch), n(orig), n(mask2d), n(offsets), n(lut), h, w, ring, presmooth, sweeps, max_shift)
        return th(field), th(cls), th(sums)

    def paste(patch, orig, mask2d, offsets, lut, field, q8, amp, frame_ids, seed, mode, h, w, feather_px, out=None):
        calls.append(("paste", len(patch), q8))
        res = R.composite(n(patch), n(orig), n(mask2d), n(offsets), n(lut), n(field), q8, n(amp), n(frame_ids), seed, GR_MODES[mode], h, w, feather_px)
        out.copy_(th(res))
        return out

    GR_MODES = ("luma", "rgb")
    monkeypatch.setattr(blend_hip, "solve", solve)
    monkeypatch.setattr(blend_hip, "paste_blend_composite", paste)
    monkeypatch.setattr(tone_hip, "ring_stats", lambda patch, orig, mask2d, offsets, h, w, ring: th(TR.sums(n(patch), n(orig), n(mask2d), n(offsets), h, w, ring)))
    monkeypatch.setattr(grain_hip, "ring_grain_stats",
                        lambda patch, orig, mask2d, offsets, lut, h, w, ring, flat: th(GR.sums(n(patch), n(orig), n(mask2d), n(offsets), n(lut), h, w, ring, flat)))


def _report_equals(rep, k, sums):
    n, rms, nh, mx, mean = R.report(sums)
    assert (rep.n[k] == n).all() and (rep.n_hole[k] == nh).all() and (rep.max_shift[k] == mx).all()
    assert np.allclose(rep.rms_diff[k], rms, rtol=1e-12, atol=0) and np.allclose(rep.mean_shift[k], mean, rtol=1e-12, atol=0)


@pytest.mark.parametrize("stages", ["alone", "tone", "tone+grain"])
def test_finish_full_frame_with_stand_ins(monkeypatch, stages):
    import torch
    from videovanish_amd import infill
    from videovanish_amd.grainmatch import GrainMatchConfig
    from videovanish_amd.tonematch import ToneMatchConfig
    calls = []
    _stand_ins(monkeypatch, calls)
    T = 3
    orig = np.stack([np.clip(TR.smooth_texture(s, 96, 130).astype(np.float64) + np.random.default_rng(s).normal(0, 3, (96, 130, 3)), 0, 255).astype(np.uint8)
                     for s in range(T)])
    x = np.clip(np.rint(np.stack([TR.smooth_texture(s, 96, 130) for s in range(T)]) * 0.95 + 4 + R.shift_field("vignette", 96, 130)[None]), 0, 255).astype(np.uint8)
    mask = np.stack([R.box_mask(), R.two_components(), np.zeros((96, 130), np.uint8)])
    dil = torch.from_numpy(mask)
    tone = ToneMatchConfig() if "tone" in stages else None
    grain = GrainMatchConfig(seed=5, min_count=64) if "grain" in stages else None
    kw = dict(tone=tone, tone_out=[]) if tone else {}
    if grain:
        kw.update(grain=grain, grain_out=[], frame0=7)
    rows = []
    cfg = SeamBlendConfig(strength=0.75)
    out = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, True, "cpu", blend=cfg, blend_out=rows, **kw))
    offs = np.zeros((T, 2), np.int32)
    want, field, cls, sums = R.apply(x, orig, mask, offs, 96, 130, 3.0, frame_ids=[7, 8, 9], strength=0.75,
                                     tone=dict(ring=12) if tone else None, grain=dict(seed=5, min_count=64) if grain else None)
    assert (out == want).all() and field[:2].any() and not field[2].any()
    assert [c[0] for c in calls] == ["solve", "paste"] and calls[0][1] == T and calls[1] == ("paste", T, 192)
    assert calls[0][2] == M.scratch_bytes(T, 96, 130) <= 4 * 3 * T * 96 * 130
    assert len(rows) == 1 and rows[0].n.shape == (1, T)
    _report_equals(rows[0], 0, sums)
    if tone:
        assert len(kw["tone_out"]) == 1 and kw["tone_out"][0].n.shape == (1, T)
        assert (kw["tone_out"][0].gain == 1.0).all() and (kw["tone_out"][0].offset[0, :2] != 0.0).any()      # the offset alone in front of the membrane
    if grain:
        assert len(kw["grain_out"]) == 1 and kw["grain_out"][0].sigma_added.any()
    # the plain paste: every pixel of the frame gets the field
    out = np.stack(infill.finish([list(x)], list(orig), dil, [], 3, False, "cpu", blend=cfg, **kw))
    assert (out == R.apply(x, orig, mask, offs, 96, 130, -1.0, frame_ids=[7, 8, 9], strength=0.75, tone=dict(ring=12) if tone else None,
                           grain=dict(seed=5, min_count=64) if grain else None)[0]).all()


def test_finish_two_windows_and_groups_with_stand_ins(monkeypatch):
    """K = 2 windows with their own shifts, the second pasted into the first's output; frames another rank holds stay None with zero rows; a
    group size below the clip's length solves group after group over one scratch buffer."""
    import torch
    from videovanish_amd import infill
    calls = []
    _stand_ins(monkeypatch, calls)
    T, H, W = 4, 96, 130
    orig = np.stack([TR.smooth_texture(10 + s, H, W) for s in range(T)])
    wins = [((0, 0), (48, 64), (12, 15, 30, 40), "ramp"), ((50, 70), (40, 56), (60, 85, 75, 110), "vignette")]
    mask = np.zeros((T, H, W), np.uint8)
    plans, outs = [], []
    for (oy, ox), (h, w), (y0, x0, y1, x1), kind in wins:
        mask[:, y0:y1, x0:x1] = 255
        offs = np.tile(np.array([[oy, ox]], np.int32), (T, 1))
        plans.append(types.SimpleNamespace(size=(h, w), offsets=offs))
        outs.append(list(np.clip(np.rint(orig[:, oy:oy + h, ox:ox + w] + R.shift_field(kind, h, w)[None]), 0, 255).astype(np.uint8)))
    outs[0][2] = None                                                                                # a frame another rank holds
    idx = [0, 1, 3]
    monkeypatch.setattr(M, "groups", lambda T, h, w: [(0, 2), (2, T)])
    rows = []
    out = infill.finish(outs, list(orig), torch.from_numpy(mask), plans, 3, True, "cpu", blend=SeamBlendConfig(), blend_out=rows)
    assert out[2] is None
    want = orig[idx]
    assert len(rows) == 1 and rows[0].n.shape == (2, T)
    for k, (plan, o) in enumerate(zip(plans, outs)):
        want, field, cls, sums = R.apply(np.stack([o[i] for i in idx]), want, mask[idx], plan.offsets[idx], *plan.size, 3.0, frame_ids=idx)
        full = np.zeros((T, 11), np.int64)
        full[idx] = sums
        _report_equals(rows[0], k, full)
    assert (np.stack([out[i] for i in idx]) == want).all()
    assert np.abs(want.astype(int) - orig[idx].astype(int)).max() <= 2
    assert [c[:2] for c in calls] == [("solve", 2), ("paste", 2), ("solve", 1), ("paste", 1)] * 2
    assert calls[0][2] == calls[2][2] == M.scratch_bytes(2, 48, 64)                                   # one buffer per window, sized for the first group


def _all_stand_ins(monkeypatch, calls, on):
    """Every device entry point finish can end a window in or measure with, as its restatement on CPU tensors; calls gets (name, frames) per
    call.  A binding whose stage is not in `on` raises from every entry point and from lib()."""
    import torch
    from videovanish_amd import blend_hip, grain_hip, hip, tone_hip
    n = lambda t: t.numpy()
    th = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    ident = lambda T: np.broadcast_to(R.IDENT, (T, 3, 256))

    def into(out, res):
        out.copy_(th(res))
        return out

    def said(name, fn):
        def f(patch, *a, **k):
            calls.append((name, len(patch)))
            return fn(patch, *a, **k)
        return f

    stand = {
        (tone_hip, "ring_stats"): lambda patch, orig, mask, offs, h, w, ring: th(TR.sums(n(patch), n(orig), n(mask), n(offs), h, w, ring)),
        (tone_hip, "paste_lut_composite"): lambda patch, orig, mask, offs, lut, h, w, feather, out=None:
            into(out, TR.composite(n(patch), n(orig), n(mask), n(offs), n(lut), h, w, feather)),
        (grain_hip, "ring_grain_stats"): lambda patch, orig, mask, offs, lut, h, w, ring, flat:
            th(GR.sums(n(patch), n(orig), n(mask), n(offs), n(lut), h, w, ring, flat)),
        (grain_hip, "paste_grain_composite"): lambda patch, orig, mask, offs, lut, amp, ids, seed, mode, h, w, feather, out=None:
            into(out, GR.composite(n(patch), n(orig), n(mask), n(offs), n(lut), n(amp), n(ids), seed, ("luma", "rgb")[mode], h, w, feather)),
        (blend_hip, "solve"): lambda patch, orig, mask, offs, lut, h, w, ring, presmooth, sweeps, max_shift, scratch=None:
            tuple(th(v) for v in R.solve(n(patch), n(orig), n(mask), n(offs), n(lut), h, w, ring, presmooth, sweeps, max_shift)),
        (blend_hip, "paste_blend_composite"): lambda patch, orig, mask, offs, lut, field, q8, amp, ids, seed, mode, h, w, feather, out=None:
            into(out, R.composite(n(patch), n(orig), n(mask), n(offs), n(lut), n(field), q8, n(amp), n(ids), seed, ("luma", "rgb")[mode], h, w, feather)),
        (hip, "roi_paste_composite"): lambda patch, orig, mask, offs, h, w, feather, out=None:
            into(out, TR.composite(n(patch), n(orig), n(mask), n(offs), ident(len(patch)), h, w, feather)),
        (hip, "feather_composite"): lambda x, orig, mask, feather:
            th(TR.composite(n(x), n(orig), n(mask), np.zeros((len(x), 2), np.int32), ident(len(x)), *x.shape[1:3], feather)),
    }
    stage_of = {tone_hip: "tone", grain_hip: "grain", blend_hip: "blend"}
    for (mod, name), fn in stand.items():
        if stage_of.get(mod, "") in on or mod is hip:
            monkeypatch.setattr(mod, name, said(name, fn))
        else:
            boom = lambda *a, _what=f"{mod.__name__}.{name}", **k: (_ for _ in ()).throw(AssertionError(f"{_what} called with its stage off"))
            monkeypatch.setattr(mod, name, boom)
            monkeypatch.setattr(mod, "lib", boom)


def _matrix_clip(layout):
    """(orig [T,H,W,3], mask [T,H,W], windows [(offsets [T,2], (h, w), model frames [T,h,w,3])], plans for finish, the frames this rank holds)."""
    H, W = 96, 130
    if layout == "full":            # test_finish_full_frame_with_stand_ins' clip
        T = 3
        orig = np.stack([np.clip(TR.smooth_texture(s, H, W).astype(np.float64) + np.random.default_rng(s).normal(0, 3, (H, W, 3)), 0, 255).astype(np.uint8)
                         for s in range(T)])
        x = np.clip(np.rint(np.stack([TR.smooth_texture(s, H, W) for s in range(T)]) * 0.95 + 4 + R.shift_field("vignette", H, W)[None]), 0, 255).astype(np.uint8)
        mask = np.stack([R.box_mask(), R.two_components(), np.zeros((H, W), np.uint8)])
        return orig, mask, [(np.zeros((T, 2), np.int32), (H, W), x)], [], [0, 1, 2]
    T = 4                           # test_finish_two_windows_and_groups_with_stand_ins' windows, the originals with grain
    smooth = np.stack([TR.smooth_texture(10 + s, H, W) for s in range(T)])
    orig = np.clip(smooth + np.random.default_rng(3).normal(0, 3, smooth.shape), 0, 255).astype(np.uint8)
    mask = np.zeros((T, H, W), np.uint8)
    wins = []
    for (oy, ox), (h, w), (y0, x0, y1, x1), kind in [((0, 0), (48, 64), (12, 15, 30, 40), "ramp"), ((50, 70), (40, 56), (60, 85, 75, 110), "vignette")]:
        mask[:, y0:y1, x0:x1] = 255
        offs = np.tile(np.array([[oy, ox]], np.int32), (T, 1))
        wins.append((offs, (h, w), np.clip(np.rint(smooth[:, oy:oy + h, ox:ox + w] * 0.95 + 4 + R.shift_field(kind, h, w)[None]), 0, 255).astype(np.uint8)))
    return orig, mask, wins, [types.SimpleNamespace(size=s, offsets=o) for o, s, _ in wins], [0, 1, 3]


_MATRIX_WANT = {}


def _matrix_want(layout, on, feather):
    """The chained references over all T frames; the frame another rank holds has no mask pixel there (no ring: zero sums, nothing pooled from
    it, as finish's zero rows), and its bytes are not compared."""
    key = (layout, on, feather)
    if key not in _MATRIX_WANT:
        orig, mask, wins, _, idx = _matrix_clip(layout)
        T = len(orig)
        held = np.zeros(T, bool)
        held[idx] = True
        mask = np.where(held[:, None, None], mask, 0).astype(np.uint8)
        ids = [7 + t for t in range(T)]
        tone = dict(ring=12) if "tone" in on else None
        want = orig
        for offs, (h, w), x in wins:
            if "blend" in on:
                want = R.apply(x, want, mask, offs, h, w, feather, frame_ids=ids, strength=0.75, tone=tone,
                               grain=dict(seed=5, min_count=64) if "grain" in on else None)[0]
            elif "grain" in on:
                want = GR.apply(x, want, mask, offs, h, w, feather, ids, tone=tone, seed=5, min_count=64)[0]
            elif "tone" in on:
                want = TR.apply(x, want, mask, offs, h, w, feather, ring=12)[0]
            else:
                want = TR.composite(x, want, mask, offs, np.broadcast_to(R.IDENT, (T, 3, 256)), h, w, feather)
        _MATRIX_WANT[key] = want
    return _MATRIX_WANT[key]


@pytest.mark.parametrize("on", [(), ("tone",), ("grain",), ("blend",), ("tone", "grain"), ("tone", "blend"), ("grain", "blend"), ("tone", "grain", "blend")],
                         ids=lambda on: "+".join(on) or "none")
@pytest.mark.parametrize("layout", ["full", "windows"])
def test_finish_stage_matrix_with_stand_ins(monkeypatch, layout, on):
    """Every subset of {tone, grain, blend} on the full frame and on two windows (one frame held by another rank), the feathered composite and
    the plain paste: the bytes of the chained restatements, exactly the entry points of that subset (a stage that is off contributes no
    call and resolves nothing of its binding), and one [K,T,...] report per requested list with zero / identity rows for the frame this rank
    does not hold."""
    import torch
    from videovanish_amd import infill
    from videovanish_amd.grainmatch import GrainMatchConfig
    from videovanish_amd.tonematch import ToneMatchConfig
    calls = []
    _all_stand_ins(monkeypatch, calls, on)
    orig, mask, wins, plans, idx = _matrix_clip(layout)
    T, K, n = len(orig), len(wins), len(idx)
    groups = [(0, n)] if layout == "full" else [(0, 2), (2, n)]
    monkeypatch.setattr(M, "groups", lambda T, h, w: groups)
    cfgs = dict(tone=ToneMatchConfig(), grain=GrainMatchConfig(seed=5, min_count=64), blend=SeamBlendConfig(strength=0.75))
    for keep in (True, False):
        del calls[:]
        outs = [[f if t in idx else None for t, f in enumerate(x)] for _, _, x in wins]
        kw = {}
        for s in on:
            kw.update({s: cfgs[s], s + "_out": []})
        if "grain" in on or "blend" in on:
            kw["frame0"] = 7
        got = infill.finish(outs, list(orig), torch.from_numpy(mask), plans, 3, keep, "cpu", **kw)
        assert [t for t in range(T) if got[t] is not None] == idx
        want = _matrix_want(layout, on, 3.0 if keep else -1.0)
        assert (np.stack([got[t] for t in idx]) == want[idx]).all()
        assert (want[idx] != orig[idx]).any()
        per_window = [("ring_stats", n)] * ("tone" in on) + [("ring_grain_stats", n)] * ("grain" in on)
        if "blend" in on:
            per_window += [(name, b - a) for a, b in groups for name in ("solve", "paste_blend_composite")]
        elif "grain" in on:
            per_window += [("paste_grain_composite", n)]
        elif "tone" in on:
            per_window += [("paste_lut_composite", n)]
        elif plans:
            per_window += [("roi_paste_composite", n)]
        elif keep:
            per_window += [("feather_composite", n)]
        assert calls == per_window * K
        away = [t for t in range(T) if t not in idx]
        for s in on:
            rows = kw[s + "_out"]
            assert len(rows) == 1
            for name, field in rows[0]._asdict().items():
                assert field.shape[:2] == (K, T)
                assert (field[:, away] == (1.0 if (s, name) == ("tone", "gain") else 0.0)).all()
            assert all((rows[0].n[k, idx[0]] > 0).any() for k in range(K))
        if "tone" in on and "blend" in on:
            assert (kw["tone_out"][0].gain == 1.0).all()                                            # the offset alone in front of the membrane
        if on == ("tone",):
            assert (kw["tone_out"][0].gain != 1.0).any()


def test_finish_without_the_option_calls_nothing_of_the_feature(monkeypatch):
    """No blend=: the tone path calls what it called before, nothing of blend_hip; run_clip passes the new keywords only when the stage is on."""
    import torch
    from videovanish_amd import blend_hip, infill, tone_hip
    from videovanish_amd.tonematch import ToneMatchConfig
    calls = []
    _stand_ins(monkeypatch, calls)
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("a seam blending call without seam_blend="))
    monkeypatch.setattr(blend_hip, "solve", boom)
    monkeypatch.setattr(blend_hip, "paste_blend_composite", boom)
    monkeypatch.setattr(blend_hip, "lib", boom)
    orig, x, mask = TR.restoration_clip(0.9, 10, T=2)

    def paste_lut(patch, orig_t, mask2d, offsets, lut, h, w, feather_px, out=None):
        out.copy_(torch.from_numpy(TR.composite(patch.numpy(), orig_t.numpy(), mask2d.numpy(), offsets.numpy(), lut.numpy(), h, w, feather_px)))
        return out

    monkeypatch.setattr(tone_hip, "paste_lut_composite", paste_lut)
    out = np.stack(infill.finish([list(x)], list(orig), torch.from_numpy(mask), [], 3, True, "cpu", tone=ToneMatchConfig()))
    assert (out == TR.apply(x, orig, mask, np.zeros((2, 2), np.int32), 96, 130, 3.0)[0]).all()
    seen = []
    monkeypatch.setattr(infill, "finish", lambda *a, **kw: seen.append(kw) or "done")
    monkeypatch.setattr(infill, "run_windows", lambda *a: [[]])
    frames = list(orig)
    assert infill.run_clip(frames, torch.from_numpy(mask), None, None, None, None, "cpu") == "done"
    assert infill.run_clip(frames, torch.from_numpy(mask), None, None, None, None, "cpu", blend=SeamBlendConfig(), blend_out=[]) == "done"
    assert seen[0] == {} and seen[1] == {"blend": SeamBlendConfig(), "blend_out": []}


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_precedence_argument_configure_environment(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_SEAM_BLEND", raising=False)
    try:
        diffuerase.configure()
        assert diffuerase.seam_blend_config() is None
        monkeypatch.setenv("VV_SEAM_BLEND", "ring=9")
        assert diffuerase.seam_blend_config() == SeamBlendConfig(ring=9)
        diffuerase.configure(seam_blend="sweeps=4")
        assert diffuerase.seam_blend_config() == SeamBlendConfig(sweeps=4)
        assert diffuerase.seam_blend_config("on") == SeamBlendConfig()
        assert diffuerase.seam_blend_config("off") is None and diffuerase.seam_blend_config(False) is None     # none whatever else is set
        diffuerase.configure(seam_blend="off")
        assert diffuerase.seam_blend_config() is None                                                      # configure("off") beats the environment
        diffuerase.configure()
        assert diffuerase.seam_blend_config() == SeamBlendConfig(ring=9)                                   # configure() resets
        with pytest.raises(ValueError, match="feather_px"):
            diffuerase.seam_blend_config(feather_px=9)
        cfg = SeamBlendConfig(presmooth=0)
        diffuerase.configure(seam_blend=cfg)
        assert diffuerase.seam_blend_config() is cfg
        with pytest.raises(ValueError):
            diffuerase.configure(seam_blend="sometimes")
        assert diffuerase.seam_blend_config() is cfg                                                       # a refused value changes nothing
        monkeypatch.setenv("VV_SEAM_BLEND", "sometimes")
        diffuerase.configure()
        with pytest.raises(ValueError):
            diffuerase.seam_blend_config()
    finally:
        diffuerase.configure()


def test_seam_blend_refuses_the_reference_early_return_and_a_narrow_ring(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_SEAM_BLEND", raising=False)
    f = [np.zeros((8, 8, 3), np.uint8)] * 2
    for value in ("on", "ring=4", SeamBlendConfig(), True):
        with pytest.raises(ValueError, match="seam_blend="):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, seam_blend=value)
    monkeypatch.setenv("VV_SEAM_BLEND", "on")
    with pytest.raises(ValueError, match="seam_blend="):
        diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)
    monkeypatch.delenv("VV_SEAM_BLEND")
    with pytest.raises(ValueError, match="feather_px"):
        diffuerase.run_infill_on_frames(f, f, seam_blend="ring=3")                                         # the default feather is 3
    with pytest.raises(ValueError, match="feather_px"):
        diffuerase.run_infill_on_frames(f, f, seam_blend="on", feather_px=12)
    with pytest.raises(TypeError):
        diffuerase.run_infill_on_frames(f, f, seamblend="on")
    assert diffuerase.last_seam_blend is None


def test_cli_seam_blend_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
    """tests/test_cli_cpu.py's stub: frame I/O and the hot path replaced."""
    import diffuerase
    from videovanish_amd import infill
    calls = []
    videos = {"mask.mkv": [np.zeros((16, 24, 3), np.uint8)] * 3}
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda path, start=0, max_frames=-1: ([f.copy() for f in videos[path]], 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    rep = infill.seam_blend_report([], [], 3)
    rep.max_shift[0, 1] = (0.0, 2.5, 0.0)
    rep.max_shift[0, 2, 2] = 3.257
    rep.rms_diff[0, 1, 0] = 4.126

    def fake(frames, masks, **kw):
        calls.append(kw)
        diffuerase.last_seam_blend = rep if "seam_blend" in kw else None
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 3
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    monkeypatch.setattr(sys, "argv", argv)
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None} and capsys.readouterr().out == ""                      # a default call passes no keyword, prints nothing
    for value in ("on", "ring=12,presmooth=2,sweeps=8,max_shift=32,strength=1.0", "sweeps=16"):
        monkeypatch.setattr(sys, "argv", argv + ["--seam-blend", value, "--roi", "static"])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "seam_blend": value, "roi": "static"}
        out = capsys.readouterr().out
        assert out.count("\n") == 1 and out == "seam blend: membrane added in 2 of 3 frames, largest |shift| 3.26, largest ring RMS 4.13\n"
    monkeypatch.setattr(sys, "argv", argv + ["--seam-blend", "on", "--tone-match", "on", "--grain-match", "luma"])
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None, "seam_blend": "on", "tone_match": "on", "grain_match": "luma"}
    capsys.readouterr()
    for bad in ("off", "yes", "ring=x", "ring=40", "sweeps=17"):
        monkeypatch.setattr(sys, "argv", argv + ["--seam-blend", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_seam_blend", None)
