"""Block-matched inpaint deflicker on the CPU: the binding of include/flicklocal.h, the product sources, the invariants of the restatement
(tests/deflickerlocal_ref.py) against the unaligned and the aligned ones (tests/deflicker_ref.py, tests/deflickeralign_ref.py), the recovery of
two planes' displacements, the rule on the two-plane flicker clip, the report, configuration and CLI."""
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
import deflickeralign_ref as RA  # noqa: E402
import deflickerlocal_ref as R  # noqa: E402

from videovanish_amd import deflickerlocal as DL  # noqa: E402
from videovanish_amd.deflickerlocal import DeflickerLocalConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_settings_parser():
    assert DL.SPELLINGS == ("on",) and (DL.BLOCKS, DL.MAX_SEARCH, DL.MAX_LAM, DL.NSTAT) == ((8, 16), 8, 65535, R.NSTAT)
    for off in (None, False, "off", "none", "", " OFF "):
        assert DL.as_config(off) is None
    assert DL.as_config("on") == DL.as_config(True) == DeflickerLocalConfig() == DeflickerLocalConfig(**R.DEFAULTS)
    assert DL.as_config(" search = 2 , block=16 ") == DeflickerLocalConfig(block=16, search=2)
    assert DL.as_config("lam=0") == DeflickerLocalConfig(lam=0) and DL.as_config("block=8,search=0,lam=65535") == DeflickerLocalConfig(8, 0, 65535)
    cfg = DeflickerLocalConfig(search=8)
    assert DL.as_config(cfg) is cfg
    for bad in ("yes", "search", "search=9", "block=12", "block=4", "lam=65536", "lam=-1", "radius=2", "search=1,search=2", "search=1.5", 3, ("on",)):
        with pytest.raises(ValueError):
            DL.as_config(bad)
    with pytest.raises(ValueError, match="deflicker_local must be"):
        DL.as_config("sometimes")
    for kw in (dict(block=True), dict(search=2.0), dict(lam="3")):
        with pytest.raises(ValueError, match="must be an integer"):
            DeflickerLocalConfig(**kw)


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_flicklocal_header():
    """flicklocal_bind.SIGNATURES declares every function of include/flicklocal.h with the header's types and in its order, lib() has applied
    it, the version and the limits agree (abiref.check_binding); arguments are refused before anything touches a device, each refusal naming
    its function; the vvk_ prefix, the header and every name belong to no other part (what test_abi_cpu.py's walk does for the parts of its
    table)."""
    from videovanish_amd import flickalign_hip, flicklocal_bind as B
    loaded, define = abiref.check_binding(B, 4)
    assert B.EXPORTS == ["vvk_abi_version", "vvk_last_error", "vvk_search", "vvk_hold"] and define("VVK_ABI_VERSION") == 1
    limits = (define("VVK_MAX_RADIUS"), define("VVK_MAX_T"), define("VVK_TRACK_INTS"), define("VVK_MAX_SEARCH"), define("VVK_MAX_LAM"), define("VVK_MV_INTS"),
              define("VVK_NSTAT"))
    assert limits == (B.MAX_RADIUS, B.MAX_T, B.TRACK_INTS, B.MAX_SEARCH, B.MAX_LAM, B.MV_INTS, B.NSTAT) == (4, 65535, 8, 8, 65535, 4, 6)
    assert limits[:3] == (flickalign_hip.MAX_RADIUS, flickalign_hip.MAX_T, flickalign_hip.TRACK_INTS) and limits[3:5] == (DL.MAX_SEARCH, DL.MAX_LAM)
    assert B.BLOCKS == DL.BLOCKS and B.NSUM == flickalign_hip.NSUM == R.NSUM == 12 and B.NSTAT == DL.NSTAT
    raw = open(os.path.join(ROOT, "include", "flicklocal.h")).read()
    for rule in ("D(t, s) = e_t - e_s", "nby = ceil(h / block)", "lexicographic minimum of (cost, dy^2 + dx^2, dy, dx)", "lam * (|dy|", "(dy, dx, 1, cost)",
                 "(0, 0, 0, 0)", "mv[t][k][yy / block][xx / block]", "Every int of mv is written", "mv is data"):
        assert rule in raw, rule                                                                     # the rules are part of the ABI
    # Nothing can be launched here: every pointer is host memory and every call below is refused before the first device call.
    buf = (ctypes.c_char * 64)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 32
    search = lambda win=a, offs=a, track=a, mv=a, stats=a, T=2, h=8, w=8, radius=1, block=8, s=4, lam=32: \
        loaded.vvk_search(win, offs, track, T, h, w, radius, block, s, lam, mv, stats, None)
    hold = lambda win=a, offs=a, track=a, mv=a, mask=a, out=b, sums=a, T=2, H0=8, W0=8, h=8, w=8, radius=1, block=8, tol=1: \
        loaded.vvk_hold(win, offs, track, mv, mask, T, H0, W0, h, w, radius, block, tol, out, sums, None)
    for kw in (dict(win=None), dict(offs=None), dict(track=None), dict(mv=None), dict(stats=None), dict(T=0), dict(h=0), dict(w=-1), dict(radius=-1), dict(block=0),
               dict(block=-8), dict(s=-1), dict(lam=-1)):
        assert search(**kw) == -1 and loaded.vvk_last_error().startswith(b"vvk_search:"), kw
    for kw in (dict(block=4), dict(block=12), dict(block=32), dict(s=9), dict(lam=65536), dict(radius=5), dict(T=65536), dict(h=1 << 16, w=1 << 15)):
        assert search(**kw) == -2 and loaded.vvk_last_error().startswith(b"vvk_search:"), kw
    assert search(s=9, T=0) == -1                                                                    # a bad argument before an unsupported one
    for kw in (dict(win=None), dict(offs=None), dict(track=None), dict(mv=None), dict(mask=None), dict(out=None), dict(sums=None), dict(T=0), dict(H0=0), dict(W0=0),
               dict(h=0), dict(w=0), dict(h=9), dict(w=9), dict(radius=-1), dict(block=0), dict(tol=-1), dict(out=a)):
        assert hold(**kw) == -1 and loaded.vvk_last_error().startswith(b"vvk_hold:"), kw
    for kw in (dict(block=12), dict(radius=5), dict(tol=256), dict(T=65536), dict(H0=1 << 16, W0=1 << 15, h=1 << 16, w=1 << 15)):
        assert hold(**kw) == -2 and loaded.vvk_last_error().startswith(b"vvk_hold:"), kw
    assert loaded.vvk_last_error() == flickalign_hip.lib().vvc_last_error()                          # one message per thread, whatever the part
    with pytest.raises(ctypes.ArgumentError):
        search(lam=2.0)
    with pytest.raises(ctypes.ArgumentError):
        hold(block=8.0)
    import torch
    f, z = torch.zeros((2, 8, 8, 3), dtype=torch.uint8), torch.zeros((2, 8, 8), dtype=torch.uint8)
    o, tr, mv = torch.zeros((2, 2), dtype=torch.int32), torch.zeros((2, 8), dtype=torch.int32), torch.zeros((2, 3, 1, 1, 4), dtype=torch.int32)
    for call in (lambda: B.search(f, o, tr, 1, DeflickerLocalConfig()), lambda: B.search(f, o, None, 1, DeflickerLocalConfig()),
                 lambda: B.hold(f, o, tr, mv, z, 1, 8, 12), lambda: B.hold(f, o, None, mv, z, 1, 8, 12)):
        with pytest.raises(RuntimeError):                                                            # no CPU fallback
            call()
    assert B.blocks(40, 56, 8) == (5, 7) and B.blocks(40, 56, 16) == (3, 4) and B.blocks(45, 83, 8) == (6, 11)
    # the part stands outside abiref.PARTS: its prefix, header and names are checked against every part here
    assert "flicklocal_bind" not in abiref.PARTS and abiref.part_of(B) is B.PART and B.PART.header == "flicklocal.h"
    assert re.fullmatch(r"vv[a-z]_", B.PART.prefix)
    from videovanish_amd import detailmatch_bind, grainshape_bind, platetone_bind
    names = set(B.SIGNATURES)
    outside = [(m, m.PART) for m in (platetone_bind, detailmatch_bind, grainshape_bind)]
    for module, part in abiref.parts() + outside:
        assert part.prefix != B.PART.prefix and part.header != B.PART.header, module.__name__
        assert not names & set(module.SIGNATURES), module.__name__
        assert not [n for n in module.SIGNATURES if n.startswith(B.PART.prefix)], module.__name__
    assert all(n.startswith("vvk_") for n in names)
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != "flicklocal.h":
            assert "vvk_" not in open(os.path.join(ROOT, "include", header)).read().lower(), header  # no header used the prefix before


def test_product_sources_of_the_feature():
    """The kernels live in a unit of their own, in the one recipe with the header among the dependencies; no environment; the reductions come
    from the shared header; the search uses the packed-byte SAD on byte-aligned LDS dwords and a 64-bit key; the settings import no torch;
    importing the drop-in and asking for the setting resolves no vvk_ symbol."""
    kernel, txt = abiref.check_sources("vv_flicklocal", "flicklocal.h", "deflickerlocal")
    for fn in ("vvk_search", "vvk_hold"):
        assert f'extern "C" int {fn}(' in kernel
    for used in ('#include "vv_wave_bytes.h"', "using vvwave::wave_sum;", "__builtin_amdgcn_sad_u8(", "__builtin_amdgcn_alignbyte(", "__shared__ unsigned area[",
                 "__shared__ unsigned ref[", "wave_min64(", "static_assert(recip_exact()"):
        assert used in kernel, used
    assert "vv_flicklocal" not in open(os.path.join(abiref.CSRC, "vv_flicker.hip")).read()          # vvf_hold and vvc_hold stay as they are
    assert "import ctypes" not in txt
    code = ("import sys, diffuerase; from videovanish_amd import flicklocal_bind, flickalign_hip, flicker_hip, hip; "
            "assert flicklocal_bind.PART.dll is None and flickalign_hip.PART.dll is None and flicker_hip.PART.dll is None and hip.CORE.dll is None; "
            "assert diffuerase.deflicker_local_config() is None and diffuerase.last_deflicker_local is None")
    env = {k: v for k, v in os.environ.items() if k not in ("VV_DEFLICKER", "VV_DEFLICKER_ALIGN", "VV_DEFLICKER_LOCAL")}
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)
    code = "import sys, videovanish_amd.deflickerlocal as d; assert 'torch' not in sys.modules and d.as_config('on').search == 4"
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)


# ---- invariants of the restatement --------------------------------------------------------------------------------------------------------
def _random_clip(seed, T=9, h=20, w=27, H0=28, W0=36, moving=True):
    """One background fixed in the frame seen through windows, +-9 levels of noise, a real change, a random mask."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H0, W0, 3))
    offsets = np.stack([rng.integers(0, H0 - h + 1, T), rng.integers(0, W0 - w + 1, T)], 1) if moving else np.tile([[3, 5]], (T, 1))
    win = np.stack([base[oy:oy + h, ox:ox + w] for oy, ox in offsets]) + rng.integers(-9, 10, (T, h, w, 3))
    win[T // 2:, :, w // 2:] += 60
    mask = (rng.random((T, H0, W0)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (T, H0, W0)).astype(np.uint8)
    return np.clip(win, 0, 255).astype(np.uint8), offsets.astype(np.int32), mask


def _panned_clip(seed, off, T=9, h=20, w=27, H0=28, W0=36):
    """One background fixed on the CANVAS: the window pixel (yy, xx) of frame t shows wide[offsets[t] + (yy, xx) + off[t]]; +-5 levels of noise."""
    rng = np.random.default_rng(seed)
    offsets = np.stack([rng.integers(0, H0 - h + 1, T), rng.integers(0, W0 - w + 1, T)], 1)
    ey, ex = offsets[:, 0] + off[:, 1], offsets[:, 1] + off[:, 0]
    wide = rng.integers(0, 256, (ey.max() - ey.min() + h, ex.max() - ex.min() + w, 3))
    win = np.stack([wide[y - ey.min():y - ey.min() + h, x - ex.min():x - ex.min() + w] for y, x in zip(ey, ex)]) + rng.integers(-5, 6, (T, h, w, 3))
    mask = (rng.random((T, H0, W0)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (T, H0, W0)).astype(np.uint8)
    return np.clip(win, 0, 255).astype(np.uint8), offsets.astype(np.int32), mask


def _zero_records(T, radius, h, w, block):
    mv = np.zeros((T, 2 * radius + 1, -(-h // block), -(-w // block), 4), np.int32)
    mv[..., 2] = 1
    return mv


@pytest.mark.parametrize("moving", [False, True])
def test_no_byte_moves_more_than_tol_and_the_identity_settings(moving):
    win, offs, mask = _random_clip(5, moving=moving)
    T, h, w, _ = win.shape
    changed = 0
    for radius, block, search, lam, tol in ((1, 8, 1, 0, 4), (2, 8, 4, 32, 12), (4, 16, 8, 65535, 255), (2, 16, 2, 0, 0), (0, 8, 4, 32, 12)):
        mv, stats = R.search(win, offs, None, radius, block, search, lam)
        out, sums = R.hold(win, offs, None, mv, mask, radius, block, tol)
        d = np.abs(out.astype(int) - win.astype(int))
        assert d.max() <= tol and (sums[:, 0] == h * w).all() and (sums[:, 3:6] == d.reshape(T, -1, 3).sum(1)).all() and (sums[:, 6:] <= sums[:, :6]).all()
        assert mv.shape == (T, 2 * radius + 1, -(-h // block), -(-w // block), 4) and not mv[:, radius].any() and set(np.unique(mv[..., 2])) <= {0, 1}
        assert (np.abs(mv[..., :2]) <= search).all() and (mv[..., 3] >= 0).all() and (stats[:, :, 0] == mv[..., 2].sum((2, 3))).all()
        assert (stats[:, :, 4] == mv[..., 3].sum((2, 3))).all() and (stats[:, :, 3] == np.abs(mv[..., :2]).max((2, 3, 4))).all()
        if radius == 0 or tol == 0:
            assert (out == win).all() and not sums[:, [1, 3, 4, 5, 7, 9, 10, 11]].any()             # the identity
        if radius == 0:
            assert (sums[:, 2] == h * w).all() and not stats.any()
        changed += int(sums[:, 1].sum())
    assert changed


def test_search_zero_on_fixed_windows_is_the_unaligned_rule():
    win, offs, mask = _random_clip(7, moving=False)
    for radius, block, tol in ((1, 8, 4), (2, 16, 12), (4, 8, 255)):
        mv, stats = R.search(win, offs, None, radius, block, 0, 32)
        assert not mv[..., :2].any() and (stats[:, :, 4] == stats[:, :, 5]).all() and not stats[:, :, 1:4].any()
        out, sums = R.hold(win, offs, None, mv, mask, radius, block, tol)
        want, wsums = R0.hold(win, offs, mask, radius, tol)
        assert (out == want).all() and (sums == wsums).all() and (out != win).any()


@pytest.mark.parametrize("block", [8, 16])
def test_zero_vectors_are_the_aligned_rule(block):
    """With every record (0, 0, 1, .) the rule is vvflickalign.h's, whatever the track and the windows' places."""
    T = 9
    off = RA.walk(T, 11, (-3, 4), (-2, 2))
    win, offs, mask = _panned_clip(6, off)
    h, w = win.shape[1:3]
    far = np.stack([np.arange(T) * (w + 1), np.arange(T) * -(h + 1)], 1)
    for track in (RA.make_track(off), RA.make_track(off, lost=(3, T - 1)), RA.make_track(np.zeros((T, 2), int)), RA.make_track(far * (1 << 23))):
        for radius, tol in ((1, 4), (2, 12), (4, 255)):
            mv = _zero_records(T, radius, h, w, block)
            mv[..., 3] = np.random.default_rng(radius).integers(-(2 ** 31), 2 ** 31, mv.shape[:-1])    # the cost is not read
            out, sums = R.hold(win, offs, track, mv, mask, radius, block, tol)
            want, wsums = RA.hold(win, offs, track, mask, radius, tol)
            assert (out == want).all() and (sums == wsums).all()
    mv[..., 2] = 2                                                                                   # only a third int of 1 gives a sample
    out, sums = R.hold(win, offs, RA.make_track(off), mv, mask, 4, block, 255)
    assert (out == win).all() and (sums[:, 2] == h * w).all()


def test_lost_frames_take_no_sample_and_give_none():
    T, L = 9, 4
    off = RA.walk(T, 3, (-2, 3), (-1, 1))
    win, offs, mask = _panned_clip(8, off)
    h, w = win.shape[1:3]
    track = RA.make_track(off, lost=(L,))
    mv, stats = R.search(win, offs, track, 2, 8, 2, 32)
    assert not mv[L].any() and not stats[L].any()
    for s in range(L - 2, L + 3):
        assert not mv[s, L - s + 2].any() and not stats[s, L - s + 2].any()
    out, sums = R.hold(win, offs, track, mv, mask, 2, 8, 12)
    assert (out[L] == win[L]).all() and sums[L, 2] == h * w and not sums[L, [1, 3, 4, 5, 7, 9, 10, 11]].any()
    full_mv, _ = R.search(win, offs, RA.make_track(off), 2, 8, 2, 32)
    full, _ = R.hold(win, offs, RA.make_track(off), full_mv, mask, 2, 8, 12)
    assert (full[L] != win[L]).any() and (out[[L - 1, L + 1]] != full[[L - 1, L + 1]]).any()       # tracked, it would have taken and given
    other = win.copy()                                                                              # nothing of a lost frame is read
    other[L] = 255 - other[L]
    mv2, stats2 = R.search(other, offs, track, 2, 8, 2, 32)
    out2, sums2 = R.hold(other, offs, track, mv2, mask, 2, 8, 12)
    others = [t for t in range(T) if t != L]
    assert (mv2 == mv).all() and (stats2 == stats).all() and (out2[others] == out[others]).all() and (sums2[others] == sums[others]).all()
    none_mv, none_stats = R.search(win, offs, RA.make_track(off, lost=range(T)), 4, 16, 4, 0)
    assert not none_mv.any() and not none_stats.any()


def test_the_winner_does_not_depend_on_the_order_of_the_walk():
    """Flat runs, a constant clip and a clip periodic in x make ties; a shuffled and a reversed walk give the same mv and stats."""
    rng = np.random.default_rng(3)
    win, offs, mask = _random_clip(9)
    win[:, :8] = win[:, :8] // 128 * 128
    flat = np.full_like(win, 90)
    stripes = np.broadcast_to(np.array([10, 200, 60, 140], np.uint8)[np.arange(win.shape[2]) % 4][None, None, :, None], win.shape).copy()
    for clip in (win, flat, stripes):
        for block, search, lam in ((8, 4, 0), (16, 2, 32)):
            want = R.search(clip, offs, None, 2, block, search, lam)
            walk = R.candidates(search)
            for order in (walk[::-1], [walk[i] for i in rng.permutation(len(walk))]):
                got = R.search(clip, offs, None, 2, block, search, lam, walk=order)
                assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    mv, _ = R.search(flat, np.zeros_like(offs), None, 2, 8, 4, 0)
    assert not mv[..., :2].any() and not mv[..., 3].any() and mv[2, [0, 1, 3, 4]][..., 2].all()     # every candidate costs the same: the zero vector


# ---- recovery -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_two_planes_are_recovered_exactly(seed):
    """A noise-free two-plane clip, lam = 0: every block that lies inside one plane, with its displaced copy inside that plane's rows and the
    window's columns, gets exactly the plane's displacement, for every displacement up to `search`."""
    clip, pan = R.two_plane_clip(seed, noise=False)
    block, search, radius = 8, 4, 2
    mv, stats = R.search(clip, np.zeros((R.T, 2), np.int32), None, radius, block, search, 0)
    checked, largest = 0, 0
    for t in range(R.T):
        for k in range(2 * radius + 1):
            s = t - radius + k
            if s == t or not 0 <= s < R.T:
                continue
            for j, (r0, r1) in enumerate(((0, R.SPLIT), (R.SPLIT, R.H))):
                dx, dy = (int(v) for v in pan[j, t] - pan[j, s])                                     # frame t's pixel p shows in frame s at p + pan[t] - pan[s]
                if max(abs(dx), abs(dy)) > search:
                    continue
                for by in range(r0 // block, r1 // block):
                    for bx in range(R.W // block):
                        y0, x0 = by * block, bx * block
                        if r0 <= y0 + dy and y0 + block + dy <= r1 and 0 <= x0 + dx and x0 + block + dx <= R.W:
                            assert tuple(mv[t, k, by, bx]) == (dy, dx, 1, 0), (t, s, by, bx)
                            checked, largest = checked + 1, max(largest, abs(dx), abs(dy))
    assert checked > 2000 and largest == search


# ---- the rule on the two-plane flicker clip: a failure here means the rule is wrong, not the kernel ------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rule_removes_flicker_on_two_planes(seed):
    """block 8, search 4, lam 32, radius 2, tol 16 on the two-plane flicker clip, the full frame as the window.  Measured: DESIGN.md section 26."""
    x, pan = R.two_plane_clip(seed)
    assert x.shape == (R.T, R.H, R.W, 3) and x.dtype == np.uint8 and x.min() >= 33 and x.max() <= 223
    assert (np.diff(pan[0, :, 0]) >= 1).all() and (np.diff(pan[0, :, 0]) <= 3).all() and (np.abs(np.diff(pan[0, :, 1])) <= 1).all()
    assert (np.diff(pan[1, :, 0]) <= -1).all() and (np.diff(pan[1, :, 0]) >= -3).all() and not pan[1, :, 1].any()
    zero, mask = np.zeros((R.T, 2), np.int32), np.zeros((R.T, R.H, R.W), np.uint8)
    mv, stats = R.search(x, zero, None, 2, 8, 4, 32)
    out, sums = R.hold(x, zero, None, mv, mask, 2, 8, 16)
    fixed, fsums = R0.hold(x, zero, mask, 2, 16)
    before, after = R.difference_along_planes(x, pan), R.difference_along_planes(out, pan)
    n, n_fixed = R.samples_per_pixel(sums), R.samples_per_pixel(fsums)
    print(f"seed {seed}: mean |frame difference| along the planes' motion {before:.2f} -> {after:.2f}, a factor of {before / after:.2f}; accepted samples "
          f"per pixel {n:.2f} block-matched, {n_fixed:.3f} at a fixed place; {int(stats[:, :, 1].sum())} of {int(stats[:, :, 0].sum())} vectors non-zero")
    assert before / after >= 3.0
    assert n >= 3.0
    assert n_fixed <= 1.1
    assert np.abs(out.astype(int) - x).max() <= 16


# ---- the report ---------------------------------------------------------------------------------------------------------------------------
def test_fit_and_report_over_spans():
    from videovanish_amd import infill
    stats = np.zeros((3, 5, 6), np.int64)
    stats[0, 1] = (10, 4, 12, 3, 500, 900)
    stats[0, 3] = (10, 0, 0, 0, 200, 200)
    stats[2, 0] = (5, 5, 20, 4, 50, 0)
    f = DL.fit(stats)
    assert DL.DeflickerLocalFit._fields == ("blocks", "moved", "mean_vector", "max_vector", "cost", "cost_zero")
    assert f.blocks.tolist() == [20, 0, 5] and f.moved.tolist() == [4, 0, 5] and f.mean_vector.tolist() == [0.6, 0.0, 4.0] and f.max_vector.tolist() == [3, 0, 4]
    assert f.cost.tolist() == [700, 0, 50] and f.cost_zero.tolist() == [1100, 0, 0] and f.blocks.dtype == np.int64 and f.max_vector.dtype == np.int64
    part = infill.DeflickerLocalReport(*(np.stack([v, v]) for v in f))
    rep = infill.deflicker_local_report([part], [(2, 5)], 7)
    assert infill.DeflickerLocalReport._fields == DL.DeflickerLocalFit._fields and rep.blocks.shape == (2, 7) and rep.mean_vector.dtype == np.float64
    assert rep.blocks[1].tolist() == [0, 0, 20, 0, 5, 0, 0] and rep.max_vector[0].tolist() == [0, 0, 3, 0, 4, 0, 0] and rep.cost_zero[0, 2] == 1100
    empty = infill.deflicker_local_report([], [], 4, K=3)
    assert empty.blocks.shape == (3, 4) and not any(v.any() for v in empty)


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_precedence_and_the_two_value_errors(monkeypatch):
    import inspect

    import diffuerase
    for name in ("VV_DEFLICKER", "VV_DEFLICKER_ALIGN", "VV_DEFLICKER_LOCAL"):
        monkeypatch.delenv(name, raising=False)
    try:
        diffuerase.configure()
        assert diffuerase.deflicker_local_config() is None
        monkeypatch.setenv("VV_DEFLICKER_LOCAL", "search=1")
        assert diffuerase.deflicker_local_config() == DeflickerLocalConfig(search=1)
        diffuerase.configure(deflicker_local="block=16")
        assert diffuerase.deflicker_local_config() == DeflickerLocalConfig(block=16) and diffuerase.deflicker_local_config("on") == DeflickerLocalConfig()
        assert diffuerase.deflicker_local_config("off") is None and diffuerase.deflicker_local_config(False) is None
        diffuerase.configure(deflicker_local="off")
        assert diffuerase.deflicker_local_config() is None                                         # configure("off") beats the environment
        diffuerase.configure()
        assert diffuerase.deflicker_local_config() == DeflickerLocalConfig(search=1)
        with pytest.raises(ValueError, match="deflicker_local must be"):
            diffuerase.configure(deflicker_local="sometimes")
        f = [np.zeros((8, 8, 3), np.uint8)] * 2
        need = r"deflicker_local= \(block-matched inpaint deflicker\) needs deflicker= \(inpaint deflicker\)"
        for kw in (dict(deflicker_local="on"), dict(), dict(deflicker_local="on", deflicker="off")):    # the second: from the environment
            with pytest.raises(ValueError, match=need):
                diffuerase.run_infill_on_frames(f, f, **kw)
        monkeypatch.setenv("VV_DEFLICKER", "on")
        with pytest.raises(ValueError, match=need):
            diffuerase.run_infill_on_frames(f, f, deflicker=False)                                  # "off" wins over the environment
        with pytest.raises(ValueError, match="cannot be combined with compat_reference_early_return=True"):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)               # past that check: deflicker comes from the environment
        monkeypatch.delenv("VV_DEFLICKER_LOCAL")
        with pytest.raises(ValueError, match="cannot be combined with compat_reference_early_return=True"):
            diffuerase.run_infill_on_frames(f, f, deflicker_local="on", compat_reference_early_return=True)
        monkeypatch.setattr(diffuerase, "ALL_OPTIONS", tuple(o for o in diffuerase.ALL_OPTIONS if o.name == "deflicker_local"))
        with pytest.raises(ValueError, match=r"deflicker_local= \(block-matched inpaint deflicker\) cannot be combined with compat_reference_early_return=True"):
            diffuerase.run_infill_on_frames(f, f, deflicker_local="on", compat_reference_early_return=True)     # its own row of the check
        monkeypatch.undo()
        for name in ("VV_DEFLICKER", "VV_DEFLICKER_ALIGN", "VV_DEFLICKER_LOCAL"):
            monkeypatch.delenv(name, raising=False)
        monkeypatch.setenv("VV_DEFLICKER", "on")
        with pytest.raises(ValueError, match="0 <= search <= 8"):
            diffuerase.run_infill_on_frames(f, f, deflicker_local="search=9")
        diffuerase.last_deflicker_local = "stale"
        with pytest.raises(ValueError):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)
        assert diffuerase.last_deflicker_local is None                                              # reset at the start of every call
    finally:
        diffuerase.configure()
    assert [o.name for o in diffuerase.ALL_OPTIONS].count("deflicker_local") == 1 and diffuerase._OPTION["deflicker_local"].env == "VV_DEFLICKER_LOCAL"
    for fn in (diffuerase.run_infill_on_frames, diffuerase.configure):
        names = list(inspect.signature(fn).parameters)
        p = inspect.signature(fn).parameters["deflicker_local"]
        assert names[names.index("deflicker_align") + 1] == "deflicker_local" and names[-1] == "plate_fill"
        assert p.default is None and (fn is diffuerase.configure or p.kind is inspect.Parameter.KEYWORD_ONLY)


def test_cli_deflicker_local_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
    import diffuerase
    from videovanish_amd import infill
    calls = []
    videos = {"mask.mkv": [np.zeros((16, 24, 3), np.uint8)] * 7}
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda path, start=0, max_frames=-1: ([f.copy() for f in videos[path]], 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    stats = np.zeros((7, 5, 6), np.int64)
    stats[1:6, 1] = (40, 10, 25, 3, 1000, 2000)
    local = infill.deflicker_local_report([infill.DeflickerLocalReport(*(v[None] for v in DL.fit(stats)))], [(0, 7)], 7)
    sums = np.zeros((7, 12), np.int64)
    sums[:, [0, 2, 6, 8]] = (384, 384 * 3, 100, 250)
    from videovanish_amd import deflicker
    flick = infill.deflicker_report([infill.DeflickerReport(*(v[None] for v in deflicker.fit(sums)))], [(0, 7)], 7)

    def fake(frames, masks, **kw):
        calls.append(kw)
        diffuerase.last_deflicker = flick if "deflicker" in kw else None
        diffuerase.last_deflicker_local = local if "deflicker_local" in kw else None
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 7
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    for value in ("on", "block=16,search=8,lam=0"):
        monkeypatch.setattr(sys, "argv", argv + ["--deflicker", "on", "--deflicker-local", value])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "deflicker": "on", "deflicker_local": value}
        lines = capsys.readouterr().out.splitlines()
        assert len(lines) == 2 and lines[0].startswith("deflicker: ")
        assert lines[1] == "deflicker local: 200 blocks matched, 25.0 % of them moved, largest |vector| 3 px, mean accepted samples inside the mask 2.50"
    monkeypatch.setattr(sys, "argv", argv + ["--deflicker", "on"])
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None, "deflicker": "on"} and "deflicker local" not in capsys.readouterr().out
    for bad in ("off", "yes", "search=9", "block=12", "radius=2"):
        monkeypatch.setattr(sys, "argv", argv + ["--deflicker-local", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_deflicker_local", None)
    monkeypatch.setattr(diffuerase, "last_deflicker", None)
