"""Clean-plate grain on the CPU: the settings, the binding of include/vvplategrain.h, the rule's restatement (tests/plategrain_ref.py) against a
second, per-pixel restatement and the rule's consequences, the statistic the option exists for, the orchestration with the device functions
replaced by the restatement, configuration and CLI."""
import ctypes
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
import platefill_ref as R  # noqa: E402
import plategrain_ref as G  # noqa: E402

from videovanish_amd import plategrain as PG  # noqa: E402
from videovanish_amd.platefill import PlateFillConfig  # noqa: E402
from videovanish_amd.plategrain import PlateGrainConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = G.NONE


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_spellings_and_config():
    assert PG.SPELLINGS == ("on",)
    for off in (None, False, "off", "none", "", " OFF "):
        assert PG.as_config(off) is None
    d = PlateGrainConfig()
    assert PG.as_config("on") == PG.as_config(" On ") == PG.as_config(True) == d and (d.depth, d.reach) == (4, 8) == tuple(G.DEFAULTS.values())
    assert PG.as_config("depth=4,reach=8") == d and PG.as_config(" reach = 3 ") == PlateGrainConfig(reach=3)
    assert PG.as_config("depth=1") == PlateGrainConfig(depth=1) and PG.as_config("reach=65535,depth=8") == PlateGrainConfig(8, 65535)
    cfg = PlateGrainConfig(depth=2)
    assert PG.as_config(cfg) is cfg
    for bad in ("yes", "depth", "depth=", "depth=x", "depth=-1", "depth=1.5", "depth=2,depth=3", "size=3", "depth=2;reach=1", "depth=0", "depth=9",
                "reach=0", "reach=65536", "on,depth=2", "depth=2,", 3, 1.0, ("on",)):
        with pytest.raises(ValueError):
            PG.as_config(bad)
    for kw in (dict(depth=0), dict(depth=9), dict(reach=0), dict(reach=65536), dict(depth=2.0), dict(depth=True), dict(reach="8")):
        with pytest.raises(ValueError):
            PlateGrainConfig(**kw)


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_vvplategrain_header():
    """plategrain_hip.SIGNATURES declares every function of include/vvplategrain.h with the header's types and in its order, plategrain_hip.lib()
    has applied it, the version and the limits agree (abiref.check_binding; test_abi_cpu.py: the vvl_ prefix belongs to no other part)."""
    from videovanish_amd import plate_hip, plategrain_hip
    loaded, define = abiref.check_binding(plategrain_hip, 3)
    assert plategrain_hip.EXPORTS == ["vvl_abi_version", "vvl_last_error", "vvl_sources"] and define("VVL_ABI_VERSION") == 1
    # vvp_sources' arguments, then depth and reach, and one more output plane
    assert list(loaded.vvl_sources.argtypes) == list(plate_hip.lib().vvp_sources.argtypes[:14]) + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 4
    assert (define("VVL_MAX_DEPTH"), define("VVL_MAX_REACH")) == (plategrain_hip.MAX_DEPTH, plategrain_hip.MAX_REACH) == (PG.MAX_DEPTH, PG.MAX_REACH) == (8, 65535)


def test_vvplate_header_is_as_it_was():
    from videovanish_amd import plate_hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vvplate.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(vvp_[a-z0-9_]+)\s*\(", src))) == sorted(plate_hip.SIGNATURES) and len(plate_hip.SIGNATURES) == 5
    assert "vvl_" not in src and not any(n.startswith("vvl_") for n in plate_hip.SIGNATURES)


def test_refusals_through_the_library():
    """Every refusal of vvl_sources: vvp_sources' own, then depth, reach and a null live; each names vvl_sources.  Nothing can be launched here:
    every pointer is host memory and every call is refused before the first device call."""
    from videovanish_amd import plategrain_hip
    abiref.built()
    loaded = plategrain_hip.lib()
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    so = lambda *v, live=a: loaded.vvl_sources(a, a, a, None, a, a, a, *v, a, live, a, None)       # T, H, W, tile, tol, outlier, max_gap, depth, reach
    ok = (2, 8, 8, 64, 6, 3, 0, 4, 8)

    def but(**kw):
        names = ("T", "H", "W", "tile", "tol", "outlier", "max_gap", "depth", "reach")
        return [kw.get(k, v) for k, v in zip(names, ok)]
    for bad in (dict(T=0), dict(H=0), dict(H=1 << 16, W=1 << 15), dict(tol=-1), dict(outlier=-1), dict(max_gap=-1), dict(depth=0), dict(depth=-3),
                dict(reach=0), dict(reach=-1)):
        assert so(*but(**bad)) == -1 and loaded.vvl_last_error().startswith(b"vvl_sources:"), bad
    assert so(*ok, live=None) == -1 and b"live" in loaded.vvl_last_error()
    assert loaded.vvl_sources(None, a, a, None, a, a, a, *ok, a, a, a, None) == -1 and loaded.vvl_sources(a, a, a, None, a, a, a, *ok, None, a, a, None) == -1
    assert loaded.vvl_sources(a, a, a, a, a, a, a, *but(tile=0), a, a, a, None) == -1                  # a tile grid needs a tile
    for bad in (dict(T=65536), dict(tol=256), dict(outlier=65), dict(max_gap=65536), dict(depth=9), dict(reach=65536)):
        assert so(*but(**bad)) == -2 and loaded.vvl_last_error().startswith(b"vvl_sources:"), bad
    assert b"depth 9" in (so(*but(depth=9)), loaded.vvl_last_error())[1]
    with pytest.raises(ctypes.ArgumentError):
        so(*but(depth=2.0))
    import torch
    f, z = torch.zeros((2, 4, 4, 3), dtype=torch.uint8), torch.zeros((2, 4, 4), dtype=torch.uint8)
    with pytest.raises(RuntimeError):                                                                # no CPU fallback
        plategrain_hip.sources(f, z, z, None, z[0], z[0].int(), f[0].int(), 6, 3, 0, 4, 8)


def test_product_sources_of_the_feature():
    """The kernel lives in vv_plate.hip with the new header among the recipe's dependencies and reads no environment; the settings import no
    torch; importing the drop-in resolves no vvl_ symbol."""
    kernel, txt = abiref.check_sources("vv_plate", "vvplategrain.h", "plategrain")
    assert "include/vvplate.h" in open(os.path.join(abiref.CSRC, "build.sh")).read() and 'extern "C" int vvl_sources(' in kernel
    assert kernel.count("void sources_kernel(") == 1                                                 # one body for vvp_sources and vvl_sources
    assert "numpy" not in txt
    code = ("import diffuerase; from videovanish_amd import plategrain_hip, plate_hip, hip; "
            "assert plategrain_hip.PART.dll is None and plate_hip.PART.dll is None and hip.CORE.dll is None; "
            "assert diffuerase.plate_grain_config() is None and diffuerase.last_plate_grain is None")
    env = {k: v for k, v in os.environ.items() if k not in ("VV_PLATE_GRAIN", "VV_PLATE_FILL")}
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------
def _live_by_lists(dil, us, depth, reach, max_gap):
    """The header once more, one pixel and one masked frame at a time with Python lists: -> (src, live) uint16."""
    T, H, W = dil.shape
    src, live = np.full((T, H, W), NONE, np.uint16), np.full((T, H, W), NONE, np.uint16)
    for y in range(H):
        for x in range(W):
            usable = [s for s in range(T) if us[s, y, x]]
            for t in range(T):
                if not dil[t, y, x] or not usable:
                    continue
                near = min(usable, key=lambda s: (abs(s - t), s))                                    # rule 5: the nearest, the earlier at a tie
                if max_gap > 0 and abs(near - t) > max_gap:
                    continue
                side = [s for s in usable if s < t][::-1] if near < t else [s for s in usable if s > t]
                kept = []
                for c in side[:depth]:
                    if abs(c - side[0]) > reach or (max_gap > 0 and abs(c - t) > max_gap):
                        break
                    kept.append(c)
                src[t, y, x], live[t, y, x] = side[0], kept[t % len(kept)]
    return src, live


def _consequences(det, dil, depth, reach, max_gap):
    """(b) src as rule 5 has it is checked by the caller; here (c) and (d) of the rule on a restatement's detail."""
    T = len(dil)
    t = np.arange(T).reshape(T, 1, 1)
    src, live, us, m, side = det["src"].astype(np.int64), det["live"].astype(np.int64), det["usable"], det["m"], det["side"]
    has = det["src"] != NONE
    assert ((det["live"] != NONE) == has).all() and (has <= (dil != 0)).all() and ((m >= 1) == has).all() and m.max() <= depth
    tt, yy, xx = np.nonzero(has)
    lv, sv = live[tt, yy, xx], src[tt, yy, xx]
    assert us[lv, yy, xx].all() and (dil[lv, yy, xx] == 0).all()                                      # (c) a usable sample frame, (e) unmasked
    assert (np.sign(lv - tt) == np.sign(sv - tt)).all() and (np.abs(lv - tt) >= np.abs(sv - tt)).all()   # on the side of src, not nearer
    assert (np.abs(lv - sv) <= reach).all() and (max_gap == 0 or (np.abs(lv - tt) <= max_gap).all())
    pair = has[1:] & has[:-1] & (side[1:] == side[:-1]) & (m[1:] >= 2) & (m[:-1] >= 2)
    if max_gap > 0:
        pair &= m[1:] == m[:-1]                                                                    # max_gap counts from t: only then can m differ
    else:
        assert (m[1:] == m[:-1])[has[1:] & has[:-1] & (side[1:] == side[:-1])].all()
    assert not (live[1:] == live[:-1])[pair].any()                                                  # (d)
    return int(pair.sum())


@pytest.mark.parametrize("a", [0, 3, 6])
def test_rule_on_the_locked_off_clip(a):
    frames, masks, clean, boxm, logom = R.locked_off_clip(a=a)
    base = R.fill_segment(frames, masks, detail=True)
    assert base[3]["src"][masks != 0].min() < NONE
    for depth, reach, more in ((1, 8, {}), (2, 8, {}), (4, 8, {}), (8, 65535, {}), (4, 2, {}), (4, 8, dict(guard=0, margin=0, max_gap=3)), (8, 1, dict(max_gap=5))):
        cfg = dict(R.DEFAULTS, **more)
        if more:
            base = R.fill_segment(frames, masks, detail=True, **cfg)
        out, dil2, counts, det = G.fill_segment(frames, masks, depth, reach, **cfg)
        assert (det["src"] == base[3]["src"]).all() and (det["r0"] == base[3]["r0"]).all() and (dil2 == base[1]).all() and (counts == base[2]).all()   # (b)
        assert (det["nearest"] == base[0]).all() and (out[masks == 0] == frames[masks == 0]).all()
        pairs = _consequences(det, masks, depth, reach, cfg["max_gap"])
        if depth == 1:
            assert (det["live"] == det["src"]).all() and (out == base[0]).all()                    # (a)
        elif not more:
            assert pairs > 1000 and (det["live"] != det["src"]).sum() > 1000
        if a == 0:
            assert (out == base[0]).all()                                                          # without noise every usable frame holds the same bytes
        else:
            assert np.abs(out[det["go"]].astype(np.int64) - clean[det["go"]]).max() <= a             # still bytes of the clip at that place
    src, live = _live_by_lists(masks, det["usable"], 8, 1, 5)                                        # the last settings of the loop
    assert (src == det["src"]).all() and (live == det["live"]).all()
    _, _, _, det = G.fill_segment(frames, masks)
    src, live = _live_by_lists(masks, det["usable"], 4, 8, 0)
    assert (src == det["src"]).all() and (live == det["live"]).all()


def test_rule_on_the_hand_made_pixel_table():
    frames, masks, us = G.table_clip()
    col = {name: x for x, name in enumerate(G.TABLE)}
    lv = lambda det, name: [int(v) if v != NONE else None for v in det["live"][:, 0, col[name]]]
    seen = {}
    for depth, reach, max_gap in ((4, 8, 0), (1, 8, 0), (4, 3, 0), (4, 8, 4), (8, 65535, 0), (2, 1, 2), (8, 65535, 7)):
        cfg = dict(G.TABLE_CFG, max_gap=max_gap)
        base = R.fill_segment(frames, masks, detail=True, **cfg)
        out, dil2, counts, det = G.fill_segment(frames, masks, depth, reach, **cfg)
        assert (det["usable"] == us).all()                                                          # the table means what its comments say
        assert (det["src"] == base[3]["src"]).all() and (dil2 == base[1]).all() and (counts == base[2]).all()
        src, live = _live_by_lists(masks, us, depth, reach, max_gap)
        assert (src == det["src"]).all() and (live == det["live"]).all()
        _consequences(det, masks, depth, reach, max_gap)
        assert (out == base[0]).all()                                                              # a pixel's usable frames hold the same bytes here
        assert (det["live"] == det["src"]).all() == (depth == 1)
        seen[depth, reach, max_gap] = det
    M = [None]
    d = seen[4, 8, 0]
    assert lv(d, "one candidate before") == M + [0] * 19 and (d["m"][1:, 0, col["one candidate before"]] == 1).all()
    assert lv(d, "cut by reach")[6:10] == [1, 0, 5, 4] and lv(seen[4, 3, 0], "cut by reach")[6:10] == [5, 4, 5, 4]
    assert lv(d, "cut by reach")[2:4] == [1, 5]                                                      # frame 2: before (1, 0), k = 2 % 2; frame 3: after (4, 5), k = 3 % 2
    assert lv(seen[4, 8, 4], "cut by max_gap")[6:12] == [3, 4, 5, 5, None, None]                     # m = 4, 3, 2, 1 (k = 2, 1, 0, 0), then no source
    assert lv(d, "outlier between")[6:10] == [1, 0, 4, 13]                                           # before 4, 3, 1, 0: k = 2, 3, 0 (frame 8: a tie, before); after 12, 13, ..: k = 1
    assert lv(seen[8, 65535, 0], "outlier between")[8:10] == [4, 15] and (seen[8, 65535, 0]["m"][6:10, 0, col["outlier between"]] == [4, 4, 4, 7]).all()
    assert lv(d, "run at the start")[:5] == [5, 6, 7, 8, 5] and lv(d, "run at the end")[15:] == [11, 14, 13, 12, 11]
    assert lv(d, "tie between the sides")[7:12] == [3, 6, 5, 14, 15] and d["src"][9, 0, col["tie between the sides"]] == 6
    assert lv(d, "never masked") == M * 20 and lv(d, "no usable frame") == M * 20
    assert (seen[8, 65535, 0]["m"][9:11, 0, col["more than eight a side"]] == [8, 8]).all()         # nine usable frames a side, eight kept
    assert lv(seen[8, 65535, 0], "more than eight a side")[9:11] == [7, 13]                          # 9 % 8 = 1 -> 7; 10 % 8 = 2 -> 11, 12, 13


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("a", [3, 6])
def test_grain_inside_the_fill_moves_as_it_does_outside(a, seed):
    """The statistic the option exists for, on the restatement (values of this test: DESIGN.md section 20): the frame-to-frame motion of the
    filled pixels over that of the never-masked pixels."""
    frames, masks, clean, boxm, logom = R.locked_off_clip(a=a, seed=seed)
    out, dil2, counts, det = G.fill_segment(frames, masks)
    go = det["go"]
    nearest, n_all = G.grain_ratio(det["nearest"], frames, masks, go)
    rotated, n_rot = G.grain_ratio(out, frames, masks, go)
    same, n_same = G.grain_ratio(out, frames, masks, go, G.same_side_pairs(det))
    print(f"a={a} seed={seed}: nearest {nearest:.4f}, rotated {rotated:.4f}, same side {same:.4f} over {n_same} of {n_all} pairs ({100 * n_same / n_all:.1f} %)")
    assert n_all == n_rot > 4000 and n_same >= 0.85 * n_all
    assert nearest <= 0.15
    assert rotated >= 0.9
    assert 0.95 <= same <= 1.05


def test_drift_stays_within_reach():
    """A quarter level per frame: a rotated source lies at most `reach` frames from the nearest, so its byte differs from the nearest rule's by
    the noise twice, the drift between the two (floored per frame, hence the 1) once."""
    a, reach = 3, 8
    frames, masks, clean, boxm, logom = R.locked_off_clip(a=a, drift_q4=1)
    out, dil2, counts, det = G.fill_segment(frames, masks, 4, reach)
    go = det["go"]
    assert go.sum() > 0.7 * boxm.sum() and (det["live"] != det["src"])[go].sum() > 1000
    diff = np.abs(out[go].astype(np.int64) - det["nearest"][go])
    print("drift clip: largest |rotated - nearest| =", int(diff.max()))
    assert diff.max() <= 2 * a + -(-reach // 4) + 1


def test_nothing_is_filled_over_a_panning_texture():
    frames, masks, boxm, logom = R.panning_clip()
    out, dil2, counts, rotated = G.plate_fill(frames, masks)
    assert (out == frames).all() and (dil2 == masks).all() and not counts[:, 0].any() and not rotated.any()


# ---- orchestration ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def host_kernels(monkeypatch):
    """infill.plate_fill with every device call replaced by the restatements on host tensors; the calls made are recorded."""
    import torch
    from videovanish_amd import hip, infill, mask_hip, plate_hip, plategrain_hip
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
        n, S1, S2 = R.stats(f.numpy(), ns.numpy() != 0)
        return t(R.steady(n, S1, S2, min_samples, tol).astype(np.uint8)), t(n.astype(np.int32)), t(S1.astype(np.int32))

    def _sources(f, d, ns, st, n, s1, tol, outlier, max_gap):
        us = R.usable(f.numpy(), ns.numpy() != 0, st.numpy() != 0, n.numpy().astype(np.int64), s1.numpy().astype(np.int64), tol, outlier)
        src = R.sources(d.numpy(), us, max_gap)
        return us, src, t(((d.numpy() != 0) & (src == NONE)).astype(np.uint8) * 255)

    def sources(f, d, ns, occ, st, n, s1, tol, outlier, max_gap):
        calls.append(("vvp_sources", max_gap))
        us, src, r0 = _sources(f, d, ns, st, n, s1, tol, outlier, max_gap)
        return t(src.view(np.int16)), r0

    def live_sources(f, d, ns, occ, st, n, s1, tol, outlier, max_gap, depth, reach):
        calls.append(("vvl_sources", max_gap, depth, reach))
        us, src, r0 = _sources(f, d, ns, st, n, s1, tol, outlier, max_gap)
        live = G.live_sources(src, us, depth, reach, max_gap)[0]
        return t(src.view(np.int16)), t(live.view(np.int16)), r0

    def fill(f, d, keep, occ, src):
        calls.append(("fill",))
        dn, s = d.numpy() != 0, src.numpy().view(np.uint16)
        left = dn & (keep.numpy() != 0)
        go = dn & ~left
        tt, yy, xx = np.nonzero(go)
        f.numpy()[tt, yy, xx] = f.numpy()[s[tt, yy, xx].astype(np.int64), yy, xx]
        T = len(dn)
        return t(left.astype(np.uint8) * 255), t(np.stack([go.reshape(T, -1).sum(1), left.reshape(T, -1).sum(1)], 1).astype(np.int64))

    monkeypatch.setattr(hip, "mask_bbox", mask_bbox)
    monkeypatch.setattr(hip, "mask_tile_union", lambda m, tile: t(np.ones((1, 1), np.uint8)))
    monkeypatch.setattr(hip, "mask_collapse_dilate", lambda m, iters: t(R.dilate(m.numpy()[..., 0] != 0, iters).astype(np.uint8) * 255))
    monkeypatch.setattr(mask_hip, "time_bridge_grow", lambda m, bridge, grow: (t(R.not_sample(m.numpy(), grow).astype(np.uint8) * 255), None))
    monkeypatch.setattr(plate_hip, "stats", stats)
    monkeypatch.setattr(plate_hip, "sources", sources)
    monkeypatch.setattr(plate_hip, "fill", fill)
    monkeypatch.setattr(plategrain_hip, "sources", live_sources)
    return infill, calls, t


def test_plate_fill_with_grain_segments_report_and_depth_one(host_kernels):
    infill, calls, t = host_kernels
    frames, masks, clean, boxm, logom = R.locked_off_clip()
    T = len(frames)
    flist = [f.copy() for f in frames]
    d = t(masks)
    for cuts in (None, [9, 15], [11]):
        for gcfg, pkw in ((PlateGrainConfig(), {}), (PlateGrainConfig(depth=2, reach=3), dict(guard=0, margin=0, max_gap=3))):
            del calls[:]
            got = []
            out, dil, rep = infill.plate_fill(flist, d, PlateFillConfig(**pkw), cuts, gcfg=gcfg, grain_out=got)
            want, wd, wc, wrot = G.plate_fill(frames, masks, cuts, gcfg.depth, gcfg.reach, **dict(R.DEFAULTS, **pkw))
            base, bd, brep = infill.plate_fill(flist, d, PlateFillConfig(**pkw), cuts)
            assert (np.stack(out) == want).all() and (dil.numpy() == wd).all() and (dil.numpy() == bd.numpy()).all()
            assert all((a == b).all() if isinstance(a, np.ndarray) else a == b for a, b in zip(rep, brep)) and len(rep) == 6      # the PlateFillReport as without it
            assert all((out[i] is flist[i]) == (wc[i, 0] == 0) for i in range(T)) and all((a == b).all() for a, b in zip(flist, frames))
            grep, = got
            assert isinstance(grep, infill.PlateGrainReport) and grep._fields == ("rotated", "filled", "segments")
            assert grep.rotated.dtype == np.int64 and (grep.rotated == wrot).all() and (grep.filled == wc[:, 0]).all() and grep.segments == rep.segments
            assert 0 < grep.rotated.sum() < grep.filled.sum() and not (np.stack(out) == np.stack(base)).all()
            segs = len(rep.segments)
            assert [c for c in calls if c[0] != "fill"][:segs] == [("vvl_sources", pkw.get("max_gap", 0), gcfg.depth, gcfg.reach)] * segs
    # depth = 1: the old call, its bytes, nothing rotated
    del calls[:]
    got = []
    out, dil, rep = infill.plate_fill(flist, d, PlateFillConfig(), None, gcfg=PlateGrainConfig(depth=1), grain_out=got)
    base, bd, brep = infill.plate_fill(flist, d, PlateFillConfig(), None)
    assert (np.stack(out) == np.stack(base)).all() and not got[0].rotated.any() and (got[0].filled == rep.filled).all()
    assert [c[0] for c in calls if c[0] != "fill"] == ["vvp_sources", "vvp_sources"]
    # skipped, empty: as without the option
    got = []
    out, dil, rep = infill.plate_fill(flist, d, PlateFillConfig(max_bytes=100), None, gcfg=PlateGrainConfig(), grain_out=got)
    assert rep.skipped == (True,) and dil is d and all(a is b for a, b in zip(out, flist)) and not got[0].rotated.any() and not got[0].filled.any()
    z, got = t(np.zeros_like(masks)), []
    out, dil, rep = infill.plate_fill(flist, z, PlateFillConfig(), None, gcfg=PlateGrainConfig(), grain_out=got)
    assert dil is z and all(a is b for a, b in zip(out, flist)) and not got[0].filled.any()
    pf, pm, _, _ = R.panning_clip()
    plist, pd, got = list(pf), t(pm), []
    out, dil, rep = infill.plate_fill(plist, pd, PlateFillConfig(), None, gcfg=PlateGrainConfig(), grain_out=got)
    assert dil is pd and all(a is b for a, b in zip(out, plist)) and not got[0].filled.any()
    infill.plate_fill(flist, d, PlateFillConfig(), None, gcfg=PlateGrainConfig())                      # no list to report into: fine


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_precedence_argument_configure_environment_and_the_need_for_plate_fill(monkeypatch):
    import diffuerase
    for name in ("VV_PLATE_GRAIN", "VV_PLATE_FILL", "VV_PLATE_ALIGN"):
        monkeypatch.delenv(name, raising=False)
    row = diffuerase._OPTION["plate_grain"]
    assert row in diffuerase.ALL_OPTIONS and row.env == "VV_PLATE_GRAIN" and row.settings is PG
    assert [PG.as_config(x) for x in row.metavar.split("|")] == [PlateGrainConfig()] * 2
    try:
        diffuerase.configure()
        assert diffuerase.plate_grain_config() is None
        monkeypatch.setenv("VV_PLATE_GRAIN", "reach=5")
        assert diffuerase.plate_grain_config() == PlateGrainConfig(reach=5)
        diffuerase.configure(plate_grain="depth=2")
        assert diffuerase.plate_grain_config() == PlateGrainConfig(depth=2) and diffuerase.plate_grain_config("on") == PlateGrainConfig()
        assert diffuerase.plate_grain_config("off") is None and diffuerase.plate_grain_config(False) is None
        diffuerase.configure(plate_grain="off")
        assert diffuerase.plate_grain_config() is None                                                     # configure("off") beats the environment
        mine = PlateGrainConfig(depth=3)
        assert diffuerase.plate_grain_config(mine) is mine
        diffuerase.configure()
        assert diffuerase.plate_grain_config() == PlateGrainConfig(reach=5)                                # configure() resets
        with pytest.raises(ValueError):
            diffuerase.configure(plate_grain="sometimes")
        f = [np.zeros((8, 8, 3), np.uint8)] * 2
        need = r"plate_grain= \(clean-plate grain\) needs plate_fill= \(clean-plate fill\)"
        for kw in (dict(plate_grain="on"), dict(), dict(plate_grain="on", plate_fill="off")):              # the second: from the environment
            with pytest.raises(ValueError, match=need):
                diffuerase.run_infill_on_frames(f, f, **kw)
        monkeypatch.setenv("VV_PLATE_FILL", "on")
        with pytest.raises(ValueError, match=need):
            diffuerase.run_infill_on_frames(f, f, plate_fill=False)                                        # "off" wins over the environment
        with pytest.raises(ValueError, match="cannot be combined with compat_reference_early_return=True"):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)
        with pytest.raises(ValueError, match="1 <= depth <= 8"):
            diffuerase.run_infill_on_frames(f, f, plate_grain="depth=9")
        monkeypatch.delenv("VV_PLATE_FILL")
        monkeypatch.delenv("VV_PLATE_GRAIN")
        with pytest.raises(ValueError, match="cannot be combined with compat_reference_early_return=True"):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, plate_fill="on", plate_grain="on")
        diffuerase.last_plate_grain = "stale"
        with pytest.raises(ValueError):
            diffuerase.run_infill_on_frames(f, f, plate_grain="on")
        assert diffuerase.last_plate_grain is None                                                         # reset at the start of every call
        monkeypatch.setenv("VV_PLATE_GRAIN", "sometimes")
        with pytest.raises(ValueError):
            diffuerase.plate_grain_config()
    finally:
        diffuerase.configure()
    for fn in (diffuerase.run_infill_on_frames, diffuerase.configure):
        names = list(inspect.signature(fn).parameters)
        p = inspect.signature(fn).parameters["plate_grain"]
        assert names[-3:] == ["plate_grain", "plate_align", "plate_fill"]
        assert p.default is None and (fn is diffuerase.configure or p.kind is inspect.Parameter.KEYWORD_ONLY)


def test_cli_plate_grain_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
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
        diffuerase.last_plate_fill = None
        diffuerase.last_plate_grain = infill.PlateGrainReport(z + [60, 0, 15], z + [100, 0, 100], ((0, 3),)) if "plate_grain" in kw else None
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 3
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    monkeypatch.setattr(sys, "argv", argv)
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None} and capsys.readouterr().out == ""                      # a default call passes no keyword, prints nothing
    for value in ("on", "depth=2,reach=3"):
        monkeypatch.setattr(sys, "argv", argv + ["--plate-fill", "on", "--plate-grain", value])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "plate_fill": "on", "plate_grain": value}
        out = capsys.readouterr().out
        assert out == "plate grain: 200 px filled, 37.5 % of them from another frame than the nearest\n"
    for bad in ("off", "yes", "depth=x", "depth=9"):
        monkeypatch.setattr(sys, "argv", argv + ["--plate-grain", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_plate_grain", None)
