"""Shadow masking on the CPU: the settings, the binding of include/vvshadow.h, the restatement (tests/shadowmask_ref.py) on the shared clip,
the stage in front of the clean-plate fill, the orchestration with the device functions replaced by the restatement, configuration and CLI."""
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
import platefill_ref as P  # noqa: E402
import shadowmask_ref as R  # noqa: E402

from videovanish_amd import shadowmask as SM  # noqa: E402
from videovanish_amd import spans  # noqa: E402
from videovanish_amd.shadowmask import ShadowMaskConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("guard", "min_samples", "tol", "lo", "hi", "drop", "chroma", "floor", "reach", "min_area", "grow")


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_spellings_and_config():
    assert SM.SPELLINGS == ("on",)
    for off in (None, False, "off", "none", "", " OFF "):
        assert SM.as_config(off) is None
    d = ShadowMaskConfig()
    assert SM.as_config("on") == SM.as_config(" On ") == SM.as_config(True) == d
    assert tuple(getattr(d, k) for k in KEYS) == (1, 4, 6, 30, 90, 12, 20, 16, 32, 16, 1) == tuple(R.DEFAULTS[k] for k in KEYS)
    assert d.max_bytes == 1 << 30 and d.widen == 33
    assert SM.as_config("guard=1,min_samples=4,tol=6,lo=30,hi=90,drop=12,chroma=20,floor=16,reach=32,min_area=16,grow=1") == d
    assert SM.as_config(" tol = 9 , guard = 0 ") == ShadowMaskConfig(guard=0, tol=9)
    assert SM.as_config("max_bytes=1000").max_bytes == 1000 and SM.as_config("reach=64,grow=16").widen == 80
    assert SM.as_config("lo=50,hi=50") == ShadowMaskConfig(lo=50, hi=50) and SM.as_config("min_area=2147483647").min_area == 2 ** 31 - 1
    cfg = ShadowMaskConfig(grow=0)
    assert SM.as_config(cfg) is cfg
    for bad in ("yes", "static", "tol", "tol=", "tol=x", "tol=-3", "tol=1.5", "tol=3,tol=4", "size=3", "tol=3;guard=1", "guard=9", "tol=256", "lo=91",
                "hi=101", "hi=29", "drop=256", "chroma=101", "floor=0", "floor=256", "reach=65", "grow=17", "min_area=2147483648", "min_samples=0",
                "min_samples=65536", "on,tol=1", "tol=3,", 3, 1.0, ("on",)):
        with pytest.raises(ValueError):
            SM.as_config(bad)
    for kw in (dict(guard=-1), dict(guard=9), dict(tol=-1), dict(tol=256), dict(lo=-1), dict(lo=60, hi=50), dict(hi=101), dict(drop=-1), dict(drop=256),
               dict(chroma=-1), dict(chroma=101), dict(floor=0), dict(floor=256), dict(reach=-1), dict(reach=65), dict(min_area=-1), dict(grow=-1),
               dict(grow=17), dict(min_samples=0), dict(min_samples=65536), dict(max_bytes=-1), dict(tol=6.0), dict(guard=True), dict(reach="2")):
        with pytest.raises(ValueError):
            ShadowMaskConfig(**kw)


def test_widen_box():
    assert SM.widen_box((10, 40, 20, 60), 100, 200, 33) == (0, 4, 53, 96)                  # clamped above, x to multiples of 4
    assert SM.widen_box((10, 40, 20, 60), 100, 200, 0) == (10, 40, 20, 60)
    assert SM.widen_box((50, 100, 60, 120), 64, 126, 5) == (45, 92, 64, 126)               # x1 stops at the frame
    assert SM.widen_box((0, 0, 40, 56), 40, 56, 80) == (0, 0, 40, 56)


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_vvshadow_header():
    """shadow_hip.SIGNATURES declares every function of include/vvshadow.h with the header's types, shadow_hip.lib() has applied it, the version
    and the range constants agree (abiref.check_binding; test_abi_cpu.py: no name could be taken for another part's), and arguments are refused
    before anything touches a device."""
    from videovanish_amd import mask_hip, shadow_hip
    loaded, define = abiref.check_binding(shadow_hip, 6)
    assert define("VVH_ABI_VERSION") == 1
    limits = tuple(define("VVH_MAX_" + k) for k in ("T", "GUARD", "TOL", "DROP", "CHROMA", "FLOOR", "REACH", "GROW"))
    assert limits == (shadow_hip.MAX_T, shadow_hip.MAX_GUARD, shadow_hip.MAX_TOL, shadow_hip.MAX_DROP, shadow_hip.MAX_CHROMA, shadow_hip.MAX_FLOOR,
                      shadow_hip.MAX_REACH, shadow_hip.MAX_GROW) == (65535, 8, 255, 255, 100, 255, 64, 16)
    assert limits == (SM.MAX_T, SM.MAX_GUARD, SM.MAX_TOL, SM.MAX_DROP, SM.MAX_CHROMA, SM.MAX_FLOOR, SM.MAX_REACH, SM.MAX_GROW)
    assert shadow_hip.MAX_GUARD == mask_hip.MAX_GROW                                                # the guard is vvm_time_bridge_grow's grow
    assert (define("VVH_GROW_TILE"), define("VVH_GROW_K")) == (shadow_hip.GROW_TILE, shadow_hip.GROW_K) == (64, 8)
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    b, c, d = a + 8, a + 16, a + 24
    pl = lambda *v: loaded.vvh_plate(a, a, *v, a, a, a, None)                                        # T, H, W, min_samples, tol
    ca = lambda *v: loaded.vvh_candidates(a, a, a, a, a, 2, 8, 8, *v, a, a, None)                    # lo, hi, drop, chroma, floor
    gr = lambda *v: loaded.vvh_grow(a, b, *v, c, d, None)                                            # T, H, W, reach
    assert loaded.vvh_plate(None, a, 2, 8, 8, 4, 6, a, a, a, None) == -1 and b"vvh_plate" in loaded.vvh_last_error()
    assert [pl(0, 8, 8, 4, 6), pl(2, 0, 8, 4, 6), pl(2, 1 << 16, 1 << 15, 4, 6), pl(2, 8, 8, 0, 6), pl(2, 8, 8, 4, -1)] == [-1] * 5
    assert [pl(65536, 8, 8, 4, 6), pl(2, 8, 8, 65536, 6), pl(2, 8, 8, 4, 256)] == [-2] * 3 and b"vvh_plate" in loaded.vvh_last_error()
    assert [ca(-1, 90, 12, 20, 16), ca(60, 50, 12, 20, 16), ca(30, 90, -1, 20, 16), ca(30, 90, 12, -1, 16), ca(30, 90, 12, 20, 0)] == [-1] * 5
    assert b"vvh_candidates" in loaded.vvh_last_error()
    assert [ca(30, 101, 12, 20, 16), ca(30, 90, 256, 20, 16), ca(30, 90, 12, 101, 16), ca(30, 90, 12, 20, 256)] == [-2] * 4
    assert loaded.vvh_candidates(a, a, a, a, a, 65536, 8, 8, 30, 90, 12, 20, 16, a, a, None) == -2
    assert [gr(0, 8, 8, 4), gr(2, 8, 8, -1), loaded.vvh_grow(a, b, 2, 8, 8, 4, c, c, None), loaded.vvh_grow(a, b, 2, 8, 8, 4, a, d, None),
            loaded.vvh_grow(a, b, 2, 8, 8, 4, c, b, None), loaded.vvh_grow(a, None, 2, 8, 8, 4, c, d, None)] == [-1] * 6
    assert b"vvh_grow" in loaded.vvh_last_error()
    assert [gr(2, 8, 8, 65), gr(65536, 8, 8, 4)] == [-2] * 2
    assert loaded.vvh_merge(a, b, 0, 8, 8, c, d, None) == -1 and b"vvh_merge" in loaded.vvh_last_error()
    assert loaded.vvh_merge(a, b, 2, 8, 8, a, d, None) == -1                                         # dil_out is not dil
    assert loaded.vvh_merge(a, b, 65536, 8, 8, c, d, None) == -2
    with pytest.raises(ctypes.ArgumentError):
        loaded.vvh_plate(a, a, 2.0, 8, 8, 4, 6, a, a, a, None)
    import torch
    f, z = torch.zeros((2, 4, 4, 3), dtype=torch.uint8), torch.zeros((2, 4, 4), dtype=torch.uint8)
    for call in (lambda: shadow_hip.plate(f, z, 4, 6), lambda: shadow_hip.grow(z, z, 3), lambda: shadow_hip.merge(z, z, torch.zeros((2, 2), dtype=torch.int64))):
        with pytest.raises(RuntimeError):
            call()                                                                                   # no CPU fallback


def test_product_sources_of_the_feature():
    """vv_shadow is in the one build recipe with its header among the dependencies and reads no environment; the settings import neither torch nor
    numpy; importing the drop-in resolves no symbol of the feature, and neither does a call's set-up without the option."""
    _, txt = abiref.check_sources("vv_shadow", "vvshadow.h", "shadowmask")
    assert not re.search(r"^\s*(import|from)\s+(torch|numpy|oracle)\b", txt, flags=re.M)
    code = ("import sys, diffuerase; from videovanish_amd import shadow_hip, hip; assert shadow_hip.PART.dll is None and hip.CORE.dll is None; "
            "assert diffuerase.shadow_mask_config() is None and diffuerase.last_shadow_mask is None; "
            "import videovanish_amd.shadowmask")
    env = {k: v for k, v in os.environ.items() if k != "VV_SHADOW_MASK"}
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)
    alone = "import sys, videovanish_amd.shadowmask; assert 'torch' not in sys.modules and 'numpy' not in sys.modules"
    subprocess.check_call([sys.executable, "-c", alone], cwd=ROOT, env=env)


# ---- the rules on the shared clip: a failure here means the rule is wrong, not the kernel ---------------------------------------------------
@pytest.fixture(scope="module")
def shared():
    """shadowmask_ref.shadow_clip for seeds 0 .. 3 and strengths 50, 60, 75, 85 with the restatement's result, computed once."""
    out = {}
    for seed in range(4):
        for strength in (50, 60, 75, 85):
            frames, dil, band, clean, masks, logom = R.shadow_clip(seed, strength)
            out[seed, strength] = (frames, dil, band, clean, logom) + R.shadow_segment(frames, dil, detail=True)
    return out


def test_reference_recall_and_precision_on_the_shared_clip(shared):
    for (seed, strength), (frames, dil, band, clean, logom, d2, counts, det) in shared.items():
        true = band & (dil == 0)
        added = (d2 != 0) & (dil == 0)
        recall = (added & true).sum() / true.sum()
        stray = int((added & ~P.dilate(band, 2)).sum())
        print(f"seed {seed} strength {strength}: {true.sum()} shadow px outside dil, recall {recall:.4f}, {stray} added px outside the band + 2")
        assert true.sum() > 1000 and recall >= 0.95, (seed, strength, recall)
        assert stray <= 0.01 * band.sum(), (seed, strength, stray)
        assert ((d2 != 0) >= (dil != 0)).all() and set(np.unique(d2)) <= {0, 255}                     # masks only grow
        assert (counts[:, 1] == added.reshape(len(d2), -1).sum(1)).all() and (counts[:, 0] == det["cand"].reshape(len(d2), -1).sum(1)).all()


def test_reference_shadowless_clip_and_pan_add_nothing():
    for seed in range(4):
        frames, masks, clean, boxm, logom = P.locked_off_clip(T=24, H=40, W=56, a=6, seed=seed)
        dil = (P.dilate(masks != 0, 2) * 255).astype(np.uint8)
        d2, counts = R.shadow_segment(frames, dil)
        assert (d2 == dil).all() and not counts[:, 1].any(), seed
        pf, pm, _, _ = P.panning_clip(seed=seed)
        pd = (P.dilate(pm != 0, 2) * 255).astype(np.uint8)
        d2, counts, det = R.shadow_segment(pf, pd, detail=True)
        assert (d2 == pd).all() and not counts.any() and not det["ok"].any(), seed                   # no plate, no candidate


def test_reference_detached_and_coloured_patches():
    T, H, W = 24, 40, 56
    # a patch at 60 % in frames 10 .. 13 that touches no mask: candidates, none added
    patch = np.zeros((T, H, W), bool)
    patch[10:14, 28:34, 30:42] = True
    frames, dil, band, *_ = R.shadow_clip(0, 60, band=patch)
    assert (band == patch).all() and not (P.dilate(dil != 0, 1) & patch).any()
    d2, counts, det = R.shadow_segment(frames, dil, detail=True)
    assert (det["cand"] & patch).sum() == patch.sum() and (d2 == dil).all() and not counts[:, 1].any() and counts[10:14, 0].all()
    # the shared band, touching the mask, darkened by (40, 85, 85) %: a dark coloured object, no candidate
    frames, dil, band, *_ = R.shadow_clip(0, gain=(40, 85, 85))
    d2, counts, det = R.shadow_segment(frames, dil, detail=True)
    assert not (det["cand"] & band).any() and not ((d2 != 0) & band & (dil == 0)).any()
    # each single channel 40 points out of line is enough (the grain of +-6 levels moves a ratio by less than 10 points)
    for gain in ((45, 45, 85), (85, 45, 45), (45, 85, 45)):
        frames, dil, band, *_ = R.shadow_clip(0, gain=gain)
        assert not (R.shadow_segment(frames, dil, detail=True)[2]["cand"] & band).any(), gain


def test_reference_reach_limits_the_growth():
    T, H, W = 24, 40, 56
    frames, dil, band, *_ = R.shadow_clip(0, 60, band=R.band_mask(T, H, W, rows=3, width=30))
    added = [int(R.shadow_segment(frames, dil, **dict(R.DEFAULTS, min_area=1, grow=0, reach=r))[1][:, 1].sum()) for r in (0, 4, 7, 32)]
    print("added px over reach 0, 4, 7, 32:", added)
    assert added[0] == 0 and added[0] < added[1] < added[2] < added[3]


def test_reference_with_the_plate_fill():
    """The stage in front of the clean-plate fill, through both restatements: fewer masked pixels are left to the model, and away from the logo no
    filled or untouched pixel is further than 12 levels from the clean background (without the stage the shadow's pixels are)."""
    frames, dil, band, clean, masks, logom = R.shadow_clip(0, 60)
    d2, _ = R.shadow_segment(frames, dil)
    res = {}
    for name, d in (("without", dil), ("with", d2)):
        out, left, counts = P.fill_segment(frames, d)
        seen = (left == 0) & ~logom[None]                                   # filled or untouched, away from the logo
        res[name] = (int(counts[:, 1].sum()), int(((np.abs(out.astype(np.int64) - clean) > 12).any(-1) & seen).sum()))
    print("masked px left, px further than 12 levels from the clean background:", res)
    assert res["with"][0] < res["without"][0] and res["with"][1] == 0 and res["without"][1] > 1000
    assert res == {"without": (3942, res["without"][1]), "with": (2857, 0)}                          # the prototype's figures


# ---- orchestration ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def host_kernels(monkeypatch):
    """infill.shadow_mask with every device call replaced by the restatement on host tensors; the calls made are recorded."""
    import torch
    from videovanish_amd import hip, infill, mask_hip, shadow_hip
    calls = []
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))

    def mask_bbox(m):
        calls.append(("bbox", tuple(m.shape)))
        out = np.zeros((len(m), 4), np.int32)
        for i, f in enumerate(m.numpy()):
            ys, xs = np.nonzero(f.any(1))[0], np.nonzero(f.any(0))[0]
            if len(ys):
                out[i] = ys[0], xs[0], ys[-1] + 1, xs[-1] + 1
        return t(out)

    def time_bridge_grow(m, bridge, grow):
        calls.append(("guard", len(m), bridge, grow))
        return t(P.not_sample(m.numpy(), grow).astype(np.uint8) * 255), None

    def plate(f, ns, min_samples, tol):
        calls.append(("plate", tuple(f.shape), min_samples, tol))
        assert f.is_contiguous() and ns.is_contiguous()
        ok, n2, T1, _ = R.plate(f.numpy(), ns.numpy() != 0, min_samples, tol)
        return t(ok.astype(np.uint8)), t(n2.astype(np.int32)), t(T1.astype(np.int32))

    def candidates(f, d, ok, n2, t1, lo, hi, drop, chroma, floor):
        calls.append(("candidates", lo, hi, drop, chroma, floor))
        assert d.is_contiguous()
        c = R.candidates(f.numpy(), d.numpy(), ok.numpy() != 0, n2.numpy().astype(np.int64), t1.numpy().astype(np.int64), lo, hi, drop, chroma, floor)
        return t(c.astype(np.uint8)), t(np.stack([c.reshape(len(c), -1).sum(1), np.zeros(len(c), np.int64)], 1).astype(np.int64))

    def grow(a0, cand, reach):
        calls.append(("grow", reach))
        return t(R.geodesic(a0.numpy() != 0, cand.numpy() != 0, reach).astype(np.uint8) * 255)

    def despeckle(dil, raw, min_area):
        calls.append(("despeckle", min_area))
        assert dil is raw
        return t(R.drop_small(dil.numpy() != 0, min_area).astype(np.uint8) * 255), None

    def dilate(m, iters):
        calls.append(("penumbra", iters))
        return t(P.dilate(m.numpy()[..., 0] != 0, iters).astype(np.uint8) * 255)

    def merge(d, s, counts):
        calls.append(("merge", tuple(d.shape)))
        dn, sn = d.numpy() != 0, s.numpy() != 0
        counts[:, 1] += t((sn & ~dn).reshape(len(dn), -1).sum(1).astype(np.int64))                   # in place, as the device does
        return t((dn | sn).astype(np.uint8) * 255)

    monkeypatch.setattr(hip, "mask_bbox", mask_bbox)
    monkeypatch.setattr(hip, "mask_collapse_dilate", dilate)
    monkeypatch.setattr(mask_hip, "time_bridge_grow", time_bridge_grow)
    monkeypatch.setattr(mask_hip, "despeckle", despeckle)
    monkeypatch.setattr(shadow_hip, "plate", plate)
    monkeypatch.setattr(shadow_hip, "candidates", candidates)
    monkeypatch.setattr(shadow_hip, "grow", grow)
    monkeypatch.setattr(shadow_hip, "merge", merge)
    return infill, calls, t


def test_shadow_mask_crop_segments_copy_on_write_and_report(host_kernels):
    infill, calls, t = host_kernels
    frames, dil, band, *_ = R.shadow_clip(0, 60, H=120, W=200)                                          # a frame the widened crop does not fill
    T, H, W = dil.shape
    flist = [f.copy() for f in frames]
    kept = [f.copy() for f in flist]
    d = t(dil)
    cfg = ShadowMaskConfig(reach=6, grow=1)
    kw = {k: getattr(cfg, k) for k in KEYS}
    for cuts in (None, [9, 15], [12]):
        del calls[:]
        got, rep = infill.shadow_mask(flist, d, cfg, cuts)
        wd, wc = R.shadow_mask(frames, dil, cuts=cuts, **kw)
        assert got is not d and (got.numpy() == wd).all() and wc[:, 1].sum() > 0
        assert rep.added.dtype == np.int64 and (rep.added == wc[:, 1]).all() and (rep.candidates <= wc[:, 0]).all() and rep.candidates.sum() > 0
        assert rep.cuts == tuple(cuts or ()) and list(rep.segments) == spans.segments(T, cuts) and rep.skipped == (False,) * len(rep.segments)
        assert all(p > 0 for p in rep.plate) and len(rep.plate) == len(rep.segments)
        assert all((a == b).all() for a, b in zip(flist, kept)) and (d.numpy() == dil).all()           # the caller's arrays are never written
        # one upload per segment: the union box of its masks widened by reach + grow = 7, clamped, x to multiples of 4
        want_shapes = []
        for s, e in spans.segments(T, cuts):
            ys, xs = np.nonzero(dil[s:e].any(axis=(0, 2)))[0], np.nonzero(dil[s:e].any(axis=(0, 1)))[0]
            y0, y1 = max(ys[0] - 7, 0), min(ys[-1] + 1 + 7, H)
            x0, x1 = max(xs[0] // 4 * 4 - 7, 0) // 4 * 4, min(W, -(-min(min(W, -(-(xs[-1] + 1) // 4) * 4) + 7, W) // 4) * 4)
            want_shapes.append((e - s, y1 - y0, x1 - x0, 3))
        assert [c[1] for c in calls if c[0] == "plate"] == want_shapes and all(sh[1] < H and sh[2] < W for sh in want_shapes)
        assert [c for c in calls if c[0] == "guard"] == [("guard", e - s, 0, 1) for s, e in spans.segments(T, cuts)]
        assert ("grow", 6) in calls and ("despeckle", 16) in calls and ("penumbra", 1) in calls and ("candidates", 30, 90, 12, 20, 16) in calls
        assert [c[0] for c in calls].count("bbox") == 1
    # the crop changes no mask: the same masks as on the full frame (a crop of the whole frame)
    wide, _ = infill.shadow_mask(flist, d, ShadowMaskConfig(reach=64, grow=16, min_area=16), None)
    assert (wide.numpy() == R.shadow_mask(frames, dil, **dict(kw, reach=64, grow=16))[0]).all()
    # guard = 0, min_area <= 1 and grow = 0 launch nothing for them
    del calls[:]
    got, rep = infill.shadow_mask(flist, d, ShadowMaskConfig(guard=0, min_area=1, grow=0), None)
    assert (got.numpy() == R.shadow_mask(frames, dil, **dict(R.DEFAULTS, guard=0, min_area=1, grow=0))[0]).all()
    assert not [c for c in calls if c[0] in ("guard", "despeckle", "penumbra")]


def test_shadow_mask_skips_and_nothing_to_do(host_kernels):
    infill, calls, t = host_kernels
    frames, dil, band, *_ = R.shadow_clip(0, 60)
    flist = list(frames)
    d = t(dil)
    # max_bytes: the widened crop of the whole clip is the whole frame, 24 * 40 * 56 * 3 bytes
    full = 24 * 40 * 56 * 3
    got, rep = infill.shadow_mask(flist, d, ShadowMaskConfig(max_bytes=full - 1), None)
    assert rep.skipped == (True,) and got is d and not rep.added.any() and not rep.candidates.any() and rep.plate == (0,)
    assert not [c for c in calls if c[0] in ("plate", "grow", "merge")]
    got, rep = infill.shadow_mask(flist, d, ShadowMaskConfig(max_bytes=full), None)
    assert rep.skipped == (False,) and rep.added.sum() > 0
    # a segment without a mask pixel uploads nothing; one segment skipped, the others run
    m2 = dil.copy()
    m2[:6] = 0
    del calls[:]
    got, rep = infill.shadow_mask(flist, t(m2), ShadowMaskConfig(max_bytes=8 * 40 * 56 * 3), [6, 14])
    assert rep.skipped == (False, False, True) and rep.plate[0] == 0 and rep.plate[1] > 0 and rep.plate[2] == 0
    assert [c[1][0] for c in calls if c[0] == "plate"] == [8] and not rep.added[:6].any() and not rep.added[14:].any() and rep.added[6:14].sum() > 0
    want = R.shadow_mask(frames, m2, cuts=[6, 14])[0]
    assert (got.numpy()[:14] == want[:14]).all() and (got.numpy()[14:] == m2[14:]).all()
    # no mask at all, a clip without a shadow, a pan: the masks come back as the same object
    z = t(np.zeros_like(dil))
    del calls[:]
    got, rep = infill.shadow_mask(flist, z, ShadowMaskConfig(), None)
    assert got is z and rep.plate == (0,) and calls == [("bbox", (24, 40, 56))]                        # nothing uploaded, nothing launched
    cf, cm, *_ = P.locked_off_clip(T=24, H=40, W=56, a=6, seed=0)
    cd = t((P.dilate(cm != 0, 2) * 255).astype(np.uint8))
    got, rep = infill.shadow_mask(list(cf), cd, ShadowMaskConfig(), None)
    assert got is cd and not rep.added.any() and rep.plate[0] > 0
    pf, pm, _, _ = P.panning_clip()
    pd = t(pm)
    got, rep = infill.shadow_mask(list(pf), pd, ShadowMaskConfig(), None)
    assert got is pd and not rep.added.any() and not rep.candidates.any() and rep.plate == (0,)


def test_the_call_runs_the_stage_between_clean_up_and_fill_and_the_detector_once(monkeypatch):
    """run_infill_on_frames with the device replaced: the stage gets the cleaned masks, the clean-plate fill gets the stage's masks, both get
    the same cuts, the span plan takes them, and infill.clip_cuts (the detector) runs once."""
    import torch

    import diffuerase
    from videovanish_amd import hip, infill
    for name in ("VV_SHADOW_MASK", "VV_PLATE_FILL", "VV_SPANS", "VV_MASK_CLEAN"):
        monkeypatch.delenv(name, raising=False)
    T = 6
    frames = [np.zeros((8, 8, 3), np.uint8) for _ in range(T)]
    log = []
    tag = lambda v: torch.full((T, 8, 8), v, dtype=torch.uint8)
    monkeypatch.setattr(diffuerase, "get_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(hip, "mask_collapse_dilate", lambda m, it: tag(1))

    def clip_cuts(f, d, scfg):
        log.append(("cuts", int(d[0, 0, 0]), scfg.cuts))
        return list(scfg.cuts) if isinstance(scfg.cuts, tuple) else [3]

    def shadow_mask(f, d, cfg, cuts=None):
        log.append(("shadow", int(d[0, 0, 0]), cuts, cfg))
        return tag(2), infill.ShadowMaskReport(np.zeros(T, np.int64), np.ones(T, np.int64), (5,), (False,), ((0, T),), tuple(cuts or ()))

    def plate_fill(f, d, cfg, cuts=None, **more):
        log.append(("fill", int(d[0, 0, 0]), cuts))
        return f, tag(3), "fill report"

    def span_plan(f, d, scfg):
        log.append(("plan", int(d[0, 0, 0]), scfg.cuts))
        return []

    monkeypatch.setattr(infill, "clip_cuts", clip_cuts)
    monkeypatch.setattr(infill, "shadow_mask", shadow_mask)
    monkeypatch.setattr(infill, "plate_fill", plate_fill)
    monkeypatch.setattr(infill, "span_plan", span_plan)
    monkeypatch.setattr(infill, "run_spans", lambda f, d, prior, plan, body, prog, **kw: list(f))
    run = lambda **kw: diffuerase.run_infill_on_frames(frames, frames, **kw)
    out = run(shadow_mask="reach=3", plate_fill="on", spans="masked-cuts")
    assert len(out) == T and [e[0] for e in log] == ["cuts", "shadow", "fill", "plan"]                # the detector once, the stage before the fill
    assert log[0] == ("cuts", 1, "auto") and log[1][:3] == ("shadow", 1, [3]) and log[1][3] == ShadowMaskConfig(reach=3)
    assert log[2] == ("fill", 2, [3]) and log[3] == ("plan", 3, (3,))
    assert diffuerase.last_shadow_mask.added.sum() == T and diffuerase.last_plate_fill == "fill report"
    # alone: it needs no plate_fill; explicit cuts go to it as they are; without spans there is one segment
    del log[:]
    run(shadow_mask="on", spans="masked", cuts=[2, 4])
    assert [e[0] for e in log] == ["cuts", "shadow", "plan"] and log[1][2] == [2, 4] and log[2] == ("plan", 2, (2, 4))
    assert diffuerase.last_plate_fill is None
    del log[:]
    monkeypatch.setattr(infill, "run_clip", lambda f, d, *a, **kw: log.append(("clip", int(d[0, 0, 0]))) or list(f))
    run(shadow_mask=ShadowMaskConfig())
    assert [e[:3] for e in log] == [("shadow", 1, None), ("clip", 2)]
    # the cuts the mask clean-up found are handed on: the detector still runs once
    del log[:]
    monkeypatch.setattr(infill, "clean_masks", lambda m, d, ccfg, cuts=None: (tag(7), infill.MaskCleanReport(*(np.zeros(T, np.int64),) * 4, tuple(cuts(d)))))
    run(shadow_mask="on", plate_fill="on", mask_clean="on", spans="cuts")
    assert [e[0] for e in log] == ["cuts", "cuts", "shadow", "fill", "plan"] and log[0] == ("cuts", 1, "auto") and log[1] == ("cuts", 7, (3,))
    assert log[2][:3] == ("shadow", 7, [3]) and log[3] == ("fill", 2, [3])
    # without the option the stage is not called
    del log[:]
    run(plate_fill="on")
    assert [e[0] for e in log] == ["fill", "clip"] and diffuerase.last_shadow_mask is None


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_precedence_argument_configure_environment(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_SHADOW_MASK", raising=False)
    row = diffuerase._OPTION["shadow_mask"]
    assert row in diffuerase.MORE_OPTIONS and row not in diffuerase.OPTIONS and len(diffuerase.OPTIONS) == 10
    assert row.env == "VV_SHADOW_MASK" and row.settings is SM and [SM.as_config(x) for x in row.metavar.split("|")] == [ShadowMaskConfig()] * 2
    try:
        diffuerase.configure()
        assert diffuerase.shadow_mask_config() is None
        monkeypatch.setenv("VV_SHADOW_MASK", "tol=9")
        assert diffuerase.shadow_mask_config() == ShadowMaskConfig(tol=9)
        diffuerase.configure(shadow_mask="guard=2")
        assert diffuerase.shadow_mask_config() == ShadowMaskConfig(guard=2)
        assert diffuerase.shadow_mask_config("on") == ShadowMaskConfig()
        assert diffuerase.shadow_mask_config("off") is None and diffuerase.shadow_mask_config(False) is None
        mine = ShadowMaskConfig(reach=3)
        assert diffuerase.shadow_mask_config(mine) is mine
        diffuerase.configure(shadow_mask="off")
        assert diffuerase.shadow_mask_config() is None                                                     # configure("off") beats the environment
        diffuerase.configure()
        assert diffuerase.shadow_mask_config() == ShadowMaskConfig(tol=9)                                  # configure() resets
        with pytest.raises(ValueError):
            diffuerase.configure(shadow_mask="sometimes")
        monkeypatch.setenv("VV_SHADOW_MASK", "sometimes")
        diffuerase.configure()
        with pytest.raises(ValueError):
            diffuerase.shadow_mask_config()
    finally:
        diffuerase.configure()


def test_shadow_mask_refuses_the_reference_early_return_and_is_keyword_only(monkeypatch):
    import inspect

    import diffuerase
    monkeypatch.delenv("VV_SHADOW_MASK", raising=False)
    f = [np.zeros((8, 8, 3), np.uint8)] * 2
    for value in ("on", "tol=1", ShadowMaskConfig()):
        with pytest.raises(ValueError, match="shadow_mask="):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, shadow_mask=value)
    monkeypatch.setenv("VV_SHADOW_MASK", "on")
    with pytest.raises(ValueError, match=r"shadow_mask= \(shadow masking\) cannot be combined with compat_reference_early_return=True"):
        diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)
    with pytest.raises(TypeError):
        diffuerase.run_infill_on_frames(f, f, shadowmask="on")
    p = inspect.signature(diffuerase.run_infill_on_frames).parameters["shadow_mask"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert "shadow_mask" in inspect.signature(diffuerase.configure).parameters
    assert diffuerase.last_shadow_mask is None                                                         # reset at the start of every call


def test_cli_shadow_mask_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
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
        diffuerase.last_shadow_mask = infill.ShadowMaskReport(z + [300, 10, 80], z + [100, 0, 50], (40,), (False,), ((0, 3),), ()) if "shadow_mask" in kw else None
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 3
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    monkeypatch.setattr(sys, "argv", argv)
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None} and capsys.readouterr().out == ""                      # a default call passes no keyword, prints nothing
    for value in ("on", "reach=8,chroma=10"):
        monkeypatch.setattr(sys, "argv", argv + ["--shadow-mask", value, "--plate-fill", "on"])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "shadow_mask": value, "plate_fill": "on"}
        out = capsys.readouterr().out
        assert out.count("\n") == 1 and out.startswith("shadow mask: 150 px added in 2 of 3 frames from 390 candidate px, 0 of 1 segments skipped")
    for bad in ("off", "yes", "tol=x", "reach=65"):
        monkeypatch.setattr(sys, "argv", argv + ["--shadow-mask", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_shadow_mask", None)
