"""Overlay masking on the CPU: the settings, the binding of include/overlaymask.h, the restatement (tests/overlaymask_ref.py) on the shared clips,
the orchestration with the device functions replaced by the restatement, configuration and CLI."""
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
import overlaymask_ref as R  # noqa: E402

from videovanish_amd import overlaymask as OM  # noqa: E402
from videovanish_amd.overlaymask import OverlayMaskConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("min_samples", "mag", "coh", "max_share", "close", "max_hole", "min_area", "max_area", "border", "grow")


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_spellings_and_config():
    assert OM.SPELLINGS == ("on",) and OM.VERDICTS == ("none", "static", "found")
    for off in (None, False, "off", "none", "", " OFF "):
        assert OM.as_config(off) is None
    d = OverlayMaskConfig()
    assert OM.as_config("on") == OM.as_config(" On ") == OM.as_config(True) == d
    assert tuple(getattr(d, k) for k in KEYS) == (12, 8, 80, 25, 2, 4096, 64, 10, 0, 3) == tuple(R.DEFAULTS[k] for k in KEYS)
    assert d.max_bytes == 1 << 30
    assert OM.as_config("min_samples=12,mag=8,coh=80,max_share=25,close=2,max_hole=4096,min_area=64,max_area=10,border=0,grow=3") == d
    assert OM.as_config(" mag = 9 , coh = 70 ") == OverlayMaskConfig(mag=9, coh=70)
    assert OM.as_config("max_bytes=1000").max_bytes == 1000 and OM.as_config("border=1").border == 1
    assert OM.as_config("min_samples=65535,mag=2040,coh=100,max_share=100,close=16,max_hole=2147483647,min_area=2147483647,max_area=100,grow=16") == \
        OverlayMaskConfig(65535, 2040, 100, 100, 16, 2 ** 31 - 1, 2 ** 31 - 1, 100, 0, 16)
    assert OM.as_config("min_samples=1,mag=1,coh=1,max_share=0,close=0,max_hole=0,min_area=0,max_area=1,grow=0") == OverlayMaskConfig(1, 1, 1, 0, 0, 0, 0, 1, 0, 0)
    cfg = OverlayMaskConfig(grow=0)
    assert OM.as_config(cfg) is cfg
    for bad in ("yes", "static", "mag", "mag=", "mag=x", "mag=-3", "mag=1.5", "mag=3,mag=4", "size=3", "mag=3;coh=1", "min_samples=0", "min_samples=65536",
                "mag=0", "mag=2041", "coh=0", "coh=101", "max_share=101", "close=17", "max_hole=2147483648", "min_area=2147483648", "max_area=0",
                "max_area=101", "border=2", "grow=17", "on,mag=1", "mag=3,", 3, 1.0, ("on",)):
        with pytest.raises(ValueError):
            OM.as_config(bad)
    for kw in (dict(min_samples=0), dict(min_samples=65536), dict(mag=0), dict(mag=2041), dict(coh=0), dict(coh=101), dict(max_share=-1), dict(max_share=101),
               dict(close=-1), dict(close=17), dict(max_hole=-1), dict(min_area=-1), dict(max_area=0), dict(max_area=101), dict(border=-1), dict(border=2),
               dict(grow=-1), dict(grow=17), dict(max_bytes=-1), dict(mag=8.0), dict(border=True), dict(grow="2")):
        with pytest.raises(ValueError):
            OverlayMaskConfig(**kw)
    # rule 6's per cent as pixels, and the batches of the upload
    assert d.max_area_px(96, 128) == 1228 and OverlayMaskConfig(max_area=100).max_area_px(46340, 46340) == 46340 * 46340 < 2 ** 31
    assert d.batch_frames(1080, 1920) == (1 << 30) // (1080 * 1920 * 3) == 172
    assert OverlayMaskConfig(max_bytes=5 * 96 * 128 * 3).batch_frames(96, 128) == 5 and OverlayMaskConfig(max_bytes=0).batch_frames(96, 128) == 1


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_overlaymask_header():
    """overlaymask_bind.SIGNATURES declares every function of include/overlaymask.h with the header's types and in its order, lib() has applied
    it, the version and the limits agree (abiref.check_binding); arguments are refused before anything touches a device; the vvo_ prefix and
    every name belong to no part of abiref.parts() (what test_abi_cpu.py's walk does for the parts of its table)."""
    from videovanish_amd import overlaymask_bind as B
    loaded, define = abiref.check_binding(B, 7)
    assert B.EXPORTS == ["vvo_abi_version", "vvo_last_error", "vvo_accumulate", "vvo_classify", "vvo_component_stats", "vvo_select", "vvo_merge"]
    assert define("VVO_ABI_VERSION") == 1
    assert (define("VVO_MAX_T"), define("VVO_MAX_MAG"), define("VVO_MAX_COH"), define("VVO_MAX_BOXES")) == (B.MAX_T, B.MAX_MAG, B.MAX_COH, B.MAX_BOXES) == \
        (OM.MAX_T, OM.MAX_MAG, OM.MAX_COH, OM.MAX_BOXES) == (65535, 2040, 100, 256) and R.MAX_BOXES == 256
    assert (define("VVO_TILE_W"), define("VVO_TILE_H")) == (B.TILE_W, B.TILE_H) == (64, 16)
    # Nothing can be launched here: every pointer is host memory and every call below is refused before the first device call.
    buf = (ctypes.c_char * 64)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 16
    acc = lambda T=2, H=8, W=8, f=a, d=a, o=a: loaded.vvo_accumulate(f, d, T, H, W, o, None)
    cla = lambda H=8, W=8, ms=12, mag=8, coh=80, s=a, e=a, c=a: loaded.vvo_classify(s, H, W, ms, mag, coh, e, c, None)
    sta = lambda H=8, W=8, l=a, s=a: loaded.vvo_component_stats(l, H, W, s, None)
    sel = lambda H=8, W=8, lo=0, hi=9, inside=1, l=a, s=a, o=a, bx=a, n=a: loaded.vvo_select(l, s, H, W, lo, hi, inside, o, bx, n, None)
    mer = lambda T=2, H=8, W=8, d=a, o=a, out=b, c=a: loaded.vvo_merge(d, o, T, H, W, out, c, None)
    for fn, name in ((acc, b"vvo_accumulate:"), (cla, b"vvo_classify:"), (sta, b"vvo_component_stats:"), (sel, b"vvo_select:"), (mer, b"vvo_merge:")):
        for bad in (dict(H=0), dict(W=0), dict(H=-1), dict(H=1 << 16, W=1 << 15)):
            assert fn(**bad) == -1 and loaded.vvo_last_error().startswith(name), (name, bad)
    assert [acc(T=0), acc(f=None), acc(d=None), acc(o=None), mer(T=0), mer(d=None), mer(o=None), mer(out=None), mer(c=None)] == [-1] * 9
    assert mer(out=a) == -1 and b"dil_out is not dil" in loaded.vvo_last_error()
    assert [acc(T=65536), mer(T=65536)] == [-2] * 2 and b"65536" in loaded.vvo_last_error()
    assert [cla(ms=0), cla(mag=0), cla(coh=0), cla(s=None), cla(e=None), cla(c=None)] == [-1] * 6
    assert [cla(ms=65536), cla(mag=2041), cla(coh=101)] == [-2] * 3 and b"coh" in loaded.vvo_last_error()
    assert [sta(l=None), sta(s=None), sel(lo=-1), sel(hi=-1), sel(l=None), sel(s=None), sel(o=None), sel(bx=None), sel(n=None)] == [-1] * 9
    with pytest.raises(ctypes.ArgumentError):
        acc(T=2.0)
    import torch
    f, z = torch.zeros((2, 4, 4, 3), dtype=torch.uint8), torch.zeros((2, 4, 4), dtype=torch.uint8)
    s4, lab = torch.zeros((4, 4, 4), dtype=torch.int32), torch.zeros((4, 4), dtype=torch.int32)
    for call in (lambda: B.accumulate(f, z, s4), lambda: B.classify(s4, 12, 8, 80), lambda: B.component_stats(lab),
                 lambda: B.select(lab, torch.zeros((16, 5), dtype=torch.int32), 0, 9, True), lambda: B.merge(z, z[0])):
        with pytest.raises(RuntimeError):                                                               # no CPU fallback
            call()
    # the part stands outside abiref.PARTS: its prefix and names are checked against every part here
    assert "overlaymask_bind" not in abiref.PARTS and abiref.part_of(B) is B.PART and B.PART.header == "overlaymask.h"
    assert B.PART.prefix == "vvo_" and re.fullmatch(r"vv[a-z]_", B.PART.prefix)
    names = set(B.SIGNATURES)
    others = list(abiref.parts())
    for extra in ("platetone_bind", "detailmatch_bind", "grainshape_bind", "flicklocal_bind"):          # the other parts outside the table
        m = __import__("videovanish_amd." + extra, fromlist=["PART"])
        others.append((m, m.PART))
    for module, part in others:
        assert part.prefix != B.PART.prefix and part.header != B.PART.header, module.__name__
        assert not names & set(module.SIGNATURES), module.__name__
        assert not [n for n in module.SIGNATURES if n.startswith(B.PART.prefix)], module.__name__
    assert all(n.startswith("vvo_") for n in names)
    # the file names stay outside the two globs of test_abi_cpu.py's walk
    assert not B.__name__.endswith("_hip") and not B.PART.header.startswith("vv")


def test_product_sources_of_the_feature():
    """vv_overlay is in the one build recipe with its header among the dependencies, reads no environment and takes its byte loads and wave
    operations from the shared header; the settings import neither torch nor numpy; importing the drop-in resolves no vvo_ symbol, and neither
    does a call's set-up without the option."""
    kernel, txt = abiref.check_sources("vv_overlay", "overlaymask.h", "overlaymask")
    for fn in ("vvo_accumulate", "vvo_classify", "vvo_component_stats", "vvo_select", "vvo_merge"):
        assert f'extern "C" int {fn}(' in kernel
    assert '#include "vv_wave_bytes.h"' in kernel and "vvwave::luma" in kernel and "__shared__ unsigned plane[2]" in kernel
    assert not re.search(r"^\s*(import|from)\s+(torch|numpy|oracle)\b", txt, flags=re.M)
    header = open(os.path.join(ROOT, "include", "overlaymask.h")).read()
    for rule in ("1. Gradients", "2. Persistent edges", "3. Guard", "4. Closing", "5. Holes", "6. Selection", "7. Fringe", "8. Counts", "build-defined"):
        assert rule in header
    code = ("import sys, diffuerase; from videovanish_amd import overlaymask_bind, hip; assert overlaymask_bind.PART.dll is None and hip.CORE.dll is None; "
            "assert diffuerase.overlay_mask_config() is None and diffuerase.last_overlay_mask is None; "
            "import videovanish_amd.overlaymask")
    env = {k: v for k, v in os.environ.items() if k != "VV_OVERLAY_MASK"}
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)
    alone = "import sys, videovanish_amd.overlaymask; assert 'torch' not in sys.modules and 'numpy' not in sys.modules"
    subprocess.check_call([sys.executable, "-c", alone], cwd=ROOT, env=env)


# ---- the rule on the shared clips: a failure here means the rule is wrong, not the kernel ---------------------------------------------------
def _zero(frames):
    return np.zeros(frames.shape[:3], np.uint8)


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("alpha, noise", [(1.0, 2.0), (0.4, 2.0), (0.4, 6.0)], ids=["opaque", "alpha0.4", "alpha0.4-noise6"])
def test_reference_finds_the_logo_and_nothing_else(alpha, noise, seed):
    frames, logo = R.overlay_clip(seed, alpha, noise=noise)
    r = R.overlay(frames, _zero(frames))
    print(f"alpha {alpha} noise {noise} seed {seed}: {r['verdict']}, {r['edges']} of {r['strong']} strong px persistent, boxes {r['boxes'].tolist()}, "
          f"{int((logo & ~r['O']).sum())} logo px missed, {int((r['O'] & R.far_from(logo, 8)).sum())} px further than 8 px from the logo")
    assert logo.sum() == 640 and r["verdict"] == "found" and r["found"] == 1 and r["boxes"].shape == (1, 5)
    assert not (logo & ~r["O"]).any() and not (r["O"] & R.far_from(logo, 8)).any()
    x0, y0, x1, y1, area = r["boxes"][0]
    assert area == r["kept"].sum() and x0 <= R.LOGO_AT[1] and y0 <= R.LOGO_AT[0] and x1 >= R.LOGO_AT[1] + 40 and y1 >= R.LOGO_AT[0] + 16
    assert (r["added"] == r["O"].sum()).all() and ((r["dil2"] != 0) == r["O"][None]).all() and set(np.unique(r["dil2"])) == {0, 255}


def test_reference_static_flat_and_band():
    for seed in range(3):
        frames, _ = R.overlay_clip(seed, speed=0)                                                      # locked off: every edge is persistent
        d = _zero(frames)
        r = R.overlay(frames, d)
        print(f"locked-off clip, seed {seed}: {r['edges']} of {r['strong']} strong px persistent")
        assert r["verdict"] == "static" and 100 * r["edges"] >= 95 * r["strong"] > 0 and r["dil2"] is d and not r["added"].any() and not r["O"].any()
    flat = np.full((24, 32, 48, 3), 90, np.uint8)
    r = R.overlay(flat, _zero(flat))
    assert r["verdict"] == "none" and r["strong"] == 0 and not r["O"].any()
    for seed in range(3):                                                                              # a horizon under a horizontal pan
        frames, _ = R.overlay_clip(seed, logo=False, band=(60, 66))
        got = {b: R.overlay(frames, _zero(frames), border=b, max_area=30) for b in (0, 1)}
        assert got[0]["verdict"] == "none" and got[0]["edges"] > 256 and not got[0]["O"].any()          # a coherent edge; only the border rule drops it
        assert got[1]["verdict"] == "found" and got[1]["found"] == 1
        x0, y0, x1, y1, area = got[1]["boxes"][0]
        assert (x0, x1) == (0, 128) and y0 < 60 and y1 > 66 and got[1]["O"][59:67].all()


@pytest.mark.parametrize("seed", range(1, 5))
def test_reference_a_user_mask_across_the_logo_changes_nothing_outside_itself(seed):
    frames, logo = R.overlay_clip(seed)
    dil = _zero(frames)
    for t in range(5, 13):                                                                              # an object passes over the logo for 8 frames
        dil[t, 8:34, 60 + 4 * (t - 5):76 + 4 * (t - 5)] = 255
    assert (dil != 0)[:, logo].any()
    base, r = R.overlay(frames, _zero(frames)), R.overlay(frames, dil)
    assert r["acc"][..., 0].min() == 20 and (r["acc"][..., 0][logo] < 24).any()                          # 16 px wide at 4 px a frame: four samples fewer
    assert r["verdict"] == "found" and (r["O"] == base["O"]).all() and ((r["dil2"] != 0) == ((dil != 0) | base["O"][None])).all()
    assert (r["added"] == (base["O"][None] & (dil == 0)).reshape(24, -1).sum(1)).all() and r["added"][5:13].max() < base["O"].sum()


def test_reference_pieces():
    """The restatement's own parts on hand-made maps: labels are smallest linear indices with 8-connectivity, boxes are exclusive, the cross."""
    m = np.zeros((5, 7), bool)
    m[0, 0] = m[1, 1] = m[3, 5] = m[4, 6] = m[3, 3] = True
    lab = R.labels(m)
    assert lab[0, 0] == lab[1, 1] == 0 and lab[3, 5] == lab[4, 6] == 26 and lab[3, 3] == 24 and (lab[~m] == -1).all()
    st = R.component_stats(lab)
    assert st[0].tolist() == [2, 0, 0, 2, 2] and st[26].tolist() == [2, 5, 3, 7, 5] and st[24].tolist() == [1, 3, 3, 4, 4] and st[1].tolist() == [0, 7, 5, 0, 0]
    out, boxes = R.select(lab, st, 1, 9, True)
    assert out.sum() == 1 and out[3, 3] and boxes.tolist() == [[24, 1, 3, 3, 4, 4]]
    out, boxes = R.select(lab, st, 2, 9, False)
    assert out.sum() == 4 and boxes[:, 0].tolist() == [0, 26]
    assert R.dilate(m, 0) is not m and (R.dilate(m, 0) == m).all() and R.dilate(np.pad(np.ones((1, 1), bool), 2), 2).sum() == 13
    f = np.zeros((1, 3, 3, 3), np.uint8)
    f[0, :, 2] = 255
    gx, gy = R.gradients(f)
    assert gx[0].tolist() == [[0, 1020, 1020]] * 3 and not gy.any()                                     # the replicated border adds no edge of its own
    assert R.luma(np.array([[255, 255, 255], [0, 0, 0], [255, 0, 0]], np.uint8)).tolist() == [255, 0, 77]


# ---- orchestration ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def host_kernels(monkeypatch):
    """infill.overlay_mask with every device call replaced by the restatement on host tensors; the calls made are recorded."""
    import torch
    from videovanish_amd import hip, infill, mask_hip, overlaymask_bind as B
    calls = []
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))

    def accumulate(f, d, acc):
        calls.append(("accumulate", tuple(f.shape)))
        assert f.is_contiguous() and d.is_contiguous() and f.dtype == torch.uint8
        acc += t(R.accumulate(f.numpy(), d.numpy()).astype(np.int32))
        return acc

    def classify(acc, min_samples, mag, coh):
        calls.append(("classify", min_samples, mag, coh))
        strong, E = R.classify(acc.numpy(), min_samples, mag, coh)
        return t(E.astype(np.uint8) * 255), torch.tensor([int(strong.sum()), int(E.sum())], dtype=torch.int64)

    def dilate(m, iters):
        calls.append(("dilate", iters))
        assert iters >= 1                                                                               # 0 would mean "to convergence"
        assert m.dim() == 4 and m.shape[3] == 1 and m.is_contiguous()
        return t(np.stack([R.dilate(x != 0, iters) for x in m.numpy()[..., 0]]).astype(np.uint8) * 255)

    def label_components(m):
        calls.append(("label", tuple(m.shape)))
        return t(np.stack([R.labels(x != 0) for x in m.numpy()]))

    def component_stats(lab):
        return t(R.component_stats(lab.numpy()))

    def select(lab, stats, min_area, max_area_px, inside_only):
        calls.append(("select", min_area, max_area_px, bool(inside_only)))
        out, boxes = R.select(lab.numpy(), stats.numpy(), min_area, max_area_px, inside_only)
        full = np.full((256, 6), -7, np.int32)
        full[:min(len(boxes), 256)] = boxes[:256][::-1]                                                 # in any order: the host sorts
        return t(out.astype(np.uint8) * 255), t(full), torch.tensor([len(boxes)], dtype=torch.int32)

    def merge(d, o):
        calls.append(("merge", tuple(d.shape)))
        dn, on = d.numpy() != 0, o.numpy() != 0
        return t((dn | on[None]).astype(np.uint8) * 255), t((on[None] & ~dn).reshape(len(dn), -1).sum(1).astype(np.int64))

    monkeypatch.setattr(hip, "mask_collapse_dilate", dilate)
    monkeypatch.setattr(mask_hip, "label_components", label_components)
    monkeypatch.setattr(B, "new_acc", lambda H, W, dev: torch.zeros((H, W, 4), dtype=torch.int32))
    for name, fn in (("accumulate", accumulate), ("classify", classify), ("component_stats", component_stats), ("select", select), ("merge", merge)):
        monkeypatch.setattr(B, name, fn)
    return infill, calls, t


def test_overlay_mask_batches_steps_and_report(host_kernels):
    infill, calls, t = host_kernels
    frames, logo = R.overlay_clip(2, 0.4)
    T, H, W = frames.shape[:3]
    flist = [f.copy() for f in frames]
    dil = _zero(frames)
    dil[3:9, 40:60, 10:30] = 255
    d = t(dil)
    want = R.overlay(frames, dil)
    for max_bytes, shapes in ((1 << 30, [(24, H, W, 3)]), (5 * H * W * 3, [(5, H, W, 3)] * 4 + [(4, H, W, 3)]), (0, [(1, H, W, 3)] * 24)):
        del calls[:]
        got, rep = infill.overlay_mask(flist, d, OverlayMaskConfig(max_bytes=max_bytes))
        assert [c[1] for c in calls if c[0] == "accumulate"] == shapes
        assert got is not d and (got.numpy() == want["dil2"]).all() and want["verdict"] == "found"
        assert isinstance(rep, infill.OverlayMaskReport) and rep._fields == ("verdict", "strong", "edges", "boxes", "found", "added", "overlay")
        assert (rep.verdict, rep.strong, rep.edges, rep.found) == ("found", want["strong"], want["edges"], 1)
        assert rep.boxes.dtype == np.int32 and (rep.boxes == want["boxes"]).all() and rep.added.dtype == np.int64 and (rep.added == want["added"]).all()
        assert rep.overlay.dtype == np.uint8 and ((rep.overlay != 0) == want["O"]).all() and rep.added[3:9].max() <= rep.added[0]
        assert [c for c in calls if c[0] != "accumulate"] == [("classify", 12, 8, 80), ("dilate", 2), ("label", (1, H, W)), ("select", 0, 4096, True),
                                                              ("merge", (1, H, W)), ("label", (1, H, W)), ("select", 64, 1228, True), ("dilate", 3),
                                                              ("merge", (T, H, W))]
    assert all((a == b).all() for a, b in zip(flist, frames)) and (d.numpy() == dil).all()               # the caller's arrays are never written
    # close = 0 and grow = 0 launch no dilation; border = 1 asks for every place; several boxes come back in label order
    del calls[:]
    two = frames.copy()
    two[:, 60:76, 20:60] = two[:, 14:30, 72:112]                                                         # the logo a second time, lower left
    got, rep = infill.overlay_mask(list(two), t(_zero(two)), OverlayMaskConfig(close=0, grow=0, border=1, min_area=16))
    want = R.overlay(two, _zero(two), close=0, grow=0, border=1, min_area=16)
    assert "dilate" not in [c[0] for c in calls] and ("select", 16, 1228, False) in calls
    assert rep.found == want["found"] >= 2 and (rep.boxes == want["boxes"]).all() and (got.numpy() == want["dil2"]).all()


def test_overlay_mask_none_and_static_hand_the_masks_back(host_kernels):
    infill, calls, t = host_kernels
    frames, _ = R.overlay_clip(0, speed=0)
    d = t(_zero(frames))
    got, rep = infill.overlay_mask(list(frames), d, OverlayMaskConfig())
    assert got is d and rep.verdict == "static" and rep.found == 0 and rep.boxes.shape == (0, 5) and not rep.added.any() and not rep.overlay.any()
    assert rep.strong > 0 and 100 * rep.edges > 25 * rep.strong and [c[0] for c in calls] == ["accumulate", "classify"]
    got, rep = infill.overlay_mask(list(frames), d, OverlayMaskConfig(max_share=100, max_area=1))     # the guard off: a locked-off scene is all overlay,
    assert got is d and rep.verdict == "none" and rep.found == 0                                         # which the area rule then drops
    flat = np.full((12, 16, 24, 3), 90, np.uint8)
    z = t(_zero(flat))
    del calls[:]
    got, rep = infill.overlay_mask(list(flat), z, OverlayMaskConfig())
    assert got is z and rep.verdict == "none" and rep.strong == 0 and [c[0] for c in calls] == ["accumulate", "classify"]
    with pytest.raises(ValueError, match="65535"):
        infill.overlay_mask([], np.zeros((65536, 1, 1), np.uint8), OverlayMaskConfig())


def test_the_call_runs_the_stage_after_the_clean_up_and_before_the_detector_and_the_shadows(monkeypatch):
    import torch

    import diffuerase
    from videovanish_amd import hip, infill
    for name in ("VV_OVERLAY_MASK", "VV_SHADOW_MASK", "VV_PLATE_FILL", "VV_SPANS", "VV_MASK_CLEAN"):
        monkeypatch.delenv(name, raising=False)
    T = 6
    frames = [np.zeros((8, 8, 3), np.uint8) for _ in range(T)]
    log = []
    tag = lambda v: torch.full((T, 8, 8), v, dtype=torch.uint8)
    report = infill.OverlayMaskReport("found", 9, 3, np.zeros((1, 5), np.int32), 1, np.ones(T, np.int64), np.zeros((8, 8), np.uint8))
    monkeypatch.setattr(diffuerase, "get_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(hip, "mask_collapse_dilate", lambda m, it: tag(1))
    monkeypatch.setattr(infill, "clean_masks", lambda m, d, ccfg, cuts=None: log.append(("clean", int(d[0, 0, 0]))) or
                        (tag(7), infill.MaskCleanReport(*(np.zeros(T, np.int64),) * 4, ())))
    monkeypatch.setattr(infill, "overlay_mask", lambda f, d, cfg: log.append(("overlay", int(d[0, 0, 0]), cfg)) or (tag(4), report))
    monkeypatch.setattr(infill, "clip_cuts", lambda f, d, scfg: log.append(("cuts", int(d[0, 0, 0]))) or [3])
    monkeypatch.setattr(infill, "shadow_mask", lambda f, d, cfg, cuts=None: log.append(("shadow", int(d[0, 0, 0]), cuts)) or
                        (tag(2), infill.ShadowMaskReport(np.zeros(T, np.int64), np.ones(T, np.int64), (5,), (False,), ((0, T),), tuple(cuts or ()))))
    monkeypatch.setattr(infill, "plate_fill", lambda f, d, cfg, cuts=None, **more: log.append(("fill", int(d[0, 0, 0]), cuts)) or (f, tag(3), "fill report"))
    monkeypatch.setattr(infill, "span_plan", lambda f, d, scfg: log.append(("plan", int(d[0, 0, 0]))) or [])
    monkeypatch.setattr(infill, "run_spans", lambda f, d, prior, plan, body, prog, **kw: list(f))
    monkeypatch.setattr(infill, "run_clip", lambda f, d, *a, **kw: log.append(("clip", int(d[0, 0, 0]))) or list(f))
    run = lambda **kw: diffuerase.run_infill_on_frames(frames, frames, **kw)
    run(overlay_mask="mag=9", mask_clean="on", shadow_mask="on", plate_fill="on", spans="masked-cuts")
    assert [e[0] for e in log] == ["clean", "overlay", "cuts", "shadow", "fill", "plan"]
    assert log[1] == ("overlay", 7, OverlayMaskConfig(mag=9)) and log[2] == ("cuts", 4) and log[3] == ("shadow", 4, [3]) and log[4] == ("fill", 2, [3])
    assert diffuerase.last_overlay_mask is report
    del log[:]
    run(overlay_mask="on")                                                                              # alone: it needs no other option
    assert log == [("overlay", 1, OverlayMaskConfig()), ("clip", 4)]
    del log[:]
    run(shadow_mask="on")                                                                               # without the option the stage is not called
    assert [e[0] for e in log] == ["shadow", "clip"] and diffuerase.last_overlay_mask is None
    del log[:]
    monkeypatch.setenv("VV_OVERLAY_MASK", "on")
    run(overlay_mask="off")
    assert log == [("clip", 1)] and diffuerase.last_overlay_mask is None


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_precedence_argument_configure_environment(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_OVERLAY_MASK", raising=False)
    row = diffuerase._OPTION["overlay_mask"]
    assert row in diffuerase.MORE_OPTIONS and row not in diffuerase.OPTIONS and len(diffuerase.OPTIONS) == 10
    assert row.env == "VV_OVERLAY_MASK" and row.settings is OM and row.phrase == "overlay masking"
    assert [OM.as_config(x) for x in row.metavar.split("|")] == [OverlayMaskConfig()] * 2
    try:
        diffuerase.configure()
        assert diffuerase.overlay_mask_config() is None
        monkeypatch.setenv("VV_OVERLAY_MASK", "mag=9")
        assert diffuerase.overlay_mask_config() == OverlayMaskConfig(mag=9)
        diffuerase.configure(overlay_mask="coh=70")
        assert diffuerase.overlay_mask_config() == OverlayMaskConfig(coh=70)
        assert diffuerase.overlay_mask_config("on") == OverlayMaskConfig()
        assert diffuerase.overlay_mask_config("off") is None and diffuerase.overlay_mask_config(False) is None
        mine = OverlayMaskConfig(grow=1)
        assert diffuerase.overlay_mask_config(mine) is mine
        diffuerase.configure(overlay_mask="off")
        assert diffuerase.overlay_mask_config() is None                                                    # configure("off") beats the environment
        diffuerase.configure()
        assert diffuerase.overlay_mask_config() == OverlayMaskConfig(mag=9)                                # configure() resets
        with pytest.raises(ValueError):
            diffuerase.configure(overlay_mask="sometimes")
        monkeypatch.setenv("VV_OVERLAY_MASK", "sometimes")
        diffuerase.configure()
        with pytest.raises(ValueError):
            diffuerase.overlay_mask_config()
    finally:
        diffuerase.configure()


def test_overlay_mask_refuses_the_reference_early_return_and_is_keyword_only(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_OVERLAY_MASK", raising=False)
    f = [np.zeros((8, 8, 3), np.uint8)] * 2
    for value in ("on", "mag=1", OverlayMaskConfig()):
        with pytest.raises(ValueError, match="overlay_mask="):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, overlay_mask=value)
    monkeypatch.setenv("VV_OVERLAY_MASK", "on")
    with pytest.raises(ValueError, match=r"overlay_mask= \(overlay masking\) cannot be combined with compat_reference_early_return=True"):
        diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)
    with pytest.raises(TypeError):
        diffuerase.run_infill_on_frames(f, f, overlaymask="on")
    for fn in (diffuerase.run_infill_on_frames, diffuerase.configure):
        names = list(inspect.signature(fn).parameters)
        p = inspect.signature(fn).parameters["overlay_mask"]
        assert names[-1] == "plate_fill" and names.index("overlay_mask") < names.index("plate_fill")
        assert p.default is None and (fn is diffuerase.configure or p.kind is inspect.Parameter.KEYWORD_ONLY)
    assert list(inspect.signature(diffuerase.find_overlays).parameters) == ["frames_rgb", "mask_frames", "overlay_mask"]
    assert inspect.signature(diffuerase.find_overlays).parameters["overlay_mask"].default == "on"
    with pytest.raises(ValueError, match="find_overlays"):
        diffuerase.find_overlays(f, None, "off")
    assert diffuerase.last_overlay_mask is None                                                         # reset at the start of every call


def test_find_overlays_loads_no_model_and_takes_the_masks_as_they_are(monkeypatch):
    import torch

    import diffuerase
    from videovanish_amd import infill
    seen = []
    report = infill.OverlayMaskReport("found", 9, 3, np.zeros((1, 5), np.int32), 1, np.ones(3, np.int64), np.full((8, 8), 255, np.uint8))
    monkeypatch.setattr(diffuerase, "get_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(diffuerase, "_load_model", lambda *a: pytest.fail("find_overlays loads no model"))
    monkeypatch.setattr(infill, "overlay_mask", lambda f, d, cfg: seen.append((d.numpy().copy(), cfg)) or (d, report))
    f = [np.zeros((8, 8, 3), np.uint8)] * 3
    o, rep = diffuerase.find_overlays(f)
    assert o is report.overlay and rep is report and seen[-1][0].shape == (3, 8, 8) and not seen[-1][0].any() and seen[-1][1] == OverlayMaskConfig()
    m3 = np.zeros((8, 8, 3), np.uint8)
    m3[2, 3, 1] = 7
    m2 = np.zeros((8, 8), np.uint8)
    m2[5, 5] = 1
    diffuerase.find_overlays(f, [m3, m2, m2 * 0], "grow=1")
    d, cfg = seen[-1]
    assert cfg == OverlayMaskConfig(grow=1) and d.dtype == np.uint8 and d.sum() == 2 * 255 and d[0, 2, 3] == 255 and d[1, 5, 5] == 255
    assert diffuerase.last_overlay_mask is None and diffuerase.video_inpainting_sd is None


def test_cli_overlay_mask_reaches_the_call_prints_one_line_and_makes_the_mask_video_optional(monkeypatch, tmp_path, capsys):
    import diffuerase
    from videovanish_amd import infill
    calls = []
    videos = {"mask.mkv": [np.full((16, 24, 3), 9, np.uint8)] * 3}
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda path, start=0, max_frames=-1: ([f.copy() for f in videos[path]], 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    overlay = np.zeros((16, 24), np.uint8)
    overlay[2:8, 4:20] = 255
    boxes = np.array([[5, 3, 19, 7, 50], [1, 9, 4, 12, 9]], np.int32)

    def fake(frames, masks, **kw):
        calls.append((masks, kw))
        diffuerase.last_overlay_mask = None
        if "overlay_mask" in kw:
            diffuerase.last_overlay_mask = infill.OverlayMaskReport("found", 400, 60, boxes, 2, np.array([96, 80, 96], np.int64), overlay)
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 3
    argv = ["diffuerase.py", "--color_video", str(color)]
    monkeypatch.setattr(sys, "argv", argv + ["--mask_video", "mask.mkv"])
    diffuerase.main()
    assert calls[-1][1] == {"propainer_frames": None} and capsys.readouterr().out == ""                   # a default call passes no keyword, prints nothing
    line = ("overlay mask: found, 2 overlays (14 x 4 at (5, 3), 50 px, 3 x 3 at (1, 9), 9 px), 96 px in the overlay, 80 .. 96 px added per frame, "
            "60 of 400 strong px persistent\n")
    for value in ("on", "mag=12,grow=1"):
        monkeypatch.setattr(sys, "argv", argv + ["--mask_video", "mask.mkv", "--overlay-mask", value])
        diffuerase.main()
        assert calls[-1][1] == {"propainer_frames": None, "overlay_mask": value} and (calls[-1][0][0] == 9).all()      # the mask video is still read
        assert capsys.readouterr().out == line
    # without a mask video: all-zero masks of the frames' size, only with the flag
    monkeypatch.setattr(sys, "argv", argv + ["--overlay-mask", "on"])
    diffuerase.main()
    masks, kw = calls[-1]
    assert kw == {"propainer_frames": None, "overlay_mask": "on"} and len(masks) == 3 and all(m.shape == (16, 24) and not m.any() for m in masks)
    assert capsys.readouterr().out == line
    n = len(calls)
    monkeypatch.setattr(sys, "argv", argv)
    with pytest.raises(SystemExit):
        diffuerase.main()
    assert "--mask_video" in capsys.readouterr().err and len(calls) == n
    for bad in ("off", "yes", "mag=x", "grow=17"):
        monkeypatch.setattr(sys, "argv", argv + ["--mask_video", "mask.mkv", "--overlay-mask", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_overlay_mask", None)
