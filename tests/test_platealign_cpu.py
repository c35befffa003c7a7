"""Clean-plate alignment on the CPU: the settings, the binding of include/vvalign.h, the reference restatement (tests/platealign_ref.py) against
the ground truth of synthetic pans, the orchestration with the device functions replaced by the reference, configuration and CLI."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abiref  # noqa: E402
import platealign_ref as A  # noqa: E402
import platefill_ref as R  # noqa: E402
from test_platefill_cpu import host_kernels  # noqa: E402,F401  (the fixture: plate_fill's device calls replaced by the reference)

from videovanish_amd import platealign as PA  # noqa: E402
from videovanish_amd.platealign import PlateAlignConfig  # noqa: E402
from videovanish_amd.platefill import PlateFillConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_spellings_and_config():
    assert PA.SPELLINGS == ("on",)
    for off in (None, False, "off", "none", "", " OFF "):
        assert PA.as_config(off) is None
    d = PlateAlignConfig()
    assert PA.as_config("on") == PA.as_config(" On ") == PA.as_config(True) == d
    assert (d.levels, d.radius, d.min_overlap, d.max_residual) == (4, 4, 25, 12) == tuple(A.DEFAULTS[k] for k in ("levels", "radius", "min_overlap", "max_residual"))
    assert PA.as_config("levels=4,radius=4,min_overlap=25,max_residual=12") == d
    assert PA.as_config(" radius = 8 , levels = 0 ") == PlateAlignConfig(levels=0, radius=8)
    cfg = PlateAlignConfig(max_residual=0)
    assert PA.as_config(cfg) is cfg
    for bad in ("yes", "follow", "radius", "radius=", "radius=x", "radius=-3", "radius=1.5", "radius=3,radius=4", "size=3", "radius=3;levels=1", "levels=7",
                "radius=0", "radius=9", "min_overlap=0", "min_overlap=101", "max_residual=256", "on,radius=1", "radius=3,", 3, 1.0, ("on",)):
        with pytest.raises(ValueError):
            PA.as_config(bad)
    for kw in (dict(levels=-1), dict(levels=7), dict(radius=0), dict(radius=9), dict(min_overlap=0), dict(min_overlap=101), dict(max_residual=-1),
               dict(max_residual=256), dict(radius=4.0), dict(levels=True), dict(radius="4")):
        with pytest.raises(ValueError):
            PlateAlignConfig(**kw)


def test_coarsest_level():
    assert [PA.coarsest_level(96, 128, n) for n in range(7)] == [0, 1, 2, 2, 2, 2, 2]                # 96 >> 2 = 24, 96 >> 3 = 12
    assert PA.coarsest_level(40, 56, 4) == 1 and PA.coarsest_level(45, 83, 4) == 1 and PA.coarsest_level(31, 500, 4) == 0
    assert PA.coarsest_level(15, 15, 4) == 0 and PA.coarsest_level(1080, 1920, 4) == 4 and PA.coarsest_level(1080, 1920, 6) == 6
    assert PA.coarsest_level(256, 1024, 6) == 4 and PA.coarsest_level(1024, 256, 6) == 4
    for H, W, n in ((96, 128, 4), (40, 56, 4), (15, 15, 4), (1080, 1920, 6), (720, 1280, 3)):
        assert PA.coarsest_level(H, W, n) == A.coarsest_level(H, W, n)


def test_canvas_box_and_slices():
    e = (0, 0, 0, 0)
    off = np.array([[0, 0], [5, -2], [-7, 3]])
    assert PA.canvas_box([e, e, e], off, [1, 1, 1]) is None
    assert PA.canvas_box([(4, 5, 19, 11), e, e], off, [1, 1, 1]) == (4, 4, 19, 12)
    assert PA.canvas_box([(4, 5, 19, 11), (4, 5, 19, 11), e], off, [1, 1, 1]) == (2, 4, 19, 16)      # frame 1 moved by (+5, -2)
    assert PA.canvas_box([(4, 5, 19, 11), (4, 5, 19, 11), (0, 1, 2, 3)], off, [1, 1, 1]) == (2, -8, 19, 16)      # negative canvas x, to multiples of 4
    assert PA.canvas_box([(4, 5, 19, 11), (4, 5, 19, 11), (0, 1, 2, 3)], off, [1, 0, 1]) == (3, -8, 19, 12)      # an untracked frame has no say
    assert PA.canvas_box([(4, 5, 19, 11)], off[:1], [0]) is None
    assert PA.canvas_bytes(7, (2, -8, 19, 16)) == 7 * 17 * 24 * 3
    # the frame's part of the box, on the canvas and in the frame
    assert PA.frame_slices((2, -8, 19, 16), (0, 0), 40, 56) == ((slice(0, 17), slice(8, 24)), (slice(2, 19), slice(0, 16)))
    assert PA.frame_slices((2, -8, 19, 16), (-7, 3), 40, 56) == ((slice(1, 17), slice(1, 24)), (slice(0, 16), slice(0, 23)))
    assert PA.frame_slices((2, -8, 19, 16), (60, 0), 40, 56) is None and PA.frame_slices((2, 4, 19, 16), (0, -40), 40, 56) is None
    rng = np.random.default_rng(0)
    dil = (rng.random((3, 40, 56)) < 0.01).astype(np.uint8) * 255
    track = np.zeros((3, 8), np.int32)
    track[:, :2], track[:, 3] = off, 1
    boxes = []
    for m in dil:
        ys, xs = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
        boxes.append((ys[0], xs[0], ys[-1] + 1, xs[-1] + 1))
    assert PA.canvas_box(boxes, off, [1, 1, 1]) == A.canvas_box(dil, track)


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_vvalign_header():
    """align_hip.SIGNATURES declares every function of include/vvalign.h with the header's types, align_hip.lib() has applied it, the version and
    the limits agree in the header, the binding and the settings (abiref.check_binding; test_abi_cpu.py: no name could be taken for another
    part's), and arguments are refused before anything touches a device."""
    from videovanish_amd import align_hip
    loaded, define = abiref.check_binding(align_hip, 10)
    assert define("VVA_ABI_VERSION") == 1
    limits = (define("VVA_MAX_LEVELS"), define("VVA_MAX_RADIUS"), define("VVA_MAX_PIXELS"), define("VVA_MAX_T"))
    assert limits == (align_hip.MAX_LEVELS, align_hip.MAX_RADIUS, align_hip.MAX_PIXELS, align_hip.MAX_T) == (6, 8, 1 << 24, 65535)
    assert limits == (PA.MAX_LEVELS, PA.MAX_RADIUS, PA.MAX_PIXELS, PA.MAX_T)
    assert (define("VVA_IN_PROGRESS"), define("VVA_TRACK_INTS")) == (align_hip.IN_PROGRESS, align_hip.TRACK_INTS) == (A.IN_PROGRESS, 8)
    assert PA.trackable(65535, 4096, 4096) and not PA.trackable(65536, 8, 8) and not PA.trackable(2, 4096, 4097)
    # the packed buffer's size: host arithmetic
    for H, W, L in ((40, 56, 1), (45, 83, 1), (96, 130, 2), (1080, 1920, 4), (16, 16, 0)):
        assert loaded.vva_frame_bytes(H, W, L) == sum(2 * (H >> l) * (W >> l) for l in range(L + 1)) == align_hip.frame_bytes(H, W, L)
    assert [loaded.vva_frame_bytes(0, 8, 0), loaded.vva_frame_bytes(8, 8, -1)] == [-1, -1]
    assert [loaded.vva_frame_bytes(4096, 4097, 0), loaded.vva_frame_bytes(64, 64, 7), loaded.vva_frame_bytes(8, 64, 4)] == [-2] * 3
    assert b"vva_frame_bytes" in loaded.vva_last_error()
    assert loaded.vva_track_launches(24, 2) == 1 + 23 * 3 * 3 == align_hip.track_launches(24, 2) and loaded.vva_track_launches(1, 4) == 1
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    assert loaded.vva_pyramid(None, a, 2, 32, 32, 1, a, None) == -1 and loaded.vva_pyramid(a, a, 0, 32, 32, 1, a, None) == -1
    assert loaded.vva_pyramid(a, a, 2, 32, 32, 7, a, None) == -2 and b"vva_pyramid" in loaded.vva_last_error()
    sad = lambda *v: loaded.vva_sad(a, a, *v, a, None)                                                 # T, H, W, L, t, level, r
    assert [sad(0, 32, 32, 1, 0, 0, 1), sad(2, 32, 32, 1, 2, 0, 1), sad(2, 32, 32, 1, -1, 0, 1), sad(2, 32, 32, 1, 1, 2, 1), sad(2, 32, 32, 1, 1, 0, -1)] == [-1] * 5
    assert [sad(65536, 32, 32, 1, 1, 0, 1), sad(2, 32, 32, 1, 1, 0, 9), sad(2, 4096, 4097, 1, 1, 0, 1)] == [-2] * 3 and b"vva_sad" in loaded.vva_last_error()
    pick = lambda *v: loaded.vva_pick(a, a, 2, 32, 32, 1, 1, 0, 1, *v, None)                           # min_overlap, max_residual
    assert [pick(0, 12), pick(101, 12), pick(25, -1), pick(25, 256)] == [-1] * 4 and b"vva_pick" in loaded.vva_last_error()
    trk = lambda *v: loaded.vva_track(a, a, a, *v, None)                                               # T, H, W, L, radius, min_overlap, max_residual
    assert [trk(0, 32, 32, 1, 4, 25, 12), trk(2, 32, 32, 1, 0, 25, 12), trk(2, 32, 32, 1, 4, 0, 12)] == [-1] * 3
    assert [trk(2, 32, 32, 1, 9, 25, 12), trk(65536, 32, 32, 1, 4, 25, 12), trk(2, 32, 32, 6, 4, 25, 12)] == [-2] * 3 and b"vva_track" in loaded.vva_last_error()
    assert loaded.vva_place_masks(a, a, 2, 8, 8, 0, 0, 0, 8, a, a, None) == -1 and loaded.vva_place_masks(a, a, 2, 8, 8, 0, 0, 1 << 16, 1 << 15, a, a, None) == -2
    assert loaded.vva_unplace_mask(a, a, a, 2, 8, 8, 0, 0, 8, 8, a, None) == -1 and b"vva_unplace_mask" in loaded.vva_last_error()      # dil_out is not dil
    assert loaded.vva_unplace_mask(a, a, a, 65536, 8, 8, 0, 0, 8, 8, a + 8, None) == -2
    with pytest.raises(ctypes.ArgumentError):
        loaded.vva_sad(a, a, 2.0, 32, 32, 1, 1, 0, 1, a, None)
    import torch
    f, z = torch.zeros((2, 32, 32, 3), dtype=torch.uint8), torch.zeros((2, 32, 32), dtype=torch.uint8)
    tr = torch.zeros((2, 8), dtype=torch.int32)
    for call in (lambda: align_hip.pyramid(f, z, 1), lambda: align_hip.place_masks(z, tr, (0, 0, 8, 8)), lambda: align_hip.unplace_mask(z[:, :8, :8], z, tr, (0, 0, 8, 8))):
        with pytest.raises(RuntimeError):
            call()                                                                                   # no CPU fallback


def test_product_sources_of_the_feature():
    """vv_align is in the one build recipe with its header among the dependencies and reads no environment; the settings import no torch; importing
    the drop-in resolves no vva_ symbol, and neither does a call's set-up without the option."""
    abiref.check_sources("vv_align", "vvalign.h", "platealign")
    code = ("import diffuerase; from videovanish_amd import align_hip, plate_hip, hip; "
            "assert align_hip.PART.dll is None and plate_hip.PART.dll is None and hip.CORE.dll is None; "
            "assert diffuerase.plate_align_config() is None and diffuerase.last_plate_align is None")
    env = {k: v for k, v in os.environ.items() if k not in ("VV_PLATE_FILL", "VV_PLATE_ALIGN")}
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)


# ---- the reference against the ground truth: a failure here means the rule is wrong, not the kernel -----------------------------------------
@pytest.fixture(scope="module")
def pans():
    return {(kind, seed): A.pan_clip(seed=seed, kind=kind) for kind in ("iid", "smooth") for seed in (0, 1)}


@pytest.mark.parametrize("kind", ["iid", "smooth"])
@pytest.mark.parametrize("seed", [0, 1])
def test_reference_recovers_the_offsets_of_a_synthetic_pan(pans, kind, seed):
    """T = 12 at 96 x 128, steps of 2 .. 5 px in x and -2 .. 2 in y, noise of +-3, a crossing box: every frame's offset is the true one."""
    frames, masks, off, clean, boxm, logom = pans[kind, seed]
    assert np.abs(np.diff(off[:, 0])).min() >= 2 and boxm.any(axis=(1, 2)).sum() >= 10
    for levels in (3, 4):
        track = A.track_segment(frames, masks, levels=levels)
        assert (track[:, :2] == off).all(), (track[:, :2].tolist(), off.tolist())
        assert (track[:, 3] == 1).all() and (track[:, 7] == 0).all() and (track[1:, 6] > 0.25 * 96 * 128).all()
        sad = track[:, 4].astype(np.int64) % (1 << 32) + (track[:, 5].astype(np.int64) << 32)
        assert (sad[1:] <= 3 * track[1:, 6]).all()                           # a mean |difference| within the noise bound: |n1 - n2| <= 6, mean below 3


def test_reference_grey_clip_exercises_the_tie_order():
    """Every candidate of a constant clip costs 0: the centre wins (the smallest distance), so every offset is zero."""
    frames = np.full((6, 40, 56, 3), 128, np.uint8)
    masks = np.zeros((6, 40, 56), np.uint8)
    masks[:, 10:20, 10:30] = 255
    track = A.track_segment(frames, masks)
    assert not track[:, :2].any() and (track[:, 3] == 1).all() and not track[:, 4:6].any() and not track[:, 2].any()
    # the order itself: equal cost -> nearer the centre, then the smaller dy, then the smaller dx
    t2 = np.zeros((2, 8), np.int32)
    t2[0, 3], t2[1] = 1, [3, -2, 0, A.IN_PROGRESS, 0, 0, 0, 0]
    acc = np.zeros((9, 2), np.int64)
    acc[:, 1] = 2000
    acc[4] = (5, 2000)                                                      # the centre is worse than its eight neighbours
    A.pick_level(acc, t2, 40, 56, 1, 1, 0, 1, 25, 12)
    assert t2[1].tolist() == [3, -3, 0, 1, 0, 0, 2000, 0]                      # distance 1: (0, -1) before (-1, 0), (1, 0), (0, 1)
    t2[1] = [3, -2, 0, A.IN_PROGRESS, 0, 0, 0, 0]
    acc[:, 0] = 7
    acc[[0, 2], 0] = 0
    acc[2, 1] = 1000                                                        # 0 / 1000 == 0 / 2000: equal, both at distance 2, dy equal: the smaller dx
    A.pick_level(acc, t2, 40, 56, 1, 1, 0, 1, 25, 12)
    assert t2[1].tolist() == [2, -3, 0, 1, 0, 0, 2000, 0]
    t2[1] = [3, -2, 0, A.IN_PROGRESS, 0, 0, 0, 0]
    acc[:, 1] = 559                                                         # 100 * 559 < 25 * 40 * 56: nothing is eligible
    A.pick_level(acc, t2, 40, 56, 1, 1, 0, 1, 25, 12)
    assert t2[1].tolist() == [0, 0, 0, 0, 0, 0, 0, 0]


def test_reference_loses_a_noise_frame_and_recovers(pans):
    frames, masks, off, clean, boxm, logom = pans["iid", 0]
    frames = frames.copy()
    frames[5] = np.random.default_rng(5).integers(0, 256, frames[5].shape)
    track = A.track_segment(frames, masks)
    assert track[:, 3].tolist() == [1] * 5 + [0] + [1] * 6
    ok = track[:, 3] == 1
    assert (track[ok, :2] == off[ok]).all() and (track[5, :2] == off[4]).all()      # the lost frame keeps the last tracked offset, for the record
    out, dil, counts, info = A.fill_segment(frames, masks)
    assert info["path"] == "canvas" and (dil[5] == masks[5]).all() and counts[5].tolist() == [0, int((masks[5] != 0).sum())]
    assert (out[5] == frames[5]).all()


def test_reference_changes_the_key_beyond_a_quarter_of_the_width():
    frames, masks, off, clean, boxm, logom = A.pan_clip(T=12, H=64, W=96, seed=2, steps_x=(5, 5), steps_y=(0, 0), box=(20, 18), box_speed=7)
    track = A.track_segment(frames, masks)
    assert (track[:, :2] == off).all() and (track[:, 3] == 1).all()
    assert track[:, 2].tolist() == [0, 0, 0, 0, 0, 0, 5, 5, 5, 5, 5, 10]              # 4 * 25 > 96 at frame 5, again 25 px later


# ---- the stage: the reference on the clip the unaligned stage cannot fill -------------------------------------------------------------------
def test_reference_fills_the_box_over_a_noise_free_pan():
    for (H, W), logo in (((40, 56), None), ((45, 83), None), ((96, 132), None), ((40, 56), (28, 20, 34, 26))):
        frames, masks, off, clean, boxm, logom = A.stage_clip(H, W, logo)
        T = len(frames)
        assert (off[:, 0] == 3 * np.arange(T)).all() and not off[:, 1].any() and (clean[masks == 0] == frames[masks == 0]).all()
        out, dil, counts = R.plate_fill(frames, masks)
        assert (out == frames).all() and (dil == masks).all() and not counts[:, 0].any()              # the unaligned stage: nothing, as pinned
        out, dil, counts, infos = A.plate_fill(frames, masks)
        assert infos[0]["path"] == "canvas" and (infos[0]["track"][:, :2] == off).all() and (infos[0]["track"][:, 3] == 1).all()
        assert not dil[boxm].any() and (out[boxm] == clean[boxm]).all()                               # every box pixel: the bytes of the clean pan
        assert (out[masks == 0] == frames[masks == 0]).all() and (counts.sum(1) == (masks != 0).reshape(T, -1).sum(1)).all()
        got = (masks != 0) & (dil == 0)
        assert (out[got] == clean[got]).all() and (out[dil != 0] == frames[dil != 0]).all()
        if logo is None:
            assert not dil.any() and counts[:, 0].sum() == boxm.sum() > 1500
        else:
            assert got[:, logom].sum() > 0.9 * logom.sum() * T                                        # other frames of the pan reveal what the logo hides


# ---- orchestration ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def host_align(host_kernels, monkeypatch):
    """host_kernels plus the functions of align_hip replaced by the reference on host tensors."""
    import torch
    from videovanish_amd import align_hip
    infill, calls, t = host_kernels
    held = {}

    def frame_bytes(H, W, L):
        return sum(2 * (H >> l) * (W >> l) for l in range(L + 1))

    def pyramid(f, d, L, out=None):
        calls.append(("pyramid", tuple(f.shape), L))
        out[:] = t(A.pack(A.pyramid(f.numpy(), d.numpy(), L)))
        held.setdefault("frames", []).append((f.numpy().copy(), d.numpy().copy()))
        return out

    def track(pyr, H, W, L, radius, min_overlap, max_residual):
        calls.append(("track", tuple(pyr.shape), L, radius, min_overlap, max_residual))
        f = np.concatenate([a for a, _ in held["frames"]])
        d = np.concatenate([b for _, b in held.pop("frames")])
        assert (A.pack(A.pyramid(f, d, L)) == pyr.numpy()).all()
        return t(A.track_segment(f, d, levels=L, radius=radius, min_overlap=min_overlap, max_residual=max_residual))

    def place_masks(d, tr, box):
        calls.append(("place", tuple(box)))
        return tuple(t(a) for a in A.place_masks(d.numpy(), tr.numpy(), box))

    def unplace_mask(dc, d, tr, box):
        calls.append(("unplace", tuple(box)))
        return t(A.unplace_mask(dc.numpy(), d.numpy(), tr.numpy(), box))

    for name, fn in (("frame_bytes", frame_bytes), ("pyramid", pyramid), ("track", track), ("place_masks", place_masks), ("unplace_mask", unplace_mask)):
        monkeypatch.setattr(align_hip, name, fn)
    return infill, calls, t


def _run_stage(infill, t, frames, masks, pcfg=PlateFillConfig(), acfg=PlateAlignConfig(), cuts=None):
    flist = [f.copy() for f in frames]
    d, got = t(masks), []
    out, dil, rep = infill.plate_fill(flist, d, pcfg, cuts, acfg=acfg, align_out=got)
    assert all((a == b).all() for a, b in zip(flist, frames)) and (d.numpy() == masks).all()          # the caller's arrays are never written
    assert len(got) == 1
    return flist, d, out, dil, rep, got[0]


def test_plate_fill_aligned_canvas_copy_on_write_and_reports(host_align):
    infill, calls, t = host_align
    frames, masks, off, clean, boxm, logom = A.stage_clip(logo=(28, 20, 34, 26))
    T = len(frames)
    for cuts in (None, [7]):
        del calls[:]
        flist, d, out, dil, rep, arep = _run_stage(infill, t, frames, masks, cuts=cuts)
        want, wd, wc, infos = A.plate_fill(frames, masks, cuts=cuts)
        assert (np.stack(out) == want).all() and (dil.numpy() == wd).all() and dil is not d
        assert (rep.filled == wc[:, 0]).all() and (rep.left == wc[:, 1]).all() and rep.filled.sum() > (0.9 * boxm.sum() if cuts is None else 0)
        assert rep.skipped == (False,) * len(rep.segments) and all(s > 0 for s in rep.steady)
        assert arep.path == ("canvas",) * len(rep.segments) and arep.segments == rep.segments
        for k, info in enumerate(infos):
            assert (arep.off[k] == info["track"][:, :2]).all() and (arep.key[k] == info["track"][:, 2]).all() and arep.tracked[k].all()
            assert arep.box[k] == info["box"] and arep.box[k][1] % 4 == 0 and arep.box[k][3] % 4 == 0 and (arep.residual[k] == 0).all()
        assert (np.concatenate(arep.off)[:, 0] == 3 * (np.arange(T) - np.repeat([s for s, e in rep.segments], [e - s for s, e in rep.segments]))).all()
        for i in range(T):
            assert (out[i] is flist[i]) == (wc[i, 0] == 0), i
        # the logo is screen-fixed: on the canvas it moves, and frames further along the pan reveal what it hides
        assert cuts is not None or rep.left.sum() < logom.sum() * T
        want_calls = sum((["track", "place"] + ["unplace"] * bool(rep.filled[s:e].any()) for s, e in rep.segments), [])      # nothing filled: no mask comes back
        assert [c[0] for c in calls if c[0] in ("track", "place", "unplace")] == want_calls and want_calls[:3] == ["track", "place", "unplace"]
    # the tracker's frames cross in batches that respect max_bytes; the canvas itself fits
    del calls[:]
    flist, d, out, dil, rep, arep = _run_stage(infill, t, frames, masks, pcfg=PlateFillConfig(max_bytes=5 * 40 * 56 * 3 + 100))
    assert [c[1][0] for c in calls if c[0] == "pyramid"] == [5, 5, 2] and arep.path == ("fallback",) and not rep.filled.any()
    assert dil is d and all(a is b for a, b in zip(out, flist)) and rep.skipped == (True,)             # the unaligned stage's own limit holds too


def test_plate_fill_aligned_static_fallback_and_untracked(host_align):
    infill, calls, t = host_align
    # a locked-off clip: every offset is zero and the unaligned stage runs as it is
    frames, masks, clean, boxm, logom = R.locked_off_clip()
    flist, d, out, dil, rep, arep = _run_stage(infill, t, frames, masks)
    base = infill.plate_fill(flist, d, PlateFillConfig(), None)
    assert arep.path == ("static",) and not arep.off[0].any() and arep.tracked[0].all() and arep.box == (None,)
    assert (np.stack(out) == np.stack(base[0])).all() and (dil.numpy() == base[1].numpy()).all()
    assert all((a == b).all() if isinstance(a, np.ndarray) else a == b for a, b in zip(rep, base[2]))
    assert not [c for c in calls if c[0] in ("place", "unplace")]
    # a canvas over max_bytes falls back to the unaligned stage and is flagged
    frames, masks, off, clean, boxm, logom = A.stage_clip()
    want, wd, wc, infos = A.plate_fill(frames, masks)
    box = infos[0]["box"]
    full = 12 * (box[2] - box[0]) * (box[3] - box[1]) * 3
    assert full < 12 * 15 * 56 * 3                                                                     # smaller than the unaligned crop: that one is skipped as well
    flist, d, out, dil, rep, arep = _run_stage(infill, t, frames, masks, pcfg=PlateFillConfig(max_bytes=full - 1))
    assert arep.path == ("fallback",) and arep.box == (box,) and rep.skipped == (True,) and not rep.filled.any() and dil is d
    flist, d, out, dil, rep, arep = _run_stage(infill, t, frames, masks, pcfg=PlateFillConfig(max_bytes=full))
    assert arep.path == ("canvas",) and (np.stack(out) == want).all() and rep.filled.sum() == boxm.sum()
    # an untracked frame counts wholly as left and keeps its bytes and mask; no mask at all: nothing is tracked
    frames = frames.copy()
    frames[7][masks[7] == 0] = np.random.default_rng(7).integers(0, 256, frames[7].shape)[masks[7] == 0]
    want, wd, wc, infos = A.plate_fill(frames, masks)
    flist, d, out, dil, rep, arep = _run_stage(infill, t, frames, masks)
    assert arep.tracked[0].tolist() == [t_ != 7 for t_ in range(12)] and out[7] is flist[7] and (dil.numpy()[7] == masks[7]).all()
    assert (np.stack(out) == want).all() and (dil.numpy() == wd).all() and (rep.left == wc[:, 1]).all() and rep.left[7] == (masks[7] != 0).sum()
    del calls[:]
    flist, d, out, dil, rep, arep = _run_stage(infill, t, frames, np.zeros_like(masks))
    assert arep.path == ("empty",) and dil is d and not [c for c in calls if c[0] in ("pyramid", "track")]


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_precedence_and_plate_align_needs_plate_fill(monkeypatch):
    import inspect

    import diffuerase
    monkeypatch.delenv("VV_PLATE_ALIGN", raising=False)
    monkeypatch.delenv("VV_PLATE_FILL", raising=False)
    try:
        diffuerase.configure()
        assert diffuerase.plate_align_config() is None
        monkeypatch.setenv("VV_PLATE_ALIGN", "radius=6")
        assert diffuerase.plate_align_config() == PlateAlignConfig(radius=6)
        diffuerase.configure(plate_align="levels=2")
        assert diffuerase.plate_align_config() == PlateAlignConfig(levels=2) and diffuerase.plate_align_config("on") == PlateAlignConfig()
        assert diffuerase.plate_align_config("off") is None
        diffuerase.configure(plate_align="off")
        assert diffuerase.plate_align_config() is None                                                     # configure("off") beats the environment
        diffuerase.configure()
        assert diffuerase.plate_align_config() == PlateAlignConfig(radius=6)
        with pytest.raises(ValueError):
            diffuerase.configure(plate_align="sometimes")
        f = [np.zeros((8, 8, 3), np.uint8)] * 2
        for kw in (dict(plate_align="on"), dict(plate_align="on", plate_fill="off"), dict()):             # the last: from the environment
            with pytest.raises(ValueError, match="plate_align="):
                diffuerase.run_infill_on_frames(f, f, **kw)
        assert diffuerase.last_plate_align is None
    finally:
        diffuerase.configure()
    for fn in (diffuerase.run_infill_on_frames, diffuerase.configure):
        p = inspect.signature(fn).parameters["plate_align"]
        assert p.default is None and (fn is diffuerase.configure or p.kind is inspect.Parameter.KEYWORD_ONLY)


def test_cli_plate_align_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
    import diffuerase
    from videovanish_amd import infill
    calls = []
    videos = {"mask.mkv": [np.zeros((16, 24, 3), np.uint8)] * 3}
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda path, start=0, max_frames=-1: ([f.copy() for f in videos[path]], 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    off = np.array([[0, 0], [7, -1], [7, -1]], np.int32)

    def fake(frames, masks, **kw):
        calls.append(kw)
        diffuerase.last_plate_align = infill.PlateAlignReport((off,), (np.zeros(3, np.int32),), (np.array([True, True, False]),), (np.zeros(3),),
                                                              ((0, 0, 8, 8),), ("canvas",), ((0, 3),)) if "plate_align" in kw else None
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    monkeypatch.setattr(diffuerase, "last_plate_fill", None)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 3
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    for value in ("on", "radius=8,levels=3"):
        monkeypatch.setattr(sys, "argv", argv + ["--plate-fill", "on", "--plate-align", value])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "plate_fill": "on", "plate_align": value}
        out = capsys.readouterr().out
        assert out == "plate align: 2 of 3 frames tracked, pan extent 7 x 1 px, 1 of 1 segments filled on a canvas\n"
    for bad in ("off", "yes", "radius=9"):
        monkeypatch.setattr(sys, "argv", argv + ["--plate-fill", "on", "--plate-align", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_plate_align", None)
