"""Clean-plate exposure matching on the GPU: the four kernels of vv_platetone.hip and the whole stage against the restatement of
include/platetone.h (tests/platetone_ref.py) byte for byte, every kernel run twice with identical bytes: both forms (4-pixel and byte) at their
width and alignment edges, T = 1 and the u32 bound of the mean's sum, the strided grid of the moments, the floor gate, clamping tables, an
identity frame between two others, refusals; infill.plate_fill(tcfg=) on the shared clips; and the drop-in's plate_tone= path against the same
call handed the restatement's frames and masks.  Tiny architecture."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import platefill_ref as R  # noqa: E402
import platetone_ref as E  # noqa: E402

from videovanish_amd import platetone as PT  # noqa: E402
from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.platefill import PlateFillConfig  # noqa: E402
from videovanish_amd.plategrain import PlateGrainConfig  # noqa: E402
from videovanish_amd.platetone import PlateToneConfig  # noqa: E402
from videovanish_amd.roi import RoiConfig  # noqa: E402
from videovanish_amd.spans import SpanConfig  # noqa: E402


def _d(a, gpu, shift=0):
    """a on the device; shift > 0: at a base that many bytes past an aligned one (contiguous all the same)."""
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if not shift:
        return torch.from_numpy(a).to(gpu)
    raw = torch.empty(a.nbytes + 8, dtype=torch.uint8, device=gpu)
    view = raw[shift:shift + a.nbytes].view(torch.from_numpy(a).dtype if a.dtype != np.uint8 else torch.uint8).view(a.shape)
    view.copy_(torch.from_numpy(a).to(gpu))
    assert view.data_ptr() % 4 == shift % 4 and view.is_contiguous()
    return view


def _twice(fn):
    """fn() -> tensors; run twice, identical bytes; the first run's results as numpy arrays."""
    a, b = fn(), fn()
    a, b = [x.cpu().numpy() for x in a], [x.cpu().numpy() for x in b]
    assert all((x == y).all() for x, y in zip(a, b))
    return a


def _tabs(raw, T):
    return np.frombuffer(raw, np.uint8).reshape(T, 3, 256).copy()


def _stage(frames, dil, gpu, tone=None, grain=None, **pcfg):
    """One cropped segment through mean_plane, moments, the host fit, apply, the fill and restore: every output against the restatement."""
    from videovanish_amd import infill, platetone_bind as B
    tone = dict(E.DEFAULTS, **(tone or {}))
    tcfg, pc = PlateToneConfig(**tone), PlateFillConfig(**pcfg)
    want, wd, wc, info = E.segment(frames, dil, tone, None if grain is None else (grain.depth, grain.reach), **pcfg)
    T = len(frames)
    f, d = _d(frames, gpu), _d(dil, gpu)
    ns = infill._not_sample(d, pc)
    mean, sup, n = _twice(lambda: B.mean_plane(f, ns, tcfg.floor))
    assert (mean == info["R"]).all() and (sup == info["U"]).all() and sup.max() <= 1 and int(n[0]) == info["n"]
    if info["path"] == "unfit":
        return info
    sums, = _twice(lambda: (B.moments(f, _d(mean, gpu), _d(sup, gpu)),))
    assert sums.tolist() == info["sums"]
    fit = PT.fit_segment(int(n[0]), sums, tcfg)
    assert (_tabs(fit.fwd, T) == info["G"]).all() and (_tabs(fit.back, T) == info["B"]).all() and list(fit.identity) == info["identity"].tolist()
    if info["path"] == "identity":
        return info
    ident = _d(np.frombuffer(fit.identity, np.uint8), gpu)
    f1, = _twice(lambda: (B.apply(f, _d(info["G"], gpu), ident),))
    assert (f1 == info["normalised"]).all()
    g = _d(f1, gpu)
    d2, c, steady = infill._fill_device(g, d, None, pc, grain, ns)
    out, = _twice(lambda: (B.restore(f, g, d, d2, _d(info["B"], gpu)),))
    assert (d2.cpu().numpy() == wd).all() and (c[:, :2] == wc).all() and (out == want).all()
    assert (f.cpu().numpy() == frames).all()                                                           # the original crop stays as it is
    return info


# ---- the kernels and the stage on the shared clips ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["drift", "flicker", "both", "still"])
def test_stage_on_the_shared_clips(gpu, kind):
    kw = dict(drift=dict(drift_q4=4), flicker=dict(flicker_pct=8), both=dict(drift_q4=4, flicker_pct=8), still=dict(a=0))[kind]
    frames, masks, clean, boxm, logom = E.exposure_clip(seed=1, **kw)                                   # 24 x 40 x 56
    info = _stage(frames, masks, gpu)
    assert info["path"] == ("identity" if kind == "still" else "matched") and info["n"] > 1024
    if kind == "both":
        _stage(frames, masks, gpu, tone=dict(mode="gain", floor=60, max_gain=5, max_offset=3), guard=0, margin=0)
        _stage(frames, masks, gpu, tone=dict(mode="offset"), grain=PlateGrainConfig(depth=3, reach=4))
        assert _stage(frames, masks, gpu, tone=dict(min_pixels=info["n"] + 1))["path"] == "unfit"
        _stage(frames[:, :, :55], masks[:, :, :55], gpu, tone=dict(min_pixels=256))                     # the byte form


@pytest.mark.parametrize("cuts", [None, [9, 15]])
def test_plate_fill_with_tone_on_the_crop(gpu, cuts):
    from videovanish_amd import infill
    frames, masks, clean, boxm, logom = E.exposure_clip(seed=3, drift_q4=4, flicker_pct=8)
    flist = [f.copy() for f in frames]
    d = _d(masks, gpu)
    for tkw, gcfg in ((dict(min_pixels=256), None), (dict(min_pixels=256, ring=8), PlateGrainConfig(depth=3, reach=4))):
        got, more = [], {} if gcfg is None else dict(gcfg=gcfg, grain_out=[])
        out, dil, rep = infill.plate_fill(flist, d, PlateFillConfig(), cuts, tcfg=PlateToneConfig(**tkw), tone_out=got, **more)
        want, wd, wc, infos = E.plate_fill(frames, masks, cuts, tone=tkw, grain=None if gcfg is None else (gcfg.depth, gcfg.reach))
        assert (np.stack(out) == want).all() and (dil.cpu().numpy() == wd).all() and (rep.filled == wc[:, 0]).all() and (rep.left == wc[:, 1]).all()
        assert got[0].path == tuple(i["path"] for i in infos) == ("matched",) * len(infos) and got[0].n == tuple(i["n"] for i in infos)
        assert got[0].identity.tolist() == np.concatenate([i["identity"] for i in infos]).tolist() and rep.filled.sum() > 100
        assert all((out[i] is flist[i]) == (wc[i, 0] == 0) for i in range(24))
        assert all((a == b).all() for a, b in zip(flist, frames)) and (d.cpu().numpy() == masks).all()      # the caller's arrays are never written
    plain = infill.plate_fill(flist, d, PlateFillConfig(), cuts)
    assert (plain[1].cpu().numpy() != dil.cpu().numpy()).any()                                         # the option fills what the plain call cannot
    # no drift, no grain: identity, the plain call's bytes and objects
    still, sm, _, _, _ = E.exposure_clip(seed=3, a=0)
    slist, sd, got = list(still), _d(sm, gpu), []
    out, dil, rep = infill.plate_fill(slist, sd, PlateFillConfig(), cuts, tcfg=PlateToneConfig(min_pixels=256), tone_out=got)
    base, bd, brep = infill.plate_fill(slist, sd, PlateFillConfig(), cuts)
    assert set(got[0].path) == {"identity"} and got[0].identity.all() and (np.stack(out) == np.stack(base)).all() and (dil == bd).all()
    assert [(o is f) for o, f in zip(out, slist)] == [(o is f) for o, f in zip(base, slist)] and rep.filled.sum() > 100


# ---- both forms at their edges --------------------------------------------------------------------------------------------------------------
def _edge_tables():
    """Three frames: tables that clamp at 0 and at 255 (gain 2 and offset -40, gain 1/2 and offset +40), an identity frame between them."""
    n, Sr, Srr = 4, 100, 3000
    rows = []
    for a_num, a_den, b in ((2, 1, -40), (1, 1, 0), (1, 2, 40)):
        v = [a_num * r // a_den + b for r in (10, 20, 30, 40)]
        rows.append([sum(v)] * 3 + [sum(x * r for x, r in zip(v, (10, 20, 30, 40)))] * 3 + [Sr] * 3 + [Srr] * 3)
    fit = PT.fit_segment(n, rows, PlateToneConfig(min_pixels=1, max_gain=100, max_offset=255))
    Gt, Bt, ident, _, _ = E.fit_tables(n, rows, min_pixels=1, max_gain=100, max_offset=255)
    assert (_tabs(fit.fwd, 3) == Gt).all() and (_tabs(fit.back, 3) == Bt).all() and ident.tolist() == [False, True, False] == [bool(x) for x in fit.identity]
    assert Gt[0, 0, 255] == 148 and Bt[0, 0, 148:].min() == 255 and Bt[0, 0, :21].max() == 0 and Gt[2, 0, :41].max() == 0 and Gt[2, 0, 168:].min() == 255
    return Gt, Bt, ident


@pytest.mark.parametrize("W,shift", [(1, 0), (3, 0), (4, 0), (5, 0), (4, 1), (8, 2), (8, 0)])
def test_mean_apply_restore_at_the_width_and_alignment_edges(gpu, W, shift):
    from videovanish_amd import platetone_bind as B
    rng = np.random.default_rng(100 * W + shift)
    T, H = 3, 5
    frames = rng.integers(0, 256, (T, H, W, 3)).astype(np.uint8)
    frames[:, 0, 0] = (16, 15, 240)                                                                     # the gate: equality in, one step past out
    frames[:, 1, 0] = (16, 239, 128)
    ns = (rng.random((T, H, W)) < 0.1).astype(np.uint8) * 255
    ns[:, :2, 0] = 0
    dil = (rng.random((T, H, W)) < 0.5).astype(np.uint8) * 255
    dil2 = dil * (rng.random((T, H, W)) < 0.5).astype(np.uint8)
    filled = rng.integers(0, 256, (T, H, W, 3)).astype(np.uint8)
    Gt, Bt, ident = _edge_tables()
    f, g = _d(frames, gpu, shift), _d(filled, gpu, shift)
    mean, sup, n = _twice(lambda: B.mean_plane(f, _d(ns, gpu, shift), 16))
    Rm, U, wn = E.mean_plane(frames, ns != 0, 16)
    assert (mean == Rm).all() and (sup == U).all() and int(n[0]) == wn and not sup[0, 0] and sup[1, 0]
    sums, = _twice(lambda: (B.moments(f, _d(mean, gpu, shift), _d(sup, gpu, shift)),))
    assert sums.tolist() == E.moments(frames, Rm, U)
    flags = _d(ident.astype(np.uint8), gpu)
    out, = _twice(lambda: (B.apply(f, _d(Gt, gpu), flags),))
    assert (out == E.lut(frames, Gt)).all() and (out[1] == frames[1]).all() and (out[0] != frames[0]).any()
    away = _d(np.zeros_like(frames), gpu, shift)
    assert B.apply(f, _d(Gt, gpu), flags, out=away) is away and (away.cpu().numpy() == out).all()
    back, = _twice(lambda: (B.restore(f, g, _d(dil, gpu, shift), _d(dil2, gpu, shift), _d(Bt, gpu)),))
    went = (dil != 0) & (dil2 == 0)
    want = frames.copy()
    want[went] = E.lut(filled, Bt)[went]
    assert (back == want).all() and went.any() and (back[~went] == frames[~went]).all()


def test_one_frame_and_the_longest_segment(gpu):
    from videovanish_amd import platetone_bind as B
    rng = np.random.default_rng(5)
    one = rng.integers(16, 240, (1, 6, 8, 3)).astype(np.uint8)                                          # T = 1: the mean is the frame
    z = np.zeros((1, 6, 8), np.uint8)
    mean, sup, n = _twice(lambda: B.mean_plane(_d(one, gpu), _d(z, gpu), 16))
    assert (mean == one[0]).all() and sup.all() and int(n[0]) == 48
    sums, = _twice(lambda: (B.moments(_d(one, gpu), _d(mean, gpu), _d(sup, gpu)),))
    assert sums.tolist() == E.moments(one, one[0], sup != 0) and PT.fit_segment(48, sums, PlateToneConfig(min_pixels=1)).all_identity
    T = 65535                                                                                           # P = 65535 * 255: the u32 bound of rule 2
    f = torch.full((T, 1, 4, 3), 255, dtype=torch.uint8, device=gpu)
    ns = torch.zeros((T, 1, 4), dtype=torch.uint8, device=gpu)
    mean, sup, n = _twice(lambda: B.mean_plane(f, ns, 0))
    assert (mean == 255).all() and sup.all() and int(n[0]) == 4
    sums, = _twice(lambda: (B.moments(f, _d(mean, gpu), _d(sup, gpu)),))
    assert (sums[:, :3] == 4 * 255).all() and (sums[:, 3:6] == 4 * 255 * 255).all() and sums[0, 6:].tolist() == [4 * 255] * 3 + [4 * 255 * 255] * 3
    assert not sums[1:, 6:].any()
    f[T // 2 + 1:, 0, 1, 2] = 254                                                                       # 32767 frames at 254: 254.5 and a bit, rounds up; one more: down
    assert B.mean_plane(f, ns, 0)[0][0, 1, 2].item() == 255
    f[T // 2, 0, 1, 2] = 254
    assert B.mean_plane(f, ns, 0)[0][0, 1, 2].item() == 254
    assert B.mean_plane(f, ns, 1)[2].item() == 0                                                        # 255 > 255 - 1: the gate


@pytest.mark.parametrize("T,H,W", [(2, 32, 64), (3, 40, 56), (24, 210, 211), (520, 96, 96)],
                         ids=["two-full-blocks", "partial-last-block", "strided-byte-form", "strided-4-pixel-form"])
def test_moments_over_blocks_and_strides(gpu, T, H, W):
    from videovanish_amd import platetone_bind as B
    rng = np.random.default_rng(T + H)
    frames = rng.integers(0, 256, (T, H, W, 3)).astype(np.uint8)
    Rm = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    U = rng.random((H, W)) < 0.7
    U[-1, -5:] = True                                                                                   # the last unit counts
    sums, = _twice(lambda: (B.moments(_d(frames, gpu), _d(Rm, gpu), _d(U.astype(np.uint8), gpu)),))
    v, r = frames.astype(np.int64)[:, U], Rm.astype(np.int64)[U]
    assert (sums[:, :3] == v.sum(1)).all() and (sums[:, 3:6] == (v * r).sum(1)).all()
    assert (sums[0, 6:9] == r.sum(0)).all() and (sums[0, 9:] == (r * r).sum(0)).all() and not sums[1:, 6:].any()


def test_refusals_launch_nothing(gpu):
    from videovanish_amd import platetone_bind as B
    lib = B.lib()
    f = torch.full((2, 8, 8, 3), 7, dtype=torch.uint8, device=gpu)
    g = torch.full((2, 8, 8, 3), 7, dtype=torch.uint8, device=gpu)
    o = torch.full((2, 8, 8, 3), 7, dtype=torch.uint8, device=gpu)
    m = torch.full((2, 8, 8), 7, dtype=torch.uint8, device=gpu)
    tab = torch.full((2, 3, 256), 7, dtype=torch.uint8, device=gpu)
    s = torch.full((2, 12), 7, dtype=torch.int64, device=gpu)
    p = lambda t: t.data_ptr()
    mean = lambda T=2, H=8, W=8, floor=16, n=p(s): lib.vve_mean_plane(p(f), p(m), T, H, W, floor, p(o), p(m), n, None)
    mom = lambda T=2, H=8, W=8, out=p(s): lib.vve_moments(p(f), p(g), p(m), T, H, W, out, None)
    app = lambda T=2, H=8, W=8, out=p(o), t=p(tab): lib.vve_apply(p(f), t, p(m), T, H, W, out, None)
    res = lambda T=2, H=8, W=8, out=p(o), t=p(tab): lib.vve_restore(p(f), p(g), p(m), p(m), t, T, H, W, out, None)
    bad = [fn(**kw) for fn in (mean, mom, app, res) for kw in (dict(T=0), dict(H=0), dict(W=-1))]
    bad += [mean(floor=-1), mean(n=None), mom(out=None), app(out=None), app(out=p(f)), res(out=p(f)), res(out=p(g)), app(t=p(tab) + 2), res(t=None)]
    assert bad == [-1] * len(bad)
    assert app(out=p(f)) == -1 and lib.vve_last_error().startswith(b"vve_apply:") and b"out is not frames" in lib.vve_last_error()
    unsupported = [fn(**kw) for fn in (mean, mom, app, res) for kw in (dict(T=65536), dict(H=4096, W=4097))] + [mean(floor=128)]
    assert unsupported == [-2] * len(unsupported) and lib.vve_last_error().startswith(b"vve_mean_plane:")
    torch.cuda.synchronize()
    assert all((x == 7).all() for x in (f, g, o, m, tab, s))                                           # nothing was launched, nothing cleared
    with pytest.raises(RuntimeError, match="out must be"):
        B.apply(f, tab, m[:, 0, 0].contiguous(), out=f)
    with pytest.raises(RuntimeError, match="floor <= 127"):
        B.mean_plane(f, m, 128)
    with pytest.raises(RuntimeError):
        B.mean_plane(f.cpu(), m.cpu(), 16)                                                              # no CPU fallback
    with pytest.raises(ctypes.ArgumentError):
        mean(floor=2.0)


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=960, num_inference_steps=2, scheduler="ddim")
T, H, W = 14, 96, 160
SPANS = SpanConfig("masked", context=1, min_len=3, min_gap=2)
ROI = RoiConfig("follow", context=0.25, pad_min=8, min_side=32)
SCREEN = (64, 96, 88, 136)        # a screen-fixed region that shows something else in every frame: never steady
LOGO = (70, 104, 80, 124)         # a mask on it in frames 4 .. 8


def _finish(frames, masks, screen=True):
    frames, masks = frames.copy(), masks.copy()
    y0, x0, y1, x1 = SCREEN
    frames[:, y0:y1, x0:x1] = np.random.default_rng(77).integers(0, 256, (T, y1 - y0, x1 - x0, 3)) if screen else 128
    masks[4:9, LOGO[0]:LOGO[2], LOGO[1]:LOGO[3]] = 255
    m3 = [np.repeat(m[..., None], 3, axis=2) for m in masks]
    prior = []
    for f, m in zip(frames, masks):
        p = f.copy()
        p[m > 0] = f.reshape(-1, 3).mean(0).astype(np.uint8)
        prior.append(p)
    return list(frames), m3, prior


@pytest.fixture(scope="module")
def drift_clip():
    frames, masks, clean, boxm, _ = E.exposure_clip(T=T, H=H, W=W, a=3, seed=5, speed=12, box=(22, 24), box_y=20, logo=None, drift_q4=8, flicker_pct=8)
    return _finish(frames, masks)


def _run(frames, masks, prior, **kw):
    import diffuerase
    diffuerase.configure(RUN)
    try:
        out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, feather_px=3, **KW, **kw)
        return out, diffuerase.last_plate_fill, diffuerase.last_plate_tone
    finally:
        diffuerase.configure(None)


def _same(a, b):
    return len(a) == len(b) == T and (np.stack(a) == np.stack(b)).all()


def _by_hand(monkeypatch, gpu, want_f, want_d, frames):
    """infill.plate_fill replaced by a stand-in that hands over the restatement's frames and masks."""
    from videovanish_amd import infill
    empty = infill.PlateFillReport(np.zeros(T, np.int64), np.zeros(T, np.int64), (0,), (False,), ((0, T),), ())

    def stand_in(f, d, cfg, cuts=None, **more):
        for key in ("tone_out", "grain_out"):
            if key in more:
                more[key].append("by hand")
        return [want_f[i] if (want_f[i] != frames[i]).any() else frames[i] for i in range(T)], _d(want_d, gpu), empty
    monkeypatch.setattr(infill, "plate_fill", stand_in)


@pytest.mark.parametrize("more", [{}, dict(plate_grain="on"), dict(spans=SPANS, roi=ROI)], ids=["plain", "grain", "spans-roi"])
def test_drop_in_equals_the_call_on_the_restatement(gpu, drift_clip, monkeypatch, more):
    from videovanish_amd import hip
    frames, masks, prior = drift_clip
    dil = hip.mask_collapse_dilate(_d(np.stack(masks), gpu), KW["mask_dilation_iter"]).cpu().numpy()
    want_f, want_d, want_c, (info,) = E.plate_fill(np.stack(frames), dil, grain=(4, 8) if "plate_grain" in more else None)
    near = R.plate_fill(np.stack(frames), dil)
    assert info["path"] == "matched" and want_c[:, 0].sum() > 1000 + 4 * near[2][:, 0].sum()          # the plain fill gets next to nothing here
    kept = [f.copy() for f in frames]
    out, rep, trep = _run(frames, masks, prior, plate_fill="on", plate_tone="on", **more)
    assert (rep.filled == want_c[:, 0]).all() and (rep.left == want_c[:, 1]).all() and rep.skipped == (False,)
    assert trep.path == ("matched",) and trep.n == (info["n"],) and trep.identity.tolist() == info["identity"].tolist() and trep.segments == ((0, T),)
    assert all((a == b).all() for a, b in zip(frames, kept))
    _by_hand(monkeypatch, gpu, want_f, want_d, frames)
    hand, _, _ = _run(frames, masks, prior, plate_fill="on", plate_tone="on", **more)
    assert _same(out, hand)
    monkeypatch.undo()
    filled = (dil != 0) & (want_d == 0)
    assert all((out[t][filled[t]] == want_f[t][filled[t]]).all() for t in range(T))
    if not more:
        with pytest.raises(ValueError, match="plate_tone="):
            _run(frames, masks, prior, plate_tone="on")


def test_drop_in_without_drift_gives_the_bytes_of_the_call_without_the_option(gpu, monkeypatch):
    from videovanish_amd import platetone_bind
    frames, masks, clean, boxm, _ = E.exposure_clip(T=T, H=H, W=W, a=0, seed=5, speed=12, box=(22, 24), box_y=20, logo=None)
    frames, masks, prior = _finish(frames, masks, screen=False)
    out, rep, trep = _run(frames, masks, prior, plate_fill="on", plate_tone="on")
    assert trep.path == ("identity",) and trep.identity.all() and (trep.gain == 1).all() and not trep.offset.any() and rep.filled.sum() > 1000
    monkeypatch.setattr(platetone_bind.PART, "dll", None)
    alone, rep0, none = _run(frames, masks, prior, plate_fill="on")
    assert none is None and platetone_bind.PART.dll is None and _same(out, alone)                       # without the option nothing of it is resolved
    assert all((a == b).all() if isinstance(a, np.ndarray) else a == b for a, b in zip(rep0, rep))
