"""Overlay masking on the GPU: every kernel of csrc/vv_overlay.hip against the restatement (tests/overlaymask_ref.py), bit for bit; the stage
(infill.overlay_mask) on the shared clip; the drop-in call against the call handed the restatement's masks."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlaymask_ref as R  # noqa: E402

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.overlaymask import OverlayMaskConfig  # noqa: E402

pytestmark = pytest.mark.gpu
TILE_W, TILE_H = 64, 16         # VVO_TILE_W, VVO_TILE_H


def _d(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _acc(f, d, batches):
    """vvo_accumulate over the batches [(s, e)] of the resident clip into one cleared acc -> int32 [H,W,4] on the host"""
    from videovanish_amd import overlaymask_bind as B
    acc = B.new_acc(f.shape[1], f.shape[2], f.device)
    for s, e in batches:
        assert B.accumulate(f[s:e], d[s:e], acc) is acc
    return acc.cpu().numpy()


def _masks(kind, rng, T, H, W):
    if kind == "none":
        return np.zeros((T, H, W), np.uint8)
    if kind == "pixel":                                                     # every frame masked at one pixel: n = 0 there
        m = np.zeros((T, H, W), np.uint8)
        m[:, H // 2, W // 2] = 255
        return m
    return rng.choice(np.array([0, 0, 0, 1, 7, 255], np.uint8), size=(T, H, W))       # unnormalised bytes


# ---- vvo_accumulate -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 3, 4, 5, 63, 64, 65, 133])
def test_accumulate_widths_heights_batches_and_masks(gpu, W):
    """Widths either side of the 4-pixel load and of the tile, heights 1, 2 and 9, T = 1, 2 and 17 (17 frames on a one-tile frame run as three
    runs over blockIdx.z with atomics, 1 and 2 as one run with plain adds), every kind of mask; 17 frames in one call equal 8 + 9 and 1 + 16
    added into the same acc."""
    rng = np.random.default_rng(W)
    for H in (1, 2, 9):
        for T in (1, 2, 17):
            frames = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
            f = _d(frames, gpu)
            for kind in ("none", "pixel", "bytes"):
                dil = _masks(kind, rng, T, H, W)
                want = R.accumulate(frames, dil)
                d = _d(dil, gpu)
                got = _acc(f, d, [(0, T)])
                assert got.dtype == np.int32 and got.shape == (H, W, 4) and (got == want).all(), (H, T, kind, int((got != want).sum()))
                assert (_acc(f, d, [(0, T)]) == got).all()
                if kind == "pixel":
                    assert not got[H // 2, W // 2].any() and (np.delete(got[..., 0].ravel(), (H // 2) * W + W // 2) == T).all()
                if T == 17:
                    assert (_acc(f, d, [(0, 8), (8, 17)]) == want).all() and (_acc(f, d, [(0, 1), (1, 17)]) == want).all()
                assert (f.cpu().numpy() == frames).all() and (d.cpu().numpy() == dil).all()


@pytest.mark.parametrize("H, W", [(TILE_H + 1, TILE_W + 1), (2 * TILE_H + 1, 2 * TILE_W + 4), (3 * TILE_H - 1, 2 * TILE_W - 1)])
def test_accumulate_across_the_tile_edges(gpu, H, W):
    """A frame that crosses the tile's edge in both axes by one pixel, and two more with several tiles either way: the halo of a tile is its
    neighbour's pixels inside the frame and the replicated border outside."""
    rng = np.random.default_rng(H * W)
    for T in (2, 17):
        frames = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
        dil = _masks("bytes", rng, T, H, W)
        want = R.accumulate(frames, dil)
        got = _acc(_d(frames, gpu), _d(dil, gpu), [(0, T)])
        assert (got == want).all(), (T, np.argwhere((got != want).any(-1))[:8].tolist())


def test_accumulate_replicates_the_border(gpu):
    """Border rows and columns that differ from their neighbours: the gradient there is that of the frame extended by its own border, so a
    flat frame inside a bright border gives nothing on the border's outer side.  By hand at one corner, and against the restatement."""
    H, W = 7, 9
    frames = np.full((3, H, W, 3), 100, np.uint8)
    frames[:, 0], frames[:, -1], frames[:, :, 0], frames[:, :, -1] = 200, 220, 180, 240
    frames[1] = frames[1] // 2
    dil = np.zeros((3, H, W), np.uint8)
    got = _acc(_d(frames, gpu), _d(dil, gpu), [(0, 3)])
    assert (got == R.accumulate(frames, dil)).all()
    # frame 0 at (0, 0): Y = 180 there and below, 200 to the right, 100 at (1, 1): gx = (200 + 400 + 100) - 4 * 180 = -20, gy = (180 + 360 + 100) - (180 + 360 + 200) = -100
    one = _acc(_d(frames[:1], gpu), _d(dil[:1], gpu), [(0, 1)])
    assert one[0, 0].tolist() == [1, -20, -100, 120]


@pytest.mark.parametrize("pattern", ["checker", "diagonal"])
def test_accumulate_sums_at_the_32_bit_bound(gpu, pattern):
    """T = 65535 frames of 8 x 8: a 0 / 255 checker, and the diagonal split whose |gx| + |gy| = 1530 is the largest a 3 x 3 Sobel pair reaches.
    The sums equal the int64 restatement (one frame's, times T) and stay below 2^31."""
    T = 65535
    y, x = np.mgrid[0:8, 0:8]
    v = ((x + y) % 2 == 1) if pattern == "checker" else (x + y > 7)
    frame = np.repeat((v * 255).astype(np.uint8)[..., None], 3, axis=2)
    one = R.accumulate(frame[None], np.zeros((1, 8, 8), np.uint8))
    want = one * T
    assert one[..., 3].max() == (1020 if pattern == "checker" else 1530) and want.dtype == np.int64 and want.max() < 2 ** 31 and want.min() >= -2 ** 31
    f = _d(frame, gpu)[None].expand(T, 8, 8, 3).contiguous()
    d = torch.zeros((T, 8, 8), dtype=torch.uint8, device=gpu)
    got = _acc(f, d, [(0, T)])
    assert (got.astype(np.int64) == want).all() and (got[..., 0] == T).all()


# ---- vvo_classify -------------------------------------------------------------------------------------------------------------------------
def test_classify_equalities_and_counts(gpu):
    from videovanish_amd import overlaymask_bind as B
    rows = [(12, 96, 0, 96),            # A == mag * n, n == min_samples, fully coherent: an edge
            (12, 95, 0, 95),            # A == mag * n - 1: not strong
            (11, 500, 0, 500),          # n == min_samples - 1: not strong
            (12, 800, 0, 1000),         # 100 (|Sx| + |Sy|) == coh * A: an edge
            (12, 799, 0, 1000),         # one below: strong, no edge
            (12, -500, -300, 1000),     # negative sums count by magnitude
            (12, -500, 300, 1000),
            (12, 500, -299, 1000),
            (24, -2040 * 24, 0, 2040 * 24),
            (0, 0, 0, 0),               # never sampled
            (65535, 65535 * 1020, -65535 * 510, 65535 * 1530)]
    acc = np.array([[n, sx, sy, a] for n, sx, sy, a in rows], np.int32)[None]
    edge, counts = B.classify(_d(acc, gpu), 12, 8, 80)
    assert edge.cpu().numpy()[0].tolist() == [255, 0, 0, 255, 0, 255, 255, 0, 255, 0, 255] and counts.cpu().numpy().tolist() == [8, 6]
    strong, E = R.classify(acc, 12, 8, 80)
    assert strong[0].tolist() == [True, False, False] + [True] * 6 + [False, True] and ((edge.cpu().numpy() != 0) == E).all()
    # random sums over several blocks, three settings: the map and both counts
    rng = np.random.default_rng(5)
    H, W = 37, 53
    n = rng.integers(0, 25, (H, W))
    A = rng.integers(0, 40, (H, W)) * n
    acc = np.stack([n, rng.integers(-1, 2, (H, W)) * (A * rng.integers(50, 101, (H, W)) // 100), rng.integers(-1, 2, (H, W)) * (A // 5), A], -1).astype(np.int32)
    for min_samples, mag, coh in ((12, 8, 80), (1, 1, 1), (24, 20, 100)):
        edge, counts = B.classify(_d(acc, gpu), min_samples, mag, coh)
        strong, E = R.classify(acc, min_samples, mag, coh)
        e = edge.cpu().numpy()
        assert set(np.unique(e)) <= {0, 255} and ((e != 0) == E).all() and counts.cpu().numpy().tolist() == [int(strong.sum()), int(E.sum())]
    assert 0 < E.sum() < strong.sum()


# ---- vvo_component_stats / vvo_select -----------------------------------------------------------------------------------------------------
def _parts(mask, gpu, min_area, max_area_px, inside_only):
    """mask [H,W] bool through the device's labelling, vvo_component_stats and vvo_select, each against the restatement -> (out bool, boxes
    sorted by label, count)."""
    from videovanish_amd import mask_hip, overlaymask_bind as B
    lab = mask_hip.label_components(_d(mask.astype(np.uint8) * 3, gpu)[None])[0]
    want_lab = R.labels(mask)
    assert (lab.cpu().numpy() == want_lab).all()                                                        # the restatement labels as the device does
    stats = B.component_stats(lab)
    want_stats = R.component_stats(want_lab)
    assert stats.dtype == torch.int32 and (stats.cpu().numpy() == want_stats).all()
    assert (B.component_stats(lab).cpu().numpy() == want_stats).all()
    out, boxes, nboxes = B.select(lab, stats, min_area, max_area_px, inside_only)
    want_out, want_boxes = R.select(want_lab, want_stats, min_area, max_area_px, inside_only)
    o, n = out.cpu().numpy(), int(nboxes.item())
    assert set(np.unique(o)) <= {0, 255} and ((o != 0) == want_out).all() and n == len(want_boxes)
    b = boxes.cpu().numpy()[:min(n, 256)]
    b = b[np.argsort(b[:, 0], kind="stable")]
    assert (b == want_boxes[:256]).all(), (b.tolist(), want_boxes[:256].tolist())
    return o != 0, b, n


def test_select_borders_by_one_pixel(gpu):
    """Four components that reach a frame border with exactly one pixel and four that miss it by one."""
    H, W = 40, 44
    m = np.zeros((H, W), bool)
    m[0:3, 10] = m[H - 3:H, 10] = m[20, 0:3] = m[20, W - 3:W] = True                                     # touch top, bottom, left, right
    m[1:4, 20] = m[H - 4:H - 1, 20] = m[30, 1:4] = m[30, W - 4:W - 1] = True                             # miss each by one
    out, boxes, n = _parts(m, gpu, 0, 9, True)
    assert n == 4 and boxes[:, 2:].tolist() == [[20, 1, 21, 4], [1, 30, 4, 31], [W - 4, 30, W - 1, 31], [20, H - 4, 21, H - 1]] and out.sum() == 12
    assert not out[0:3, 10].any() and not out[20].any() and not out[H - 3:H, 10].any() and out[1:4, 20].all()
    out, boxes, n = _parts(m, gpu, 0, 9, False)
    assert n == 8 and (out == m).all()


def test_select_area_bounds_and_diagonal_joins(gpu):
    H, W = 24, 40
    m = np.zeros((H, W), bool)
    m[2, 2:7] = True            # 5 px
    m[6, 2:8] = True            # 6 px
    m[10, 2:9] = True           # 7 px
    m[14, 20] = m[15, 21] = m[16, 22] = True                                                            # joined only diagonally: one component of 3
    m[20, 30] = m[20, 32] = True                                                                        # a gap of one: two components
    for (lo, hi), areas in (((6, 6), [6]), ((5, 7), [5, 6, 7]), ((6, 7), [6, 7]), ((5, 6), [5, 6]), ((7, 2 ** 31 - 1), [7]), ((0, 1), [1, 1]), ((3, 3), [3]),
                            ((0, 0), []), ((8, 9), [])):
        out, boxes, n = _parts(m, gpu, lo, hi, True)
        assert boxes[:, 1].tolist() == areas and out.sum() == sum(areas), (lo, hi)
    out, boxes, n = _parts(m, gpu, 3, 3, True)
    assert boxes.tolist() == [[14 * W + 20, 3, 20, 14, 23, 17]]


@pytest.mark.parametrize("count", [255, 256, 257, 300])
def test_select_more_components_than_rows(gpu, count):
    """One-pixel components with min_area = 1: at most 256 boxes, those of the smallest labels, the true count beside them, every pixel in out."""
    H, W = 42, 40
    m = np.zeros((H, W), bool)
    ys, xs = np.divmod(np.arange(count), 20)
    m[2 * ys + 1, 2 * xs] = True
    out, boxes, n = _parts(m, gpu, 1, 1, False)
    assert n == count and len(boxes) == min(count, 256) and out.sum() == count and (out == m).all()
    assert boxes[:, 0].tolist() == np.flatnonzero(m)[:256].tolist() and (boxes[:, 1] == 1).all()


def test_stats_large_parts_and_an_empty_map(gpu):
    """A part that fills whole waves (the reduced path), a ring around a hole, parts that straddle rows of a width that is no multiple of 64; and
    an empty map: every stats row cleared, nothing kept, no box."""
    from videovanish_amd import overlaymask_bind as B
    H, W = 80, 140
    m = np.zeros((H, W), bool)
    m[3:75, 5:136] = True
    m[20:40, 30:90] = False
    m[25:35, 40:80] = True
    out, boxes, n = _parts(m, gpu, 64, H * W, True)
    assert n == 2 and boxes[:, 1].tolist() == [72 * 131 - 20 * 60, 400]
    out, boxes, n = _parts(~m, gpu, 0, 4096, True)                                                      # rule 5's call: the hole joins, the outside does not
    assert n == 1 and boxes[0, 1] == 20 * 60 - 400 and out.sum() == 800
    z = np.zeros((9, 33), bool)
    out, boxes, n = _parts(z, gpu, 0, 2 ** 31 - 1, False)
    assert n == 0 and not out.any() and len(boxes) == 0
    stats = B.component_stats(torch.full((9, 33), -1, dtype=torch.int32, device=gpu)).cpu().numpy()
    assert (stats == np.array([0, 33, 9, 0, 0])).all()
    full = np.ones((5, 70), bool)
    out, boxes, n = _parts(full, gpu, 0, 350, False)
    assert boxes.tolist() == [[0, 350, 0, 0, 70, 5]] and _parts(full, gpu, 0, 349, False)[2] == 0 and _parts(full, gpu, 0, 350, True)[2] == 0


# ---- vvo_merge ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T, H, W", [(1, 9, 16), (5, 7, 13), (3, 33, 132)])
def test_merge_union_and_counts(gpu, T, H, W):
    from videovanish_amd import overlaymask_bind as B
    rng = np.random.default_rng(T * W)
    dil = rng.choice(np.array([0, 0, 1, 7, 255], np.uint8), size=(T, H, W))
    o = rng.choice(np.array([0, 0, 0, 2, 255], np.uint8), size=(H, W))
    d, om = _d(dil, gpu), _d(o, gpu)
    out, added = B.merge(d, om)
    want = (dil != 0) | (o != 0)[None]
    assert (out.cpu().numpy() == want.astype(np.uint8) * 255).all() and added.dtype == torch.int64
    assert added.cpu().numpy().tolist() == ((o != 0)[None] & (dil == 0)).reshape(T, -1).sum(1).tolist() and added.sum() > 0
    assert (d.cpu().numpy() == dil).all() and (om.cpu().numpy() == o).all()
    lib, p = B.lib(), lambda t: t.data_ptr()
    assert lib.vvo_merge(p(d), p(om), T, H, W, p(d), p(added), None) == -1 and b"dil_out is not dil" in lib.vvo_last_error()
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == dil).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(gpu):
    """Every -1 / -2 of the header: the outputs keep their bytes, the counters are not cleared."""
    from videovanish_amd import overlaymask_bind as B
    lib = B.lib()
    f = torch.full((2, 8, 8, 3), 7, dtype=torch.uint8, device=gpu)
    m = torch.full((2, 8, 8), 7, dtype=torch.uint8, device=gpu)
    m2 = torch.full((2, 8, 8), 7, dtype=torch.uint8, device=gpu)
    w = torch.full((64, 5), 7, dtype=torch.int32, device=gpu)           # acc [8,8,4], labels, stats [64,5], boxes: any of them
    cnt = torch.full((4,), 7, dtype=torch.int64, device=gpu)
    p = lambda t: t.data_ptr()
    acc = lambda T=2, H=8, W=8, a=p(f), b=p(m), o=p(w): lib.vvo_accumulate(a, b, T, H, W, o, None)
    cla = lambda H=8, W=8, ms=12, mag=8, coh=80, s=p(w), e=p(m2), c=p(cnt): lib.vvo_classify(s, H, W, ms, mag, coh, e, c, None)
    sta = lambda H=8, W=8, l=p(w), s=p(w): lib.vvo_component_stats(l, H, W, s, None)
    sel = lambda H=8, W=8, lo=0, hi=9, l=p(w), s=p(w), o=p(m2), bx=p(w), n=p(cnt): lib.vvo_select(l, s, H, W, lo, hi, 1, o, bx, n, None)
    mer = lambda T=2, H=8, W=8, d=p(m), o=p(m), out=p(m2), c=p(cnt): lib.vvo_merge(d, o, T, H, W, out, c, None)
    bad = [acc(T=0), acc(H=0), acc(W=0), acc(H=1 << 16, W=1 << 15), acc(a=None), acc(b=None), acc(o=None),
           cla(H=0), cla(W=-1), cla(H=1 << 16, W=1 << 15), cla(ms=0), cla(mag=0), cla(coh=0), cla(s=None), cla(e=None), cla(c=None),
           sta(H=0), sta(W=0), sta(H=1 << 16, W=1 << 15), sta(l=None), sta(s=None),
           sel(H=0), sel(W=0), sel(H=1 << 16, W=1 << 15), sel(lo=-1), sel(hi=-1), sel(l=None), sel(s=None), sel(o=None), sel(bx=None), sel(n=None),
           mer(T=0), mer(H=0), mer(W=0), mer(H=1 << 16, W=1 << 15), mer(d=None), mer(o=None), mer(out=None), mer(c=None), mer(out=p(m))]
    assert bad == [-1] * len(bad) and b"vvo_merge" in lib.vvo_last_error()
    unsupported = [cla(ms=65536), cla(mag=2041), cla(coh=101), mer(T=65536), acc(T=65536)]
    assert unsupported == [-2] * len(unsupported) and b"65536" in lib.vvo_last_error()
    torch.cuda.synchronize()
    assert (f == 7).all() and (m == 7).all() and (m2 == 7).all() and (w == 7).all() and (cnt == 7).all()      # nothing was launched, nothing cleared
    with pytest.raises(RuntimeError, match="coh <= 100"):
        B.classify(torch.zeros((8, 8, 4), dtype=torch.int32, device=gpu), 12, 8, 101)
    with pytest.raises(RuntimeError):
        B.accumulate(f.cpu(), m.cpu(), torch.zeros((8, 8, 4), dtype=torch.int32))                       # no CPU fallback
    with pytest.raises(RuntimeError, match="acc"):
        B.accumulate(f, m, torch.zeros((8, 8, 3), dtype=torch.int32, device=gpu))
    with pytest.raises(ctypes.ArgumentError):
        lib.vvo_accumulate(p(f), p(m), 2.0, 8, 8, p(w), None)


# ---- the stage ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shared():
    """The shared clip at alpha 0.4 with a user mask that crosses the logo for a few frames, and the restatement's result, computed once."""
    frames, logo = R.overlay_clip(2, 0.4)
    dil = np.zeros(frames.shape[:3], np.uint8)
    for t in range(5, 13):
        dil[t, 8:34, 60 + 4 * (t - 5):76 + 4 * (t - 5)] = 255
    return frames, dil, logo, R.overlay(frames, dil)


def _same_report(rep, want):
    assert (rep.verdict, rep.strong, rep.edges, rep.found) == (want["verdict"], want["strong"], want["edges"], want["found"])
    assert rep.boxes.shape == want["boxes"].shape and (rep.boxes == want["boxes"]).all() and (rep.added == want["added"]).all()
    assert rep.overlay.dtype == np.uint8 and set(np.unique(rep.overlay)) <= {0, 255} and ((rep.overlay != 0) == want["O"]).all()


def test_stage_equals_the_restatement_whatever_the_batches(gpu, shared):
    from videovanish_amd import infill, overlaymask_bind as B
    frames, dil, logo, want = shared
    T, H, W = dil.shape
    assert want["verdict"] == "found" and want["found"] == 1 and not (logo & ~want["O"]).any()
    acc = _acc(_d(frames, gpu), _d(dil, gpu), [(0, T)])
    assert (acc == want["acc"]).all()
    edge, counts = B.classify(_d(acc, gpu), 12, 8, 80)
    assert ((edge.cpu().numpy() != 0) == want["E"]).all() and counts.cpu().numpy().tolist() == [want["strong"], want["edges"]]
    d = _d(dil, gpu)
    flist = list(frames)
    for max_bytes in (1 << 30, 5 * H * W * 3, 0):                                                       # one batch, batches of 5 frames, of one
        got, rep = infill.overlay_mask(flist, d, OverlayMaskConfig(max_bytes=max_bytes))
        assert got is not d and (got.cpu().numpy() == want["dil2"]).all()
        _same_report(rep, want)
    assert (d.cpu().numpy() == dil).all()
    # other settings: nothing closed or grown, the border allowed, small parts kept
    cfg = dict(close=0, grow=0, border=1, min_area=4, coh=60, mag=4)
    got, rep = infill.overlay_mask(flist, d, OverlayMaskConfig(**cfg))
    other = R.overlay(frames, dil, **cfg)
    assert other["found"] > 1 and (got.cpu().numpy() == other["dil2"]).all()
    _same_report(rep, other)


def test_stage_static_and_none_hand_the_masks_back(gpu):
    from videovanish_amd import infill
    frames, _ = R.overlay_clip(0, speed=0)
    d = _d(np.zeros(frames.shape[:3], np.uint8), gpu)
    got, rep = infill.overlay_mask(list(frames), d, OverlayMaskConfig())
    want = R.overlay(frames, np.zeros(frames.shape[:3], np.uint8))
    assert got is d and want["verdict"] == "static"
    _same_report(rep, want)
    flat = np.full((12, 20, 36, 3), 90, np.uint8)
    z = _d(np.zeros((12, 20, 36), np.uint8), gpu)
    got, rep = infill.overlay_mask(list(flat), z, OverlayMaskConfig())
    assert got is z and (rep.verdict, rep.strong, rep.edges, rep.found) == ("none", 0, 0, 0) and not rep.added.any()
    band, _ = R.overlay_clip(1, logo=False, band=(60, 66))                                              # the horizon: dropped by the border rule, kept without it
    zb = _d(np.zeros(band.shape[:3], np.uint8), gpu)
    for border in (0, 1):
        got, rep = infill.overlay_mask(list(band), zb, OverlayMaskConfig(border=border, max_area=30))
        want = R.overlay(band, np.zeros(band.shape[:3], np.uint8), border=border, max_area=30)
        assert want["verdict"] == ("found" if border else "none") and (got is zb) == (not border)
        _same_report(rep, want)


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------------
# "The call without the option on the restatement's masks" is the call whose infill.overlay_mask is a stand-in that returns the restatement's
# dil' (tests/test_shadowmask_gpu.py: mask_dilation_iter = 0 does not hand masks over as they are).
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=960, num_inference_steps=2, scheduler="ddim")
T_CLIP = 14


@pytest.fixture(scope="module")
def clip():
    """The shared clip at alpha 0.4, 14 frames, with all-zero masks as 3-channel frames, and the restatement's result."""
    frames, logo = R.overlay_clip(1, 0.4, T=T_CLIP)
    zero = np.zeros(frames.shape[:3], np.uint8)
    want = R.overlay(frames, zero)
    assert want["verdict"] == "found" and want["found"] == 1 and not (logo & ~want["O"]).any()
    return list(frames), [np.zeros(frames.shape[1:], np.uint8) for _ in frames], [f.copy() for f in frames], logo, want


def _run(frames, masks, prior, **kw):
    import diffuerase
    diffuerase.configure(RUN)
    try:
        out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, **KW, **kw)
        return out, diffuerase.last_overlay_mask
    finally:
        diffuerase.configure(None)


def _same(a, b):
    return len(a) == len(b) == T_CLIP and (np.stack(a) == np.stack(b)).all()


@pytest.mark.parametrize("more", [{}, dict(shadow_mask="on", plate_fill="on"), dict(spans="masked", roi="static")], ids=["plain", "shadow-plate", "spans-roi"])
def test_drop_in_equals_the_call_on_the_restatements_masks(gpu, clip, monkeypatch, more):
    from videovanish_amd import infill
    frames, masks, prior, logo, want = clip
    kept = [f.copy() for f in frames]
    out, rep = _run(frames, masks, prior, overlay_mask="on", **more)
    assert rep is not None
    _same_report(rep, want)
    assert all((a == b).all() for a, b in zip(frames, kept)) and not np.stack(masks).any()               # the caller's arrays are not written
    stand_in = infill.OverlayMaskReport("found", 0, 0, np.zeros((0, 5), np.int32), 0, np.zeros(T_CLIP, np.int64), np.zeros(logo.shape, np.uint8))
    monkeypatch.setattr(infill, "overlay_mask", lambda f, d, cfg: (_d(want["dil2"], gpu), stand_in))
    hand, _ = _run(frames, masks, prior, overlay_mask="on", **more)
    assert _same(out, hand)
    monkeypatch.undo()
    base, none = _run(frames, masks, prior, **more)
    assert none is None and not _same(out, base)                                                        # without the option nobody removes the logo
    far = R.far_from(want["O"], 6)                                                                      # further from O than the feather (3 px) reaches
    for t in range(T_CLIP):
        assert (out[t][far] == frames[t][far]).all()
    assert any((out[t][logo] != frames[t][logo]).any() for t in range(T_CLIP))                          # the logo's pixels went to the model


def test_a_locked_off_clip_is_static_and_gives_the_bytes_of_the_call_without(gpu):
    frames, _ = R.overlay_clip(0, 0.4, T=T_CLIP, speed=0)
    flist, masks = list(frames), [np.zeros(frames.shape[1:], np.uint8) for _ in frames]
    prior = [f.copy() for f in flist]
    out, rep = _run(flist, masks, prior, overlay_mask="on")
    assert rep is not None and rep.verdict == "static" and not rep.added.any() and rep.found == 0
    base, none = _run(flist, masks, prior)
    assert none is None and _same(out, base)


def test_find_overlays_is_the_stage_without_a_model(gpu, clip, monkeypatch):
    import diffuerase
    frames, masks, prior, logo, want = clip
    monkeypatch.setattr(diffuerase, "_load_model", lambda *a: pytest.fail("find_overlays loads no model"))
    monkeypatch.setattr(diffuerase, "_load_prior", lambda *a: pytest.fail("find_overlays loads no prior"))
    for given in (None, masks):
        overlay, rep = diffuerase.find_overlays(frames, given)
        assert overlay is rep.overlay and ((overlay != 0) == want["O"]).all()
        _same_report(rep, want)
    overlay, rep = diffuerase.find_overlays(frames, None, "grow=0")
    assert ((overlay != 0) == R.overlay(np.stack(frames), np.zeros((T_CLIP,) + logo.shape, np.uint8), grow=0)["O"]).all()
    assert diffuerase.last_overlay_mask is None or diffuerase.last_overlay_mask is not rep
