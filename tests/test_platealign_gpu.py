"""Clean-plate alignment on the GPU: the entry points of vv_align.hip against the numpy restatement of include/vvalign.h
(tests/platealign_ref.py) bit for bit, each run twice with identical bytes; infill.plate_fill(acfg=) on the clip the unaligned stage cannot
fill; and the drop-in's plate_align= path against the same call handed the reference's frames and masks.  Tiny architecture."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import platealign_ref as A  # noqa: E402
import platefill_ref as R  # noqa: E402

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.platealign import PlateAlignConfig  # noqa: E402
from videovanish_amd.platefill import PlateFillConfig  # noqa: E402
from videovanish_amd.roi import RoiConfig  # noqa: E402
from videovanish_amd.spans import SpanConfig  # noqa: E402

SIZES = [(40, 56), (45, 83), (96, 130), (96, 132)]      # below one tile; odd; the byte path with a remainder tile; the 4-pixel path


def _d(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _twice(fn):
    """fn() -> tensors; run twice, identical bytes; the first run's results as numpy arrays."""
    a, b = fn(), fn()
    a, b = [x.cpu().numpy() for x in a], [x.cpu().numpy() for x in b]
    assert all((x == y).all() for x, y in zip(a, b))
    return a


def _random_clip(T, H, W, seed):
    """Random bytes, and masks of every kind: a block, speckles of any non-zero value, one frame masked completely, one not at all."""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (T, H, W, 3)).astype(np.uint8)
    m = rng.random((T, H, W)) < 0.03
    m[:, H // 3: H // 2, W // 4: W // 2] = True
    m[1], m[2] = True, False
    return frames, (m * rng.integers(1, 256, m.shape)).astype(np.uint8)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_pyramid(gpu, H, W):
    from videovanish_amd import align_hip
    frames, masks = _random_clip(5, H, W, H + W)
    f, d = _d(frames, gpu), _d(masks, gpu)
    for L in (0, 1, 2):
        want = A.pack(A.pyramid(frames, masks, L))
        assert want.shape == (5, align_hip.frame_bytes(H, W, L))
        got, = _twice(lambda: (align_hip.pyramid(f, d, L),))
        assert got.dtype == np.uint8 and (got == want).all(), (L, int((got != want).sum()))
        # in batches into the rows of one buffer, as the host does: rows 1 .. 4 start wherever S puts them
        buf = torch.full((5, want.shape[1]), 7, dtype=torch.uint8, device=gpu)
        align_hip.pyramid(f[:1], d[:1], L, out=buf[:1])
        align_hip.pyramid(f[1:], d[1:], L, out=buf[1:])
        assert (buf.cpu().numpy() == want).all()


def _level_case(gpu, pyr_host, pyr_dev, H, W, L, track, t, level, r, mo=25, mr=12):
    """One vva_sad + vva_pick against the restatement; returns (acc, track after)."""
    from videovanish_amd import align_hip
    want_acc = A.sad_level(pyr_host, track, t, level, r)
    tr = _d(track, gpu)
    acc, = _twice(lambda: (align_hip.sad(pyr_dev, tr, H, W, L, t, level, r),))
    assert acc.dtype == np.int64 and (acc == want_acc).all(), (t, level, r, acc.tolist(), want_acc.tolist())
    want_tr = track.copy()
    A.pick_level(want_acc, want_tr, H, W, L, t, level, r, mo, mr)
    got_tr, = _twice(lambda: (align_hip.pick(_d(acc, gpu), _d(track, gpu), H, W, L, t, level, r, mo, mr),))
    assert (got_tr == want_tr).all(), (t, level, r, got_tr.tolist(), want_tr.tolist())
    return acc, got_tr


@pytest.mark.parametrize("H,W", SIZES)
def test_sad_and_pick_on_single_levels(gpu, H, W):
    from videovanish_amd import align_hip
    T = 5
    frames, masks, off, clean, boxm, logom = A.pan_clip(T=T, H=H, W=W, seed=H, box=(H // 3, W // 4), box_speed=W // 6)
    masks[3] = 255                                                           # an all-invalid plane
    L = 2 if H >= 64 else 1
    pyr = A.pyramid(frames, masks, L)
    pyr_dev = align_hip.pyramid(_d(frames, gpu), _d(masks, gpu), L)
    base = np.zeros((T, 8), np.int32)
    base[:, 3] = 1
    base[1, :2] = off[1]

    def rec(t, cx, cy, key, level):
        tr = base.copy()
        tr[t] = [cx, cy, key, A.IN_PROGRESS, 0, 0, 0, level]
        return tr
    Wl, Hl = W >> L, H >> L
    acc, tr = _level_case(gpu, pyr, pyr_dev, H, W, L, rec(2, 0, 0, 0, L), 2, L, 4)                 # the first level of a frame
    assert tr[2, 3] == A.IN_PROGRESS and tr[2, 7] == L - 1 and acc[:, 1].min() > 0
    _level_case(gpu, pyr, pyr_dev, H, W, L, rec(2, 1, -1, 1, L), 2, L, 8)                           # the largest radius, another key
    _level_case(gpu, pyr, pyr_dev, H, W, L, rec(2, 1, -1, 1, 0), 2, 0, 8)                           # ... on the full plane: more than one block
    acc, tr = _level_case(gpu, pyr, pyr_dev, H, W, L, rec(2, Wl - 2, 2 - Hl, 0, L), 2, L, 3)        # candidates leave the plane: some n = 0
    assert (acc[:, 1] == 0).any() and (acc[:, 1] > 0).any() and tr[2, 3] == 0 and tr[2, 7] == L     # too little overlap everywhere: lost
    acc, tr = _level_case(gpu, pyr, pyr_dev, H, W, L, rec(2, 1000, -1000, 0, L), 2, L, 2)           # every candidate outside: n = 0 throughout
    assert not acc.any() and tr[2].tolist() == [int(off[1, 0]), int(off[1, 1]), 0, 0, 0, 0, 0, L]   # lost: the last tracked frame's offset
    assert tr[3].tolist() == [int(off[1, 0]) >> L, -((-int(off[1, 1])) >> L) if off[1, 1] < 0 else int(off[1, 1]) >> L, 0, A.IN_PROGRESS, 0, 0, 0, L]
    acc, tr = _level_case(gpu, pyr, pyr_dev, H, W, L, rec(3, 0, 0, 0, L), 3, L, 4)                  # an all-invalid frame
    assert not acc.any() and tr[3, 3] == 0
    acc, tr = _level_case(gpu, pyr, pyr_dev, H, W, L, rec(4, 0, 0, 3, L), 4, L, 4)                  # an all-invalid key
    assert not acc.any()
    # level 0 ends the frame: the true offset against key 0 is found from a centre one off, accepted, and frame t + 1 begins
    c = off[2] + [1, -1]
    acc, tr = _level_case(gpu, pyr, pyr_dev, H, W, L, rec(2, int(c[0]), int(c[1]), 0, 0), 2, 0, 1)
    assert tr[2, :4].tolist() == [int(off[2, 0]), int(off[2, 1]), 0, 1] and tr[2, 6] > 0 and tr[3, 3] == A.IN_PROGRESS and tr[3, 7] == L
    acc, tr0 = _level_case(gpu, pyr, pyr_dev, H, W, L, rec(2, int(c[0]), int(c[1]), 0, 0), 2, 0, 1, mr=0)      # the same best, refused by max_residual 0
    assert tr0[2, :4].tolist() == [int(off[1, 0]), int(off[1, 1]), 0, 0] and (tr0[2, 4:] == tr[2, 4:]).all()
    # r = 0: one candidate; the last frame starts no next one; a record that is finished, or in progress at another level, is left alone
    _level_case(gpu, pyr, pyr_dev, H, W, L, rec(4, int(off[4, 0]), int(off[4, 1]), 0, 0), 4, 0, 0)
    for tr in (base, rec(2, 0, 0, 0, L - 1), rec(2, 0, 0, T, L), rec(2, 0, 0, -1, L), rec(2, 1 << 25, 0, 0, L)):
        acc, after = _level_case(gpu, pyr, pyr_dev, H, W, L, tr, 2, L, 2)
        assert not acc.any() and (after == tr).all()


def _track_case(gpu, frames, masks, **cfg):
    from videovanish_amd import align_hip
    from videovanish_amd.platealign import coarsest_level
    cfg = dict(A.DEFAULTS, **cfg)
    T, H, W = masks.shape
    L = coarsest_level(H, W, cfg["levels"])
    want = A.track_segment(frames, masks, **cfg)
    pyr = align_hip.pyramid(_d(frames, gpu), _d(masks, gpu), L)
    got, = _twice(lambda: (align_hip.track(pyr, H, W, L, cfg["radius"], cfg["min_overlap"], cfg["max_residual"]),))
    assert got.dtype == np.int32 and (got == want).all(), (got.tolist(), want.tolist())
    return want


@pytest.mark.parametrize("kind", ["iid", "smooth"])
def test_track_on_the_synthetic_pans(gpu, kind):
    frames, masks, off, clean, boxm, logom = A.pan_clip(seed=0, kind=kind)
    for levels in (3, 0):
        track = _track_case(gpu, frames, masks, levels=levels, radius=4 if levels else 8)
        assert (track[:, :2] == off).all() and (track[:, 3] == 1).all()


def test_track_grey_lost_frame_key_change_and_short_clips(gpu):
    frames = np.full((6, 40, 56, 3), 128, np.uint8)
    masks = np.zeros((6, 40, 56), np.uint8)
    masks[:, 10:20, 10:30] = 255
    assert not _track_case(gpu, frames, masks)[:, :2].any()                  # the tie order: the centre
    _track_case(gpu, frames[:1], masks[:1])                                  # T = 1: the record of frame 0 and nothing else
    _track_case(gpu, frames[:2], masks[:2])
    frames, masks, off, clean, boxm, logom = A.pan_clip(seed=0)
    frames[5] = np.random.default_rng(5).integers(0, 256, frames[5].shape)
    assert _track_case(gpu, frames, masks)[:, 3].tolist() == [1] * 5 + [0] + [1] * 6
    masks[8] = 255                                                           # and a frame without a valid pixel: lost at the coarsest level
    track = _track_case(gpu, frames, masks)
    assert track[8].tolist()[3:] == [0, 0, 0, 0, 2] and track[9, 3] == 1
    frames, masks, off, clean, boxm, logom = A.pan_clip(T=12, H=64, W=96, seed=2, steps_x=(5, 5), steps_y=(0, 0), box=(20, 18), box_speed=7)
    assert _track_case(gpu, frames, masks)[:, 2].tolist() == [0, 0, 0, 0, 0, 0, 5, 5, 5, 5, 5, 10]


@pytest.mark.parametrize("H,W", SIZES)
def test_track_on_the_stage_clips_and_odd_sizes(gpu, H, W):
    if (H, W) in A.STAGE_CLIPS:
        frames, masks, off, clean, boxm, logom = A.stage_clip(H, W)
    else:
        frames, masks, off, clean, boxm, logom = A.pan_clip(T=8, H=H, W=W, seed=4, steps_x=(-4, 4), steps_y=(-3, 3), box=(30, 26))
    track = _track_case(gpu, frames, masks)
    assert (track[:, :2] == off).all() and (track[:, 3] == 1).all()
    _track_case(gpu, frames, masks, levels=1, radius=2, min_overlap=90, max_residual=0)      # settings under which frames are lost


def test_place_and_unplace_masks(gpu):
    from videovanish_amd import align_hip
    T, H, W = 5, 45, 83
    frames, masks = _random_clip(T, H, W, 11)
    track = np.zeros((T, 8), np.int32)
    track[:, 3] = 1
    track[1, :2], track[2, :2], track[3, :2], track[4, :2] = (9, -4), (-13, 6), (200, 0), (5, 5)
    track[4, 3] = 0                                                          # untracked; frame 3 lies outside every box below but the last
    d, tr = _d(masks, gpu), _d(track, gpu)
    whole = A.canvas_box(masks, track)
    for box in ((-6, -16, 51, 96), (3, 8, 30, 60), (10, 20, 11, 24), whole):
        want_d, want_i = A.place_masks(masks, track, box)
        got_d, got_i = _twice(lambda: align_hip.place_masks(d, tr, box))
        assert (got_d == want_d).all() and (got_i == want_i).all() and set(np.unique(got_i)) <= {0, 255}
        assert (got_i[4] == 255).all() and not got_d[4].any() and (box == whole or (got_i[3] == 255).all())
        back = np.random.default_rng(3).integers(0, 2, want_d.shape).astype(np.uint8) * 255
        want = A.unplace_mask(back, masks, track, box)
        got, = _twice(lambda: (align_hip.unplace_mask(_d(back, gpu), d, tr, box),))
        assert (got == want).all() and (got[4] == masks[4]).all() and (box == whole or (got[3] == masks[3]).all())
    same, = _twice(lambda: (align_hip.unplace_mask(align_hip.place_masks(d, tr, whole)[0], d, tr, whole),))
    assert (same == masks).all()                                             # the round trip of an untouched canvas


def test_refusals_launch_nothing(gpu):
    from videovanish_amd import align_hip
    lib = align_hip.lib()
    H = W = 32
    S = align_hip.frame_bytes(H, W, 1)
    f = torch.full((2, H, W, 3), 7, dtype=torch.uint8, device=gpu)
    m = torch.full((2, H, W), 7, dtype=torch.uint8, device=gpu)
    pyr = torch.full((2, S), 7, dtype=torch.uint8, device=gpu)
    tr = torch.full((2, 8), 7, dtype=torch.int32, device=gpu)
    acc = torch.full((289, 2), 7, dtype=torch.int64, device=gpu)
    p = lambda t: t.data_ptr()
    bad = [lib.vva_pyramid(p(f), p(m), 0, H, W, 1, p(pyr), None), lib.vva_pyramid(p(f), None, 2, H, W, 1, p(pyr), None),
           lib.vva_sad(p(pyr), p(tr), 2, H, W, 1, 2, 0, 1, p(acc), None), lib.vva_sad(p(pyr), p(tr), 2, H, W, 1, 1, 2, 1, p(acc), None),
           lib.vva_pick(p(acc), p(tr), 2, H, W, 1, 1, 0, 1, 0, 12, None), lib.vva_track(p(pyr), p(tr), p(acc), 2, H, W, 1, 0, 25, 12, None),
           lib.vva_place_masks(p(m), p(tr), 2, H, W, 0, 0, 0, 8, p(m), p(m), None), lib.vva_unplace_mask(p(m), p(m), p(tr), 2, H, W, 0, 0, H, W, p(m), None)]
    assert bad == [-1] * len(bad) and b"vva_unplace_mask" in lib.vva_last_error()
    unsupported = [lib.vva_pyramid(p(f), p(m), 2, H, W, 7, p(pyr), None), lib.vva_pyramid(p(f), p(m), 2, 8, W, 4, p(pyr), None),
                   lib.vva_sad(p(pyr), p(tr), 2, H, W, 1, 1, 0, 9, p(acc), None), lib.vva_track(p(pyr), p(tr), p(acc), 65536, H, W, 1, 4, 25, 12, None),
                   lib.vva_place_masks(p(m), p(tr), 65536, H, W, 0, 0, 8, 8, p(m), p(m), None)]
    assert unsupported == [-2] * len(unsupported) and b"65536" in lib.vva_last_error()
    torch.cuda.synchronize()
    assert (f == 7).all() and (m == 7).all() and (pyr == 7).all() and (tr == 7).all() and (acc == 7).all()      # nothing was launched, nothing cleared
    with pytest.raises(RuntimeError, match="r <= 8"):
        align_hip.sad(pyr, tr, H, W, 1, 1, 0, 9)
    with pytest.raises(RuntimeError):
        align_hip.pyramid(f.cpu(), m.cpu(), 1)                                                                # no CPU fallback
    with pytest.raises(ctypes.ArgumentError):
        lib.vva_sad(p(pyr), p(tr), 2.0, H, W, 1, 1, 0, 1, p(acc), None)


# ---- infill.plate_fill(acfg=) -------------------------------------------------------------------------------------------------------------
def _stage(gpu, frames, masks, pcfg=PlateFillConfig(), acfg=PlateAlignConfig(), cuts=None):
    from videovanish_amd import infill
    flist = [f.copy() for f in frames]
    d, got = _d(masks, gpu), []
    out, dil, rep = infill.plate_fill(flist, d, pcfg, cuts, acfg=acfg, align_out=got)
    assert all((a == b).all() for a, b in zip(flist, frames)) and (d.cpu().numpy() == masks).all()          # the caller's arrays are never written
    return flist, d, out, dil, rep, got[0]


@pytest.mark.parametrize("H,W", [(40, 56), (45, 83), (96, 132)])
def test_plate_align_fills_the_box_over_a_pan(gpu, H, W):
    """The clip the unaligned stage cannot fill: with plate_align every box pixel gets exactly the bytes of the clean pan and every pixel
    outside the mask keeps its own; without it nothing is filled."""
    from videovanish_amd import infill
    frames, masks, off, clean, boxm, logom = A.stage_clip(H, W)
    T = len(frames)
    flist, d, out, dil, rep, arep = _stage(gpu, frames, masks)
    out = np.stack(out)
    assert arep.path == ("canvas",) and (arep.off[0] == off).all() and arep.tracked[0].all() and not arep.residual[0].any()
    assert not dil.cpu().numpy().any() and (out[boxm] == clean[boxm]).all() and (out[masks == 0] == frames[masks == 0]).all()
    assert rep.filled.sum() == boxm.sum() and not rep.left.any() and rep.skipped == (False,)
    want, wd, wc, infos = A.plate_fill(frames, masks)
    assert (out == want).all() and (rep.filled == wc[:, 0]).all() and arep.box == (infos[0]["box"],)
    plain, pdil, prep = infill.plate_fill(flist, d, PlateFillConfig(), None)
    assert pdil is d and all(a is b for a, b in zip(plain, flist)) and not prep.filled.any()               # the pinned behaviour of the stage as it was


def test_plate_align_logo_cuts_lost_frame_and_fallback(gpu):
    logo = (28, 20, 34, 26)
    frames, masks, off, clean, boxm, logom = A.stage_clip(logo=logo)
    T = len(frames)
    for cuts in (None, [7]):
        flist, d, out, dil, rep, arep = _stage(gpu, frames, masks, cuts=cuts)
        want, wd, wc, infos = A.plate_fill(frames, masks, cuts=cuts)
        assert (np.stack(out) == want).all() and (dil.cpu().numpy() == wd).all() and (rep.filled == wc[:, 0]).all() and (rep.left == wc[:, 1]).all()
        assert all((out[i] is flist[i]) == (wc[i, 0] == 0) for i in range(T)) and arep.path == ("canvas",) * len(rep.segments)
    flist, d, out, dil, rep, arep = _stage(gpu, frames, masks)
    got = (masks != 0) & (dil.cpu().numpy() == 0)
    assert got[:, logom].sum() > 0.9 * logom.sum() * T and (np.stack(out)[got] == clean[got]).all()         # the screen-fixed logo: revealed by other frames
    # a frame of unrelated noise is lost: no sample, no fill, its mask stays; every other frame as the restatement has it
    noisy = frames.copy()
    noisy[7][masks[7] == 0] = np.random.default_rng(7).integers(0, 256, noisy[7].shape)[masks[7] == 0]
    flist, d, out, dil, rep, arep = _stage(gpu, noisy, masks)
    want, wd, wc, infos = A.plate_fill(noisy, masks)
    assert arep.tracked[0].tolist() == [t != 7 for t in range(T)] and out[7] is flist[7] and rep.left[7] == (masks[7] != 0).sum()
    assert (np.stack(out) == want).all() and (dil.cpu().numpy() == wd).all() and (rep.left == wc[:, 1]).all() and (rep.filled == wc[:, 0]).all()
    # other settings of the fill on the canvas
    pc = PlateFillConfig(guard=0, margin=0, max_gap=3)
    flist, d, out, dil, rep, arep = _stage(gpu, frames, masks, pcfg=pc)
    want, wd, wc, infos = A.plate_fill(frames, masks, **dict(R.DEFAULTS, guard=0, margin=0, max_gap=3))
    assert (np.stack(out) == want).all() and (dil.cpu().numpy() == wd).all() and (rep.filled == wc[:, 0]).all()
    # a canvas over max_bytes: the unaligned stage, flagged
    box = infos[0]["box"]
    full = T * (box[2] - box[0]) * (box[3] - box[1]) * 3
    flist, d, out, dil, rep, arep = _stage(gpu, frames, masks, pcfg=PlateFillConfig(max_bytes=full - 1))
    assert arep.path == ("fallback",) and dil is d and all(a is b for a, b in zip(out, flist)) and not rep.filled.any()
    flist, d, out, dil, rep, arep = _stage(gpu, frames, masks, pcfg=PlateFillConfig(max_bytes=full))
    assert arep.path == ("canvas",) and rep.filled.sum() > boxm.sum()


def test_plate_align_on_a_locked_off_clip_is_the_stage_without_it(gpu):
    from videovanish_amd import infill
    frames, masks, clean, boxm, logom = R.locked_off_clip()
    for cuts in (None, [9, 15]):
        flist, d, out, dil, rep, arep = _stage(gpu, frames, masks, cuts=cuts)
        base_out, base_dil, base = infill.plate_fill(flist, d, PlateFillConfig(), cuts)
        assert arep.path == ("static",) * len(rep.segments) and not np.concatenate(arep.off).any() and np.concatenate(arep.tracked).all()
        assert (np.stack(out) == np.stack(base_out)).all() and (dil.cpu().numpy() == base_dil.cpu().numpy()).all() and rep.filled.sum() > 0
        assert all((a == b).all() if isinstance(a, np.ndarray) else a == b for a, b in zip(rep, base))       # the PlateFillReport, field by field
        assert all((out[i] is flist[i]) == (base_out[i] is flist[i]) for i in range(len(flist)))


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=960, num_inference_steps=2, scheduler="ddim")
T, H, W = 14, 96, 160
SPANS = SpanConfig("masked", context=1, min_len=3, min_gap=2)
ROI = RoiConfig("follow", context=0.25, pad_min=8, min_side=32)
SCREEN = (64, 96, 88, 136)        # a screen-fixed region that shows something else in every frame: never steady on the canvas either
LOGO = (70, 104, 80, 124)         # a mask on it in frames 4 .. 8


@pytest.fixture(scope="module")
def clip():
    frames, masks, off, clean, boxm, _ = A.pan_clip(T=T, H=H, W=W, seed=5, noise=0, steps_x=(3, 3), steps_y=(0, 0), box=(22, 24), box_speed=-12)
    rng = np.random.default_rng(77)
    y0, x0, y1, x1 = SCREEN
    frames[:, y0:y1, x0:x1] = rng.integers(0, 256, (T, y1 - y0, x1 - x0, 3))
    masks[4:9, LOGO[0]:LOGO[2], LOGO[1]:LOGO[3]] = 255
    m3 = [np.repeat(m[..., None], 3, axis=2) for m in masks]
    prior = []
    for f, m in zip(frames, masks):
        p = f.copy()
        p[m > 0] = f.reshape(-1, 3).mean(0).astype(np.uint8)
        prior.append(p)
    return list(frames), m3, prior, off


def _run(frames, masks, prior, **kw):
    import diffuerase
    diffuerase.configure(RUN)
    try:
        out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, feather_px=3, **KW, **kw)
        return out, diffuerase.last_plate_fill, diffuerase.last_plate_align
    finally:
        diffuerase.configure(None)


def _same(a, b):
    return len(a) == len(b) == T and (np.stack(a) == np.stack(b)).all()


@pytest.mark.parametrize("more", [{}, dict(spans=SPANS, roi=ROI)], ids=["plain", "spans-roi"])
def test_drop_in_equals_the_call_on_the_reference_stage(gpu, clip, monkeypatch, more):
    from videovanish_amd import hip, infill
    frames, masks, prior, off = clip
    dil = hip.mask_collapse_dilate(_d(np.stack(masks), gpu), KW["mask_dilation_iter"]).cpu().numpy()
    want_f, want_d, want_c, infos = A.plate_fill(np.stack(frames), dil)
    assert infos[0]["path"] == "canvas" and (infos[0]["track"][:, :2] == off).all() and (infos[0]["track"][:, 3] == 1).all()
    kept = [f.copy() for f in frames]
    out, rep, arep = _run(frames, masks, prior, plate_fill="on", plate_align="on", **more)
    assert rep is not None and (rep.filled == want_c[:, 0]).all() and (rep.left == want_c[:, 1]).all() and rep.skipped == (False,)
    assert arep is not None and arep.path == ("canvas",) and (arep.off[0] == off).all() and arep.tracked[0].all()
    assert rep.filled.sum() > 0 and (rep.left > 0).tolist() == [4 <= t < 9 for t in range(T)]              # the box is filled, the logo is left
    assert all((a == b).all() for a, b in zip(frames, kept))
    empty = infill.PlateFillReport(np.zeros(T, np.int64), np.zeros(T, np.int64), (0,), (False,), ((0, T),), ())

    def by_hand(f, d, cfg, cuts=None, acfg=None, align_out=None):
        assert acfg == PlateAlignConfig()
        align_out.append(arep)
        return [want_f[i] if (want_f[i] != frames[i]).any() else frames[i] for i in range(T)], _d(want_d, gpu), empty
    monkeypatch.setattr(infill, "plate_fill", by_hand)
    hand, _, _ = _run(frames, masks, prior, plate_fill="on", plate_align="on", **more)
    assert _same(out, hand)
    monkeypatch.undo()
    filled = (dil != 0) & (want_d == 0)
    if more:
        assert all((out[t] == want_f[t]).all() for t in (0, 1, 11, 12, 13)) and not (out[6] == want_f[6]).all()
        assert all((out[t][filled[t]] == want_f[t][filled[t]]).all() for t in range(T))
    unaligned, urep, none = _run(frames, masks, prior, plate_fill="on", **more)
    assert none is None and not urep.filled.any() and not _same(out, unaligned)                            # without the option: the stage as it was
    with pytest.raises(ValueError, match="plate_align="):
        _run(frames, masks, prior, plate_align="on", **more)
