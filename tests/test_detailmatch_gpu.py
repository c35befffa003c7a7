"""Seam detail matching on the GPU: vvd_ring_detail_stats and vvd_sharpen against the restatement of include/detailmatch.h
(tests/detailmatch_ref.py), sums and bytes bit for bit, every launch twice with identical results; then the drop-in on the tiny architecture."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detailmatch_ref as R  # noqa: E402
import spans_ref  # noqa: E402

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.roi import RoiConfig  # noqa: E402
from videovanish_amd.spans import SpanConfig  # noqa: E402


def _d(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _clip(seed, T, Hm, Wm, H0, W0, boxes=((0.3, 0.3, 0.6, 0.65),), salt=0.004):
    """(patch [T,Hm,Wm,3], orig [T,H0,W0,3], mask [T,H0,W0]): bytes of every size with flat parts (spreads below and above any edge), masks of a
    few boxes (fractions of the frame) and a salt of single pixels, which the 5 x 5 gate has to clear by two pixels each."""
    rng = np.random.default_rng(seed)
    orig = rng.integers(0, 256, (T, H0, W0, 3))
    orig[:, : H0 // 3] = orig[:, : H0 // 3] // 16 + 100
    patch = rng.integers(0, 256, (T, Hm, Wm, 3))
    patch[:, :, Wm // 2:] = patch[:, :, Wm // 2:] // 8 + 60
    mask = (rng.random((T, H0, W0)) < salt) * rng.integers(1, 256, (T, H0, W0))
    for y0, x0, y1, x1 in boxes:
        mask[:, int(y0 * H0):int(y1 * H0), int(x0 * W0):int(x1 * W0)] = 255
    return patch.astype(np.uint8), orig.astype(np.uint8), mask.astype(np.uint8)


def _stats_twice(patch, orig, mask, offs, h, w, ring, edge, gpu):
    from videovanish_amd import detailmatch_bind as B
    args = (_d(patch, gpu), _d(orig, gpu), _d(mask, gpu), _d(np.asarray(offs, np.int32), gpu))
    a, b = (B.ring_detail_stats(*args, h, w, ring, edge).cpu().numpy() for _ in range(2))
    assert (a == b).all() and a.dtype == np.int64 and a.shape == (len(patch), 12)
    return a


def _sharpen_twice(patch, amount, h, w, overshoot, gpu):
    from videovanish_amd import detailmatch_bind as B
    args = (_d(patch, gpu), _d(np.asarray(amount, np.int32), gpu))
    a, b = (B.sharpen(*args, h, w, overshoot).cpu().numpy() for _ in range(2))
    assert (a == b).all() and a.dtype == np.uint8 and a.shape == (len(patch), h, w, 3)
    return a


def _against_the_restatement(patch, orig, mask, offs, h, w, gpu, rings=(8,), edges=(12,), amounts=None, overshoots=(4,)):
    """Both kernels on one case -> the sums of the last setting."""
    offs = np.asarray(offs, np.int32)
    for ring in rings:
        for edge in edges:
            got = _stats_twice(patch, orig, mask, offs, h, w, ring, edge, gpu)
            want = R.sums(patch, orig, mask, offs, h, w, ring, edge)
            assert (got == want).all(), (ring, edge, got[0].tolist(), want[0].tolist())
    T = len(patch)
    for amount in amounts or ([(300, -200, 0, 1024, -1024, 37)[t % 6] for t in range(T)],):
        for ov in overshoots:
            got_px = _sharpen_twice(patch, amount, h, w, ov, gpu)
            assert (got_px == R.sharpen(patch, amount, h, w, ov)).all(), (amount, ov)
    return got


# ---- tiles ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(37, 70), (32, 64), (70, 37), (33, 129)])
def test_windows_round_the_tile(gpu, h, w):
    """Partial tiles on both axes, one tile exactly, several tiles; w = 64 takes the 4-pixel stores, the others the byte form."""
    T, H0, W0 = 3, h + 11, w + 13
    patch, orig, mask = _clip(h * w, T, h, w, H0, W0)
    s = _against_the_restatement(patch, orig, mask, [(5, 6)] * T, h, w, gpu, rings=(1, 8, 32), edges=(0, 12, 40), overshoots=(0, 4))
    assert (s.reshape(T, 3, 4)[:, :, 0] > 0).all()


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_windows_no_5x5_fits_in(gpu, k):
    """h or w of 1 .. 4: no pixel has a 5 x 5 neighbourhood inside the window, so every sum is zero; at 5 exactly the middle row or column
    has one.  The apply replicates the window's edge pixels."""
    T, H0, W0 = 2, 24, 40
    for h, w in ((k, 36), (20, k), (k, k)):
        patch, orig, mask = _clip(7 * k + h, T, h, w, H0, W0, boxes=((0.0, 0.0, 1.0, 0.1), (0.0, 0.0, 0.1, 1.0)), salt=0.0)
        s = _against_the_restatement(patch, orig, mask, [(2, 3)] * T, h, w, gpu, edges=(0,))
        assert (k == 5 and min(h, w) == 5) or not s.any()


# ---- windows and the frame -------------------------------------------------------------------------------------------------------------------
def test_windows_over_the_frame_edges_and_moving_offsets(gpu):
    """One frame per edge with the window hanging over it (pixels outside the frame are no samples and block every 5 x 5 that reaches them), then
    windows that move inside the frame."""
    h, w, H0, W0 = 40, 72, 48, 90
    over = [(-6, 9), (H0 - h + 7, 9), (4, -8), (4, W0 - w + 10), (-3, -5), (H0 - h + 2, W0 - w + 3)]
    patch, orig, mask = _clip(3, len(over), h, w, H0, W0, boxes=((0.2, 0.2, 0.8, 0.8),))
    s = _against_the_restatement(patch, orig, mask, over, h, w, gpu, rings=(8, 32), edges=(0,))
    assert (s.reshape(-1, 3, 4)[:, :, 0] > 0).all()
    rng = np.random.default_rng(4)
    moving = np.stack([rng.integers(0, H0 - h + 1, 7), rng.integers(0, W0 - w + 1, 7)], 1)
    patch, orig, mask = _clip(5, 7, h, w, H0, W0)
    _against_the_restatement(patch, orig, mask, moving, h, w, gpu)


@pytest.mark.parametrize("Hm,Wm", [(20, 36), (64, 100), (40, 36), (33, 72)])
def test_model_size_differs_from_the_window(gpu, Hm, Wm):
    """The model's frame resized up, down and along one axis: the statistic and the apply read the window's pixel as the paste kernels do."""
    h, w, H0, W0, T = 40, 72, 50, 80, 2
    patch, orig, mask = _clip(Hm + Wm, T, Hm, Wm, H0, W0)
    _against_the_restatement(patch, orig, mask, [(3, 4), (7, 2)], h, w, gpu, amounts=([0, 0], [256, -256]))


# ---- the gates -------------------------------------------------------------------------------------------------------------------------------
def test_edge_at_equality_and_one_past(gpu):
    """x has a spread of exactly 12 wherever it has one: edge = 12 counts those pixels, edge = 13 none."""
    h, w = 40, 72
    rng = np.random.default_rng(8)
    patch = (100 + 12 * (rng.random((1, h, w, 3)) < 0.3)).astype(np.uint8)
    _, orig, mask = _clip(9, 1, h, w, h, w, salt=0.0)
    at, past = (_against_the_restatement(patch, orig, mask, [(0, 0)], h, w, gpu, edges=(e,)) for e in (12, 13))
    assert (at.reshape(3, 4)[:, 0] > 100).all() and not past.any()


def test_a_mask_pixel_two_and_three_pixels_from_a_ring_pixel(gpu):
    """One mask pixel: the ring pixels within two pixels of it (a box) have it in their 5 x 5 and do not count, those three away do."""
    h, w, ring = 40, 72, 8
    patch, orig, _ = _clip(10, 1, h, w, h, w)
    for y, x in ((20, 31), (20, 63), (20, 64), (31, 40), (32, 40)):                                  # inside a tile, at the tile's last column, first column, rows
        mask = np.zeros((1, h, w), np.uint8)
        mask[0, y, x] = 1
        s = _against_the_restatement(patch, orig, mask, [(0, 0)], h, w, gpu, rings=(ring,), edges=(0,))
        y0, y1, x0, x1 = max(y - ring, 2), min(y + ring, h - 3), max(x - ring, 2), min(x + ring, w - 3)       # the 5 x 5 stays inside the window
        assert s.reshape(3, 4)[:, 0].tolist() == [(y1 - y0 + 1) * (x1 - x0 + 1) - 25] * 3
    # two mask pixels five apart: the pixel between them is two from one and three from the other
    mask = np.zeros((1, h, w), np.uint8)
    mask[0, 20, 30] = mask[0, 20, 35] = 255
    _against_the_restatement(patch, orig, mask, [(0, 0)], h, w, gpu, rings=(3,), edges=(0,))


def test_extreme_bytes_need_64_bits(gpu):
    """A 0 / 255 checkerboard against its inverse, and a lattice of single 255 pixels: the largest |K| bytes give, sums beyond 32 bits in one
    tile; amounts of +-1024 on bytes 0 and 255."""
    h, w = 37, 70
    yy, xx = np.mgrid[:h, :w]
    board = (255 * ((yy + xx) % 2)).astype(np.uint8)
    lattice = (255 * ((yy % 2 == 0) & (xx % 2 == 0))).astype(np.uint8)
    patch = np.stack([np.repeat(p[..., None], 3, -1) for p in (board, lattice, 255 - lattice)])
    orig = np.stack([255 - patch[0], patch[1] // 2, patch[2]])
    mask = np.zeros((3, h, w), np.uint8)
    mask[:, 15:22, 30:40] = 255
    s = _against_the_restatement(patch, orig, mask, [(0, 0)] * 3, h, w, gpu, edges=(0, 255), amounts=([1024] * 3, [-1024] * 3, [1, -1, 0]), overshoots=(0, 4, 255))
    s = s.reshape(3, 3, 4)
    assert (s[:, :, 2] > 1 << 32).all() and s[0, 0, 1] < -(1 << 32) and not s[2, :, 3].any()


# ---- the apply -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [72, 71, 4, 8])
def test_sharpen_forms_alignment_and_poison(gpu, w):
    """w % 4 == 0 with an aligned base takes the 4-pixel stores, w % 4 != 0 and a base one or two bytes past an aligned one the byte form; every
    byte of out is written and none outside it; an amount-0 frame between two others is the window's pixel itself; T = 1."""
    from videovanish_amd import detailmatch_bind as B
    T, h = 3, 37
    patch, _, _ = _clip(w, T, h, w, h, w)
    amount = [411, 0, -256]
    want = R.sharpen(patch, amount, h, w, 4)
    assert (want[1] == patch[1]).all() and (want[0] != patch[0]).any() and (want[2] != patch[2]).any()
    n, G = want.size, 4096
    for shift in (0, 1, 2):
        for poison in (0x00, 0xFF):
            buf = torch.full((n + 2 * G,), poison, dtype=torch.uint8, device=gpu)
            out = B.sharpen(_d(patch, gpu), _d(np.asarray(amount, np.int32), gpu), h, w, 4, out=buf[G + shift:G + shift + n].view(want.shape))
            assert out.data_ptr() == buf.data_ptr() + G + shift and (out.cpu().numpy() == want).all()
            assert (buf[:G + shift] == poison).all() and (buf[G + shift + n:] == poison).all()
    for a in (0, 700):
        assert (_sharpen_twice(patch[:1], [a], h, w, 0, gpu) == R.sharpen(patch[:1], [a], h, w, 0)).all()
    # a resized window into a poisoned buffer: the amount-0 frame is the resize
    small = patch[:, : h // 2 + 1, : max(w // 2, 1)]
    want = R.sharpen(small, amount, h, w, 4)
    buf = torch.full((n + 2 * G,), 0xA5, dtype=torch.uint8, device=gpu)
    out = B.sharpen(_d(small, gpu), _d(np.asarray(amount, np.int32), gpu), h, w, 4, out=buf[G:G + n].view(want.shape))
    assert (out.cpu().numpy() == want).all() and (want[1] == R.window_image(small[1], h, w)).all() and (buf[:G] == 0xA5).all() and (buf[G + n:] == 0xA5).all()


def test_refusals_launch_and_clear_nothing(gpu):
    from videovanish_amd import detailmatch_bind as B
    from videovanish_amd import hip
    z = torch.full((2, 8, 8, 3), 7, dtype=torch.uint8, device=gpu)
    m, offs = torch.zeros((2, 8, 8), dtype=torch.uint8, device=gpu), torch.zeros((2, 2), dtype=torch.int32, device=gpu)
    amount = torch.full((2,), 300, dtype=torch.int32, device=gpu)
    for bad in (lambda: B.ring_detail_stats(z, z, m, offs, 8, 8, 0, 12), lambda: B.ring_detail_stats(z, z, m, offs, 8, 8, 33, 12),
                lambda: B.ring_detail_stats(z, z, m, offs, 8, 8, 8, 256), lambda: B.ring_detail_stats(z, z, m, offs, 9, 8, 8, 12),
                lambda: B.ring_detail_stats(z, z, m[:, :7].contiguous(), offs, 8, 8, 8, 12), lambda: B.ring_detail_stats(z, z, None, offs, 8, 8, 8, 12),
                lambda: B.sharpen(z, amount, 8, 8, 256), lambda: B.sharpen(z, amount, 8, 8, -1), lambda: B.sharpen(z, amount, 8, 8, 4, out=z),
                lambda: B.sharpen(z, amount[:1], 8, 8, 4), lambda: B.sharpen(z, amount, 4, 4, 4, out=torch.empty_like(z)),
                lambda: B.sharpen(z.cpu(), amount, 8, 8, 4)):
        with pytest.raises(RuntimeError):
            bad()
    # the launchers themselves: a refused call clears no sum and writes no byte
    lib = B.lib()
    sums = torch.full((2, 12), 5, dtype=torch.int64, device=gpu)
    p = hip._p
    assert lib.vvd_ring_detail_stats(p(z), 8, 8, p(z), p(m), p(offs), 2, 8, 8, 8, 8, 33, 12, p(sums), None) == -2
    assert lib.vvd_ring_detail_stats(p(z), 8, 8, p(z), p(m), p(offs), 2, 8, 8, 9, 8, 8, 12, p(sums), None) == -1
    assert lib.vvd_sharpen(p(z), 8, 8, p(amount), 2, 8, 8, 4, p(z), None) == -1 and lib.vvd_sharpen(p(z), 8, 8, p(amount), 2, 8, 8, 256, p(m), None) == -2
    torch.cuda.synchronize()
    assert (sums == 5).all() and (z == 7).all() and not m.any()


# ---- the drop-in on the tiny architecture ---------------------------------------------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=80, num_inference_steps=2, scheduler="ddim")         # the model runs at 48 x 80, the frame is 96 x 160
T, H, W = 9, 96, 160
REGIONS = RoiConfig("follow", context=0.25, pad_min=8, min_side=32, smooth=1, max_regions=8)
SPANS = SpanConfig("masked", context=1, min_len=3, min_gap=2)
BOXES = [(6, 26, 6, 40, 2), (60, 86, 110, 148, -2)]          # top left moving right, bottom right moving left, in frames 2 .. 6
# the tiny architecture's weights are random: its rendering of the ring has little to do with the original's detail, so the fit is given no
# dead zone and a small support, and whatever amount it finds is applied
ON = "edge=4,min_pixels=16,dead=0"
EVERYTHING = dict(spans=SPANS, roi=REGIONS, tone_match="on", seam_blend="on", grain_match="on", deflicker="on")


@pytest.fixture(scope="module")
def clip():
    frames, _ = spans_ref.shots_clip(61, (T,), (3,), H, W)
    masks, prior = [], []
    for t in range(T):
        m = np.zeros((H, W, 3), np.uint8)
        if 2 <= t <= 6:
            for y0, y1, x0, x1, vx in BOXES:
                m[y0:y1, x0 + vx * t: x1 + vx * t] = 255
        masks.append(m)
        p = frames[t].copy()
        p[m[..., 0] > 0] = frames[t].reshape(-1, 3).mean(0).astype(np.uint8)
        prior.append(p)
    return frames, masks, prior


@pytest.fixture(scope="module")
def run(gpu, clip):
    """run(**kw) -> (output frames, last_detail_match, whether detailmatch_bind resolved its symbols) of the drop-in on the tiny architecture; the
    results are kept, so every distinct call of this module runs once.  host=True: detailmatch_bind's two functions are the restatement."""
    import diffuerase
    from videovanish_amd import detailmatch_bind as B
    frames, masks, prior = clip
    seen = {}

    def call(host=False, **kw):
        key = repr((host, sorted(kw.items(), key=lambda i: i[0])))
        if key not in seen:
            device = B.ring_detail_stats, B.sharpen
            diffuerase.configure(RUN)
            if host:
                B.ring_detail_stats, B.sharpen = R.hip_ring_detail_stats, R.hip_sharpen
            try:
                out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, feather_px=3, **KW, **kw)
                seen[key] = (np.stack(out), diffuerase.last_detail_match, B.PART.dll is not None)
            finally:
                B.ring_detail_stats, B.sharpen = device
                diffuerase.configure(None)
        return seen[key]
    return call


def test_no_resolution_without_the_option(gpu, clip):
    """A fresh binding stays unresolved through whole calls without the option, whatever else is on."""
    import diffuerase
    from videovanish_amd import detailmatch_bind as B
    frames, masks, prior = clip
    kept, B.PART.dll = B.PART.dll, None
    diffuerase.configure(RUN)
    try:
        for kw in (dict(), dict(detail_match="off", tone_match="on"), dict(roi=REGIONS, spans=SPANS, deflicker="on")):
            diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, feather_px=3, **KW, **kw)
            assert B.PART.dll is None and diffuerase.last_detail_match is None
    finally:
        diffuerase.configure(None)
        B.PART.dll = kept


@pytest.mark.parametrize("kw", [dict(), EVERYTHING], ids=["plain", "spans-regions-seams-deflicker"])
def test_drop_in_stage_equals_the_restatement(gpu, run, kw):
    out, rep, resolved = run(detail_match=ON, **kw)
    want, wrep, _ = run(host=True, detail_match=ON, **kw)
    assert resolved and (out == want).all()
    for a, b in zip(rep, wrep):
        assert a.shape == b.shape and (a == b).all()
    K = 2 if kw else 1
    assert rep.n.shape == rep.amount.shape == rep.residual.shape == rep.clamped.shape == rep.dead.shape == (K, T)
    print("detail match report:", dict(n=rep.n.tolist(), amount=rep.amount.tolist(), clamped=rep.clamped.tolist()))
    assert rep.n[:, 2:7].all() and rep.amount.any() and (np.abs(rep.amount) <= 2.0).all() and (rep.amount >= -1.0).all()
    if kw:                                                                                          # frames outside the span: zero rows
        assert not any(v[:, [0, 8]].any() for v in rep)
    base, none, _ = run(**kw)
    assert none is None and (out != base).any()                                                     # and None after a call without the option


@pytest.mark.parametrize("kw", [dict(), EVERYTHING], ids=["plain", "spans-regions-seams-deflicker"])
def test_drop_in_strength_0_is_the_call_without_the_option(gpu, clip, run, kw):
    """strength = 0 only materialises the resize that the paste kernels otherwise do on the fly: byte for byte the call without the option, at a
    max_img_size that makes the model run at another size than the frame."""
    base, none, _ = run(**kw)
    out, rep, _ = run(detail_match=ON + ",strength=0", **kw)
    assert none is None and rep is not None and (out == base).all() and not rep.amount.any() and rep.n.any()
    assert (out != np.stack(clip[0])).any()
