"""Block-matched inpaint deflicker on the GPU: vvk_search and vvk_hold against the numpy restatement (tests/deflickerlocal_ref.py) bit for bit,
each call run twice with identical bytes; inputs on which ties decide; vvk_hold against the existing kernels (vvc_hold with every record
(0, 0, 1, 0), vvf_hold at search = 0); poisoned buffers with guard bands; refusals; and the drop-in's deflicker_local= path on the tiny
architecture against the same call with the two device functions replaced by the restatement.  No tolerances."""
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflicker_ref as R0  # noqa: E402
import deflickeralign_ref as RA  # noqa: E402
import deflickerlocal_ref as R  # noqa: E402
import spans_ref  # noqa: E402

from videovanish_amd.config import TINY_UNET, TINY_VAE, RunConfig  # noqa: E402
from videovanish_amd.deflickerlocal import DeflickerLocalConfig as Cfg  # noqa: E402
from videovanish_amd.roi import RoiConfig  # noqa: E402
from videovanish_amd.spans import SpanConfig  # noqa: E402

TS = (1, 2, 9, 17)
# (radius, search, block, lam, tol): every value of radius {0, 1, 2, 4}, search {0, 1, 4, 8}, block {8, 16}, lam {0, 32, 65535}, tol {0, 6, 255}
SETTINGS = ((0, 4, 8, 32, 6), (1, 1, 16, 0, 0), (2, 4, 8, 32, 6), (2, 0, 16, 32, 255), (4, 4, 16, 65535, 255))
SMALL_T_EDGES = (4, 8, 8, 0, 255)           # with T <= 9
LARGE_T_EDGES = (4, 8, 16, 65535, 6)        # T = 17 with search = 8: one case in the file


def _d(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _clip(seed, T, h, w, H0, W0, offsets, off):
    """test_deflickeralign_gpu's clip: one textured background fixed on the canvas, seen through the windows of the panned frames: the window
    pixel (yy, xx) of frame t shows wide[offsets[t] + (yy, xx) + (off[t].y, off[t].x)]; +-5 levels of flicker, a block that changes for good
    half way, flat runs (where lam decides) and a mask of random bytes over a third of the frame."""
    rng = np.random.default_rng(seed)
    ey, ex = offsets[:, 0] + off[:, 1], offsets[:, 1] + off[:, 0]
    wide = rng.integers(0, 256, (int(ey.max() - ey.min()) + h, int(ex.max() - ex.min()) + w, 3))
    wide[: len(wide) // 3] = wide[: len(wide) // 3] // 64 * 64
    win = np.stack([wide[y - ey.min():y - ey.min() + h, x - ex.min():x - ex.min() + w] for y, x in zip(ey, ex)])
    win = win + rng.integers(-5, 6, (T, h, w, 3)) * (rng.random((T, h, w, 1)) < 0.8)
    win[T // 2:, h // 4: h // 2, w // 3:] += 40
    mask = (rng.random((T, H0, W0)) < 0.33) * rng.integers(1, 256, (T, H0, W0))
    return np.clip(win, 0, 255).astype(np.uint8), mask.astype(np.uint8)


def _moving_offsets(T, h, w, H0, W0, seed):
    """Offsets that move by 0 .. 3 px per frame, bounce off the frame's edges and touch them (test_deflicker_gpu's)."""
    rng = np.random.default_rng(seed)
    o = np.zeros((T, 2), np.int64)
    o[0] = (H0 - h, 0)
    d = np.array([-1, 1])
    for t in range(1, T):
        for a, lim in ((0, H0 - h), (1, W0 - w)):
            v = o[t - 1, a] + d[a] * rng.integers(0, 4)
            if v < 0 or v > lim:
                d[a] = -d[a]
                v = min(max(v, 0), lim)
            o[t, a] = v
    return o


def _wild(T, h, w):
    """Tracks whose steps exceed the window, and whose values lie at the ends of int32."""
    far, t = np.stack([np.arange(T) * (w + 12), np.arange(T) * -(h + 12)], 1), np.arange(T)
    wild = np.stack([np.where(t % 2, 2 ** 31 - 1 - 100 * t, -(2 ** 31) + 100 * t), np.where(t % 2, -(2 ** 31) + 100 * t, 2 ** 31 - 1 - 100 * t)], 1)
    return far, wild


def _scenes(T):
    """name -> (win, offsets, track, mask): the window placements and the tracks of the file.  The pictures follow a pan that the track given to
    the kernels misses by -2 .. 2 px per frame (none at all for the zero track), which is what the search has to find."""
    out = {}
    h, w, H0, W0 = 40, 56, 64, 96
    rng = np.random.default_rng(T)
    miss = rng.integers(-2, 3, (T, 2))
    fixed = np.tile([[12, 8]], (T, 1))
    off = RA.walk(T, T, (0, 5), (-2, 2))
    out["fixed-walk-lost"] = _clip(T * 1000 + h, T, h, w, H0, W0, fixed, off + miss) + (fixed, RA.make_track(off, lost=(3, T - 1)))
    pan = RA.walk(T, T + 50, (0, 3), (-1, 1))
    zero = np.zeros((T, 2), np.int64)
    out["full-odd-zero"] = _clip(T, T, 45, 83, 45, 83, zero, pan) + (zero, R.zero_track(T))
    moving = _moving_offsets(T, h, w, H0, W0, T)
    off = RA.walk(T, T + 90, (-4, 1), (-2, 2))
    out["moving-walk"] = _clip(T + 7, T, h, w, H0, W0, moving, off + miss) + (moving, RA.make_track(off))
    out["moving-zero"] = _clip(T + 8, T, h, w, H0, W0, moving, pan) + (moving, R.zero_track(T))
    far, wild = _wild(T, h, w)
    still = _clip(T + 3, T, h, w, H0, W0, moving, zero)
    out["moving-far"] = still + (moving, RA.make_track(far))
    out["moving-int32-ends"] = still + (moving, RA.make_track(wild))
    return {k: (v[0], v[2], v[3], v[1]) for k, v in out.items()}


def _search_twice(win, offs, track, radius, cfg, gpu):
    from videovanish_amd import flicklocal_bind as B
    args = (_d(win, gpu), _d(np.asarray(offs, np.int32), gpu), None if track is None else _d(np.asarray(track, np.int32), gpu))
    a, b = (B.search(*args, radius, cfg) for _ in range(2))
    mv, stats = a[0].cpu().numpy(), a[1].cpu().numpy()
    assert (mv == b[0].cpu().numpy()).all() and (stats == b[1].cpu().numpy()).all()
    T, h, w, _ = win.shape
    assert mv.dtype == np.int32 and mv.shape == (T, 2 * radius + 1) + B.blocks(h, w, cfg.block) + (4,)
    assert stats.dtype == np.int64 and stats.shape == (T, 2 * radius + 1, 6)
    return a[0], mv, stats


def _hold_twice(win, offs, track, mv, mask, radius, block, tol, gpu):
    from videovanish_amd import flicklocal_bind as B
    args = (_d(win, gpu), _d(np.asarray(offs, np.int32), gpu), None if track is None else _d(np.asarray(track, np.int32), gpu),
            mv if torch.is_tensor(mv) else _d(np.asarray(mv, np.int32), gpu), _d(mask, gpu))
    a, b = (B.hold(*args, radius, block, tol) for _ in range(2))
    out, sums = a[0].cpu().numpy(), a[1].cpu().numpy()
    assert (out == b[0].cpu().numpy()).all() and (sums == b[1].cpu().numpy()).all()
    assert out.dtype == np.uint8 and out.shape == win.shape and sums.dtype == np.int64 and sums.shape == (len(win), 12)
    return out, sums


def _against_the_restatement(win, offs, track, mask, settings, gpu):
    """Every (radius, search, block, lam, tol) of `settings`: mv, stats, out and sums bit for bit -> {setting: (mv, stats, out, sums)}."""
    got = {}
    for radius, search, block, lam, tol in settings:
        mv_t, mv, stats = _search_twice(win, offs, track, radius, Cfg(block, search, lam), gpu)
        want_mv, want_stats = R.search(win, offs, track, radius, block, search, lam)
        key = (radius, search, block, lam, tol)
        assert (mv == want_mv).all(), (key, int((mv != want_mv).any(-1).sum()), mv[(mv != want_mv).any(-1)][:3].tolist(), want_mv[(mv != want_mv).any(-1)][:3].tolist())
        assert (stats == want_stats).all(), (key, stats.reshape(-1, 6)[:3].tolist(), want_stats.reshape(-1, 6)[:3].tolist())
        out, sums = _hold_twice(win, offs, track, mv_t, mask, radius, block, tol, gpu)
        want, wsums = R.hold(win, offs, track, want_mv, mask, radius, block, tol)
        assert (out == want).all(), (key, int((out != want).sum()))
        assert (sums == wsums).all(), (key, sums[0].tolist(), wsums[0].tolist())
        got[key] = mv, stats, out, sums
    return got


def _settings(T, large=False):
    return SETTINGS + ((SMALL_T_EDGES,) if T <= 9 else ()) + ((LARGE_T_EDGES,) if large and T == 17 else ())


# ---- vvk_search and vvk_hold against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
def test_window_fixed_in_the_frame_with_lost_frames(gpu, T):
    """A 40 x 56 window at (12, 8) of a 64 x 96 frame (block 8: whole blocks; block 16: half blocks on both edges), a random-walk track that
    misses the picture's pan by -2 .. 2 px, frames 3 and T - 1 lost."""
    win, offs, track, mask = _scenes(T)["fixed-walk-lost"]
    got = _against_the_restatement(win, offs, track, mask, _settings(T, large=True), gpu)
    mv, stats, out, sums = got[(2, 4, 8, 32, 6)]
    for t in {3, T - 1} & set(range(T)):
        assert not mv[t].any() and not stats[t].any() and (out[t] == win[t]).all() and sums[t, 2] == 40 * 56
        for s in range(max(t - 2, 0), min(t + 3, T)):
            assert not mv[s, t - s + 2].any() and not stats[s, t - s + 2].any()                     # and gives no sample
    assert not mv[:, 2].any()                                                                       # the slot of s == t
    if T >= 9:
        assert stats[:, :, 1].sum() > 0 and stats[:, :, 3].max() >= 2 and sums[:, 1].any()          # the search found the miss


@pytest.mark.parametrize("T", TS)
def test_full_frame_odd_width(gpu, T):
    """The full frame at 45 x 83: an odd width, tail blocks in both directions and a tail launch block; the zero track, the picture pans."""
    win, offs, track, mask = _scenes(T)["full-odd-zero"]
    got = _against_the_restatement(win, offs, None, mask, _settings(T), gpu)
    mv, stats, out, sums = got[(2, 4, 8, 32, 6)]
    assert (sums[:, 0] == 45 * 83).all() and sums[:, 1].any() == (T > 1) and (stats[:, :, 0].sum() > 0) == (T > 1)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("scene", ["moving-walk", "moving-zero"])
def test_moving_windows(gpu, T, scene):
    """40 x 56 windows whose offsets move 0 .. 3 px per frame and touch the frame's edges: under a track that walks left and up as well, and
    under the zero track."""
    win, offs, track, mask = _scenes(T)[scene]
    assert offs[:, 0].max() == 24 and offs[:, 1].min() == 0
    got = _against_the_restatement(win, offs, track, mask, _settings(T), gpu)
    assert got[(2, 4, 8, 32, 6)][3][:, 1].any() == (T > 1)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("scene", ["moving-far", "moving-int32-ends"])
def test_steps_beyond_the_window_give_no_vector_and_no_sample(gpu, T, scene):
    """Tracks whose steps exceed the window and whose values lie at the ends of int32: no candidate is valid, n = 1 everywhere."""
    win, offs, track, mask = _scenes(T)[scene]
    for mv, stats, out, sums in _against_the_restatement(win, offs, track, mask, _settings(T), gpu).values():
        assert not mv.any() and not stats.any() and (out == win).all() and (sums[:, 2] == 40 * 56).all() and not sums[:, 1].any()


# ---- ties ----------------------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_zero_vector_and_to_the_nearer_match(gpu):
    T, h, w = 5, 40, 56
    offs, mask = np.zeros((T, 2), np.int64), np.zeros((T, h, w), np.uint8)
    flat = np.full((T, h, w, 3), 117, np.uint8)                                                    # constant in space: every candidate costs the same
    for key, (mv, stats, out, sums) in _against_the_restatement(flat, offs, None, mask, ((2, 4, 8, 0, 6), (2, 8, 16, 0, 6)), gpu).items():
        slots = [k for k in range(5) if k != 2]
        inside = np.array([[0 <= t - 2 + k < T for k in slots] for t in range(T)])
        assert not mv[..., :2].any() and not mv[..., 3].any() and (mv[:, slots][inside][..., 2] == 1).all() and (out == flat).all()
    stripes = np.zeros((T, h, w, 3), np.uint8)                                                     # periodic in x with period 4, moving 1 px per frame
    vals = np.array([[30, 200, 90], [220, 40, 10], [120, 130, 250], [5, 60, 170]], np.uint8)
    for t in range(T):
        stripes[t] = vals[(np.arange(w) + t) % 4][None]
    for key, (mv, stats, out, sums) in _against_the_restatement(stripes, offs, None, mask, ((1, 4, 8, 0, 6), (1, 8, 16, 0, 6)), gpu).items():
        # frame t + 1 shows frame t's column x at x - 1 (and at x + 3, x - 5, x + 7, at every dy): the nearest of the equal matches wins
        assert (mv[:-1, 2, 1:-1, 1:-1] == (0, -1, 1, 0)).all() and (mv[1:, 0, 1:-1, 1:-1] == (0, 1, 1, 0)).all(), key
        assert (mv[:-1, 2, :, 0] == (0, 3, 1, 0)).all()                                             # at the left edge x - 1 is not valid: the next nearest


# ---- the existing kernels as yardsticks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 9])
def test_hold_with_zero_vectors_is_the_aligned_kernel(gpu, T):
    """vvk_hold with every record (0, 0, 1, 0) against flickalign_hip.hold, for every track and window placement of the file."""
    from videovanish_amd import flickalign_hip, flicklocal_bind as B
    for name, (win, offs, track, mask) in _scenes(T).items():
        h, w = win.shape[1:3]
        args = _d(win, gpu), _d(offs.astype(np.int32), gpu), _d(np.asarray(track, np.int32), gpu)
        for radius, block, tol in ((1, 8, 6), (2, 16, 12), (4, 8, 255)):
            mv = torch.zeros((T, 2 * radius + 1) + B.blocks(h, w, block) + (4,), dtype=torch.int32, device=gpu)
            mv[..., 2] = 1
            want = flickalign_hip.hold(*args, _d(mask, gpu), radius, tol)
            for _ in range(2):
                out, sums = B.hold(*args, mv, _d(mask, gpu), radius, block, tol)
                assert (out == want[0]).all() and (sums == want[1]).all(), (name, radius, block, tol)


def test_hold_with_random_vectors_is_the_restatement(gpu):
    """mv is data: random int32 records, the ends of int32 and flags other than 0 and 1 included."""
    from videovanish_amd import flicklocal_bind as B
    T = 9
    rng = np.random.default_rng(4)
    for name in ("fixed-walk-lost", "full-odd-zero", "moving-walk"):
        win, offs, track, mask = _scenes(T)[name]
        h, w = win.shape[1:3]
        for radius, block, tol in ((2, 8, 12), (4, 16, 255)):
            shape = (T, 2 * radius + 1) + B.blocks(h, w, block)
            mv = rng.integers(-6, 7, shape + (4,))
            mv[..., 2] = rng.integers(-1, 3, shape)
            ends = rng.random(shape) < 0.2
            mv[ends, 0] = rng.choice([-(2 ** 31), 2 ** 31 - 1, 0], int(ends.sum()))
            mv[ends, 1] = rng.choice([-(2 ** 31), 2 ** 31 - 1, 1], int(ends.sum()))
            mv[..., 3] = rng.integers(-(2 ** 31), 2 ** 31, shape)
            mv = mv.astype(np.int32)
            out, sums = _hold_twice(win, offs, track, mv, mask, radius, block, tol, gpu)
            want, wsums = R.hold(win, offs, track, mv, mask, radius, block, tol)
            assert (out == want).all() and (sums == wsums).all(), (name, radius, block, tol)
            assert (out != win).any()


def test_search_zero_on_fixed_windows_is_the_unaligned_filter(gpu):
    from videovanish_amd import flicker_hip, flicklocal_bind as B
    T, h, w, H0, W0 = 17, 40, 56, 64, 96
    offs, zero = np.tile([[12, 8]], (T, 1)), np.zeros((T, 2), np.int64)
    win, mask = _clip(21, T, h, w, H0, W0, offs, zero)
    args = _d(win, gpu), _d(offs.astype(np.int32), gpu)
    for radius, block, tol in ((1, 8, 6), (2, 16, 12), (4, 8, 255)):
        want = flicker_hip.hold(*args, _d(mask, gpu), radius, tol, fixed=True)
        for _ in range(2):
            mv, stats = B.search(*args, None, radius, Cfg(block, 0, 32))
            out, sums = B.hold(*args, None, mv, _d(mask, gpu), radius, block, tol)
            assert (out == want[0]).all() and (sums == want[1]).all()
        assert (out.cpu().numpy() != win).any() and not mv[..., :2].any()


# ---- every int of mv, stats, out and sums is written, nothing outside them ----------------------------------------------------------------
def test_poisoned_buffers_with_guard_bands(gpu):
    from videovanish_amd import flicklocal_bind as B
    T, h, w, H0, W0, radius, G = 9, 41, 55, 64, 96, 2, 4096
    offs, off = _moving_offsets(T, h, w, H0, W0, 2), RA.walk(T, 8, (-3, 4), (-2, 2))
    track = RA.make_track(off, lost=(5,))
    win, mask = _clip(9, T, h, w, H0, W0, offs, off + np.random.default_rng(1).integers(-2, 3, (T, 2)))
    win_t, offs_t, track_t, mask_t = _d(win, gpu), _d(offs.astype(np.int32), gpu), _d(track, gpu), _d(mask, gpu)
    for block, search in ((8, 4), (16, 8)):
        want_mv, want_stats = R.search(win, offs, track, radius, block, search, 32)
        want, wsums = R.hold(win, offs, track, want_mv, mask, radius, block, 6)
        for poison in (0x00, 0xFF):
            fill = -1 if poison else 0x0101010101010101
            for _ in range(2):
                mbuf = torch.full((want_mv.size + 2 * G,), -1 if poison else 0x01010101, dtype=torch.int32, device=gpu)
                tbuf = torch.full((want_stats.size + 2 * 16,), fill, dtype=torch.int64, device=gpu)
                obuf = torch.full((win.size + 2 * G,), poison, dtype=torch.uint8, device=gpu)
                sbuf = torch.full((T * 12 + 2 * 16,), fill, dtype=torch.int64, device=gpu)
                guards = [int(b[0].item()) for b in (mbuf, tbuf, obuf, sbuf)]
                mv, stats = mbuf[G:G + want_mv.size].view(want_mv.shape), tbuf[16:16 + want_stats.size].view(want_stats.shape)
                out, sums = obuf[G:G + win.size].view(win.shape), sbuf[16:16 + T * 12].view(T, 12)
                got = B.search(win_t, offs_t, track_t, radius, Cfg(block, search, 32), mv=mv, stats=stats)
                assert got[0].data_ptr() == mv.data_ptr() and got[1].data_ptr() == stats.data_ptr()
                got = B.hold(win_t, offs_t, track_t, mv, mask_t, radius, block, 6, out=out, sums=sums)
                assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == sums.data_ptr()
                assert (mv.cpu().numpy() == want_mv).all() and (stats.cpu().numpy() == want_stats).all()
                assert (out.cpu().numpy() == want).all() and (sums.cpu().numpy() == wsums).all()
                for buf, lo, n, guard in ((mbuf, G, want_mv.size, guards[0]), (tbuf, 16, want_stats.size, guards[1]), (obuf, G, win.size, guards[2]),
                                          (sbuf, 16, T * 12, guards[3])):
                    assert (buf[:lo] == guard).all() and (buf[lo + n:] == guard).all()


def test_refusals_launch_nothing_and_name_the_function(gpu):
    from videovanish_amd import flicklocal_bind as B, hip
    win, offs, mask = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=gpu), torch.zeros((2, 2), dtype=torch.int32, device=gpu), \
        torch.zeros((2, 8, 8), dtype=torch.uint8, device=gpu)
    track = torch.zeros((2, 8), dtype=torch.int32, device=gpu)
    mv = torch.zeros((2, 5, 1, 1, 4), dtype=torch.int32, device=gpu)
    cfg = Cfg()
    for bad in (lambda: B.search(win, offs, track, 5, cfg), lambda: B.search(win, offs, track, 2, types.SimpleNamespace(block=8, search=9, lam=32)),
                lambda: B.search(win, offs, track, 2, types.SimpleNamespace(block=8, search=4, lam=65536)),
                lambda: B.search(win, offs, track, 2, types.SimpleNamespace(block=12, search=4, lam=32)), lambda: B.search(win, offs[:1], track, 2, cfg),
                lambda: B.search(win, offs, track[:, :7].contiguous(), 2, cfg), lambda: B.search(win, offs, track.cpu(), 2, cfg),
                lambda: B.search(win, offs, track, 2, cfg, mv=mv[:, :4].contiguous()), lambda: B.search(win.cpu(), offs, None, 2, cfg),
                lambda: B.hold(win, offs, track, mv, mask, 5, 8, 12), lambda: B.hold(win, offs, track, mv, mask, 2, 8, 256),
                lambda: B.hold(win, offs, track, mv, mask, 2, 8, 12, out=win), lambda: B.hold(win, offs, track, mv[:, :3].contiguous(), mask, 2, 8, 12),
                lambda: B.hold(win, offs, track, mv.to(torch.int64), mask, 2, 8, 12), lambda: B.hold(win, offs, track, mv, mask[:, :7].contiguous(), 2, 8, 12),
                lambda: B.hold(win, offs, track, mv, mask, 2, 12, 12), lambda: B.hold(win, offs, track, mv.cpu(), mask, 2, 8, 12)):
        with pytest.raises(RuntimeError):
            bad()
    # the launchers themselves: device pointers, refused before anything is launched, the message names the function
    lib, p, st = B.lib(), hip._p, hip._stream()
    stats, sums, out = torch.zeros((2, 5, 6), dtype=torch.int64, device=gpu), torch.zeros((2, 12), dtype=torch.int64, device=gpu), torch.empty_like(win)
    search = lambda T=2, h=8, w=8, radius=2, block=8, s=4, lam=32, m=mv: lib.vvk_search(p(win), p(offs), p(track), T, h, w, radius, block, s, lam, p(m), p(stats), st)
    hold = lambda T=2, H0=8, W0=8, h=8, w=8, radius=2, block=8, tol=6, o=out: lib.vvk_hold(p(win), p(offs), p(track), p(mv), p(mask), T, H0, W0, h, w, radius, block,
                                                                                   tol, p(o), p(sums), st)
    for kw in (dict(T=0), dict(h=0), dict(w=-1), dict(radius=-1), dict(block=0), dict(s=-1), dict(lam=-1), dict(m=None)):
        assert search(**kw) == -1 and lib.vvk_last_error().startswith(b"vvk_search:"), kw
    for kw in (dict(block=12), dict(s=9), dict(lam=65536), dict(radius=5), dict(T=65536), dict(h=1 << 16, w=1 << 15)):
        assert search(**kw) == -2 and lib.vvk_last_error().startswith(b"vvk_search:"), kw
    for kw in (dict(T=0), dict(H0=0), dict(h=9), dict(w=9), dict(radius=-1), dict(block=-8), dict(tol=-1), dict(o=win), dict(o=None)):
        assert hold(**kw) == -1 and lib.vvk_last_error().startswith(b"vvk_hold:"), kw
    for kw in (dict(block=4), dict(radius=5), dict(tol=256), dict(T=65536), dict(H0=1 << 16, W0=1 << 15, h=1 << 16, w=1 << 15)):
        assert hold(**kw) == -2 and lib.vvk_last_error().startswith(b"vvk_hold:"), kw
    torch.cuda.synchronize()
    assert not stats.any() and not sums.any() and not mv.any()


# ---- the drop-in on the tiny architecture (the fixtures of test_deflicker_gpu.py) -------------------------------------------------------------
RUN = RunConfig(steps=2, chunk=4, overlap=2, seed=3, dtype="fp16", unet=TINY_UNET, vae=TINY_VAE)
KW = dict(mask_dilation_iter=2, max_img_size=80, num_inference_steps=2, scheduler="ddim")         # the model runs at 48 x 80, the frame is 96 x 160
T, H, W = 9, 96, 160
REGIONS = RoiConfig("follow", context=0.25, pad_min=8, min_side=32, smooth=1, max_regions=8)
SPANS = SpanConfig("masked", context=1, min_len=3, min_gap=2)
BOXES = [(6, 18, 6, 30, 2), (70, 86, 124, 148, -2)]          # top left moving right, bottom right moving left, in frames 2 .. 6
LOGO = (40, 100, 64, 150)                                    # screen-fixed across the split between the planes, in frames 2 .. 6


def _with_prior(frames, masks):
    prior = []
    for f, m in zip(frames, masks):
        p = f.copy()
        p[m[..., 0] > 0] = f.reshape(-1, 3).mean(0).astype(np.uint8)
        prior.append(p)
    return prior


@pytest.fixture(scope="module")
def still_clip():
    """test_deflicker_gpu's clip with the camera locked off."""
    frames, _ = spans_ref.shots_clip(61, (T,), (0,), H, W)
    masks = []
    for t in range(T):
        m = np.zeros((H, W, 3), np.uint8)
        if 2 <= t <= 6:
            for y0, y1, x0, x1, vx in BOXES:
                m[y0:y1, x0 + vx * t: x1 + vx * t] = 255
        masks.append(m)
    return frames, masks, _with_prior(frames, masks)


@pytest.fixture(scope="module")
def two_plane_clip():
    """Two planes of motion behind a screen-fixed logo: the rows above 48 pan 1 .. 3 px per frame to the right, those below to the left, over
    iid textures with +-3 levels of noise; in frames 2 .. 6 the logo (masked) and a box that crosses the upper plane."""
    rng = np.random.default_rng(12)
    tex = rng.integers(40, 216, (2, H, W + 80, 3))
    pan = np.stack([np.cumsum(rng.integers(1, 4, T)), np.cumsum(rng.integers(-3, 0, T))])
    frames, masks = [], []
    for t in range(T):
        f = np.concatenate([tex[0, :H // 2, 40 + pan[0, t]:40 + pan[0, t] + W], tex[1, H // 2:, 40 + pan[1, t]:40 + pan[1, t] + W]]) + rng.integers(-3, 4, (H, W, 3))
        f = np.clip(f, 0, 255).astype(np.uint8)
        m = np.zeros((H, W, 3), np.uint8)
        if 2 <= t <= 6:
            m[LOGO[0]:LOGO[2], LOGO[1]:LOGO[3]] = 255
            m[6:22, 6 + 9 * t: 30 + 9 * t] = 255
            f[m[..., 0] > 0] = 20
        frames.append(f)
        masks.append(m)
    return frames, masks, _with_prior(frames, masks)


def _call(clip, host=False, **kw):
    """-> (output frames, last_deflicker, last_deflicker_local) of the drop-in on the tiny architecture.  host=True: flicklocal_bind.search and
    flicklocal_bind.hold are the restatement."""
    import diffuerase
    from videovanish_amd import flicklocal_bind as B
    frames, masks, prior = clip[:3]
    device = B.search, B.hold
    diffuerase.configure(RUN)
    if host:
        B.search, B.hold = R.bind_search, R.bind_hold
    try:
        out = diffuerase.run_infill_on_frames(frames, masks, propainer_frames=prior, feather_px=3, **KW, **kw)
        return np.stack(out), diffuerase.last_deflicker, diffuerase.last_deflicker_local
    finally:
        B.search, B.hold = device
        diffuerase.configure(None)


def test_drop_in_search_zero_on_a_locked_off_clip_is_deflicker_alone_and_nothing_is_resolved_without_the_option(gpu, still_clip):
    from videovanish_amd import flicklocal_bind as B
    kept, B.PART.dll = B.PART.dll, None
    try:
        base, rep, none = _call(still_clip, deflicker="on")
        assert none is None and rep is not None and B.PART.dll is None                              # a full call without the option
        same, _, zero_rows = _call(still_clip, deflicker="radius=0", deflicker_local="on")
        assert B.PART.dll is None and not zero_rows.blocks.any()                                    # radius = 0: the existing path
    finally:
        B.PART.dll = kept
    out, lrep_rep, lrep = _call(still_clip, deflicker="on", deflicker_local="search=0")
    assert (out == base).all() and (out != np.stack(still_clip[0])).any()
    for a, b in zip(rep, lrep_rep):
        assert (a == b).all()
    assert lrep.blocks.shape == (1, T) and lrep.blocks.sum() > 0 and not lrep.moved.any() and not lrep.max_vector.any() and (lrep.cost == lrep.cost_zero).all()
    assert rep.changed_mask.sum() > 0


# with two planes the tracker's best translation fits neither well: max_residual=255 keeps its frames tracked, so that the search runs on top of a
# track that is not zero (with the default every frame but the first is lost and stays unfiltered, as DESIGN.md section 19 says)
@pytest.mark.parametrize("kw", [dict(), dict(deflicker_align="max_residual=255"), dict(spans=SPANS, roi=REGIONS)], ids=["plain", "align", "spans-follow-regions"])
def test_drop_in_on_two_planes_equals_the_restatement(gpu, two_plane_clip, kw):
    import diffuerase
    out, rep, lrep = _call(two_plane_clip, deflicker="on", deflicker_local="on", **kw)
    if "deflicker_align" in kw:
        found = diffuerase.last_deflicker_align
        assert found.path == ("tracked",) and found.tracked[0].all() and found.off[0].any()
    want, wrep, wlrep = _call(two_plane_clip, host=True, deflicker="on", deflicker_local="on", **kw)
    assert (out == want).all()
    for a, b in zip(tuple(rep) + tuple(lrep), tuple(wrep) + tuple(wlrep)):
        assert a.shape == b.shape and (a == b).all()
    assert lrep.blocks.shape == rep.n.shape and lrep.blocks.shape[1] == T and lrep.blocks.sum() > 0 and (lrep.moved <= lrep.blocks).all() and lrep.max_vector.max() <= 4
    assert rep.changed_mask.sum() > 0 and (rep.changed_mask <= rep.n_mask).all()
    print("deflicker local report:", dict(blocks=lrep.blocks.tolist(), moved=lrep.moved.tolist(), max_vector=lrep.max_vector.tolist(),
                                          samples_mask=np.round(rep.samples_mask, 2).tolist()))
    alone, _, none = _call(two_plane_clip, deflicker="on", **kw)
    assert none is None and (out != alone).any()                                                    # and None after a call without the option
