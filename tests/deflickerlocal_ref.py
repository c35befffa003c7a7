"""Helpers of the block-matched inpaint deflicker tests: the numpy restatement of include/flicklocal.h, written from the
header and independent of the product code, the two-plane synthetic clip the rule is judged on, and the restatement in the shape of
videovanish_amd/flicklocal_bind.py's two functions (for tests that replace them).  No test in here."""
import numpy as np

NSUM, NSTAT = 12, 6
T, H, W = 12, 64, 96        # the two-plane clip
SPLIT = 32                  # rows 0 .. SPLIT - 1 show plane 0, the others plane 1
DEFAULTS = dict(block=8, search=4, lam=32)


def zero_track(T):
    track = np.zeros((T, 8), np.int32)
    track[:, 3] = 1
    return track


def candidates(search):
    return [(dy, dx) for dy in range(-search, search + 1) for dx in range(-search, search + 1)]


def search(win, offsets, track, radius, block, search, lam, walk=None):
    """Rules D, B, S: win [T,h,w,3] u8, offsets [T,2] (oy, ox), track [T,8] (dx, dy, key, tracked, ...) -> (mv [T,2 radius+1,nby,nbx,4] int32,
    stats [T,2 radius+1,6] int64).  One whole-window absolute difference per (t, s, candidate), block sums by np.add.reduceat.  walk: the
    order in which the candidates are tried (the winner must not depend on it)."""
    win = np.asarray(win, np.uint8)
    T, h, w, _ = win.shape
    K = 2 * radius + 1
    track = zero_track(T) if track is None else np.asarray(track, np.int64)
    e = np.asarray(offsets, np.int64) + track[:, [1, 0]]
    tracked = track[:, 3] == 1
    ys0, xs0 = np.arange(0, h, block), np.arange(0, w, block)
    bh, bw = np.minimum(block, h - ys0), np.minimum(block, w - xs0)
    x = win.astype(np.int64)
    mv = np.zeros((T, K, len(ys0), len(xs0), 4), np.int32)
    stats = np.zeros((T, K, NSTAT), np.int64)
    walk = candidates(search) if walk is None else walk
    for t in range(T):
        for k in range(K):
            s = t - radius + k
            if s == t or s < 0 or s >= T or not (tracked[t] and tracked[s]):
                continue
            Dy, Dx = (int(v) for v in e[t] - e[s])
            have = np.zeros((len(ys0), len(xs0)), bool)
            best = np.zeros((4,) + have.shape, np.int64)                # cost, dy^2 + dx^2, dy, dx
            for dy, dx in walk:
                oy, ox = Dy + dy, Dx + dx
                valid = ((ys0 + oy >= 0) & (ys0 + bh + oy <= h))[:, None] & ((xs0 + ox >= 0) & (xs0 + bw + ox <= w))[None, :]
                if not valid.any():
                    continue
                y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
                diff = np.zeros((h, w), np.int64)
                diff[y0:y1, x0:x1] = np.abs(x[s, y0 + oy:y1 + oy, x0 + ox:x1 + ox] - x[t, y0:y1, x0:x1]).sum(-1)
                sad = np.add.reduceat(np.add.reduceat(diff, ys0, 0), xs0, 1)
                if dy == 0 and dx == 0:
                    stats[t, k, 5] = sad[valid].sum()
                key = (sad + lam * (abs(dy) + abs(dx)), dy * dy + dx * dx, dy, dx)
                less = np.zeros(have.shape, bool)
                equal = np.ones(have.shape, bool)
                for j in range(4):
                    less |= equal & (key[j] < best[j])
                    equal &= key[j] == best[j]
                take = valid & (~have | less)
                for j in range(4):
                    best[j] = np.where(take, key[j], best[j])
                have |= take
            mv[t, k, ..., 0], mv[t, k, ..., 1], mv[t, k, ..., 2], mv[t, k, ..., 3] = best[2] * have, best[3] * have, have, best[0] * have
            dy, dx = np.abs(best[2][have]), np.abs(best[3][have])
            stats[t, k, :5] = have.sum(), ((dy | dx) != 0).sum(), (dy + dx).sum(), np.maximum(dy, dx).max(initial=0), best[0][have].sum()
    return mv, stats


def hold(win, offsets, track, mv, mask2d, radius, block, tol):
    """Rule 2'', lost frames, vvflicker.h's 3 - 5: win [T,h,w,3] u8, offsets [T,2] (oy, ox), track [T,8], mv [T,2 radius+1,nby,nbx,4] (any int32
    content), mask2d [T,H0,W0] -> (out [T,h,w,3] u8, sums [T,12] int64)."""
    win = np.asarray(win, np.uint8)
    T, h, w, _ = win.shape
    offsets = np.asarray(offsets, np.int64)
    track = zero_track(T) if track is None else np.asarray(track, np.int64)
    mv = np.asarray(mv, np.int64)
    mask2d = np.asarray(mask2d)
    _, H0, W0 = mask2d.shape
    x = win.astype(np.int64)
    out = np.empty_like(win)
    sums = np.zeros((T, NSUM), np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    e = offsets + track[:, [1, 0]]
    tracked = track[:, 3] == 1
    for t in range(T):
        py, px = offsets[t, 0] + yy, offsets[t, 1] + xx                  # p, in frame t
        S, n = x[t].copy(), np.ones((h, w), np.int64)
        for s in range(max(0, t - radius), min(T, t + radius + 1)):
            if s == t or not (tracked[t] and tracked[s]):
                continue
            rec = mv[t, s - t + radius][yy // block, xx // block]
            ys, xs = yy + (e[t, 0] - e[s, 0]) + rec[..., 0], xx + (e[t, 1] - e[s, 1]) + rec[..., 1]
            inside = (rec[..., 2] == 1) & (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
            v = x[s][np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)]
            ok = inside & (np.abs(v - x[t]) <= tol).all(-1)
            S += v * ok[..., None]
            n += ok
        o = (2 * S + n[..., None]) // (2 * n[..., None])
        out[t] = o
        d = np.abs(o - x[t])
        inframe = (py >= 0) & (py < H0) & (px >= 0) & (px < W0)
        masked = inframe & (mask2d[t][np.clip(py, 0, H0 - 1), np.clip(px, 0, W0 - 1)] != 0)
        for k, sel in ((0, np.ones((h, w), bool)), (6, masked)):
            sums[t, k] = sel.sum()
            sums[t, k + 1] = (d.any(-1) & sel).sum()
            sums[t, k + 2] = n[sel].sum()
            sums[t, k + 3:k + 6] = d[sel].sum(0)
    return out, sums


# ---- the two-plane clip ----------------------------------------------------------------------------------------------------------------------
def two_plane_clip(seed, noise=True):
    """Two iid textures behind one another's edge: rows 0 .. 31 show texture 0 panning 1 .. 3 px per frame in x and -1 .. 1 px in y, rows 32 ..
    63 texture 1 panning -3 .. -1 px per frame in x; rendered T times with +-3 levels of per-pixel noise and +-4 levels of per-frame pumping
    (noise=False: the clean planes; the draws are made all the same) -> (clip u8 [T,H,W,3], pan int [2,T,2] = (x, y) per plane and frame:
    frame t shows plane j's texture at its pixel + pan[j, t])."""
    rng = np.random.default_rng(seed)
    tex = rng.integers(40, 216, (2, 144, 176, 3))
    pan = np.zeros((2, T, 2), np.int64)
    pan[0, :, 0] = np.cumsum(rng.integers(1, 4, T))
    pan[1, :, 0] = np.cumsum(rng.integers(-3, 0, T))
    pan[0, :, 1] = np.cumsum(rng.integers(-1, 2, T))
    clean = np.empty((T, H, W, 3), np.int64)
    for t in range(T):
        for j, (r0, r1) in enumerate(((0, SPLIT), (SPLIT, H))):
            px, py = pan[j, t]
            clean[t, r0:r1] = tex[j, 40 + py + r0:40 + py + r1, 40 + px:40 + px + W]
    for t in range(T):                                                   # per frame: the per-pixel noise, then the one pump
        grain = rng.integers(-3, 4, clean[t].shape)
        pump = rng.integers(-4, 5)
        if noise:
            clean[t] += grain + pump
    return np.clip(clean, 0, 255).astype(np.uint8), pan


def difference_along_planes(x, pan):
    """The mean absolute difference of frame t and frame t + 1 along each plane's own motion: frame t at p against frame t + 1 at p + pan[j, t]
    - pan[j, t + 1], over the pixels of plane j that lie 4 rows away from the split and the edges and 8 columns away from the sides."""
    x = np.asarray(x, np.int64)
    total = count = 0
    for j, (r0, r1) in enumerate(((4, SPLIT - 4), (SPLIT + 4, H - 4))):
        for t in range(len(x) - 1):
            dx, dy = (int(v) for v in pan[j, t] - pan[j, t + 1])
            d = np.abs(x[t + 1, r0 + dy:r1 + dy, 8 + dx:W - 8 + dx] - x[t, r0:r1, 8:W - 8])
            total, count = total + int(d.sum()), count + d.size
    return total / count


def samples_per_pixel(sums):
    return float(sums[:, 2].sum() / sums[:, 0].sum())


# ---- the restatement in place of flicklocal_bind's functions (device tensors in, device tensors out) -------------------------------------------
def _host(t):
    return None if t is None else t.cpu().numpy()


def bind_search(win, offsets, track, radius, cfg, mv=None, stats=None):
    import torch
    m, s = search(_host(win), _host(offsets), _host(track), int(radius), int(cfg.block), int(cfg.search), int(cfg.lam))
    return torch.from_numpy(m).to(win.device), torch.from_numpy(s).to(win.device)


def bind_hold(win, offsets, track, mv, mask2d, radius, block, tol, out=None, sums=None):
    import torch
    o, s = hold(_host(win), _host(offsets), _host(track), _host(mv), _host(mask2d), int(radius), int(block), int(tol))
    return torch.from_numpy(o).to(win.device), torch.from_numpy(s).to(win.device)
