"""Helpers of the aligned inpaint deflicker tests: the numpy restatement of include/vvflickalign.h, written from the header
in frame coordinates and independent of the product code, the synthetic pan the rule is judged on, random-walk tracks, and the restatement in
the shape of videovanish_amd/flickalign_hip.py's function (for tests that replace it).  No test in here."""
import numpy as np

NSUM = 12
T, H, W = 24, 40, 56        # the synthetic pan


def hold(win, offsets, track, mask2d, radius, tol):
    """Rules 2', lost frames, 3, 4, 5': win [T,h,w,3] u8, offsets [T,2] (oy, ox), track [T,8] (dx, dy, key, tracked, ...), mask2d [T,H0,W0]
    -> (out [T,h,w,3] u8, sums [T,12] int64)."""
    win = np.asarray(win, np.uint8)
    offsets = np.asarray(offsets, np.int64)
    track = np.asarray(track, np.int64)
    mask2d = np.asarray(mask2d)
    T, h, w, _ = win.shape
    _, H0, W0 = mask2d.shape
    x = win.astype(np.int64)
    out = np.empty_like(win)
    sums = np.zeros((T, NSUM), np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    ok_frame = track[:, 3] == 1
    for t in range(T):
        py, px = offsets[t, 0] + yy, offsets[t, 1] + xx                  # p, in frame t
        S, n = x[t].copy(), np.ones((h, w), np.int64)
        for s in range(max(0, t - radius), min(T, t + radius + 1)):
            if s == t or not (ok_frame[t] and ok_frame[s]):
                continue
            qy, qx = py + track[t, 1] - track[s, 1], px + track[t, 0] - track[s, 0]      # q = p + off[t] - off[s], in frame s
            ys, xs = qy - offsets[s, 0], qx - offsets[s, 1]                                # in frame s's window
            inside = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
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


def make_track(off, lost=()):
    """off [T,2] = (x, y) per frame -> track [T,8] int32 with every frame tracked but those of `lost` (which keep their offset for the record,
    as vvalign.h's lost frames do); the fields the filter does not read hold a pattern."""
    off = np.asarray(off)
    track = np.zeros((len(off), 8), np.int32)
    track[:, :2] = off
    track[:, 2] = 0
    track[:, 3] = 1
    track[:, 4:] = np.arange(len(off))[:, None] * 3 + 7
    for t in lost:
        if 0 <= t < len(off):
            track[t, 3] = 0
    return track


def walk(T, seed, steps_x=(0, 5), steps_y=(-2, 2)):
    """A random-walk track: off [T,2] int = (x, y), off[0] = (0, 0), steps drawn from the inclusive ranges."""
    rng = np.random.default_rng(seed)
    off = np.zeros((T, 2), np.int64)
    if T > 1:
        off[1:, 0] = np.cumsum(rng.integers(steps_x[0], steps_x[1] + 1, T - 1))
        off[1:, 1] = np.cumsum(rng.integers(steps_y[0], steps_y[1] + 1, T - 1))
    return off


def pan_flicker_clip(seed):
    """One iid texture seen through a frame that pans 2 .. 5 px in x and -2 .. 2 px in y per frame, rendered T times with +-3 levels of per-pixel
    noise and +-4 levels of per-frame pumping -> (clip int64 [T,H,W,3] inside 33 .. 223, off [T,2] int = (x, y): frame t shows the texture at
    its pixel + off[t])."""
    rng = np.random.default_rng(seed)
    off = walk(T, rng.integers(1 << 30), (2, 5), (-2, 2))
    my = int(max(-off[:, 1].min(), 0))
    wide = rng.integers(40, 216, (H + my + int(off[:, 1].max()), W + int(off[:, 0].max()), 3))
    clean = np.stack([wide[my + oy: my + oy + H, ox: ox + W] for ox, oy in off])
    return clean + rng.integers(-3, 4, clean.shape) + rng.integers(-4, 5, (T, 1, 1, 1)), off


def difference_along(x, off):
    """The mean absolute frame-to-frame difference along the motion: frame t at p against frame t + 1 at p + off[t] - off[t + 1], over the
    pixels both frames hold."""
    x = np.asarray(x, np.int64)
    total, count = 0, 0
    Hh, Ww = x.shape[1:3]
    for t in range(len(x) - 1):
        dx, dy = int(off[t][0] - off[t + 1][0]), int(off[t][1] - off[t + 1][1])
        y0, y1, x0, x1 = max(0, -dy), min(Hh, Hh - dy), max(0, -dx), min(Ww, Ww - dx)
        if y1 <= y0 or x1 <= x0:
            continue
        d = np.abs(x[t + 1, y0 + dy:y1 + dy, x0 + dx:x1 + dx] - x[t, y0:y1, x0:x1])
        total, count = total + int(d.sum()), count + d.size
    return total / count


def samples_per_pixel(sums):
    return float(sums[:, 2].sum() / sums[:, 0].sum())


# ---- the restatement in place of flickalign_hip's function (device tensors in, device tensors out) ---------------------------------------------
def hip_hold(win, offsets, track, mask2d, radius, tol, out=None):
    import torch
    o, s = hold(win.cpu().numpy(), offsets.cpu().numpy(), track.cpu().numpy(), mask2d.cpu().numpy(), int(radius), int(tol))
    return torch.from_numpy(o).to(win.device), torch.from_numpy(s).to(win.device)
