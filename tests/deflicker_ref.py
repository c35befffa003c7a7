"""Helpers of the inpaint deflicker tests: the numpy restatement of include/vvflicker.h, the synthetic clips the rule is
judged on, and the restatement in the shape of videovanish_amd/flicker_hip.py's two functions (for tests that replace them)."""
import numpy as np

DEFAULTS = dict(radius=2, tol=12)
NSUM = 12
T, H, W = 24, 40, 56        # the synthetic clips


def window_pixels(patch, h, w):
    """Rule 1: patch [T,Hm,Wm,3] u8 -> [T,h,w,3] u8 (cv2's fixed-point INTER_LINEAR; the bytes as they are at equal size)."""
    from oracle import imageops_ref as I
    patch = np.asarray(patch, np.uint8)
    if patch.shape[1:3] == (h, w):
        return patch.copy()
    return np.stack([I.resize_bilinear_u8(f, w, h) for f in patch])


def hold(win, offsets, mask2d, radius, tol):
    """Rules 2 - 5: win [T,h,w,3] u8, offsets [T,2] (oy, ox), mask2d [T,H0,W0] -> (out [T,h,w,3] u8, sums [T,12] int64)."""
    win = np.asarray(win, np.uint8)
    offsets = np.asarray(offsets, np.int64)
    mask2d = np.asarray(mask2d)
    T, h, w, _ = win.shape
    _, H0, W0 = mask2d.shape
    x = win.astype(np.int64)
    out = np.empty_like(win)
    sums = np.zeros((T, NSUM), np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    for t in range(T):
        py, px = offsets[t, 0] + yy, offsets[t, 1] + xx
        S, n = x[t].copy(), np.ones((h, w), np.int64)
        for s in range(max(0, t - radius), min(T, t + radius + 1)):
            if s == t:
                continue
            ys, xs = py - offsets[s, 0], px - offsets[s, 1]
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


def flicker_clip(seed):
    """One background rendered T times: +-3 levels of per-pixel noise and +-4 levels of per-frame pumping -> int64 [T,H,W,3] inside 33 .. 223."""
    rng = np.random.default_rng(seed)
    base = rng.integers(40, 216, (H, W, 3))
    noise = rng.integers(-3, 4, (T, H, W, 3))
    pump = rng.integers(-4, 5, (T, 1, 1, 1))
    return base + noise + pump


def edge_clip(seed):
    """A vertical step edge from 60 to 140 at x = 4 + 2 t with +-3 levels of noise -> (clip, clean) int64 [T,H,W,3]."""
    rng = np.random.default_rng(seed)
    clean = np.full((T, H, W, 3), 60, np.int64)
    for t in range(T):
        clean[t, :, 4 + 2 * t:] = 140
    return clean + rng.integers(-3, 4, (T, H, W, 3)), clean


def temporal_difference(x):
    """The mean absolute frame-to-frame difference."""
    x = np.asarray(x, np.int64)
    return float(np.abs(x[1:] - x[:-1]).mean())


# ---- the restatement in place of flicker_hip's functions (device tensors in, device tensors out) ---------------------------------------------
def hip_window_pixels(patch, h, w):
    import torch
    return torch.from_numpy(window_pixels(patch.cpu().numpy(), int(h), int(w))).to(patch.device)


def hip_hold(win, offsets, mask2d, radius, tol, fixed=None, out=None):
    import torch
    o, s = hold(win.cpu().numpy(), offsets.cpu().numpy(), mask2d.cpu().numpy(), int(radius), int(tol))
    return torch.from_numpy(o).to(win.device), torch.from_numpy(s).to(win.device)
