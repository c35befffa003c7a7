"""Seam tone matching restated in numpy / scipy, independently of the product's host code (videovanish_amd/tonematch.py) and kernels
(csrc/vv_tone.hip): the ring, the sums, the fit, the tables and the composite.  The resize and the feathered composite are the oracle's
(oracle/imageops_ref.py), which the image kernels equal byte for byte (tests/test_kernels_gpu.py)."""
import math

import numpy as np
from scipy import ndimage

from oracle import imageops_ref as I


def ring(mask, win, r):
    """mask [H,W] u8, win = (oy, ox, h, w) -> bool [H,W]: unmasked, inside the window, a mask pixel of the frame within the (2r+1)^2 box."""
    m = mask > 0
    near = ndimage.binary_dilation(m, structure=np.ones((2 * r + 1, 2 * r + 1), bool))        # outside the frame: nothing
    oy, ox, h, w = win
    inside = np.zeros_like(m)
    inside[max(oy, 0):oy + h, max(ox, 0):ox + w] = True
    return near & ~m & inside


def window_image(patch, h, w):
    """One frame of the model's output [Hm,Wm,3] as the window sees it [h,w,3]."""
    return I.resize_bilinear_u8(np.ascontiguousarray(patch), w, h)


def sums(patch, orig, mask, offsets, h, w, r):
    """patch [T,Hm,Wm,3], orig [T,H,W,3], mask [T,H,W], offsets [T,2] -> [T,16] int64."""
    out = np.zeros((len(patch), 16), np.int64)
    for t in range(len(patch)):
        oy, ox = (int(v) for v in offsets[t])
        sel = ring(mask[t], (oy, ox, h, w), r)
        x_full = np.zeros(orig[t].shape, np.int64)
        x_full[oy:oy + h, ox:ox + w] = window_image(patch[t], h, w)
        x, y = x_full[sel], orig[t][sel].astype(np.int64)
        out[t] = [len(x), *x.sum(0), *y.sum(0), *(x * x).sum(0), *(x * y).sum(0), *(y * y).sum(0)] if len(x) else 0
    return out


def fit(s, mode="affine", smooth=2, max_gain=1.25, max_offset=32.0, min_count=64, min_var=4.0):
    """s [T,16] integers -> (gain [T,3], offset [T,3]) float64, in Python integers and floats, frame by frame."""
    T = len(s)
    gain, offset = np.ones((T, 3)), np.zeros((T, 3))
    rows = [[int(v) for v in row] for row in s]
    for t in range(T):
        p = [sum(rows[u][k] for u in range(max(0, t - smooth), min(T, t + smooth + 1))) for k in range(16)]
        if rows[t][0] == 0 or p[0] < min_count:
            continue
        n = float(p[0])
        for c in range(3):
            xm, ym = p[1 + c] / n, p[4 + c] / n
            vx = p[7 + c] / n - xm * xm
            cxy = p[10 + c] / n - xm * ym
            if mode == "offset" or vx < min_var or vx <= 0.0:
                g = 1.0
            else:
                g = min(max(cxy / vx, 1.0 / max_gain), max_gain)
            gain[t, c] = g
            offset[t, c] = min(max(ym - g * xm, -max_offset), max_offset)
    return gain, offset


def tables(gain, offset):
    """[T,3] each -> [T,3,256] u8."""
    out = np.zeros((len(gain), 3, 256), np.uint8)
    for t in range(len(gain)):
        for c in range(3):
            for v in range(256):
                out[t, c, v] = min(max(int(np.rint(gain[t, c] * v + offset[t, c])), 0), 255)
    return out


def rms(s, gain, offset):
    """(rms of y - x, rms of y - (g x + o)) [T,3] each over every frame's own ring, from its own sums; 0 where the ring is empty."""
    T = len(s)
    before, after = np.zeros((T, 3)), np.zeros((T, 3))
    for t in range(T):
        n = int(s[t][0])
        for c in range(3):
            if n:
                sx, sy, sxx, sxy, syy = (float(s[t][k + c]) for k in (1, 4, 7, 10, 13))
                g, o = gain[t, c], offset[t, c]
                before[t, c] = math.sqrt(max((syy - 2 * sxy + sxx) / n, 0.0))
                after[t, c] = math.sqrt(max((syy - 2 * g * sxy - 2 * o * sy + g * g * sxx + 2 * g * o * sx + n * o * o) / n, 0.0))
    return before, after


def composite(patch, orig, mask, offsets, lut, h, w, feather):
    """The fused paste with a table: resize, look up, paste at the offset, feathered composite with the full-frame mask (feather < 0: the paste)."""
    out = np.empty_like(orig)
    for t in range(len(patch)):
        oy, ox = (int(v) for v in offsets[t])
        x = window_image(patch[t], h, w)
        x = np.stack([lut[t, c][x[..., c]] for c in range(3)], axis=-1)
        pasted = orig[t].copy()
        pasted[oy:oy + h, ox:ox + w] = x
        out[t] = pasted if feather < 0 else I.composite(pasted, orig[t], I.feather_alpha(mask[t], feather))
    return out


def apply(patch, orig, mask, offsets, h, w, feather, **cfg):
    """The whole stage for one window: (composite, sums, gain, offset)."""
    r = cfg.pop("ring", 12)
    s = sums(patch, orig, mask, offsets, h, w, r)
    gain, offset = fit(s, **cfg)
    return composite(patch, orig, mask, offsets, tables(gain, offset), h, w, feather), s, gain, offset


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def smooth_texture(seed, H, W, lo=20, hi=220):
    """A smooth [H,W,3] u8 image with values in lo .. hi that uses the whole range: a few low-frequency waves per channel."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    img = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(4):
            fy, fx, ph = rng.uniform(0.02, 0.12), rng.uniform(0.02, 0.12), rng.uniform(0, 2 * np.pi)
            img[..., c] += rng.uniform(0.5, 1.0) * np.sin(fy * yy + fx * xx + ph)
        img[..., c] = (img[..., c] - img[..., c].min()) / (img[..., c].max() - img[..., c].min())
    return np.rint(lo + (hi - lo) * img).astype(np.uint8)


RESTORE_CASES = ((0.9, 10), (1.1, -10), (1.0, 6), (0.85, 20), (1.2, -25))


def restoration_clip(a, b, T=3, H=96, W=130, box=(30, 50), at=(33, 40), seed=0):
    """(orig [T,H,W,3], x = clip(rint(a orig + b)) [T,H,W,3], mask [T,H,W] with one box of `box` pixels at `at`)."""
    orig = np.stack([smooth_texture(seed + 17 * t, H, W) for t in range(T)])
    x = np.clip(np.rint(a * orig.astype(np.float64) + b), 0, 255).astype(np.uint8)
    mask = np.zeros((T, H, W), np.uint8)
    mask[:, at[0]:at[0] + box[0], at[1]:at[1] + box[1]] = 255
    return orig, x, mask
