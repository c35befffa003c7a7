"""Seam grain matching restated in numpy / scipy, independently of the product's host code (videovanish_amd/grainmatch.py) and kernels
(csrc/vv_grain.hip): the ring, the selection, the sums, the fit, the tables, the noise and the composite.  The resize and
the feathered composite are the oracle's (oracle/imageops_ref.py), which the image kernels equal byte for byte (tests/test_kernels_gpu.py)."""
import math
import os
import sys

import numpy as np
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tonematch_ref as TR  # noqa: E402

from oracle import imageops_ref as I  # noqa: E402

K = np.array([[1, -2, 1], [-2, 4, -2], [1, -2, 1]], np.int64)      # Immerkaer's operator: zero on planes, variance 36 sigma^2 on white noise
IDENT = np.broadcast_to(np.arange(256, dtype=np.uint8), (3, 256))
BOX = np.ones((3, 3), bool)


def looked_up(patch_t, lut_t, h, w):
    """One frame of the model's output [Hm,Wm,3] as the window sees it [h,w,3], after the table [3,256]."""
    x = TR.window_image(patch_t, h, w)
    return np.stack([lut_t[c][x[..., c]] for c in range(3)], axis=-1)


def selection(x_full, mask, win, r, flat):
    """x_full [H,W,3] (the window's pixels at their place in the frame, anything elsewhere), mask [H,W], win = (oy, ox, h, w) -> bool [H,W,3]:
    (a) in the ring, (b) the 3 x 3 neighbourhood inside the window and the frame and unmasked, (c) max - min of x_c over it <= flat."""
    oy, ox, h, w = win
    free = np.zeros(mask.shape, bool)
    free[max(oy, 0):oy + h, max(ox, 0):ox + w] = True
    free &= mask == 0
    near = ndimage.maximum_filter((mask != 0).astype(np.uint8), size=2 * r + 1, mode="constant", cval=0) > 0       # outside the frame: nothing
    ab = near & free & ndimage.binary_erosion(free, structure=BOX, border_value=0)
    x = x_full.astype(np.int64)
    spread = ndimage.maximum_filter(x, size=(3, 3, 1), mode="nearest") - ndimage.minimum_filter(x, size=(3, 3, 1), mode="nearest")
    return ab[..., None] & (spread <= flat)


def noise_response(img):
    """img [H,W,3] -> L [H,W,3] int64 (the border rows and columns are never selected)."""
    return ndimage.correlate(img.astype(np.int64), K[:, :, None], mode="constant", cval=0)


def sums(patch, orig, mask, offsets, lut, h, w, r, flat):
    """patch [T,Hm,Wm,3], orig [T,H,W,3], mask [T,H,W], offsets [T,2], lut [T,3,256] -> [T,36] int64 = [T][c][band][n, Sx, Sy]."""
    out = np.zeros((len(patch), 3, 4, 3), np.int64)
    for t in range(len(patch)):
        oy, ox = (int(v) for v in offsets[t])
        x_full = np.zeros(orig[t].shape, np.uint8)
        x_full[oy:oy + h, ox:ox + w] = looked_up(patch[t], lut[t], h, w)
        sel = selection(x_full, mask[t], (oy, ox, h, w), r, flat)
        lx, ly = noise_response(x_full), noise_response(orig[t])
        for c in range(3):
            for b in range(4):
                pick = sel[..., c] & (x_full[..., c] // 64 == b)
                out[t, c, b] = [pick.sum(), (lx[..., c][pick] ** 2).sum(), (ly[..., c][pick] ** 2).sum()]
    return out.reshape(len(patch), 36)


def fit(s, smooth=4, strength=1.0, max_sigma=12.0, min_count=256):
    """s [T,36] integers -> (sigma_orig, sigma_model, sigma_added) [T,3,4] float64 each, in Python integers and floats, frame by frame."""
    T = len(s)
    rows = [[int(v) for v in row] for row in np.asarray(s).reshape(T, 36)]
    so, sm, sa = np.zeros((T, 3, 4)), np.zeros((T, 3, 4)), np.zeros((T, 3, 4))
    for t in range(T):
        if sum(rows[t][0::3]) == 0:
            continue
        p = [sum(rows[u][k] for u in range(max(0, t - smooth), min(T, t + smooth + 1))) for k in range(36)]
        for c in range(3):
            chan = [sum(p[(c * 4 + b) * 3 + k] for b in range(4)) for k in range(3)]
            for b in range(4):
                n, sx, sy = p[(c * 4 + b) * 3:(c * 4 + b) * 3 + 3]
                if n < min_count:
                    n, sx, sy = chan
                if n < min_count:
                    continue
                so[t, c, b] = math.sqrt(sy / (36.0 * n))
                sm[t, c, b] = math.sqrt(sx / (36.0 * n))
                sa[t, c, b] = min(strength * math.sqrt(max(sy - sx, 0) / (36.0 * n)), max_sigma)
    return so, sm, sa


def tables(sigma_added):
    """[T,3,4] -> [T,3,256] u8: rint(16 sigma(v)), sigma(v) linear between the centres 32, 96, 160, 224, flat beyond."""
    out = np.zeros((len(sigma_added), 3, 256), np.uint8)
    for t in range(len(sigma_added)):
        for c in range(3):
            s = [float(v) for v in sigma_added[t, c]]
            for v in range(256):
                if v <= 32:
                    at = s[0]
                elif v >= 224:
                    at = s[3]
                else:
                    k = (v - 32) // 64
                    f = (v - 32 - 64 * k) / 64.0
                    at = s[k] * (1.0 - f) + s[k + 1] * f
                out[t, c, v] = min(max(int(np.rint(16.0 * at)), 0), 255)
    return out


def noise(seed, frame_id, H, W, mode):
    """s [H,W,3] int64 of one frame: the centred byte sum of splitmix64's finaliser of the pixel's key (include/vvgrain.h)."""
    u = np.uint64
    yy, xx = np.mgrid[:H, :W].astype(np.uint64)
    with np.errstate(over="ignore"):
        key = (u(seed) << u(32)) ^ ((u(frame_id) * u(H) + yy) * u(W) + xx)
        keys = [key, key, key] if mode == "luma" else [key * u(3) + u(c) for c in range(3)]
        out = []
        for z in keys:
            z = z + u(0x9E3779B97F4A7C15)
            z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
            z = z ^ (z >> u(31))
            out.append(sum(((z >> u(8 * k)) & u(255)).astype(np.int64) for k in range(8)) - 1020)
    return np.stack(out, axis=-1)


def grain(img, amp_t, s):
    """img [h,w,3] u8, amp_t [3,256] u8, s [h,w,3] int64 -> clip(img + d), d = (amp s 5017 + 2^23) >> 24 (an arithmetic shift: a floor)."""
    a = np.stack([amp_t[c][img[..., c]] for c in range(3)], axis=-1).astype(np.int64)
    d = (a * s * 5017 + (1 << 23)) >> 24
    return np.clip(img.astype(np.int64) + d, 0, 255).astype(np.uint8), d


def composite(patch, orig, mask, offsets, lut, amp, frame_ids, seed, mode, h, w, feather):
    """The fused paste with a table and grain: resize, look up, add the noise of the pixel's frame position, paste at the offset, feathered
    composite with the full-frame mask (feather < 0: the paste)."""
    out = np.empty_like(orig)
    H, W = orig.shape[1:3]
    for t in range(len(patch)):
        oy, ox = (int(v) for v in offsets[t])
        s = noise(seed, int(frame_ids[t]), H, W, mode)[oy:oy + h, ox:ox + w]
        x, _ = grain(looked_up(patch[t], lut[t], h, w), amp[t], s)
        pasted = orig[t].copy()
        pasted[oy:oy + h, ox:ox + w] = x
        out[t] = pasted if feather < 0 else I.composite(pasted, orig[t], I.feather_alpha(mask[t], feather))
    return out


def apply(patch, orig, mask, offsets, h, w, feather, frame_ids, tone=None, mode="luma", ring=12, flat=24, seed=0, **fitkw):
    """The whole stage for one window: (composite, sums, sigma_orig, sigma_model, sigma_added); tone = the keywords of tonematch_ref.fit (with
    ring) when tone matching runs in front."""
    lut = np.broadcast_to(IDENT, (len(patch), 3, 256))
    if tone is not None:
        tone = dict(tone)
        ts = TR.sums(patch, orig, mask, offsets, h, w, tone.pop("ring", 12))
        lut = TR.tables(*TR.fit(ts, **tone))
    s = sums(patch, orig, mask, offsets, lut, h, w, ring, flat)
    so, sm, sa = fit(s, **fitkw)
    return composite(patch, orig, mask, offsets, lut, tables(sa), frame_ids, seed, mode, h, w, feather), s, so, sm, sa


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
RECOVERY_SIGMAS = (2, 4, 8)
RECOVERY_SEEDS = tuple(range(12))


def recovery_clip(s, sigma):
    """(orig, x, mask) [1,96,130,...]: x = tonematch_ref.restoration_clip(1.0, 0, T=1, seed=s), the smooth clip, as the model's frame; orig = x
    plus seeded Gaussian noise of `sigma`, rounded and clipped."""
    smooth, _, mask = TR.restoration_clip(1.0, 0, T=1, seed=s)
    g = np.random.default_rng(7919 * s + sigma).normal(0.0, float(sigma), smooth.shape) if sigma else 0.0
    return np.clip(np.rint(smooth + g), 0, 255).astype(np.uint8), smooth, mask


def inside_estimate(out_t, x_t, mask_t):
    """Immerkaer's estimate [3] of the noise the composite out_t carries over the model's frame x_t on the pixels
    at least four pixels deep in the mask, where a feather of up to 3 leaves the pasted bytes as they are: sqrt((sum L(out)^2 - sum L(x)^2) / (36 n))."""
    core = ndimage.binary_erosion(mask_t > 0, structure=np.ones((9, 9), bool), border_value=0)
    lo, lx = noise_response(out_t), noise_response(x_t)
    return np.sqrt(np.maximum((lo[core] ** 2).sum(0) - (lx[core] ** 2).sum(0), 0) / (36.0 * core.sum()))


# The worst relative deviation |estimate / sigma - 1| of this restatement with the default settings (luma, ring 12, flat 24, min_count 256,
# strength 1, seed 0) over recovery_clip(s, sigma), s = 0 .. 11, the three channels and the four bands (144 values per sigma), measured by
# tests/test_grainmatch_cpu.py::test_reference_recovers_a_known_grain (which prints them): "fit" of sigma_added, "inside" of inside_estimate on
# the composite at feather 3.  The tests assert 1.5 times these.
MEASURED_DEVIATION = {
    "fit": {2: 0.1509, 4: 0.1768, 8: 0.2072},
    "inside": {2: 0.0893, 4: 0.1079, 8: 0.0912},
}
