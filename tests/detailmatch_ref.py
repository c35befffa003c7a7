"""Seam detail matching restated from include/detailmatch.h in numpy int64 / scipy and Python integers, independently of the product's host code
(videovanish_amd/detailmatch.py) and kernels (csrc/vv_detail.hip): the ring, the 5 x 5 gate, the sums, the fit, the clamped unsharp mask; the
synthetic clips the rule is judged on; and the restatement in the shape of videovanish_amd/detailmatch_bind.py's two functions (for tests that
replace them).  The resize is the oracle's (oracle/imageops_ref.py), which the image kernels equal byte for byte (tests/test_kernels_gpu.py)."""
import math
from fractions import Fraction

import numpy as np
from scipy import ndimage

from oracle import imageops_ref as I

DEFAULTS = dict(ring=8, edge=12, smooth=2, min_pixels=256, max_sharpen=2.0, max_soften=1.0, dead=0.06, overshoot=4, strength=1.0)
NSUM = 12
MAX_AMOUNT = 1024
B = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.int64)


def window_image(patch_t, h, w):
    """One frame of the model's output [Hm,Wm,3] as the window sees it [h,w,3] int64."""
    patch_t = np.ascontiguousarray(patch_t, np.uint8)
    return (patch_t if patch_t.shape[:2] == (h, w) else I.resize_bilinear_u8(patch_t, w, h)).astype(np.int64)


def highpass(img, mode="constant"):
    """H(I) = 16 I - B * I on [h,w,3] int64; outside the array 0 ("constant": never a tap of a counted pixel) or the edge pixel ("nearest")."""
    return 16 * img - ndimage.correlate(img, B[:, :, None], mode=mode, cval=0)


def from_frame(a, oy, ox, h, w):
    """Frame array a [H,W,...] seen from the window at (oy, ox): (values [h,w,...] with 0 outside the frame, inside-the-frame flags [h,w])."""
    H, W = a.shape[:2]
    yy, xx = oy + np.arange(h), ox + np.arange(w)
    valid = ((yy >= 0) & (yy < H))[:, None] & ((xx >= 0) & (xx < W))[None, :]
    v = a[np.clip(yy, 0, H - 1)[:, None], np.clip(xx, 0, W - 1)[None, :]]
    return np.where(valid.reshape(valid.shape + (1,) * (v.ndim - 2)), v, np.zeros((), v.dtype)), valid


def selection(x, mask_t, oy, ox, r, edge):
    """x [h,w,3] int64 (the window's pixels), mask_t [H,W] -> bool [h,w,3]: (a) in the ring, (b) the 5 x 5 neighbourhood inside the window and the
    frame and unmasked, (c) max - min of x_c over the 3 x 3 neighbourhood >= edge."""
    h, w = x.shape[:2]
    m = mask_t != 0
    near = ndimage.maximum_filter(m.astype(np.uint8), size=2 * r + 1, mode="constant", cval=0) > 0        # outside the frame: nothing
    near_w, valid = from_frame(near, oy, ox, h, w)
    m_w, _ = from_frame(m, oy, ox, h, w)
    free = valid & ~m_w
    ab = near_w & free & ndimage.binary_erosion(free, structure=np.ones((5, 5), bool), border_value=0)
    spread = ndimage.maximum_filter(x, size=(3, 3, 1), mode="nearest") - ndimage.minimum_filter(x, size=(3, 3, 1), mode="nearest")
    return ab[..., None] & (spread >= edge)


def sums(patch, orig, mask, offsets, h, w, r, edge):
    """Rule 1: patch [T,Hm,Wm,3], orig [T,H,W,3], mask [T,H,W], offsets [T,2] -> [T,12] int64 = [T][c][n, sum D K, sum K K, sum D D]."""
    out = np.zeros((len(patch), 3, 4), np.int64)
    for t in range(len(patch)):
        oy, ox = (int(v) for v in offsets[t])
        x = window_image(patch[t], h, w)
        y, _ = from_frame(np.asarray(orig[t]).astype(np.int64), oy, ox, h, w)
        sel = selection(x, np.asarray(mask[t]), oy, ox, r, edge)
        hx = highpass(x)
        D, K = highpass(y) - hx, highpass(hx)
        for c in range(3):
            d, k = D[..., c][sel[..., c]], K[..., c][sel[..., c]]
            out[t, c] = [len(d), (d * k).sum(), (k * k).sum(), (d * d).sum()]
    return out.reshape(len(patch), NSUM)


def q(v):
    return math.floor(Fraction(256) * Fraction(v) + Fraction(1, 2))


def fit(s, smooth=2, min_pixels=256, max_sharpen=2.0, max_soften=1.0, dead=0.06, strength=1.0, **_):
    """Rule 2: s [T,12] integers -> (q8 amounts, clamped flags, dead flags), lists over the frames, in Python integers and fractions."""
    rows = [[int(v) for v in row] for row in np.asarray(s).reshape(-1, NSUM)]
    T = len(rows)
    amounts, clamped, deads = [], [], []
    for t in range(T):
        pool = [sum(rows[u][c * 4 + k] for u in range(max(0, t - smooth), min(T, t + smooth + 1)) for c in range(3)) for k in range(4)]
        count, P, Q = pool[0], pool[1], pool[2]
        a, cl, de = 0, False, False
        if count // 3 >= min_pixels and Q != 0:
            a = math.floor(Fraction(4096 * P, Q) + Fraction(1, 2))
            lo, hi = -q(max_soften), q(max_sharpen)
            cl = a < lo or a > hi
            a = min(max(a, lo), hi)
            if abs(a) < q(dead):
                a, de = 0, True
            else:
                a = math.floor(Fraction(a * q(strength) + 128, 256))
        amounts.append(a)
        clamped.append(cl)
        deads.append(de)
    return amounts, clamped, deads


def sharpen(patch, amount, h, w, overshoot):
    """Rule 3: patch [T,Hm,Wm,3] u8, amount [T] integers (q8) -> [T,h,w,3] u8."""
    out = np.empty((len(patch), h, w, 3), np.uint8)
    for t in range(len(patch)):
        x = window_image(patch[t], h, w)
        a = min(max(int(amount[t]), -MAX_AMOUNT), MAX_AMOUNT)
        lo = ndimage.minimum_filter(x, size=(3, 3, 1), mode="nearest")
        hi = ndimage.maximum_filter(x, size=(3, 3, 1), mode="nearest")
        v = (4096 * x + a * highpass(x, "nearest") + 2048) >> 12
        out[t] = np.clip(np.clip(v, lo - overshoot, hi + overshoot), 0, 255)
    return out


def apply(patch, orig, mask, offsets, h, w, **cfg):
    """The whole stage for one window: (the sharpened window pixels [T,h,w,3], sums [T,12], q8 amounts, clamped, dead)."""
    cfg = dict(DEFAULTS, **cfg)
    s = sums(patch, orig, mask, offsets, h, w, cfg["ring"], cfg["edge"])
    amounts, clamped, dead = fit(s, **cfg)
    return sharpen(patch, amounts, h, w, cfg["overshoot"]), s, amounts, clamped, dead


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
H, W = 64, 96               # the synthetic clips
BOX = (20, 28, 44, 68)      # the mask: y0, x0, y1, x1


def texture(seed, h=H, w=W):
    """A structured [h,w,3] image in float64 inside 40 .. 215: low-frequency waves under a mosaic of 4 x 4 blocks with sharp edges (+-35 levels)
    and a pixel-sized weave (+-10 levels): detail up to the top octave, as a focused image of a textured surface has."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(4):
            f, th, ph = rng.uniform(0.02, 0.1), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
            img[..., c] += 13.0 * rng.uniform(0.5, 1.0) * np.sin(f * (np.cos(th) * yy + np.sin(th) * xx) + ph)
        blocks = rng.uniform(-35.0, 35.0, (-(-h // 4), -(-w // 4)))
        img[..., c] += np.kron(blocks, np.ones((4, 4)))[:h, :w] + rng.uniform(-10.0, 10.0, (h, w))
    return np.clip(127.5 + img, 40.0, 215.0)


def blur(img):
    """The 3 x 3 binomial mean of a float image, edges replicated."""
    return ndimage.correlate(img, B[:, :, None].astype(np.float64) / 16.0, mode="nearest")


def box_mask(h=H, w=W, box=BOX):
    m = np.zeros((h, w), np.uint8)
    m[box[0]:box[2], box[1]:box[3]] = 255
    return m


def detail_clip(kind, seed, grain=0):
    """(orig [1,H,W,3] u8, model [1,H,W,3] u8, mask [1,H,W] u8, the clean truth the model's frame should show [H,W,3] float64).  kind "soft":
    the model is the binomial blur of the original; "crisp": the original is the binomial blur of the model; "same": the model is the
    original.  The model carries +-1 level of noise, the original `grain` levels (uniform, +-grain)."""
    rng = np.random.default_rng(1000 * seed + 17)
    tex = texture(seed)
    sharp, soft = tex, blur(tex)
    truth, model = {"soft": (sharp, soft), "crisp": (soft, sharp), "same": (sharp, sharp)}[kind]
    orig = truth + (rng.integers(-grain, grain + 1, truth.shape) if grain else 0)
    if kind == "same":
        model = np.clip(np.rint(orig), 0, 255)
    model = model + rng.integers(-1, 2, model.shape)
    u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return u8(orig)[None], u8(model)[None], box_mask()[None], truth


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


# ---- the restatement in place of detailmatch_bind's functions (device tensors in, device tensors out) ------------------------------------------
def hip_ring_detail_stats(patch, orig, mask2d, offsets, h, w, ring, edge):
    import torch
    s = sums(patch.cpu().numpy(), orig.cpu().numpy(), mask2d.cpu().numpy(), offsets.cpu().numpy(), int(h), int(w), int(ring), int(edge))
    return torch.from_numpy(s).to(patch.device)


def hip_sharpen(patch, amount, h, w, overshoot, out=None):
    import torch
    return torch.from_numpy(sharpen(patch.cpu().numpy(), amount.cpu().numpy(), int(h), int(w), int(overshoot))).to(patch.device)
