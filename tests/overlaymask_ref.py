"""Overlay masking restated in numpy / scipy.ndimage from include/overlaymask.h, independent of the product code, and the clips the tests share.
Every array is a host array; every function follows one rule of the header and keeps its integer arithmetic (int64 throughout)."""
import numpy as np
from scipy import ndimage

DEFAULTS = dict(min_samples=12, mag=8, coh=80, max_share=25, close=2, max_hole=4096, min_area=64, max_area=10, border=0, grow=3)
MAX_BOXES = 256
CROSS = ndimage.generate_binary_structure(2, 1)
SQUARE = np.ones((3, 3), bool)


# ---- rule 1 -------------------------------------------------------------------------------------------------------------------------------
def luma(frames):
    f = frames.astype(np.int64)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def gradients(frames):
    """frames [T,H,W,3] u8 -> (gx, gy) [T,H,W] int64: the 3 x 3 Sobel responses of the luma, the frame's border replicated."""
    Y = np.pad(luma(frames), ((0, 0), (1, 1), (1, 1)), mode="edge")
    at = lambda dy, dx: Y[:, 1 + dy:Y.shape[1] - 1 + dy, 1 + dx:Y.shape[2] - 1 + dx]
    gx = at(-1, 1) + 2 * at(0, 1) + at(1, 1) - at(-1, -1) - 2 * at(0, -1) - at(1, -1)
    gy = at(1, -1) + 2 * at(1, 0) + at(1, 1) - at(-1, -1) - 2 * at(-1, 0) - at(-1, 1)
    return gx, gy


def accumulate(frames, dil):
    """-> acc [H,W,4] int64 = (n, Sx, Sy, A) over the frames with dil == 0."""
    gx, gy = gradients(frames)
    c = (dil == 0).astype(np.int64)
    return np.stack([c.sum(0), (gx * c).sum(0), (gy * c).sum(0), ((np.abs(gx) + np.abs(gy)) * c).sum(0)], axis=-1)


# ---- rule 2 -------------------------------------------------------------------------------------------------------------------------------
def classify(acc, min_samples, mag, coh):
    """-> (strong, E) [H,W] bool"""
    n, Sx, Sy, A = (acc[..., k].astype(np.int64) for k in range(4))
    strong = (n >= min_samples) & (A >= mag * n)
    return strong, strong & (100 * (np.abs(Sx) + np.abs(Sy)) >= coh * A)


# ---- rules 4 to 7 -------------------------------------------------------------------------------------------------------------------------
def dilate(m, k):
    """m dilated k times with the 3 x 3 cross, nothing set outside the frame"""
    return ndimage.binary_dilation(m, structure=CROSS, iterations=k) if k > 0 else m.copy()


def labels(m):
    """m [H,W] bool -> int32 [H,W]: the smallest linear index of the pixel's 8-connected component, -1 outside m"""
    lab, n = ndimage.label(m, structure=SQUARE)
    out = np.full(m.shape, -1, np.int32)
    if n:
        lin = np.arange(m.size, dtype=np.int64).reshape(m.shape)
        first = np.asarray(ndimage.minimum(lin, lab, index=np.arange(1, n + 1))).astype(np.int64)
        out[m] = first[lab[m] - 1]
    return out


def component_stats(lab):
    """lab = labels(m) -> stats [H*W,5] int32: (area, x0, y0, x1, y1) at a component's label, (0, W, H, 0, 0) elsewhere"""
    H, W = lab.shape
    stats = np.tile(np.array([0, W, H, 0, 0], np.int32), (H * W, 1))
    ys, xs = np.nonzero(lab >= 0)
    l = lab[ys, xs].astype(np.int64)
    np.add.at(stats[:, 0], l, 1)
    np.minimum.at(stats[:, 1], l, xs.astype(np.int32))
    np.minimum.at(stats[:, 2], l, ys.astype(np.int32))
    np.maximum.at(stats[:, 3], l, (xs + 1).astype(np.int32))
    np.maximum.at(stats[:, 4], l, (ys + 1).astype(np.int32))
    return stats


def select(lab, stats, min_area, max_area_px, inside_only):
    """-> (out [H,W] bool, boxes [K,6] int32 = (label, area, x0, y0, x1, y1) of every kept component in label order)"""
    H, W = lab.shape
    a, x0, y0, x1, y1 = (stats[:, k].astype(np.int64) for k in range(5))
    keep = (a > 0) & (a >= min_area) & (a <= max_area_px)
    if inside_only:
        keep &= (x0 > 0) & (y0 > 0) & (x1 < W) & (y1 < H)
    out = np.zeros((H, W), bool)
    inside = lab >= 0
    out[inside] = keep[lab[inside]]
    roots = np.nonzero(keep)[0]
    return out, np.concatenate([roots[:, None].astype(np.int32), stats[roots]], axis=1).astype(np.int32).reshape(-1, 6)


def kept_parts(m, min_area, max_area_px, inside_only):
    lab = labels(m)
    return select(lab, component_stats(lab), min_area, max_area_px, inside_only)


def overlay(frames, dil, **cfg):
    """The whole rule on one clip call -> dict(verdict, strong, edges, acc, E, C, F, kept, O, boxes [K,5] = (x0, y0, x1, y1, area) (at most 256),
    found, dil2 [T,H,W] u8, added [T] int64)."""
    c = dict(DEFAULTS, **cfg)
    T, H, W = dil.shape
    acc = accumulate(frames, dil)
    strong, E = classify(acc, c["min_samples"], c["mag"], c["coh"])
    res = dict(strong=int(strong.sum()), edges=int(E.sum()), acc=acc, E=E, O=np.zeros((H, W), bool), boxes=np.zeros((0, 5), np.int32), found=0,
               dil2=dil, added=np.zeros(T, np.int64))
    if res["strong"] == 0:
        return dict(res, verdict="none")
    if 100 * res["edges"] > c["max_share"] * res["strong"]:
        return dict(res, verdict="static")
    C = dilate(E, c["close"])
    holes, _ = kept_parts(~C, 0, c["max_hole"], True)
    F = C | holes
    kept, boxes = kept_parts(F, c["min_area"], c["max_area"] * H * W // 100, not c["border"])
    res.update(C=C, F=F, kept=kept)
    if len(boxes) == 0:
        return dict(res, verdict="none")
    O = dilate(kept, c["grow"])
    masked = dil != 0
    return dict(res, verdict="found", O=O, boxes=boxes[:MAX_BOXES][:, [2, 3, 4, 5, 1]], found=len(boxes),
                dil2=((masked | O[None]) * 255).astype(np.uint8), added=(O[None] & ~masked).reshape(T, -1).sum(1).astype(np.int64))


# ---- the shared clips ---------------------------------------------------------------------------------------------------------------------
LOGO_AT, LOGO_SIZE = (14, 72), (16, 40)


def background(seed, H, W, travel):
    """Gaussian-filtered noise (sigma 2) stretched to 28 .. 228, [H, W + travel] float"""
    rng = np.random.default_rng(seed)
    g = ndimage.gaussian_filter(rng.standard_normal((H, W + travel)), 2.0)
    return 28.0 + 200.0 * (g - g.min()) / (g.max() - g.min())


def logo_mask(H, W, at=LOGO_AT, size=LOGO_SIZE):
    m = np.zeros((H, W), bool)
    m[at[0]:at[0] + size[0], at[1]:at[1] + size[1]] = True
    return m


def overlay_clip(seed=0, alpha=1.0, T=24, H=96, W=128, speed=3, noise=2.0, logo=True, band=None):
    """A background that pans `speed` px a frame under sensor noise of sigma `noise`, with a 16 x 40 logo (a 4-px checker of 40 / 230, blended at
    `alpha`) fixed on the screen; band = (y0, y1): those rows darkened to 30 % across the whole width, fixed on the screen (a horizon under a
    horizontal pan).  speed = 0 is the locked-off version.  -> (frames [T,H,W,3] u8, the logo's pixels [H,W] bool)."""
    bg = background(seed, H, W, speed * T)
    rng = np.random.default_rng(seed + 1000)
    lm = logo_mask(H, W) if logo else np.zeros((H, W), bool)
    yy, xx = np.mgrid[0:H, 0:W]
    checker = np.where(((yy // 4) + (xx // 4)) % 2 == 0, 40.0, 230.0)
    frames = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        v = bg[:, speed * t:speed * t + W].copy()
        if band is not None:
            v[band[0]:band[1]] *= 0.3
        v[lm] = (1.0 - alpha) * v[lm] + alpha * checker[lm]
        frames[t] = np.clip(np.rint(v[..., None] + noise * rng.standard_normal((H, W, 3))), 0, 255).astype(np.uint8)
    return frames, lm


def far_from(m, px):
    """the pixels further than px (3 x 3 square steps) from every pixel of m"""
    return ~ndimage.binary_dilation(m, structure=SQUARE, iterations=px) if px > 0 else ~m
