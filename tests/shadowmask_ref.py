"""Helpers of the shadow-masking tests: the numpy / scipy restatement of rules 1 - 8 of include/vvshadow.h, written from
the header and independent of the product code, and the clip the tests share.  No test in here."""
import numpy as np
from scipy import ndimage

import platefill_ref as P

SQUARE = np.ones((3, 3), bool)
DEFAULTS = dict(guard=1, min_samples=4, tol=6, lo=30, hi=90, drop=12, chroma=20, floor=16, reach=32, min_area=16, grow=1)
PAIRS = ((0, 1), (1, 2), (0, 2))


def plate(frames, ns, min_samples, tol):
    """Rules 2 and 3: frames [T,H,W,3] u8, ns [T,H,W] bool (rule 1, complemented) -> (ok [H,W] bool, n2 [H,W], T1 [H,W,3]) int64, and the lit
    samples [T,H,W] bool."""
    v = np.asarray(frames).astype(np.int64)
    smp = ~ns
    L = v.sum(-1)
    n = smp.sum(0).astype(np.int64)
    S = (L * smp).sum(0)
    lit = smp & (n[None] * L + 3 * tol * n[None] >= S[None])
    n2 = lit.sum(0).astype(np.int64)
    w = v * lit[..., None]
    T1, T2 = w.sum(0), (w * w).sum(0)
    nn = n2[..., None]
    ok = (n2 >= min_samples) & (nn * T2 - T1 * T1 <= tol * tol * nn * nn).all(-1)
    return ok, n2, T1, lit


def candidates(frames, dil, ok, n2, T1, lo, hi, drop, chroma, floor):
    """Rule 4 -> cand [T,H,W] bool."""
    v = np.asarray(frames).astype(np.int64)
    n = n2[None, ..., None]
    t1 = T1[None]
    c = (np.asarray(dil) == 0) & ok[None]
    c &= (t1 >= floor * n).all(-1)
    c &= ((lo * t1 <= 100 * n * v) & (100 * n * v <= hi * t1)).all(-1)
    c &= (t1 - n * v).sum(-1) >= 3 * drop * n2[None]
    for a, b in PAIRS:
        c &= np.abs(v[..., a] * t1[..., b] - v[..., b] * t1[..., a]) * 100 * n2[None] <= chroma * t1[..., a] * t1[..., b]
    return c


def geodesic(a0, cand, reach):
    """Rule 5, sweep by sweep as the header states it: a0, cand [T,H,W] bool -> S = A_reach & ~A_0."""
    out = np.zeros_like(a0)
    for t in range(len(a0)):
        a = a0[t].copy()
        for _ in range(reach):
            nxt = a | (cand[t] & ndimage.binary_dilation(a, structure=SQUARE))
            if (nxt == a).all():
                break
            a = nxt
        out[t] = a & ~a0[t]
    return out


def drop_small(s, min_area):
    """Rule 6: 8-connected components of s [T,H,W] bool with fewer than min_area pixels are dropped."""
    if min_area <= 1:
        return s.copy()
    out = np.zeros_like(s)
    for t in range(len(s)):
        lab, k = ndimage.label(s[t], structure=SQUARE)
        if k:
            size = np.bincount(lab.ravel(), minlength=k + 1)
            keep = size >= min_area
            keep[0] = False
            out[t] = keep[lab]
    return out


def shadow_segment(frames, dil, guard=1, min_samples=4, tol=6, lo=30, hi=90, drop=12, chroma=20, floor=16, reach=32, min_area=16, grow=1,
                   detail=False):
    """One segment: frames [T,H,W,3] u8, dil [T,H,W] u8 -> (dil' u8 {0, 255}, counts [T,2] int64 = candidates, pixels added); detail=True adds
    a dict of the intermediate arrays."""
    frames, dil = np.asarray(frames), np.asarray(dil)
    T = len(frames)
    ns = P.not_sample(dil, guard)
    ok, n2, T1, lit = plate(frames, ns, min_samples, tol)
    cand = candidates(frames, dil, ok, n2, T1, lo, hi, drop, chroma, floor)
    a0 = dil != 0
    s = geodesic(a0, cand, reach)
    s6 = drop_small(s, min_area)
    s7 = P.dilate(s6, grow) & ~a0
    out = ((a0 | s7) * 255).astype(np.uint8)
    counts = np.stack([cand.reshape(T, -1).sum(1), s7.reshape(T, -1).sum(1)], axis=1).astype(np.int64)
    res = (out, counts)
    if detail:
        res += (dict(ns=ns, ok=ok, n2=n2, T1=T1, lit=lit, cand=cand, s=s, s6=s6, s7=s7),)
    return res


def shadow_mask(frames, dil, cuts=None, **cfg):
    """The whole clip: every segment of `cuts` on its own -> (dil', counts [T,2])."""
    frames, dil = np.asarray(frames), np.asarray(dil)
    dout, counts = np.zeros_like(dil), np.zeros((len(frames), 2), np.int64)
    for s, e in P.segments(len(frames), cuts):
        dout[s:e], counts[s:e] = shadow_segment(frames[s:e], dil[s:e], **cfg)
    return dout, counts


# ---- the shared clip --------------------------------------------------------------------------------------------------------------------------
def band_mask(T, H, W, rows=6, row0=19, width=20):
    """The shadow band under the box of platefill_ref.locked_off_clip: `rows` rows from row0, row r spanning `width` px from x0 + 2 r, with
    x0 = -8 + 2 t -> [T,H,W] bool."""
    band = np.zeros((T, H, W), bool)
    for t in range(T):
        x0 = -8 + 2 * t
        for r in range(rows):
            a, b = x0 + 2 * r, x0 + 2 * r + width
            band[t, row0 + r, max(a, 0):max(min(b, W), 0)] = True
    return band


def shadow_clip(seed=0, strength=60, T=24, H=40, W=56, a=6, band=None, gain=None):
    """platefill_ref.locked_off_clip(T, H, W, a, seed) with a shadow band (band_mask, or `band` [T,H,W] bool) added: the raw masks are taken out
    of the band, inside it every channel is v * strength // 100 (gain = three percentages: one per channel), dil = the masks dilated by 2 steps
    of the cross.  Returns (frames u8, dil u8 {0, 255}, band bool, clean int64, masks u8, logo bool)."""
    frames, masks, clean, boxm, logom = P.locked_off_clip(T=T, H=H, W=W, a=a, seed=seed)
    band = band_mask(T, H, W) if band is None else band
    band = band & (masks == 0)
    g = np.array(gain if gain is not None else (strength,) * 3, np.int64)
    frames = frames.copy()
    frames[band] = (frames[band].astype(np.int64) * g // 100).astype(np.uint8)
    dil = (P.dilate(masks != 0, 2) * 255).astype(np.uint8)
    return frames, dil, band, clean, masks, logom
