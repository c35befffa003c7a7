"""Helpers of the clean-plate exposure matching tests: the restatement of rules 1 - 6 of include/platetone.h, written from
the header and independent of the product code -- numpy for the planes and the sums, Python integers and fractions for the fit and the tables
-- built on platefill_ref / plategrain_ref for the fill itself, and the clips the tests share.  No test in here."""
from fractions import Fraction

import numpy as np

import platefill_ref as R
import plategrain_ref as G

DEFAULTS = dict(mode="affine", ring=32, floor=16, min_pixels=1024, max_gain=25, max_offset=32)
IDENT = np.arange(256, dtype=np.uint8)


# ---- rule 1 -----------------------------------------------------------------------------------------------------------------------------------
def crop(dil, ring, align=4):
    """The union box of the masks of one segment, x aligned to 4, widened by ring, clamped, x aligned again -> (y0, x0, y1, x1) or None."""
    T, H, W = dil.shape
    ys, xs = np.nonzero((dil != 0).any(0).any(1))[0], np.nonzero((dil != 0).any(0).any(0))[0]
    if not len(ys):
        return None
    y0, y1, x0, x1 = ys[0], ys[-1] + 1, xs[0], xs[-1] + 1
    x0, x1 = x0 - x0 % align, min(W, -(-x1 // align) * align)
    y0, y1, x0, x1 = max(y0 - ring, 0), min(y1 + ring, H), max(x0 - ring, 0), min(x1 + ring, W)
    return int(y0), int(x0 - x0 % align), int(y1), int(min(W, -(-x1 // align) * align))


# ---- rules 2 and 3 ----------------------------------------------------------------------------------------------------------------------------
def mean_plane(frames, ns, floor):
    """frames [T,h,w,3] u8, ns [T,h,w] bool -> (R [h,w,3] u8, U [h,w] bool, n)."""
    T = len(frames)
    P = frames.astype(np.int64).sum(0)
    Rm = (2 * P + T) // (2 * T)
    U = ~ns.any(0) & ((Rm >= floor) & (Rm <= 255 - floor)).all(-1)
    return Rm.astype(np.uint8), U, int(U.sum())


def moments(frames, Rm, U):
    """-> [T][12] Python integers: Sv[3], Svr[3], and on row 0 Sr[3], Srr[3] (zeros on the other rows)."""
    r = Rm.astype(np.int64)[U]                                   # [n,3]
    rows = []
    for t, f in enumerate(frames):
        v = f.astype(np.int64)[U]
        first = t == 0
        rows.append([int(x) for x in v.sum(0)] + [int(x) for x in (v * r).sum(0)] + [int(x) * first for x in r.sum(0)] + [int(x) * first for x in (r * r).sum(0)])
    return rows


# ---- rules 4 and 5 ----------------------------------------------------------------------------------------------------------------------------
def fit(n, Sv, Svr, Sr, Srr, mode, max_gain, max_offset):
    """-> (a, b) as Fractions, clamped."""
    if mode == "affine":
        N, D = n * Svr - Sv * Sr, n * Srr - Sr * Sr
        if D < 16 * n * n:
            mode = "gain"
        else:
            a = Fraction(N, D)
    if mode == "gain":
        a = Fraction(Sv, Sr) if Sr else Fraction(1)
    elif mode == "offset":
        a = Fraction(1)
    a = min(max(a, Fraction(100, 100 + max_gain)), Fraction(100 + max_gain, 100))
    b = Fraction(0) if mode == "gain" else (Sv - a * Sr) / n
    return a, min(max(b, Fraction(-max_offset)), Fraction(max_offset))


def rnd(x):
    """A Fraction rounded to the nearest integer, halves up, as rule 2 rounds."""
    return (2 * x.numerator + x.denominator) // (2 * x.denominator)


def tables(a, b):
    """-> (G, B) [256] u8."""
    g = [min(max(rnd((v - b) / a), 0), 255) for v in range(256)]
    bk = [min(max(rnd(a * u + b), 0), 255) for u in range(256)]
    return np.array(g, np.uint8), np.array(bk, np.uint8)


def fit_tables(n, sums, mode="affine", min_pixels=1024, max_gain=25, max_offset=32, **_):
    """-> (G [T,3,256] u8, B [T,3,256] u8, identity [T] bool, fits [T][3] of (a, b), fit: False = unfit)."""
    T = len(sums)
    Gt, Bt = np.broadcast_to(IDENT, (T, 3, 256)).copy(), np.broadcast_to(IDENT, (T, 3, 256)).copy()
    ident, fits = np.ones(T, bool), [[(Fraction(1), Fraction(0))] * 3 for _ in range(T)]
    if n < min_pixels:
        return Gt, Bt, ident, fits, False
    for t, row in enumerate(sums):
        for c in range(3):
            fits[t][c] = fit(n, row[c], row[3 + c], sums[0][6 + c], sums[0][9 + c], mode, max_gain, max_offset)
            Gt[t, c], Bt[t, c] = tables(*fits[t][c])
        ident[t] = bool((Gt[t] == IDENT).all())
        if ident[t]:
            Bt[t] = IDENT
    return Gt, Bt, ident, fits, True


def lut(frames, tabs):
    """frames [T,h,w,3] through tabs [T,3,256]."""
    out = np.empty_like(frames)
    for t in range(len(frames)):
        for c in range(3):
            out[t, ..., c] = tabs[t, c][frames[t, ..., c]]
    return out


# ---- rule 6 -----------------------------------------------------------------------------------------------------------------------------------
def _fill(frames, dil, grain, pcfg):
    if grain is None:
        return R.fill_segment(frames, dil, **pcfg)
    return G.fill_segment(frames, dil, grain[0], grain[1], **pcfg)[:3]


def segment(frames, dil, tone=None, grain=None, **pcfg):
    """One segment ALREADY cropped as rule 1 says: frames [T,h,w,3] u8, dil [T,h,w] u8; tone = the settings (DEFAULTS' keys, any subset), grain =
    (depth, reach) or None, pcfg = plate_fill's settings -> (out u8, d2 u8, counts [T,2], info): info = dict(path, n, G, B, identity, fits, R,
    U, sums, normalised).  On the paths "identity" and "unfit" out, d2 and the counts are the plain fill's."""
    tone = dict(DEFAULTS, **(tone or {}))
    pc = dict(R.DEFAULTS, **pcfg)
    ns = R.not_sample(dil, pc["guard"])
    Rm, U, n = mean_plane(frames, ns, tone["floor"])
    sums = moments(frames, Rm, U) if n >= tone["min_pixels"] else [[0] * 12 for _ in frames]
    Gt, Bt, ident, fits, ok = fit_tables(n, sums, **tone)
    info = dict(n=n, G=Gt, B=Bt, identity=ident, fits=fits, R=Rm, U=U, sums=sums, normalised=None)
    if not ok or ident.all():
        info["path"] = "identity" if ok else "unfit"
        return _fill(frames, dil, grain, pc) + (info,)
    f1 = lut(frames, Gt)
    f2, d2, counts = _fill(f1, dil, grain, pc)
    went = (dil != 0) & (d2 == 0)
    out = frames.copy()
    out[went] = lut(f2, Bt)[went]
    info.update(path="matched", normalised=f1)
    return out, d2, counts, info


def plate_fill(frames, dil, cuts=None, tone=None, grain=None, **pcfg):
    """The whole clip: every segment of `cuts` on its own, each on its crop of rule 1 (a segment on the path "identity" or "unfit": the plain
    fill, whose result does not depend on the crop) -> (frames', dil', counts [T,2], infos: one per segment, None for a segment without a mask
    pixel)."""
    frames, dil = np.asarray(frames), np.asarray(dil)
    ring = dict(DEFAULTS, **(tone or {}))["ring"]
    out, dout, counts, infos = frames.copy(), np.zeros_like(dil), np.zeros((len(frames), 2), np.int64), []
    for s, e in R.segments(len(frames), cuts):
        box = crop(dil[s:e], ring)
        infos.append(None)
        if box is None:
            continue
        y0, x0, y1, x1 = box
        out[s:e, y0:y1, x0:x1], dout[s:e, y0:y1, x0:x1], counts[s:e], infos[-1] = segment(frames[s:e, y0:y1, x0:x1], dil[s:e, y0:y1, x0:x1], tone, grain, **pcfg)
        infos[-1]["box"] = box
    return out, dout, counts, infos


# ---- clips ------------------------------------------------------------------------------------------------------------------------------------
def flicker_gains(T, pct):
    """Per-frame gains (100 + p_t) / 100 as the integers p_t: +pct on even frames, -pct on odd ones (mains flicker beating with the frame rate),
    the case that leaves the plain fill the least."""
    return np.array([pct if t % 2 == 0 else -pct for t in range(T)], np.int64)


NOISE = 7


def exposure_clip(seed=0, drift_q4=0, flicker_pct=0, a=NOISE, **kw):
    """platefill_ref.locked_off_clip with additive drift (its drift_q4: drift_q4 / 4 levels per frame) and / or a per-frame gain flicker of
    +-flicker_pct percent on top: every byte v of frame t becomes (v (100 + p_t) + 50) // 100 -> (frames u8, masks u8, clean [T,H,W,3]
    float64 = the noise-free background of each frame at its own exposure, boxm, logom).
    The noise is +-7, not locked_off_clip's +-6: the tests first assert that the plain fill fills NOTHING on these clips, and at 1 level per
    frame that is a narrow thing at +-6.  The columns the box leaves first have 18 consecutive samples; their variance is (18^2 - 1) / 12 =
    26.9 from the drift plus a (a + 1) / 3 from the noise: 40.9 at a = 6, 14 % over tol^2 = 36, and the sample variance of 18 values scatters
    by more than that (at seed 3 two of 5460 pixels pass and are filled); 45.6 at a = 7.  At a = 8 the noise alone (24) comes so close to
    tol^2 that the clip without drift loses a third of its fill."""
    frames, masks, clean, boxm, logom = R.locked_off_clip(seed=seed, a=a, drift_q4=drift_q4, **kw)
    clean = clean.astype(np.float64)
    if flicker_pct:
        p = flicker_gains(len(frames), flicker_pct).reshape(-1, 1, 1, 1)
        frames = np.clip((frames.astype(np.int64) * (100 + p) + 50) // 100, 0, 255).astype(np.uint8)
        clean = clean * (100 + p) / 100.0
    return frames, masks, clean, boxm, logom
