"""Helpers of the clean-plate fill tests: the numpy / scipy restatement of rules 1 - 7 and the counts of include/vvplate.h,
written from the header and independent of the product code, and the clips the tests share.  No test in here."""
import numpy as np
from scipy import ndimage

NONE = 65535
CROSS = ndimage.generate_binary_structure(2, 1)
DEFAULTS = dict(guard=1, min_samples=4, tol=6, outlier=3, max_gap=0, margin=2)


def segments(T, cuts):
    edges = [0] + sorted({int(c) for c in (cuts or ()) if 0 < int(c) < T}) + [T]
    return [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]


def not_sample(dil, guard):
    """Rule 1, complemented: [T,H,W] bool, True where some frame within `guard` of t (inside the segment) is masked."""
    m = np.asarray(dil) != 0
    out = m.copy()
    for j in range(1, guard + 1):
        out[j:] |= m[:-j]
        out[:-j] |= m[j:]
    return out


def stats(frames, ns):
    """Rule 2 -> (n [H,W], S1 [H,W,3], S2 [H,W,3]) int64."""
    smp = ~ns
    v = np.asarray(frames).astype(np.int64) * smp[..., None]
    return smp.sum(0).astype(np.int64), v.sum(0), (v * v).sum(0)


def steady(n, S1, S2, min_samples, tol):
    """Rule 3 -> [H,W] bool."""
    nn = n[..., None]
    return (n >= min_samples) & (nn * S2 - S1 * S1 <= tol * tol * nn * nn).all(-1)


def usable(frames, ns, st, n, S1, tol, outlier):
    """Rule 4 -> [T,H,W] bool."""
    v = np.asarray(frames).astype(np.int64)
    near = (np.abs(n[None, ..., None] * v - S1[None]) <= outlier * tol * n[None, ..., None]).all(-1)
    return ~ns & st[None] & near


def sources(dil, us, max_gap):
    """Rule 5 -> src [T,H,W] uint16, NONE where the pixel is unmasked or has no source."""
    T = len(dil)
    t = np.arange(T).reshape(T, 1, 1)
    big = 4 * T + 4
    before = np.maximum.accumulate(np.where(us, t, -1), axis=0)
    after = np.minimum.accumulate(np.where(us, t, big)[::-1], axis=0)[::-1]
    has_b, has_a = before >= 0, after < big
    take_b = has_b & (~has_a | (t - before <= after - t))             # the smaller index wins a tie
    pick = np.where(take_b, before, after)
    found = (has_b | has_a) & (np.asarray(dil) != 0)
    if max_gap > 0:
        found &= np.abs(pick - t) <= max_gap
    return np.where(found, pick, NONE).astype(np.uint16)


def dilate(m, iters):
    """`iters` steps of the 3 x 3 cross on every frame of m [T,H,W] bool (0: m itself)."""
    if iters == 0:
        return m.copy()
    return np.stack([ndimage.binary_dilation(f, structure=CROSS, iterations=iters) for f in m])


def fill_segment(frames, dil, guard=1, min_samples=4, tol=6, outlier=3, max_gap=0, margin=2, detail=False):
    """One segment: frames [T,H,W,3] u8, dil [T,H,W] u8 -> (frames' u8, dil' u8 {0, 255}, counts [T,2] int64 = pixels filled, masked pixels left);
    detail=True adds a dict of the intermediate arrays."""
    frames, dil = np.asarray(frames), np.asarray(dil)
    T = len(frames)
    ns = not_sample(dil, guard)
    n, S1, S2 = stats(frames, ns)
    st = steady(n, S1, S2, min_samples, tol)
    us = usable(frames, ns, st, n, S1, tol, outlier)
    src = sources(dil, us, max_gap)
    masked = dil != 0
    r0 = masked & (src == NONE)
    keep = dilate(r0, margin) & masked                                   # rule 6: dil'
    go = masked & ~keep
    out = frames.copy()
    tt, yy, xx = np.nonzero(go)
    out[tt, yy, xx] = frames[src[tt, yy, xx].astype(np.int64), yy, xx]   # rule 7
    counts = np.stack([go.reshape(T, -1).sum(1), keep.reshape(T, -1).sum(1)], axis=1).astype(np.int64)
    res = (out, keep.astype(np.uint8) * 255, counts)
    if detail:
        res += (dict(ns=ns, n=n, S1=S1, S2=S2, steady=st, usable=us, src=src, r0=r0.astype(np.uint8) * 255),)
    return res


def plate_fill(frames, dil, cuts=None, **cfg):
    """The whole clip: every segment of `cuts` on its own -> (frames', dil', counts [T,2])."""
    frames, dil = np.asarray(frames), np.asarray(dil)
    out, dout, counts = frames.copy(), np.zeros_like(dil), np.zeros((len(frames), 2), np.int64)
    for s, e in segments(len(frames), cuts):
        out[s:e], dout[s:e], counts[s:e] = fill_segment(frames[s:e], dil[s:e], **cfg)
    return out, dout, counts


# ---- clips ----------------------------------------------------------------------------------------------------------------------------------
def background(H, W, seed):
    """A still: a gradient plus a fixed texture, in 40 .. 215 so that noise of a few levels never clips."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    base = 60 + (yy * 90) // max(H - 1, 1) + (xx * 40) // max(W - 1, 1)
    return np.clip(base[..., None] + rng.integers(-15, 16, (H, W, 3)), 40, 215).astype(np.int64)


def locked_off_clip(T=24, H=40, W=56, a=6, seed=0, speed=2, box=(15, 16), box_y=4, logo=(26, 4, 38, 8), drift_q4=0):
    """A locked-off shot: the still of background() plus iid noise in [-a, a] per frame (plus drift_q4 / 4 levels per frame), a bright box of
    box = (h, w) that enters from the left and moves `speed` px per frame, and a fixed logo (y0, x0, y1, x1; None for none).  Returns (frames
    [T,H,W,3] u8, masks [T,H,W] u8 {0, 255} = box | logo, clean [T,H,W,3] int64 = the noise-free background, box [T,H,W] bool, logo [H,W] bool)."""
    rng = np.random.default_rng(seed + 1000)
    still = background(H, W, seed)
    clean = np.stack([still + (t * drift_q4) // 4 for t in range(T)])
    frames = clean + rng.integers(-a, a + 1, (T, H, W, 3))
    boxm = np.zeros((T, H, W), bool)
    for t in range(T):
        x0 = -box[1] // 2 + speed * t
        boxm[t, box_y:box_y + box[0], max(x0, 0):max(min(x0 + box[1], W), 0)] = True
    logom = np.zeros((H, W), bool)
    if logo is not None:
        logom[logo[0]:logo[2], logo[1]:logo[3]] = True
    frames[boxm] = 250 - rng.integers(0, 30, (int(boxm.sum()), 3))
    frames[:, logom] = 20
    return np.clip(frames, 0, 255).astype(np.uint8), ((boxm | logom[None]) * 255).astype(np.uint8), clean, boxm, logom


def panning_clip(T=24, H=40, W=56, seed=0, speed=3, **kw):
    """The masks of locked_off_clip over an iid random texture that pans `speed` px per frame: no pixel sees the same thing twice."""
    rng = np.random.default_rng(seed + 2000)
    wide = rng.integers(0, 256, (H, W + speed * T, 3))
    frames, masks, _, boxm, logom = locked_off_clip(T, H, W, seed=seed, **kw)
    pan = np.stack([wide[:, speed * t: speed * t + W] for t in range(T)]).astype(np.uint8)
    hole = masks != 0
    pan[hole] = frames[hole]
    return pan, masks, boxm, logom
