"""Helpers of the clean-plate grain tests: the numpy restatement of the rule of include/vvplategrain.h, written from the
header in another form than the kernel's two walks -- every pixel's usable frames as one sorted list, a candidate being a position in it --
and built on platefill_ref for rules 1 - 7; the statistic of the issue and the hand-made pixel table the tests share.  No test in here."""
import numpy as np

import platefill_ref as R

NONE = R.NONE
DEFAULTS = dict(depth=4, reach=8)


def usable_lists(us):
    """us [T,H,W] bool -> (U [T,H,W]: per pixel its usable frames ascending, then T; cnt [H,W]: how many; rank [T,H,W]: where frame s stands in
    its pixel's list, for a usable s)."""
    T = len(us)
    t = np.arange(T).reshape(T, 1, 1)
    return np.sort(np.where(us, t, T), axis=0), us.sum(0), np.cumsum(us, axis=0) - 1


def live_sources(src, us, depth, reach, max_gap):
    """The rule: src [T,H,W] uint16 (rule 5, after max_gap), us [T,H,W] bool (rule 4) -> (live [T,H,W] uint16, m [T,H,W]: the candidates kept,
    0 where there is no source, side [T,H,W]: -1 before, +1 after, 0 none)."""
    T = len(src)
    t = np.arange(T).reshape(T, 1, 1)
    U, cnt, rank = usable_lists(us)
    has = src != NONE
    s = np.where(has, src, 0).astype(np.int64)
    j = np.take_along_axis(rank, s, axis=0)                  # c_0 = U[j]
    side = np.where(has, np.where(s < t, -1, 1), 0)
    m, alive = np.zeros(src.shape, np.int64), has.copy()
    for i in range(depth):
        pos = j + side * i                                    # going away from t
        inside = (pos >= 0) & (pos < cnt[None])
        c = np.take_along_axis(U, np.clip(pos, 0, T - 1), axis=0)
        alive = alive & inside & (np.abs(c - s) <= reach)
        if max_gap > 0:
            alive &= np.abs(c - t) <= max_gap
        m += alive
    k = t % np.maximum(m, 1)
    live = np.take_along_axis(U, np.clip(j + side * k, 0, T - 1), axis=0)
    return np.where(has, live, NONE).astype(np.uint16), m, side


def fill_segment(frames, dil, depth=4, reach=8, invalid=None, **cfg):
    """One segment under plate_fill's settings cfg and the rule -> (frames' u8, dil' u8, counts [T,2] int64, detail); invalid [T,H,W] bool =
    places that give no sample besides rule 1's (the canvas places no frame covers).  dil', the counts and detail's src / r0 are those of
    rules 1 - 6 alone; detail adds live, m, side, go (the filled pixels) and nearest (the frames rule 7 gives with src)."""
    frames, dil = np.asarray(frames), np.asarray(dil)
    cfg = dict(R.DEFAULTS, **cfg)
    T = len(frames)
    ns = R.not_sample(dil, cfg["guard"])
    if invalid is not None:
        ns = ns | invalid
    n, S1, S2 = R.stats(frames, ns)
    st = R.steady(n, S1, S2, cfg["min_samples"], cfg["tol"])
    us = R.usable(frames, ns, st, n, S1, cfg["tol"], cfg["outlier"])
    src = R.sources(dil, us, cfg["max_gap"])
    live, m, side = live_sources(src, us, depth, reach, cfg["max_gap"])
    masked = dil != 0
    r0 = masked & (src == NONE)
    keep = R.dilate(r0, cfg["margin"]) & masked
    go = masked & ~keep
    tt, yy, xx = np.nonzero(go)
    out, near = frames.copy(), frames.copy()
    out[tt, yy, xx] = frames[live[tt, yy, xx].astype(np.int64), yy, xx]
    near[tt, yy, xx] = frames[src[tt, yy, xx].astype(np.int64), yy, xx]
    counts = np.stack([go.reshape(T, -1).sum(1), keep.reshape(T, -1).sum(1)], axis=1).astype(np.int64)
    det = dict(ns=ns, n=n, S1=S1, steady=st, usable=us, src=src, r0=r0.astype(np.uint8) * 255, live=live, m=m, side=side, go=go, nearest=near)
    return out, keep.astype(np.uint8) * 255, counts, det


def fill_on_canvas(frames, dil, depth=4, reach=8, **cfg):
    """One tracked segment filled on its canvas (platealign_ref's steps, the rule in place of rule 7's source) -> (frames', dil', counts [T,2],
    rotated [T]).  Every frame must be tracked and the canvas must exist."""
    import platealign_ref as A
    frames, dil = np.asarray(frames), np.asarray(dil)
    track = A.track_segment(frames, dil, **A.DEFAULTS)
    assert (track[:, 3] == 1).all() and track[:, :2].any()
    box = A.canvas_box(dil, track)
    canvas, _ = A.place(frames, track, box, tracked_only=False)
    dil_c, inv_c = A.place_masks(dil, track, box)
    out_c, d2_c, counts, det = fill_segment(canvas, dil_c, depth, reach, invalid=inv_c != 0, **cfg)
    out = frames.copy()
    for t, yy, xx in zip(*np.nonzero(det["go"])):
        out[t, yy + box[0] - track[t, 1], xx + box[1] - track[t, 0]] = out_c[t, yy, xx]
    rotated = (det["go"] & (det["live"] != det["src"])).reshape(len(frames), -1).sum(1)
    return out, A.unplace_mask(d2_c, dil, track, box), counts, rotated


def plate_fill(frames, dil, cuts=None, depth=4, reach=8, **cfg):
    """The whole clip, every segment of `cuts` on its own (t of `t mod m` counts from the segment's start) -> (frames', dil', counts [T,2],
    rotated [T] = the filled pixels whose live source is not the nearest one)."""
    frames, dil = np.asarray(frames), np.asarray(dil)
    T = len(frames)
    out, dout, counts, rotated = frames.copy(), np.zeros_like(dil), np.zeros((T, 2), np.int64), np.zeros(T, np.int64)
    for s, e in R.segments(T, cuts):
        out[s:e], dout[s:e], counts[s:e], det = fill_segment(frames[s:e], dil[s:e], depth, reach, **cfg)
        rotated[s:e] = (det["go"] & (det["live"] != det["src"])).reshape(e - s, -1).sum(1)
    return out, dout, counts, rotated


# ---- the statistic --------------------------------------------------------------------------------------------------------------------------
def motion(frames, pairs):
    """Mean absolute difference frames[t + 1] - frames[t] over the pixels of pairs [T-1,H,W] bool (all channels)."""
    d = np.abs(np.asarray(frames)[1:].astype(np.int64) - np.asarray(frames)[:-1])
    return float(d[pairs].mean())


def grain_ratio(out, frames, masks, go, pairs=None):
    """The frame-to-frame motion of the filled pixels of `out` (those of go [T,H,W] filled in both frames of a pair; `pairs` narrows them) over
    that of the pixels no frame masks -> (ratio, the number of pairs counted)."""
    both = go[1:] & go[:-1]
    if pairs is not None:
        both = both & pairs
    free = np.broadcast_to(~(np.asarray(masks) != 0).any(0), both.shape)
    return motion(out, both) / motion(frames, free), int(both.sum())


def same_side_pairs(det):
    """Pairs of consecutive frames on one side with at least two candidates in both."""
    return (det["side"][1:] == det["side"][:-1]) & (det["side"][1:] != 0) & (det["m"][1:] >= 2) & (det["m"][:-1] >= 2)


# ---- the hand-made pixel table ----------------------------------------------------------------------------------------------------------------
# One row per pixel, one character per frame: u = unmasked at the pixel's steady value (a usable sample), o = unmasked but 10 levels off (a
# sample that is no usable one while fewer than 4 in 10 samples are such), M = masked.  With TABLE_CFG (guard 0, one sample is enough, a
# usable sample lies within tol of the mean, no margin) the usable frames are exactly the u's.
TABLE = {
    "one candidate before":      "uMMMMMMMMMMMMMMMMMMM",      # the only usable frame is frame 0
    "cut by reach":              "uuMMuuMMMMMMMMMMMMMM",      # frame 6 on: candidates 5, 4, 1, 0; reach 3 keeps 5, 4
    "cut by max_gap":            "uuuuuuMMMMMMMMMMMMMM",      # max_gap 4: frame 6 keeps 5, 4, 3, 2; frame 9 keeps 5; frame 10 has no source
    "outlier between":           "uuouuoMMMMoouuouuuuu",      # before 4, 3, 1, 0 and after 12, 13, 15, 16: the o's are stepped over
    "run at the start":          "MMMMMuuuuuuuuuuuuuuu",      # the after side only
    "run at the end":            "uuuuuuuuuuuuuuuMMMMM",      # the before side only
    "tie between the sides":     "uuuuuuuMMMMMuuuuuuuu",      # frame 9: 6 and 12 are both 3 away, the earlier wins
    "never masked":              "uuuuuuuuuuuuuuuuuuuu",
    "more than eight a side":    "uuuuuuuuuMMuuuuuuuuu",
    "no usable frame":           "MMMMMMMMMMMMMMMMMMMM",
}
TABLE_CFG = dict(guard=0, min_samples=1, tol=6, outlier=1, max_gap=0, margin=0)


def table_clip(rows=None):
    """The table as a clip of H = 1: frames [T,1,W,3] u8 (a u is 100 + the pixel's number, an o 10 more, an M 250), masks [T,1,W] u8, and the
    wanted usable frames [T,1,W] bool."""
    rows = list((rows or TABLE).values())
    T, W = len(rows[0]), len(rows)
    frames, masks, us = np.zeros((T, 1, W, 3), np.uint8), np.zeros((T, 1, W), np.uint8), np.zeros((T, 1, W), bool)
    for x, row in enumerate(rows):
        assert len(row) == T
        for t, ch in enumerate(row):
            frames[t, 0, x] = {"u": 100 + x, "o": 110 + x, "M": 250}[ch]
            masks[t, 0, x] = 255 * (ch == "M")
            us[t, 0, x] = ch == "u"
    return frames, masks, us
