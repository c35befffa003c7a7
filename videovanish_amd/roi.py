"""Mask-region inference: the plan of the crop window the model runs on (pure host logic; covered by CPU tests).

The masked area of a typical clip (a logo, a watermark, one person) is a few per cent of the frame.  Instead of running the prior, the VAE,
the denoise loop and the decode over the whole (downscaled) frame, the drop-in (diffuerase.run_infill_on_frames(roi=...)) crops every frame
to one window around the dilated masks, runs the unchanged pipeline on that smaller clip and pastes the result back
(hip.roi_paste_composite).  Every frame of a clip gets a window of the SAME size, so chunking, overlap blending and sharding see an ordinary
clip.  Rules and the reasons for them: DESIGN.md, "Mask-region inference".

With max_regions > 1 each separate masked region gets a window of its own (label_tiles, plan_regions): the connected parts of the clip's
mask footprint, merged until their windows are pairwise disjoint in every frame and there are at most max_regions of them.
"""
import collections
import dataclasses
import math

import numpy as np

MODES = ("static", "follow")
REGION_SPELLINGS = {"static-regions": "static", "follow-regions": "follow"}      # RoiConfig(mode, max_regions=8)
SPELLINGS = MODES + tuple(REGION_SPELLINGS)


@dataclasses.dataclass(frozen=True)
class RoiConfig:
    """mode: "static" = one window for the whole clip; "follow" = a fixed-size window per frame that follows the mask.
    context: padding as a fraction of the mask box's longer side; pad_min: least padding (px); min_side: least window side (px, capped at the
    frame side) -- SD-1.5 needs surrounding context; smooth: radius (frames) of the moving average of the "follow" centres.
    max_regions: 1 = one window around all masks; > 1 = one window per separate masked region, at most this many (plan_regions)."""
    mode: str
    context: float = 0.5
    pad_min: int = 32
    min_side: int = 512
    smooth: int = 8
    max_regions: int = 1

    def __post_init__(self):
        if self.mode not in MODES:
            raise ValueError(f"RoiConfig.mode must be one of {MODES}, not {self.mode!r}")
        if self.context < 0 or self.pad_min < 0 or self.min_side < 1 or self.smooth < 0 or self.max_regions < 1:
            raise ValueError(f"RoiConfig: bad parameters {self}")


@dataclasses.dataclass(frozen=True)
class RoiPlan:
    """size = (h, w) of every frame's window; offsets [T,2] int32 = (oy, ox) of frame t's window; centers [T,2] float64 = the (smoothed)
    window centres the offsets were derived from (before the shift into the frame)."""
    mode: str
    size: tuple
    offsets: np.ndarray
    centers: np.ndarray

    def crop(self, frames):
        """One contiguous copy of each frame's window (frames: a list of [H0,W0(,C)] arrays; None entries stay None)."""
        h, w = self.size
        return [None if f is None else np.ascontiguousarray(f[oy:oy + h, ox:ox + w]) for f, (oy, ox) in zip(frames, self.offsets.tolist())]


def as_config(roi):
    """None / False / "off" / "none" / "" -> None (full frame); "static" / "follow" -> RoiConfig(mode); "static-regions" / "follow-regions" ->
    RoiConfig(mode, max_regions=8); a RoiConfig as it is."""
    if roi is None or roi is False:
        return None
    if isinstance(roi, RoiConfig):
        return roi
    if isinstance(roi, str):
        r = roi.strip().lower()
        if r in ("", "off", "none"):
            return None
        if r in MODES:
            return RoiConfig(r)
        if r in REGION_SPELLINGS:
            return RoiConfig(REGION_SPELLINGS[r], max_regions=8)
    raise ValueError(f"roi must be None, 'static', 'follow', 'static-regions', 'follow-regions' or a RoiConfig, not {roi!r}")


def _empty(b):
    return (b[:, 2] <= b[:, 0]) | (b[:, 3] <= b[:, 1])


def _side(extent, frame, pad, min_side):
    s = max(extent + 2 * pad, min(min_side, frame))
    s = -(-s // 8) * 8
    return min(s, frame)


def _smooth(c, r):
    """Centred moving average of radius r, ends held (edge-replicated): a step of the result is never larger than the largest step of c."""
    if r <= 0 or len(c) <= 1:
        return c.astype(np.float64)
    p = np.concatenate([np.full(r, c[0]), c, np.full(r, c[-1])]).astype(np.float64)
    k = np.ones(2 * r + 1) / (2 * r + 1)
    return np.convolve(p, k, mode="valid")


def plan_roi(bboxes, H0, W0, feather_px, cfg):
    """bboxes [T,4] int: half-open (y0, x0, y1, x1) of each frame's DILATED mask, a frame without mask pixels has y1 <= y0 or x1 <= x0
    (hip.mask_bbox gives (0, 0, 0, 0)).  Returns a RoiPlan, or None when the full-frame path is to run: no mask pixel at all, or every
    window is the whole frame.  Guarantee: every mask pixel and its ceil(feather_px) neighbourhood lie inside the frame's window."""
    b = np.asarray(bboxes, dtype=np.int64).reshape(-1, 4)
    T = b.shape[0]
    has = ~_empty(b)
    if T == 0 or not has.any():
        return None
    R = max(0, math.ceil(feather_px))
    bh_t, bw_t = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    if cfg.mode == "static":
        u = np.array([b[has, 0].min(), b[has, 1].min(), b[has, 2].max(), b[has, 3].max()])
        bh, bw = int(u[2] - u[0]), int(u[3] - u[1])
    else:
        bh, bw = int(bh_t[has].max()), int(bw_t[has].max())
    pad = max(cfg.pad_min, R + 2, math.ceil(cfg.context * max(bh, bw)))
    h, w = _side(bh, H0, pad, cfg.min_side), _side(bw, W0, pad, cfg.min_side)
    if (h, w) == (H0, W0):
        return None
    if cfg.mode == "static":
        oy = min(max(int(u[0]) - (h - bh) // 2, 0), H0 - h)
        ox = min(max(int(u[1]) - (w - bw) // 2, 0), W0 - w)
        offsets = np.tile(np.array([[oy, ox]], np.int32), (T, 1))
        centers = np.tile(np.array([[(u[0] + u[2]) / 2.0, (u[1] + u[3]) / 2.0]]), (T, 1))
        return RoiPlan("static", (h, w), offsets, centers)
    # follow: per-frame box centres, gaps interpolated (ends held), smoothed, then each window shifted as little as possible into the frame
    # and around its own box grown by R + 1
    idx = np.nonzero(has)[0]
    t = np.arange(T)
    cy = np.interp(t, idx, (b[idx, 0] + b[idx, 2]) / 2.0)
    cx = np.interp(t, idx, (b[idx, 1] + b[idx, 3]) / 2.0)
    cy, cx = _smooth(cy, cfg.smooth), _smooth(cx, cfg.smooth)
    g = R + 1
    offsets = np.zeros((T, 2), np.int32)
    for k in range(T):
        for a, (c, s, F, lo, hi) in enumerate(((cy[k], h, H0, b[k, 0], b[k, 2]), (cx[k], w, W0, b[k, 1], b[k, 3]))):
            lo_o, hi_o = 0, F - s
            if has[k]:
                lo_o = max(lo_o, min(F, int(hi) + g) - s)
                hi_o = min(hi_o, max(0, int(lo) - g))
            o = int(math.floor(c - s / 2.0 + 0.5))
            offsets[k, a] = min(max(o, lo_o), hi_o)
    return RoiPlan("follow", (h, w), offsets, np.stack([cy, cx], axis=1))


# ---- several regions ------------------------------------------------------------------------------------------------------------------
def _label8(occ):
    """8-connected components of a boolean grid: labels (-1 = empty) numbered in raster order of their first cell, and their count."""
    Hc, Wc = occ.shape
    lab = np.full((Hc, Wc), -1, np.int32)
    K = 0
    for y0, x0 in zip(*np.nonzero(occ)):
        if lab[y0, x0] >= 0:
            continue
        lab[y0, x0] = K
        q = collections.deque([(y0, x0)])
        while q:
            y, x = q.popleft()
            for yy in range(max(0, y - 1), min(Hc, y + 2)):
                for xx in range(max(0, x - 1), min(Wc, x + 2)):
                    if occ[yy, xx] and lab[yy, xx] < 0:
                        lab[yy, xx] = K
                        q.append((yy, xx))
        K += 1
    return lab, K


def label_tiles(occ, max_components=64, tile=16):
    """occ [Hc,Wc] (hip.mask_tile_union on tile x tile cells) -> (labels [Hc',Wc'] int32 with -1 = empty, K, tile'): the 8-connected components
    of the occupied cells.  While there are more than max_components, the grid is OR-pooled 2 x 2 (the tile doubles) and labelled again, so
    nearby components merge first and K stays bounded for salt-like masks."""
    g = np.asarray(occ).astype(bool)
    while True:
        lab, K = _label8(g)
        if K <= max_components or g.size <= 1:
            return lab, K, tile
        Hc, Wc = g.shape
        g = np.pad(g, ((0, Hc % 2), (0, Wc % 2)))
        g = g[0::2, 0::2] | g[0::2, 1::2] | g[1::2, 0::2] | g[1::2, 1::2]
        tile *= 2


def _union(a, b):
    """Per-frame union of two [T,4] box tracks (an empty box is the identity; both empty -> (0, 0, 0, 0))."""
    ea, eb = _empty(a), _empty(b)
    u = np.stack([np.minimum(a[:, 0], b[:, 0]), np.minimum(a[:, 1], b[:, 1]), np.maximum(a[:, 2], b[:, 2]), np.maximum(a[:, 3], b[:, 3])], 1)
    u[ea] = b[ea]
    u[eb & ~ea] = a[eb & ~ea]
    return u


class _Region:
    """One region: its box track, its plan (None = the whole frame), its windows [T,4] = (y0, x0, y1, x1) and its clip box (the union of its
    boxes over the clip)."""

    def __init__(self, boxes, H0, W0, feather_px, cfg):
        self.boxes = boxes
        self.plan = plan_roi(boxes, H0, W0, feather_px, cfg)
        if self.plan is None:
            self.win = np.tile(np.array([[0, 0, H0, W0]], np.int64), (len(boxes), 1))
        else:
            o = self.plan.offsets.astype(np.int64)
            self.win = np.concatenate([o, o + np.array(self.plan.size, np.int64)], 1)
        has = ~_empty(boxes)
        self.clip = (int(boxes[has, 0].min()), int(boxes[has, 1].min()), int(boxes[has, 2].max()), int(boxes[has, 3].max()))
        self.key = self.clip + tuple(boxes.ravel().tolist())     # geometry only: orders regions whatever their numbering


def _overlap(a, b):
    wa, wb = a.win, b.win
    return bool(((np.maximum(wa[:, 0], wb[:, 0]) < np.minimum(wa[:, 2], wb[:, 2])) & (np.maximum(wa[:, 1], wb[:, 1]) < np.minimum(wa[:, 3], wb[:, 3]))).any())


def _pair_key(a, b):
    """Merge order: overlapping pairs first, then the smaller merged clip box, then coordinates."""
    y0, x0, y1, x1 = min(a.clip[0], b.clip[0]), min(a.clip[1], b.clip[1]), max(a.clip[2], b.clip[2]), max(a.clip[3], b.clip[3])
    lo, hi = sorted((a.key, b.key))
    return (not _overlap(a, b), (y1 - y0) * (x1 - x0), (y0, x0, y1, x1), lo, hi)


def plan_regions(bboxes, H0, W0, feather_px, cfg):
    """bboxes [T,K,4] int: half-open (y0, x0, y1, x1) of region k's DILATED mask in frame t (hip.mask_bbox_tiles).  Returns RoiPlans sorted by
    the regions' (y0, x0), or None when the full-frame path is to run.  Each region is planned by plan_roi on its own track; while two windows
    overlap in some frame, or there are more than cfg.max_regions regions, one pair is merged (its box in frame t: the union of the two boxes)
    and planned again.  Guarantees: the windows are pairwise disjoint in every frame; every mask pixel of a region and its ceil(feather_px)
    neighbourhood lie inside that region's window; at most cfg.max_regions plans; with max_regions = 1 or one region the result is
    [plan_roi(per-frame bbox of the whole mask)], or None when that is None."""
    b = np.asarray(bboxes, dtype=np.int64)
    if b.size == 0:
        return None
    T = b.shape[0]
    b = b.reshape(T, -1, 4)
    tracks = [np.ascontiguousarray(b[:, k]) for k in range(b.shape[1]) if not _empty(b[:, k]).all()]
    if not tracks:
        return None
    if cfg.max_regions == 1 or len(tracks) == 1:
        u = tracks[0]
        for tr in tracks[1:]:
            u = _union(u, tr)
        p = plan_roi(u, H0, W0, feather_px, cfg)
        return None if p is None else [p]
    regs = {i: _Region(tr, H0, W0, feather_px, cfg) for i, tr in enumerate(tracks)}
    pairs = {(i, j): _pair_key(regs[i], regs[j]) for i in regs for j in regs if i < j}
    nxt = len(tracks)
    while len(regs) > 1:
        (i, j), key = min(pairs.items(), key=lambda kv: kv[1])
        if key[0] and len(regs) <= cfg.max_regions:              # no two windows overlap and few enough regions: done
            break
        new = _Region(_union(regs[i].boxes, regs[j].boxes), H0, W0, feather_px, cfg)
        del regs[i], regs[j]
        pairs = {p: k for p, k in pairs.items() if i not in p and j not in p}
        for r in regs:                                           # only the pairs that involve the new region are tested
            pairs[(r, nxt)] = _pair_key(regs[r], new)
        regs[nxt] = new
        nxt += 1
    out = sorted(regs.values(), key=lambda r: r.key)
    if len(out) == 1:
        return None if out[0].plan is None else [out[0].plan]
    return [r.plan for r in out]
