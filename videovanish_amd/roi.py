"""Mask-region inference: the plan of the crop window the model runs on (pure host logic; covered by CPU tests).

The masked area of a typical clip (a logo, a watermark, one person) is a few per cent of the frame.  Instead of running the prior, the VAE,
the denoise loop and the decode over the whole (downscaled) frame, the drop-in (diffuerase.run_infill_on_frames(roi=...)) crops every frame
to one window around the dilated masks, runs the unchanged pipeline on that smaller clip and pastes the result back
(hip.roi_paste_composite).  Every frame of a clip gets a window of the SAME size, so chunking, overlap blending and sharding see an ordinary
clip.  Rules and the reasons for them: DESIGN.md, "Mask-region inference".
"""
import dataclasses
import math

import numpy as np

MODES = ("static", "follow")


@dataclasses.dataclass(frozen=True)
class RoiConfig:
    """mode: "static" = one window for the whole clip; "follow" = a fixed-size window per frame that follows the mask.
    context: padding as a fraction of the mask box's longer side; pad_min: least padding (px); min_side: least window side (px, capped at the
    frame side) -- SD-1.5 needs surrounding context; smooth: radius (frames) of the moving average of the "follow" centres."""
    mode: str
    context: float = 0.5
    pad_min: int = 32
    min_side: int = 512
    smooth: int = 8

    def __post_init__(self):
        if self.mode not in MODES:
            raise ValueError(f"RoiConfig.mode must be one of {MODES}, not {self.mode!r}")
        if self.context < 0 or self.pad_min < 0 or self.min_side < 1 or self.smooth < 0:
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
    """None / False / "off" / "none" / "" -> None (full frame); "static" / "follow" -> RoiConfig(mode); a RoiConfig as it is."""
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
    raise ValueError(f"roi must be None, 'static', 'follow' or a RoiConfig, not {roi!r}")


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
