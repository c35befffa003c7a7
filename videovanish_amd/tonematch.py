"""Seam tone matching: the settings, the per-frame fit and the tables of the stage in front of the composite (pure host logic, numpy only, no
torch; covered by CPU tests).

The feathered composite assumes that the model's frame and the original agree in tone.  In the ring -- the unmasked pixels of the window within
`ring` pixels of the mask -- both the original pixel y and the model's rendering x of the same pixel exist; a per-frame, per-channel fit of
y as a function of x over the ring says how to move the model's pixels before they are blended.  The device sums the ring (csrc/vv_tone.hip:
16 integers per frame), this module turns the sums into a gain and an offset (fit) and those into a 256-entry table per frame and channel
(tables), and the fused paste looks every pasted byte up (infill.finish).  Rules, guarantees and limits: DESIGN.md, "Seam tone matching".
"""
import dataclasses
from typing import NamedTuple

import numpy as np

MAX_RING = 32           # the limit of vvt_ring_stats (include/vvtone.h)
NSUM = 16               # per frame: n, sum x_c, sum y_c, sum x_c^2, sum x_c y_c, sum y_c^2 (c = 0, 1, 2)
SPELLINGS = ("on", "affine", "offset")      # what --tone-match / $VV_TONE_MATCH / tone_match= accept as a word (besides "off"); also "mode=offset,ring=8,smooth=0", any subset
_KEYS = {"mode": str, "ring": int, "smooth": int, "max_gain": float, "max_offset": float, "min_count": int, "min_var": float}


@dataclasses.dataclass(frozen=True)
class ToneMatchConfig:
    """mode: "affine" fits a gain and an offset per channel, "offset" an offset only.  ring: width of the band round the mask, in pixels (a box).
    smooth: the sums of the frames t - smooth .. t + smooth are pooled for frame t's fit.  max_gain: the gain stays in [1 / max_gain, max_gain].
    max_offset: the offset stays in [-max_offset, max_offset] (8-bit levels).  min_count: a frame whose pooled ring has fewer pixels is left
    as it is.  min_var: a channel whose ring has less variance in x gets the gain 1 (a flat ring says nothing about a slope).  The defaults are
    build-defined: nobody has measured the tone shift of the real checkpoints, or run real footage through this stage."""
    mode: str = "affine"
    ring: int = 12
    smooth: int = 2
    max_gain: float = 1.25
    max_offset: float = 32.0
    min_count: int = 64
    min_var: float = 4.0

    def __post_init__(self):
        if self.mode not in ("affine", "offset"):
            raise ValueError(f"ToneMatchConfig.mode must be 'affine' or 'offset', not {self.mode!r}")
        for name in ("ring", "smooth", "min_count"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"ToneMatchConfig.{name} must be an integer, not {v!r}")
        for name in ("max_gain", "max_offset", "min_var"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
                raise ValueError(f"ToneMatchConfig.{name} must be a number, not {v!r}")
        if not (1 <= self.ring <= MAX_RING and 0 <= self.smooth <= 16 and 1.0 <= self.max_gain <= 2.0 and 0 <= self.max_offset <= 128
                and self.min_count >= 1 and self.min_var >= 0):
            raise ValueError(f"ToneMatchConfig: 1 <= ring <= {MAX_RING}, 0 <= smooth <= 16, 1 <= max_gain <= 2, 0 <= max_offset <= 128, min_count >= 1 "
                             f"and min_var >= 0 are supported, not {self}")


def _number(kind, val):
    """val as an int ("12") or a float ("1.25", "4"); None where it is neither."""
    if kind is int:
        return int(val) if val.isascii() and val.isdigit() else None
    try:
        v = float(val)
    except ValueError:
        return None
    return v if val.isascii() and v == v and abs(v) != float("inf") else None


def as_config(tone_match):
    """None / False / "off" / "none" / "" -> None (no tone matching); "on" (or True) -> ToneMatchConfig(); "affine" / "offset" -> the defaults with
    that mode; "mode=offset,ring=8,smooth=0" (any subset, each key once) -> the defaults with those fields; a ToneMatchConfig as it is."""
    if tone_match is None or tone_match is False:
        return None
    if tone_match is True:
        return ToneMatchConfig()
    if isinstance(tone_match, ToneMatchConfig):
        return tone_match
    if isinstance(tone_match, str):
        s = tone_match.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return ToneMatchConfig()
        if s in ("affine", "offset"):
            return ToneMatchConfig(mode=s)
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or key in kw:
                break
            kw[key] = val if _KEYS[key] is str else _number(_KEYS[key], val)
            if kw[key] is None:
                break
        else:
            return ToneMatchConfig(**kw)
    raise ValueError("tone_match must be None, 'on', 'off', 'affine', 'offset', 'mode=..,ring=N,smooth=N,max_gain=X,max_offset=X,min_count=N,min_var=X' "
                     f"(any subset) or a ToneMatchConfig, not {tone_match!r}")


class ToneFit(NamedTuple):
    """The fit of one window: per frame the pixels of its own ring, per frame and channel the gain and offset applied (1 and 0: the frame is left
    as it is) and the RMS of y - x and of y - (gain x + offset) over the frame's own ring (0 where it is empty)."""
    n: np.ndarray               # [T] int64
    gain: np.ndarray            # [T,3] float64
    offset: np.ndarray          # [T,3] float64
    rms_before: np.ndarray      # [T,3] float64
    rms_after: np.ndarray       # [T,3] float64


def pool(sums, smooth):
    """pooled[t] = the integer sum of sums[max(0, t - smooth) .. t + smooth] ([T,16] int64 both)."""
    sums = np.asarray(sums, np.int64)
    c = np.concatenate([np.zeros((1, sums.shape[1]), np.int64), np.cumsum(sums, axis=0)])
    t = np.arange(len(sums))
    return c[np.minimum(t + smooth + 1, len(sums))] - c[np.maximum(t - smooth, 0)]


def fit(sums, cfg):
    """sums [T,16] int64 (a frame this rank does not hold, or without a ring: zeros) -> ToneFit.  Frame t is fitted to the pooled sums of frames
    t - smooth .. t + smooth; it keeps gain 1 and offset 0 when its own ring is empty or the pooled one has fewer than min_count pixels.  Per
    channel in fp64: gain = cov(x, y) / var(x) inside [1 / max_gain, max_gain] (1 in "offset" mode, or where var(x) < min_var or is not
    positive), offset = mean(y) - gain mean(x) inside +-max_offset.  Where x == y on the ring, cov and var are the same number computed the
    same way, so the gain is exactly 1.0 and the offset exactly 0.0."""
    sums = np.asarray(sums, np.int64).reshape(-1, NSUM)
    T = len(sums)
    gain, offset = np.ones((T, 3)), np.zeros((T, 3))
    p = pool(sums, cfg.smooth)
    for t in np.nonzero((sums[:, 0] > 0) & (p[:, 0] >= cfg.min_count))[0]:
        n = float(p[t, 0])
        for c in range(3):
            xm, ym = p[t, 1 + c] / n, p[t, 4 + c] / n
            vx = p[t, 7 + c] / n - xm * xm
            cxy = p[t, 10 + c] / n - xm * ym
            g = 1.0 if (cfg.mode == "offset" or vx < cfg.min_var or vx <= 0.0) else min(max(cxy / vx, 1.0 / cfg.max_gain), float(cfg.max_gain))
            gain[t, c] = g
            offset[t, c] = min(max(ym - g * xm, -float(cfg.max_offset)), float(cfg.max_offset))
    # the residuals over each frame's own ring, in closed form from its own sums: sum (y - g x - o)^2 expanded
    n = sums[:, :1].astype(np.float64)
    sx, sy, sxx, sxy, syy = (sums[:, k:k + 3].astype(np.float64) for k in (1, 4, 7, 10, 13))
    with np.errstate(divide="ignore", invalid="ignore"):
        before = (sums[:, 13:16] - 2 * sums[:, 10:13] + sums[:, 7:10]) / n
        after = (syy - 2 * gain * sxy - 2 * offset * sy + gain * gain * sxx + 2 * gain * offset * sx + n * offset * offset) / n
    has = np.broadcast_to(n > 0, before.shape)
    rms = lambda v: np.sqrt(np.where(has, np.maximum(v, 0.0), 0.0))
    return ToneFit(sums[:, 0].copy(), gain, offset, rms(before), rms(after))


def tables(gain, offset):
    """gain, offset [..., 3] -> uint8 [..., 3, 256]: table[v] = clip(rint(gain v + offset), 0, 255), halves to even.  Gain 1, offset 0: the identity."""
    v = np.arange(256, dtype=np.float64)
    return np.clip(np.rint(np.asarray(gain, np.float64)[..., None] * v + np.asarray(offset, np.float64)[..., None]), 0, 255).astype(np.uint8)
