"""Seam grain matching: the settings, the per-frame fit and the amplitude tables of the stage in front of the composite (pure host logic, numpy
only, no torch; covered by CPU tests).

Pixels pasted inside the mask have passed through the fp16 VAE, a 2-step schedule and often a bilinear upscale, which remove sensor noise and
film grain; the pixels outside the mask are the original bytes and still carry it.  In the ring -- the unmasked pixels of the window within
`ring` pixels of the mask -- both the original pixel y and the model's rendering x of the same pixel exist; the grain that y has and x lacks
there is the grain the pasted pixels lack.  The device takes the statistics of the flat part of the ring (csrc/vv_grain.hip: per channel and
brightness band the count and the squared responses of Immerkaer's noise operator on x and on y, 36 integers per frame), this module turns
them into a noise level per channel and band (fit) and that into a 256-entry amplitude table per frame and channel (tables), and the fused
paste adds stateless noise of that amplitude to every pasted byte (infill.finish).  Rules, guarantees and limits: DESIGN.md, "Seam grain
matching".
"""
import dataclasses
from typing import NamedTuple

import numpy as np

from .tonematch import _number, pool

MAX_RING = 32           # the limit of vvg_ring_grain_stats (include/vvgrain.h)
BANDS = 4               # brightness bands of 64 levels: band = value >> 6
NSUM = 36               # per frame [3 channels][4 bands][n, Sx = sum L(x)^2, Sy = sum L(y)^2]
OP_GAIN = 36.0          # the variance of Immerkaer's operator on white noise of variance 1: 4 * 1 + 4 * 4 + 16
CENTRES = (32.0, 96.0, 160.0, 224.0)
MODES = ("luma", "rgb")                     # the kernel's mode argument is the index
SPELLINGS = ("on", "luma", "rgb")           # what --grain-match / $VV_GRAIN_MATCH / grain_match= accept as a word (besides "off"); also "mode=rgb,ring=8,strength=0.8,seed=3", any subset
_KEYS = {"mode": str, "ring": int, "smooth": int, "strength": float, "max_sigma": float, "flat": int, "min_count": int, "seed": int}


@dataclasses.dataclass(frozen=True)
class GrainMatchConfig:
    """mode: "luma" adds one noise value per pixel to all three channels, each at its own amplitude (codecs keep luma grain and wipe chroma
    grain); "rgb" an independent value per channel.  ring: width of the band round the mask, in pixels (a box).  smooth: the sums of the frames
    t - smooth .. t + smooth are pooled for frame t's fit (grain is stationary within a shot).  strength: multiplier on the fitted sigma.
    max_sigma: cap on the added sigma, in 8-bit levels.  flat: a ring pixel counts for a channel only where the model's 3 x 3 neighbourhood
    spans at most `flat` levels (texture is not grain).  min_count: a band whose pooled ring has fewer pixels takes the channel's value over
    all bands, and nothing is added where that is short too.  seed: the seed of the noise.  The defaults are build-defined: nobody has
    measured the grain of real footage against the real checkpoints, or run real footage through this stage."""
    mode: str = "luma"
    ring: int = 12
    smooth: int = 4
    strength: float = 1.0
    max_sigma: float = 12.0
    flat: int = 24
    min_count: int = 256
    seed: int = 0

    def __post_init__(self):
        if self.mode not in MODES:
            raise ValueError(f"GrainMatchConfig.mode must be 'luma' or 'rgb', not {self.mode!r}")
        for name in ("ring", "smooth", "flat", "min_count", "seed"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"GrainMatchConfig.{name} must be an integer, not {v!r}")
        for name in ("strength", "max_sigma"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
                raise ValueError(f"GrainMatchConfig.{name} must be a number, not {v!r}")
        if not (1 <= self.ring <= MAX_RING and 0 <= self.smooth <= 16 and 0 <= self.strength <= 2 and 0 <= self.max_sigma <= 15.9
                and 0 <= self.flat <= 255 and self.min_count >= 1 and 0 <= self.seed <= 2 ** 31 - 1):
            raise ValueError(f"GrainMatchConfig: 1 <= ring <= {MAX_RING}, 0 <= smooth <= 16, 0 <= strength <= 2, 0 <= max_sigma <= 15.9, "
                             f"0 <= flat <= 255, min_count >= 1 and 0 <= seed <= 2^31 - 1 are supported, not {self}")


def as_config(grain_match):
    """None / False / "off" / "none" / "" -> None (no grain matching); "on" (or True) -> GrainMatchConfig(); "luma" / "rgb" -> the defaults with
    that mode; "mode=rgb,ring=8,strength=0.8,seed=3" (any subset, each key once) -> the defaults with those fields; a GrainMatchConfig as it is."""
    if grain_match is None or grain_match is False:
        return None
    if grain_match is True:
        return GrainMatchConfig()
    if isinstance(grain_match, GrainMatchConfig):
        return grain_match
    if isinstance(grain_match, str):
        s = grain_match.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return GrainMatchConfig()
        if s in MODES:
            return GrainMatchConfig(mode=s)
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or key in kw:
                break
            kw[key] = val if _KEYS[key] is str else _number(_KEYS[key], val)
            if kw[key] is None:
                break
        else:
            return GrainMatchConfig(**kw)
    raise ValueError("grain_match must be None, 'on', 'off', 'luma', 'rgb', 'mode=..,ring=N,smooth=N,strength=X,max_sigma=X,flat=N,min_count=N,seed=N' "
                     f"(any subset) or a GrainMatchConfig, not {grain_match!r}")


class GrainFit(NamedTuple):
    """The fit of one window, per frame, channel and band: the flat ring pixels of the frame's own ring, the grain (sigma, 8-bit levels) of the
    original and of the model's rendering over the pooled ring, and the sigma of the noise that is added (0: nothing is added)."""
    n: np.ndarray               # [T,3,4] int64
    sigma_orig: np.ndarray      # [T,3,4] float64
    sigma_model: np.ndarray     # [T,3,4] float64
    sigma_added: np.ndarray     # [T,3,4] float64


def variances(sums, cfg):
    """The part of fit that grainshape.fit shares: sums [T,36] int64 -> (own [T,3,4,3] = the sums as given, live [T,3,4] bool, den [T,3,4] =
    36 n of the pooled ring (36 where not live), sx, sy [T,3,4] int64 = the pooled sums of the band, or of the channel where the band is short)."""
    sums = np.asarray(sums, np.int64).reshape(-1, 3, BANDS, 3)
    T = len(sums)
    p = pool(sums.reshape(T, NSUM), cfg.smooth).reshape(T, 3, BANDS, 3)
    whole = np.broadcast_to(p.sum(axis=2, keepdims=True), p.shape)
    use = np.where((p[..., :1] >= cfg.min_count), p, whole)                     # the band's own sums, else the channel's
    n, sx, sy = use[..., 0], use[..., 1], use[..., 2]
    live = (n >= cfg.min_count) & (sums[..., 0].sum(axis=(1, 2)) > 0)[:, None, None]
    den = OP_GAIN * np.where(live, n, 1).astype(np.float64)
    return sums, live, den, sx, sy


def fit(sums, cfg):
    """sums [T,36] int64 (a frame this rank does not hold, or without a ring: zeros) -> GrainFit.  Frame t is fitted to the pooled sums of frames
    t - smooth .. t + smooth.  Per channel and band in fp64: var = (Sy - Sx) / (36 n), the difference taken on the integers; a band whose pooled
    n < min_count takes the channel's sums over all four bands, and 0 where those are short of min_count too; sigma_added = min(strength *
    sqrt(max(var, 0)), max_sigma).  A frame whose own ring holds no counted pixel gets 0.  Where Sx == Sy the result is exactly 0.0."""
    sums, live, den, sx, sy = variances(sums, cfg)
    sigma = lambda s: np.where(live, np.sqrt(np.maximum(s, 0).astype(np.float64) / den), 0.0)
    added = np.minimum(float(cfg.strength) * sigma(sy - sx), float(cfg.max_sigma))
    return GrainFit(sums[..., 0].copy(), sigma(sy), sigma(sx), added)


def tables(sigma_added):
    """sigma_added [..., 3, 4] -> uint8 [..., 3, 256]: the amplitude in Q4, rint(16 sigma(v)), for every value v, sigma(v) interpolated linearly
    between the band centres 32, 96, 160, 224 and held flat beyond 32 and 224.  All-zero sigma: an all-zero table."""
    s = np.asarray(sigma_added, np.float64)
    v = np.arange(256, dtype=np.float64)
    k = np.clip(np.floor((v - CENTRES[0]) / 64.0).astype(np.int64), 0, BANDS - 2)
    f = np.clip((v - CENTRES[0]) / 64.0 - k, 0.0, 1.0)
    at = s[..., k] * (1.0 - f) + s[..., k + 1] * f
    return np.ascontiguousarray(np.clip(np.rint(16.0 * at), 0, 255).astype(np.uint8))
