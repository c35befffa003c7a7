"""Grain shape: the settings and the per-frame fit of the companion of seam grain matching that gives the added grain a SIZE (pure host logic,
numpy only, no torch; covered by CPU tests).

Seam grain matching (grainmatch.py) assumes that the grain the pasted pixels lack is white at pixel scale.  Footage that has been upscaled,
debayered, denoised or compressed carries grain that is spatially correlated: Immerkaer's operator, which reads the top octave only, then
reports a fraction of its level, and pixel-sharp noise of that level is the wrong texture as well.  The model here (include/grainshape.h):
the grain is white noise through the separable kernel [a_x, 1, a_x] (x) [a_y, 1, a_y], 0 <= a <= 0.5, from white to the binomial blur.  The
device adds, next to grain matching's statistic, the lag-1 products of the operator's responses over the ring's pairs of adjacent counted
pixels (csrc/vv_grainshape.hip: 30 integers per frame); this module turns them into a per axis, reads the true level off grain matching's own
variance (the operator's gain on shaped noise is known in closed form) and hands the paste the taps and the amplitude of the white noise in
front of the shaping kernel.  Rules, guarantees and limits: DESIGN.md, "Grain shape".
"""
import dataclasses
from typing import NamedTuple

import numpy as np

from . import grainmatch
from .tonematch import _number, pool

NSUM = 30               # per frame [3 channels][2 axes][pairs, Cx, Cy, Dx, Dy] (include/grainshape.h)
MAX_TAP = 128           # rint(256 a) at a = 0.5
SPELLINGS = ("on",)     # what --grain-shape / $VV_GRAIN_SHAPE / grain_shape= accept as a word (besides "off"); also "max_a=0.5,dead=0.05", any subset
_KEYS = {"max_a": float, "dead": float, "min_pairs": int, "smooth": int, "max_gain": float}


def P0(a):
    """The variance of the [1, -2, 1] response of unit white noise shaped by [a, 1, a]."""
    return 6.0 - 16.0 * a + 14.0 * a * a


def P1(a):
    """Its lag-1 covariance."""
    return -4.0 + 14.0 * a - 12.0 * a * a


def r0(a):
    """The variance of unit white noise shaped by [a, 1, a]."""
    return 1.0 + 2.0 * a * a


def rho(a):
    """P1 / P0: -2/3 at a = 0, 0 at a = 0.5, monotone between."""
    return P1(a) / P0(a)


def a_of(rho_value, max_a=0.5):
    """The root of rho(a) = rho_value in [0, max_a], clamped at both ends (fp64): the smaller root of (14 rho + 12) a^2 - (16 rho + 14) a +
    (6 rho + 4) = 0, whose discriminant is 4 - 64 rho - 80 rho^2."""
    r = np.clip(np.asarray(rho_value, np.float64), -2.0 / 3.0, 0.0)
    a = ((16.0 * r + 14.0) - np.sqrt(np.maximum(4.0 - 64.0 * r - 80.0 * r * r, 0.0))) / (2.0 * (14.0 * r + 12.0))
    return np.clip(a, 0.0, float(max_a))


@dataclasses.dataclass(frozen=True)
class GrainShapeConfig:
    """max_a: the cap on the fitted a (0.5 = the binomial blur, the end of the family: rho(a) turns back beyond about 0.6).  dead: a fitted a
    below this is taken for 0 (white grain scatters round 0).  min_pairs: an axis whose pooled ring has fewer counted pairs keeps a = 0.
    smooth: the sums of the frames t - smooth .. t + smooth are pooled for frame t's shape.  max_gain: the cap on the factor by which the
    level read by Immerkaer's operator is raised (6 at a = 0.5 on both axes).  The defaults are build-defined: nobody has measured the grain
    of real footage, or run real footage through this stage."""
    max_a: float = 0.5
    dead: float = 0.05
    min_pairs: int = 512
    smooth: int = 4
    max_gain: float = 6.0

    def __post_init__(self):
        for name in ("min_pairs", "smooth"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"GrainShapeConfig.{name} must be an integer, not {v!r}")
        for name in ("max_a", "dead", "max_gain"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
                raise ValueError(f"GrainShapeConfig.{name} must be a number, not {v!r}")
        if not (0 <= self.max_a <= 0.5 and 0 <= self.dead <= 0.5 and 1 <= self.min_pairs <= 2 ** 31 - 1 and 0 <= self.smooth <= 16
                and 1 <= self.max_gain <= 6):
            raise ValueError("GrainShapeConfig: 0 <= max_a <= 0.5, 0 <= dead <= 0.5, 1 <= min_pairs <= 2^31 - 1, 0 <= smooth <= 16 and "
                             f"1 <= max_gain <= 6 are supported, not {self}")


def as_config(grain_shape):
    """None / False / "off" / "none" / "" -> None (white grain); "on" (or True) -> GrainShapeConfig(); "max_a=0.5,dead=0.05,min_pairs=512,
    smooth=4,max_gain=6" (any subset, each key once) -> the defaults with those fields; a GrainShapeConfig as it is."""
    if grain_shape is None or grain_shape is False:
        return None
    if grain_shape is True:
        return GrainShapeConfig()
    if isinstance(grain_shape, GrainShapeConfig):
        return grain_shape
    if isinstance(grain_shape, str):
        s = grain_shape.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return GrainShapeConfig()
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or key in kw:
                break
            kw[key] = _number(_KEYS[key], val)
            if kw[key] is None:
                break
        else:
            return GrainShapeConfig(**kw)
    raise ValueError("grain_shape must be None, 'on', 'off', 'max_a=X,dead=X,min_pairs=N,smooth=N,max_gain=X' (any subset) or a GrainShapeConfig, "
                     f"not {grain_shape!r}")


class GrainShapeFit(NamedTuple):
    """The fit of one window.  Per frame, channel and axis (0 = x, 1 = y): the counted pairs of the frame's own ring, rho of the pooled ring (0
    where the axis is not live), the a applied (quantised: taps / 256), and whether the fit was cut at an end of [0, max_a] or fell into the
    dead zone.  Per frame and channel: k, the factor on the level.  Per frame, channel and band: the sigma of the shaped noise at pixel scale.
    taps and amp are what the paste takes."""
    pairs: np.ndarray           # [T,3,2] int64
    rho: np.ndarray             # [T,3,2] float64
    a: np.ndarray               # [T,3,2] float64
    k: np.ndarray               # [T,3] float64
    sigma_pixel: np.ndarray     # [T,3,4] float64
    clamped: np.ndarray         # [T,3,2] bool
    dead: np.ndarray            # [T,3,2] bool
    taps: np.ndarray            # [T,3,2] int32
    amp: np.ndarray             # [T,3,256] uint8


def fit(shape_sums, grain_sums, grain_cfg, cfg):
    """shape_sums [T,30] int64 (vvn_ring_shape_stats), grain_sums [T,36] int64 (vvg_ring_grain_stats), a frame this rank does not hold or
    without a ring: zeros; grain_cfg the grainmatch.GrainMatchConfig, cfg the GrainShapeConfig -> GrainShapeFit.
    Shape: the sums of frames t - smooth .. t + smooth are pooled, in "luma" mode the three channels are summed as well (one shape per frame).
    Per axis the pool is live when it holds >= min_pairs pairs and D = Dy - Dx > 0; then rho = 2 (Cy - Cx) / D (the differences on the
    integers) and a = a_of(rho, max_a); a < dead gives 0; a is quantised to aq / 256, aq = rint(256 a).  An axis that is not live keeps 0.
    Level: k = min(sqrt(36 r0x r0y / (P0x P0y)), max_gain) at the quantised a (exactly 1 at a = 0), sigma_pixel = min(strength k
    sqrt(max(var, 0)), max_sigma) with grainmatch.fit's own var, strength and max_sigma, and amp = grainmatch.tables(sigma_pixel /
    sqrt(r0x r0y)), the white sigma in front of the shaping kernel: with a = 0 on both axes grainmatch's own table."""
    s = np.asarray(shape_sums, np.int64).reshape(-1, 3, 2, 5)
    T = len(s)
    p = pool(s.reshape(T, NSUM), cfg.smooth).reshape(T, 3, 2, 5)
    if grain_cfg.mode == "luma":
        p = np.broadcast_to(p.sum(axis=1, keepdims=True), p.shape)
    n, num, den = p[..., 0], 2 * (p[..., 2] - p[..., 1]), p[..., 4] - p[..., 3]
    live = (n >= cfg.min_pairs) & (den > 0)
    r = np.where(live, num / np.where(live, den, 1).astype(np.float64), 0.0)
    raw = np.where(live, a_of(r), 0.0)
    clamped = live & ((r < -2.0 / 3.0) | (r > 0.0) | (raw > float(cfg.max_a)))                                           # beyond an end of the family
    a = np.minimum(raw, float(cfg.max_a))
    dead = live & (a < float(cfg.dead))
    taps = np.where(dead, 0.0, np.rint(256.0 * a)).astype(np.int32)
    a = taps / 256.0
    shape_var = r0(a[..., 0]) * r0(a[..., 1])                                                                            # [T,3]
    k = np.minimum(np.sqrt(36.0 * shape_var / (P0(a[..., 0]) * P0(a[..., 1]))), float(cfg.max_gain))
    _, glive, gden, sx, sy = grainmatch.variances(grain_sums, grain_cfg)
    sigma = np.where(glive, np.sqrt(np.maximum(sy - sx, 0).astype(np.float64) / gden), 0.0)
    sigma_pixel = np.minimum(float(grain_cfg.strength) * k[..., None] * sigma, float(grain_cfg.max_sigma))
    amp = grainmatch.tables(sigma_pixel / np.sqrt(shape_var)[..., None])
    return GrainShapeFit(s[..., 0].copy(), r, a, k, sigma_pixel, clamped, dead, np.ascontiguousarray(taps), amp)
