"""Seam membrane blending: the settings, the level plan and the report of the stage in front of the composite (pure host logic, numpy only,
no torch; covered by CPU tests).

Tone matching fits one gain and offset per frame, channel and window; a tone error that varies across the hole (a vignette, a lighting
gradient, the VAE's low-frequency drift, two logos in different light) is left as a step along part of the mask's outline.  On the ring -- the
unmasked pixels of the window within `ring` pixels of the mask -- both the original pixel y and the model's rendering x exist.  The device
(csrc/vv_blend.hip) interpolates the difference y - x harmonically from the ring into the hole -- a membrane, as in Poisson or mean-value
cloning -- with a cascadic multigrid in integers (include/vvblend.h), and the fused paste adds it to every pasted pixel, which then meets the
original at every point of the outline (infill.finish).  Rules, guarantees and limits: DESIGN.md, "Seam membrane blending".
"""
import dataclasses
import math
from typing import NamedTuple

import numpy as np

from .tonematch import _number

MAX_RING = 32           # the limits of include/vvblend.h
MAX_PRESMOOTH = 4
MAX_SWEEPS = 16
MAX_SHIFT = 255
NSUM = 11               # per frame: n ring, sum d_c^2 [3], n unknown, sum |m_c| [3] (Q6), max |m_c| [3] (Q6)
Q = 64                  # the field's unit: 1/64 level
SCRATCH_FACTOR = 4      # finish keeps a group's scratch at or below this many times the bytes of the window's uint8 frames
_KEYS = {"ring": int, "presmooth": int, "sweeps": int, "max_shift": int, "strength": float}


@dataclasses.dataclass(frozen=True)
class SeamBlendConfig:
    """ring: width of the band round the mask whose pixels carry the boundary values, in pixels (a box).  presmooth: a ring pixel's value is the
    mean of y - x over the ring pixels within `presmooth` pixels of it, which keeps the grain of y from being drawn into the hole as streaks.
    sweeps: Jacobi sweeps per level of the cascade.  max_shift: the boundary values stay in [-max_shift, max_shift] (8-bit levels), and so does
    the field.  strength: multiplier on the field.  The defaults are build-defined: they come from reasoning and synthetic tests; nobody has
    run real checkpoints or footage through this stage."""
    ring: int = 12
    presmooth: int = 2
    sweeps: int = 8
    max_shift: int = 32
    strength: float = 1.0

    def __post_init__(self):
        for name in ("ring", "presmooth", "sweeps", "max_shift"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"SeamBlendConfig.{name} must be an integer, not {v!r}")
        v = self.strength
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
            raise ValueError(f"SeamBlendConfig.strength must be a number, not {v!r}")
        if not (1 <= self.ring <= MAX_RING and 0 <= self.presmooth <= MAX_PRESMOOTH and 1 <= self.sweeps <= MAX_SWEEPS
                and 1 <= self.max_shift <= MAX_SHIFT and 0 <= self.strength <= 2):
            raise ValueError(f"SeamBlendConfig: 1 <= ring <= {MAX_RING}, 0 <= presmooth <= {MAX_PRESMOOTH}, 1 <= sweeps <= {MAX_SWEEPS}, "
                             f"1 <= max_shift <= {MAX_SHIFT} and 0 <= strength <= 2 are supported, not {self}")

    @property
    def strength_q8(self):
        """The strength as the paste kernel takes it."""
        return int(round(float(self.strength) * 256.0))


def as_config(seam_blend, feather_px=None):
    """None / False / "off" / "none" / "" -> None (no blending); "on" (or True) -> SeamBlendConfig(); "ring=12,presmooth=2,sweeps=8,max_shift=32,
    strength=1.0" (any subset, each key once) -> the defaults with those fields; a SeamBlendConfig as it is.  With feather_px, a ring that is
    not wider than ceil(feather_px) is refused: every pixel the feather takes from the model has to be a cell of the field."""
    cfg = _parse(seam_blend)
    if cfg is not None and feather_px is not None and cfg.ring <= math.ceil(float(feather_px)):
        raise ValueError(f"seam_blend: ring = {cfg.ring} must be wider than ceil(feather_px) = {math.ceil(float(feather_px))}")
    return cfg


def _parse(seam_blend):
    if seam_blend is None or seam_blend is False:
        return None
    if seam_blend is True:
        return SeamBlendConfig()
    if isinstance(seam_blend, SeamBlendConfig):
        return seam_blend
    if isinstance(seam_blend, str):
        s = seam_blend.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return SeamBlendConfig()
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or key in kw:
                break
            kw[key] = _number(_KEYS[key], val)
            if kw[key] is None:
                break
        else:
            return SeamBlendConfig(**kw)
    raise ValueError("seam_blend must be None, 'on', 'off', 'ring=N,presmooth=N,sweeps=N,max_shift=N,strength=X' (any subset) or a SeamBlendConfig, "
                     f"not {seam_blend!r}")


def level_sizes(h, w):
    """[(h_l, w_l)] of include/vvblend.h: level 0 is the window, every further level halves both sides (ceil), while the larger side is > 2."""
    out = [(int(h), int(w))]
    while max(out[-1]) > 2:
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def level_plan(T, h, w):
    """([(val_offset, cls_offset, h_l, w_l)] in bytes per level, total bytes): the scratch layout of include/vvblend.h for T frames."""
    plan, at = [], 0
    for hl, wl in level_sizes(h, w):
        plan.append((at, at + 6 * T * hl * wl, hl, wl))
        at += (7 * T * hl * wl + 15) & ~15
    return plan, at


def scratch_bytes(T, h, w):
    return level_plan(T, h, w)[1]


def groups(T, h, w):
    """The frame groups [(a, b)] finish solves one after another: the largest group size whose scratch is at most SCRATCH_FACTOR times the bytes
    of the window's T uint8 frames (3 T h w), at least one frame."""
    g = T
    while g > 1 and scratch_bytes(g, h, w) > SCRATCH_FACTOR * 3 * T * h * w:
        g -= 1
    return [(a, min(a + g, T)) for a in range(0, T, g)]


class SeamBlendFit(NamedTuple):
    """What the stage measured in one window, per frame: the ring pixels that gave data, the RMS of y - x on them per channel (after the tone
    table), the pixels of the hole, and the largest and the mean |m| inside it per channel (8-bit levels, before `strength`)."""
    n: np.ndarray               # [T] int64
    rms_diff: np.ndarray        # [T,3] float64
    n_hole: np.ndarray          # [T] int64
    max_shift: np.ndarray       # [T,3] float64
    mean_shift: np.ndarray      # [T,3] float64


def fit(sums):
    """sums [T,11] int64 (a frame this rank does not hold: zeros) -> SeamBlendFit: closed forms of the exact integer sums."""
    s = np.asarray(sums, np.int64).reshape(-1, NSUM)
    n, nh = s[:, 0].copy(), s[:, 4].copy()
    one = lambda k: np.maximum(k, 1).astype(np.float64)[:, None]
    return SeamBlendFit(n, np.sqrt(s[:, 1:4] / one(n)), nh, s[:, 8:11] / float(Q), s[:, 5:8] / (float(Q) * one(nh)))
