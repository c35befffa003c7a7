"""Seam detail matching: the settings and the per-frame fit of the stage that makes the pasted patch as sharp as the footage round it (pure host
logic, Python integers and numpy for the arrays it hands back, no torch; covered by CPU tests).

The model's frame has been through the fp16 VAE, is usually resized up to the window's size on the way back and may have been averaged along time
by the deflicker: with tone, membrane and grain matched it is a soft island in a crisp frame; over a background that is out of focus or
motion-blurred it is the other way round, a patch crisper than everything round it.  In the ring -- the unmasked pixels of the window within `ring`
pixels of the mask -- both the original pixel y and the model's rendering x of the same pixel exist.  With H the 3 x 3 binomial high-pass, the
least-squares a of H(y) ~ H(x) + a H(H(x)) over the structured part of the ring says how much of its own high-pass x lacks (a > 0) or has too
much of (a < 0); the device sums the ring (csrc/vv_detail.hip: 12 integers per frame), this module turns the sums into one amount per frame
(fit), and a clamped unsharp mask applies it to every pixel of the window before the other seam stages read them (infill.finish).

  ring         width of the band round the mask, in pixels (a box)
  edge         a ring pixel counts for a channel only where the model's 3 x 3 neighbourhood spans at least `edge` levels (flat areas say
               nothing about sharpness: they are grain matching's part of the ring)
  smooth       the sums of the frames t - smooth .. t + smooth of the clip call are pooled for frame t's fit
  min_pixels   a frame whose pooled ring has fewer counted pixels is left as it is
  max_sharpen  cap on a positive amount (1.0 = the whole high-pass added once)
  max_soften   cap on a negative amount (1.0 = the 3 x 3 binomial blur itself)
  dead         an amount smaller than this is taken for 0: a rendering that is as sharp as the footage is not touched
  overshoot    levels a sharpened byte may leave the range of its 3 x 3 neighbourhood by
  strength     multiplier on the fitted amount; 0 applies nothing

The rules are the ABI and stand in include/detailmatch.h; guarantees, limits and measurements: DESIGN.md, "Seam detail matching".
"""
import dataclasses
from typing import NamedTuple

import numpy as np

from .tonematch import _number

MAX_RING, MAX_EDGE, MAX_OVERSHOOT, MAX_AMOUNT, MAX_PIXELS = 32, 255, 255, 1024, 1 << 24       # the limits of include/detailmatch.h
NQ, NSUM = 4, 12        # per frame [3 channels][n, sum D K, sum K K, sum D D]
SPELLINGS = ("on",)     # what --detail-match / $VV_DETAIL_MATCH / detail_match= accept as a word (besides "off"); also "ring=8,edge=12,strength=0.5", any subset
_KEYS = {"ring": int, "edge": int, "smooth": int, "min_pixels": int, "max_sharpen": float, "max_soften": float, "dead": float, "overshoot": int,
         "strength": float}


def q8_of(v):
    """A setting in units of 1 / 256, rounded half up."""
    return int(256.0 * v + 0.5)


@dataclasses.dataclass(frozen=True)
class DetailMatchConfig:
    """See the module's text.  The defaults are build-defined: they come from reasoning and synthetic clips;
    nobody has run real checkpoints through it, or measured how soft their output is."""
    ring: int = 8
    edge: int = 12
    smooth: int = 2
    min_pixels: int = 256
    max_sharpen: float = 2.0
    max_soften: float = 1.0
    dead: float = 0.06
    overshoot: int = 4
    strength: float = 1.0

    def __post_init__(self):
        for name, kind in _KEYS.items():
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int,) if kind is int else (int, float)) or v != v:
                raise ValueError(f"DetailMatchConfig.{name} must be {'an integer' if kind is int else 'a number'}, not {v!r}")
        if not (1 <= self.ring <= MAX_RING and 0 <= self.edge <= MAX_EDGE and 0 <= self.smooth <= 16 and 1 <= self.min_pixels <= 2 ** 31 - 1
                and 0 <= self.max_sharpen <= 4 and 0 <= self.max_soften <= 1 and 0 <= self.dead <= 1 and 0 <= self.overshoot <= MAX_OVERSHOOT
                and 0 <= self.strength <= 1):
            raise ValueError(f"DetailMatchConfig: 1 <= ring <= {MAX_RING}, 0 <= edge <= {MAX_EDGE}, 0 <= smooth <= 16, 1 <= min_pixels <= 2^31 - 1, "
                             f"0 <= max_sharpen <= 4, 0 <= max_soften <= 1, 0 <= dead <= 1, 0 <= overshoot <= {MAX_OVERSHOOT} and 0 <= strength <= 1 "
                             f"are supported, not {self}")


def as_config(detail_match):
    """None / False / "off" / "none" / "" -> None (no detail matching); "on" (or True) -> DetailMatchConfig(); "ring=8,edge=12,strength=0.5" (any
    subset, each key once) -> the defaults with those fields; a DetailMatchConfig as it is."""
    if detail_match is None or detail_match is False:
        return None
    if detail_match is True:
        return DetailMatchConfig()
    if isinstance(detail_match, DetailMatchConfig):
        return detail_match
    if isinstance(detail_match, str):
        s = detail_match.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return DetailMatchConfig()
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or key in kw:
                break
            kw[key] = _number(_KEYS[key], val)
            if kw[key] is None:
                break
        else:
            return DetailMatchConfig(**kw)
    raise ValueError("detail_match must be None, 'on', 'off', 'ring=N,edge=N,smooth=N,min_pixels=N,max_sharpen=X,max_soften=X,dead=X,overshoot=N,"
                     f"strength=X' (any subset) or a DetailMatchConfig, not {detail_match!r}")


class DetailFit(NamedTuple):
    """The fit of one window, per frame: the counted pixels of the frame's own ring (the sum of the three channels' counts // 3), the amount
    applied (the q8 integer / 256: exact; 0 = the frame is left as it is), the mean of D^2 over the frame's own ring before the stage (sum D D
    / n; 0 where n is 0), and whether the cap cut the fitted amount (clamped) or the dead zone took it for 0 (dead)."""
    n: np.ndarray               # [T] int64
    amount: np.ndarray          # [T] float64
    residual: np.ndarray        # [T] float64
    clamped: np.ndarray         # [T] bool
    dead: np.ndarray            # [T] bool


def amount_q8(p_dk, q_kk, count, cfg):
    """Rule 2 of include/detailmatch.h on the pooled integers of one frame: P = sum D K, Q = sum K K, count = the sum of the three channels'
    counts -> (a q8, clamped, dead)."""
    if count // 3 < cfg.min_pixels or q_kk == 0:
        return 0, False, False
    a = (8192 * p_dk + q_kk) // (2 * q_kk)
    lo, hi = -q8_of(cfg.max_soften), q8_of(cfg.max_sharpen)
    clamped = not lo <= a <= hi
    a = min(max(a, lo), hi)
    if abs(a) < q8_of(cfg.dead):
        return 0, clamped, True
    return (a * q8_of(cfg.strength) + 128) >> 8, clamped, False


def fit(sums, cfg):
    """sums [T,12] int64 (a frame this rank does not hold, or without a ring: zeros) -> DetailFit.  Frame t is fitted to the sums of the frames
    t - smooth .. t + smooth, the three channels pooled, in Python integers."""
    rows = [[int(v) for v in row] for row in np.asarray(sums, np.int64).reshape(-1, NSUM)]
    T = len(rows)
    n, amount, residual = np.zeros(T, np.int64), np.zeros(T), np.zeros(T)
    clamped, dead = np.zeros(T, bool), np.zeros(T, bool)
    for t in range(T):
        near = rows[max(0, t - cfg.smooth):t + cfg.smooth + 1]
        count, p_dk, q_kk = (sum(row[c * NQ + k] for row in near for c in range(3)) for k in range(3))
        a, clamped[t], dead[t] = amount_q8(p_dk, q_kk, count, cfg)
        amount[t] = a / 256.0
        n[t] = sum(rows[t][c * NQ] for c in range(3)) // 3
        if n[t]:
            residual[t] = sum(rows[t][c * NQ + 3] for c in range(3)) / int(n[t])
    return DetailFit(n, amount, residual, clamped, dead)


def held_rows(f, idx):
    """The DetailFit f with zero rows for every frame outside idx (the frames this rank holds): a frame another rank holds has no sums here, and
    what its neighbours pooled says nothing about what that rank applies."""
    held = np.zeros(len(f.n), bool)
    held[list(idx)] = True
    return DetailFit(*(np.where(held, v, np.zeros((), v.dtype)) for v in f))


def q8(amount):
    """The amounts of a DetailFit back as the kernel's q8 integers (exact: every amount is a multiple of 1 / 256 inside +-4) -> int32."""
    return np.ascontiguousarray(np.rint(np.asarray(amount, np.float64) * 256.0).astype(np.int32))
