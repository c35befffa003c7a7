"""Inpaint deflicker: the settings and the report arithmetic of the first stage that works along time (pure host logic, numpy only, no torch;
covered by CPU tests).

What stays with the model after the clean-plate fill is the never-revealed part, and the model renders it as T separate hallucinations of one
background: the pasted patch shimmers and pumps from frame to frame while the real pixels round it hold still.  Tone matching removes what one
gain and offset per frame can express; this stage takes what varies per pixel.  The rule is Lee's sigma filter along time: a pixel of the
model's output becomes the rounded mean of those temporal neighbours (at most `radius` frames away, inside the clip call) that lie within `tol`
levels of it in all three channels.  What changes over time by less than `tol` is flicker and is averaged; what changes by more is a moving
edge or a real change of the background and is left as it is: the failure mode is "not smoothed", never "ghosted", because no output byte
moves more than `tol` levels from the model's own byte.  The device filters (csrc/vv_flicker.hip), in front of tone matching, membrane blending
and grain matching, which all measure the filtered rendering (infill.finish); this module turns the device's 12 integer sums per frame into the
report (fit).

  radius   the temporal neighbours are the frames t - radius .. t + radius of the clip call
  tol      8-bit levels: a neighbour is accepted when it differs by at most tol in every channel

The rule is the ABI and stands in include/vvflicker.h; guarantees, limits and measurements: DESIGN.md, "Inpaint deflicker".
"""
import dataclasses
from typing import NamedTuple

import numpy as np

MAX_RADIUS = 4          # the limits of include/vvflicker.h
MAX_TOL = 255
MAX_T = 65535
NSUM = 12               # per frame: pixels, pixels changed, sum n, sum |out_c - in_c| (c = 0, 1, 2); the same over the masked pixels
SPELLINGS = ("on",)     # what --deflicker / $VV_DEFLICKER / deflicker= accept as a word (besides "off"); also "radius=2,tol=12", any subset
_KEYS = ("radius", "tol")


@dataclasses.dataclass(frozen=True)
class DeflickerConfig:
    """radius (frames), tol (8-bit levels): see the module's text.  radius = 0 or tol = 0 leave every pixel as it is.  The defaults are
    build-defined: they come from reasoning and synthetic clips; nobody has measured the flicker of the real checkpoints."""
    radius: int = 2
    tol: int = 12

    def __post_init__(self):
        for name in _KEYS:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"DeflickerConfig.{name} must be an integer, not {v!r}")
        if not (0 <= self.radius <= MAX_RADIUS and 0 <= self.tol <= MAX_TOL):
            raise ValueError(f"DeflickerConfig: 0 <= radius <= {MAX_RADIUS} and 0 <= tol <= {MAX_TOL} are supported, not {self}")


def as_config(deflicker):
    """None / False / "off" / "none" / "" -> None (no deflicker); "on" (or True) -> DeflickerConfig(); "radius=2,tol=12" (any subset, each key
    once, integers) -> the defaults with those fields; a DeflickerConfig as it is."""
    if deflicker is None or deflicker is False:
        return None
    if deflicker is True:
        return DeflickerConfig()
    if isinstance(deflicker, DeflickerConfig):
        return deflicker
    if isinstance(deflicker, str):
        s = deflicker.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return DeflickerConfig()
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or key in kw or not (val.isascii() and val.isdigit()):
                break
            kw[key] = int(val)
        else:
            return DeflickerConfig(**kw)
    raise ValueError(f"deflicker must be None, 'on', 'off', 'radius=N,tol=N' (any subset) or a DeflickerConfig, not {deflicker!r}")


class DeflickerFit(NamedTuple):
    """What the filter did in one window, per frame, over the whole window and over its masked pixels (`_mask`): the pixels counted, the pixels
    with any byte changed, the mean number of accepted samples (1 = nothing but the pixel itself; 0 where no pixel was counted) and the mean
    |out - in| per channel in 8-bit levels."""
    n: np.ndarray               # [T] int64
    changed: np.ndarray         # [T] int64
    samples: np.ndarray         # [T] float64
    shift: np.ndarray           # [T,3] float64
    n_mask: np.ndarray          # [T] int64
    changed_mask: np.ndarray    # [T] int64
    samples_mask: np.ndarray    # [T] float64
    shift_mask: np.ndarray      # [T,3] float64


def fit(sums):
    """sums [T,12] int64 (a frame this rank does not hold: zeros) -> DeflickerFit: the closed forms of the exact integer sums."""
    sums = np.asarray(sums, np.int64).reshape(-1, NSUM)
    out = []
    for k in (0, 6):
        n = sums[:, k]
        d = np.maximum(n, 1).astype(np.float64)
        out += [n.copy(), sums[:, k + 1].copy(), sums[:, k + 2] / d, sums[:, k + 3:k + 6] / d[:, None]]
    return DeflickerFit(*out)
