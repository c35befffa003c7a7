"""Block-matched inpaint deflicker: the settings of the motion search that lets the deflicker follow more than one plane of motion, and the
host's reading of its statistics (pure host logic, numpy only, no torch; covered by CPU tests).

The deflicker (deflicker.py) filters at a fixed frame place and deflicker_align (deflickeralign.py) along ONE integer translation per frame.
Parallax, a slow zoom, traffic behind a logo, water or foliage behind a timestamp are more than one translation: where the picture has texture
every neighbour fails the `tol` gate, the filter accepts one sample per pixel -- the pixel itself -- and the patch shimmers as if the stage were
off.  With deflicker_local every block x block pixels of a window get one integer displacement per temporal neighbour, found by block matching
on the window's own pixels (csrc/vv_flicklocal.hip, vvk_search: the smallest byte SAD plus lam (|dy| + |dx|) among the displacements of at most
`search` px that keep the whole block inside the neighbour's window), and the filter reads each neighbour there (vvk_hold; rules:
include/flicklocal.h).  It relates to deflicker as deflicker_align does and composes with it: the search then starts from the tracked
translation.  The gate is unchanged: a wrong vector fails it, so no output byte moves more than `tol` levels from the model's own byte.

  block    8 or 16: the side of a block in window pixels
  search   0 .. 8: the largest |dy| and |dx| tried per temporal neighbour; 0 leaves the filter where deflicker (or deflicker_align) reads it
  lam      0 .. 65535: what a pixel of displacement costs, in summed byte differences of a block; it keeps flat blocks at the zero vector

The rule is the ABI and stands in include/flicklocal.h; guarantees, limits and measurements: DESIGN.md, "Block-matched inpaint deflicker".
"""
import dataclasses
from typing import NamedTuple

import numpy as np

BLOCKS = (8, 16)        # the limits of include/flicklocal.h
MAX_SEARCH = 8
MAX_LAM = 65535
NSTAT = 6               # per frame and slot: blocks matched, moved, sum |dy| + |dx|, largest max(|dy|, |dx|), sum of the winners' costs, sum of the zero candidate's
SPELLINGS = ("on",)     # what --deflicker-local / $VV_DEFLICKER_LOCAL / deflicker_local= accept as a word (besides "off"); also "block=8,search=4,lam=32", any subset
_KEYS = ("block", "search", "lam")


@dataclasses.dataclass(frozen=True)
class DeflickerLocalConfig:
    """block (px), search (px), lam (summed byte differences per px of displacement): see the module's text.  The defaults are build-defined:
    they come from reasoning and synthetic clips; nobody has run real footage or real checkpoints through the stage."""
    block: int = 8
    search: int = 4
    lam: int = 32

    def __post_init__(self):
        for name in _KEYS:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"DeflickerLocalConfig.{name} must be an integer, not {v!r}")
        if self.block not in BLOCKS or not (0 <= self.search <= MAX_SEARCH and 0 <= self.lam <= MAX_LAM):
            raise ValueError(f"DeflickerLocalConfig: block in {BLOCKS}, 0 <= search <= {MAX_SEARCH} and 0 <= lam <= {MAX_LAM} are supported, not {self}")


def as_config(deflicker_local):
    """None / False / "off" / "none" / "" -> None (no search); "on" (or True) -> DeflickerLocalConfig(); "block=8,search=4,lam=32" (any subset,
    each key once, integers) -> the defaults with those fields; a DeflickerLocalConfig as it is."""
    if deflicker_local is None or deflicker_local is False:
        return None
    if deflicker_local is True:
        return DeflickerLocalConfig()
    if isinstance(deflicker_local, DeflickerLocalConfig):
        return deflicker_local
    if isinstance(deflicker_local, str):
        s = deflicker_local.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return DeflickerLocalConfig()
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or key in kw or not (val.isascii() and val.isdigit()):
                break
            kw[key] = int(val)
        else:
            return DeflickerLocalConfig(**kw)
    raise ValueError("deflicker_local must be None, 'on', 'off', 'block=N,search=N,lam=N' (any subset) or a DeflickerLocalConfig, "
                     f"not {deflicker_local!r}")


class DeflickerLocalFit(NamedTuple):
    """What the search found in one window, per frame, over its temporal neighbours: the blocks matched (block and neighbour pairs with a
    winner), how many of them moved (a non-zero vector), the mean |dy| + |dx| and the largest max(|dy|, |dx|) over the matched ones, and the
    winners' summed cost against the zero candidate's where that one was valid."""
    blocks: np.ndarray          # [T] int64
    moved: np.ndarray           # [T] int64
    mean_vector: np.ndarray     # [T] float64
    max_vector: np.ndarray      # [T] int64
    cost: np.ndarray            # [T] int64
    cost_zero: np.ndarray       # [T] int64


def fit(stats):
    """stats [T,2 radius+1,6] int64 (a frame this rank does not hold: zeros) -> DeflickerLocalFit: the slots of a frame summed (the largest
    vector: their maximum)."""
    stats = np.asarray(stats, np.int64)
    stats = stats.reshape(stats.shape[0], -1, NSTAT)
    total = stats.sum(1)
    blocks = total[:, 0]
    return DeflickerLocalFit(blocks.copy(), total[:, 1].copy(), total[:, 2] / np.maximum(blocks, 1), stats[:, :, 3].max(1, initial=0), total[:, 4].copy(),
                             total[:, 5].copy())
