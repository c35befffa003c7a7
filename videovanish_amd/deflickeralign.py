"""Aligned inpaint deflicker: the settings of the tracker that lets the deflicker follow a panning camera, and the host's reading of its track
(pure host logic, numpy only, no torch; covered by CPU tests).

The deflicker (deflicker.py) filters at a fixed frame place.  Under a pan or tilt the background moves through that place, every textured pixel
fails the `tol` gate and stays as the model rendered it: the patch shimmers against a background that moves smoothly.  With deflicker_align the
clip call first tracks ONE integer translation per frame on its original frames (the tracker of the clean-plate alignment: platealign.py,
csrc/vv_align.hip, rules: include/vvalign.h), and the filter then reads each temporal neighbour at the place where the same piece of background
sits in that neighbour frame (csrc/vv_flicker.hip, vvc_hold; rules: include/vvflickalign.h).  It relates to deflicker as plate_align relates to
plate_fill.  Translation only: what one translation cannot express (rotation, zoom, parallax, sub-pixel residue) fails the gate and stays
"not smoothed"; no output byte moves more than `tol` levels from the model's own byte.

The grammar and the fields are the tracker's, platealign.PlateAlignConfig's: "on" | "levels=4,radius=4,min_overlap=25,max_residual=12" (any
subset).  The defaults are build-defined: nobody has run real footage through this stage.  Guarantees, limits and measurements: DESIGN.md,
"Aligned inpaint deflicker".
"""
import numpy as np

from . import platealign
from .platealign import PlateAlignConfig as DeflickerAlignConfig      # one class: the settings are the tracker's

SPELLINGS = platealign.SPELLINGS    # what --deflicker-align / $VV_DEFLICKER_ALIGN / deflicker_align= accept as a word (besides "off")
TRACK_BYTES = 1 << 28               # bytes of frames the tracker's pyramid uploads at a time (only the luma planes stay resident)
PATHS = ("tracked", "static", "untracked", "none")


def as_config(deflicker_align):
    """platealign.as_config under this option's name: None / False / "off" / "none" / "" -> None; "on" (or True) -> PlateAlignConfig();
    "levels=4,radius=4,min_overlap=25,max_residual=12" (any subset) -> the defaults with those fields; a PlateAlignConfig as it is."""
    try:
        return platealign.as_config(deflicker_align)
    except ValueError as e:
        raise ValueError(str(e).replace("plate_align", "deflicker_align", 1)) from None


def identity_track(T):
    """The track of a clip nobody tracked: every frame tracked at offset zero against key 0 ([T,8] int32, vvalign.h's record)."""
    track = np.zeros((T, 8), np.int32)
    track[:, 3] = 1
    return track


def path_of(track):
    """"static" when every frame is tracked at offset zero (the unaligned filter gives the same bytes and runs as it is), else "tracked"."""
    track = np.asarray(track)
    return "static" if (track[:, 3] == 1).all() and not track[:, :2].any() else "tracked"
