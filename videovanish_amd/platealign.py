"""Clean-plate alignment: the settings of the tracker that lets the clean-plate fill follow a panning camera, and the host's part of its plan
(pure host logic, no torch; covered by CPU tests).

The clean-plate fill (platefill.py) needs the background at the same place in every frame, so a camera that moves at all fills only flat areas.
With plate_align the stage first finds, per frame of a segment, ONE integer translation against a held key frame (a coarse-to-fine search of
the sum of absolute luma differences over the unmasked pixels; kernels: csrc/vv_align.hip), lays the masks out on a canvas in which the
background stands still, and runs the unchanged fill there (infill.plate_fill(acfg=)).  A gather stays an exact copy of real bytes; what one
translation cannot express (sub-pixel residue, rotation, zoom, parallax) makes a pixel unsteady, and it stays with the model.

  levels         the coarsest pyramid level the search may start at (the level actually used keeps min(H, W) >> L >= 16)
  radius         the search radius at that level, in its pixels, round the prediction
  min_overlap    per cent of a level's pixels a displacement must compare to be eligible
  max_residual   the largest mean absolute luma difference at level 0 with which a frame counts as tracked

The rules are the ABI and stand in include/vvalign.h; guarantees, limits and measurements: DESIGN.md, "Clean-plate alignment".
"""
import dataclasses

MAX_LEVELS = 6          # the limits of include/vvalign.h
MAX_RADIUS = 8
MAX_PIXELS = 1 << 24
MAX_T = 65535
MIN_SIDE = 16           # px: the smaller side of the coarsest level used
SPELLINGS = ("on",)     # what --plate-align / $VV_PLATE_ALIGN / plate_align= accept as a word (besides "off"); also "levels=4,radius=4,...", any subset
_KEYS = ("levels", "radius", "min_overlap", "max_residual")


@dataclasses.dataclass(frozen=True)
class PlateAlignConfig:
    """levels, radius, min_overlap (per cent), max_residual (8-bit levels): see the module's text.  The defaults are build-defined: they come
    from reasoning and synthetic clips; nobody has run real footage through this stage."""
    levels: int = 4
    radius: int = 4
    min_overlap: int = 25
    max_residual: int = 12

    def __post_init__(self):
        for name in _KEYS:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"PlateAlignConfig.{name} must be an integer, not {v!r}")
        if not (0 <= self.levels <= MAX_LEVELS and 1 <= self.radius <= MAX_RADIUS and 1 <= self.min_overlap <= 100 and 0 <= self.max_residual <= 255):
            raise ValueError(f"PlateAlignConfig: 0 <= levels <= {MAX_LEVELS}, 1 <= radius <= {MAX_RADIUS}, 1 <= min_overlap <= 100 and "
                             f"0 <= max_residual <= 255 are supported, not {self}")


def as_config(plate_align):
    """None / False / "off" / "none" / "" -> None (no alignment); "on" (or True) -> PlateAlignConfig(); "levels=4,radius=4,min_overlap=25,
    max_residual=12" (any subset, each key once, integers) -> the defaults with those fields; a PlateAlignConfig as it is."""
    if plate_align is None or plate_align is False:
        return None
    if plate_align is True:
        return PlateAlignConfig()
    if isinstance(plate_align, PlateAlignConfig):
        return plate_align
    if isinstance(plate_align, str):
        s = plate_align.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return PlateAlignConfig()
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or key in kw or not (val.isascii() and val.isdigit()):
                break
            kw[key] = int(val)
        else:
            return PlateAlignConfig(**kw)
    raise ValueError("plate_align must be None, 'on', 'off', 'levels=N,radius=N,min_overlap=N,max_residual=N' (any subset) or a PlateAlignConfig, "
                     f"not {plate_align!r}")


def coarsest_level(H, W, levels):
    """L of include/vvalign.h: the largest l <= levels with min(H, W) >> l >= 16 (0 when even the frame is smaller)."""
    L = 0
    for l in range(1, levels + 1):
        if min(H, W) >> l >= MIN_SIDE:
            L = l
    return L


def trackable(T, H, W):
    """Whether the tracker takes a segment of this size at all (vvalign.h's limits)."""
    return T <= MAX_T and H * W <= MAX_PIXELS


def canvas_box(boxes, off, tracked, align=4):
    """The canvas of one segment: boxes [T,4] = half-open (y0, x0, y1, x1) per frame in frame coordinates, empty where y1 <= y0 or x1 <= x0
    (hip.mask_bbox), off [T,2] = (x, y) per frame, tracked [T] -> the union of the tracked frames' boxes moved by their offsets, in canvas
    coordinates (which may be negative or beyond the frame), x0 rounded down and x1 up to a multiple of `align`; None when no tracked frame
    has a mask pixel."""
    live = [(int(b[0]) + int(o[1]), int(b[1]) + int(o[0]), int(b[2]) + int(o[1]), int(b[3]) + int(o[0]))
            for b, o, k in zip(boxes, off, tracked) if k and b[2] > b[0] and b[3] > b[1]]
    if not live:
        return None
    y0, x0 = min(b[0] for b in live), min(b[1] for b in live)
    y1, x1 = max(b[2] for b in live), max(b[3] for b in live)
    return y0, x0 - x0 % align, y1, -(-x1 // align) * align


def canvas_bytes(T, box):
    """Bytes of the assembled canvas [T, ch, cw, 3] u8."""
    return T * (box[2] - box[0]) * (box[3] - box[1]) * 3


def frame_slices(box, off, H, W):
    """Where frame content lies on the canvas: for the box and one frame's offset (x, y) -> ((canvas rows, canvas columns), (frame rows, frame
    columns)) as slices, or None when the frame does not reach the box."""
    y0, x0, y1, x1 = box
    ox, oy = int(off[0]), int(off[1])
    fy0, fy1 = max(y0 - oy, 0), min(y1 - oy, H)
    fx0, fx1 = max(x0 - ox, 0), min(x1 - ox, W)
    if fy1 <= fy0 or fx1 <= fx0:
        return None
    return ((slice(fy0 + oy - y0, fy1 + oy - y0), slice(fx0 + ox - x0, fx1 + ox - x0)), (slice(fy0, fy1), slice(fx0, fx1)))
