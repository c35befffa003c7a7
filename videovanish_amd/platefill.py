"""Clean-plate fill: the settings of the stage between the mask clean-up and the planners, and the host's part of its plan (pure host logic, no
torch; covered by CPU tests).

Every masked pixel goes to the diffusion model, yet behind an object that crosses a locked-off shot most of them are visible, as real pixels, a
few frames earlier or later at the same place.  The stage (infill.plate_fill; kernels: csrc/vv_plate.hip) takes the frames and the dilated masks
and returns what replaces both for everything downstream: a masked pixel whose background the shot shows steadily is filled with the bytes of
the nearest frame that shows it and leaves the mask; what is never revealed stays with the model.  Per segment between cuts and per pixel:

  sample    a frame is a sample of the pixel when the pixel is unmasked in it and in the `guard` frames either side
  steady    at least min_samples samples whose standard deviation is at most tol in every channel
  usable    a sample within outlier * tol of the pixel's mean in every channel
  source    the usable sample nearest in time to the masked frame (the earlier one at a tie), at most max_gap frames away when max_gap > 0
  margin    the masked pixels without a source, dilated `margin` times inside the mask, stay masked; all others are filled

The rules are the ABI and stand in include/vvplate.h; guarantees, limits and measurements: DESIGN.md, "Clean-plate fill".
"""
import dataclasses

MAX_GUARD = 8           # the limits of include/vvplate.h
MAX_TOL = 255
MAX_OUTLIER = 64
MAX_GAP = 65535
MAX_T = 65535
MAX_MARGIN = 16         # iterations of the 3 x 3 cross
SPELLINGS = ("on",)     # what --plate-fill / $VV_PLATE_FILL / plate_fill= accept as a word (besides "off"); also "guard=1,tol=6,...", any subset
_KEYS = ("guard", "min_samples", "tol", "outlier", "max_gap", "margin", "max_bytes")


@dataclasses.dataclass(frozen=True)
class PlateFillConfig:
    """guard: frames either side of a mask's presence that give no sample (motion blur, the contact shadow).  min_samples: samples a pixel needs.
    tol: largest standard deviation of the samples, per channel, in 8-bit levels (grain passes, a moving background does not).  outlier: a sample
    further than outlier * tol from the mean is not pasted.  max_gap: largest distance in frames between a masked frame and its source, 0 = any.
    margin: pixels the unfilled remainder is grown by inside the mask.  max_bytes: a segment whose uploaded crop [T, h, w, 3] is larger is left
    unfilled.  The defaults are build-defined: they come from reasoning and synthetic clips; nobody has run real footage through this stage."""
    guard: int = 1
    min_samples: int = 4
    tol: int = 6
    outlier: int = 3
    max_gap: int = 0
    margin: int = 2
    max_bytes: int = 1 << 30

    def __post_init__(self):
        for name in _KEYS:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"PlateFillConfig.{name} must be an integer, not {v!r}")
        if not (0 <= self.guard <= MAX_GUARD and 1 <= self.min_samples <= MAX_T and 0 <= self.tol <= MAX_TOL and 0 <= self.outlier <= MAX_OUTLIER
                and 0 <= self.max_gap <= MAX_GAP and 0 <= self.margin <= MAX_MARGIN and 0 <= self.max_bytes < 2 ** 62):
            raise ValueError(f"PlateFillConfig: 0 <= guard <= {MAX_GUARD}, 1 <= min_samples <= {MAX_T}, 0 <= tol <= {MAX_TOL}, 0 <= outlier <= "
                             f"{MAX_OUTLIER}, 0 <= max_gap <= {MAX_GAP}, 0 <= margin <= {MAX_MARGIN} and max_bytes >= 0 are supported, not {self}")


def as_config(plate_fill):
    """None / False / "off" / "none" / "" -> None (no fill); "on" (or True) -> PlateFillConfig(); "guard=1,min_samples=4,tol=6,outlier=3,max_gap=0,
    margin=2,max_bytes=N" (any subset, each key once, integers) -> the defaults with those fields; a PlateFillConfig as it is."""
    if plate_fill is None or plate_fill is False:
        return None
    if plate_fill is True:
        return PlateFillConfig()
    if isinstance(plate_fill, PlateFillConfig):
        return plate_fill
    if isinstance(plate_fill, str):
        s = plate_fill.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return PlateFillConfig()
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or key in kw or not (val.isascii() and val.isdigit()):
                break
            kw[key] = int(val)
        else:
            return PlateFillConfig(**kw)
    raise ValueError("plate_fill must be None, 'on', 'off', 'guard=N,min_samples=N,tol=N,outlier=N,max_gap=N,margin=N,max_bytes=N' (any subset) or a "
                     f"PlateFillConfig, not {plate_fill!r}")


def crop_box(boxes, H, W, align=4):
    """The crop of one segment: boxes [T,4] = half-open (y0, x0, y1, x1) per frame, empty where y1 <= y0 or x1 <= x0 (hip.mask_bbox) -> the union
    (y0, x0, y1, x1) with x0 rounded down and x1 up to a multiple of `align` (x1 at most W: the kernels' 4-pixel form needs a width that is a
    multiple of 4), or None when every box is empty.  Widening the crop changes no result: the rules are per pixel but for the margin, and the
    margin never leaves the mask."""
    live = [(int(b[0]), int(b[1]), int(b[2]), int(b[3])) for b in boxes if b[2] > b[0] and b[3] > b[1]]
    if not live:
        return None
    y0, x0 = min(b[0] for b in live), min(b[1] for b in live)
    y1, x1 = max(b[2] for b in live), max(b[3] for b in live)
    x0 -= x0 % align
    x1 = min(W, -(-x1 // align) * align)
    return max(y0, 0), max(x0, 0), min(y1, H), x1


def crop_bytes(T, box):
    """Bytes of the uploaded crop [T, h, w, 3] u8."""
    return T * (box[2] - box[0]) * (box[3] - box[1]) * 3
