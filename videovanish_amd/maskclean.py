"""Mask clean-up: the settings of the stage between the dilation and the planners (pure host logic, no torch; covered by CPU tests).

roi.py reads the outermost mask pixel of a frame and spans.py asks whether a frame has any: one stray pixel of a thresholded or hand-painted
mask undoes what both save, and a frame whose mask dropped out shows the object again.  The stage (infill.clean_masks; kernels: csrc/vv_mask.hip)
takes the dilated masks and returns what replaces them for everything downstream, in three steps:

  despeckle  the 8-connected components of every dilated frame that hold fewer than min_area RAW mask pixels are cleared
  bridge     per pixel along time, a run of at most `bridge` zero frames between two set frames is set
  grow       out[t] = OR of frames t - grow .. t + grow

Bridge and grow work inside the segments between cuts and never carry a mask across one.  Rules, order, guarantees and limits: DESIGN.md,
"Mask clean-up".
"""
import dataclasses
import math

MAX_BRIDGE = 16         # the limits of vvm_time_bridge_grow (include/vvmask.h)
MAX_GROW = 8
SPELLINGS = ("on",)     # what --mask-clean / $VV_MASK_CLEAN / mask_clean= accept as a word (besides "off"); also "area=64,bridge=2,grow=1", any subset
_KEYS = {"area": "min_area", "bridge": "bridge", "grow": "grow"}


@dataclasses.dataclass(frozen=True)
class MaskCleanConfig:
    """min_area: components of the dilated mask holding fewer raw mask pixels than this are cleared; None = four cells of SAM 2's 256 x 256
    mask-logit grid at the clip's size (area_for); <= 1 clears nothing.  bridge: longest dropout, in frames, that is filled.  grow: frames the
    mask is extended by at both ends of its presence.  The defaults are build-defined: nobody has run SAM 2 with real weights, or real footage,
    through this stage."""
    min_area: object = None
    bridge: int = 2
    grow: int = 0

    def __post_init__(self):
        for name in ("bridge", "grow") + (("min_area",) if self.min_area is not None else ()):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"MaskCleanConfig.{name} must be an integer, not {v!r}")
        if (self.min_area is not None and not 0 <= self.min_area < 2 ** 31) or not 0 <= self.bridge <= MAX_BRIDGE or not 0 <= self.grow <= MAX_GROW:
            raise ValueError(f"MaskCleanConfig: min_area >= 0, 0 <= bridge <= {MAX_BRIDGE} and 0 <= grow <= {MAX_GROW} are supported, not {self}")

    def area_for(self, H, W):
        """The threshold for H x W frames: min_area, or max(1, ceil(4 * H * W / 65536)) (127 px at 1080p, 57 px at 720p)."""
        return self.min_area if self.min_area is not None else max(1, math.ceil(4 * H * W / 65536))


def as_config(mask_clean):
    """None / False / "off" / "none" / "" -> None (no clean-up); "on" (or True) -> MaskCleanConfig(); "area=64,bridge=2,grow=1" (any subset, each
    key once, integers) -> the defaults with those fields; a MaskCleanConfig as it is."""
    if mask_clean is None or mask_clean is False:
        return None
    if mask_clean is True:
        return MaskCleanConfig()
    if isinstance(mask_clean, MaskCleanConfig):
        return mask_clean
    if isinstance(mask_clean, str):
        s = mask_clean.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return MaskCleanConfig()
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or _KEYS[key] in kw or not (val.isascii() and val.isdigit()):
                break
            kw[_KEYS[key]] = int(val)
        else:
            return MaskCleanConfig(**kw)
    raise ValueError(f"mask_clean must be None, 'on', 'off', 'area=N,bridge=N,grow=N' (any subset) or a MaskCleanConfig, not {mask_clean!r}")
