"""Shadow masking: the settings of the stage between the mask clean-up and the clean-plate fill (pure host logic, no torch, no numpy; covered
by CPU tests).

The pipeline removes what the mask covers and nothing else, and a segmentation or a hand-painted mask covers the object, not the shadow it
casts: the call leaves a shadow with nothing casting it, and the clean-plate fill samples that shadow as background.  The stage
(infill.shadow_mask; kernels: csrc/vv_shadow.hip) takes the frames and the dilated masks and returns larger masks; it never changes a frame
byte.  Per segment between cuts and per pixel:

  sample     a frame is a sample of the pixel when the pixel is unmasked in it and in the `guard` frames either side
  lit        a sample whose channel sum is not more than 3 * tol below the mean of the samples: a shadow only darkens, so this trim drops
             the shadowed samples
  plate      at least min_samples lit samples whose standard deviation is at most tol in every channel; their mean is the clean background
  candidate  an unmasked pixel with a plate of at least `floor` whose three channels stand at lo .. hi percent of the plate, at least `drop`
             levels darker on average, the three ratios within `chroma` percentage points of each other
  growth     per frame, candidates join the mask while they touch it (3 x 3), `reach` times
  small      parts of fewer than min_area added pixels are dropped
  penumbra   what is left is grown by `grow` pixels (3 x 3 cross) and joins the mask

The rules are the ABI and stand in include/vvshadow.h; guarantees, limits and measurements: DESIGN.md, "Shadow masking".
"""
import dataclasses

MAX_GUARD = 8           # the limits of include/vvshadow.h
MAX_TOL = 255
MAX_DROP = 255
MAX_CHROMA = 100
MAX_FLOOR = 255
MAX_REACH = 64
MAX_GROW = 16
MAX_T = 65535
MAX_AREA = 2 ** 31 - 1
SPELLINGS = ("on",)     # what --shadow-mask / $VV_SHADOW_MASK / shadow_mask= accept as a word (besides "off"); also "guard=1,tol=6,...", any subset
_KEYS = ("guard", "min_samples", "tol", "lo", "hi", "drop", "chroma", "floor", "reach", "min_area", "grow", "max_bytes")


@dataclasses.dataclass(frozen=True)
class ShadowMaskConfig:
    """guard: frames either side of a mask's presence that give no sample.  min_samples: lit samples a pixel needs.  tol: largest standard
    deviation of the lit samples, per channel, in 8-bit levels, and the trim's slack.  lo, hi: the darkening, in percent of the plate, a shadow
    lies between.  drop: least mean darkening in levels.  chroma: largest disagreement of the three channels' ratios, in percentage points.
    floor: darkest plate, per channel, a shadow is looked for on.  reach: growth steps from the frame's mask.  min_area: smallest added part
    in pixels.  grow: pixels the added parts are grown by.  max_bytes: a segment whose uploaded crop [T, h, w, 3] is larger is left as it is.
    The defaults are build-defined: they come from reasoning and synthetic clips; nobody has run real footage through this stage."""
    guard: int = 1
    min_samples: int = 4
    tol: int = 6
    lo: int = 30
    hi: int = 90
    drop: int = 12
    chroma: int = 20
    floor: int = 16
    reach: int = 32
    min_area: int = 16
    grow: int = 1
    max_bytes: int = 1 << 30

    def __post_init__(self):
        for name in _KEYS:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"ShadowMaskConfig.{name} must be an integer, not {v!r}")
        if not (0 <= self.guard <= MAX_GUARD and 1 <= self.min_samples <= MAX_T and 0 <= self.tol <= MAX_TOL and 0 <= self.lo <= self.hi <= 100
                and 0 <= self.drop <= MAX_DROP and 0 <= self.chroma <= MAX_CHROMA and 1 <= self.floor <= MAX_FLOOR and 0 <= self.reach <= MAX_REACH
                and 0 <= self.min_area <= MAX_AREA and 0 <= self.grow <= MAX_GROW and 0 <= self.max_bytes < 2 ** 62):
            raise ValueError(f"ShadowMaskConfig: 0 <= guard <= {MAX_GUARD}, 1 <= min_samples <= {MAX_T}, 0 <= tol <= {MAX_TOL}, 0 <= lo <= hi <= 100, "
                             f"0 <= drop <= {MAX_DROP}, 0 <= chroma <= {MAX_CHROMA}, 1 <= floor <= {MAX_FLOOR}, 0 <= reach <= {MAX_REACH}, "
                             f"0 <= min_area <= {MAX_AREA}, 0 <= grow <= {MAX_GROW} and max_bytes >= 0 are supported, not {self}")

    @property
    def widen(self):
        """Pixels an added pixel can lie from the frame's mask: the crop of the masks is widened by this much."""
        return self.reach + self.grow


def as_config(shadow_mask):
    """None / False / "off" / "none" / "" -> None (no stage); "on" (or True) -> ShadowMaskConfig(); "guard=1,min_samples=4,tol=6,lo=30,hi=90,
    drop=12,chroma=20,floor=16,reach=32,min_area=16,grow=1,max_bytes=N" (any subset, each key once, integers) -> the defaults with those fields;
    a ShadowMaskConfig as it is."""
    if shadow_mask is None or shadow_mask is False:
        return None
    if shadow_mask is True:
        return ShadowMaskConfig()
    if isinstance(shadow_mask, ShadowMaskConfig):
        return shadow_mask
    if isinstance(shadow_mask, str):
        s = shadow_mask.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return ShadowMaskConfig()
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or key in kw or not (val.isascii() and val.isdigit()):
                break
            kw[key] = int(val)
        else:
            return ShadowMaskConfig(**kw)
    raise ValueError("shadow_mask must be None, 'on', 'off', 'guard=N,min_samples=N,tol=N,lo=N,hi=N,drop=N,chroma=N,floor=N,reach=N,min_area=N,grow=N,"
                     f"max_bytes=N' (any subset) or a ShadowMaskConfig, not {shadow_mask!r}")


def widen_box(box, H, W, by, align=4):
    """The crop (y0, x0, y1, x1) of platefill.crop_box widened by `by` pixels on every side, clamped to the frame, x0 rounded down and x1 up to
    a multiple of `align` (x1 at most W).  A growth path of rule 5 stays within reach of the mask pixel it starts from and rule 7 adds grow,
    so every pixel the stage can add, and everything that decides it, lies inside this crop: the masks are those of the full frame."""
    y0, x0, y1, x1 = box
    y0, y1 = max(y0 - by, 0), min(y1 + by, H)
    x0, x1 = max(x0 - by, 0), min(x1 + by, W)
    x0 -= x0 % align
    x1 = min(W, -(-x1 // align) * align)
    return y0, x0, y1, x1
