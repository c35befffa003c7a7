"""Overlay masking: the settings of the stage between the mask clean-up and the shadow masking (pure host logic, no torch, no numpy; covered
by CPU tests).

A station logo, a channel bug or the frame of a timestamp is the one object a user would otherwise outline by hand, and the one the clip gives
away: its edges stand at the same pixels in every frame while the picture under them changes.  The stage (infill.overlay_mask; kernels:
csrc/vv_overlay.hip) takes the frames and the dilated masks (all zero when the user painted none) and returns larger masks; it never changes
a frame byte.  Over the whole clip call and per pixel:

  sums       over the frames in which the pixel is unmasked: the 3 x 3 Sobel responses of the luma, summed with their signs and by magnitude
  strong     at least min_samples samples whose mean gradient magnitude is at least `mag`
  edge       a strong pixel whose signed sums reach `coh` percent of the magnitude sum: the gradient kept its direction
  guard      more than max_share percent of the strong pixels are edges: the scene itself stands still, nothing is added ("static")
  closing    the edges grown by `close` pixels (3 x 3 cross)
  holes      what the closed edges enclose, up to max_hole pixels, away from the frame's border
  selection  parts of at least min_area pixels and at most max_area percent of the frame that do not touch the frame's border (border=1: may)
  fringe     the kept parts grown by `grow` pixels join the mask of every frame

The rules are the ABI and stand in include/overlaymask.h; guarantees, limits and measurements: DESIGN.md, "Overlay masking".
"""
import dataclasses

MAX_T = 65535           # the limits of include/overlaymask.h
MAX_MAG = 2040
MAX_COH = 100
MAX_BOXES = 256
MAX_CLOSE = 16          # vv_mask_collapse_dilate's iterations, as shadowmask.MAX_GROW
MAX_GROW = 16
MAX_AREA = 2 ** 31 - 1
VERDICTS = ("none", "static", "found")
SPELLINGS = ("on",)     # what --overlay-mask / $VV_OVERLAY_MASK / overlay_mask= accept as a word (besides "off"); also "mag=8,coh=80,...", any subset
_KEYS = ("min_samples", "mag", "coh", "max_share", "close", "max_hole", "min_area", "max_area", "border", "grow", "max_bytes")


@dataclasses.dataclass(frozen=True)
class OverlayMaskConfig:
    """min_samples: unmasked frames a pixel needs.  mag: least mean |gx| + |gy| of a strong pixel, in Sobel units of 8-bit luma.  coh: least
    |sum gx| + |sum gy| of an edge, in percent of the magnitude sum.  max_share: largest share of edges among the strong pixels, in percent,
    above which the clip is called static and left alone.  close: pixels the edges are grown by before holes are filled.  max_hole: largest
    enclosed hole that is filled, in pixels.  min_area: smallest kept part in pixels.  max_area: largest kept part in percent of the frame.
    border: 1 keeps parts whose bounding box touches the frame's border.  grow: pixels the kept parts are grown by.  max_bytes: bounds one
    uploaded batch of frames (a batch holds at least one frame).  The defaults are build-defined: they come from synthetic clips; nobody has
    run real footage through this stage."""
    min_samples: int = 12
    mag: int = 8
    coh: int = 80
    max_share: int = 25
    close: int = 2
    max_hole: int = 4096
    min_area: int = 64
    max_area: int = 10
    border: int = 0
    grow: int = 3
    max_bytes: int = 1 << 30

    def __post_init__(self):
        for name in _KEYS:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"OverlayMaskConfig.{name} must be an integer, not {v!r}")
        if not (1 <= self.min_samples <= MAX_T and 1 <= self.mag <= MAX_MAG and 1 <= self.coh <= MAX_COH and 0 <= self.max_share <= 100
                and 0 <= self.close <= MAX_CLOSE and 0 <= self.max_hole <= MAX_AREA and 0 <= self.min_area <= MAX_AREA and 1 <= self.max_area <= 100
                and self.border in (0, 1) and 0 <= self.grow <= MAX_GROW and 0 <= self.max_bytes < 2 ** 62):
            raise ValueError(f"OverlayMaskConfig: 1 <= min_samples <= {MAX_T}, 1 <= mag <= {MAX_MAG}, 1 <= coh <= {MAX_COH}, 0 <= max_share <= 100, "
                             f"0 <= close <= {MAX_CLOSE}, 0 <= max_hole <= {MAX_AREA}, 0 <= min_area <= {MAX_AREA}, 1 <= max_area <= 100, border 0 or 1, "
                             f"0 <= grow <= {MAX_GROW} and max_bytes >= 0 are supported, not {self}")

    def max_area_px(self, H, W):
        """Rule 6's 100 * area <= max_area * H * W as a pixel count."""
        return self.max_area * H * W // 100

    def batch_frames(self, H, W):
        """Frames of one uploaded batch: as many as max_bytes holds, at least one."""
        return max(1, self.max_bytes // (H * W * 3))


def as_config(overlay_mask):
    """None / False / "off" / "none" / "" -> None (no stage); "on" (or True) -> OverlayMaskConfig(); "min_samples=12,mag=8,coh=80,max_share=25,
    close=2,max_hole=4096,min_area=64,max_area=10,border=0,grow=3,max_bytes=N" (any subset, each key once, integers) -> the defaults with
    those fields; an OverlayMaskConfig as it is."""
    if overlay_mask is None or overlay_mask is False:
        return None
    if overlay_mask is True:
        return OverlayMaskConfig()
    if isinstance(overlay_mask, OverlayMaskConfig):
        return overlay_mask
    if isinstance(overlay_mask, str):
        s = overlay_mask.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return OverlayMaskConfig()
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or key in kw or not (val.isascii() and val.isdigit()):
                break
            kw[key] = int(val)
        else:
            return OverlayMaskConfig(**kw)
    raise ValueError("overlay_mask must be None, 'on', 'off', 'min_samples=N,mag=N,coh=N,max_share=N,close=N,max_hole=N,min_area=N,max_area=N,border=N,"
                     f"grow=N,max_bytes=N' (any subset) or an OverlayMaskConfig, not {overlay_mask!r}")
