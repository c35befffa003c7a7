"""Clean-plate grain: the settings of the source rotation of the clean-plate fill (pure host logic, no torch; covered by CPU tests).

The clean-plate fill (platefill.py) gives every masked frame of a steady pixel the bytes of the nearest usable frame, so one frame's grain
stands still inside the fill for as long as that frame stays the nearest, while the grain round the fill moves.  With plate_grain the fill
takes its bytes from a few usable frames in turn (infill.plate_fill(gcfg=); kernel: vvl_sources of csrc/vv_plate.hip): still real bytes of
the clip at that place, the same pixels filled, and grain that changes from frame to frame.  Per masked frame t of a pixel:

  side          that of the nearest usable frame (the fill's source), before or after t
  candidates    that source and the next usable frames going away from t on its side, `depth` of them at most, none further than `reach`
                frames from the source (nor than the fill's max_gap from t)
  live source   candidate number t mod (the number of candidates kept)

The rule is the ABI and stands in include/vvplategrain.h; guarantees, limits and measurements: DESIGN.md, "Clean-plate grain".
"""
import dataclasses

MAX_DEPTH = 8           # the limits of include/vvplategrain.h
MAX_REACH = 65535
SPELLINGS = ("on",)     # what --plate-grain / $VV_PLATE_GRAIN / plate_grain= accept as a word (besides "off"); also "depth=4,reach=8", any subset
_KEYS = ("depth", "reach")


@dataclasses.dataclass(frozen=True)
class PlateGrainConfig:
    """depth: the usable frames a masked frame's bytes rotate over, 1 = the nearest alone (the fill as it is without this option).  reach: the
    furthest a rotated source may lie from the nearest one, in frames, so that slow drift is still followed.  The defaults are build-defined:
    they come from reasoning and synthetic clips; nobody has run real footage through this stage."""
    depth: int = 4
    reach: int = 8

    def __post_init__(self):
        for name in _KEYS:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"PlateGrainConfig.{name} must be an integer, not {v!r}")
        if not (1 <= self.depth <= MAX_DEPTH and 1 <= self.reach <= MAX_REACH):
            raise ValueError(f"PlateGrainConfig: 1 <= depth <= {MAX_DEPTH} and 1 <= reach <= {MAX_REACH} are supported, not {self}")


def as_config(plate_grain):
    """None / False / "off" / "none" / "" -> None (the nearest source); "on" (or True) -> PlateGrainConfig(); "depth=4,reach=8" (any subset,
    each key once, integers) -> the defaults with those fields; a PlateGrainConfig as it is."""
    if plate_grain is None or plate_grain is False:
        return None
    if plate_grain is True:
        return PlateGrainConfig()
    if isinstance(plate_grain, PlateGrainConfig):
        return plate_grain
    if isinstance(plate_grain, str):
        s = plate_grain.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return PlateGrainConfig()
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or key in kw or not (val.isascii() and val.isdigit()):
                break
            kw[key] = int(val)
        else:
            return PlateGrainConfig(**kw)
    raise ValueError(f"plate_grain must be None, 'on', 'off', 'depth=N,reach=N' (any subset) or a PlateGrainConfig, not {plate_grain!r}")
