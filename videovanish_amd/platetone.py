"""Clean-plate exposure matching: the settings of the stage in front of the clean-plate fill, the integer fit and the tables (pure host logic on
Python integers; covered by CPU tests).

The clean-plate fill (platefill.py) calls a pixel steady only when its samples agree to `tol` levels across the whole segment, so under
auto-exposure drift or mains flicker nothing is filled.  With plate_tone every frame of a segment is first mapped to the segment's common
exposure, the unchanged fill runs on that, and every filled pixel is mapped back to the exposure of the frame it lands in
(infill.plate_fill(tcfg=); kernels: csrc/vv_platetone.hip).  Per segment between cuts:

  support   the pixels of the widened crop that no frame masks (nor the `guard` frames round a mask) and whose mean over the segment stays
            `floor` levels away from 0 and 255; fewer than min_pixels of them: the segment is unfit and stays as it is
  fit       per frame and channel v ~ a R + b against the segment's mean image R over the support (mode affine, gain or offset), a clamped to
            +-max_gain percent, b to +-max_offset levels
  tables    forward (frame -> common exposure) and back, 256 bytes per frame and channel; a frame whose forward tables are the identity is
            left alone, and a segment of such frames runs the fill as if the option were off

The rules are the ABI and stand in include/platetone.h; guarantees, limits and measurements: DESIGN.md, "Clean-plate exposure matching".
"""
import dataclasses
from typing import NamedTuple

MAX_T = 65535               # the limits of include/platetone.h
MAX_PIXELS = 1 << 24
MAX_RING = 64
MAX_FLOOR = 127
MAX_GAIN = 100
MAX_OFFSET = 255
MAX_MIN_PIXELS = 2 ** 31 - 1
NSUM = 12                   # a row of vve_moments: Sv[3], Svr[3], and on row 0 Sr[3], Srr[3]
MIN_SPREAD = 4              # affine needs D >= MIN_SPREAD^2 n^2: a standard deviation of R over the support of 4 levels
MODES = ("affine", "gain", "offset")
SPELLINGS = ("on",)         # what --plate-tone / $VV_PLATE_TONE / plate_tone= accept as a word (besides "off"); also "mode=affine,ring=32,...", any subset
PATHS = ("matched", "identity", "unfit", "canvas", "skipped")
_KEYS = ("mode", "ring", "floor", "min_pixels", "max_gain", "max_offset")
IDENTITY = bytes(range(256))


@dataclasses.dataclass(frozen=True)
class PlateToneConfig:
    """mode: what is fitted per frame and channel (affine: gain and offset; gain; offset).  ring: pixels the fill's crop is widened by, so that
    the support reaches past the object's union box.  floor: a support pixel's mean lies in [floor, 255 - floor] in every channel.  min_pixels:
    support a segment needs.  max_gain: the largest gain, in percent away from 1 either way.  max_offset: the largest |offset| in 8-bit
    levels.  The defaults are build-defined: they come from reasoning and synthetic clips; nobody has run real footage through this stage."""
    mode: str = "affine"
    ring: int = 32
    floor: int = 16
    min_pixels: int = 1024
    max_gain: int = 25
    max_offset: int = 32

    def __post_init__(self):
        if self.mode not in MODES:
            raise ValueError(f"PlateToneConfig.mode must be one of {MODES}, not {self.mode!r}")
        for name in _KEYS[1:]:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"PlateToneConfig.{name} must be an integer, not {v!r}")
        if not (0 <= self.ring <= MAX_RING and 0 <= self.floor <= MAX_FLOOR and 1 <= self.min_pixels <= MAX_MIN_PIXELS
                and 0 <= self.max_gain <= MAX_GAIN and 0 <= self.max_offset <= MAX_OFFSET):
            raise ValueError(f"PlateToneConfig: 0 <= ring <= {MAX_RING}, 0 <= floor <= {MAX_FLOOR}, 1 <= min_pixels <= {MAX_MIN_PIXELS}, 0 <= max_gain <= "
                             f"{MAX_GAIN} and 0 <= max_offset <= {MAX_OFFSET} are supported, not {self}")


def as_config(plate_tone):
    """None / False / "off" / "none" / "" -> None (no matching); "on" (or True) -> PlateToneConfig(); "mode=affine,ring=32,floor=16,min_pixels=1024,
    max_gain=25,max_offset=32" (any subset, each key once; integers but for mode) -> the defaults with those fields; a PlateToneConfig as it is."""
    if plate_tone is None or plate_tone is False:
        return None
    if plate_tone is True:
        return PlateToneConfig()
    if isinstance(plate_tone, PlateToneConfig):
        return plate_tone
    if isinstance(plate_tone, str):
        s = plate_tone.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return PlateToneConfig()
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or key in kw:
                break
            if key == "mode":
                if val not in MODES:
                    break
                kw[key] = val
            elif not (val.isascii() and val.isdigit()):
                break
            else:
                kw[key] = int(val)
        else:
            return PlateToneConfig(**kw)
    raise ValueError("plate_tone must be None, 'on', 'off', 'mode=affine|gain|offset,ring=N,floor=N,min_pixels=N,max_gain=N,max_offset=N' (any subset) "
                     f"or a PlateToneConfig, not {plate_tone!r}")


class Fit(NamedTuple):
    """One frame and channel: a = an / ad, b = bn / bd (ad, bd > 0), exact."""
    an: int
    ad: int
    bn: int
    bd: int


def fit_channel(n, Sv, Svr, Sr, Srr, cfg):
    """Rule 4 of platetone.h for one frame and channel from the exact sums over the support (n >= 1) -> Fit."""
    n, Sv, Svr, Sr, Srr = int(n), int(Sv), int(Svr), int(Sr), int(Srr)
    mode = cfg.mode
    if mode == "affine":
        an, ad = n * Svr - Sv * Sr, n * Srr - Sr * Sr
        if ad < MIN_SPREAD * MIN_SPREAD * n * n:
            mode = "gain"
    if mode == "gain":
        an, ad = (Sv, Sr) if Sr > 0 else (1, 1)
    elif mode == "offset":
        an, ad = 1, 1
    hi = 100 + cfg.max_gain
    if hi * an < 100 * ad:
        an, ad = 100, hi
    elif 100 * an > hi * ad:
        an, ad = hi, 100
    if mode == "gain":
        return Fit(an, ad, 0, 1)
    bn, bd = Sv * ad - an * Sr, ad * n
    if abs(bn) > cfg.max_offset * bd:
        bn, bd = (cfg.max_offset if bn > 0 else -cfg.max_offset), 1
    return Fit(an, ad, bn, bd)


def forward_table(f):
    """G of rule 5: bytes of 256."""
    den = 2 * f.bd * f.an
    return bytes(min(max((2 * (v * f.bd - f.bn) * f.ad + f.bd * f.an) // den, 0), 255) for v in range(256))


def back_table(f):
    """B of rule 5: bytes of 256."""
    den = 2 * f.ad * f.bd
    return bytes(min(max((2 * (f.an * u * f.bd + f.bn * f.ad) + f.ad * f.bd) // den, 0), 255) for u in range(256))


class SegmentFit(NamedTuple):
    """A segment's tables: fwd and back = T * 3 * 256 bytes each ([T][3][256]), identity = T bytes (1: the frame is left alone), fits [T][3] Fit
    (the identity frames' as fitted), n = the support, fit = False when the segment is unfit."""
    fwd: bytes
    back: bytes
    identity: bytes
    fits: tuple
    n: int
    fit: bool

    @property
    def all_identity(self):
        return all(self.identity)


def fit_segment(n, sums, cfg):
    """Rules 2 (unfit), 4 and 5 for one segment: n = the support, sums = T rows of the 12 integers of vve_moments -> SegmentFit."""
    T = len(sums)
    one = Fit(1, 1, 0, 1)
    if int(n) < cfg.min_pixels:
        return SegmentFit(IDENTITY * (3 * T), IDENTITY * (3 * T), bytes([1]) * T, ((one,) * 3,) * T, int(n), False)
    Sr, Srr = [int(x) for x in sums[0][6:9]], [int(x) for x in sums[0][9:12]]
    fwd, back, ident, fits = [], [], [], []
    for row in sums:
        fs = tuple(fit_channel(n, row[c], row[3 + c], Sr[c], Srr[c], cfg) for c in range(3))
        g = [forward_table(f) for f in fs]
        same = all(x == IDENTITY for x in g)
        fwd += g
        back += [IDENTITY] * 3 if same else [back_table(f) for f in fs]
        ident.append(1 if same else 0)
        fits.append(fs)
    return SegmentFit(b"".join(fwd), b"".join(back), bytes(ident), tuple(fits), int(n), True)
