"""Clean-plate warp: the settings of the stage that lets the clean-plate fill follow zoom and roll, and the host's part of it: the exact fit of
one affine map per frame, the composition with the key's map, the inverse, the fixed-point tables the device reads and the canvas box (pure host
logic, no torch, no floats in the fit; covered by CPU tests).

plate_align (platealign.py) gives every frame ONE integer translation against a held key.  A hand or a gimbal adds a fraction of a degree of
roll and a per cent of zoom, which at the corners of a frame is several pixels no translation expresses.  With plate_warp the stage matches
whole blocks of every tracked frame against its key round that translation (kernel: csrc/vv_platewarp.hip, vvw_search), fits here
u(x, y) = a + b x + c y and v(x, y) likewise to the blocks' vectors by exact least squares with trimming, and builds and reads the canvas through
the fitted maps with nearest-neighbour gathers (vvw_place, vvw_unplace): a filled byte stays an exact byte of the clip.

  block          side of the matched blocks, 16 or 32 px
  search         the candidates round plate_align's translation, +- px (at most 8): zoom and roll against the held key beyond it are not found
  min_texture    the least mean activity (sum of absolute neighbour differences per pixel) with which a block is matched at all
  min_blocks     the least number of blocks a frame's fit needs after trimming
  trim           tenths of a pixel: a block whose vector lies further from the fit is dropped and the fit repeated
  rounds         how often at most
  max_linear     thousandths: a fit with a larger linear coefficient (zoom, roll, shear) fails

A frame whose fit fails keeps plate_align's translation.  The rules are the ABI and stand in include/platewarp.h; guarantees, limits and
measurements: DESIGN.md, "Clean-plate warp".
"""
import dataclasses
from fractions import Fraction

FRAC_BITS = 20          # the limits of include/platewarp.h
MAX_SEARCH = 8
MAX_T = 65535
MAX_PIXELS = 1 << 24
BLOCKS = (16, 32)
MAX_LINEAR = 250        # thousandths: keeps every fitted map, and so every composition, invertible
ONE = 1 << FRAC_BITS
SPELLINGS = ("on",)     # what --plate-warp / $VV_PLATE_WARP / plate_warp= accept as a word (besides "off"); also "block=16,search=8,...", any subset
_KEYS = ("block", "search", "min_texture", "min_blocks", "trim", "rounds", "max_linear")
IDENTITY = ((Fraction(0), Fraction(1), Fraction(0)), (Fraction(0), Fraction(0), Fraction(1)))


@dataclasses.dataclass(frozen=True)
class PlateWarpConfig:
    """block, search, min_texture, min_blocks, trim (tenths of a pixel), rounds, max_linear (thousandths): see the module's text.  The defaults
    are build-defined: they come from reasoning and synthetic clips; nobody has run real footage through this stage."""
    block: int = 16
    search: int = 8
    min_texture: int = 2
    min_blocks: int = 12
    trim: int = 10
    rounds: int = 3
    max_linear: int = 50

    def __post_init__(self):
        for name in _KEYS:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"PlateWarpConfig.{name} must be an integer, not {v!r}")
        if not (self.block in BLOCKS and 0 <= self.search <= MAX_SEARCH and 0 <= self.min_texture <= 510 and 3 <= self.min_blocks <= 1 << 20 and
                1 <= self.trim <= 1000 and 0 <= self.rounds <= 16 and 0 <= self.max_linear <= MAX_LINEAR):
            raise ValueError(f"PlateWarpConfig: block in {BLOCKS}, 0 <= search <= {MAX_SEARCH}, 0 <= min_texture <= 510, 3 <= min_blocks <= 2^20, "
                             f"1 <= trim <= 1000, 0 <= rounds <= 16 and 0 <= max_linear <= {MAX_LINEAR} are supported, not {self}")


def as_config(plate_warp):
    """None / False / "off" / "none" / "" -> None (no warp); "on" (or True) -> PlateWarpConfig(); "block=16,search=8,min_texture=2,min_blocks=12,
    trim=10,rounds=3,max_linear=50" (any subset, each key once, integers) -> the defaults with those fields; a PlateWarpConfig as it is."""
    if plate_warp is None or plate_warp is False:
        return None
    if plate_warp is True:
        return PlateWarpConfig()
    if isinstance(plate_warp, PlateWarpConfig):
        return plate_warp
    if isinstance(plate_warp, str):
        s = plate_warp.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s == "on":
            return PlateWarpConfig()
        kw = {}
        for item in s.split(","):
            key, eq, val = (x.strip() for x in item.partition("="))
            if not eq or key not in _KEYS or key in kw or not (val.isascii() and val.isdigit()):
                break
            kw[key] = int(val)
        else:
            return PlateWarpConfig(**kw)
    raise ValueError("plate_warp must be None, 'on', 'off', 'block=N,search=N,min_texture=N,min_blocks=N,trim=N,rounds=N,max_linear=N' (any subset) or "
                     f"a PlateWarpConfig, not {plate_warp!r}")


def searchable(T, H, W):
    """Whether vvw_search takes a segment of this size at all (platewarp.h's limits)."""
    return T <= MAX_T and H * W <= MAX_PIXELS


# ---- the fit: exact, in Python integers and Fractions ---------------------------------------------------------------------------------------
def _solve(pts):
    """Least squares of u = a + b' X + c' Y and v likewise over pts = [(X, Y, u, v)] (integers; X, Y = the DOUBLED coordinates of the blocks'
    centres) by Cramer's rule -> (d, (Na, Nb', Nc'), (Na, Nb', Nc')): integers, the coefficients are N / d; or None when the normal matrix is
    singular (fewer than three points, or collinear)."""
    n = sx = sy = sxx = sxy = syy = su = sxu = syu = sv = sxv = syv = 0
    for X, Y, u, v in pts:
        n += 1; sx += X; sy += Y; sxx += X * X; sxy += X * Y; syy += Y * Y
        su += u; sxu += X * u; syu += Y * u; sv += v; sxv += X * v; syv += Y * v
    m = ((n, sx, sy), (sx, sxx, sxy), (sy, sxy, syy))

    def det3(a):
        return (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))

    d = det3(m)
    if d == 0:
        return None
    out = [d]
    for rhs in ((su, sxu, syu), (sv, sxv, syv)):
        out.append(tuple(det3(tuple(tuple(rhs[i] if j == col else m[i][j] for j in range(3)) for i in range(3))) for col in range(3)))
    return tuple(out)


class Fit:
    """One frame's fit: ok, the displacement field ((au, bu, cu), (av, bv, cv)) in pixel coordinates as Fractions (the pure translation d0 when
    the fit failed), the indices of the kept blocks, and the mean squared residual of the kept blocks as a Fraction (0 when failed)."""
    __slots__ = ("ok", "field", "kept", "mse")

    def __init__(self, ok, field, kept, mse):
        self.ok, self.field, self.kept, self.mse = ok, field, kept, mse


def fit_frame(vectors, d0, cfg):
    """vectors = [(bx, by, dx, dy)] of the frame's USED blocks (block indices and the winner of vvw_search), d0 = (x, y) = off[t] - off[key_t]
    -> Fit.  The targets are d0 + (dx, dy) at the blocks' centres; trimming drops the blocks with 100 (rx^2 + ry^2) > trim^2 (of all the
    blocks: one a biased first fit dropped comes back when a later fit passes near it) and refits, until the set is stable or `rounds`
    refits are done.  The fit fails with fewer than min_blocks blocks, a singular normal matrix, or a linear
    coefficient over max_linear / 1000."""
    B = cfg.block
    pts = [(2 * bx * B + B - 1, 2 * by * B + B - 1, int(d0[0]) + dx, int(d0[1]) + dy) for bx, by, dx, dy in vectors]
    failed = Fit(False, ((Fraction(int(d0[0])), Fraction(0), Fraction(0)), (Fraction(int(d0[1])), Fraction(0), Fraction(0))), (), Fraction(0))
    kept = list(range(len(pts)))

    def residuals(sol, idx):
        """d^2 (rx^2 + ry^2) of the blocks idx, in integers: d r = d u - (Na + Nb' X + Nc' Y)."""
        d, (a0, a1, a2), (b0, b1, b2) = sol
        out = []
        for i in idx:
            X, Y, u, v = pts[i]
            rx, ry = d * u - (a0 + a1 * X + a2 * Y), d * v - (b0 + b1 * X + b2 * Y)
            out.append(rx * rx + ry * ry)
        return out

    sol = None
    everyone = range(len(pts))
    for rnd in range(cfg.rounds + 1):
        if len(kept) < cfg.min_blocks:
            return failed
        sol = _solve([pts[i] for i in kept])
        if sol is None:
            return failed
        if rnd == cfg.rounds:
            break
        lim = cfg.trim * cfg.trim * sol[0] * sol[0]
        new = [i for i, r in zip(everyone, residuals(sol, everyone)) if 100 * r <= lim]
        if new == kept:
            break
        kept = new
    # X = 2 x: the slope per pixel is twice the slope per doubled unit
    d = sol[0]
    field = tuple((Fraction(s[0], d), Fraction(2 * s[1], d), Fraction(2 * s[2], d)) for s in sol[1:])
    if any(abs(c) * 1000 > cfg.max_linear for f in field for c in f[1:]):
        return failed
    return Fit(True, field, tuple(kept), Fraction(sum(residuals(sol, kept)), d * d * len(kept)))


# ---- maps: ((ax, bx, cx), (ay, by, cy)) of Fractions, (x, y) -> (ax + bx x + cx y, ay + by x + cy y) -----------------------------------------
def field_map(field):
    """The displacement field (u, v) as the map p -> p + (u(p), v(p))."""
    (au, bu, cu), (av, bv, cv) = field
    return ((au, 1 + bu, cu), (av, bv, 1 + cv))


def compose(outer, inner):
    """outer o inner, exactly."""
    (a, b, c), (d, e, f) = outer
    (ia, ib, ic), (id_, ie, if_) = inner
    return ((a + b * ia + c * id_, b * ib + c * ie, b * ic + c * if_), (d + e * ia + f * id_, e * ib + f * ie, e * ic + f * if_))


def invert(m):
    """The exact inverse; ValueError when the linear part is singular."""
    (a, b, c), (d, e, f) = m
    det = b * f - c * e
    if det == 0:
        raise ValueError("platewarp.invert: the map's linear part is singular")
    ib, ic, ie, if_ = f / det, -c / det, -e / det, b / det
    return ((-(ib * a + ic * d), ib, ic), (-(ie * a + if_ * d), ie, if_))


def to_fixed(m):
    """The map rounded ONCE to FRAC_BITS fraction bits (half up) -> the 6 integers (ax, bx, cx, ay, by, cy) of platewarp.h's rule M."""
    return tuple((2 * v.numerator * ONE + v.denominator) // (2 * v.denominator) for row in m for v in (Fraction(x) for x in row))


def apply_fixed(tab, x, y):
    """Rule M on Python integers (no wrap-around: the tables made here stay far below 2^63 for every coordinate a frame or canvas has)."""
    half = ONE >> 1
    return (tab[0] + tab[1] * x + tab[2] * y + half) >> FRAC_BITS, (tab[3] + tab[4] * x + tab[5] * y + half) >> FRAC_BITS


def translation_table(ox, oy):
    return (int(ox) * ONE, ONE, 0, int(oy) * ONE, 0, ONE)


class Plan:
    """A segment's maps: fits [T] (a Fit, or None for frame 0, an untracked frame and a frame with no key), maps [T] frame -> canvas (Fractions;
    None for an untracked frame), fwd / inv [T][6] the fixed-point tables (the identity's for an untracked frame), tracked [T], and
    `translation`: every tracked frame's map is exactly plate_align's integer translation."""
    __slots__ = ("fits", "maps", "fwd", "inv", "tracked", "translation")

    def __init__(self, fits, maps, fwd, inv, tracked, translation):
        self.fits, self.maps, self.fwd, self.inv, self.tracked, self.translation = fits, maps, fwd, inv, tracked, translation


def on_border(bx, by, vx, vy, dx, dy, H, W, cfg, kbox=None):
    """Whether the winner (dx, dy) of block (bx, by), whose whole vector is (vx, vy) = d0 + (dx, dy), lies on the border of its candidate set:
    at the search range's edge (for search >= 1), or so that the block moved one pixel further up, down, left or right would leave the key's
    H x W plane or enter kbox, the half-open box (y0, x0, y1, x1) of the key's mask (every invalid pixel of the key lies inside it).  The
    cost's true minimum may lie beyond such a winner (a block at the frame's edge whose content has left the key is clamped there), so the fit
    does not take it."""
    B = cfg.block
    x0, y0 = bx * B + vx, by * B + vy
    if (cfg.search >= 1 and max(abs(dx), abs(dy)) == cfg.search) or x0 - 1 < 0 or y0 - 1 < 0 or x0 + B + 1 > W or y0 + B + 1 > H:
        return True
    if kbox is None or kbox[2] <= kbox[0] or kbox[3] <= kbox[1]:
        return False
    return x0 - 1 < kbox[3] and x0 + B + 1 > kbox[1] and y0 - 1 < kbox[2] and y0 + B + 1 > kbox[0]


def plan_segment(track, rec, cfg, H, W, boxes=None):
    """track [T][8] (vva_track's records: dx, dy, key, tracked, ...), rec [T][nby][nbx][4] (vvw_search's: dx, dy, used, cost) as nested
    sequences or arrays of integers, H x W the frame, boxes [T][4] the frames' mask boxes (hip.mask_bbox; None: no masks) -> Plan.  Frame 0 (its own key) is the identity; a tracked frame's map to the canvas is
    its key's map composed with its own fitted map to the key; keys come before their frames, so one pass in time order suffices.  The fit
    takes the used blocks whose winner is not on_border."""
    track, rec, boxes = (v.tolist() if hasattr(v, "tolist") else v for v in (track, rec, boxes))      # Python integers from here on
    T = len(track)
    fits, maps, fwd, inv, tracked = [], [], [], [], []
    translation = True
    for t in range(T):
        dx, dy, key, ok = (int(v) for v in track[t][:4])
        ok = ok == 1
        tracked.append(ok)
        fit = None
        m = None
        if ok:
            if 0 <= key < t and maps[key] is not None:
                d0 = (dx - int(track[key][0]), dy - int(track[key][1]))
                kbox = None if boxes is None else tuple(int(v) for v in boxes[key])
                vectors = [(bx, by, r[0], r[1]) for by, row in enumerate(rec[t]) for bx, r in enumerate(row) if r[2] == 1 and
                           not on_border(bx, by, d0[0] + r[0], d0[1] + r[1], r[0], r[1], H, W, cfg, kbox)]
                fit = fit_frame(vectors, d0, cfg)
                m = compose(maps[key], field_map(fit.field))
            else:                       # frame 0, or a record no tracker writes: the translation the record states
                m = ((Fraction(dx), Fraction(1), Fraction(0)), (Fraction(dy), Fraction(0), Fraction(1)))
            translation = translation and m == ((dx, 1, 0), (dy, 0, 1))
        fits.append(fit)
        maps.append(m)
        fwd.append(to_fixed(m if m is not None else IDENTITY))
        inv.append(to_fixed(invert(m) if m is not None else IDENTITY))
    return Plan(fits, maps, fwd, inv, tracked, translation)


def canvas_box(boxes, fwd, tracked, align=4):
    """The canvas of one segment: boxes [T,4] = half-open (y0, x0, y1, x1) per frame in frame coordinates, empty where y1 <= y0 or x1 <= x0
    (hip.mask_bbox), fwd [T][6] the forward tables -> the union of the tracked frames' forward-mapped box corners, grown by one pixel on every
    side (the rounding of a nearest-neighbour map), in canvas coordinates, x0 rounded down and x1 up to a multiple of `align`; None when no
    tracked frame has a mask pixel."""
    pts = []
    for b, tab, k in zip(boxes, fwd, tracked):
        y0, x0, y1, x1 = (int(v) for v in b)
        if k and y1 > y0 and x1 > x0:
            pts += [apply_fixed(tab, x, y) for x in (x0, x1 - 1) for y in (y0, y1 - 1)]
    if not pts:
        return None
    x0, x1 = min(p[0] for p in pts) - 1, max(p[0] for p in pts) + 2
    y0, y1 = min(p[1] for p in pts) - 1, max(p[1] for p in pts) + 2
    return y0, x0 - x0 % align, y1, -(-x1 // align) * align


def canvas_bytes(T, box):
    """Bytes of the canvas [T, ch, cw, 3] u8."""
    return T * (box[2] - box[0]) * (box[3] - box[1]) * 3
