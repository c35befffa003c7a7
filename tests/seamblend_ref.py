"""Seam membrane blending restated in numpy / scipy from include/vvblend.h, independently of the product's host code
(videovanish_amd/seamblend.py) and kernels (csrc/vv_blend.hip): the ring, the presmoothed boundary values, the classes, the pull, the cascadic
push, the paste and the report sums; and a direct fp64 sparse solve of the same Dirichlet problem to hold the cascade against.  The ring, the
resize and the feathered composite are those of tests/tonematch_ref.py and oracle/imageops_ref.py, the grain that of tests/grainmatch_ref.py."""
import os
import sys

import numpy as np
from scipy import ndimage, sparse
from scipy.sparse.linalg import spsolve

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grainmatch_ref as GR  # noqa: E402
import tonematch_ref as TR  # noqa: E402

from oracle import imageops_ref as I  # noqa: E402

INACTIVE, KNOWN, UNKNOWN = 0, 1, 2
Q = 64
IDENT = GR.IDENT
DEFAULTS = dict(ring=12, presmooth=2, sweeps=8, max_shift=32)


def rdiv(s, n):
    """(2 s + n) // (2 n) on integer arrays, n > 0: the floor division."""
    return (2 * s + n) // (2 * n)


def classes(mask, win, r):
    """mask [H,W] u8, win = (oy, ox, h, w) -> cls [h,w] u8 of the window's cells (the window may hang over the frame: inactive there)."""
    oy, ox, h, w = win
    H, W = mask.shape
    full = np.zeros((H, W), np.uint8)
    inside = np.zeros((H, W), bool)
    inside[max(oy, 0):max(oy + h, 0), max(ox, 0):max(ox + w, 0)] = True
    full[(mask > 0) & inside] = UNKNOWN
    full[TR.ring(mask, win, r)] = KNOWN
    out = np.zeros((h, w), np.uint8)
    y0, x0, y1, x1 = max(oy, 0), max(ox, 0), min(oy + h, H), min(ox + w, W)
    if y1 > y0 and x1 > x0:
        out[y0 - oy:y1 - oy, x0 - ox:x1 - ox] = full[y0:y1, x0:x1]
    return out


def boundary(x_win, y_win, cls, presmooth, max_shift):
    """x_win, y_win [h,w,3] u8 (the tabled model pixels and the original ones of the window), cls [h,w] -> (val [h,w,3] int64 Q6: on the known
    cells the clamped rounded mean of d = y - x over the known cells within `presmooth` pixels (a box, clipped to the window), 0 elsewhere;
    d [h,w,3] int64: y - x on the known cells, 0 elsewhere)."""
    k = cls == KNOWN
    d = np.where(k[..., None], y_win.astype(np.int64) - x_win.astype(np.int64), 0)
    box = np.ones((2 * presmooth + 1, 2 * presmooth + 1), np.int64)
    n = ndimage.correlate(k.astype(np.int64), box, mode="constant", cval=0)
    s = ndimage.correlate(d, box[:, :, None], mode="constant", cval=0)
    v = np.clip(rdiv(Q * s, np.maximum(n, 1)[..., None]), -Q * max_shift, Q * max_shift)
    return np.where(k[..., None], v, 0), d


def pull(cls, val):
    """One level up: cls [h,w], val [h,w,3] -> the same of the ceil-halved grid."""
    h, w = cls.shape
    hu, wu = (h + 1) // 2, (w + 1) // 2
    c = np.zeros((2 * hu, 2 * wu), np.uint8)
    c[:h, :w] = cls
    v = np.zeros((2 * hu, 2 * wu, 3), np.int64)
    v[:h, :w] = val
    c4 = c.reshape(hu, 2, wu, 2)
    known = c4 == KNOWN
    n = known.sum(axis=(1, 3))
    s = (v.reshape(hu, 2, wu, 2, 3) * known[..., None]).sum(axis=(1, 3))
    up = np.where(n > 0, KNOWN, np.where((c4 == UNKNOWN).any(axis=(1, 3)), UNKNOWN, INACTIVE)).astype(np.uint8)
    return up, np.where((n > 0)[..., None], rdiv(s, np.maximum(n, 1)[..., None]), 0)


def sweep(cls, val):
    """One Jacobi sweep: every unknown cell <- (N + S + W + E + 2) >> 2 of the values before; a neighbour outside the grid or inactive is the
    cell itself."""
    act = np.pad(cls != INACTIVE, 1, constant_values=False)
    v = np.pad(val, ((1, 1), (1, 1), (0, 0)))
    total = np.zeros_like(val)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        a = act[1 + dy:act.shape[0] - 1 + dy, 1 + dx:act.shape[1] - 1 + dx]
        total += np.where(a[..., None], v[1 + dy:v.shape[0] - 1 + dy, 1 + dx:v.shape[1] - 1 + dx], val)
    return np.where((cls == UNKNOWN)[..., None], (total + 2) >> 2, val)


def relax(cls, val, sweeps, parent=None, start=True):
    """The unknown cells start from their parent (None: 0) when start, else from val; then `sweeps` sweeps."""
    if start:
        h, w = cls.shape
        init = np.zeros_like(val) if parent is None else parent[np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1]
        val = np.where((cls == UNKNOWN)[..., None], init, val)
    for _ in range(sweeps):
        val = sweep(cls, val)
    return val


def solve_levels(cls, val, sweeps):
    """The cascade of one frame: -> the field [h,w,3] int64 (Q6)."""
    levels = [(cls, val)]
    while max(levels[-1][0].shape) > 2:
        levels.append(pull(*levels[-1]))
    parent = None
    for c, v in reversed(levels):
        parent = relax(c, v, sweeps, parent)
    return parent


def window_pair(patch_t, orig_t, lut_t, win):
    """(x, y) [h,w,3] u8 of one frame's window: the tabled model pixels, and the original ones (0 where the window hangs over the frame)."""
    oy, ox, h, w = win
    H, W = orig_t.shape[:2]
    x = GR.looked_up(patch_t, lut_t, h, w)
    y = np.zeros((h, w, 3), np.uint8)
    y0, x0, y1, x1 = max(oy, 0), max(ox, 0), min(oy + h, H), min(ox + w, W)
    if y1 > y0 and x1 > x0:
        y[y0 - oy:y1 - oy, x0 - ox:x1 - ox] = orig_t[y0:y1, x0:x1]
    return x, y


def level0(patch, orig, mask, offsets, lut, h, w, ring=12, presmooth=2, max_shift=32):
    """-> (cls [T,h,w] u8, val [T,h,w,3] int16, sums [T,11] int64 with entries 0 .. 3): what vvb_ring_diff writes."""
    T = len(patch)
    cls, val, sums = np.zeros((T, h, w), np.uint8), np.zeros((T, h, w, 3), np.int16), np.zeros((T, 11), np.int64)
    for t in range(T):
        win = (int(offsets[t][0]), int(offsets[t][1]), h, w)
        cls[t] = classes(mask[t], win, ring)
        x, y = window_pair(patch[t], orig[t], lut[t], win)
        v, d = boundary(x, y, cls[t], presmooth, max_shift)
        val[t] = v
        sums[t, 0] = (cls[t] == KNOWN).sum()
        sums[t, 1:4] = (d * d).sum(axis=(0, 1))
    return cls, val, sums


def field_sums(cls, field, sums):
    """Entries 4 .. 10 from the unknown cells of the field [T,h,w,3]."""
    for t in range(len(cls)):
        m = np.abs(field[t].astype(np.int64))[cls[t] == UNKNOWN]
        sums[t, 4] = len(m)
        if len(m):
            sums[t, 5:8], sums[t, 8:11] = m.sum(axis=0), m.max(axis=0)
    return sums


def solve(patch, orig, mask, offsets, lut, h, w, ring=12, presmooth=2, sweeps=8, max_shift=32):
    """-> (field [T,h,w,3] int16, cls [T,h,w] u8, sums [T,11] int64): what vvb_solve leaves."""
    cls, val, sums = level0(patch, orig, mask, offsets, lut, h, w, ring, presmooth, max_shift)
    field = np.stack([solve_levels(cls[t], val[t].astype(np.int64), sweeps) for t in range(len(cls))]).astype(np.int16)
    return field, cls, field_sums(cls, field, sums)


def report(sums):
    """(n, rms_diff [T,3], n_hole, max_shift [T,3], mean_shift [T,3]) in Python numbers, frame by frame."""
    T = len(sums)
    n, nh = [int(v) for v in sums[:, 0]], [int(v) for v in sums[:, 4]]
    rms, mx, mean = np.zeros((T, 3)), np.zeros((T, 3)), np.zeros((T, 3))
    for t in range(T):
        for c in range(3):
            rms[t, c] = (int(sums[t, 1 + c]) / max(n[t], 1)) ** 0.5
            mx[t, c] = int(sums[t, 8 + c]) / 64.0
            mean[t, c] = int(sums[t, 5 + c]) / (64.0 * max(nh[t], 1))
    return np.array(n, np.int64), rms, np.array(nh, np.int64), mx, mean


def strength_q8(strength):
    return int(round(strength * 256.0))


def membrane(img, field_t, q8):
    """img [h,w,3] u8 (tabled) -> clip(img + ((m q8 + 2^13) >> 14))."""
    return np.clip(img.astype(np.int64) + ((field_t.astype(np.int64) * q8 + (1 << 13)) >> 14), 0, 255).astype(np.uint8)


def composite(patch, orig, mask, offsets, lut, field, q8, amp, frame_ids, seed, mode, h, w, feather):
    """The fused paste: resize, look up, add the membrane, add the grain of the pixel's frame position at the tabled value's amplitude, paste at
    the offset, feathered composite with the full-frame mask (feather < 0: the paste)."""
    out = np.empty_like(orig)
    H, W = orig.shape[1:3]
    for t in range(len(patch)):
        oy, ox = (int(v) for v in offsets[t])
        x = GR.looked_up(patch[t], lut[t], h, w)
        s = GR.noise(seed, int(frame_ids[t]), H, W, mode)[oy:oy + h, ox:ox + w]
        _, g = GR.grain(x, amp[t], s)
        x = np.clip(membrane(x, field[t], q8).astype(np.int64) + g, 0, 255).astype(np.uint8)
        pasted = orig[t].copy()
        pasted[oy:oy + h, ox:ox + w] = x
        out[t] = pasted if feather < 0 else I.composite(pasted, orig[t], I.feather_alpha(mask[t], feather))
    return out


def apply(patch, orig, mask, offsets, h, w, feather, frame_ids=None, tone=None, grain=None, strength=1.0, **cfg):
    """The whole stage for one window: (composite, field, cls, sums); tone / grain = the keywords of tonematch_ref.fit / grainmatch_ref.apply's
    fit (with ring, and for grain flat, mode, seed) when those stages run with it.  In front of the membrane the tone stage fits the offset alone
    (DESIGN.md section 15), whatever mode the keywords name."""
    T = len(patch)
    frame_ids = list(range(T)) if frame_ids is None else frame_ids
    lut = np.broadcast_to(IDENT, (T, 3, 256))
    if tone is not None:
        tone = dict(tone)
        ts = TR.sums(patch, orig, mask, offsets, h, w, tone.pop("ring", 12))
        lut = TR.tables(*TR.fit(ts, **dict(tone, mode="offset")))
    amp, seed, mode = np.zeros((T, 3, 256), np.uint8), 0, "luma"
    if grain is not None:
        grain = dict(grain)
        seed, mode = grain.pop("seed", 0), grain.pop("mode", "luma")
        gs = GR.sums(patch, orig, mask, offsets, lut, h, w, grain.pop("ring", 12), grain.pop("flat", 24))
        amp = GR.tables(GR.fit(gs, **grain)[2])
    field, cls, sums = solve(patch, orig, mask, offsets, lut, h, w, **dict(DEFAULTS, **cfg))
    return composite(patch, orig, mask, offsets, lut, field, strength_q8(strength), amp, frame_ids, seed, mode, h, w, feather), field, cls, sums


# ---- the direct solve ----------------------------------------------------------------------------------------------------------------------
def direct_solve(cls, val):
    """The same Dirichlet problem in fp64: on the unknown cells the five-point Laplace equation, a neighbour outside the grid or inactive
    replaced by the cell itself, the known cells' values val [h,w,3] (levels) as they are; an unknown region that touches no known cell gets 0.
    -> [h,w,3] float64."""
    h, w = cls.shape
    unk = cls == UNKNOWN
    idx = -np.ones((h, w), np.int64)
    idx[unk] = np.arange(unk.sum())
    n = int(unk.sum())
    out = np.where((cls == KNOWN)[..., None], val, 0.0).astype(np.float64)
    if n == 0:
        return out
    ys, xs = np.nonzero(unk)
    rows, cols, data = [], [], []
    diag = np.zeros(n)
    rhs = np.zeros((n, 3))
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        y, x = ys + dy, xs + dx
        ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
        c = np.where(ok, cls[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], INACTIVE)
        diag += c != INACTIVE
        u = c == UNKNOWN
        rows.append(idx[ys[u], xs[u]]); cols.append(idx[y[u], x[u]]); data.append(-np.ones(u.sum()))
        k = c == KNOWN
        rhs[idx[ys[k], xs[k]]] += out[y[k], x[k]]
    # a component without a known neighbour is singular: pin it to 0 with a small diagonal term (its solution is then exactly 0)
    A = sparse.csr_matrix((np.concatenate(data), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)) + sparse.diags(diag + 1e-9)
    sol = spsolve(A.tocsc(), rhs)
    out[unk] = np.asarray(sol).reshape(n, 3)
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def box_mask(H=96, W=130, box=(30, 50), at=(33, 40)):
    m = np.zeros((H, W), np.uint8)
    m[at[0]:at[0] + box[0], at[1]:at[1] + box[1]] = 255
    return m


def ellipse_with_hole(H=300, W=400, axes=(75, 125), hole=(20, 30)):
    """An elliptical mask of 2 axes[1] x 2 axes[0] pixels round the centre with an elliptical hole in it."""
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    cy, cx = H / 2, W / 2
    e = lambda a: ((yy - cy) / a[0]) ** 2 + ((xx - cx) / a[1]) ** 2
    return (((e(axes) <= 1) & (e(hole) > 1)) * 255).astype(np.uint8)


def two_components(H=96, W=130):
    m = np.zeros((H, W), np.uint8)
    m[20:50, 15:45] = 255
    yy, xx = np.mgrid[:H, :W]
    m[(yy - 60) ** 2 + (xx - 95) ** 2 <= 18 ** 2] = 255
    return m


MASKS = {"box": box_mask, "ellipse": ellipse_with_hole, "two": two_components}


def shift_field(kind, H, W):
    """[H,W,3] float64: "ramp": a linear ramp per channel (harmonic: the direct solve restores it exactly); "vignette": the ramp plus a
    quadratic vignette (not harmonic)."""
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    u, v = yy / (H - 1) - 0.5, xx / (W - 1) - 0.5
    out = np.stack([12 * u + 8 * v + 3, -10 * u + 14 * v - 2, 6 * u - 16 * v + 1], axis=-1)
    if kind == "vignette":
        out = out + np.stack([-24 * (u * u + v * v), 18 * (u * u + v * v), -12 * (u * u - v * v)], axis=-1)
    return out


def case(mask_name, kind, sigma, seed=0):
    """(orig, x, mask, shift) of one frame: orig = a smooth texture (with Gaussian grain of `sigma` when sigma > 0), x = clip(rint(smooth -
    shift)): the model's rendering is the smooth frame with the tone error -shift, so y - x is the shift (plus the grain)."""
    mask = MASKS[mask_name]()
    H, W = mask.shape
    smooth = TR.smooth_texture(seed, H, W, lo=60, hi=190).astype(np.float64)
    shift = shift_field(kind, H, W)
    g = np.random.default_rng(101 * seed + sigma).normal(0.0, float(sigma), smooth.shape) if sigma else 0.0
    orig = np.clip(np.rint(smooth + g), 0, 255).astype(np.uint8)
    x = np.clip(np.rint(smooth - shift), 0, 255).astype(np.uint8)
    return orig, x, mask, shift


CASES = [(m, k, s) for m in ("box", "ellipse", "two") for k in ("ramp", "vignette") for s in (0, 4)]

# The worst deviation, in 8-bit levels, of this restatement's field (defaults: ring 12, presmooth 2, sweeps 8, max_shift 32) from direct_solve of
# the same boundary values over the unknown cells and the three channels, per case of CASES, measured by
# tests/test_seamblend_cpu.py::test_cascade_against_the_direct_solve (which prints them).  The tests assert 1.5 times these.
MEASURED_DEVIATION = {
    ("box", "ramp", 0): 0.1997,
    ("box", "ramp", 4): 0.3631,
    ("box", "vignette", 0): 0.2080,
    ("box", "vignette", 4): 0.3685,
    ("ellipse", "ramp", 0): 0.2954,
    ("ellipse", "ramp", 4): 0.6614,
    ("ellipse", "vignette", 0): 0.2513,
    ("ellipse", "vignette", 4): 0.7169,
    ("two", "ramp", 0): 0.1904,
    ("two", "ramp", 4): 0.5139,
    ("two", "vignette", 0): 0.2132,
    ("two", "vignette", 4): 0.4808,
}
