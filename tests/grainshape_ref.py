"""Grain shape restated in numpy, independently of the product's host code (videovanish_amd/grainshape.py) and kernels
(csrc/vv_grainshape.hip), on top of tests/grainmatch_ref.py (selection, noise_response, noise, looked_up, composite): the pair sums, the fit
in Python numbers frame by frame, the shaped noise and the composite, with the exact integer rules of include/grainshape.h."""
import math
import os
import sys

import numpy as np
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grainmatch_ref as GR  # noqa: E402
import seamblend_ref as BR  # noqa: E402
import tonematch_ref as TR  # noqa: E402

from oracle import imageops_ref as I  # noqa: E402

IDENT = GR.IDENT
DEFAULTS = dict(max_a=0.5, dead=0.05, min_pairs=512, smooth=4, max_gain=6.0)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def P0(a):
    return 6.0 - 16.0 * a + 14.0 * a * a


def P1(a):
    return -4.0 + 14.0 * a - 12.0 * a * a


def r0(a):
    return 1.0 + 2.0 * a * a


def rho(a):
    return P1(a) / P0(a)


def a_of(r, max_a=0.5):
    """rho's inverse on [0, max_a] by bisection (rho rises on [0, 0.5]), clamped at both ends."""
    if r <= rho(0.0):
        return 0.0
    if r >= rho(max_a):
        return float(max_a)
    lo, hi = 0.0, float(max_a)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if rho(mid) < r:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


# ---- the statistic --------------------------------------------------------------------------------------------------------------------------
def sums(patch, orig, mask, offsets, lut, h, w, r, flat):
    """-> [T,30] int64 = [T][c][axis][pairs, Cx, Cy, Dx, Dy]: over the pairs (p, p + (1, 0)) (axis 0) and (p, p + (0, 1)) (axis 1) whose two
    pixels both count for c (grainmatch_ref.selection)."""
    out = np.zeros((len(patch), 3, 2, 5), np.int64)
    for t in range(len(patch)):
        oy, ox = (int(v) for v in offsets[t])
        x_full = np.zeros(orig[t].shape, np.uint8)
        x_full[oy:oy + h, ox:ox + w] = GR.looked_up(patch[t], lut[t], h, w)
        sel = GR.selection(x_full, mask[t], (oy, ox, h, w), r, flat)
        lx, ly = GR.noise_response(x_full), GR.noise_response(orig[t])
        for c in range(3):
            for axis, (p, q) in enumerate((((slice(None), slice(None, -1)), (slice(None), slice(1, None))),
                                           ((slice(None, -1), slice(None)), (slice(1, None), slice(None))))):
                both = sel[..., c][p] & sel[..., c][q]
                xp, xq, yp, yq = lx[..., c][p][both], lx[..., c][q][both], ly[..., c][p][both], ly[..., c][q][both]
                out[t, c, axis] = [both.sum(), (xp * xq).sum(), (yp * yq).sum(), (xp * xp + xq * xq).sum(), (yp * yp + yq * yq).sum()]
    return out.reshape(len(patch), 30)


# ---- the fit --------------------------------------------------------------------------------------------------------------------------------
def fit(shape_sums, grain_sums, mode="luma", max_a=0.5, dead=0.05, min_pairs=512, smooth=4, max_gain=6.0, grain_smooth=4, strength=1.0,
        max_sigma=12.0, min_count=256):
    """-> (rho [T,3,2], taps [T,3,2] int, k [T,3], sigma_pixel [T,3,4], clamped [T,3,2], dead [T,3,2], amp [T,3,256] u8), in Python integers
    and floats, frame by frame.  The level starts from grainmatch_ref.fit's white estimate at strength 1 without a cap."""
    T = len(shape_sums)
    rows = [[int(v) for v in row] for row in np.asarray(shape_sums).reshape(T, 30)]
    white = GR.fit(grain_sums, smooth=grain_smooth, strength=1.0, max_sigma=float("inf"), min_count=min_count)[2]
    rh, taps, ks = np.zeros((T, 3, 2)), np.zeros((T, 3, 2), np.int64), np.ones((T, 3))
    clamped, deadz = np.zeros((T, 3, 2), bool), np.zeros((T, 3, 2), bool)
    sp, sw = np.zeros((T, 3, 4)), np.zeros((T, 3, 4))
    for t in range(T):
        p = [sum(rows[u][k] for u in range(max(0, t - smooth), min(T, t + smooth + 1))) for k in range(30)]
        for c in range(3):
            for axis in range(2):
                chans = range(3) if mode == "luma" else (c,)
                n, cx, cy, dx, dy = (sum(p[(ch * 2 + axis) * 5 + k] for ch in chans) for k in range(5))
                if n < min_pairs or dy - dx <= 0:
                    continue
                r = rh[t, c, axis] = 2 * (cy - cx) / (dy - dx)
                a = a_of(r, 0.5)
                clamped[t, c, axis] = r < -2.0 / 3.0 or r > 0.0 or a > max_a
                a = min(a, max_a)
                deadz[t, c, axis] = a < dead
                taps[t, c, axis] = 0 if a < dead else int(np.rint(256.0 * a))
            ax, ay = taps[t, c, 0] / 256.0, taps[t, c, 1] / 256.0
            shape_var = r0(ax) * r0(ay)
            ks[t, c] = min(math.sqrt(36.0 * shape_var / (P0(ax) * P0(ay))), max_gain)
            for b in range(4):
                sp[t, c, b] = min(strength * ks[t, c] * white[t, c, b], max_sigma)
                sw[t, c, b] = sp[t, c, b] / math.sqrt(shape_var)
    return rh, taps, ks, sp, clamped, deadz, GR.tables(sw)


# ---- the noise and the composite ----------------------------------------------------------------------------------------------------------------
def field(seed, frame_id, H, W, mode):
    """s [H + 2, W + 2, 3] int64: the white field of include/vvgrain.h at the frame's pixels and one pixel beyond on every side, element (j, i) =
    frame pixel (i - 1, j - 1); the key from signed coordinates, modulo 2^64."""
    u = np.uint64
    yy, xx = (v.astype(np.int64).astype(np.uint64) for v in np.mgrid[-1:H + 1, -1:W + 1])
    with np.errstate(over="ignore"):
        key = (u(seed) << u(32)) ^ ((u(frame_id) * u(H) + yy) * u(W) + xx)
        keys = [key, key, key] if mode == "luma" else [key * u(3) + u(c) for c in range(3)]
        out = []
        for z in keys:
            z = z + u(0x9E3779B97F4A7C15)
            z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
            z = z ^ (z >> u(31))
            out.append(sum(((z >> u(8 * k)) & u(255)).astype(np.int64) for k in range(8)) - 1020)
    return np.stack(out, axis=-1)


def shaped(seed, frame_id, H, W, mode, taps_t):
    """u [H,W,3] int64: (sum_j wy_j sum_i wx_i s(X + i, Y + j) + 2^15) >> 16, w = [aq, 256, aq], taps_t [3,2] = aq per channel and axis."""
    s = field(seed, frame_id, H, W, mode)
    out = np.zeros((H, W, 3), np.int64)
    for c in range(3):
        wx, wy = ([int(taps_t[c][k]), 256, int(taps_t[c][k])] for k in range(2))
        acc = np.zeros((H, W), np.int64)
        for j in range(3):
            for i in range(3):
                acc += wy[j] * wx[i] * s[j:j + H, i:i + W, c]
        out[..., c] = (acc + (1 << 15)) >> 16
    return out


def composite(patch, orig, mask, offsets, lut, membrane, q8, amp, taps, frame_ids, seed, mode, h, w, feather):
    """The fused paste: resize, look up, add the membrane (membrane [T,h,w,3] int16 or None), add the shaped grain of the pixel's frame position
    at the tabled value's amplitude with a 64-bit product, clip, paste at the offset, feathered composite (feather < 0: the paste)."""
    out = np.empty_like(orig)
    H, W = orig.shape[1:3]
    for t in range(len(patch)):
        oy, ox = (int(v) for v in offsets[t])
        x = GR.looked_up(patch[t], lut[t], h, w)
        u = shaped(seed, int(frame_ids[t]), H, W, mode, taps[t])[oy:oy + h, ox:ox + w]
        a = np.stack([amp[t][c][x[..., c]] for c in range(3)], axis=-1).astype(np.int64)
        d = (a * u * 5017 + (1 << 23)) >> 24
        v = x if membrane is None else BR.membrane(x, membrane[t], q8)
        x = np.clip(v.astype(np.int64) + d, 0, 255).astype(np.uint8)
        pasted = orig[t].copy()
        pasted[oy:oy + h, ox:ox + w] = x
        out[t] = pasted if feather < 0 else I.composite(pasted, orig[t], I.feather_alpha(mask[t], feather))
    return out


def apply(patch, orig, mask, offsets, h, w, feather, frame_ids=None, tone=None, blend=None, mode="luma", ring=12, flat=24, seed=0, grain=None,
          **cfg):
    """The whole stage for one window: (composite, shape sums, grain sums, fit).  grain = the fit keywords of grain matching (smooth, strength,
    max_sigma, min_count), cfg = the shape's; tone = the keywords of tonematch_ref.fit (with ring); blend = dict(strength=, **seamblend_ref
    settings): the membrane runs in between, and in front of it tone fits the offset alone."""
    T = len(patch)
    frame_ids = list(range(T)) if frame_ids is None else frame_ids
    lut = np.broadcast_to(IDENT, (T, 3, 256))
    if tone is not None:
        tone = dict(tone)
        ts = TR.sums(patch, orig, mask, offsets, h, w, tone.pop("ring", 12))
        lut = TR.tables(*TR.fit(ts, **(dict(tone, mode="offset") if blend is not None else tone)))
    g = dict(grain or {})
    gs = GR.sums(patch, orig, mask, offsets, lut, h, w, ring, flat)
    ss = sums(patch, orig, mask, offsets, lut, h, w, ring, flat)
    f = fit(ss, gs, mode=mode, grain_smooth=g.get("smooth", 4), strength=g.get("strength", 1.0), max_sigma=g.get("max_sigma", 12.0),
            min_count=g.get("min_count", 256), **dict(DEFAULTS, **cfg))
    membrane, q8 = None, 0
    if blend is not None:
        blend = dict(blend)
        q8 = BR.strength_q8(blend.pop("strength", 1.0))
        membrane = BR.solve(patch, orig, mask, offsets, lut, h, w, **dict(BR.DEFAULTS, **blend))[0]
    return composite(patch, orig, mask, offsets, lut, membrane, q8, f[6], f[1], frame_ids, seed, mode, h, w, feather), ss, gs, f


# ---- stand-ins of the device entry points on CPU tensors (tests/test_grainshape_cpu.py) -----------------------------------------------------
def hip_ring_shape_stats(patch, orig, mask, offs, lut, h, w, ring, flat):
    import torch
    n = lambda t: t.numpy()
    return torch.from_numpy(sums(n(patch), n(orig), n(mask), n(offs), n(lut), h, w, ring, flat))


def hip_paste_shaped_composite(patch, orig, mask, offs, lut, membrane, q8, amp, taps, ids, seed, mode, h, w, feather, out=None):
    import torch
    n = lambda t: t.numpy()
    res = composite(n(patch), n(orig), n(mask), n(offs), n(lut), None if membrane is None else n(membrane), q8, n(amp), n(taps), n(ids), seed,
                    ("luma", "rgb")[mode], h, w, feather)
    out.copy_(torch.from_numpy(np.ascontiguousarray(res)))
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
RECOVERY_SHAPES = ((0.0, 0.0), (0.25, 0.25), (0.5, 0.5), (0.5, 0.0))      # (a_x, a_y)
RECOVERY_SIGMAS = GR.RECOVERY_SIGMAS
RECOVERY_SEEDS = GR.RECOVERY_SEEDS
RECOVERY_T = 1      # frames per recovery clip: grainmatch_ref.recovery_clip's ring at T = 1 pools 5358 pairs per axis over the three channels, ten times min_pairs


def shape_noise(rng, sigma, shape, ax, ay):
    """Gaussian noise of PIXEL sigma `sigma` shaped by [ax, 1, ax] along x and [ay, 1, ay] along y (white noise of sigma / sqrt(r0x r0y) in
    front of the kernel), [H,W,3]."""
    g = rng.normal(0.0, float(sigma) / math.sqrt(r0(ax) * r0(ay)), shape)
    g = ndimage.correlate1d(g, [ax, 1.0, ax], axis=1, mode="wrap")
    return ndimage.correlate1d(g, [ay, 1.0, ay], axis=0, mode="wrap")


def recovery_clip(s, sigma, ax, ay, T=RECOVERY_T):
    """(orig, x, mask) [T,96,130,...]: x = grainmatch_ref.recovery_clip(s, 0)'s smooth frame T times, as the model's frames; orig = x plus
    seeded shaped Gaussian noise of pixel sigma `sigma`, fresh per frame, rounded and clipped."""
    _, smooth, mask = GR.recovery_clip(s, 0)
    smooth, mask = np.repeat(smooth, T, axis=0), np.repeat(mask, T, axis=0)
    rng = np.random.default_rng(104729 * s + 31 * sigma + int(round(64 * ax)) * 7 + int(round(64 * ay)))
    g = np.stack([shape_noise(rng, sigma, smooth.shape[1:], ax, ay) for _ in range(T)])
    return np.clip(np.rint(smooth.astype(np.float64) + g), 0, 255).astype(np.uint8), smooth, mask


def inside_estimate(out_t, x_t, mask_t):
    """The shaped estimator on the pixels at least four deep in the mask (the analogue of grainmatch_ref.inside_estimate): per channel the pixel
    sigma of what the composite out_t carries over the model's frame x_t there, from the variance and the lag-1 covariances of L along x and
    y: a per axis from rho = 2 C / D over the core's pairs, then sqrt(var r0x r0y / (P0x P0y))."""
    core = ndimage.binary_erosion(mask_t > 0, structure=np.ones((9, 9), bool), border_value=0)
    lo, lx = GR.noise_response(out_t), GR.noise_response(x_t)
    est = np.zeros(3)
    for c in range(3):
        a = []
        for p, q in (((slice(None), slice(None, -1)), (slice(None), slice(1, None))), ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):
            both = core[p] & core[q]
            cy, cx = (lo[..., c][p][both] * lo[..., c][q][both]).sum(), (lx[..., c][p][both] * lx[..., c][q][both]).sum()
            dy = (lo[..., c][p][both] ** 2 + lo[..., c][q][both] ** 2).sum()
            dx = (lx[..., c][p][both] ** 2 + lx[..., c][q][both] ** 2).sum()
            a.append(a_of(2.0 * (cy - cx) / max(dy - dx, 1)))
        var = max((lo[..., c][core] ** 2).sum() - (lx[..., c][core] ** 2).sum(), 0) / float(core.sum())
        est[c] = math.sqrt(var * r0(a[0]) * r0(a[1]) / (P0(a[0]) * P0(a[1])))
    return est


# The deviations of this restatement with the default settings (luma, ring 12, flat 24, min_count 256, min_pairs 512, dead 0.05, smooth 4, strength
# 1, max_sigma 12) over recovery_clip(s, sigma, ax, ay), s = 0 .. 11, T = 1 (5358 pooled pairs per axis, ten times min_pairs), measured by
# tests/test_grainshape_cpu.py::test_reference_recovers_shape_and_level (which prints them).  Per (ax, ay) and sigma: "a" = the worst |a_fit - a|
# over seeds and axes, "sigma" = the worst |sigma_pixel / sigma - 1| over seeds, channels and bands, "white" / "white_least" = the worst and the
# smallest of the same of grain matching's own sigma_added (what the stage adds without the option; on shaped grain its shortfall), "inside" = the
# worst |inside_estimate / sigma - 1| of the composite at feather 3 over seeds and channels (::test_reference_adds_the_level_inside_the_mask).  The tests
# assert 1.5 times "a", "sigma", "inside" and "white", and a shortfall of at least "white_least" / 1.5 (DESIGN.md section 14's convention: the margin covers
# the seed-to-seed scatter of a statistic over a few thousand pixels).  On white grain the dead zone gives a = 0 for all 36 clips (the largest
# fitted a before it is 0.031).  At (0.5, 0.5) and sigma 2 the fit reads a = 0.33 .. 0.36: the rounding to bytes adds white noise of sigma 0.29,
# which is most of what the top octave of so soft and weak a grain holds.
MEASURED_DEVIATION = {
    (0.0, 0.0): {
        2: {"a": 0.0, "sigma": 0.1636, "white": 0.1636, "white_least": 0.0009, "inside": 0.182},
        4: {"a": 0.0, "sigma": 0.1413, "white": 0.1413, "white_least": 0.0002, "inside": 0.1068},
        8: {"a": 0.0, "sigma": 0.2028, "white": 0.2028, "white_least": 0.0002, "inside": 0.1317},
    },
    (0.25, 0.25): {
        2: {"a": 0.0313, "sigma": 0.1232, "white": 0.5988, "white_least": 0.4841, "inside": 0.1271},
        4: {"a": 0.0157, "sigma": 0.0902, "white": 0.6029, "white_least": 0.5214, "inside": 0.0867},
        8: {"a": 0.0157, "sigma": 0.1261, "white": 0.6056, "white_least": 0.5211, "inside": 0.0805},
    },
    (0.5, 0.5): {
        2: {"a": 0.1719, "sigma": 0.433, "white": 0.8273, "white_least": 0.758, "inside": 0.4122},
        4: {"a": 0.0743, "sigma": 0.2302, "white": 0.8441, "white_least": 0.7904, "inside": 0.2133},
        8: {"a": 0.0391, "sigma": 0.1704, "white": 0.8503, "white_least": 0.8084, "inside": 0.1243},
    },
    (0.5, 0.0): {
        2: {"a": 0.0547, "sigma": 0.1671, "white": 0.6375, "white_least": 0.5154, "inside": 0.1088},
        4: {"a": 0.0235, "sigma": 0.1339, "white": 0.6365, "white_least": 0.5269, "inside": 0.0812},
        8: {"a": 0.0157, "sigma": 0.1888, "white": 0.6653, "white_least": 0.5426, "inside": 0.078},
    },
}
