"""Helpers of the mask clean-up tests: the numpy / scipy restatement of csrc/vv_mask.hip and infill.clean_masks, and the
clips the tests share.  No test in here."""
import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3), int)


def labels(mask2d):
    """mask2d [S,H,W] -> int32 [S,H,W]: the smallest linear index y * W + x of the pixel's 8-connected component within its frame, -1 on zeros."""
    mask2d = np.asarray(mask2d)
    S, H, W = mask2d.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    out = np.full((S, H, W), -1, np.int32)
    for t in range(S):
        lab, n = ndimage.label(mask2d[t] > 0, structure=EIGHT)
        if n:
            low = np.asarray(ndimage.minimum(idx, lab, np.arange(1, n + 1))).astype(np.int64)
            out[t][lab > 0] = low[lab[lab > 0] - 1]
    return out


def despeckle(dil, raw, min_area):
    """dil [S,H,W] u8, raw [S,H,W,ch] (or [S,H,W]) u8 -> (out [S,H,W] u8, counts [S,2] int64 = components removed, pixels cleared): the components
    of dil > 0 holding fewer than min_area raw pixels (any channel > 0) are cleared; min_area <= 1 clears nothing."""
    dil, raw = np.asarray(dil), np.asarray(raw)
    out, counts = dil.copy(), np.zeros((len(dil), 2), np.int64)
    if min_area <= 1:
        return out, counts
    for t in range(len(dil)):
        b = bbox(dil[t])
        if b is None:
            continue
        win = (t, slice(b[0], b[2]), slice(b[1], b[3]))          # the components lie inside the frame's box: label there
        any_raw = raw[win] > 0 if raw.ndim == 3 else (raw[win] > 0).any(axis=-1)
        lab, n = ndimage.label(dil[win] > 0, structure=EIGHT)
        weight = np.asarray(ndimage.sum(any_raw, lab, np.arange(1, n + 1))).astype(np.int64)
        light = np.nonzero(weight < min_area)[0] + 1
        kill = np.isin(lab, light)
        out[win][kill] = 0
        counts[t] = len(light), kill.sum()
    return out, counts


def bridge(x, g):
    """x [T,...] bool -> bool: per pixel along axis 0, every run of at most g False frames with a True frame on both sides becomes True (a
    per-pixel run fill: for every frame the nearest True frame before and after it, over the pixels that are ever True)."""
    x = np.asarray(x, bool)
    T = x.shape[0]
    flat = x.reshape(T, -1)
    live = flat.any(axis=0)
    col = flat[:, live]
    t = np.arange(T)[:, None]
    before = np.maximum.accumulate(np.where(col, t, -1), axis=0)                     # -1: none yet
    after = np.minimum.accumulate(np.where(col, t, 2 * T)[::-1], axis=0)[::-1]       # 2 T: none to come
    fill = ~col & (before >= 0) & (after < T) & (after - before - 1 <= g)
    out = flat.copy()
    out[:, live] = col | fill
    return out.reshape(x.shape)


def grow(x, k):
    """out[t] = OR x[t - k .. t + k], clamped to the clip (shifted ORs)."""
    x = np.asarray(x, bool)
    out = x.copy()
    for j in range(1, k + 1):
        out[j:] |= x[:-j]
        out[:-j] |= x[j:]
    return out


def segments(T, cuts):
    edges = [0] + sorted({int(c) for c in (cuts or ()) if 0 < int(c) < T}) + [T]
    return [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]


def time_clean(x, g, k, cuts=None):
    """Bridge then grow inside every segment -> (out [T,H,W] u8 {0, 255}, counts [T,2] int64 = pixels bridged, pixels grown per frame).  Only the
    pixels that are ever set are worked on: the others stay zero under both steps."""
    x = np.asarray(x)
    T = len(x)
    flat = x.reshape(T, -1)
    live = np.nonzero(flat.any(axis=0))[0]
    col = flat[:, live] > 0
    res, counts = np.zeros(col.shape, bool), np.zeros((T, 2), np.int64)
    for s, e in segments(T, cuts):
        b = bridge(col[s:e], g)
        res[s:e] = grow(b, k)
        counts[s:e, 0] = (b & ~col[s:e]).sum(1)
        counts[s:e, 1] = (res[s:e] & ~b).sum(1)
    out = np.zeros(flat.shape, np.uint8)
    out[:, live] = res * np.uint8(255)
    return out.reshape(x.shape), counts


def clean(dil, raw, min_area, g, k, cuts=None):
    """The whole stage -> (out [T,H,W] u8, counts [T,4] int64 = components removed, pixels cleared, bridged, grown)."""
    d, c1 = despeckle(dil, raw, min_area)
    o, c2 = time_clean(d, g, k, cuts)
    return o, np.concatenate([c1, c2], axis=1)


def dilate(raw, iters):
    """The dilation of hip.mask_collapse_dilate restated for iters >= 1: collapse the channels (any > 0), then `iters` steps of the 3 x 3 cross,
    {0, 255}."""
    assert iters >= 1
    raw = np.asarray(raw)
    m = raw > 0 if raw.ndim == 3 else (raw > 0).any(axis=-1)
    m = np.stack([ndimage.binary_dilation(f, structure=ndimage.generate_binary_structure(2, 1), iterations=iters) for f in m])
    return m.astype(np.uint8) * 255


def serpentine(H, W):
    """One winding path: full rows at even y joined by one pixel at alternating ends of the odd rows."""
    m = np.zeros((H, W), np.uint8)
    m[0::2] = 1
    for y in range(1, H, 2):
        m[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    return m


def bbox(f):
    """Half-open (y0, x0, y1, x1) of the non-zero pixels of one frame, None when there is none."""
    ys, xs = np.nonzero(f.any(axis=1))[0], np.nonzero(f.any(axis=0))[0]
    return None if len(ys) == 0 else (int(ys[0]), int(xs[0]), int(ys[-1]) + 1, int(xs[-1]) + 1)


def logo_clip(T=96, H=1080, W=1920, box=(90, 160), frames=(28, 52)):
    """The planner table of the issue: boolean raw masks [T,H,W] with a box[0] x box[1] logo in frames[0] .. frames[1] - 1."""
    m = np.zeros((T, H, W), bool)
    y0, x0 = 300, 400
    m[frames[0]:frames[1], y0:y0 + box[0], x0:x0 + box[1]] = True
    return m
