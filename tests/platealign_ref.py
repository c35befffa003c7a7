"""Helpers of the clean-plate alignment tests: the numpy restatement of include/vvalign.h and of the canvas path of
infill.plate_fill(acfg=), written from the header on top of platefill_ref.py and independent of the product code, and the clips the tests
share.  No test in here."""
import numpy as np

import platefill_ref as R

IN_PROGRESS = -1
DEFAULTS = dict(levels=4, radius=4, min_overlap=25, max_residual=12)


# ---- luma and pyramid ---------------------------------------------------------------------------------------------------------------------
def coarsest_level(H, W, levels):
    return max([l for l in range(levels + 1) if l == 0 or min(H, W) >> l >= 16])


def pyramid(frames, dil, L):
    """-> [(Y [T,Hl,Wl] int64, valid [T,Hl,Wl] bool)] for levels 0 .. L."""
    f = np.asarray(frames).astype(np.int64)
    Y = (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8
    V = np.asarray(dil) == 0
    out = [(Y, V)]
    for _ in range(L):
        h, w = Y.shape[1] // 2 * 2, Y.shape[2] // 2 * 2
        a, b, c, d = Y[:, 0:h:2, 0:w:2], Y[:, 0:h:2, 1:w:2], Y[:, 1:h:2, 0:w:2], Y[:, 1:h:2, 1:w:2]
        Y = (a + b + c + d + 2) >> 2
        V = V[:, 0:h:2, 0:w:2] & V[:, 0:h:2, 1:w:2] & V[:, 1:h:2, 0:w:2] & V[:, 1:h:2, 1:w:2]
        out.append((Y, V))
    return out


def pack(pyr):
    """The packed buffer [T, S] u8 of the header."""
    T = len(pyr[0][0])
    return np.concatenate([p.reshape(T, -1).astype(np.uint8) for lv in pyr for p in lv], axis=1)


# ---- cost, one level ------------------------------------------------------------------------------------------------------------------------
def cost(Yk, Vk, Yt, Vt, dx, dy):
    H, W = Yt.shape
    x0, x1, y0, y1 = max(0, -dx), min(W, W - dx), max(0, -dy), min(H, H - dy)
    if x1 <= x0 or y1 <= y0:
        return 0, 0
    both = Vt[y0:y1, x0:x1] & Vk[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    diff = np.abs(Yk[y0 + dy:y1 + dy, x0 + dx:x1 + dx] - Yt[y0:y1, x0:x1])
    return int(diff[both].sum()), int(both.sum())


def live(rec, T, level):
    return rec[3] == IN_PROGRESS and rec[7] == level and 0 <= rec[2] < T and abs(int(rec[0])) <= 1 << 24 and abs(int(rec[1])) <= 1 << 24


def sad_level(pyr, track, t, level, r):
    """vva_sad -> acc [(2r+1)^2, 2] int64."""
    side = 2 * r + 1
    acc = np.zeros((side * side, 2), np.int64)
    rec = track[t]
    if not live(rec, len(track), level):
        return acc
    Y, V = pyr[level]
    k = int(rec[2])
    for j in range(side):
        for i in range(side):
            acc[j * side + i] = cost(Y[k], V[k], Y[t], V[t], int(rec[0]) + i - r, int(rec[1]) + j - r)
    return acc


def pick_level(acc, track, H, W, L, t, level, r, min_overlap, max_residual):
    """vva_pick, in place on track [T,8] int32."""
    T = len(track)
    rec = track[t]
    if not live(rec, T, level):
        return
    cx, cy, key = int(rec[0]), int(rec[1]), int(rec[2])
    side = 2 * r + 1
    Hl, Wl = H >> level, W >> level
    best = None
    for c in range(side * side):
        s, n = int(acc[c, 0]), int(acc[c, 1])
        if n < 1 or 100 * n < min_overlap * Hl * Wl:
            continue
        ox, oy = c % side - r, c // side - r
        cand = (s, n, ox * ox + oy * oy, cy + oy, cx + ox)
        if best is None:
            best = cand
            continue
        l, rr = cand[0] * best[1], best[0] * cand[1]
        if l < rr or (l == rr and cand[2:] < best[2:]):
            best = cand
    if best is not None and level > 0:
        rec[0], rec[1], rec[7] = 2 * best[4], 2 * best[3], level - 1
        return
    tracked = best is not None and best[0] <= max_residual * best[1]
    q = t - 1
    while q > 0 and track[q, 3] != 1:
        q -= 1
    q = max(q, 0)
    kx, ky = int(track[key, 0]), int(track[key, 1])
    ox, oy = (kx + best[4], ky + best[3]) if tracked else (int(track[q, 0]), int(track[q, 1]))
    s, n = (best[0], best[1]) if best is not None else (0, 0)
    lo = ((s & 0xffffffff) ^ 0x80000000) - 0x80000000                    # the low word as the int32 the record holds
    track[t] = [ox, oy, key, int(tracked), lo, s >> 32, n, level]
    if t + 1 < T:
        far = 4 * abs(ox - kx) > W or 4 * abs(oy - ky) > H
        nkey = t if tracked and far else key
        nq = t if tracked else q
        px, py = int(track[nq, 0]) - int(track[nkey, 0]), int(track[nq, 1]) - int(track[nkey, 1])
        tz = lambda v: -((-v) >> L) if v < 0 else v >> L                   # toward zero
        track[t + 1] = [tz(px), tz(py), nkey, IN_PROGRESS, 0, 0, 0, L]


def track_segment(frames, dil, levels=4, radius=4, min_overlap=25, max_residual=12, pyr=None):
    """vva_track on the host's L -> track [T,8] int32."""
    T, H, W = np.asarray(dil).shape
    L = coarsest_level(H, W, levels)
    pyr = pyramid(frames, dil, L) if pyr is None else pyr
    track = np.zeros((T, 8), np.int32)
    track[0, 3] = 1
    if T > 1:
        track[1] = [0, 0, 0, IN_PROGRESS, 0, 0, 0, L]
    for t in range(1, T):
        for level in range(L, -1, -1):
            r = radius if level == L else 1
            pick_level(sad_level(pyr, track, t, level, r), track, H, W, L, t, level, r, min_overlap, max_residual)
    return track


# ---- canvas ---------------------------------------------------------------------------------------------------------------------------------
def canvas_box(dil, track):
    """The union of the tracked frames' mask boxes moved by their offsets, x to multiples of 4 -> (y0, x0, y1, x1) or None."""
    y0 = x0 = 1 << 40
    y1 = x1 = -(1 << 40)
    for m, rec in zip(np.asarray(dil) != 0, track):
        if rec[3] != 1 or not m.any():
            continue
        ys, xs = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
        y0, y1 = min(y0, ys[0] + rec[1]), max(y1, ys[-1] + 1 + rec[1])
        x0, x1 = min(x0, xs[0] + rec[0]), max(x1, xs[-1] + 1 + rec[0])
    if y1 <= y0:
        return None
    return int(y0), int(x0 // 4 * 4), int(y1), int(-(-x1 // 4) * 4)


def place(arr, track, box, fill=0, tracked_only=True):
    """arr [T,H,W,...] in frame coordinates -> [T,ch,cw,...] on the canvas, `fill` where no tracked frame pixel lies; and the bool plane of
    those places."""
    y0, x0, y1, x1 = box
    T, H, W = arr.shape[:3]
    out = np.full((T, y1 - y0, x1 - x0) + arr.shape[3:], fill, arr.dtype)
    inv = np.ones((T, y1 - y0, x1 - x0), bool)
    for t, rec in enumerate(track):
        if tracked_only and rec[3] != 1:
            continue
        ox, oy = int(rec[0]), int(rec[1])
        fy0, fy1, fx0, fx1 = max(y0 - oy, 0), min(y1 - oy, H), max(x0 - ox, 0), min(x1 - ox, W)
        if fy1 <= fy0 or fx1 <= fx0:
            continue
        out[t, fy0 + oy - y0:fy1 + oy - y0, fx0 + ox - x0:fx1 + ox - x0] = arr[t, fy0:fy1, fx0:fx1]
        inv[t, fy0 + oy - y0:fy1 + oy - y0, fx0 + ox - x0:fx1 + ox - x0] = False
    return out, inv


def place_masks(dil, track, box):
    """vva_place_masks -> (dil_c, invalid_c u8 {0, 255})."""
    d, inv = place(np.asarray(dil), track, box)
    return d, inv.astype(np.uint8) * 255


def unplace_mask(dil_out_c, dil, track, box):
    """vva_unplace_mask -> dil_out [T,H,W]."""
    y0, x0, y1, x1 = box
    out = np.asarray(dil).copy()
    T, H, W = out.shape
    for t, rec in enumerate(track):
        if rec[3] != 1:
            continue
        ox, oy = int(rec[0]), int(rec[1])
        fy0, fy1, fx0, fx1 = max(y0 - oy, 0), min(y1 - oy, H), max(x0 - ox, 0), min(x1 - ox, W)
        if fy1 > fy0 and fx1 > fx0:
            out[t, fy0:fy1, fx0:fx1] = dil_out_c[t, fy0 + oy - y0:fy1 + oy - y0, fx0 + ox - x0:fx1 + ox - x0]
    return out


def fill_canvas(canvas, dil_c, inv_c, guard=1, min_samples=4, tol=6, outlier=3, max_gap=0, margin=2):
    """Rules 1 - 7 of vvplate.h on the canvas, with the places no frame covers added to `notsample` -> (canvas', dil_c', counts [T,2])."""
    T = len(canvas)
    ns = R.not_sample(dil_c, guard) | (inv_c != 0)
    n, S1, S2 = R.stats(canvas, ns)
    st = R.steady(n, S1, S2, min_samples, tol)
    us = R.usable(canvas, ns, st, n, S1, tol, outlier)
    src = R.sources(dil_c, us, max_gap)
    masked = dil_c != 0
    keep = R.dilate(masked & (src == R.NONE), margin) & masked
    go = masked & ~keep
    out = canvas.copy()
    tt, yy, xx = np.nonzero(go)
    out[tt, yy, xx] = canvas[src[tt, yy, xx].astype(np.int64), yy, xx]
    return out, keep.astype(np.uint8) * 255, np.stack([go.reshape(T, -1).sum(1), keep.reshape(T, -1).sum(1)], axis=1).astype(np.int64)


def fill_segment(frames, dil, acfg=None, max_bytes=1 << 30, **cfg):
    """One segment with alignment -> (frames', dil', counts [T,2], info): info = dict(track, box, path) with path "static" (every offset zero:
    platefill_ref.fill_segment), "canvas", "fallback" (the canvas exceeds max_bytes: the static path) or "none" (no tracked frame has a mask)."""
    frames, dil = np.asarray(frames), np.asarray(dil)
    cfg = dict(R.DEFAULTS, **cfg)
    track = track_segment(frames, dil, **dict(DEFAULTS, **(acfg or {})))
    info = dict(track=track, box=None, path="static")
    if (track[:, 3] == 1).all() and not track[:, :2].any():
        return R.fill_segment(frames, dil, **cfg) + (info,)
    box = canvas_box(dil, track)
    info["box"] = box
    counts = np.zeros((len(frames), 2), np.int64)
    counts[:, 1] = (dil != 0).reshape(len(dil), -1).sum(1)
    if box is None:
        info["path"] = "none"
        return frames.copy(), dil.copy(), counts, info
    if len(frames) * (box[2] - box[0]) * (box[3] - box[1]) * 3 > max_bytes:
        info["path"] = "fallback"
        return R.fill_segment(frames, dil, **cfg) + (info,)
    info["path"] = "canvas"
    canvas, _ = place(frames, track, box, tracked_only=False)
    dil_c, inv_c = place_masks(dil, track, box)
    out_c, d2_c, c = fill_canvas(canvas, dil_c, inv_c, **cfg)
    ok = track[:, 3] == 1
    counts[ok] = c[ok]
    filled_c = (dil_c != 0) & (d2_c == 0)
    out = frames.copy()
    y0, x0 = box[0], box[1]
    for t, yy, xx in zip(*np.nonzero(filled_c)):
        out[t, yy + y0 - track[t, 1], xx + x0 - track[t, 0]] = out_c[t, yy, xx]
    return out, unplace_mask(d2_c, dil, track, box), counts, info


def plate_fill(frames, dil, cuts=None, acfg=None, max_bytes=1 << 30, **cfg):
    """The whole clip -> (frames', dil', counts [T,2], [info per segment])."""
    frames, dil = np.asarray(frames), np.asarray(dil)
    out, dout, counts, infos = frames.copy(), np.zeros_like(dil), np.zeros((len(frames), 2), np.int64), []
    for s, e in R.segments(len(frames), cuts):
        out[s:e], dout[s:e], counts[s:e], info = fill_segment(frames[s:e], dil[s:e], acfg, max_bytes, **cfg)
        infos.append(info)
    return out, dout, counts, infos


# ---- clips ----------------------------------------------------------------------------------------------------------------------------------
def smooth(a, k=2):
    """A box blur of 2k + 1 along both image axes (wrapping), integers."""
    a = a.astype(np.int64)
    for ax in (0, 1):
        a = sum(np.roll(a, s, axis=ax) for s in range(-k, k + 1)) // (2 * k + 1)
    return a


def pan_clip(T=12, H=96, W=128, seed=0, kind="iid", noise=3, steps_x=(2, 5), steps_y=(-2, 2), box=(30, 28), box_speed=9, logo=None):
    """A pan over a wide still with integer offsets: frame t shows wide[oy_t : oy_t + H, ox_t : ox_t + W] plus iid noise in [-noise, noise], a
    bright box crossing the screen at box_speed px per frame (negative: from the right) and an optional screen-fixed logo (y0, x0, y1, x1).  kind: "iid" texture or "smooth" (its blur, stretched
    back over the range).  Returns (frames u8, masks u8 {0, 255}, off [T,2] int = (x, y) against frame 0, clean [T,H,W,3] = the noise-free
    pan, boxm [T,H,W] bool, logom [H,W] bool)."""
    rng = np.random.default_rng(seed + 3000)
    sx = rng.integers(steps_x[0], steps_x[1] + 1, T - 1)
    sy = rng.integers(steps_y[0], steps_y[1] + 1, T - 1)
    off = np.zeros((T, 2), np.int64)
    off[1:, 0], off[1:, 1] = np.cumsum(sx), np.cumsum(sy)
    my, mx = int(max(-off[:, 1].min(), 0)), int(max(-off[:, 0].min(), 0))
    wide = rng.integers(0, 256, (H + my + int(off[:, 1].max()) + 1, W + mx + int(off[:, 0].max()) + 1, 3))
    if kind == "smooth":
        s = smooth(wide)
        wide = np.clip((s - 128) * 4 + 128, 20, 235)
    else:
        wide = np.clip(wide, 20, 235)
    clean = np.stack([wide[my + oy: my + oy + H, mx + ox: mx + ox + W] for ox, oy in off])
    frames = clean + rng.integers(-noise, noise + 1, clean.shape) if noise else clean.copy()
    boxm = np.zeros((T, H, W), bool)
    for t in range(T):
        x0 = (-box[1] // 2 if box_speed >= 0 else W - box[1] // 2) + box_speed * t      # enters from the left, or from the right
        boxm[t, H // 4: H // 4 + box[0], max(x0, 0): max(min(x0 + box[1], W), 0)] = True
    logom = np.zeros((H, W), bool)
    if logo is not None:
        logom[logo[0]:logo[2], logo[1]:logo[3]] = True
    frames[boxm] = 250 - rng.integers(0, 30, (int(boxm.sum()), 3))
    frames[:, logom] = 20
    return np.clip(frames, 0, 255).astype(np.uint8), ((boxm | logom[None]) * 255).astype(np.uint8), off, clean, boxm, logom


STAGE_CLIPS = {(40, 56): dict(T=12, box=(15, 12), box_speed=-6), (45, 83): dict(T=16, box=(15, 16), box_speed=-8),
               (96, 132): dict(T=20, box=(30, 24), box_speed=-10)}


def stage_clip(H=40, W=56, logo=None, seed=1):
    """The clip the unaligned stage cannot fill: a noise-free iid texture panning 3 px per frame, a box that enters from the right and crosses
    against the pan (so every place it hides is in view, unhidden, in at least four other frames), an optional screen-fixed logo.  Returns
    pan_clip's tuple."""
    return pan_clip(H=H, W=W, seed=seed, noise=0, steps_x=(3, 3), steps_y=(0, 0), logo=logo, **STAGE_CLIPS[H, W])
