"""Host restatement of the clean-plate warp (include/platewarp.h): vvw_search, vvw_place and vvw_unplace in numpy, the stage round them
(platealign_ref's tracker and fill, videovanish_amd.platewarp's exact fit: that module is pure Python and is the product's own host part), and
the synthetic clip with pan, zoom and roll.  Everything is integer; the device must agree bit for bit."""
import numpy as np

import platealign_ref as A
import platefill_ref as R
from videovanish_amd import platewarp as PW

DEFAULTS = dict(block=16, search=8, min_texture=2, min_blocks=12, trim=10, rounds=3, max_linear=50)
MAXS = 8


# ---- rule S -----------------------------------------------------------------------------------------------------------------------------------
def _moved(plane, sy, sx, h, w):
    """out[y, x] = plane[y + sy, x + sx] for (y, x) in [0, h) x [0, w), 0 where the plane has no pixel."""
    H, W = plane.shape
    out = np.zeros((h, w), plane.dtype)
    y0, y1, x0, x1 = max(0, -sy), min(h, H - sy), max(0, -sx), min(w, W - sx)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = plane[y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    return out


def search(Y, V, track, block=16, search=8, min_texture=2, max_residual=12):
    """vvw_search: Y [T,H,W] integer luma, V [T,H,W] bool valid (level 0 of platealign_ref.pyramid), track [T,8] -> (rec [T,nby,nbx,4] int32,
    stats [T,4] int64)."""
    Y, V = np.asarray(Y).astype(np.int64), np.asarray(V) != 0
    T, H, W = Y.shape
    B = block
    nby, nbx = H // B, W // B
    rec, stats = np.zeros((T, nby, nbx, 4), np.int32), np.zeros((T, 4), np.int64)
    if nby == 0 or nbx == 0:
        return rec, stats
    h, w = nby * B, nbx * B
    sums = lambda a: a.reshape(nby, B, nbx, B).sum(axis=(1, 3))
    NOBODY = np.iinfo(np.int64).max
    for t in range(T):
        key = int(track[t][2])
        if track[t][3] != 1 or not (0 <= key < T) or key == t:
            continue
        Yt, Vt = Y[t, :h, :w], V[t, :h, :w]
        act = np.zeros_like(Yt)
        dxa, dya = np.abs(np.diff(Yt, axis=1)), np.abs(np.diff(Yt, axis=0))
        dxa[:, B - 1::B] = 0                      # a difference across two blocks belongs to neither
        dya[B - 1::B, :] = 0
        act[:, :-1] += dxa
        act[:-1, :] += dya
        usable = (sums(Vt.astype(np.int64)) == B * B) & (sums(act) >= min_texture * B * B)
        d0x, d0y = int(track[t][0]) - int(track[key][0]), int(track[t][1]) - int(track[key][1])
        best = np.full((nby, nbx), NOBODY, np.int64)
        for dy in range(-search, search + 1):
            for dx in range(-search, search + 1):
                Yk, Vk = _moved(Y[key], d0y + dy, d0x + dx, h, w), _moved(V[key], d0y + dy, d0x + dx, h, w)
                cost, valid = sums(np.abs(Yk - Yt)), sums(Vk.astype(np.int64)) == B * B
                k = (cost << 32) | ((dx * dx + dy * dy) << 16) | ((dy + MAXS) << 8) | (dx + MAXS)
                best = np.where(valid & (k < best), k, best)
        cost = best >> 32
        used = usable & (best != NOBODY) & (cost <= max_residual * B * B)
        rec[t, ..., 0] = np.where(used, (best & 255) - MAXS, 0)
        rec[t, ..., 1] = np.where(used, ((best >> 8) & 255) - MAXS, 0)
        rec[t, ..., 2] = used
        rec[t, ..., 3] = np.where(used, cost, 0)
        stats[t] = [usable.sum(), used.sum(), np.where(used, cost, 0).sum(), (np.abs(rec[t, ..., 0]) + np.abs(rec[t, ..., 1])).sum()]
    return rec, stats


# ---- rules M, P, U ----------------------------------------------------------------------------------------------------------------------------
def map_points(tab, x, y):
    """Rule M on int64 arrays: numpy's int64 products and sums wrap modulo 2^64 and >> is arithmetic, as the rule says."""
    tab = np.asarray([int(v) for v in tab], dtype=np.int64)
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    with np.errstate(over="ignore"):
        half = np.int64(1 << 19)
        return (tab[0] + tab[1] * x + tab[2] * y + half) >> 20, (tab[3] + tab[4] * x + tab[5] * y + half) >> 20


def place(frames, dil, inv, tracked, box):
    """vvw_place -> (canvas [T,ch,cw,3], dil_c, invalid_c [T,ch,cw]) u8."""
    frames, dil = np.asarray(frames), np.asarray(dil)
    T, H, W = dil.shape
    y0, x0, y1, x1 = box
    ch, cw = y1 - y0, x1 - x0
    canvas, dil_c, inv_c = np.zeros((T, ch, cw, 3), np.uint8), np.zeros((T, ch, cw), np.uint8), np.full((T, ch, cw), 255, np.uint8)
    cy, cx = np.mgrid[y0:y1, x0:x1]
    for t in range(T):
        if not tracked[t]:
            continue
        fx, fy = map_points(inv[t], cx, cy)
        ok = (fy >= 0) & (fy < H) & (fx >= 0) & (fx < W)
        canvas[t][ok] = frames[t][fy[ok], fx[ok]]
        dil_c[t][ok] = dil[t][fy[ok], fx[ok]]
        inv_c[t][ok] = 0
    return canvas, dil_c, inv_c


def unplace(canvas, dil_c, dil_out_c, dil, fwd, tracked, box, patch_box):
    """vvw_unplace -> (patch [T,ph,pw,3] u8, dil_out [T,H,W] u8)."""
    dil = np.asarray(dil)
    T, H, W = dil.shape
    y0, x0, y1, x1 = box
    py0, px0, py1, px1 = patch_box
    full, out = np.zeros((T, H, W, 3), np.uint8), dil.copy()
    yy, xx = np.mgrid[0:H, 0:W]
    for t in range(T):
        if not tracked[t]:
            continue
        jx, jy = map_points(fwd[t], xx, yy)
        jx, jy = jx - x0, jy - y0
        ok = (dil[t] != 0) & (jy >= 0) & (jy < y1 - y0) & (jx >= 0) & (jx < x1 - x0)
        jyc, jxc = np.where(ok, jy, 0), np.where(ok, jx, 0)
        ok &= (dil_c[t][jyc, jxc] != 0) & (dil_out_c[t][jyc, jxc] == 0)
        full[t][ok] = canvas[t][jyc[ok], jxc[ok]]
        out[t][ok] = 0
    return full[:, py0:py1, px0:px1].copy(), out


def mask_boxes(dil):
    """hip.mask_bbox: [T,4] half-open (y0, x0, y1, x1), all zero for an empty mask."""
    out = np.zeros((len(dil), 4), np.int64)
    for t, m in enumerate(np.asarray(dil) != 0):
        if m.any():
            ys, xs = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
            out[t] = [ys[0], xs[0], ys[-1] + 1, xs[-1] + 1]
    return out


def patch_box(boxes, H, W):
    """platefill.crop_box."""
    live = [b for b in boxes if b[2] > b[0] and b[3] > b[1]]
    y0, x0, y1, x1 = min(b[0] for b in live), min(b[1] for b in live), max(b[2] for b in live), max(b[3] for b in live)
    return int(y0), int(x0 - x0 % 4), int(y1), int(min(W, -(-x1 // 4) * 4))


# ---- the stage --------------------------------------------------------------------------------------------------------------------------------
def fill_segment(frames, dil, acfg=None, wcfg=None, max_bytes=1 << 30, **cfg):
    """One segment with alignment and warp -> (frames', dil', counts [T,2], info): platealign_ref.fill_segment's answer with info["path"] as
    plate_align gives it unless the segment is searched (plate_align's path "canvas"); then info gains warp = "warp" / "translation" /
    "fallback", plan (a platewarp.Plan), rec, stats and wbox, and on "warp" the answer is the warped canvas'."""
    frames, dil = np.asarray(frames), np.asarray(dil)
    acfg = dict(A.DEFAULTS, **(acfg or {}))
    wcfg = PW.PlateWarpConfig(**dict(DEFAULTS, **(wcfg or {})))
    T, H, W = dil.shape
    base = A.fill_segment(frames, dil, acfg, max_bytes, **cfg)
    info = base[3]
    info["warp"] = info["path"]
    if info["path"] != "canvas":
        return base
    track = info["track"]
    Y, V = A.pyramid(frames, dil, 0)[0]
    rec, stats = search(Y, V, track, wcfg.block, wcfg.search, wcfg.min_texture, acfg["max_residual"])
    boxes = mask_boxes(dil)
    plan = PW.plan_segment(track, rec, wcfg, H, W, boxes)
    info.update(rec=rec, stats=stats, plan=plan, wbox=None)
    if plan.translation:
        info["warp"] = "translation"
        return base
    wbox = PW.canvas_box(boxes, plan.fwd, plan.tracked)
    info["wbox"] = wbox
    if wbox is None or PW.canvas_bytes(T, wbox) > max_bytes:
        info["warp"] = "fallback"
        return base
    info["warp"] = "warp"
    canvas, dil_c, inv_c = place(frames, dil, plan.inv, plan.tracked, wbox)
    out_c, d2_c, _ = A.fill_canvas(canvas, dil_c, inv_c, **dict(R.DEFAULTS, **cfg))
    pbox = patch_box(boxes, H, W)
    patch, dil2 = unplace(out_c, dil_c, d2_c, dil, plan.fwd, plan.tracked, wbox, pbox)
    went = (dil != 0) & (dil2 == 0)
    out = frames.copy()
    view = out[:, pbox[0]:pbox[2], pbox[1]:pbox[3]]
    m = went[:, pbox[0]:pbox[2], pbox[1]:pbox[3]]
    view[m] = patch[m]
    counts = np.stack([went.reshape(T, -1).sum(1), (dil2 != 0).reshape(T, -1).sum(1)], axis=1).astype(np.int64)
    return out, dil2, counts, info


def plate_fill(frames, dil, cuts=None, acfg=None, wcfg=None, max_bytes=1 << 30, **cfg):
    """The whole clip -> (frames', dil', counts [T,2], [info per segment])."""
    frames, dil = np.asarray(frames), np.asarray(dil)
    out, dout, counts, infos = frames.copy(), np.zeros_like(dil), np.zeros((len(frames), 2), np.int64), []
    for s, e in R.segments(len(frames), cuts):
        out[s:e], dout[s:e], counts[s:e], info = fill_segment(frames[s:e], dil[s:e], acfg, wcfg, max_bytes, **cfg)
        infos.append(info)
    return out, dout, counts, infos


# ---- the clip ---------------------------------------------------------------------------------------------------------------------------------
def still(h, w, seed=0, k=2):
    """Smoothed iid noise: two box blurs of 2k + 1, rescaled to 20 .. 235 -> [h,w,3] float64."""
    rng = np.random.default_rng(seed + 5000)
    s = A.smooth(A.smooth(rng.integers(0, 256, (h, w, 3)) * 256, k), k).astype(np.float64)
    lo, hi = s.min(), s.max()
    return 20.0 + (s - lo) * (215.0 / (hi - lo))


def true_map(t, H, W, zoom=0.004, roll=0.15):
    """Frame t's pixel (x, y) shows the still at centre + pan_t + z_t R(roll_t) ((x, y) - centre); frame 0 is the identity plus the centre, so this
    is also the true map from frame t to frame 0 -> ((ax, bx, cx), (ay, by, cy)) floats."""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    z, a = 1.0 + zoom * t, np.deg2rad(roll * t)
    px, py = float(2 * t), float(t // 4)
    b, c, e, f = z * np.cos(a), -z * np.sin(a), z * np.sin(a), z * np.cos(a)
    return ((cx + px - b * cx - c * cy, b, c), (cy + py - e * cx - f * cy, e, f))


def warp_clip(T=12, H=96, W=128, seed=0, box=24, box_speed=9, dilate=2, zoom=0.004, roll=0.15):
    """T frames of H x W sampled bilinearly from still() with pan (2 t, t // 4), zoom 1 + zoom t and roll roll t degrees about the centre; a
    bright box of `box` px crosses from the left and is masked, the mask dilated `dilate` times.  Noise-free.  -> (frames u8, masks u8
    {0, 255}, truth u8 = the same sampling without the box, maps [T] = true_map)."""
    margin = 40
    wide = still(H + 2 * margin + T // 4, W + 2 * margin + 2 * T, seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    truth, maps = [], []
    for t in range(T):
        (ax, bx, cx), (ay, by, cy) = m = true_map(t, H, W, zoom, roll)
        maps.append(m)
        sx, sy = ax + bx * xx + cx * yy + margin, ay + by * xx + cy * yy + margin
        x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
        fx, fy = (sx - x0)[..., None], (sy - y0)[..., None]
        v = (wide[y0, x0] * (1 - fx) + wide[y0, x0 + 1] * fx) * (1 - fy) + (wide[y0 + 1, x0] * (1 - fx) + wide[y0 + 1, x0 + 1] * fx) * fy
        truth.append(np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8))
    truth = np.stack(truth)
    rng = np.random.default_rng(seed + 6000)
    boxm = np.zeros((T, H, W), bool)
    for t in range(T):
        x0 = -box // 2 + box_speed * t
        boxm[t, H // 3: H // 3 + box, max(x0, 0): max(min(x0 + box, W), 0)] = True
    frames = truth.copy()
    frames[boxm] = 250 - rng.integers(0, 30, (int(boxm.sum()), 3))
    return frames, (R.dilate(boxm, dilate) * 255).astype(np.uint8), truth, maps
