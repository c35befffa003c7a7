"""Clean-plate warp, measured on one MI355X: the block search, the two canvas kernels, and the whole stage beside plate_align alone.

--frames (32) frames at 1280 x 720 and at 1920 x 1080, sampled bilinearly from a wide still with a fixed smooth texture: a pan of 2 px per
frame, a zoom that grows to 0.4 per cent and a roll that grows to 0.2 degrees over the clip, about the centre (together under 6 px at the
corners against frame 0: inside the default search of 8), grain of +-2 levels per frame, a box of 1/8 of the frame's width and 5/18 of its
height that crosses the frame against the pan; the masks are the box, dilated 8 times.  Per case, in one process on the same tensors:

  search             vvw_search of all T frames on the resident pyramid (one launch)
  place / unplace    vvw_place of all T frames onto the warped canvas, vvw_unplace back onto the frames' union mask box

Each call is warmed up once, then --rounds (9) rounds time every call once, in turn (events around the call on the launch stream); the median
and the spread (min .. max) are printed.  Then the stage itself on the host frames, wall clock, best of three: infill.plate_fill with
plate_align + plate_warp and with plate_align alone on the same clip.  Before any time is reported the tool checks that the fitted maps
predict the clip's true displacement at the four corners of every frame within one pixel.  No speed is asserted.

  python tools/bench_platewarp.py [--frames 32] [--rounds 9] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = ((720, 1280), (1080, 1920))
ZOOM, ROLL_DEG, PAN = 0.004, 0.2, 2


def true_map(t, T, H, W):
    """Frame t's pixel (x, y) shows what frame 0 shows at ((ax, bx, cx), (ay, by, cy)) applied to it."""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    u = t / max(T - 1, 1)
    z, a = 1.0 + ZOOM * u, math.radians(ROLL_DEG * u)
    b, c, e, f = z * math.cos(a), -z * math.sin(a), z * math.sin(a), z * math.cos(a)
    return ((cx + PAN * t - b * cx - c * cy, b, c), (cy - e * cx - f * cy, e, f))


def make_clip(T, H, W, dev, seed=7):
    """(frames: list of T [H,W,3] u8, raw masks [T,H,W,1] u8, maps [T] = true_map); sampled on the device, in float64."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    margin = 16
    Hw, Ww = H + 2 * margin, W + 2 * margin + PAN * T
    yy, xx = torch.meshgrid(torch.arange(Hw, dtype=torch.float64), torch.arange(Ww, dtype=torch.float64), indexing="ij")
    noise = torch.randint(-60, 61, (Hw, Ww), generator=g).double()
    for ax in (0, 1):                                                       # a 3-tap box blur along both axes: a texture bilinear sampling keeps
        noise = (noise + noise.roll(1, ax) + noise.roll(-1, ax)) / 3.0
    wide = torch.stack([127.5 + 40.0 * (torch.sin(9 * xx / W + 3 * yy / H + c) + torch.sin(7 * yy / H - 4 * xx / W + 2 * c)) / 2 + noise for c in range(3)], -1).to(dev)
    py, px = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    bw, bh = W // 8, H * 5 // 18
    y0 = H // 2 - bh // 2
    raw = np.zeros((T, H, W, 1), np.uint8)
    frames, maps = [], []
    for t in range(T):
        (ax_, bx_, cx_), (ay_, by_, cy_) = m = true_map(t, T, H, W)
        maps.append(m)
        sx, sy = ax_ + bx_ * px + cx_ * py + margin, ay_ + by_ * px + cy_ * py + margin
        x0, y0f = sx.floor().long(), sy.floor().long()
        fx, fy = (sx - x0)[..., None], (sy - y0f)[..., None]
        v = (wide[y0f, x0] * (1 - fx) + wide[y0f, x0 + 1] * fx) * (1 - fy) + (wide[y0f + 1, x0] * (1 - fx) + wide[y0f + 1, x0 + 1] * fx) * fy
        v = v + torch.randint(-2, 3, (H, W, 3), generator=g).double().to(dev)
        f = v.round().clamp(0, 255).to(torch.uint8).cpu().numpy()
        bx0 = W - (t * (W + bw)) // max(T - 1, 1)
        a, b = max(bx0, 0), max(min(bx0 + bw, W), 0)
        raw[t, y0:y0 + bh, a:b] = 255
        f[y0:y0 + bh, a:b] = 240
        frames.append(f)
    return frames, raw, maps


def corner_error(plan, maps, H, W):
    """The largest distance, per component, between a fitted and a true map at the corners of every tracked frame, in pixels."""
    worst = 0.0
    for m, tm in zip(plan.maps, maps):
        if m is None:
            return float("inf")
        for x in (0, W - 1):
            for y in (0, H - 1):
                worst = max(worst, *(abs(float(r[0] + r[1] * x + r[2] * y) - (q[0] + q[1] * x + q[2] * y)) for r, q in zip(m, tm)))
    return worst


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="32")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from videovanish_amd import align_hip, hip, infill, platealign, platefill, platewarp, platewarp_bind
    if not torch.cuda.is_available():
        raise SystemExit("bench_platewarp.py measures on the GPU: no HIP device visible")
    lines, records = [], []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def wall_ms(fn, n=3):
        best = None
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        return best, r

    pcfg, acfg, wcfg = platefill.PlateFillConfig(), platealign.PlateAlignConfig(), platewarp.PlateWarpConfig()
    dev = torch.device("cuda:0")
    emit(f"# bench_platewarp: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds after one warm-up, median (min .. max) ms; {wcfg}; {acfg}; {pcfg}")
    for T in [int(x) for x in args.frames.split(",")]:
        for H, W in SIZES:
            frames, raw, maps = make_clip(T, H, W, dev)
            dil = torch.cat([hip.mask_collapse_dilate(torch.from_numpy(raw[a:a + 32]).to(dev).contiguous(), 8) for a in range(0, T, 32)])
            del raw
            L = platealign.coarsest_level(H, W, acfg.levels)
            f = torch.from_numpy(np.stack(frames)).to(dev)
            pyr = align_hip.pyramid(f, dil, L)
            track_t = align_hip.track(pyr, H, W, L, acfg.radius, acfg.min_overlap, acfg.max_residual)
            track = track_t.cpu().numpy()
            boxes = hip.mask_bbox(dil).cpu().numpy()
            rec, stats = platewarp_bind.search(pyr, track_t, H, W, wcfg, acfg.max_residual)
            plan = platewarp.plan_segment(track, rec.cpu().numpy(), wcfg, H, W, boxes)
            err = corner_error(plan, maps, H, W)
            if not ((track[:, 3] == 1).all() and err < 1.0 and not plan.translation):
                raise SystemExit(f"bench_platewarp.py: the fit did not recover the clip's maps (largest corner error {err:.2f} px)")
            box = platewarp.canvas_box(boxes, plan.fwd, plan.tracked)
            pbox = platefill.crop_box(boxes, H, W)
            inv_t, fwd_t, flags = platewarp_bind.tables(plan.inv, dev), platewarp_bind.tables(plan.fwd, dev), platewarp_bind.flags(plan.tracked, dev)
            canvas, dil_c, inv_c = platewarp_bind.place(f, dil, inv_t, flags, box)
            d2 = torch.zeros_like(dil_c)
            calls = [("search", lambda: platewarp_bind.search(pyr, track_t, H, W, wcfg, acfg.max_residual)),
                     ("place", lambda: platewarp_bind.place(f, dil, inv_t, flags, box, out=(canvas, dil_c, inv_c))),
                     ("unplace", lambda: platewarp_bind.unplace(canvas, dil_c, d2, dil, fwd_t, flags, box, pbox))]
            for _, fn in calls:
                event_ms(fn)                                                                   # warm-up
            ms = {name: [] for name, _ in calls}
            for _ in range(args.rounds):
                for name, fn in calls:
                    ms[name].append(event_ms(fn))
            st = stats.cpu().numpy()
            emit(f"# {W}x{H}, {T} frames: block {wcfg.block}, search {wcfg.search}, {rec.shape[1] * rec.shape[2]} blocks a frame, {int(st[:, 0].sum())} usable, "
                 f"{int(st[:, 1].sum())} used, {sum(len(x.kept) for x in plan.fits if x is not None)} kept; canvas {box[3] - box[1]}x{box[2] - box[0]} "
                 f"({platewarp.canvas_bytes(T, box) / 2 ** 20:.0f} MiB); largest corner error {err:.2f} px; maps recovered: True")
            for name, _ in calls:
                v = ms[name]
                med = statistics.median(v)
                records.append({"frame": f"{W}x{H}", "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med, 4),
                                "ms_per_frame": round(med / T, 5)})
                emit(f"{W}x{H} T={T:3d} {name:24s} {med:8.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med / T:.4f} ms/frame")
            del f, pyr, canvas, dil_c, inv_c, d2
            torch.cuda.empty_cache()
            got = []
            warped, (_, _, rep) = wall_ms(lambda: infill.plate_fill(frames, dil, pcfg, None, acfg=acfg, wcfg=wcfg, warp_out=got))
            aligned, (_, _, rep0) = wall_ms(lambda: infill.plate_fill(frames, dil, pcfg, None, acfg=acfg))
            records.append({"frame": f"{W}x{H}", "frames": T, "call": "stage", "warp_ms": round(warped, 2), "align_ms": round(aligned, 2), "path": got[-1].path[0],
                            "filled_warp": int(rep.filled.sum()), "filled_align": int(rep0.filled.sum()), "corner_error_px": round(err, 3)})
            emit(f"{W}x{H} T={T:3d} stage (wall, best of 3): with plate_align + plate_warp {warped:.1f} ms ({got[-1].path[0]}; {int(rep.filled.sum())} px filled, "
                 f"{int(rep.left.sum())} px left); with plate_align alone {aligned:.1f} ms ({int(rep0.filled.sum())} px filled, {int(rep0.left.sum())} px left)")
            flush()
            del frames, dil
            torch.cuda.empty_cache()
    js = json.dumps({"bench_platewarp": records, "rounds": args.rounds})
    print(js)
    lines.append(js)
    flush()


if __name__ == "__main__":
    main()
