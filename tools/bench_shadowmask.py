"""Shadow masking, measured on one MI355X: its kernels one by one on the same inputs, and the stage's transfers.

--frames (32,256) resident frames at 1280 x 720 and at 1920 x 1080: a locked-off still with grain of +-4 levels, a box of 5/24 of the frame's
width and 5/18 of its height that crosses the frame from edge to edge during the clip, a shadow band under it (a sheared strip 1/8 of the
frame's height deep at 60 % of the background) and a static 160 x 90 logo that no frame reveals; the masks are box | logo, dilated 8 times.
The kernels run on what the stage uploads: the crop of the masks' union box widened by reach + grow.  Per case, in one process on the same
tensors:

  guard time_bridge_grow   vvm_time_bridge_grow(dil, 0, guard): the sample frames
  plate                    vvh_plate: two walks over the frames (rules 2 and 3)
  candidates               vvh_candidates (rule 4)
  grow                     vvh_grow: ceil(reach / 8) passes of the LDS-tiled growth (rule 5)
  despeckle                vvm_despeckle of what was added (rule 6)
  penumbra dilate          vv_mask_collapse_dilate, `grow` iterations (rule 7)
  merge                    vvh_merge: the union and the counts

Each call is warmed up once, then --rounds (9) rounds time every call once, in turn (events around the call on the launch stream), so the
calls share whatever else the box is doing; the median and the spread (min .. max) are printed, and for vvh_plate the bytes it has to move
(two reads of the image and of the sample flags, one write of its planes) against its median.  Then the stage itself (infill.shadow_mask on
the host frames), wall clock, best of three: the whole call, and its upload (the crop, stacked and copied) measured on its own.  No speed is
asserted.

  python tools/bench_shadowmask.py [--frames 32,256] [--rounds 9] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = ((720, 1280), (1080, 1920))


def make_clip(T, H, W, seed=7, strength=60):
    """(frames: list of T [H,W,3] u8, raw masks [T,H,W,1] u8, the shadow band [T,H,W] bool)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W].astype(np.float32)
    still = np.stack([127.5 + 43.0 * (np.sin(5 * xx / W + 3 * yy / H + c) + np.sin(7 * yy / H - 2 * xx / W + 2 * c)) / 2 for c in range(3)], axis=-1)
    still = np.rint(still).astype(np.int16)
    bw, bh, sh = W * 5 // 24, H * 5 // 18, H // 8
    y0 = H // 4
    ly, lx = y0 + bh + sh + 40, W // 2
    raw = np.zeros((T, H, W, 1), np.uint8)
    band = np.zeros((T, H, W), bool)
    frames = []
    for t in range(T):
        f = np.clip(still + rng.integers(-4, 5, (H, W, 3), dtype=np.int16), 0, 255).astype(np.uint8)
        x0 = -bw + (t * (W + bw)) // max(T - 1, 1)
        a, b = max(x0, 0), max(min(x0 + bw, W), 0)
        for r in range(sh):
            band[t, y0 + bh + r, max(x0 + r, 0):max(min(x0 + r + bw, W), 0)] = True
        f[band[t]] = (f[band[t]].astype(np.uint16) * strength // 100).astype(np.uint8)
        raw[t, y0:y0 + bh, a:b] = 255
        f[y0:y0 + bh, a:b] = 240
        raw[t, ly:ly + 90, lx:lx + 160] = 255
        f[ly:ly + 90, lx:lx + 160] = 16
        frames.append(f)
    return frames, raw, band


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="32,256")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from videovanish_amd import hip, infill, mask_hip, platefill, shadow_hip, shadowmask
    if not torch.cuda.is_available():
        raise SystemExit("bench_shadowmask.py measures on the GPU: no HIP device visible")
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

    cfg = shadowmask.ShadowMaskConfig()
    dev = torch.device("cuda:0")
    emit(f"# bench_shadowmask: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds after one warm-up, median (min .. max) ms; {cfg}")
    for T in [int(x) for x in args.frames.split(",")]:
        for H, W in SIZES:
            frames, raw, band = make_clip(T, H, W)
            dil = torch.cat([hip.mask_collapse_dilate(torch.from_numpy(raw[a:a + 32]).to(dev).contiguous(), 8) for a in range(0, T, 32)])
            del raw
            box = platefill.crop_box(hip.mask_bbox(dil).cpu().numpy(), H, W)
            y0, x0, y1, x1 = shadowmask.widen_box(box, H, W, cfg.widen)
            d = dil[:, y0:y1, x0:x1].contiguous()
            f = torch.from_numpy(np.stack([fr[y0:y1, x0:x1] for fr in frames])).to(dev)
            ns = mask_hip.time_bridge_grow(d, 0, cfg.guard)[0]
            ok, n2, t1 = shadow_hip.plate(f, ns, cfg.min_samples, cfg.tol)
            cand, counts = shadow_hip.candidates(f, d, ok, n2, t1, cfg.lo, cfg.hi, cfg.drop, cfg.chroma, cfg.floor)
            s5 = shadow_hip.grow(d, cand, cfg.reach)
            s6 = mask_hip.despeckle(s5, s5, cfg.min_area)[0]
            s7 = hip.mask_collapse_dilate(s6[..., None], cfg.grow)
            d2 = shadow_hip.merge(d, s7, counts)
            c = counts.cpu().numpy()
            true = torch.from_numpy(band[:, y0:y1, x0:x1]).to(dev) & (d == 0)
            found = int(((d2 != 0) & true).sum().item())
            scratch = torch.empty_like(counts)
            calls = [("guard time_bridge_grow", lambda: mask_hip.time_bridge_grow(d, 0, cfg.guard)),
                     ("plate", lambda: shadow_hip.plate(f, ns, cfg.min_samples, cfg.tol)),
                     ("candidates", lambda: shadow_hip.candidates(f, d, ok, n2, t1, cfg.lo, cfg.hi, cfg.drop, cfg.chroma, cfg.floor)),
                     ("grow", lambda: shadow_hip.grow(d, cand, cfg.reach)),
                     ("despeckle", lambda: mask_hip.despeckle(s5, s5, cfg.min_area)),
                     ("penumbra dilate", lambda: hip.mask_collapse_dilate(s6[..., None], cfg.grow)),
                     ("merge", lambda: shadow_hip.merge(d, s7, scratch))]
            for _, fn in calls:
                event_ms(fn)                                                                   # warm-up
            ms = {name: [] for name, _ in calls}
            for _ in range(args.rounds):
                for name, fn in calls:
                    ms[name].append(event_ms(fn))
            h, w = y1 - y0, x1 - x0
            emit(f"# {W}x{H}, {T} frames: crop {w}x{h} ({f.numel() / 2 ** 20:.0f} MiB), {int(ok.sum().item())} of {h * w} px have a plate; "
                 f"{int(c[:, 0].sum())} candidate px, {int(c[:, 1].sum())} px added, {found} of {int(true.sum().item())} shadow px outside the mask found")
            plate_bytes = 2 * T * h * w * 4 + h * w * 17
            for name, _ in calls:
                v = ms[name]
                med = statistics.median(v)
                rec = {"frame": f"{W}x{H}", "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "ms_per_frame": round(med / T, 5)}
                more = ""
                if name == "plate":
                    rec.update(bytes=plate_bytes, tb_per_s=round(plate_bytes / med / 1e9, 3))
                    more = f"  {plate_bytes / 2 ** 20:.0f} MiB moved, {plate_bytes / med / 1e9:.2f} TB/s"
                records.append(rec)
                emit(f"{W}x{H} T={T:3d} {name:24s} {med:8.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med / T:.4f} ms/frame{more}")
            up, _ = wall_ms(lambda: torch.from_numpy(np.stack([fr[y0:y1, x0:x1] for fr in frames])).to(dev))
            total, (_, rep) = wall_ms(lambda: infill.shadow_mask(frames, dil, cfg, None))
            records.append({"frame": f"{W}x{H}", "frames": T, "call": "stage", "upload_ms": round(up, 2), "total_ms": round(total, 2)})
            emit(f"{W}x{H} T={T:3d} stage (wall, best of 3): upload {up:.1f} ms, whole call {total:.1f} ms "
                 f"({int(rep.candidates.sum())} candidate px, {int(rep.added.sum())} px added)")
            flush()
            del frames, band, dil, d, f, ns, ok, n2, t1, cand, counts, s5, s6, s7, d2, true, scratch
            torch.cuda.empty_cache()
    js = json.dumps({"bench_shadowmask": records, "rounds": args.rounds})
    print(js)
    lines.append(js)
    flush()


if __name__ == "__main__":
    main()
