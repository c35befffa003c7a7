"""Clean-plate exposure matching, measured on one MI355X: its kernels one by one on the same inputs, and the stage against the fill alone.

--frames (32,256) resident frames at 1280 x 720 and at 1920 x 1080: a locked-off still with grain of +-4 levels whose exposure drifts by
1 level per frame and flickers by +-4 % from frame to frame, a box of 5/24 of the frame's width and 5/18 of its height that crosses the
frame from edge to edge during the clip and a static 160 x 90 logo that no frame reveals; the masks are box | logo, dilated 8 times.  The
kernels run on what the stage uploads: the crop of the masks' union box widened by `ring`.  Per case, in one process on the same tensors:

  guard time_bridge_grow   vvm_time_bridge_grow(dil, 0, guard): the sample frames (the fill needs them too)
  mean_plane               vve_mean_plane: one walk over the frames and the sample flags (rules 1 and 2)
  moments                  vve_moments: the image where the support is set, and the mean (rule 3)
  apply                    vve_apply: the crop through the forward tables (rule 6)
  restore                  vve_restore: the filled pixels through the back tables into a fresh crop (rule 6)

Each call is warmed up once, then --rounds (9) rounds time every call once, in turn (events around the call on the launch stream), so the
calls share whatever else the box is doing; the median and the spread (min .. max) are printed, and for vve_mean_plane and vve_apply the
nominal bytes (mean_plane: the image and the flags read once, its planes written; apply: the image read and written) against the median.
Then the stage itself (infill.plate_fill on the host frames, with and without tcfg=), wall clock, best of three.  No speed is asserted.

  python tools/bench_platetone.py [--frames 32,256] [--rounds 9] [--out FILE]
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


def make_clip(T, H, W, seed=7):
    """(frames: list of T [H,W,3] u8, raw masks [T,H,W,1] u8)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W].astype(np.float32)
    still = np.stack([120.0 + 40.0 * (np.sin(5 * xx / W + 3 * yy / H + c) + np.sin(7 * yy / H - 2 * xx / W + 2 * c)) / 2 for c in range(3)], axis=-1)
    still = np.rint(still).astype(np.int32)
    bw, bh = W * 5 // 24, H * 5 // 18
    y0 = H // 4
    ly, lx = y0 + bh + 60, W // 2
    raw = np.zeros((T, H, W, 1), np.uint8)
    frames = []
    for t in range(T):
        lit = (still + min(t, 40)) * (104 if t % 2 == 0 else 96) // 100                    # the drift stops at 40 levels: nothing clips
        f = np.clip(lit + rng.integers(-4, 5, (H, W, 3), dtype=np.int32), 0, 255).astype(np.uint8)
        x0 = -bw + (t * (W + bw)) // max(T - 1, 1)
        a, b = max(x0, 0), max(min(x0 + bw, W), 0)
        raw[t, y0:y0 + bh, a:b] = 255
        f[y0:y0 + bh, a:b] = 240
        raw[t, ly:ly + 90, lx:lx + 160] = 255
        f[ly:ly + 90, lx:lx + 160] = 16
        frames.append(f)
    return frames, raw


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="32,256")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from videovanish_amd import hip, infill, mask_hip, platefill, platetone, platetone_bind, shadowmask
    if not torch.cuda.is_available():
        raise SystemExit("bench_platetone.py measures on the GPU: no HIP device visible")
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

    cfg, pcfg = platetone.PlateToneConfig(), platefill.PlateFillConfig(max_bytes=1 << 32)
    dev = torch.device("cuda:0")
    emit(f"# bench_platetone: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds after one warm-up, median (min .. max) ms; {cfg}")
    for T in [int(x) for x in args.frames.split(",")]:
        for H, W in SIZES:
            frames, raw = make_clip(T, H, W)
            dil = torch.cat([hip.mask_collapse_dilate(torch.from_numpy(raw[a:a + 32]).to(dev).contiguous(), 8) for a in range(0, T, 32)])
            del raw
            box = platefill.crop_box(hip.mask_bbox(dil).cpu().numpy(), H, W)
            y0, x0, y1, x1 = shadowmask.widen_box(box, H, W, cfg.ring)
            d = dil[:, y0:y1, x0:x1].contiguous()
            f = torch.from_numpy(np.stack([fr[y0:y1, x0:x1] for fr in frames])).to(dev)
            ns = mask_hip.time_bridge_grow(d, 0, pcfg.guard)[0]
            mean, support, n = platetone_bind.mean_plane(f, ns, cfg.floor)
            fit = platetone.fit_segment(int(n.item()), platetone_bind.moments(f, mean, support).cpu().numpy(), cfg)
            fwd, back = infill._tables(fit.fwd, T, dev), infill._tables(fit.back, T, dev)
            ident = torch.from_numpy(np.frombuffer(fit.identity, np.uint8).copy()).to(dev)
            f1 = platetone_bind.apply(f, fwd, ident)
            d2 = infill._fill_device(f1, d, None, pcfg, None, ns)[0]
            calls = [("guard time_bridge_grow", lambda: mask_hip.time_bridge_grow(d, 0, pcfg.guard)),
                     ("mean_plane", lambda: platetone_bind.mean_plane(f, ns, cfg.floor)),
                     ("moments", lambda: platetone_bind.moments(f, mean, support)),
                     ("apply", lambda: platetone_bind.apply(f, fwd, ident)),
                     ("restore", lambda: platetone_bind.restore(f, f1, d, d2, back))]
            for _, fn in calls:
                event_ms(fn)                                                                   # warm-up
            ms = {name: [] for name, _ in calls}
            for _ in range(args.rounds):
                for name, fn in calls:
                    ms[name].append(event_ms(fn))
            h, w = y1 - y0, x1 - x0
            gains = [p.an / p.ad for fs in fit.fits for p in fs]
            emit(f"# {W}x{H}, {T} frames: crop {w}x{h} ({f.numel() / 2 ** 20:.0f} MiB), support {fit.n} of {h * w} px, {T - sum(fit.identity)} of {T} frames "
                 f"matched, gains {min(gains):.3f} .. {max(gains):.3f}, {int(((d != 0) & (d2 == 0)).sum().item())} px filled")
            nominal = {"mean_plane": T * h * w * 4 + h * w * 4, "apply": T * h * w * 6}
            for name, _ in calls:
                v = ms[name]
                med = statistics.median(v)
                rec = {"frame": f"{W}x{H}", "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "ms_per_frame": round(med / T, 5)}
                more = ""
                if name in nominal:
                    rec.update(bytes=nominal[name], tb_per_s=round(nominal[name] / med / 1e9, 3))
                    more = f"  {nominal[name] / 2 ** 20:.0f} MiB nominal, {nominal[name] / med / 1e9:.2f} TB/s"
                records.append(rec)
                emit(f"{W}x{H} T={T:3d} {name:24s} {med:8.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med / T:.4f} ms/frame{more}")
            del f, f1, d2, fwd, back, mean, support, ns
            torch.cuda.empty_cache()
            plain, (_, _, rep0) = wall_ms(lambda: infill.plate_fill(frames, dil, pcfg, None))
            toned, (_, _, rep1) = wall_ms(lambda: infill.plate_fill(frames, dil, pcfg, None, tcfg=cfg))
            records.append({"frame": f"{W}x{H}", "frames": T, "call": "stage", "plate_fill_ms": round(plain, 2), "with_plate_tone_ms": round(toned, 2)})
            emit(f"{W}x{H} T={T:3d} stage (wall, best of 3): plate_fill alone {plain:.1f} ms ({int(rep0.filled.sum())} px filled), with plate_tone "
                 f"{toned:.1f} ms ({int(rep1.filled.sum())} px filled)")
            flush()
            del frames, dil, d
            torch.cuda.empty_cache()
    js = json.dumps({"bench_platetone": records, "rounds": args.rounds})
    print(js)
    lines.append(js)
    flush()


if __name__ == "__main__":
    main()
