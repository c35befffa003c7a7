"""Clean-plate grain, measured on one MI355X: vvl_sources against vvp_sources at equal arguments, on the same box, interleaved.

The four geometries of tools/bench_platefill.py (its clips: --frames (32,256) resident frames at 1280 x 720 and at 1920 x 1080, the crop the stage
uploads, the occupancy grid given).  Per case, in one process on the same tensors, the tool first checks that vvl_sources gives vvp_sources'
src and r0 bit for bit and that depth = 1 gives live == src, then times

  vvp_sources              the nearest usable frame (the reference of the ratio)
  vvl_sources depth=D      the same walk that also keeps the candidates and writes the live sources, for each D of --depths (1,4,8), reach 8

Each call is warmed up once, then --rounds (9) rounds time every call once, in turn (events around the call on the launch stream), so the calls
share whatever else the box is doing; the median, the spread (min .. max) and the ratio of the medians are printed.  No speed is asserted.

  python tools/bench_plategrain.py [--frames 32,256] [--rounds 9] [--depths 1,4,8] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_platefill import SIZES, make_clip  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="32,256")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--depths", default="1,4,8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from videovanish_amd import hip, mask_hip, plate_hip, platefill, plategrain, plategrain_hip
    if not torch.cuda.is_available():
        raise SystemExit("bench_plategrain.py measures on the GPU: no HIP device visible")
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

    cfg, reach = platefill.PlateFillConfig(), plategrain.PlateGrainConfig().reach
    depths = [int(x) for x in args.depths.split(",")]
    dev = torch.device("cuda:0")
    emit(f"# bench_plategrain: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds after one warm-up, median (min .. max) ms; {cfg}, reach {reach}")
    for T in [int(x) for x in args.frames.split(",")]:
        for H, W in SIZES:
            frames, raw = make_clip(T, H, W)
            dil = torch.cat([hip.mask_collapse_dilate(torch.from_numpy(raw[a:a + 32]).to(dev).contiguous(), 8) for a in range(0, T, 32)])
            del raw
            y0, x0, y1, x1 = platefill.crop_box(hip.mask_bbox(dil).cpu().numpy(), H, W)
            d = dil[:, y0:y1, x0:x1].contiguous()
            f = torch.from_numpy(np.stack([fr[y0:y1, x0:x1] for fr in frames])).to(dev)
            occ = hip.mask_tile_union(d, plate_hip.TILE)
            ns = mask_hip.time_bridge_grow(d, 0, cfg.guard)[0]
            st, n, s1 = plate_hip.stats(f, ns, occ, cfg.min_samples, cfg.tol)
            near = lambda: plate_hip.sources(f, d, ns, occ, st, n, s1, cfg.tol, cfg.outlier, cfg.max_gap)
            rot = lambda depth: plategrain_hip.sources(f, d, ns, occ, st, n, s1, cfg.tol, cfg.outlier, cfg.max_gap, depth, reach)
            src, r0 = near()
            rotated = {}
            for depth in sorted(set(depths + [1])):
                s2, live, r2 = rot(depth)
                if not ((s2 == src).all().item() and (r2 == r0).all().item()):
                    raise SystemExit("bench_plategrain.py: vvl_sources changed src or r0")
                if depth == 1 and not (live == src).all().item():
                    raise SystemExit("bench_plategrain.py: depth = 1 does not give live == src")
                rotated[depth] = int(((live != src) & (src != -1)).sum().item())
            sourced = int((src != -1).sum().item())
            calls = [("vvp_sources", near)] + [(f"vvl_sources depth={depth}", (lambda depth=depth: rot(depth))) for depth in depths]
            for _, fn in calls:
                event_ms(fn)                                                                   # warm-up
            ms = {name: [] for name, _ in calls}
            for _ in range(args.rounds):
                for name, fn in calls:
                    ms[name].append(event_ms(fn))
            emit(f"# {W}x{H}, {T} frames: crop {x1 - x0}x{y1 - y0} ({f.numel() / 2 ** 20:.0f} MiB); {sourced} masked pixels have a source; src and r0 equal "
                 f"vvp_sources', depth = 1 gives live == src; rotated: " + ", ".join(f"depth {k}: {v}" for k, v in rotated.items()))
            base = statistics.median(ms["vvp_sources"])
            for name, _ in calls:
                v = ms[name]
                med = statistics.median(v)
                records.append({"frame": f"{W}x{H}", "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med, 4),
                                "ratio": round(med / base, 3)})
                emit(f"{W}x{H} T={T:3d} {name:24s} {med:8.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med / base:5.2f} x vvp_sources")
            flush()
            del frames, dil, d, f, ns, occ, st, n, s1, src, r0, s2, live, r2
            torch.cuda.empty_cache()
    js = json.dumps({"bench_plategrain": records, "rounds": args.rounds})
    print(js)
    lines.append(js)
    flush()


if __name__ == "__main__":
    main()
