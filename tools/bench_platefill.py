"""Clean-plate fill, measured on one MI355X: its kernels with and without tile skipping on the same inputs, and the stage's transfers.

--frames (32,256) resident frames at 1280 x 720 and at 1920 x 1080: a locked-off still with grain of +-4 levels, a box of 5/24 of the frame's
width and 5/18 of its height that crosses the frame from edge to edge during the clip, and a static 160 x 90 logo below it that no frame
reveals; the masks are box | logo, dilated 8 times.  The kernels run on what the stage uploads: the crop of the masks' union box (the box's
band and the logo, the full width).  Per case, in one process on the same tensors:

  guard time_bridge_grow          vvm_time_bridge_grow(dil, 0, guard): the sample frames
  tile_union                      vv_mask_tile_union: the occupancy grid
  stats / sources / fill, tiles   vvp_stats, vvp_sources, vvp_fill with the occupancy grid (a tile without a mask pixel reads no image byte)
  stats / sources / fill, all     the same kernels with skipping switched off (occ = NULL)
  margin dilate                   vv_mask_collapse_dilate of the unfilled remainder, `margin` iterations

The tool checks that both forms give the same frames, masks and counts.  Each call is warmed up once, then --rounds (9) rounds time every
call once, in turn (events around the call on the launch stream), so the calls share whatever else the box is doing; the median and the spread
(min .. max) are printed.  Then the stage itself (infill.plate_fill on the host frames), wall clock, best of three: the whole call, and its
upload (the crop, stacked and copied) and download (the crops of the filled frames) measured on their own.  No speed is asserted.

--e2e also runs the drop-in (random-init weights of the full architecture, 2 steps) with spans="masked", roi="follow" on a 1280 x 720 clip of
--e2e-frames (16) frames, with and without plate_fill, and records the seconds per call (the second call of each: weights loaded).

  python tools/bench_platefill.py [--frames 32,256] [--rounds 9] [--e2e] [--out FILE]
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
    still = np.stack([127.5 + 43.0 * (np.sin(5 * xx / W + 3 * yy / H + c) + np.sin(7 * yy / H - 2 * xx / W + 2 * c)) / 2 for c in range(3)], axis=-1)
    still = np.rint(still).astype(np.int16)
    bw, bh = W * 5 // 24, H * 5 // 18
    y0 = H // 2 - bh // 2
    ly, lx = min(y0 + bh + 40, H - 100), W // 2
    raw = np.zeros((T, H, W, 1), np.uint8)
    frames = []
    for t in range(T):
        f = np.clip(still + rng.integers(-4, 5, (H, W, 3), dtype=np.int16), 0, 255).astype(np.uint8)
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
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--e2e-frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from videovanish_amd import hip, infill, mask_hip, plate_hip, platefill
    if not torch.cuda.is_available():
        raise SystemExit("bench_platefill.py measures on the GPU: no HIP device visible")
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

    cfg = platefill.PlateFillConfig()
    dev = torch.device("cuda:0")
    emit(f"# bench_platefill: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds after one warm-up, median (min .. max) ms; {cfg}")
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

            def chain(o, g):
                st, n, s1 = plate_hip.stats(g, ns, o, cfg.min_samples, cfg.tol)
                src, r0 = plate_hip.sources(g, d, ns, o, st, n, s1, cfg.tol, cfg.outlier, cfg.max_gap)
                keep = hip.mask_collapse_dilate(r0[..., None], cfg.margin)
                return (st, n, s1, src, r0, keep) + tuple(plate_hip.fill(g, d, keep, o, src))

            g1, g2 = f.clone(), f.clone()
            with_t, without = chain(occ, g1), chain(None, g2)
            same = bool((g1 == g2).all().item() and (with_t[6] == without[6]).all().item() and (with_t[7] == without[7]).all().item())
            if not same:
                raise SystemExit("bench_platefill.py: tile skipping changed the result")
            counts = with_t[7].cpu().numpy()
            st, n, s1, src, r0, keep = with_t[:6]
            st2, n2, s12, src2, r02, keep2 = without[:6]
            calls = [("guard time_bridge_grow", lambda: mask_hip.time_bridge_grow(d, 0, cfg.guard)),
                     ("tile_union", lambda: hip.mask_tile_union(d, plate_hip.TILE)),
                     ("stats, tiles", lambda: plate_hip.stats(f, ns, occ, cfg.min_samples, cfg.tol)),
                     ("stats, all", lambda: plate_hip.stats(f, ns, None, cfg.min_samples, cfg.tol)),
                     ("sources, tiles", lambda: plate_hip.sources(f, d, ns, occ, st, n, s1, cfg.tol, cfg.outlier, cfg.max_gap)),
                     ("sources, all", lambda: plate_hip.sources(f, d, ns, None, st2, n2, s12, cfg.tol, cfg.outlier, cfg.max_gap)),
                     ("margin dilate", lambda: hip.mask_collapse_dilate(r0[..., None], cfg.margin)),
                     ("fill, tiles", lambda: plate_hip.fill(g1, d, keep, occ, src)),
                     ("fill, all", lambda: plate_hip.fill(g2, d, keep2, None, src2))]
            for _, fn in calls:
                event_ms(fn)                                                                   # warm-up
            ms = {name: [] for name, _ in calls}
            for _ in range(args.rounds):
                for name, fn in calls:
                    ms[name].append(event_ms(fn))
            occ_n = occ.cpu().numpy()
            emit(f"# {W}x{H}, {T} frames: crop {x1 - x0}x{y1 - y0} ({f.numel() / 2 ** 20:.0f} MiB), {int(occ_n.sum())} of {occ_n.size} tiles occupied; "
                 f"{int(counts[:, 0].sum())} px filled, {int(counts[:, 1].sum())} px left; both forms give the same bytes: {same}")
            for name, _ in calls:
                v = ms[name]
                med = statistics.median(v)
                records.append({"frame": f"{W}x{H}", "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med, 4),
                                "ms_per_frame": round(med / T, 5)})
                emit(f"{W}x{H} T={T:3d} {name:24s} {med:8.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med / T:.4f} ms/frame")
            idx = torch.from_numpy(np.nonzero(counts[:, 0])[0]).to(dev)
            up, _ = wall_ms(lambda: torch.from_numpy(np.stack([fr[y0:y1, x0:x1] for fr in frames])).to(dev))
            down, _ = wall_ms(lambda: g1[idx].cpu().numpy())
            total, (_, _, rep) = wall_ms(lambda: infill.plate_fill(frames, dil, cfg, None))
            records.append({"frame": f"{W}x{H}", "frames": T, "call": "stage", "upload_ms": round(up, 2), "download_ms": round(down, 2),
                            "total_ms": round(total, 2), "filled_frames": int(len(idx))})
            emit(f"{W}x{H} T={T:3d} stage (wall, best of 3): upload {up:.1f} ms, download of {len(idx)} filled crops {down:.1f} ms, whole call {total:.1f} ms "
                 f"({int(rep.filled.sum())} px filled, {int(rep.left.sum())} px left)")
            flush()
            del frames, dil, d, f, g1, g2, with_t, without, st, n, s1, src, r0, keep, st2, n2, s12, src2, r02, keep2, ns, occ
            torch.cuda.empty_cache()
    if args.e2e:
        import diffuerase
        H, W = SIZES[0]
        frames, raw = make_clip(args.e2e_frames, H, W)
        masks = [np.repeat(m, 3, axis=2) for m in raw]
        for label, kw in (("without plate_fill", {}), ("with plate_fill", {"plate_fill": "on"})):
            secs = []
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                diffuerase.run_infill_on_frames(frames, masks, spans="masked", roi="follow", num_inference_steps=2, **kw)
                torch.cuda.synchronize()
                secs.append(time.perf_counter() - t0)
            rep = diffuerase.last_plate_fill
            records.append({"e2e": label, "frame": f"{W}x{H}", "frames": args.e2e_frames, "seconds": [round(s, 3) for s in secs]})
            emit(f"e2e {W}x{H} T={args.e2e_frames} spans=masked roi=follow {label:20s} {secs[1]:.2f} s per call (first call, with loading: {secs[0]:.2f} s)"
                 + ("" if rep is None else f"; {int(rep.filled.sum())} px filled, {int(rep.left.sum())} px left"))
            flush()
    js = json.dumps({"bench_platefill": records, "rounds": args.rounds})
    print(js)
    lines.append(js)
    flush()


if __name__ == "__main__":
    main()
