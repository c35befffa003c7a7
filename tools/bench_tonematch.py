"""Seam tone matching, measured on one MI355X: its two kernels beside the closing step they extend.

--frames (32) resident frames at 1280 x 720 and 1920 x 1080, a 400 x 300 mask box that drifts 2 px per frame, dilated 8 times, and two window
shapes: "full" = the full frame as the window (0, 0, H, W), the model's frames at three quarters of the size (the resize of max_img_size), and
"512" = one static 512 x 512 window round the box, the model's frames at the window's size.  Per case, in one process on the same tensors:

  roi_paste_composite      the closing step without the stage (the baseline: the parent's kernel, unchanged)
  paste_lut_composite      the same step with the table look-up
  ring_stats, ring r       the statistic, r in 4, 12, 32
  stage, ring 12           what infill.finish adds per window: ring_stats, the [T,16] sums to the host, tonematch.fit and tables, the [T,3,256]
                           tables to the device (host clock around it, ending in the upload; the paste is timed above)

Each call is warmed up once, then --rounds (9) rounds time every call once, in turn (events around the call on the launch stream), so the
calls share whatever else the box is doing; the median and the spread (min .. max) are printed.  No speed is asserted.  One line per
measurement, then one JSON line with everything; --out also writes them to a file.

  python tools/bench_tonematch.py [--frames 32] [--rounds 9] [--sizes 720,1080] [--out FILE]
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

SIZES = {"720": (720, 1280), "1080": (1080, 1920)}
RINGS = (4, 12, 32)


def make_case(H, W, T, window, rng):
    """(patch, orig, raw masks [T,H,W,1], offsets, h, w) as numpy arrays."""
    orig = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    raw = np.zeros((T, H, W, 1), np.uint8)
    y0, x0 = H // 2 - 150, W // 2 - 200 - T
    for t in range(T):
        raw[t, y0:y0 + 300, x0 + 2 * t:x0 + 2 * t + 400] = 255
    if window == "full":
        h, w, offs = H, W, np.zeros((T, 2), np.int32)
        patch = rng.integers(0, 256, (T, H * 3 // 4 // 8 * 8, W * 3 // 4 // 8 * 8, 3), dtype=np.uint8)
    else:
        h = w = 512
        offs = np.tile(np.array([[H // 2 - 256, W // 2 - 256]], np.int32), (T, 1))
        patch = rng.integers(0, 256, (T, h, w, 3), dtype=np.uint8)
    return patch, orig, raw, offs, h, w


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="720,1080")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from videovanish_amd import hip, tone_hip, tonematch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tonematch.py measures on the GPU: no HIP device visible")
    lines, records = [], []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def host_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    T = args.frames
    cfg = tonematch.ToneMatchConfig()
    emit(f"# bench_tonematch: {torch.cuda.get_device_name(0)}, {T} frames, {args.rounds} interleaved rounds after one warm-up, median (min .. max) ms")
    for size in args.sizes.split(","):
        H, W = SIZES[size]
        for window in ("full", "512"):
            patch, orig, raw, offs, h, w = make_case(H, W, T, window, np.random.default_rng(7))
            dp, do, df = (torch.from_numpy(a).cuda().contiguous() for a in (patch, orig, offs))
            dm = hip.mask_collapse_dilate(torch.from_numpy(raw).cuda().contiguous(), 8)
            out = torch.empty_like(do)
            ident = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8), (T, 3, 256)))).cuda()

            def stage():
                s = tone_hip.ring_stats(dp, do, dm, df, h, w, cfg.ring).cpu().numpy()
                f = tonematch.fit(s, cfg)
                return torch.from_numpy(tonematch.tables(f.gain, f.offset)).cuda()

            calls = [("roi_paste_composite", event_ms, lambda: hip.roi_paste_composite(dp, do, dm, df, h, w, 3.0, out=out)),
                     ("paste_lut_composite", event_ms, lambda: tone_hip.paste_lut_composite(dp, do, dm, df, ident, h, w, 3.0, out=out))]
            calls += [(f"ring_stats, ring {r}", event_ms, (lambda r=r: tone_hip.ring_stats(dp, do, dm, df, h, w, r))) for r in RINGS]
            calls.append((f"stage, ring {cfg.ring} (stats + host fit + tables)", host_ms, stage))
            ring_px = {r: int(tone_hip.ring_stats(dp, do, dm, df, h, w, r)[:, 0].sum().item()) for r in RINGS}
            for _, clock, fn in calls:
                clock(fn)                                                                      # warm-up
            ms = {name: [] for name, _, _ in calls}
            for _ in range(args.rounds):
                for name, clock, fn in calls:
                    ms[name].append(clock(fn))
            emit(f"# {W}x{H}, window {window} ({w}x{h}, model frames {patch.shape[2]}x{patch.shape[1]}); ring pixels per frame: "
                 + ", ".join(f"ring {r}: {ring_px[r] // T}" for r in RINGS))
            for name, _, _ in calls:
                v = ms[name]
                med = statistics.median(v)
                records.append({"frame": f"{W}x{H}", "window": window, "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med, 4),
                                "ms_per_frame": round(med / T, 5), "ring_px_per_frame": {str(r): ring_px[r] // T for r in RINGS}})
                emit(f"{W}x{H} {window:4s} {name:50s} {med:8.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med / T:.4f} ms/frame")
            del dp, do, df, dm, out, ident
    js = json.dumps({"bench_tonematch": records, "rounds": args.rounds})
    print(js)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + js + "\n")


if __name__ == "__main__":
    main()
