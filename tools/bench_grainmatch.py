"""Seam grain matching, measured on one MI355X: each of its two kernels beside the tone matching kernel it extends, on the same inputs.

--frames (32) resident frames at 1920 x 1080, a smooth picture with grain of sigma 4 as the original and the same picture without grain as the
model's frames (so the flat test passes and every ring pixel is worked on), a 400 x 300 mask box that drifts 2 px per frame, dilated 8 times,
and two window shapes: "full" = the full frame as the window (0, 0, H, W), the model's frames at three quarters of the size (the resize of
max_img_size), and "512" = one static 512 x 512 window round the box, the model's frames at the window's size.  Per case, in one process on the
same tensors:

  tone ring_stats            vvt_ring_stats, ring 12 (the counterpart of the parent commit, unchanged)
  grain ring_grain_stats     vvg_ring_grain_stats, ring 12, flat 24, the identity table
  tone paste_lut_composite   vvt_paste_lut_composite, feather 3 (the counterpart)
  grain paste_grain_composite, luma / rgb    vvg_paste_grain_composite, feather 3, amplitude 64 (sigma 4)
  stage (stats + host fit + tables)          what infill.finish adds per window: ring_grain_stats, the [T,36] sums to the host,
                                             grainmatch.fit and tables, the [T,3,256] amplitudes to the device (host clock, ending in the upload)

Each call is warmed up once, then --rounds (9) rounds time every call once, in turn (events around the call on the launch stream), so the
calls share whatever else the box is doing; the median and the spread (min .. max) are printed.  No speed is asserted.  One line per
measurement, then one JSON line with everything; --out also writes them to a file.

  python tools/bench_grainmatch.py [--frames 32] [--rounds 9] [--out FILE]
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

H, W = 1080, 1920


def picture(h, w, T):
    """[T,h,w,3] float64 in 40 .. 215: a few low-frequency waves, the same picture at every size."""
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    yy, xx = yy / h, xx / w
    base = np.stack([np.sin(5 * xx + 3 * yy + c) + np.sin(7 * yy - 2 * xx + 2 * c) for c in range(3)], axis=-1)
    return np.broadcast_to(127.5 + 43.0 * base, (T, h, w, 3))


def make_case(T, window, rng):
    """(patch, orig, raw masks [T,H,W,1], offsets, h, w) as numpy arrays."""
    clean = picture(H, W, T)
    orig = np.stack([np.clip(np.rint(clean[t] + rng.normal(0.0, 4.0, clean[t].shape)), 0, 255).astype(np.uint8) for t in range(T)])
    raw = np.zeros((T, H, W, 1), np.uint8)
    y0, x0 = H // 2 - 150, W // 2 - 200 - T
    for t in range(T):
        raw[t, y0:y0 + 300, x0 + 2 * t:x0 + 2 * t + 400] = 255
    if window == "full":
        h, w, offs = H, W, np.zeros((T, 2), np.int32)
        patch = np.rint(picture(H * 3 // 4 // 8 * 8, W * 3 // 4 // 8 * 8, T)).astype(np.uint8)
    else:
        h = w = 512
        offs = np.tile(np.array([[H // 2 - 256, W // 2 - 256]], np.int32), (T, 1))
        patch = np.rint(clean[:, offs[0, 0]:offs[0, 0] + h, offs[0, 1]:offs[0, 1] + w]).astype(np.uint8)
    return patch, orig, raw, offs, h, w


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from videovanish_amd import grain_hip, grainmatch, hip, tone_hip
    if not torch.cuda.is_available():
        raise SystemExit("bench_grainmatch.py measures on the GPU: no HIP device visible")
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
    cfg = grainmatch.GrainMatchConfig()
    emit(f"# bench_grainmatch: {torch.cuda.get_device_name(0)}, {T} frames of {W}x{H}, {args.rounds} interleaved rounds after one warm-up, "
         "median (min .. max) ms")
    for window in ("full", "512"):
        patch, orig, raw, offs, h, w = make_case(T, window, np.random.default_rng(7))
        dp, do, df = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (patch, orig, offs))
        dm = hip.mask_collapse_dilate(torch.from_numpy(raw).cuda().contiguous(), 8)
        out = torch.empty_like(do)
        ident = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8), (T, 3, 256)))).cuda()
        amp = torch.full((T, 3, 256), 64, dtype=torch.uint8, device="cuda")
        ids = torch.arange(T, dtype=torch.int32, device="cuda")

        def stage():
            s = grain_hip.ring_grain_stats(dp, do, dm, df, ident, h, w, cfg.ring, cfg.flat).cpu().numpy()
            return torch.from_numpy(grainmatch.tables(grainmatch.fit(s, cfg).sigma_added)).cuda()

        calls = [("tone ring_stats", event_ms, lambda: tone_hip.ring_stats(dp, do, dm, df, h, w, cfg.ring)),
                 ("grain ring_grain_stats", event_ms, lambda: grain_hip.ring_grain_stats(dp, do, dm, df, ident, h, w, cfg.ring, cfg.flat)),
                 ("tone paste_lut_composite", event_ms, lambda: tone_hip.paste_lut_composite(dp, do, dm, df, ident, h, w, 3.0, out=out)),
                 ("grain paste_grain_composite, luma", event_ms,
                  lambda: grain_hip.paste_grain_composite(dp, do, dm, df, ident, amp, ids, 0, 0, h, w, 3.0, out=out)),
                 ("grain paste_grain_composite, rgb", event_ms,
                  lambda: grain_hip.paste_grain_composite(dp, do, dm, df, ident, amp, ids, 0, 1, h, w, 3.0, out=out)),
                 ("stage (stats + host fit + tables)", host_ms, stage)]
        s = grain_hip.ring_grain_stats(dp, do, dm, df, ident, h, w, cfg.ring, cfg.flat).cpu().numpy()
        fitted = grainmatch.fit(s, cfg)
        ring_px = int(tone_hip.ring_stats(dp, do, dm, df, h, w, cfg.ring)[:, 0].sum().item()) // T
        counted = int(fitted.n.sum()) // (3 * T)
        for _, clock, fn in calls:
            clock(fn)                                                                      # warm-up
        ms = {name: [] for name, _, _ in calls}
        for _ in range(args.rounds):
            for name, clock, fn in calls:
                ms[name].append(clock(fn))
        emit(f"# window {window} ({w}x{h}, model frames {patch.shape[2]}x{patch.shape[1]}); ring pixels per frame {ring_px}, counted per frame and "
             f"channel {counted}; fitted sigma {float(fitted.sigma_added[fitted.n > 0].min(initial=99.0)):.2f} .. {float(fitted.sigma_added.max()):.2f} (true: 4)")
        for name, _, _ in calls:
            v = ms[name]
            med = statistics.median(v)
            records.append({"frame": f"{W}x{H}", "window": window, "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med, 4),
                            "ms_per_frame": round(med / T, 5), "ring_px_per_frame": ring_px, "counted_per_frame_and_channel": counted})
            emit(f"{window:4s} {name:40s} {med:8.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med / T:.4f} ms/frame")
        del dp, do, df, dm, out, ident, amp, ids
    js = json.dumps({"bench_grainmatch": records, "rounds": args.rounds})
    print(js)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + js + "\n")


if __name__ == "__main__":
    main()
