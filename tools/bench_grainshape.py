"""Grain shape, measured on one MI355X: each of its two kernels beside the grain matching kernel it stands next to, on the same inputs.

Two cases, the original a smooth picture with binomial grain of sigma 4 (a bank of 8 noise frames, repeated) and the same picture without grain
as the model's frames (so the flat test passes and every ring pixel is worked on), a mask box that drifts 2 px per frame, dilated 8 times:
  "720p"  32 resident frames at 1280 x 720, the full frame as the window, the model's frames at three quarters of the size
  "1080p" 256 resident frames at 1920 x 1080, one static 512 x 512 window round the box, the model's frames at the window's size
Per case, in one process on the same tensors:

  grain ring_grain_stats              vvg_ring_grain_stats, ring 12, flat 24, the identity table (the parent's kernel: the yardstick)
  shape ring_shape_stats              vvn_ring_shape_stats, the same arguments
  grain paste_grain_composite, luma / rgb       vvg_paste_grain_composite, feather 3, amplitude 64 (the yardstick)
  shape paste_shaped_composite, taps 0 / 128, luma / rgb     vvn_paste_shaped_composite, no field, the same arguments (its check of the taps on
                                                             the host, one synchronisation, is inside the host clock only)
  finish, grain / grain + shape       infill.finish on the host's frames with grain matching alone and with the option: the whole stage's share
                                      of a call is the difference (host clock; --finish-rounds, 3)

Each call is warmed up once, then --rounds (9) rounds time every call once, in turn (events around the call on the launch stream), so the calls
share whatever else the box is doing; the median and the spread (min .. max) are printed, with the nominal bytes (the frame read, the mask read,
the frame written, the model's frames read; for the statistics the window's pixels of the model, the original and the mask) over the median.
No speed is asserted.  One line per measurement, then one JSON line with everything; --out also writes them to a file.

  python tools/bench_grainshape.py [--cases 720p,1080p] [--rounds 9] [--finish-rounds 3] [--out FILE]
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

CASES = {"720p": (32, 720, 1280, "full"), "1080p": (256, 1080, 1920, "512")}
BANK = 8


def picture(h, w):
    """[h,w,3] float64 in 40 .. 215: a few low-frequency waves, the same picture at every size."""
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    yy, xx = yy / h, xx / w
    return 127.5 + 43.0 * np.stack([np.sin(5 * xx + 3 * yy + c) + np.sin(7 * yy - 2 * xx + 2 * c) for c in range(3)], axis=-1)


def make_case(T, H, W, window, rng):
    """(patch [T,..], orig [T,H,W,3], raw masks [T,H,W,1], offsets, h, w) as numpy arrays."""
    from scipy import ndimage
    clean = picture(H, W)
    bank = []
    for _ in range(BANK):
        g = rng.normal(0.0, 4.0 / 1.5, clean.shape)                                # [1/2, 1, 1/2] on both axes: r0 = 1.5 each
        g = ndimage.correlate1d(ndimage.correlate1d(g, [0.5, 1.0, 0.5], axis=0, mode="wrap"), [0.5, 1.0, 0.5], axis=1, mode="wrap")
        bank.append(np.clip(np.rint(clean + g), 0, 255).astype(np.uint8))
    orig = np.stack([bank[t % BANK] for t in range(T)])
    raw = np.zeros((T, H, W, 1), np.uint8)
    bh, bw = (300, 400) if window == "full" else (200, 240)
    y0, x0 = H // 2 - bh // 2, W // 2 - bw // 2 - 32
    for t in range(T):
        d = 2 * (t % 32)
        raw[t, y0:y0 + bh, x0 + d:x0 + d + bw] = 255
    if window == "full":
        h, w, offs = H, W, np.zeros((T, 2), np.int32)
        small = np.rint(picture(H * 3 // 4 // 8 * 8, W * 3 // 4 // 8 * 8)).astype(np.uint8)
    else:
        h = w = 512
        offs = np.tile(np.array([[H // 2 - 256, W // 2 - 256]], np.int32), (T, 1))
        small = np.rint(clean[offs[0, 0]:offs[0, 0] + h, offs[0, 1]:offs[0, 1] + w]).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(small, (T,) + small.shape)), orig, raw, offs, h, w


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="720p,1080p")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--finish-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from videovanish_amd import grain_hip, grainmatch, grainshape, grainshape_bind, hip, infill
    from videovanish_amd.roi import RoiPlan
    if not torch.cuda.is_available():
        raise SystemExit("bench_grainshape.py measures on the GPU: no HIP device visible")
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

    gcfg, ncfg = grainmatch.GrainMatchConfig(), grainshape.GrainShapeConfig()
    emit(f"# bench_grainshape: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds after one warm-up, median (min .. max) ms")
    for case in args.cases.split(","):
        T, H, W, window = CASES[case]
        patch, orig, raw, offs, h, w = make_case(T, H, W, window, np.random.default_rng(7))
        dp, do, df = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (patch, orig, offs))
        dm = hip.mask_collapse_dilate(torch.from_numpy(raw).cuda().contiguous(), 8)
        out = torch.empty_like(do)
        ident = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8), (T, 3, 256)))).cuda()
        amp = torch.full((T, 3, 256), 64, dtype=torch.uint8, device="cuda")
        ids = torch.arange(T, dtype=torch.int32, device="cuda")
        taps = {a: torch.full((T, 3, 2), a, dtype=torch.int32, device="cuda") for a in (0, 128)}
        stat_bytes = T * h * w * (3 + 3 + 1)
        paste_bytes = T * H * W * (3 + 1 + 3) + patch.size
        calls = [("grain ring_grain_stats", stat_bytes, lambda: grain_hip.ring_grain_stats(dp, do, dm, df, ident, h, w, gcfg.ring, gcfg.flat)),
                 ("shape ring_shape_stats", stat_bytes, lambda: grainshape_bind.ring_shape_stats(dp, do, dm, df, ident, h, w, gcfg.ring, gcfg.flat))]
        for mode, name in enumerate(("luma", "rgb")):
            calls.append((f"grain paste_grain_composite, {name}", paste_bytes,
                          lambda mode=mode: grain_hip.paste_grain_composite(dp, do, dm, df, ident, amp, ids, 0, mode, h, w, 3.0, out=out)))
            for a in (0, 128):
                calls.append((f"shape paste_shaped_composite, taps {a}, {name}", paste_bytes,
                              lambda mode=mode, a=a: grainshape_bind.paste_shaped_composite(dp, do, dm, df, ident, None, 0, amp, taps[a], ids, 0, mode, h, w,
                                                                                            3.0, out=out)))
        s = grainshape_bind.ring_shape_stats(dp, do, dm, df, ident, h, w, gcfg.ring, gcfg.flat).cpu().numpy()
        g = grain_hip.ring_grain_stats(dp, do, dm, df, ident, h, w, gcfg.ring, gcfg.flat).cpu().numpy()
        fitted = grainshape.fit(s, g, gcfg, ncfg)
        for _, _, fn in calls:
            event_ms(fn)                                                                   # warm-up
        ms = {name: [] for name, _, _ in calls}
        for _ in range(args.rounds):
            for name, _, fn in calls:
                ms[name].append(event_ms(fn))
        emit(f"# case {case}: {T} frames of {W}x{H}, window {w}x{h}, model frames {patch.shape[2]}x{patch.shape[1]}; pairs per frame, channel and axis "
             f"{int(fitted.pairs.sum()) // (6 * T)}; fitted a {float(fitted.a.min()):.3f} .. {float(fitted.a.max()):.3f} (true: 0.5), sigma_pixel "
             f"{float(fitted.sigma_pixel.min()):.2f} .. {float(fitted.sigma_pixel.max()):.2f} (true: 4)")
        for name, nbytes, _ in calls:
            v = ms[name]
            med = statistics.median(v)
            records.append({"case": case, "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "ms_per_frame": round(med / T, 5),
                            "nominal_bytes": nbytes, "nominal_GBps": round(nbytes / med / 1e6, 1)})
            emit(f"{case:5s} {name:48s} {med:8.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med / T:.4f} ms/frame  {nbytes / med / 1e6:8.1f} GB/s nominal")
        del dp, do, out
        # the whole stage inside a finish call, from the host's frames and back
        frames, model = list(orig), list(patch)
        plans = [] if window == "full" else [RoiPlan("static", (h, w), offs, offs.astype(np.float64))]
        fin = {"finish, grain": dict(grain=gcfg), "finish, grain + shape": dict(grain=gcfg, grain_shape=ncfg)}
        fms = {name: [] for name in fin}
        for r in range(args.finish_rounds + 1):
            for name, kw in fin.items():
                t = host_ms(lambda: infill.finish([list(model)], frames, dm, plans, 3, True, torch.device("cuda"), **kw))
                if r:
                    fms[name].append(t)
        for name, v in fms.items():
            med = statistics.median(v)
            records.append({"case": case, "frames": T, "call": name, "ms": [round(x, 3) for x in v], "median_ms": round(med, 3), "ms_per_frame": round(med / T, 4)})
            emit(f"{case:5s} {name:48s} {med:8.1f} ({min(v):.1f} .. {max(v):.1f}) ms  {med / T:.3f} ms/frame")
        a, b = (statistics.median(fms[k]) for k in fin)
        emit(f"{case:5s} the option's share of the finish call: {(b - a) / b * 100:.1f} % ({b - a:.1f} ms of {b:.1f} ms)")
        del dm, frames, model
    js = json.dumps({"bench_grainshape": records, "rounds": args.rounds})
    print(js)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + js + "\n")


if __name__ == "__main__":
    main()
