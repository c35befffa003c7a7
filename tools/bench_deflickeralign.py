"""Aligned inpaint deflicker, measured on one MI355X: vvc_hold against vvf_hold's gather form, and the tracker's time per clip call.

Resident clips of --frames (32,256) frames at 1280 x 720 and 1920 x 1080, the full frame as the window: one iid background panned 3 px per frame
with +-3 levels of per-pixel noise per frame (along the track every neighbour passes the gate: the most arithmetic the rule can ask for), a
400 x 300 mask box.  Per shape, in one process on the same tensors, radius 2:

  vvf_hold gather          the unaligned one-thread-per-pixel form (the C entry with the "fixed" flag off): the reference
  vvc_hold, 3 px/frame     the same arguments plus the clip's track, reported against the reference
  vvc_hold, zero track     the same arguments plus an all-zero, all-tracked track: the reference's own reads, through the other instantiation

Before anything is timed the zero-track call is held against the reference byte for byte (out and sums); a difference ends the run.  Each call
is warmed up once, then --rounds (9) rounds time every call once, in turn (events around the call on the launch stream), so the calls share
whatever else the box is doing; the median and the spread (min .. max) are printed.  Then the tracker as a clip call pays for it
(infill._track_segment: upload in batches, pyramid, vva_track, the read-back; wall time, best of 3) against the filter's median.  No speed is
asserted.  One line per measurement, then one JSON line with everything; --out also writes them to a file.

  python tools/bench_deflickeralign.py [--frames 32,256] [--rounds 9] [--sizes 720,1080] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = {"720": (720, 1280), "1080": (1080, 1920)}
RADIUS, TOL, STEP = 2, 12, 3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="32,256")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="720,1080")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from videovanish_amd import deflickeralign, flickalign_hip, flicker_hip, infill, platealign
    if not torch.cuda.is_available():
        raise SystemExit("bench_deflickeralign.py measures on the GPU: no HIP device visible")
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

    acfg = platealign.PlateAlignConfig()
    emit(f"# bench_deflickeralign: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds after one warm-up, median (min .. max) ms; "
         f"radius {RADIUS}, tol {TOL}, a pan of {STEP} px per frame; tracker: {acfg}")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for size in args.sizes.split(","):
        H, W = SIZES[size]
        for T in (int(t) for t in args.frames.split(",")):
            wide = torch.randint(40, 216, (H, W + STEP * (T - 1), 3), device="cuda", generator=gen, dtype=torch.int16)
            win = torch.empty((T, H, W, 3), dtype=torch.uint8, device="cuda")
            for t in range(T):
                win[t] = (wide[:, STEP * t:STEP * t + W] + torch.randint(-3, 4, (H, W, 3), device="cuda", generator=gen, dtype=torch.int16)).to(torch.uint8)
            del wide
            mask = torch.zeros((T, H, W), dtype=torch.uint8, device="cuda")
            mask[:, H // 2 - 150:H // 2 + 150, W // 2 - 200:W // 2 + 200] = 255
            offs = torch.zeros((T, 2), dtype=torch.int32, device="cuda")
            pan = deflickeralign.identity_track(T)
            pan[:, 0] = STEP * np.arange(T)
            pan_t, zero_t = torch.from_numpy(pan).to("cuda"), torch.from_numpy(deflickeralign.identity_track(T)).to("cuda")
            out = torch.empty_like(win)
            a, sa = flicker_hip.hold(win, offs, mask, RADIUS, TOL, fixed=False)
            b, sb = flickalign_hip.hold(win, offs, zero_t, mask, RADIUS, TOL)
            if not ((a == b).all().item() and (sa == sb).all().item()):
                raise SystemExit("bench_deflickeralign.py: vvc_hold under a zero track does not give vvf_hold's bytes")
            _, sp = flickalign_hip.hold(win, offs, pan_t, mask, RADIUS, TOL)
            accepted = {"fixed place": float(sa[:, 2].sum().item()) / (T * H * W), "along the track": float(sp[:, 2].sum().item()) / (T * H * W)}
            del a, b
            ref = "vvf_hold gather"
            calls = [(ref, lambda: flicker_hip.hold(win, offs, mask, RADIUS, TOL, fixed=False, out=out)),
                     (f"vvc_hold, {STEP} px/frame track", lambda: flickalign_hip.hold(win, offs, pan_t, mask, RADIUS, TOL, out=out)),
                     ("vvc_hold, zero track", lambda: flickalign_hip.hold(win, offs, zero_t, mask, RADIUS, TOL, out=out))]
            for _, fn in calls:
                event_ms(fn)                                                                       # warm-up
            ms = {name: [] for name, _ in calls}
            for _ in range(args.rounds):
                for name, fn in calls:
                    ms[name].append(event_ms(fn))
            emit(f"# {W}x{H}, {T} frames ({win.numel() / 2 ** 20:.0f} MiB of pixels); mean accepted samples at a fixed place {accepted['fixed place']:.2f}, "
                 f"along the track {accepted['along the track']:.2f}; the zero track gives vvf_hold's bytes: True")
            med = {name: statistics.median(v) for name, v in ms.items()}
            for name, _ in calls:
                v = ms[name]
                rec = {"frame": f"{W}x{H}", "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med[name], 4),
                       "ms_per_frame": round(med[name] / T, 5), "against": ref, "ratio": round(med[name] / med[ref], 3)}
                records.append(rec)
                emit(f"{W}x{H} T={T:3d} {name:30s} {med[name]:8.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med[name] / T:.4f} ms/frame  {rec['ratio']:.2f} x {ref}")
            # the tracker, as a clip call pays for it: host frames in, the track on the device and on the host out
            frames = list(win.cpu().numpy())
            del out
            torch.cuda.empty_cache()
            best, track = None, None
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, track = infill._track_segment(frames, mask, acfg, deflickeralign.TRACK_BYTES)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                best = dt if best is None else min(best, dt)
            recovered = bool((track[:, :2] == pan[:, :2]).all() and (track[:, 3] == 1).all())
            filt = med[f"vvc_hold, {STEP} px/frame track"]
            records.append({"frame": f"{W}x{H}", "frames": T, "call": "tracker per clip call", "wall_ms": round(best, 2), "ms_per_frame": round(best / T, 4),
                            "filter_ms": round(filt, 4), "ratio_to_filter": round(best / filt, 1), "offsets_recovered": recovered})
            emit(f"{W}x{H} T={T:3d} tracker per clip call (wall, best of 3; upload + pyramid + track + read-back) {best:8.1f} ms  {best / T:.3f} ms/frame  "
                 f"{best / filt:.0f} x the filter; offsets recovered: {recovered}")
            del win, mask, offs, frames
            torch.cuda.empty_cache()
    js = json.dumps({"bench_deflickeralign": records, "rounds": args.rounds, "radius": RADIUS, "tol": TOL, "step": STEP})
    print(js)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + js + "\n")


if __name__ == "__main__":
    main()
