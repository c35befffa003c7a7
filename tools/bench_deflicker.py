"""Inpaint deflicker, measured on one MI355X: vvf_hold in its two forms and vvf_window_pixels.

Resident clips of --frames (32,256) frames at 1280 x 720 and 1920 x 1080, the full frame as the window: one background with +-3 levels of
per-pixel noise per frame (every neighbour passes the gate: the most arithmetic the rule can ask for), a 400 x 300 mask box.  Per shape, in one
process on the same tensors:

  hold fixed, radius r     the streaming form, r in 0, 1, 2, 4.  radius 0 launches the same kernel and is a pure read-once, write-once copy of
                           the clip with the sums: the floor every other radius is reported against
  hold gather, radius 2    the one-thread-per-pixel form at the arguments of "hold fixed, radius 2" (the C entry with the "fixed" flag off),
                           reported against it
  window_pixels            the materialised resize of model frames at three quarters of the size (the resize of max_img_size)

Each call is warmed up once, then --rounds (9) rounds time every call once, in turn (events around the call on the launch stream), so the
calls share whatever else the box is doing; the median and the spread (min .. max) are printed, and the bytes the rule has to move (the clip
read once, written once, the mask read once) over the median.  No speed is asserted.  One line per measurement, then one JSON line with
everything; --out also writes them to a file.

  python tools/bench_deflicker.py [--frames 32,256] [--rounds 9] [--sizes 720,1080] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = {"720": (720, 1280), "1080": (1080, 1920)}
RADII = (0, 1, 2, 4)
TOL = 12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="32,256")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="720,1080")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from videovanish_amd import flicker_hip
    if not torch.cuda.is_available():
        raise SystemExit("bench_deflicker.py measures on the GPU: no HIP device visible")
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

    emit(f"# bench_deflicker: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds after one warm-up, median (min .. max) ms; tol {TOL}")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for size in args.sizes.split(","):
        H, W = SIZES[size]
        for T in (int(t) for t in args.frames.split(",")):
            base = torch.randint(40, 216, (H, W, 3), device="cuda", generator=gen, dtype=torch.int16)
            win = torch.empty((T, H, W, 3), dtype=torch.uint8, device="cuda")
            for t in range(T):
                win[t] = (base + torch.randint(-3, 4, (H, W, 3), device="cuda", generator=gen, dtype=torch.int16)).to(torch.uint8)
            mask = torch.zeros((T, H, W), dtype=torch.uint8, device="cuda")
            mask[:, H // 2 - 150:H // 2 + 150, W // 2 - 200:W // 2 + 200] = 255
            offs = torch.zeros((T, 2), dtype=torch.int32, device="cuda")
            out = torch.empty_like(win)
            Hm, Wm = H * 3 // 4 // 8 * 8, W * 3 // 4 // 8 * 8
            patch = win[:, :Hm, :Wm].contiguous()
            calls = [(f"hold fixed, radius {r}", (lambda r=r: flicker_hip.hold(win, offs, mask, r, TOL, fixed=True, out=out))) for r in RADII]
            calls.append(("hold gather, radius 2", lambda: flicker_hip.hold(win, offs, mask, 2, TOL, fixed=False, out=out)))
            calls.append((f"window_pixels {Wm}x{Hm} -> {W}x{H}", lambda: flicker_hip.window_pixels(patch, H, W)))
            a, sa = flicker_hip.hold(win, offs, mask, 2, TOL, fixed=True)
            b, sb = flicker_hip.hold(win, offs, mask, 2, TOL, fixed=False)
            same = bool((a == b).all().item() and (sa == sb).all().item())
            accepted = float(sa[:, 2].sum().item()) / (T * H * W)
            del a, b
            for _, fn in calls:
                event_ms(fn)                                                                       # warm-up
            ms = {name: [] for name, _ in calls}
            for _ in range(args.rounds):
                for name, fn in calls:
                    ms[name].append(event_ms(fn))
            moved = T * H * W * 7
            emit(f"# {W}x{H}, {T} frames ({win.numel() / 2 ** 20:.0f} MiB of pixels); mean accepted samples at radius 2: {accepted:.2f}; both forms give the same "
                 f"bytes: {same}")
            med = {name: statistics.median(v) for name, v in ms.items()}
            for name, _ in calls:
                v = ms[name]
                rec = {"frame": f"{W}x{H}", "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med[name], 4),
                       "ms_per_frame": round(med[name] / T, 5)}
                tail = ""
                if name.startswith("hold"):
                    against = "hold fixed, radius 2" if "gather" in name else "hold fixed, radius 0"
                    rec.update(gb_per_s=round(moved / med[name] / 1e6, 1), against=against, ratio=round(med[name] / med[against], 3))
                    tail = f"  {rec['gb_per_s']:7.1f} GB/s  {rec['ratio']:.2f} x {against}"
                records.append(rec)
                emit(f"{W}x{H} T={T:3d} {name:38s} {med[name]:8.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med[name] / T:.4f} ms/frame{tail}")
            del win, mask, offs, out, patch, base
            torch.cuda.empty_cache()
    js = json.dumps({"bench_deflicker": records, "rounds": args.rounds, "tol": TOL})
    print(js)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + js + "\n")


if __name__ == "__main__":
    main()
