"""Seam detail matching, measured on one MI355X: vvd_ring_detail_stats and vvd_sharpen, and beside them vvg_ring_grain_stats, the sibling in tiling.

Resident clips of --frames (32) frames at 1280 x 720 and 1920 x 1080, the full frame as the window: one textured background (random bytes:
every ring pixel passes `edge`, the most arithmetic the rule can ask for) as the original, its copy with +-3 levels of noise as the model's
frame, a 400 x 300 mask box, ring 8.  Per shape, in one process on the same tensors:

  ring_detail_stats          the statistic at the window's size, and with the model at three quarters of the size (the resize of max_img_size)
  ring_grain_stats           vv_grain.hip's statistic on the same window, ring and tile, with flat = 255 (every ring pixel counts too)
  sharpen, amount a          a = 300 on every frame, and a = 0 (the block-uniform copy: the floor the filter is reported against); at the
                             window's size and from three quarters of it

Each call is warmed up once, then --rounds (9) rounds time every call once, in turn (events around the call on the launch stream), so the
calls share whatever else the box is doing; the median and the spread (min .. max) are printed, and the bytes the step has to move over the
median: the statistics read the mask once and, in the tiles that hold a counted pixel, the model's frame and the original (reported against
the whole window, 7 bytes a pixel: an upper bound of what they move); the apply reads the model's frame once and writes the window once.  No
speed is asserted.  One line per measurement, then one JSON line with everything; --out also writes them to a file.

  python tools/bench_detailmatch.py [--frames 32] [--rounds 9] [--sizes 720,1080] [--out FILE]
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
RING, EDGE, OVERSHOOT = 8, 12, 4


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="32")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="720,1080")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from videovanish_amd import detailmatch_bind, grain_hip
    if not torch.cuda.is_available():
        raise SystemExit("bench_detailmatch.py measures on the GPU: no HIP device visible")
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

    emit(f"# bench_detailmatch: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds after one warm-up, median (min .. max) ms; "
         f"ring {RING}, edge {EDGE}, overshoot {OVERSHOOT}")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for size in args.sizes.split(","):
        H, W = SIZES[size]
        for T in (int(t) for t in args.frames.split(",")):
            orig = torch.randint(40, 216, (T, H, W, 3), device="cuda", generator=gen, dtype=torch.int16)
            model = (orig + torch.randint(-3, 4, (T, H, W, 3), device="cuda", generator=gen, dtype=torch.int16)).to(torch.uint8)
            orig = orig.to(torch.uint8)
            mask = torch.zeros((T, H, W), dtype=torch.uint8, device="cuda")
            mask[:, H // 2 - 150:H // 2 + 150, W // 2 - 200:W // 2 + 200] = 255
            offs = torch.zeros((T, 2), dtype=torch.int32, device="cuda")
            ident = torch.arange(256, dtype=torch.uint8, device="cuda").repeat(T, 3, 1).contiguous()
            out = torch.empty_like(model)
            Hm, Wm = H * 3 // 4 // 8 * 8, W * 3 // 4 // 8 * 8
            small = model[:, :Hm, :Wm].contiguous()
            on, off = torch.full((T,), 300, dtype=torch.int32, device="cuda"), torch.zeros((T,), dtype=torch.int32, device="cuda")
            calls = [("ring_detail_stats", lambda: detailmatch_bind.ring_detail_stats(model, orig, mask, offs, H, W, RING, EDGE)),
                     (f"ring_detail_stats {Wm}x{Hm} -> {W}x{H}", lambda: detailmatch_bind.ring_detail_stats(small, orig, mask, offs, H, W, RING, EDGE)),
                     ("ring_grain_stats", lambda: grain_hip.ring_grain_stats(model, orig, mask, offs, ident, H, W, RING, 255)),
                     ("sharpen, amount 0", lambda: detailmatch_bind.sharpen(model, off, H, W, OVERSHOOT, out=out)),
                     ("sharpen, amount 300", lambda: detailmatch_bind.sharpen(model, on, H, W, OVERSHOOT, out=out)),
                     (f"sharpen, amount 0, {Wm}x{Hm} -> {W}x{H}", lambda: detailmatch_bind.sharpen(small, off, H, W, OVERSHOOT, out=out)),
                     (f"sharpen, amount 300, {Wm}x{Hm} -> {W}x{H}", lambda: detailmatch_bind.sharpen(small, on, H, W, OVERSHOOT, out=out))]
            counted = int(detailmatch_bind.ring_detail_stats(model, orig, mask, offs, H, W, RING, EDGE)[:, 0].sum().item())
            for _, fn in calls:
                event_ms(fn)                                                                       # warm-up
            ms = {name: [] for name, _ in calls}
            for _ in range(args.rounds):
                for name, fn in calls:
                    ms[name].append(event_ms(fn))
            emit(f"# {W}x{H}, {T} frames ({model.numel() / 2 ** 20:.0f} MiB of pixels); counted ring pixels of channel 0: {counted}")
            med = {name: statistics.median(v) for name, v in ms.items()}
            for name, _ in calls:
                v = ms[name]
                src = small if "->" in name else model
                moved = T * H * W * 7 if name.startswith("ring") else src.numel() + out.numel()
                rec = {"frame": f"{W}x{H}", "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med[name], 4),
                       "ms_per_frame": round(med[name] / T, 5), "bytes": moved, "gb_per_s": round(moved / med[name] / 1e6, 1)}
                records.append(rec)
                emit(f"{W}x{H} T={T:3d} {name:44s} {med[name]:8.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med[name] / T:.4f} ms/frame  {rec['gb_per_s']:7.1f} GB/s")
            del orig, model, mask, offs, out, small, ident
            torch.cuda.empty_cache()
    js = json.dumps({"bench_detailmatch": records, "rounds": args.rounds, "ring": RING, "edge": EDGE})
    print(js)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + js + "\n")


if __name__ == "__main__":
    main()
