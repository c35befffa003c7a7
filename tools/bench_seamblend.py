"""Seam membrane blending, measured on one MI355X: its kernels beside the tone / grain kernels they extend, on the same inputs, and the blocked
relax beside the single sweeps it replaces.

--frames (32) resident frames at 1280 x 720 and at 1920 x 1080, a smooth picture with grain of sigma 4 as the original and the same picture
without grain plus a tone error that varies across the frame as the model's frames, a mask box of 5/24 of the frame's width that drifts 2 px
per frame, dilated 8 times, and two window shapes: "full" = the full frame as the window (0, 0, H, W), the model's frames at three quarters of
the size (the resize of max_img_size), and "512" = one static 512 x 512 window round the box, the model's frames at the window's size.  Per
case, in one process on the same tensors:

  tone ring_stats                 vvt_ring_stats, ring 12 (the counterpart)
  blend ring_diff                 vvb_ring_diff, ring 12, presmooth 2 (classes, boundary values, sums)
  blend relax level 0, 1 x 8      vvb_relax on level 0, sweeps 8, one launch (the tile and a halo of 8 in LDS)
  blend relax level 0, 8 x 1      the same eight sweeps as eight launches of sweeps 1 (the same bytes; each streams the level through memory)
  blend solve                     vvb_solve: ring_diff, every pull, every level's relax
  grain paste_grain_composite     vvg_paste_grain_composite, feather 3, amplitude 64 (the counterpart)
  blend paste_blend_composite     vvb_paste_blend_composite, the same with the field

Each call is warmed up once, then --rounds (9) rounds time every call once, in turn (events around the call on the launch stream), so the
calls share whatever else the box is doing; the median and the spread (min .. max) are printed.  No speed is asserted.  One line per
measurement, then one JSON line with everything; --out also writes them to a file.

  python tools/bench_seamblend.py [--frames 32] [--rounds 9] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = ((720, 1280), (1080, 1920))


def picture(h, w, T):
    """[T,h,w,3] float64 in 40 .. 215: a few low-frequency waves, the same picture at every size."""
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    yy, xx = yy / h, xx / w
    base = np.stack([np.sin(5 * xx + 3 * yy + c) + np.sin(7 * yy - 2 * xx + 2 * c) for c in range(3)], axis=-1)
    return np.broadcast_to(127.5 + 43.0 * base, (T, h, w, 3))


def tone_error(h, w):
    """[h,w,3]: a ramp and a vignette of up to about 12 levels."""
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    u, v = yy / h - 0.5, xx / w - 0.5
    return np.stack([12 * u + 8 * v - 20 * (u * u + v * v), -10 * u + 14 * v, 6 * u - 16 * v + 16 * (u * u + v * v)], axis=-1)


def make_case(T, H, W, window, rng):
    """(patch, orig, raw masks [T,H,W,1], offsets, h, w) as numpy arrays."""
    clean = picture(H, W, T)
    orig = np.stack([np.clip(np.rint(clean[t] + rng.normal(0.0, 4.0, clean[t].shape)), 0, 255).astype(np.uint8) for t in range(T)])
    raw = np.zeros((T, H, W, 1), np.uint8)
    bw, bh = W * 5 // 24, H * 5 // 18
    y0, x0 = H // 2 - bh // 2, W // 2 - bw // 2 - T
    for t in range(T):
        raw[t, y0:y0 + bh, x0 + 2 * t:x0 + 2 * t + bw] = 255
    if window == "full":
        h, w, offs = H, W, np.zeros((T, 2), np.int32)
        hm, wm = H * 3 // 4 // 8 * 8, W * 3 // 4 // 8 * 8
        patch = np.clip(np.rint(picture(hm, wm, T) - tone_error(hm, wm)), 0, 255).astype(np.uint8)
    else:
        h = w = 512
        offs = np.tile(np.array([[H // 2 - 256, W // 2 - 256]], np.int32), (T, 1))
        oy, ox = offs[0]
        patch = np.clip(np.rint(clean[:, oy:oy + h, ox:ox + w] - tone_error(H, W)[oy:oy + h, ox:ox + w]), 0, 255).astype(np.uint8)
    return patch, orig, raw, offs, h, w


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from videovanish_amd import blend_hip, grain_hip, hip, seamblend, tone_hip
    if not torch.cuda.is_available():
        raise SystemExit("bench_seamblend.py measures on the GPU: no HIP device visible")
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

    T = args.frames
    cfg = seamblend.SeamBlendConfig()
    emit(f"# bench_seamblend: {torch.cuda.get_device_name(0)}, {T} frames, {args.rounds} interleaved rounds after one warm-up, median (min .. max) ms")
    for H, W in SIZES:
        for window in ("full", "512"):
            patch, orig, raw, offs, h, w = make_case(T, H, W, window, np.random.default_rng(7))
            dp, do, df = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (patch, orig, offs))
            dm = hip.mask_collapse_dilate(torch.from_numpy(raw).cuda().contiguous(), 8)
            out = torch.empty_like(do)
            ident = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8), (T, 3, 256)))).cuda()
            amp = torch.full((T, 3, 256), 64, dtype=torch.uint8, device="cuda")
            ids = torch.arange(T, dtype=torch.int32, device="cuda")
            scratch = torch.empty((seamblend.scratch_bytes(T, h, w),), dtype=torch.uint8, device="cuda")
            cls, val, _ = blend_hip.ring_diff(dp, do, dm, df, ident, h, w, cfg.ring, cfg.presmooth, cfg.max_shift)
            parent = blend_hip.pull(cls, val)[1]
            a, b = torch.empty_like(val), torch.empty_like(val)

            def single_sweeps():
                blend_hip.relax(cls, val, 1, parent=parent, out=a)
                src, dst = a, b
                for _ in range(cfg.sweeps - 1):
                    blend_hip.relax(cls, src, 1, start=False, out=dst)
                    src, dst = dst, src
                return src

            one = blend_hip.relax(cls, val, cfg.sweeps, parent=parent)
            same = bool((one == single_sweeps()).all().item())
            solve = lambda: blend_hip.solve(dp, do, dm, df, ident, h, w, cfg.ring, cfg.presmooth, cfg.sweeps, cfg.max_shift, scratch=scratch)
            field, _, sums = solve()
            fit = seamblend.fit(sums.cpu().numpy())
            field = field.clone()
            calls = [("tone ring_stats", lambda: tone_hip.ring_stats(dp, do, dm, df, h, w, cfg.ring)),
                     ("blend ring_diff", lambda: blend_hip.ring_diff(dp, do, dm, df, ident, h, w, cfg.ring, cfg.presmooth, cfg.max_shift)),
                     (f"blend relax level 0, 1 x {cfg.sweeps}", lambda: blend_hip.relax(cls, val, cfg.sweeps, parent=parent, out=a)),
                     (f"blend relax level 0, {cfg.sweeps} x 1", single_sweeps),
                     ("blend solve", solve),
                     ("grain paste_grain_composite", lambda: grain_hip.paste_grain_composite(dp, do, dm, df, ident, amp, ids, 0, 0, h, w, 3.0, out=out)),
                     ("blend paste_blend_composite",
                      lambda: blend_hip.paste_blend_composite(dp, do, dm, df, ident, field, cfg.strength_q8, amp, ids, 0, 0, h, w, 3.0, out=out))]
            for _, fn in calls:
                event_ms(fn)                                                                   # warm-up
            ms = {name: [] for name, _ in calls}
            for _ in range(args.rounds):
                for name, fn in calls:
                    ms[name].append(event_ms(fn))
            emit(f"# {W}x{H}, window {window} ({w}x{h}, model frames {patch.shape[2]}x{patch.shape[1]}); ring pixels per frame {int(fit.n.mean())}, hole "
                 f"pixels per frame {int(fit.n_hole.mean())}; largest |m| {float(fit.max_shift.max()):.2f}; scratch {scratch.numel() / 2 ** 20:.1f} MiB; "
                 f"blocked relax equals the single sweeps: {same}")
            for name, _ in calls:
                v = ms[name]
                med = statistics.median(v)
                records.append({"frame": f"{W}x{H}", "window": window, "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med, 4),
                                "ms_per_frame": round(med / T, 5)})
                emit(f"{W}x{H} {window:4s} {name:34s} {med:8.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med / T:.4f} ms/frame")
            del dp, do, df, dm, out, ident, amp, ids, scratch, cls, val, parent, a, b, one, field
    js = json.dumps({"bench_seamblend": records, "rounds": args.rounds})
    print(js)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + js + "\n")


if __name__ == "__main__":
    main()
