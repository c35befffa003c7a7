"""Mask clean-up, measured on one MI355X: (a) its two kernels alone, (b) what it gives back to the planners of roi= and spans= on noisy masks.

(a) --kernel-frames (64) resident 1920 x 1080 frames, two mask sets: "speckled" = one 400 x 300 blob and 200 stray pixels per frame, the blob
    missing in every 8th frame; "filled" = every pixel set (what mask_dilation_iter=0 hands over: one frame-filling component, the longest
    union-find chains).  Per set, events around each call, one warm-up and 5 timed calls, in the same process on the same masks:
    hip.mask_collapse_dilate with 8 iterations, mask_hip.despeckle (label + weigh + clear, in slabs of mask_hip.slab_frames frames),
    mask_hip.time_bridge_grow (bridge 2, grow 0 and grow 1), and a device-to-device copy of the dilated masks; GB/s are bytes the call must move
    at least (dilate: raw in, masks out; despeckle: masks in and out, raw in; time: masks in and out; copy: in and out) beside the 6.29 TB/s
    float4 copy of DESIGN.md section 5.
(b) the drop-in call, full-width SD-1.5 / SD-VAE shapes with seeded random-init weights, regimes as in tools/bench_roi.py ("gui": every default
    of run_infill_on_frames; "s50": 50 DDIM steps, prior supplied, max_img_size = the long side), each configuration warmed up once and timed
    --repeats times, host clock around the whole call:
      roi    tools/bench_roi.py's clip b (16 frames 1920 x 1080, a 160 x 90 logo) with roi="static": as drawn; with one stray pixel in one
             frame in the opposite corner; the same with mask_clean="on"
      spans  tools/bench_spans.py's clip (96 frames 1280 x 720, the object in 24 consecutive frames) with spans="masked": as drawn; with one stray
             pixel in each of frames 3, 70, 90; the same with mask_clean="on"
    The expectation to confirm or refute: with the clean-up the noisy clips get the plans, and so the times, of the clips as drawn.
No speed is asserted.  One line per measurement, then one JSON line with everything; --out also writes them to a file.

  python tools/bench_maskclean.py [--kernel-frames 64] [--repeats 2] [--regimes gui] [--parts kernels,roi,spans] [--steps 50] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

COPY_TBPS = 6.29
H, W = 1080, 1920


def kernel_masks(kind, T):
    """Raw masks [T,H,W,3] u8 (the GUI hands over 3-channel mask frames)."""
    if kind == "filled":
        return np.full((T, H, W, 3), 255, np.uint8)
    rng = np.random.default_rng(12)
    m = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        if t % 8 != 5:
            m[t, 300:600, 700 + 2 * t:1100 + 2 * t] = 255
        m[t, rng.integers(0, H, 200), rng.integers(0, W, 200)] = 255
    return np.repeat(m[..., None], 3, axis=3)


def stray(masks, frames, y, x):
    out = [m.copy() for m in masks]
    for t in frames:
        out[t][y, x] = 255
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel-frames", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--regimes", default="gui")
    ap.add_argument("--parts", default="kernels,roi,spans")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import diffuerase
    from videovanish_amd import hip, infill, mask_hip, roi, spans
    from videovanish_amd.config import RunConfig
    if not torch.cuda.is_available():
        raise SystemExit("bench_maskclean.py measures on the GPU: no HIP device visible")
    lines, records = [], {"kernels": [], "calls": []}
    parts = args.parts.split(",")

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, n=5):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    def plan_of(frames, masks, opt):
        """The plan the call makes: the same dilation, clean-up and planners, on the side."""
        raw = torch.from_numpy(np.stack(masks)).cuda().contiguous()
        dil = hip.mask_collapse_dilate(raw, 8)
        if "mask_clean" in opt:
            dil = infill.clean_masks(raw, dil, diffuerase.maskclean.as_config(opt["mask_clean"]), None)[0]
        if "spans" in opt:
            return str(infill.span_plan(frames, dil, spans.as_config(opt["spans"])))
        h, w = frames[0].shape[:2]
        plan = roi.plan_roi(hip.mask_bbox(dil).cpu().numpy(), h, w, 3, roi.as_config(opt["roi"]))
        return "full frame" if plan is None else f"window {plan.size[1]}x{plan.size[0]}"

    emit(f"# bench_maskclean: {torch.cuda.get_device_name(0)}")
    if "kernels" in parts:
        S = args.kernel_frames
        area = diffuerase.maskclean.MaskCleanConfig().area_for(H, W)
        emit(f"# kernels: {S} resident frames {W}x{H}, 3-channel raw masks, min_area {area}, despeckle slabs of {mask_hip.slab_frames(H, W)} frames")
        for kind in ("speckled", "filled"):
            raw = torch.from_numpy(kernel_masks(kind, S)).cuda().contiguous()
            dil = hip.mask_collapse_dilate(raw, 8)
            px = S * H * W
            clean, counts = mask_hip.despeckle(dil, raw, area)
            _, tc = mask_hip.time_bridge_grow(clean, 2, 1)
            tc = tc.sum(0).tolist()
            changed = counts.sum(0).tolist() + tc
            dst = torch.empty_like(dil)
            for name, fn, nbytes in (("mask_collapse_dilate, 8 iterations", lambda: hip.mask_collapse_dilate(raw, 8), 4 * px),
                                     ("despeckle", lambda: mask_hip.despeckle(dil, raw, area), 5 * px),
                                     ("time_bridge_grow bridge 2 grow 0", lambda: mask_hip.time_bridge_grow(clean, 2, 0), 2 * px),
                                     ("time_bridge_grow bridge 2 grow 1", lambda: mask_hip.time_bridge_grow(clean, 2, 1), 2 * px),
                                     ("device copy of the dilated masks", lambda: dst.copy_(dil), 2 * px)):
                ms = timed(fn)
                best = min(ms)
                rec = {"masks": kind, "call": name, "frames": S, "ms": [round(x, 4) for x in ms], "ms_per_frame": round(best / S, 5),
                       "min_bytes": nbytes, "GBps": round(nbytes / best / 1e6, 1), "share_of_copy": round(nbytes / best / 1e6 / (COPY_TBPS * 1e3), 3)}
                records["kernels"].append(rec)
                emit(f"{kind:8s} {name:36s} ms {' '.join(f'{x:.3f}' for x in ms)}  {rec['GBps']:.0f} GB/s of the bytes it must move "
                     f"({100 * rec['share_of_copy']:.1f} % of {COPY_TBPS} TB/s)")
            emit(f"{kind:8s} changed: {changed[0]} components / {changed[1]} px cleared, {changed[2]} px bridged, {changed[3]} px grown (bridge 2, grow 1)")
            records["kernels"].append({"masks": kind, "components_removed": changed[0], "px_cleared": changed[1], "px_bridged": changed[2], "px_grown": changed[3]})
            del raw, dil, clean, dst

    if "roi" in parts or "spans" in parts:
        diffuerase.configure(RunConfig())
        cases = []
        if "roi" in parts:
            import bench_roi
            frames, masks, priors = bench_roi.make_clip("b", 16)
            noisy = stray(masks, [7], 1000, 60)
            cases += [("roi", "as drawn", frames, masks, priors, dict(roi="static")), ("roi", "1 stray px", frames, noisy, priors, dict(roi="static")),
                      ("roi", "1 stray px", frames, noisy, priors, dict(roi="static", mask_clean="on"))]
        if "spans" in parts:
            import bench_spans
            frames, masks, priors = bench_spans.make_clip(96, 24)
            noisy = stray(masks, [3, 70, 90], 700, 20)
            cases += [("spans", "as drawn", frames, masks, priors, dict(spans="masked")), ("spans", "3 stray px", frames, noisy, priors, dict(spans="masked")),
                      ("spans", "3 stray px", frames, noisy, priors, dict(spans="masked", mask_clean="on"))]
        for regime in args.regimes.split(","):
            for part, what, frames, masks, priors, opt in cases:
                h, w = frames[0].shape[:2]
                if regime == "gui":
                    kw, warm_kw = {}, {}
                else:
                    kw = dict(propainer_frames=priors, max_img_size=max(h, w), num_inference_steps=args.steps, scheduler="ddim")
                    warm_kw = dict(kw, num_inference_steps=2)
                plan = plan_of(frames, masks, opt)
                diffuerase.run_infill_on_frames(frames, masks, **opt, **warm_kw)
                secs = []
                for _ in range(args.repeats):
                    torch.cuda.synchronize()
                    t0 = time.time()
                    out = diffuerase.run_infill_on_frames(frames, masks, **opt, **kw)
                    torch.cuda.synchronize()
                    secs.append(time.time() - t0)
                    assert len(out) == len(frames)
                untouched = sum(o is f for o, f in zip(out, frames))
                r = diffuerase.last_mask_clean
                rep = None if r is None else {"components_removed": int(r.removed.sum()), "px_cleared": int(r.cleared.sum()), "px_bridged": int(r.bridged.sum())}
                rec = {"regime": regime, "part": part, "masks": what, "frame": f"{w}x{h}", "frames": len(frames), "options": opt, "plan": plan,
                       "seconds": [round(s, 3) for s in secs], "frames_returned_untouched": untouched, "mask_clean": rep}
                records["calls"].append(rec)
                emit(f"{regime:4s} {part:5s} {len(frames)} frames {w}x{h}  masks {what:10s} {' '.join(f'{k}={v}' for k, v in opt.items()):32s} "
                     f"plan {plan}  seconds {' '.join(f'{s:.3f}' for s in secs)}  untouched frames {untouched}  clean-up {rep}")
        diffuerase.configure()
    js = json.dumps({"bench_maskclean": records, "repeats": args.repeats, "steps_s50": args.steps})
    print(js)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + js + "\n")


if __name__ == "__main__":
    main()
