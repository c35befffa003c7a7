"""Mask-region inference, measured: the drop-in call diffuerase.run_infill_on_frames with roi=None / "static" / "follow" / "static-regions" /
"follow-regions" on one MI355X,
full-width SD-1.5 / SD-VAE shapes with seeded random-init weights (the drop-in's own models; build time not counted).

Clips (T frames each):
  a  bench.py's synthetic clip (synth_frame: an H/4 x W/4 box moving 2 px per frame) at 1280 x 720
  b  a fixed 160 x 90 "logo" box near the top-right corner of a 1920 x 1080 clip
  c  clip b's logo and a second 160 x 90 logo near the bottom-left corner (two separate regions)
Regimes:
  gui  the GUI's call: every default of run_infill_on_frames (dilation 8, 2-step TCD, RAFT prior computed, max_img_size 960)
  s50  50 DDIM steps (--steps), max_img_size = the frame's long side, prior supplied (bench.py's synthetic prior)
Every (regime, clip, mode) is warmed up once (s50: with 2 steps) and then timed --repeats times, host clock around the whole call (it returns
host frames, so the device is idle at both ends).  One line per timed run, then one JSON line with everything; --out also writes them to a file.

  python tools/bench_roi.py [--frames 16] [--steps 50] [--repeats 2] [--regimes gui,s50] [--clips a,b,c] [--modes none,static,follow,...] [--out FILE]
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

CLIPS = {"a": (720, 1280), "b": (1080, 1920), "c": (1080, 1920)}


def make_clip(name, T):
    from bench import synth_frame
    H, W = CLIPS[name]
    frames, masks, priors = [], [], []
    for t in range(T):
        f, m, p = synth_frame(t, H, W)
        if name in ("b", "c"):
            m = np.zeros((H, W), np.uint8)
            m[40:130, W - 220: W - 60] = 255                     # 160 x 90 logo
            if name == "c":
                m[H - 130:H - 40, 60:220] = 255                  # and one in the opposite corner
            p = f.copy()
            p[m > 0] = f.reshape(-1, 3).mean(0).astype(np.uint8)
        frames.append(f)
        masks.append(np.repeat(m[..., None], 3, axis=2))         # the GUI hands over 3-channel mask frames
        priors.append(p)
    return frames, masks, priors


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--regimes", default="gui,s50")
    ap.add_argument("--clips", default="a,b")
    ap.add_argument("--modes", default="none,static,follow")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import diffuerase
    from videovanish_amd import hip, infill, roi
    from videovanish_amd.config import RunConfig
    from videovanish_amd.pipeline import model_size
    if not torch.cuda.is_available():
        raise SystemExit("bench_roi.py measures on the GPU: no HIP device visible")
    diffuerase.configure(RunConfig())
    lines, records = [], []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# bench_roi: {torch.cuda.get_device_name(0)}, {args.frames} frames per clip, full-width synthetic weights, fp16")
    for regime in args.regimes.split(","):
        for clip in args.clips.split(","):
            frames, masks, priors = make_clip(clip, args.frames)
            H, W = CLIPS[clip]
            if regime == "gui":
                kw, warm_kw = {}, {}
            else:
                kw = dict(propainer_frames=priors, max_img_size=max(H, W), num_inference_steps=args.steps, scheduler="ddim")
                warm_kw = dict(kw, num_inference_steps=2)
            for mode in args.modes.split(","):
                r = None if mode == "none" else mode
                # the plan the call makes: the same dilation + bbox kernels and planner, on the side
                dil = hip.mask_collapse_dilate(torch.from_numpy(np.stack(masks)).cuda().contiguous(), 8)
                cfg = roi.as_config(r)
                if cfg is None:
                    plans = None
                elif cfg.max_regions > 1:
                    plans = infill.region_plans(dil, H, W, 3, cfg)
                else:
                    plans = roi.plan_roi(hip.mask_bbox(dil).cpu().numpy(), H, W, 3, cfg)
                    plans = None if plans is None else [plans]
                sizes = [p.size for p in plans] if plans is not None else [(H, W)]
                msizes = [model_size(h, w, kw.get("max_img_size", 960)) for h, w in sizes]
                win_s = "+".join(f"{w}x{h}" for h, w in sizes)
                model_s = "+".join(f"{mw}x{mh}" for mh, mw in msizes)
                frac = round(sum(h * w for h, w in sizes) / (H * W), 3)
                diffuerase.run_infill_on_frames(frames, masks, roi=r or "off", **warm_kw)
                secs = []
                for _ in range(args.repeats):
                    torch.cuda.synchronize()
                    t0 = time.time()
                    out = diffuerase.run_infill_on_frames(frames, masks, roi=r or "off", **kw)
                    torch.cuda.synchronize()
                    secs.append(time.time() - t0)
                    assert len(out) == args.frames and out[0].shape == (H, W, 3)
                best = min(secs)
                rec = {"regime": regime, "clip": clip, "frame": f"{W}x{H}", "roi": mode, "window": win_s, "model": model_s,
                       "window_px_frac": frac, "seconds": [round(s, 3) for s in secs], "frames_per_s": round(args.frames / best, 3),
                       "offsets_first_last": [p.offsets[[0, -1]].tolist() for p in plans] if plans is not None else None}
                records.append(rec)
                emit(f"{regime:4s} clip {clip} {W}x{H}  roi={mode:14s} window {win_s} (model {model_s}, {frac:.3f} of the frame)  "
                     f"seconds {' '.join(f'{s:.3f}' for s in secs)}  frames/s {rec['frames_per_s']:.3f}")
    diffuerase.configure()
    js = json.dumps({"bench_roi": records, "frames": args.frames, "steps_s50": args.steps, "repeats": args.repeats})
    print(js)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + js + "\n")


if __name__ == "__main__":
    main()
