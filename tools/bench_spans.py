"""Mask-span inference, measured: the drop-in call diffuerase.run_infill_on_frames with spans=None / "masked" / "masked-cuts" on one MI355X,
full-width SD-1.5 / SD-VAE shapes with seeded random-init weights (the drop-in's own models; build time not counted).

Clip: bench.py's synthetic clip (synth_frame: an H/4 x W/4 box moving 2 px per frame) at 1280 x 720, --frames frames (96), the object present only
in --object consecutive frames (24) in the middle of the clip; the other frames have an empty mask.
Regimes (tools/bench_roi.py's):
  gui  the GUI's call: every default of run_infill_on_frames (dilation 8, 2-step TCD, RAFT prior computed, max_img_size 960)
  s50  50 DDIM steps (--steps), max_img_size = the frame's long side, prior supplied (bench.py's synthetic prior)
Every (regime, mode) is warmed up once (s50: with 2 steps) and then timed --repeats times, host clock around the whole call (it returns host frames,
so the device is idle at both ends).  Mode "none" is the full-clip call, the code path of a build without spans=.  No speed-up is asserted: the
expectation to compare with is seconds proportional to the processed frames after chunk quantisation ("chunks" below: chunk_plan of every span).
Then the statistics kernel alone (vvs_frame_pair_stats on a --stat-frames slab resident on the device, events around the launch): its time and the bytes
it asks for per second (every frame is asked for twice, as the second frame of one pair and the first of the next; HBM sees about half) beside the 6.3 TB/s
achievable figure of DESIGN.md.  One line per timed run, then one JSON line with everything; --out also writes them to a file.

  python tools/bench_spans.py [--frames 96] [--object 24] [--steps 50] [--repeats 2] [--regimes gui,s50] [--modes none,masked,masked-cuts] [--out FILE]
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

H, W = 720, 1280
ACHIEVABLE_TBPS = 6.3


def make_clip(T, n_obj):
    from bench import synth_frame
    a = (T - n_obj) // 2
    frames, masks, priors = [], [], []
    for t in range(T):
        f, m, p = synth_frame(t, H, W)
        if not a <= t < a + n_obj:
            m, p = np.zeros((H, W), np.uint8), f.copy()
        frames.append(f)
        masks.append(np.repeat(m[..., None], 3, axis=2))         # the GUI hands over 3-channel mask frames
        priors.append(p)
    return frames, masks, priors


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--object", type=int, default=24)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--regimes", default="gui,s50")
    ap.add_argument("--modes", default="none,masked,masked-cuts")
    ap.add_argument("--stat-frames", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import diffuerase
    from videovanish_amd import hip, infill, spans, spans_hip
    from videovanish_amd.config import RunConfig
    from videovanish_amd.pipeline import chunk_plan
    if not torch.cuda.is_available():
        raise SystemExit("bench_spans.py measures on the GPU: no HIP device visible")
    run = RunConfig()
    diffuerase.configure(run)
    lines, records = [], []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    T = args.frames
    emit(f"# bench_spans: {torch.cuda.get_device_name(0)}, {T} frames {W}x{H}, object in {args.object} consecutive frames, full-width synthetic weights, fp16")
    frames, masks, priors = make_clip(T, args.object)
    dil = hip.mask_collapse_dilate(torch.from_numpy(np.stack(masks)).cuda().contiguous(), 8)
    for regime in args.regimes.split(","):
        if regime == "gui":
            kw, warm_kw = {}, {}
        else:
            kw = dict(propainer_frames=priors, max_img_size=max(H, W), num_inference_steps=args.steps, scheduler="ddim")
            warm_kw = dict(kw, num_inference_steps=2)
        for mode in args.modes.split(","):
            s = None if mode == "none" else mode
            cfg = spans.as_config(s)
            plan = [(0, T)] if cfg is None else infill.span_plan(frames, dil, cfg)      # the plan the call makes, on the side
            processed = sum(b - a for a, b in plan)
            chunks = [len(chunk_plan(b - a, run.chunk, run.overlap)) for a, b in plan]
            diffuerase.run_infill_on_frames(frames, masks, spans=s or "off", **warm_kw)
            secs = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t0 = time.time()
                out = diffuerase.run_infill_on_frames(frames, masks, spans=s or "off", **kw)
                torch.cuda.synchronize()
                secs.append(time.time() - t0)
                assert len(out) == T and out[0].shape == (H, W, 3)
            best = min(secs)
            rec = {"regime": regime, "spans": mode, "plan": plan, "processed_frames": processed, "chunks": chunks,
                   "seconds": [round(x, 3) for x in secs], "clip_frames_per_s": round(T / best, 3), "seconds_per_processed_frame": round(best / max(processed, 1), 4)}
            records.append(rec)
            emit(f"{regime:4s} spans={mode:12s} plan {plan} ({processed} of {T} frames, chunks {'+'.join(map(str, chunks))})  "
                 f"seconds {' '.join(f'{x:.3f}' for x in secs)}  s/processed frame {rec['seconds_per_processed_frame']:.4f}")
    # the statistics kernel alone
    S = min(args.stat_frames, T)
    f_dev = torch.from_numpy(np.stack(frames[:S])).cuda().contiguous()
    stat = {}
    for name, m_dev in (("no mask", None), ("masked", dil[:S].contiguous())):
        spans_hip.pair_stats(f_dev, m_dev)
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            spans_hip.pair_stats(f_dev, m_dev)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        nbytes = 2 * (S - 1) * H * W * (3 + (m_dev is not None))
        best = min(ms)
        stat[name] = {"frames": S, "ms": [round(x, 4) for x in ms], "bytes_asked": nbytes, "GBps_asked": round(nbytes / best / 1e6, 1),
                      "share_of_achievable": round(nbytes / best / 1e6 / (ACHIEVABLE_TBPS * 1e3), 3)}
        emit(f"frame_pair_stats {S} frames {W}x{H} ({name}): ms {' '.join(f'{x:.3f}' for x in ms)}  {stat[name]['GBps_asked']:.0f} GB/s asked for "
             f"({100 * stat[name]['share_of_achievable']:.1f} % of {ACHIEVABLE_TBPS} TB/s)")
    t0 = time.time()
    spans_hip.frame_pair_stats(frames, dil)
    torch.cuda.synchronize()
    stat["whole_clip_host_to_host_s"] = round(time.time() - t0, 3)
    emit(f"frame_pair_stats of the whole clip from host frames (upload in slabs of {spans_hip.SLAB} + kernel + download): {stat['whole_clip_host_to_host_s']:.3f} s")
    diffuerase.configure()
    js = json.dumps({"bench_spans": records, "frame_pair_stats": stat, "frames": T, "object_frames": args.object, "steps_s50": args.steps, "repeats": args.repeats})
    print(js)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + js + "\n")


if __name__ == "__main__":
    main()
