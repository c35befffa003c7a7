"""Clean-plate alignment, measured on one MI355X: the tracker's kernels, the canvas kernels, and the whole stage beside the unaligned one.

--frames (32,256) frames at 1280 x 720 and at 1920 x 1080: a pan of 2 px per frame (and a tilt of one pixel up or down every eighth frame)
over a wide still with a fixed fine texture, grain of +-2 levels per frame, a box of 1/8 of the frame's width and 5/18 of its height that
crosses the frame against the pan during the clip; the masks are the box, dilated 8 times.  Per case, in one process on the same tensors:

  pyramid                    vva_pyramid of all T frames (resident), levels 0 .. L
  sad, level L / level 0     vva_sad of one frame pair at the coarsest level (radius from the settings) and at level 0 (radius 1)
  pick                       vva_pick of one level
  track                      vva_track of the segment: every launch of T - 1 frames enqueued at once (their number is printed)
  place_masks / unplace_mask the canvas kernels on the segment's canvas box

Each call is warmed up once, then --rounds (9) rounds time every call once, in turn (events around the call on the launch stream), so the
calls share whatever else the box is doing; the median and the spread (min .. max) are printed.  Then the stage itself on the host frames,
wall clock, best of three: infill.plate_fill with the alignment and without it on the same clip (without it the pan lets it fill nothing:
that is the stage of the parent commit), and the tracker's part of the aligned call (upload in batches, pyramid, track, read-back).  The tool
checks that the tracker recovered the clip's true offsets.  No speed is asserted.

  python tools/bench_platealign.py [--frames 32,256] [--rounds 9] [--out FILE]
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

SIZES = ((720, 1280), (1080, 1920))


def make_clip(T, H, W, seed=7):
    """(frames: list of T [H,W,3] u8, raw masks [T,H,W,1] u8, off [T,2] = the true (x, y) of every frame)."""
    rng = np.random.default_rng(seed)
    off = np.stack([2 * np.arange(T), np.cumsum((np.arange(T) % 8 == 7) * np.where((np.arange(T) // 8) % 2, -1, 1))], axis=1)
    my = int(max(-off[:, 1].min(), 0))
    Hw, Ww = H + my + int(off[:, 1].max()), W + int(off[:, 0].max())
    yy, xx = np.mgrid[:Hw, :Ww].astype(np.float32)
    wide = np.stack([127.5 + 40.0 * (np.sin(9 * xx / W + 3 * yy / H + c) + np.sin(7 * yy / H - 4 * xx / W + 2 * c)) / 2 for c in range(3)], axis=-1)
    wide = np.rint(wide).astype(np.int16) + rng.integers(-20, 21, (Hw, Ww, 1), dtype=np.int16)
    bw, bh = W // 8, H * 5 // 18
    y0 = H // 2 - bh // 2
    raw = np.zeros((T, H, W, 1), np.uint8)
    frames = []
    for t in range(T):
        ox, oy = int(off[t, 0]), my + int(off[t, 1])
        f = np.clip(wide[oy:oy + H, ox:ox + W] + rng.integers(-2, 3, (H, W, 3), dtype=np.int16), 0, 255).astype(np.uint8)
        x0 = W - (t * (W + bw)) // max(T - 1, 1)
        a, b = max(x0, 0), max(min(x0 + bw, W), 0)
        raw[t, y0:y0 + bh, a:b] = 255
        f[y0:y0 + bh, a:b] = 240
        frames.append(f)
    return frames, raw, off


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="32,256")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from videovanish_amd import align_hip, hip, infill, platealign, platefill
    if not torch.cuda.is_available():
        raise SystemExit("bench_platealign.py measures on the GPU: no HIP device visible")
    lines, records = [], []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def wall_ms(fn, n=3):
        best = None
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        return best, r

    pcfg, acfg = platefill.PlateFillConfig(), platealign.PlateAlignConfig()
    dev = torch.device("cuda:0")
    emit(f"# bench_platealign: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds after one warm-up, median (min .. max) ms; {acfg}; {pcfg}")
    for T in [int(x) for x in args.frames.split(",")]:
        for H, W in SIZES:
            frames, raw, off = make_clip(T, H, W)
            dil = torch.cat([hip.mask_collapse_dilate(torch.from_numpy(raw[a:a + 32]).to(dev).contiguous(), 8) for a in range(0, T, 32)])
            del raw
            L = platealign.coarsest_level(H, W, acfg.levels)
            f = torch.from_numpy(np.stack(frames)).to(dev)
            pyr = align_hip.pyramid(f, dil, L)
            track_t = align_hip.track(pyr, H, W, L, acfg.radius, acfg.min_overlap, acfg.max_residual)
            track = track_t.cpu().numpy()
            if not ((track[:, :2] == off).all() and (track[:, 3] == 1).all()):
                raise SystemExit("bench_platealign.py: the tracker did not recover the clip's offsets")
            box = platealign.canvas_box(hip.mask_bbox(dil).cpu().numpy(), track[:, :2], track[:, 3] == 1)
            dil_c, inv_c = align_hip.place_masks(dil, track_t, box)
            step = np.zeros((T, 8), np.int32)
            step[:, 3] = 1
            coarse, fine = step.copy(), step.copy()
            coarse[1] = [0, 0, 0, align_hip.IN_PROGRESS, 0, 0, 0, L]
            fine[1] = [off[1, 0], off[1, 1], 0, align_hip.IN_PROGRESS, 0, 0, 0, 0]
            coarse_t, fine_t = torch.from_numpy(coarse).to(dev), torch.from_numpy(fine).to(dev)
            acc = align_hip.sad(pyr, fine_t, H, W, L, 1, 0, 1)
            done = torch.from_numpy(step).to(dev)                                              # finished records: vva_pick reads acc and the record, writes nothing
            calls = [("pyramid", lambda: align_hip.pyramid(f, dil, L, out=pyr)),
                     (f"sad, level {L} r={acfg.radius}", lambda: align_hip.sad(pyr, coarse_t, H, W, L, 1, L, acfg.radius)),
                     ("sad, level 0 r=1", lambda: align_hip.sad(pyr, fine_t, H, W, L, 1, 0, 1)),
                     ("pick (and the copy of the record)", lambda: align_hip.pick(acc, fine_t.clone(), H, W, L, 1, 0, 1, acfg.min_overlap, acfg.max_residual)),
                     ("pick, nothing to do", lambda: align_hip.pick(acc, done, H, W, L, 1, 0, 1, acfg.min_overlap, acfg.max_residual)),
                     ("track", lambda: align_hip.track(pyr, H, W, L, acfg.radius, acfg.min_overlap, acfg.max_residual)),
                     ("place_masks", lambda: align_hip.place_masks(dil, track_t, box)),
                     ("unplace_mask", lambda: align_hip.unplace_mask(dil_c, dil, track_t, box))]
            for _, fn in calls:
                event_ms(fn)                                                                   # warm-up
            ms = {name: [] for name, _ in calls}
            for _ in range(args.rounds):
                for name, fn in calls:
                    ms[name].append(event_ms(fn))
            launches = align_hip.track_launches(T, L)
            emit(f"# {W}x{H}, {T} frames: L = {L}, pyramid {pyr.numel() / 2 ** 20:.0f} MiB, canvas {box[3] - box[1]}x{box[2] - box[0]} "
                 f"({platealign.canvas_bytes(T, box) / 2 ** 20:.0f} MiB), pan {int(off[:, 0].max())} px, track = {launches} launches and memsets; offsets recovered: True")
            for name, _ in calls:
                v = ms[name]
                med = statistics.median(v)
                records.append({"frame": f"{W}x{H}", "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med, 4),
                                "ms_per_frame": round(med / T, 5)})
                emit(f"{W}x{H} T={T:3d} {name:24s} {med:8.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med / T:.4f} ms/frame")
            del f, pyr, dil_c, inv_c
            torch.cuda.empty_cache()
            trk, _ = wall_ms(lambda: infill._track_segment(frames, dil, acfg, pcfg.max_bytes))
            got = []
            aligned, (_, _, rep) = wall_ms(lambda: infill.plate_fill(frames, dil, pcfg, None, acfg=acfg, align_out=got))
            plain, (_, _, rep0) = wall_ms(lambda: infill.plate_fill(frames, dil, pcfg, None))
            track_ms = statistics.median(ms["track"])
            records.append({"frame": f"{W}x{H}", "frames": T, "call": "stage", "aligned_ms": round(aligned, 2), "unaligned_ms": round(plain, 2),
                            "tracker_ms": round(trk, 2), "track_launches": launches, "track_share": round(track_ms / aligned, 4), "path": got[-1].path[0]})
            emit(f"{W}x{H} T={T:3d} stage (wall, best of 3): with plate_align {aligned:.1f} ms ({got[-1].path[0]}; {int(rep.filled.sum())} px filled, "
                 f"{int(rep.left.sum())} px left), of which upload + pyramid + track + read-back {trk:.1f} ms and vva_track alone {track_ms:.2f} ms "
                 f"({100 * track_ms / aligned:.1f} % of the stage, {launches} launches); without it {plain:.1f} ms ({int(rep0.filled.sum())} px filled, "
                 f"{int(rep0.left.sum())} px left)")
            flush()
            del frames, dil
            torch.cuda.empty_cache()
    js = json.dumps({"bench_platealign": records, "rounds": args.rounds})
    print(js)
    lines.append(js)
    flush()


if __name__ == "__main__":
    main()
