"""Overlay masking, measured on one MI355X: its kernels one by one on the same inputs, a device-to-device copy as the box's own streaming rate,
and the stage with its transfers.

--frames (32,256) resident frames at 1280 x 720 and at 1920 x 1080: a smooth textured background that pans 3 px a frame under grain of +-4
levels, and a 160 x 64 logo (an 8-px checker of 40 / 230 at alpha 0.4) fixed on the screen; the masks are all zero.  Per case, in one process
on the same tensors:

  accumulate               vvo_accumulate: the whole clip in one call (rule 1)
  copy (same bytes)        a device-to-device copy of T * H * W * 4 bytes: what the box streams when nothing is computed
  classify                 vvo_classify (rule 2)
  close dilate             vv_mask_collapse_dilate, `close` iterations (rule 4)
  label ~C / label F       vvm_label_components (rules 5 and 6)
  stats ~C / stats F       vvo_component_stats
  select holes / select    vvo_select
  fill merge               vvo_merge with T = 1: C | holes
  fringe dilate            vv_mask_collapse_dilate, `grow` iterations (rule 7)
  merge                    vvo_merge: the union over the clip and the counts

Each call is warmed up once, then --rounds (9) rounds time every call once, in turn (events around the call on the launch stream), so the
calls share whatever else the box is doing; the median and the spread (min .. max) are printed.  For vvo_accumulate the bytes it has to read
(T * H * W * 4: three image bytes and one mask byte a pixel and frame) over its median, and the same figure for the copy, which reads those
bytes and writes them too.  Then the stage itself (infill.overlay_mask on the host frames), wall clock, best of three: the whole call, and
its upload (the frames stacked and copied) measured on its own.  No speed is asserted.

  python tools/bench_overlaymask.py [--frames 32,256] [--rounds 9] [--out FILE]
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
LOGO = (64, 160)


def make_clip(T, H, W, seed=7, speed=3, alpha=0.4):
    """(frames: list of T [H,W,3] u8, the logo's pixels [H,W] bool)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W + speed * T].astype(np.float32)
    wide = 128.0 + 50.0 * (np.sin(xx / 9.0 + yy / 23.0) + np.sin(yy / 7.0 - xx / 31.0)) + 25.0 * np.sin(xx / 3.0) * np.sin(yy / 4.0)
    logo = np.zeros((H, W), bool)
    ly, lx = H // 10, W - W // 10 - LOGO[1]
    logo[ly:ly + LOGO[0], lx:lx + LOGO[1]] = True
    cy, cx = np.mgrid[:H, :W]
    checker = np.where(((cy // 8) + (cx // 8)) % 2 == 0, 40.0, 230.0).astype(np.float32)
    frames = []
    for t in range(T):
        v = wide[:, speed * t:speed * t + W].copy()
        v[logo] = (1.0 - alpha) * v[logo] + alpha * checker[logo]
        f = np.rint(v).astype(np.int16)[..., None] + rng.integers(-4, 5, (H, W, 3), dtype=np.int16)
        frames.append(np.clip(f, 0, 255).astype(np.uint8))
    return frames, logo


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="32,256")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from videovanish_amd import hip, infill, mask_hip, overlaymask, overlaymask_bind as B
    if not torch.cuda.is_available():
        raise SystemExit("bench_overlaymask.py measures on the GPU: no HIP device visible")
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

    cfg = overlaymask.OverlayMaskConfig()
    dev = torch.device("cuda:0")
    emit(f"# bench_overlaymask: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds after one warm-up, median (min .. max) ms; {cfg}")
    for T in [int(x) for x in args.frames.split(",")]:
        for H, W in SIZES:
            frames, logo = make_clip(T, H, W)
            f = torch.from_numpy(np.stack(frames)).to(dev)
            dil = torch.zeros((T, H, W), dtype=torch.uint8, device=dev)
            acc = B.accumulate(f, dil, B.new_acc(H, W, dev))
            edge, counts = B.classify(acc, cfg.min_samples, cfg.mag, cfg.coh)
            strong, edges = counts.cpu().numpy().tolist()
            closed = hip.mask_collapse_dilate(edge[None, ..., None], cfg.close)
            inv = (closed == 0).to(torch.uint8)
            lab5 = mask_hip.label_components(inv)[0]
            st5 = B.component_stats(lab5)
            holes = B.select(lab5, st5, 0, cfg.max_hole, True)[0]
            filled = B.merge(closed, holes)[0]
            lab6 = mask_hip.label_components(filled)[0]
            st6 = B.component_stats(lab6)
            kept, boxes, nboxes = B.select(lab6, st6, cfg.min_area, cfg.max_area_px(H, W), True)
            o = hip.mask_collapse_dilate(kept[None, ..., None], cfg.grow)[0]
            d2, added = B.merge(dil, o)
            missed = int((torch.from_numpy(logo).to(dev) & (o == 0)).sum().item())
            nbytes = T * H * W * 4
            src = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            scratch = B.new_acc(H, W, dev)
            calls = [("accumulate", lambda: B.accumulate(f, dil, scratch)),
                     ("copy (same bytes)", lambda: dst.copy_(src)),
                     ("classify", lambda: B.classify(acc, cfg.min_samples, cfg.mag, cfg.coh)),
                     ("close dilate", lambda: hip.mask_collapse_dilate(edge[None, ..., None], cfg.close)),
                     ("label ~C", lambda: mask_hip.label_components(inv)),
                     ("stats ~C", lambda: B.component_stats(lab5)),
                     ("select holes", lambda: B.select(lab5, st5, 0, cfg.max_hole, True)),
                     ("fill merge", lambda: B.merge(closed, holes)),
                     ("label F", lambda: mask_hip.label_components(filled)),
                     ("stats F", lambda: B.component_stats(lab6)),
                     ("select", lambda: B.select(lab6, st6, cfg.min_area, cfg.max_area_px(H, W), True)),
                     ("fringe dilate", lambda: hip.mask_collapse_dilate(kept[None, ..., None], cfg.grow)),
                     ("merge", lambda: B.merge(dil, o))]
            for _, fn in calls:
                event_ms(fn)                                                                   # warm-up
            ms = {name: [] for name, _ in calls}
            for _ in range(args.rounds):
                for name, fn in calls:
                    ms[name].append(event_ms(fn))
            emit(f"# {W}x{H}, {T} frames ({f.numel() / 2 ** 20:.0f} MiB): {edges} of {strong} strong px persistent, {int(nboxes.item())} overlays, "
                 f"{int((o != 0).sum().item())} px in the overlay, {missed} of {int(logo.sum())} logo px missed, {int(added.sum().item())} px added")
            for name, _ in calls:
                v = ms[name]
                med = statistics.median(v)
                rec = {"frame": f"{W}x{H}", "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med, 4)}
                more = ""
                if name in ("accumulate", "copy (same bytes)"):
                    rec.update(bytes=nbytes, tb_per_s=round(nbytes / med / 1e9, 3))
                    more = f"  {nbytes / 2 ** 20:.0f} MiB read{' and written' if name != 'accumulate' else ''}, {nbytes / med / 1e9:.2f} TB/s"
                records.append(rec)
                emit(f"{W}x{H} T={T:3d} {name:24s} {med:8.3f} ({min(v):.3f} .. {max(v):.3f}) ms{more}")
            up, _ = wall_ms(lambda: torch.from_numpy(np.stack(frames)).to(dev))
            total, (_, rep) = wall_ms(lambda: infill.overlay_mask(frames, dil, cfg))
            records.append({"frame": f"{W}x{H}", "frames": T, "call": "stage", "upload_ms": round(up, 2), "total_ms": round(total, 2)})
            emit(f"{W}x{H} T={T:3d} stage (wall, best of 3): upload {up:.1f} ms, whole call {total:.1f} ms ({rep.verdict}, {rep.found} overlays, "
                 f"{int(rep.added.sum())} px added)")
            flush()
            del frames, f, dil, acc, edge, closed, inv, lab5, st5, holes, filled, lab6, st6, kept, boxes, o, d2, added, src, dst, scratch
            torch.cuda.empty_cache()
    js = json.dumps({"bench_overlaymask": records, "rounds": args.rounds})
    print(js)
    lines.append(js)
    flush()


if __name__ == "__main__":
    main()
