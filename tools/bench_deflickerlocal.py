"""Block-matched inpaint deflicker, measured on one MI355X: vvk_hold against vvc_hold at equal arguments, and vvk_search against its two floors.

Resident clips of --frames (32,256) frames at 1280 x 720 and 1920 x 1080, the full frame as the window: two iid planes (the upper half pans 2 px
per frame to the right, the lower half 2 px to the left) with +-3 levels of per-pixel noise per frame, a 400 x 300 mask box, radius 2.  Per
shape, in one process on the same tensors:

  vvc_hold, zero track            the existing one-thread-per-pixel kernel: the reference
  vvk_hold, zero vectors          the same arguments plus records (0, 0, 1, 0) for every block: the reference's own reads through the new kernel
  vvk_hold, searched vectors      the records of vvk_search (block 8, search 4, lam 32)
  vvk_search block B, search S    B in 8, 16; S in 2, 4, 8; lam 32

Before anything is timed vvk_hold with zero vectors is held against the reference byte for byte (out and sums); a difference ends the run.  Each
call is warmed up once, then --rounds (9) rounds time every call once, in turn (events around the call on the launch stream), so the calls
share whatever else the box is doing; the median and the spread (min .. max) are printed.  For the search the byte differences of the call
(block pixels x 3 x candidates x frame pairs; candidates that leave the window at its edges are counted too) give a rate, set against two
floors: the count over the packed SAD's peak (4 byte differences per lane and v_sad_u8, 64 lanes per clock and CU, 256 CUs at the 2400 MHz
maximum clock: 1.57e14 per second) and the time to read the clip once per temporal neighbour from HBM at the measured 6.29 TB/s.  Then the stage
(search at block 8, search 4, plus the filter) as a share of the model's 580 ms per frame.  No speed is asserted.  One line per measurement, then
one JSON line with everything; --out also writes them to a file.

  python tools/bench_deflickerlocal.py [--frames 32,256] [--rounds 9] [--sizes 720,1080] [--out FILE]
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
RADIUS, TOL, STEP, LAM = 2, 12, 2, 32
SAD_PEAK = 4 * 64 * 256 * 2.4e9         # byte differences per second: v_sad_u8 on every lane of every CU at the maximum clock
HBM_RATE = 6.29e12                      # bytes per second, measured (float4 copy)
MODEL_MS_PER_FRAME = 580.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="32,256")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="720,1080")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from videovanish_amd import deflickeralign, flickalign_hip, flicklocal_bind
    from videovanish_amd.deflickerlocal import DeflickerLocalConfig
    if not torch.cuda.is_available():
        raise SystemExit("bench_deflickerlocal.py measures on the GPU: no HIP device visible")
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

    emit(f"# bench_deflickerlocal: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds after one warm-up, median (min .. max) ms; "
         f"radius {RADIUS}, tol {TOL}, lam {LAM}, two planes panning {STEP} px per frame against each other")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for size in args.sizes.split(","):
        H, W = SIZES[size]
        for T in (int(t) for t in args.frames.split(",")):
            wide = torch.randint(40, 216, (H, W + STEP * (T - 1), 3), device="cuda", generator=gen, dtype=torch.int16)
            win = torch.empty((T, H, W, 3), dtype=torch.uint8, device="cuda")
            for t in range(T):
                f = torch.cat([wide[:H // 2, STEP * t:STEP * t + W], wide[H // 2:, STEP * (T - 1 - t):STEP * (T - 1 - t) + W]])
                win[t] = (f + torch.randint(-3, 4, (H, W, 3), device="cuda", generator=gen, dtype=torch.int16)).to(torch.uint8)
            del wide, f
            mask = torch.zeros((T, H, W), dtype=torch.uint8, device="cuda")
            mask[:, H // 2 - 150:H // 2 + 150, W // 2 - 200:W // 2 + 200] = 255
            offs = torch.zeros((T, 2), dtype=torch.int32, device="cuda")
            zero_t = torch.from_numpy(deflickeralign.identity_track(T)).to("cuda")
            out = torch.empty_like(win)
            K = 2 * RADIUS + 1
            pairs = sum(1 for t in range(T) for s in range(t - RADIUS, t + RADIUS + 1) if s != t and 0 <= s < T)
            zero_mv = torch.zeros((T, K) + flicklocal_bind.blocks(H, W, 8) + (4,), dtype=torch.int32, device="cuda")
            zero_mv[..., 2] = 1
            a, sa = flickalign_hip.hold(win, offs, zero_t, mask, RADIUS, TOL)
            b, sb = flicklocal_bind.hold(win, offs, zero_t, zero_mv, mask, RADIUS, 8, TOL)
            if not ((a == b).all().item() and (sa == sb).all().item()):
                raise SystemExit("bench_deflickerlocal.py: vvk_hold with zero vectors does not give vvc_hold's bytes")
            del a, b
            found, stats = flicklocal_bind.search(win, offs, zero_t, RADIUS, DeflickerLocalConfig(8, 4, LAM))
            _, sf = flicklocal_bind.hold(win, offs, zero_t, found, mask, RADIUS, 8, TOL)
            accepted = {"fixed place": float(sa[:, 2].sum().item()) / (T * H * W), "along the vectors": float(sf[:, 2].sum().item()) / (T * H * W)}
            moved = float(stats[:, :, 1].sum().item()) / max(float(stats[:, :, 0].sum().item()), 1.0)
            ref = "vvc_hold, zero track"
            calls = [(ref, lambda: flickalign_hip.hold(win, offs, zero_t, mask, RADIUS, TOL, out=out)),
                     ("vvk_hold, zero vectors", lambda: flicklocal_bind.hold(win, offs, zero_t, zero_mv, mask, RADIUS, 8, TOL, out=out)),
                     ("vvk_hold, searched vectors", lambda: flicklocal_bind.hold(win, offs, zero_t, found, mask, RADIUS, 8, TOL, out=out))]
            searches = {}
            for block in (8, 16):
                mv = torch.empty((T, K) + flicklocal_bind.blocks(H, W, block) + (4,), dtype=torch.int32, device="cuda")
                st = torch.empty((T, K, 6), dtype=torch.int64, device="cuda")
                for search in (2, 4, 8):
                    name = f"vvk_search block {block}, search {search}"
                    searches[name] = (block, search)
                    calls.append((name, lambda c=DeflickerLocalConfig(block, search, LAM), m=mv, s=st: flicklocal_bind.search(win, offs, zero_t, RADIUS, c, mv=m, stats=s)))
            for _, fn in calls:
                event_ms(fn)                                                                       # warm-up
            ms = {name: [] for name, _ in calls}
            for _ in range(args.rounds):
                for name, fn in calls:
                    ms[name].append(event_ms(fn))
            emit(f"# {W}x{H}, {T} frames ({win.numel() / 2 ** 20:.0f} MiB of pixels); mean accepted samples at a fixed place {accepted['fixed place']:.2f}, "
                 f"along the searched vectors {accepted['along the vectors']:.2f}; {100 * moved:.1f} % of the vectors non-zero; zero vectors give vvc_hold's bytes: True")
            med = {name: statistics.median(v) for name, v in ms.items()}
            hbm_ms = pairs * H * W * 3 / HBM_RATE * 1e3
            for name, _ in calls:
                v = ms[name]
                rec = {"frame": f"{W}x{H}", "frames": T, "call": name, "ms": [round(x, 4) for x in v], "median_ms": round(med[name], 4),
                       "ms_per_frame": round(med[name] / T, 5)}
                if name in searches:
                    block, search = searches[name]
                    diffs = pairs * H * W * 3 * (2 * search + 1) ** 2
                    sad_ms = diffs / SAD_PEAK * 1e3
                    rec.update(byte_differences=diffs, per_second=round(diffs / (med[name] * 1e-3), 0), sad_floor_ms=round(sad_ms, 4), hbm_floor_ms=round(hbm_ms, 4),
                               bound_by="packed SAD" if sad_ms >= hbm_ms else "HBM", share_of_floor=round(max(sad_ms, hbm_ms) / med[name], 4))
                    emit(f"{W}x{H} T={T:3d} {name:30s} {med[name]:9.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med[name] / T:.4f} ms/frame  {diffs:.3e} byte differences, "
                         f"{rec['per_second']:.3e} /s; floors: packed SAD {sad_ms:.3f} ms, HBM {hbm_ms:.3f} ms -> {100 * rec['share_of_floor']:.1f} % of the {rec['bound_by']} floor")
                else:
                    rec.update(against=ref, ratio=round(med[name] / med[ref], 3))
                    emit(f"{W}x{H} T={T:3d} {name:30s} {med[name]:9.3f} ({min(v):.3f} .. {max(v):.3f}) ms  {med[name] / T:.4f} ms/frame  {rec['ratio']:.2f} x {ref}")
                records.append(rec)
            stage = med["vvk_search block 8, search 4"] + med["vvk_hold, searched vectors"]
            records.append({"frame": f"{W}x{H}", "frames": T, "call": "stage (search block 8, search 4 + filter)", "median_ms": round(stage, 4),
                            "ms_per_frame": round(stage / T, 5), "share_of_model": round(stage / T / MODEL_MS_PER_FRAME, 6),
                            "search_share_of_stage": round(med["vvk_search block 8, search 4"] / stage, 4)})
            emit(f"{W}x{H} T={T:3d} the stage (search block 8, search 4 + filter) {stage:9.3f} ms  {stage / T:.4f} ms/frame = {100 * stage / T / MODEL_MS_PER_FRAME:.3f} % of the "
                 f"model's {MODEL_MS_PER_FRAME:.0f} ms per frame; the search is {100 * med['vvk_search block 8, search 4'] / stage:.0f} % of it")
            del win, mask, offs, out, zero_mv, found, mv, st
            torch.cuda.empty_cache()
    js = json.dumps({"bench_deflickerlocal": records, "rounds": args.rounds, "radius": RADIUS, "tol": TOL, "step": STEP, "lam": LAM})
    print(js)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + js + "\n")


if __name__ == "__main__":
    main()
