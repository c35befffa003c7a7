"""The table the cut detector's defaults (videovanish_amd/spans.py, SpanConfig.cut_*) were read from: the detector's two statistics and their peak
ratios over the seeded synthetic clip families of tests/spans_ref.py (320 x 180), at the true cuts and at every other frame pair.  Host only (the
numpy restatement of the device statistics, which the GPU tests hold equal to the kernel bit for bit).  Nobody has run the detector on real video.

  python tools/spans_detector_table.py [--seeds 6] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seeds", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import spans_ref as R
    from videovanish_amd import spans as S
    cfg = S.SpanConfig()
    fams = {}

    def add(fam, frames, cuts, masks=None):
        sad, n, hist = R.pair_stats(np.stack(frames), masks)
        m, h = S.cut_statistics(sad, n, hist)
        rh, rm = S.peak_ratios(h, cfg.cut_window), S.peak_ratios(m, cfg.cut_window)
        found = S.find_cuts(sad, n, hist, cfg, npix=R.H * R.W)
        rec = fams.setdefault(fam, {"cut": [], "other": [], "clips": 0, "exact": 0})
        rec["clips"] += 1
        rec["exact"] += found == cuts
        for p in range(len(m)):
            rec["cut" if p + 1 in cuts else "other"].append((h[p], m[p], rh[p], rm[p]))

    for seed in range(args.seeds):
        for v in (2, 6, 12):
            add(f"two shots, pan {v} px", *R.shots_clip(100 + seed * 10 + v, (12, 12), (v, v)))
        add("three shots, pans 2 / 12 / 6 px", *R.shots_clip(200 + seed, (10, 9, 11), (2, 12, 6)))
        add("pan only", *R.shots_clip(250 + seed, (20,), (2 + 5 * (seed % 3),)))
        add("8-frame dissolve", *R.dissolve_clip(300 + seed))
        add("+70 one-frame flash", *R.flash_clip(400 + seed))
        add("white noise", *R.noise_clip(500 + seed))
        frames, cuts = R.shots_clip(600 + seed, (12, 12), (6, 6))
        masks = R.moving_box(24)
        add("two shots, moving masked box", R.paint(frames, masks, seed), cuts, masks)

    lines = [f"# spans_detector_table: {args.seeds} seeds per family, {R.W}x{R.H}, window +-{cfg.cut_window} pairs; defaults: h >= {cfg.cut_h_min}, m >= {cfg.cut_m_min}, "
             f"h ratio >= {cfg.cut_h_ratio}, m ratio >= {cfg.cut_m_ratio}, cover >= {cfg.cut_min_cover}, segment >= {cfg.cut_min_seg}",
             "| family | pairs | h | m | h peak ratio | m peak ratio | clips with exactly the true cuts |", "|---|---|---|---|---|---|---|"]
    rng = lambda a: "-" if not len(a) else (f"{min(a):.3g}" if min(a) == max(a) else f"{min(a):.3g} - {max(a):.3g}")
    allc, allo = [], []
    for fam, rec in fams.items():
        for kind in ("cut", "other"):
            rows = np.array(rec[kind]).reshape(-1, 4)
            if not len(rows):
                continue
            (allc if kind == "cut" else allo).append(rows)
            lines.append(f"| {fam} | {'at the cut' if kind == 'cut' else 'every other pair'} ({len(rows)}) | {rng(rows[:, 0])} | {rng(rows[:, 1])} | {rng(rows[:, 2])} | "
                         f"{rng(rows[:, 3])} | {rec['exact']} of {rec['clips']} |")
    c, o = np.concatenate(allc), np.concatenate(allo)
    lines.append(f"all families: h peak ratio at cuts >= {c[:, 2].min():.3g}, elsewhere <= {o[:, 2].max():.3g}; m peak ratio at cuts >= {c[:, 3].min():.3g}, elsewhere <= "
                 f"{o[:, 3].max():.3g}; at cuts h >= {c[:, 0].min():.3g}, m >= {c[:, 1].min():.3g}; elsewhere h <= {o[:, 0].max():.3g}, m <= {o[:, 1].max():.3g}")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
