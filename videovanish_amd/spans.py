"""Mask-span inference: the temporal plan of a call (pure host logic, no torch; covered by CPU tests).

The cost of diffuerase.run_infill_on_frames follows the clip length whatever the masks say, and its chunks, their cross-fade, temporal attention
and the flow-guided prior all assume temporal continuity.  One piece of temporal planning answers both: the frames are split into SPANS -- at
hard cuts, and (mode "masked") around the runs of masked frames only -- and each span is an ordinary shorter clip for the unchanged pipeline, the
way a region window (roi.py) is an ordinary smaller clip.  Frames outside every span are returned as they came.  Rules, guarantees, limits and
the table the detector's defaults were read from: DESIGN.md, "Mask-span inference".

  plan_spans   masked flags + cuts + SpanConfig -> half-open spans
  find_cuts    per-pair statistics of the device kernel (spans_hip.frame_pair_stats) -> hard cuts
"""
import dataclasses

import numpy as np

MODES = ("masked", "all")
SPELLINGS = ("masked", "cuts", "masked-cuts")        # what --spans / $VV_SPANS / spans= accept as a string (besides "off"): (mode, cuts) below
_SPELLED = {"masked": ("masked", None), "cuts": ("all", "auto"), "masked-cuts": ("masked", "auto")}


@dataclasses.dataclass(frozen=True)
class SpanConfig:
    """mode: "masked" = only spans around masked frames are processed; "all" = every frame is, but split at cuts.
    cuts: None, "auto" (find_cuts on the device statistics) or frame indices: c means frames c - 1 and c belong to different shots.
    context: unmasked frames kept on each side of a masked run (the prior and temporal attention draw the background from frames where it is
    visible; the default is RunConfig.overlap, build-defined).  min_len: least span length (the fused C=320 motion module runs for 16 <= F <= 32).
    min_gap: a gap of fewer unprocessed frames than this between two spans is run rather than split.
    Detector (find_cuts; m = mean absolute luma difference of a frame pair, h = half the L1 distance of the pair's normalised luma histograms):
    cut_m_min / cut_h_min: floors both statistics must clear; cut_h_ratio / cut_m_ratio: each must be at least this many times the largest value
    of the other pairs within +-cut_window pairs (an isolated peak); cut_min_cover: least unmasked share of the frame for a decision;
    cut_min_seg: cuts that would leave a segment shorter than this many frames are dropped together.  The defaults were read from the statistics of
    synthetic clips (DESIGN.md section 11 has the table); nobody has run the detector on real video."""
    mode: str = "masked"
    cuts: object = None
    context: int = 8
    min_len: int = 16
    min_gap: int = 8
    cut_m_min: float = 10.0
    cut_h_min: float = 0.05
    cut_h_ratio: float = 4.0
    cut_m_ratio: float = 0.5
    cut_window: int = 4
    cut_min_cover: float = 0.25
    cut_min_seg: int = 4

    def __post_init__(self):
        if self.mode not in MODES:
            raise ValueError(f"SpanConfig.mode must be one of {MODES}, not {self.mode!r}")
        c = self.cuts
        if isinstance(c, str):
            if c.strip().lower() != "auto":
                raise ValueError(f"SpanConfig.cuts must be None, 'auto' or frame indices, not {c!r}")
            object.__setattr__(self, "cuts", "auto")
        elif c is not None:
            c = tuple(sorted({int(v) for v in c}))
            if any(v < 0 for v in c):
                raise ValueError(f"SpanConfig.cuts: negative frame index in {c}")
            object.__setattr__(self, "cuts", c)
        if self.context < 0 or self.min_len < 1 or self.min_gap < 0 or self.cut_window < 1 or self.cut_min_seg < 1 or not 0 <= self.cut_min_cover <= 1 \
                or min(self.cut_m_min, self.cut_h_min, self.cut_h_ratio, self.cut_m_ratio) < 0:
            raise ValueError(f"SpanConfig: bad parameters {self}")


def as_config(spans):
    """None / False / "off" / "none" / "" -> None (the full clip); "masked" -> SpanConfig("masked"); "cuts" -> SpanConfig("all", cuts="auto");
    "masked-cuts" -> SpanConfig("masked", cuts="auto"); a SpanConfig as it is."""
    if spans is None or spans is False:
        return None
    if isinstance(spans, SpanConfig):
        return spans
    if isinstance(spans, str):
        s = spans.strip().lower()
        if s in ("", "off", "none"):
            return None
        if s in _SPELLED:
            mode, cuts = _SPELLED[s]
            return SpanConfig(mode, cuts=cuts)
    raise ValueError(f"spans must be None, 'masked', 'cuts', 'masked-cuts', 'off' or a SpanConfig, not {spans!r}")


def parse_cuts(text):
    """"120,431" -> (120, 431) (the CLI's --cuts)."""
    return tuple(sorted({int(v) for v in str(text).replace(" ", "").split(",") if v}))


def segments(T, cuts):
    """The maximal ranges between cuts: half-open (s, e) covering [0, T).  Cuts outside [1, T - 1] separate nothing and are ignored."""
    if T <= 0:
        return []
    edges = [0] + sorted({int(c) for c in (cuts or ()) if 0 < int(c) < T}) + [T]
    return [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]


def _merge(spans, min_gap):
    """Left to right: a span that overlaps the one before it, touches it, or leaves a gap below min_gap joins it."""
    out = []
    for a, b in spans:
        if out and (a - out[-1][1] <= 0 or a - out[-1][1] < min_gap):
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def plan_spans(masked, cuts, cfg):
    """masked: bool [T] (frame t has a pixel in its dilated mask); cuts: frame indices (None: cfg.cuts when that is a sequence, else none).
    Returns the half-open spans [(a, b)], sorted and disjoint.  Segments are the ranges between cuts and nothing crosses one.  Mode "all": the
    spans are the segments.  Mode "masked", inside each segment: the maximal runs of masked frames, grown by cfg.context on both sides (clamped
    to the segment), merged where they overlap or their gap is below cfg.min_gap, raised to min(cfg.min_len, segment length) by growing left and
    right alternately (clamped), merged again.  Depends on nothing but its arguments: every rank makes the same plan."""
    masked = np.asarray(masked).astype(bool).reshape(-1)
    T = len(masked)
    if cuts is None:
        cuts = cfg.cuts if isinstance(cfg.cuts, tuple) else ()
    segs = segments(T, cuts)
    if cfg.mode == "all":
        return [(s, e) for s, e in segs]
    out = []
    for s, e in segs:
        idx = np.nonzero(masked[s:e])[0] + s
        if len(idx) == 0:
            continue
        brk = np.nonzero(np.diff(idx) > 1)[0]
        runs = zip(np.concatenate([idx[:1], idx[brk + 1]]).tolist(), (np.concatenate([idx[brk], idx[-1:]]) + 1).tolist())
        spans = _merge([(max(s, a - cfg.context), min(e, b + cfg.context)) for a, b in runs], cfg.min_gap)
        need = min(cfg.min_len, e - s)
        for sp in spans:
            left = True
            while sp[1] - sp[0] < need:
                if (left and sp[0] > s) or sp[1] >= e:
                    sp[0] -= 1
                else:
                    sp[1] += 1
                left = not left
        out += [(a, b) for a, b in _merge(spans, cfg.min_gap)]
    return out


def cut_statistics(sad, n, hist):
    """The detector's two statistics per frame pair: m = sad / n and h = half the L1 distance of the two normalised histograms (0 where n = 0).
    sad, n: [P] integers; hist: [P, 2, 64] integers."""
    sad, n, hist = np.asarray(sad, np.float64), np.asarray(n, np.float64), np.asarray(hist, np.float64)
    d = np.maximum(n, 1.0)
    m = np.where(n > 0, sad / d, 0.0)
    h = np.where(n > 0, 0.5 * np.abs(hist[:, 0] - hist[:, 1]).sum(axis=1) / d, 0.0)
    return m, h


def peak_ratios(v, window):
    """v[p] over the largest v of the other pairs within +-window (inf where that is 0 and v[p] > 0; 0 where v[p] is 0)."""
    v = np.asarray(v, np.float64)
    out = np.zeros(len(v))
    for p in range(len(v)):
        others = np.concatenate([v[max(0, p - window):p], v[p + 1:p + 1 + window]])
        top = others.max() if len(others) else 0.0
        out[p] = 0.0 if v[p] <= 0 else (np.inf if top <= 0 else v[p] / top)
    return out


def find_cuts(sad, n, hist, cfg, npix=None):
    """Hard cuts from the pair statistics (pair p = frames p, p + 1; a cut is reported as the frame index p + 1).  Pair p is a cut when m and h
    both clear their floors, both are isolated peaks (peak_ratios >= cfg.cut_h_ratio / cfg.cut_m_ratio) and n covers at least cfg.cut_min_cover
    of the frame's npix pixels (None: the largest n stands for the frame); then the cuts that would leave a segment shorter than cfg.cut_min_seg
    frames are dropped together.  Dissolves and fades are continuous and are not cuts."""
    n = np.asarray(n, np.int64).reshape(-1)
    P = len(n)
    if P == 0:
        return []
    m, h = cut_statistics(sad, n, hist)
    full = float(npix) if npix is not None else float(n.max())
    ok = (n > 0) & (n >= cfg.cut_min_cover * full) & (m >= cfg.cut_m_min) & (h >= cfg.cut_h_min)
    ok &= (peak_ratios(h, cfg.cut_window) >= cfg.cut_h_ratio) & (peak_ratios(m, cfg.cut_window) >= cfg.cut_m_ratio)
    cuts = [int(p) + 1 for p in np.nonzero(ok)[0]]
    edges = [0] + cuts + [P + 1]
    short = {edges[i + k] for i in range(len(edges) - 1) if edges[i + 1] - edges[i] < cfg.cut_min_seg for k in (0, 1)}
    return [c for c in cuts if c not in short]
