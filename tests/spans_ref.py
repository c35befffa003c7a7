"""Helpers of the mask-span tests: the numpy restatement of the device's frame-pair statistics (csrc/vv_spans.hip) and the seeded synthetic
clip families the cut detector's defaults were read from.  No test in here."""
import numpy as np

BINS = 64


def luma(rgb):
    """Integer luma of [..., 3] uint8: (77 R + 150 G + 29 B + 128) >> 8."""
    c = rgb.astype(np.int64)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8


def pair_stats(frames, masks=None):
    """frames [T,H,W,3] u8, masks [T,H,W] u8 or None -> (sad [T-1], n [T-1], hist [T-1,2,64]) int64: per adjacent pair, over the pixels that are zero
    in both frames' masks, the luma sum of absolute differences, the pixel count and the two luma histograms (bin = luma >> 2)."""
    frames = np.asarray(frames)
    T = frames.shape[0]
    y = luma(frames)
    sad, n, hist = np.zeros(T - 1, np.int64), np.zeros(T - 1, np.int64), np.zeros((T - 1, 2, BINS), np.int64)
    for p in range(T - 1):
        keep = np.ones(y.shape[1:], bool) if masks is None else (np.asarray(masks[p]) == 0) & (np.asarray(masks[p + 1]) == 0)
        a, b = y[p][keep], y[p + 1][keep]
        n[p] = keep.sum()
        sad[p] = np.abs(a - b).sum()
        hist[p, 0] = np.bincount(a >> 2, minlength=BINS)
        hist[p, 1] = np.bincount(b >> 2, minlength=BINS)
    return sad, n, hist


# ---- synthetic families -----------------------------------------------------------------------------------------------------------------
H, W = 180, 320


def texture(rng, h, w):
    """One shot's world: per channel a weighted sum of three random block textures at 32, 8 and 2 px, with the shot's own exposure."""
    out = np.zeros((h, w, 3))
    wts = rng.dirichlet((2.0, 2.0, 2.0))
    for c in range(3):
        for b, wt in zip((32, 8, 2), wts):
            g = rng.integers(0, 256, (-(-h // b), -(-w // b))).astype(np.float64)
            out[..., c] += wt * np.repeat(np.repeat(g, b, 0), b, 1)[:h, :w]
    gain, offset = rng.uniform(0.6, 1.0), rng.uniform(-40, 40)
    return np.clip((out - 128) * gain + 128 + offset, 0, 255).astype(np.uint8)


def pan_shot(rng, T, v, h=H, w=W):
    """T frames (h x w) of a shot panned v px per frame."""
    world = texture(rng, h, w + v * T)
    return [world[:, v * t: v * t + w].copy() for t in range(T)]


def shots_clip(seed, lengths, speeds, h=H, w=W):
    """Shots of the given lengths under pans of the given speeds, joined by hard cuts -> (frames, true cuts)."""
    rng = np.random.default_rng(seed)
    frames, cuts = [], []
    for L, v in zip(lengths, speeds):
        if frames:
            cuts.append(len(frames))
        frames += pan_shot(rng, L, v, h, w)
    return frames, cuts


def dissolve_clip(seed, L=12, D=8, v=4):
    """Two shots joined by a D-frame linear dissolve: no hard cut."""
    rng = np.random.default_rng(seed)
    a, b = pan_shot(rng, L + D, v), pan_shot(rng, L + D, v)
    frames = a[:L]
    for k in range(D):
        w = (k + 1) / (D + 1)
        frames.append(np.clip((1 - w) * a[L + k].astype(np.float64) + w * b[k] + 0.5, 0, 255).astype(np.uint8))
    return frames + b[D:], []


def flash_clip(seed, T=24, at=11, v=4, gain=70):
    """One shot with frame `at` brightened by `gain` grey levels: two adjacent peaks, no cut."""
    rng = np.random.default_rng(seed)
    frames = pan_shot(rng, T, v)
    frames[at] = np.clip(frames[at].astype(np.int64) + gain, 0, 255).astype(np.uint8)
    return frames, []


def noise_clip(seed, T=16):
    """Independent white-noise frames: every pair differs alike, no pair is a peak."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(T)], []


def moving_box(T, v=6, size=(60, 90), y0=50):
    """Masks [T,H,W] u8 of a box crossing the frame v px per frame."""
    m = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        x = 10 + v * t
        m[t, y0:y0 + size[0], x:x + size[1]] = 255
    return m


def paint(frames, masks, seed):
    """The object that is about to be removed: flickering noise inside the mask (it must not vote for a cut)."""
    rng = np.random.default_rng(seed)
    out = []
    for f, m in zip(frames, masks):
        f = f.copy()
        f[m > 0] = rng.integers(0, 256, 3) if rng.random() < 0.5 else 255 - rng.integers(0, 64, 3)
        out.append(f)
    return out
