"""Plain restatements of the helper kernels whose only direct test was a first-generation one: the uint8 image kernels of vv_image.hip past their grid cap, the
flow-completion and generator helpers of vv_deform.hip and the SAM 2 helpers of vv_sam2.hip, written from include/vvhip.h and the comments above the kernels, on the
CPU, without the HIP library.  The sibling of tests/auxref.py, whose pieces it uses (the units U, the sentinels, bound(), noise_of(), the caps).

EXACT kernels: the integer image kernels (against oracle/imageops_ref.py and the host routine vvio_ycbcr_to_rgb), gathers and selects, and the float kernels whose
result does not depend on contraction (products with 0, 1 or a power of two, a lone division, a lone sum): ft = torch.float32 is what the GPU must EQUAL, ft =
torch.float64 anchors it.  ROUNDED kernels (tanh, GELU, sigmoid, sinf / cosf / powf, fma accumulation; vv_deform.hip and vv_sam2.hip leave contraction to the
compiler) are compared against ft = torch.float64, rounded to h16 where the kernel stores h16:

    |got - ref| <= B = ceil(4 N) u max(1, max |ref|)          (auxref.bound with NOISE below)

N >= 1: the noise of the same formula in fp32 on the CPU, measured by tests/test_aux2ref_cpu.py on the GPU test's own inputs (a stale entry fails there).
Mutants (`mut=`) restate an indexing mistake; the CPU test shows each one misses at the GPU test's shapes."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import auxref as A
from auxref import F32, F64, U, TD, IMAGE_CAP, ACT_NONE, ACT_SILU, ACT_RELU, ACT_GELU, ACT_SIGMOID, cf, r16, gen, randn, noise_of  # noqa: F401

# N of every rounded kernel, per output type (test_aux2ref_cpu.py::test_noise_floor measures them on the GPU test's own inputs; never below 1 in the bound).
NOISE = {"dwconv:fp32": 3.893, "fold:bf16": 0.441, "fold:fp16": 0.239, "fold:fp32": 1.810, "gen_compose:fp32": 1.228, "hyper_masks:fp32": 3.784,
         "pixel_shuffle:bf16": 0.000, "pixel_shuffle:fp16": 0.000, "pixel_shuffle:fp32": 1.502, "prompt_points:fp32": 8.429, "resize_f32:fp32": 28.869,
         "rope:bf16": 0.000, "rope:fp16": 0.000, "sine_pe_large:fp32": 31751.296, "sine_pe_small:fp32": 0.864, "upsample2x:bf16": 0.753, "upsample2x:fp16": 0.606,
         "upsample2x:fp32": 5.189}


def bound(key, out_dtype, ref, gelu_x=None):
    return A.bound(key, out_dtype, ref, gelu_x, table=NOISE)


def nrng(seed):
    return np.random.default_rng(seed)


# ================================================================================================================ vv_image.hip past IMAGE_CAP (exact, integer)
CLIP = dict(T=80, H=245, W=245)          # 4 802 000 pixels: many small odd-sized DISTINCT frames, ten of them past the cap, so the oracle runs per small frame
RESIZE_DST = (230, 262)                  # Hd, Wd: 80 x 60 260 = 4 820 800 destination pixels
RESIZE_SRC = {"up": (97, 131), "down": (517, 301)}          # Hs, Ws: non-integer ratios, one above and one below 1 on each axis
YCC_MODES = [(1, 1), (0, 0), (2, 0)]     # (hshift, vshift)
DIST_BIG_F = float(np.float32(0x7fffffff >> 2) * np.float32(1.0 / 65536.0))          # what vv_chamfer_dt writes beyond its radius


def frames_past_cap(T, per):
    """whole frames that lie past the cap"""
    return T - (IMAGE_CAP + per - 1) // per


def ycc_inputs(hs, vs):
    T, H, W = CLIP["T"], CLIP["H"], CLIP["W"]
    ch, cw = (H + (1 << vs) - 1) >> vs, (W + (1 << hs) - 1) >> hs
    r = nrng(110 + 3 * hs + vs)
    return tuple(r.integers(0, 256, s, dtype=np.uint8) for s in ((T, H, W), (T, ch, cw), (T, ch, cw)))


def ycc_host(y, cb, cr, hs, vs, full):
    """the host routine vvio_ycbcr_to_rgb, frame by frame"""
    from videovanish_amd import frameio
    return frameio.ycbcr_to_rgb(y, cb, cr, hs, vs, full, device=False)


def clip_masks(ch, T=None, H=None, W=None, seed=120):
    """u8 [T,H,W,ch]: frame t is empty (t % 4 == 0), holds one set pixel near the centre (1), sparse set pixels in ONE channel with the first and the last row and
    column touched (2), or a block with holes plus sparse pixels (3); every kind occurs past the cap, all non-empty frames differ"""
    T, H, W = T or CLIP["T"], H or CLIP["H"], W or CLIP["W"]
    r = nrng(seed + ch)
    m = np.zeros((T, H, W, ch), np.uint8)
    for t in range(T):
        k = t % 4
        if k == 1:
            m[t, H // 2 - 20 + t % 41, W // 2 - 20 + (7 * t) % 41, t % ch] = 1 + t
        elif k >= 2:
            sp = r.random((H, W)) < 0.002
            m[t, ..., t % ch][sp] = r.integers(1, 256, int(sp.sum()), dtype=np.uint8)
            m[t, 0, (3 * t) % W, 0] = m[t, H - 1, (5 * t) % W, 0] = m[t, (7 * t) % H, 0, 0] = m[t, (11 * t) % H, W - 1, 0] = 255
            if k == 3:
                y0, x0 = 5 + t % 60, 9 + (3 * t) % 50
                m[t, y0:y0 + 40 + t % 30, x0:x0 + 60 + t % 50, :] = 200
                hole = r.random((H, W)) < 0.01
                m[t][hole] = 0
    return m


def collapse_dilate(masks, iters, mut=None):
    """oracle/imageops_ref.py frame by frame -> u8 [T,H,W].  mut "frame_index": the any-pixel flag of the whole-frame fill (iters < 1) read at i / (npix + 1);
    "no_frame_edge": the dilation walks the stacked frames as one tall image"""
    from oracle import imageops_ref as I
    T, H, W, _ = masks.shape
    if mut == "no_frame_edge":
        return np.asarray(I.collapse_and_dilate([masks.reshape(T * H, W, -1)], iters)[0]).reshape(T, H, W)
    if iters < 1 and mut == "frame_index":          # scipy's "until nothing changes" on a 4-connected grid: the whole frame as soon as one pixel is set
        flag = np.any(masks > 0, axis=(1, 2, 3))
        fr = np.arange(T * H * W) // (H * W + 1)
        return (flag[fr].astype(np.uint8) * 255).reshape(T, H, W)
    return np.stack(I.collapse_and_dilate(list(masks), iters))


def resize_inputs(kind, ch):
    Hs, Ws = RESIZE_SRC[kind]
    return nrng(130 + ch + (0 if kind == "up" else 7)).integers(0, 256, (CLIP["T"], Hs, Ws, ch), dtype=np.uint8)


def resize_u8(src, Hd, Wd, mode, mut=None):
    """oracle frame by frame -> u8 [T,Hd,Wd,ch]; mut "frame_base": every frame reads frame 0"""
    from oracle import imageops_ref as I
    fn = I.resize_bilinear_u8 if mode == "bilinear" else I.resize_nearest_u8
    return np.stack([fn(src[0 if mut == "frame_base" else t], Wd, Hd) for t in range(src.shape[0])])


def dt_frames(bin_u8):
    """cv2.distanceTransform(DIST_L2, 5) frame by frame, by the C form of the oracle (oracle/imageops_c.py: the numpy form walks every pixel in Python; the CPU test
    holds the two equal on whole frames)"""
    from oracle import imageops_c as IC
    return np.stack([IC.distance_transform_l2_5(f) for f in bin_u8])


def chamfer_dt(bin_u8, R, mut=None):
    """vv_chamfer_dt: the oracle's distance where it is <= R, DIST_BIG beyond (the window of radius R cannot vouch for more); mut "frame_base": frame 0's mask"""
    m = np.where(bin_u8 > 0, 255, 0).astype(np.uint8)
    d = dt_frames(m if mut != "frame_base" else np.repeat(m[:1], m.shape[0], 0))
    return np.where(d <= R, d, np.float32(DIST_BIG_F)).astype(np.float32)


def feather_composite(inp, orig, mask, feather, mut=None):
    from oracle import imageops_ref as I
    mb = np.where(mask > 0, 255, 0).astype(np.uint8)
    if mut == "frame_base":
        mb = np.repeat(mb[:1], mb.shape[0], 0)
    if feather > 0:
        d_in, d_out = dt_frames(mb), dt_frames(np.bitwise_not(mb))
        return np.stack([I.composite(inp[t], orig[t], I.feather_alpha(mb[t], feather, d_in[t], d_out[t])) for t in range(mb.shape[0])])
    return np.stack([I.composite(inp[t], orig[t], I.feather_alpha(mb[t], feather)) for t in range(mb.shape[0])])


def blur_compose(pix, orig, mask, mut=None):
    from oracle import imageops_ref as I
    return np.stack([I.blur_compose(pix[t], orig[t], mask[0 if mut == "frame_base" else t]) for t in range(mask.shape[0])])


def compose_inputs(T=None, H=None, W=None, seed=140):
    """(inp u8 [T,H,W,3], orig u8 [T,H,W,3], pix fp32 [T,H,W,3] in [0, 1), mask u8 [T,H,W])"""
    T, H, W = T or CLIP["T"], H or CLIP["H"], W or CLIP["W"]
    r = nrng(seed)
    mask = clip_masks(1, T, H, W, seed + 1)[..., 0] if H > 40 else (r.random((T, H, W)) < 0.3).astype(np.uint8) * 255
    return r.integers(0, 256, (T, H, W, 3), dtype=np.uint8), r.integers(0, 256, (T, H, W, 3), dtype=np.uint8), r.random((T, H, W, 3), dtype=np.float32), mask


# ================================================================================================================ vv_deform.hip: flow completion and generator helpers
FC_SHAPE = (3, 5, 7)          # T, H, W
FC_PADS = [0, 2, 9]           # 9 > H: the replicate clamp folds whole rows of padding onto the border


def fc_inputs():
    T, H, W = FC_SHAPE
    return randn(201, T, H, W, 2, scale=3.0), (torch.rand(T, H, W, generator=gen(202)) < 0.4).to(torch.uint8) * torch.tensor([255, 1, 7], dtype=torch.uint8)[:, None, None]


def fc_input(flow, mask, pad, ft=F32, mut=None):
    """(flow * (1 - m) | m | 0 x 5) of the pixel clamped into the frame -> [T, H + 2 pad, W + 2 pad, 8]  (exact: m is 0 or 1); mut "frame_base": frame 0's pixels"""
    T, H, W, _ = flow.shape
    ys, xs = (torch.arange(H + 2 * pad) - pad).clamp(0, H - 1), (torch.arange(W + 2 * pad) - pad).clamp(0, W - 1)
    src_f, src_m = (flow, mask) if mut != "frame_base" else (flow[:1].expand_as(flow), mask[:1].expand_as(mask))
    m = (src_m != 0).to(ft)[:, ys][:, :, xs]
    out = torch.zeros((T, H + 2 * pad, W + 2 * pad, 8), dtype=ft)
    out[..., :2] = src_f.to(ft)[:, ys][:, :, xs] * (1.0 - m)[..., None]
    out[..., 2] = m
    return out


UP2_CASES = [(2, 5, 7, 8), (2, 1, 6, 24), (2, 4, 1, 8), (2, 3, 3, 24)]          # B, H, W, C: non-square over a block boundary (280 lanes), H = 1, W = 1, C = 24


def up2_inputs(B, H, W, C):
    return randn(210 + H * 10 + W, B, H, W, C, scale=2.0)


def upsample2x(x, ft=F64, mut=None):
    """[B,H,W,C] -> [B,2H,2W,C]: F.interpolate(scale_factor 2, bilinear, align_corners=True): source position o (n - 1) / (2n - 1), 0 when the output has one row;
    mut "batch_out": the batch stride of the INPUT taken from the output size; "xy_swap": the scale of x used along y and the converse"""
    B, H, W, C = x.shape
    Ho, Wo = 2 * H, 2 * W
    def scale(n):
        return (torch.ones((), dtype=F32) * (n - 1) / (2 * n - 1)).to(ft) if ft == F32 else torch.tensor((n - 1) / (2 * n - 1), dtype=ft)

    sy, sx = (scale(H), scale(W)) if mut != "xy_swap" else (scale(W), scale(H))
    fy, fx = sy * torch.arange(Ho).to(ft), sx * torch.arange(Wo).to(ft)
    y0, x0 = fy.long().clamp_max(H - 1), fx.long().clamp_max(W - 1)          # the clamp only holds a mutant inside the image
    y1, x1 = (y0 + 1).clamp_max(H - 1), (x0 + 1).clamp_max(W - 1)
    ly, lx = (fy - y0.to(ft))[:, None], (fx - x0.to(ft))[None, :]
    flat = x.to(ft).reshape(-1, C)
    b = torch.arange(B)[:, None, None] * (Ho * Wo if mut == "batch_out" else H * W)

    def tap(yy, xx):
        return flat[(b + yy[None, :, None] * W + xx[None, None, :]) % flat.shape[0]]          # [B,Ho,Wo,C]; the modulo only keeps a mutant inside the buffer

    w = [(1.0 - ly) * (1.0 - lx), (1.0 - ly) * lx, ly * (1.0 - lx), ly * lx]
    out = torch.zeros((B, Ho, Wo, C), dtype=ft)
    for wt, (yy, xx) in zip(w, ((y0, x0), (y0, x1), (y1, x0), (y1, x1))):
        out = out + wt[None, :, :, None] * tap(yy, xx)
    return out


PIX_N = 3 * 11 * 13          # 429 pixels: over a block, not a multiple of 256
LD_PRED = {"flow_combine": [2, 8], "gen_compose": [3, 8]}          # the minimum and the real row pitch


def mask_0_1_255(n, seed):
    return torch.tensor([0, 1, 255, 0], dtype=torch.uint8)[torch.randint(0, 4, (n,), generator=gen(seed))]


def flow_combine(pred, flow, mask, mut=None):
    """pred [N,ld], flow [N,2], mask u8 [N] -> pred[:, :2] in the hole, flow outside (a select); mut "ld_min": pred read with a pitch of 2"""
    p = pred[:, :2] if mut != "ld_min" else pred.reshape(-1)[:2 * pred.shape[0]].reshape(-1, 2)
    return torch.where((mask != 0)[:, None], p, flow)


GC_N = 5 * 23 * 29          # 3335 pixels, 10 005 values: 0.1 % left out is 10 values
GC_SEED = 231
GC_CAP = 0.001


def gen_compose_inputs(ld, seed=GC_SEED):
    """pred [N,ld] (|x| to 3, and saturating +-12 / +-25), ori u8 [N,3], mask u8 [N] in {0, 1, 255}, acc: the first visit's integers 0 .. 255 as fp32 [N,3]"""
    pred = randn(seed, GC_N, ld, scale=1.2)
    pred[:4, 0] = torch.tensor([12.0, -12.0, 25.0, -25.0])
    mask = mask_0_1_255(GC_N, seed + 1)
    mask[:4] = 255
    return pred, torch.randint(0, 256, (GC_N, 3), generator=gen(seed + 2), dtype=torch.uint8), mask, torch.randint(0, 256, (GC_N, 3), generator=gen(seed + 3)).to(F32)


def gen_compose_t(pred, ft=F64):
    """(tanh(x) + 1) * 0.5 * 255 of the three channels, before the clamp and the floor"""
    return (torch.tanh(pred[:, :3].to(ft)) + 1.0) * 0.5 * 255.0


def gen_compose(pred, ori, mask, acc, first, ft=F64, mut=None):
    """v = hole ? floor(clamp((tanh(x) + 1) / 2 * 255, 0, 255)) : ori; acc = first ? v : floor(acc / 2 + v / 2)  (the reference's uint8 arithmetic);
    mut "ld_min": pred read with a pitch of 3"""
    p = pred if mut != "ld_min" else pred.reshape(-1)[:3 * pred.shape[0]].reshape(-1, 3)
    v = torch.where((mask != 0)[:, None], torch.floor(gen_compose_t(p, ft).clamp(0.0, 255.0)), ori.to(ft))
    return v if first else torch.floor(acc.to(ft) * 0.5 + v * 0.5)


def gen_compose_keep(pred, mask, band):
    """the values compared: outside the hole all; inside, those whose fp64 (tanh + 1) 127.5 lies further than `band` from the integers 1 .. 255 or exactly ON one
    (within the band, but off the integer, the floor hangs on the rounding of tanhf; near 0 it does not: the clamp holds both sides at 0; exactly 255 is what a
    saturated tanh gives in fp64 as in fp32, so the upper clamp is compared)"""
    t = gen_compose_t(pred, F64)
    k = torch.round(t)
    return ~((mask != 0)[:, None] & ((t - k).abs() > 0) & ((t - k).abs() <= band) & (k >= 1))


def gen_input(frames, m_in, m_up, ft=F32):
    """u8 [N,3], u8 [N] x 2 -> [N,8] = (x / 127.5 - 1 | m_in != 0 | m_up != 0 | 0 0 0)"""
    out = torch.zeros((frames.shape[0], 8), dtype=ft)
    out[:, :3] = frames.to(ft) / 127.5 - 1.0
    out[:, 3], out[:, 4] = (m_in != 0).to(ft), (m_up != 0).to(ft)
    return out


GATHER_N, GATHER_ROWS = 301, 37          # 301 and 903 sixteen-byte chunks


def gather_idx(kind, seed=241):
    if kind == "all -1":
        return torch.full((GATHER_N,), -1, dtype=torch.int32)
    idx = torch.randint(-1, GATHER_ROWS, (GATHER_N,), generator=gen(seed), dtype=torch.int32)
    idx[:6] = torch.tensor([GATHER_ROWS - 1, 0, 5, 5, -1, GATHER_ROWS - 1], dtype=torch.int32)
    idx[-1] = GATHER_ROWS - 1
    return idx


def gather_rows(src, idx, mut=None):
    """out[i] = src[idx[i]], a zero row where idx < 0; mut "neg_wraps": a negative index counted from the end"""
    out = src[idx.long().clamp_min(0) if mut != "neg_wraps" else idx.long() % src.shape[0]]
    return out if mut == "neg_wraps" else torch.where((idx < 0)[:, None], torch.zeros((), dtype=src.dtype), out)


FOLD_GEOM = [(7, 3, 3, 11, 14), (3, 2, 0, 6, 7), (3, 2, 0, 6, 8)]          # k, stride, pad, h, w: (3, 2, 0) leaves the last row (and at w = 8 the last column) uncovered
FOLD_C = [8, 24]
FOLD_FLAGS = [(False, False), (True, False), (False, True), (True, True)]          # normalise, gelu
FOLD_B = 2


def fold_grid(k, s, p, h, w):
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def fold_inputs(k, s, p, h, w, C):
    fh, fw = fold_grid(k, s, p, h, w)
    return randn(250 + k + h + w + C, FOLD_B * fh * fw, k * k * C)


def fold_patches(x, B, C, h, w, k, s, p, normalise, gelu, ft=F64, mut=None):
    """tap-major patch rows [B fh fw, k k C] (tap ky k + kx) -> ([B h w, C], max |x| into the GELU): pixel (y, x) sums the patches (py, px) that cover it with
    tap (y + p - py s, x + p - px s); normalise: divided by their number, and a pixel NO patch covers is 0 (F.fold / count gives 0 / 0 = NaN there: the kernel's
    contract is 0); gelu on the result.  mut "tap_order": tap kx k + ky; "fw_for_fh": the batch stride of the patch grid taken as fw fw; "py_lo": the first
    covering patch row of every pixel skipped"""
    fh, fw = fold_grid(k, s, p, h, w)
    rows = x.to(ft).reshape(B * fh * fw, k * k, C)
    out, cnt = torch.zeros((B, h, w, C), dtype=ft), torch.zeros((h, w), dtype=ft)
    bi = torch.arange(B)[:, None, None]
    for ky in range(k):
        ys = torch.arange(fh) * s - p + ky
        vy = (ys >= 0) & (ys < h)
        if mut == "py_lo":
            vy &= torch.arange(fh) > ((ys + p - k + s).div(s, rounding_mode="floor")).clamp_min(0)
        for kx in range(k):
            xs = torch.arange(fw) * s - p + kx
            vx = (xs >= 0) & (xs < w)
            if not bool(vy.any()) or not bool(vx.any()):
                continue
            py, px = torch.arange(fh)[vy], torch.arange(fw)[vx]
            ridx = ((bi * (fw if mut == "fw_for_fh" else fh) + py[None, :, None]) * fw + px[None, None, :]) % rows.shape[0]
            out[:, ys[vy][:, None], xs[vx][None, :]] += rows[ridx, kx * k + ky if mut == "tap_order" else ky * k + kx]
            cnt[ys[vy][:, None], xs[vx][None, :]] += 1.0
    if normalise:
        out = torch.where(cnt[None, :, :, None] > 0, out * (1.0 / cnt.clamp_min(1.0))[None, :, :, None], out)
    gx = out.abs().max().item()
    return (A.act(out, ACT_GELU, ft) if gelu else out).reshape(B * h * w, C), gx


DOWN4_SHAPES = [(3, 4, 4), (3, 8, 20), (3, 36, 44)]          # T, H, W: one output pixel per frame, non-square, 297 outputs


def flow_down4(flow, ft=F32):
    """[T,H,W,2] -> [T,H/4,W/4,2] = (((a + b) / 2 / 2 + (c + d) / 2 / 2) / 4 of the 2 x 2 block at (4y + 1, 4x + 1): every product is by a power of two, so the
    value does not depend on contraction: exact"""
    f = flow.to(ft)
    a, b, c, d = f[:, 1::4, 1::4], f[:, 1::4, 2::4], f[:, 2::4, 1::4], f[:, 2::4, 2::4]
    return ((a + b) * 0.5 * 0.5 + (c + d) * 0.5 * 0.5) * 0.25


# ================================================================================================================ vv_sam2.hip helpers
POOL = dict(B=3, H=6, W=10, C=20, x_off=24, gap=40)          # in_bs = H W C + gap: images apart, the first one x_off elements in; 900 outputs


def pool_inputs():
    """a flat buffer of all-NEGATIVE values (a maximum started at 0 would win everywhere)"""
    d = POOL
    return -(randn(301, d["x_off"] + d["B"] * (d["H"] * d["W"] * d["C"] + d["gap"])).abs() + 0.125)


def maxpool2x2(buf, mut=None):
    """-> [B (H/2) (W/2), C]; mut "zero_init": the maximum started at 0; "batch_contig": in_bs ignored"""
    d = POOL
    per = d["H"] * d["W"] * d["C"]
    bs = per if mut == "batch_contig" else per + d["gap"]
    x = torch.stack([buf[d["x_off"] + b * bs:d["x_off"] + b * bs + per] for b in range(d["B"])]).reshape(d["B"], d["H"] // 2, 2, d["W"] // 2, 2, d["C"])
    out = x.amax(dim=(2, 4))
    return (out.clamp_min(0.0) if mut == "zero_init" else out).reshape(-1, d["C"])


ROPE_CASES = [dict(D=64, rows=11, rows_rope=9, n_table=4, col0=8, ld=80), dict(D=256, rows=5, rows_rope=4, n_table=3, col0=16, ld=288)]


def rope_inputs(c, td):
    ang = torch.rand(c["n_table"], c["D"] // 2, generator=gen(310 + c["D"])) * 6.0 - 3.0
    return randn(311 + c["D"], c["rows"], c["ld"], scale=2.0).to(td), torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).contiguous()


def rope_apply(x, cs, c, td, ft=F64, mut=None):
    """h16 x [rows, ld] -> the same matrix with the pairs (col0 + 2i, col0 + 2i + 1), i < D / 2, of rows < rows_rope rotated by cs[r % n_table][i] = (cos, sin) and
    rounded to h16, every other element as it was.  mut "swap": re and im exchanged; "no_wrap": table row r; "dense": the row pitch taken as D"""
    D, rr, n, col0, ld = c["D"], c["rows_rope"], c["n_table"], c["col0"], c["ld"]
    out = x.to(ft).reshape(-1).clone()
    r, i = torch.arange(rr)[:, None], torch.arange(D // 2)[None, :]
    pos = (r * (D if mut == "dense" else ld) + col0 + 2 * i).reshape(-1)
    t = cs.to(ft)[(r.clamp_max(n - 1) if mut == "no_wrap" else r % n).expand(rr, D // 2).reshape(-1), i.expand(rr, D // 2).reshape(-1)]
    re, im = (out[pos], out[pos + 1]) if mut != "swap" else (out[pos + 1], out[pos])
    out[pos], out[pos + 1] = r16(re * t[:, 0] - im * t[:, 1], td), r16(re * t[:, 1] + im * t[:, 0], td)
    return out.reshape(x.shape)


def rope_region(c):
    m = torch.zeros((c["rows"], c["ld"]), dtype=torch.bool)
    m[:c["rows_rope"], c["col0"]:c["col0"] + c["D"]] = True
    return m


DW_CASES = [(k, C, H, W) for k in (3, 7) for C in (1, 24) for (H, W) in ((9, 11), (2, 3))]          # 2 x 3: smaller than k / 2 + 1 in both directions at k = 7


def dw_inputs(k, C, H, W):
    return randn(320 + k + C + H, H * W, C), randn(321 + k + C + H, C, k, k, scale=0.3), randn(322 + k + C, C)


def dwconv(x, H, W, w, bias, ft=F64, mut=None):
    """NHWC rows [H W, C], w [C,k,k] (c, dy, dx), zero padding k / 2 -> [H W, C]; mut "w_layout": the weights read as (c, dx, dy); "xy_swap": the rows walked as a
    W x H image"""
    C, k = w.shape[0], w.shape[-1]
    ww = w.transpose(1, 2) if mut == "w_layout" else w
    hh, wd = (W, H) if mut == "xy_swap" else (H, W)
    y = F.conv2d(x.to(ft).reshape(hh, wd, C).permute(2, 0, 1)[None], ww.to(ft)[:, None], bias.to(ft), padding=k // 2, groups=C)
    return y[0].permute(1, 2, 0).reshape(H * W, C)


PS = dict(h=5, w=7, C=8)          # 1120 outputs, h != w
PS_ACTS = [ACT_NONE, ACT_SILU, ACT_RELU, ACT_GELU, ACT_SIGMOID]


def ps_inputs():
    d = PS
    return randn(330, d["h"] * d["w"], 4 * d["C"], scale=2.0), randn(331, d["C"]), randn(332, 4 * d["h"] * d["w"], d["C"])


def pixel_shuffle2(y, bias, add, h, w, a, ft=F64, mut=None):
    """y [h w, 4 C] (dy, dx, c) -> ([2h 2w, C] = act(y[(Y / 2, X / 2), (Y & 1, X & 1), c] + bias[c] (+ add)), max |x| into the activation);
    mut "yx_swap": the quadrant (X & 1, Y & 1); "w_for_2w": the output row split by w"""
    C = y.shape[1] // 4
    r = torch.arange(4 * h * w)
    X, Y = (r % (2 * w), r // (2 * w)) if mut != "w_for_2w" else (r % w, r // w)
    q = (Y & 1) * 2 + (X & 1) if mut != "yx_swap" else (X & 1) * 2 + (Y & 1)
    src = (((Y >> 1) * w + (X >> 1)) % (h * w)) * 4 + q
    v = y.to(ft).reshape(h * w * 4, C)[src] + bias.to(ft)
    if add is not None:
        v = v + add.to(ft)
    return A.act(v, a, ft), v.abs().max().item()


RESIZE_F32 = [(1, 5, 4, 9, 1), (6, 1, 11, 3, 3), (7, 9, 7, 9, 3), (7, 9, 17, 20, 1), (23, 31, 9, 13, 3)]          # Hs, Ws, Hd, Wd, C: Hs = 1, Ws = 1, identity, x 2.43 / 2.22, / 2.56 / 2.38


def resize_f32_inputs(Hs, Ws, C):
    return randn(340 + Hs + Ws, Hs * Ws, C)


def resize_bilinear_f32(src, Hs, Ws, Hd, Wd, ft=F64):
    """[Hs Ws, C] -> [Hd Wd, C]: torch's bilinear, align_corners = False: source position max(0, (o + 0.5) s - 0.5) with s = in / out as a C float"""
    C = src.shape[1]

    def axis(n_in, n_out):
        s = (torch.ones((), dtype=F32) * n_in / n_out).to(ft) if ft == F32 else torch.tensor(n_in / n_out, dtype=ft)
        f = ((torch.arange(n_out).to(ft) + 0.5) * s - 0.5).clamp_min(0.0)
        i0 = f.long()
        return i0, i0 + (i0 < n_in - 1).long(), f - i0.to(ft)

    y0, y1, ly = axis(Hs, Hd)
    x0, x1, lx = axis(Ws, Wd)
    p = src.to(ft).reshape(Hs, Ws, C)
    hy, hx, ly, lx = (1.0 - ly)[:, None, None], (1.0 - lx)[None, :, None], ly[:, None, None], lx[None, :, None]
    out = hy * (hx * p[y0][:, x0] + lx * p[y0][:, x1]) + ly * (hx * p[y1][:, x0] + lx * p[y1][:, x1])
    return out.reshape(Hd * Wd, C)


PP_D = [64, 256]
PP_SIZE = 128


def pp_inputs(D):
    """six points: every label, coordinates at 0 and at size - 1"""
    coords = torch.tensor([[0.0, 0.0], [PP_SIZE - 1.0, PP_SIZE - 1.0], [10.0, 20.0], [100.5, 3.25], [0.0, PP_SIZE - 1.0], [64.0, 127.0]])
    return coords, torch.tensor([1, 0, -1, 3, 2, -1], dtype=torch.int32), randn(350 + D, 2, D // 2), randn(351 + D, 5, D)


def prompt_points(coords, labels, inv_size, gauss, table, ft=F64):
    """out[p] = (label < 0 ? 0 : [sin | cos](2 pi ((2 (c + 0.5) inv_size - 1) @ gauss))) + table[label + 1]"""
    c = 2.0 * ((coords.to(ft) + 0.5) * cf(inv_size, ft)) - 1.0
    g = gauss.to(ft)
    a = torch.tensor(2.0 * math.pi, dtype=ft) * (c[:, :1] * g[0][None] + c[:, 1:] * g[1][None])
    pe = torch.where((labels >= 0)[:, None], torch.cat([torch.sin(a), torch.cos(a)], dim=1), torch.zeros((), dtype=ft))
    return pe + table.to(ft)[(labels + 1).long()]


SINE_DIMS = [64, 256]
# two sets, each with its own N: normalised positions as the model passes them, and arguments of sinf to 3e4, where the argument reduction matters and the rounding
# of pos / t alone moves the result by thousands of u
SINE_POS = {"small": torch.tensor([0.0, -0.2, 7.0 / 15.0, 1.0, -0.9375]), "large": torch.tensor([0.0, 1000.0, -30000.7, 12345.678, -777.25])}


def sine_pe_1d(pos, dim, temperature=10000.0, ft=F64):
    """[n] -> [n, dim] = [sin(pos / t_j) | cos(pos / t_j)], t_j = temperature^(2 (j / 2) / (dim / 2))"""
    half = dim // 2
    e = (2 * (torch.arange(half) // 2)).to(F32) / float(half)
    t = torch.pow(cf(temperature, ft), e.to(ft))
    a = pos.to(ft)[:, None] / t[None]
    return torch.cat([torch.sin(a), torch.cos(a)], dim=1)


HYPER = dict(C=32, HW=403, nms=[1, 4, 8])


def hyper_inputs(nm):
    return randn(360 + nm, nm, HYPER["C"]), randn(361 + nm, HYPER["HW"], HYPER["C"])


def hyper_masks(hyper, up, ft=F64, mut=None):
    """masks [nm, HW] = hyper [nm, C] @ up [HW, C]^T; mut "pj_layout": written [p][j]"""
    m = hyper.to(ft) @ up.to(ft).T
    return m.T.contiguous().reshape(m.shape) if mut == "pj_layout" else m


def sam_pick(masks, sel, no_obj):
    """sel[1] ? masks[sel[0]] : no_obj"""
    return masks[int(sel[0])].clone() if int(sel[1]) else torch.full((masks.shape[1],), float(cf(no_obj, F32)), dtype=F32)


HOLES = dict(H=40, W=80)
HOLE_AREAS = [1, 8, 64]


def _spiral(n):
    """a one-pixel-wide spiral corridor in an n x n box (n odd), arms two apart: bool [n, n]"""
    s = np.zeros((n, n), bool)
    y = x = 0
    lo, hi = 0, n - 1
    s[0, 0] = True
    while hi - lo >= 2:
        for dy, dx, stop in ((0, 1, hi), (1, 0, hi), (0, -1, lo), (-1, 0, lo + 2)):
            while (x if dx else y) != stop:
                y, x = y + dy, x + dx
                s[y, x] = True
        lo, hi = lo + 2, hi - 2
        if hi - lo >= 2:          # step into the next ring
            while x != lo:
                x += 1
                s[y, x] = True
    return s


def holes_mask(A_):
    """fp32 [H, W], foreground > 0, background <= 0 (some of it exactly 0), for max_area A_: a straight snake of A_ pixels (its smallest index at one end: A_ - 1
    rounds of propagation) and one of A_ + 1; two segments touching only diagonally with joint area A_ (from 2 on) and A_ + 1; a spiral of more than 64 pixels; a
    hole on the border, one in the corner; scattered small holes"""
    H, W = HOLES["H"], HOLES["W"]
    g = gen(370 + A_)
    m = torch.rand(H, W, generator=g) * 2.5 + 0.5
    bg = torch.zeros(H, W, dtype=torch.bool)
    bg[0, 30:32] = True                                   # on the border, area 2
    bg[2, 2:2 + A_] = True                                # snake of A_
    bg[5, 2:3 + A_] = True                                # snake of A_ + 1
    for row, tot in ((8, A_), (12, A_ + 1)):
        a1 = (tot + 1) // 2
        if tot >= 2:
            bg[row, 2:2 + a1] = True
            bg[row + 1, 2 + a1:2 + tot] = True
    bg[16:31, 2:17] = torch.from_numpy(_spiral(15))
    bg[16:37, 20:79] = torch.rand(21, 59, generator=g) < 0.22
    bg[H - 1, W - 1] = True                               # the corner, area 1
    vals = torch.where(torch.rand(H, W, generator=g) < 0.3, torch.zeros(()), -(torch.rand(H, W, generator=g) * 3.0 + 0.01))
    return torch.where(bg, vals, m)


def fill_holes(mask, max_area, mut=None):
    """8-connected components of (mask <= 0) with at most max_area pixels become 0.1 (scipy.ndimage.label); mut "rows_of_H": the pixels walked as a W x H image"""
    from scipy import ndimage
    H, W = mask.shape
    m = mask.reshape(W, H) if mut == "rows_of_H" else mask
    lab, _ = ndimage.label((m <= 0).numpy(), structure=np.ones((3, 3), dtype=bool))
    small = torch.from_numpy((lab > 0) & (np.bincount(lab.ravel())[lab] <= max_area)).reshape(H, W)
    return torch.where(small, torch.tensor(0.1, dtype=F32), mask)
