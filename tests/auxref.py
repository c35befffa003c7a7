"""Plain restatements of the helper kernels of vv_elem.hip, vv_flow.hip, vv_sam2.hip, vv_deform.hip (raw mode) and the LayerNorms, written from include/vvhip.h
and the comments above the kernels, on the CPU, without the HIP library.

Two kinds.  EXACT kernels are compiled with fp contraction off and use only + - * / min max floor compare: every function below takes `ft`, the type it computes
in; ft = torch.float32 is the restatement the GPU must EQUAL (torch rounds every fp32 operation separately, as the GPU does), ft = torch.float64 is the same formula
in high precision, which tests/test_auxref_cpu.py uses to anchor the fp32 one.  ROUNDED kernels (tanh, exp, sigmoid, GELU, rsqrt, a reduction, or a file where the
compiler may contract) are compared against ft = torch.float64, rounded to h16 exactly where the kernel stores h16:

    |got - ref| <= B = ceil(4 N) u max(1, max |ref|)  (+ 0.5 max |x| 1.5e-7 where an fp32 output went through the Abramowitz-Stegun erf GELU of vv_common.h)

u: unit of the output type; N >= 1: the rounding noise of the same formula evaluated in fp32 on the CPU, in the same unit, measured by tests/test_auxref_cpu.py
(NOISE below fails that file when it goes stale); the factor 4 over it is the fused tests' margin (another summation order, the hardware exp / rcp / rsqrt).

Layouts are the kernels' (NHWC rows).  Mutants (`mut=`) restate an indexing mistake a kernel could make; the CPU test shows each one fails at the test's shapes."""
import math

import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
U = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TD = {"fp16": torch.float16, "bf16": torch.bfloat16}
SENTINEL = 1000.0          # exact in fp32, fp16 and bf16
SENTINEL_INT = 0xA5        # guard value of the integer buffers
ELEM_CAP = 8192 * 256      # threads of the largest grid of vv_elem.hip: an index past it is reached in a second pass of the grid-stride loop
FLOW_CAP = 16384 * 256     # the same for vv_flow.hip
IMAGE_CAP = 16384 * 256    # the same for vv_image.hip (grid_for)
ACT_NONE, ACT_SILU, ACT_RELU, ACT_GELU, ACT_SIGMOID = 0, 1, 2, 4, 5
GELU_ERF_ERR = 1.5e-7      # |error| of the erf approximation in gelu_f (vv_common.h)

# N of every rounded kernel, per output type (test_auxref_cpu.py::test_noise_floor measures them on the GPU test's own inputs; never below 1).
NOISE = {"act:bf16": 0.000, "act:fp16": 0.064, "act:fp32": 1.484, "convex_upsample:fp32": 2.992, "corr_lookup:bf16": 0.000, "corr_lookup:fp16": 0.000, 
         "ctx_split:bf16": 0.000, "ctx_split:fp16": 0.000, "ctx_split:fp32": 0.531, "deform_raw:bf16": 0.168, "deform_raw:fp16": 0.337, 
         "gru_rh:bf16": 0.000, "gru_rh:fp16": 0.033, "gru_update:bf16": 0.000, "gru_update:fp16": 0.245, "gru_update:fp32": 1.366, 
         "layernorm:bf16": 0.000, "layernorm:fp16": 0.122, "layernorm_ex:bf16": 0.256, "layernorm_ex:fp16": 1.000, "layernorm_ex:fp32": 3.600, 
         "layernorm_ex_offset:bf16": 0.500, "layernorm_ex_offset:fp16": 1.000, "layernorm_ex_offset:fp32": 25.668, "mask_mem_sigmoid:bf16": 0.003, 
         "mask_mem_sigmoid:fp16": 0.050, "maskdown_mid:bf16": 0.000, "maskdown_mid:fp16": 0.011, "maskdown_out:bf16": 0.004, 
         "maskdown_out:fp16": 0.056, "silu:fp32": 0.512, "u8_normalize:bf16": 0.000, "u8_normalize:fp16": 0.000}


def cf(v, ft):
    """a C `float` argument in ft"""
    return torch.tensor(float(v), dtype=F32).to(ft)


def r16(x, td):
    """round to the storage type and come back"""
    return x if td is None else x.to(td).to(x.dtype)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bound(key, out_dtype, ref, gelu_x=None, table=None):
    """B for a rounded kernel; key: entry of NOISE (or of `table`, the NOISE of a sibling file); gelu_x: max |x| that went through gelu_f into an fp32 output"""
    k = math.ceil(4 * max(1.0, (NOISE if table is None else table)[key]))
    b = k * U[out_dtype] * max(1.0, ref.abs().max().item())
    if gelu_x is not None and out_dtype == torch.float32:
        b += 0.5 * gelu_x * GELU_ERF_ERR
    return b


def noise_of(v32, v64, out_dtype):
    """N of one evaluation: max |fp32 - fp64| / (u max(1, max |ref|))"""
    return (v32.double() - v64).abs().max().item() / (U[out_dtype] * max(1.0, v64.abs().max().item()))


# ---------------------------------------------------------------------------------------------------------------- vv_elem.hip (exact)
def axpby(x, y, ca, cb, ft=F32):
    return cf(ca, ft) * x.to(ft) + cf(cb, ft) * y.to(ft)


def sched_step(x, eps, z, sa_t, sb_t, c_x0, c_eps, c_z, ft=F32):
    e = eps.to(ft)
    x0 = (x.to(ft) - cf(sb_t, ft) * e) / cf(sa_t, ft)
    v = cf(c_x0, ft) * x0 + cf(c_eps, ft) * e
    return v if z is None else v + cf(c_z, ft) * z.to(ft)


def add_inplace(x, y, ft=F32):
    return x.to(ft) + y.to(ft)


def pad_channels(x, cpad, scale, ft=F32):
    """[rows, cin] -> [rows, cpad] = x * scale, zero beyond cin (the h16 form rounds this once)"""
    out = torch.zeros(x.shape[:-1] + (cpad,), dtype=ft)
    out[..., :x.shape[-1]] = x.to(ft) * cf(scale, ft)
    return out


def split_f32(x, lo_scale, td, ft=F32):
    """-> (hi, lo) in ft, both h16 values: hi = h16(x), lo = h16((x - hi) * lo_scale)"""
    a = x.to(ft)
    hi = r16(a, td)
    return hi, r16((a - hi) * cf(lo_scale, ft), td)


def split3(x, td, ft=F32):
    """[M, C] -> [M, 3C] = [hi | (x - hi) * 2^4 | hi * 2^-10], every group rounded to h16"""
    a = x.to(ft)
    hi = r16(a, td)
    return torch.cat([hi, r16((a - hi) * 16.0, td), r16(hi * 2.0 ** -10, td)], dim=-1)


def decode_blend(dec, w, acc, ft=F32, mut=None):
    """dec [T, HW, ld], w [T], acc [T, HW, 3] -> acc * (1 - w) + clamp(dec / 2 + 0.5, 0, 1) * w"""
    T, HW, _ = dec.shape
    frame = torch.arange(T * HW) // (HW + 1 if mut == "frame_index" else HW)
    wt = w.to(ft)[frame].reshape(T, HW, 1)
    p = (dec[..., :3].to(ft) / 2.0 + 0.5).clamp(0.0, 1.0)
    return acc.to(ft) * (1.0 - wt) + p * wt


def window_average(value, count, ft=F32, mut=None):
    """value [T, per_frame], count [T] -> value / count of its frame"""
    T, per = value.shape
    frame = torch.arange(T * per) // (per + 1 if mut == "frame_index" else per)
    return value.to(ft) / count.to(ft)[frame].reshape(T, per)


def preprocess(frames, mask, ft=F32):
    """u8 [T,H,W,3], mask u8 [T,H,W] -> (img, masked) [T,H,W,8] before the h16 rounding: x / 127.5 - 1, masked = img * (mask > 0 ? 0 : 1), channels 3.. zero"""
    v = torch.zeros(frames.shape[:-1] + (8,), dtype=ft)
    v[..., :3] = frames.to(ft) / 127.5 - 1.0
    keep = torch.where(mask > 0, 0.0, 1.0).to(ft)[..., None]
    return v, v * keep


def brushnet_input(lat, cond, mask, H, W, ft=F32, mut=None):
    """lat, cond [F,h,w,4]; mask u8 [F,H,W] -> [F,h,w,16] = (lat | cond | mask(nearest: floor(y H / h), floor(x W / w)) > 0 | 0 x 7)"""
    Fr, h, w, _ = lat.shape
    ys, xs = (torch.arange(h) * H) // h, (torch.arange(w) * W) // w
    m = mask if mut != "frame_base" else mask[:1].expand_as(mask)
    out = torch.zeros((Fr, h, w, 16), dtype=ft)
    out[..., 0:4], out[..., 4:8] = lat.to(ft), cond.to(ft)
    out[..., 8] = (m[:, ys][:, :, xs] > 0).to(ft)
    return out


# ---------------------------------------------------------------------------------------------------------------- vv_flow.hip (exact)
def avgpool2(x, ft=F32):
    """[N,h,w] -> [N,h//2,w//2]: ((a + b) + (c + d)) * 0.25, an odd last row / column dropped"""
    ho, wo = x.shape[1] // 2, x.shape[2] // 2
    a = x.to(ft)[:, :2 * ho, :2 * wo]
    return ((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + (a[:, 1::2, 0::2] + a[:, 1::2, 1::2])) * 0.25


def raft_flow_prep(coords1, w, h, ft=F32, mut=None):
    """coords1 [M,2] (x, y) over stacked h x w grids -> flow [M,2] = coords1 - (m % w, (m / w) % h)   (h16-rounded into flow8[:, 0:2] and xbuf[:, 254:256])"""
    m = torch.arange(coords1.shape[0])
    gy = (m // w) if mut == "frame_base" else (m // w) % h
    return torch.stack([coords1[:, 0].to(ft) - (m % w).to(ft), coords1[:, 1].to(ft) - gy.to(ft)], dim=1)


def add_flow(coords1, dflow, ft=F32):
    return coords1.to(ft) + dflow[:, :2].to(ft)


def add_relu(a, b, ft=F32):
    return (a.to(ft) + b.to(ft)).clamp_min(0.0)


def _bilinear_zero(img, x, y):
    """img [H,W,C] in the computing type; x, y [n] -> [n,C]: ((1-wx)(1-wy) v00 + wx(1-wy) v01) + (1-wx) wy v10) + wx wy v11, taps outside the image 0"""
    H, W, _ = img.shape
    x0, y0 = torch.floor(x), torch.floor(y)
    wx, wy = (x - x0)[:, None], (y - y0)[:, None]
    x0, y0 = x0.long(), y0.long()

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return torch.where(ok[:, None], img[yy.clamp(0, H - 1), xx.clamp(0, W - 1)], torch.zeros((), dtype=img.dtype))

    a = ((1.0 - wx) * (1.0 - wy)) * tap(y0, x0)
    b = (wx * (1.0 - wy)) * tap(y0, x0 + 1)
    c = ((1.0 - wx) * wy) * tap(y0 + 1, x0)
    d = (wx * wy) * tap(y0 + 1, x0 + 1)
    return ((a + b) + c) + d


def _pixel_grid(H, W, ft):
    i = torch.arange(H * W)
    return (i % W).to(ft), (i // W).to(ft)


def fb_valid(f_ab, f_ba, ft=F32):
    """[H,W,2] x 2 -> (valid u8 [H,W], near bool [H,W]): |f_ab + warp(f_ba, f_ab)|^2 < 0.01 (|f_ab|^2 + |warp f_ba|^2) + 0.5; near: lhs within 8 fp32 ulps of rhs"""
    H, W, _ = f_ab.shape
    xs, ys = _pixel_grid(H, W, ft)
    a = f_ab.reshape(-1, 2).to(ft)
    b = _bilinear_zero(f_ba.to(ft), xs + a[:, 0], ys + a[:, 1])
    dx, dy = a[:, 0] + b[:, 0], a[:, 1] + b[:, 1]
    lhs = dx * dx + dy * dy
    rhs = cf(0.01, ft) * ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1])) + 0.5
    near = (lhs - rhs).abs() <= 8 * U[F32] * torch.maximum(lhs.abs(), rhs.abs())
    return (lhs < rhs).to(torch.uint8).reshape(H, W), near.reshape(H, W)


def prop_fill(cur_t, cur_nb, known_t, known_nb, valid, flow, ft=F32):
    """one sweep step of vv_prop_fill with its commit -> (cur_t', known_t', filled, near): an unknown pixel with a consistent flow whose NEAREST source pixel
    (floor(s + 0.5)) is known takes the bilinear sample of cur_nb; near: s + 0.5 within 8 fp32 ulps of an integer but not on it (the nearest pixel hangs on the rounding)"""
    H, W, _ = cur_t.shape
    xs, ys = _pixel_grid(H, W, ft)
    f = flow.reshape(-1, 2).to(ft)
    sxf, syf = xs + f[:, 0], ys + f[:, 1]
    hx, hy = sxf + 0.5, syf + 0.5
    sx, sy = torch.floor(hx).long(), torch.floor(hy).long()
    dist = lambda v: (v - torch.round(v)).abs()          # 0: exactly on x.5, which fp32 holds and decides as fp64 does (small integers plus a half)
    near = ((dist(hx) > 0) & (dist(hx) <= 8 * U[F32] * hx.abs().clamp_min(1.0))) | ((dist(hy) > 0) & (dist(hy) <= 8 * U[F32] * hy.abs().clamp_min(1.0)))
    inb = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    src_known = inb & (known_nb[sy.clamp(0, H - 1), sx.clamp(0, W - 1)] != 0)
    take = (known_t.reshape(-1) == 0) & (valid.reshape(-1) != 0) & src_known
    warped = _bilinear_zero(cur_nb.to(ft), sxf, syf)
    cur = torch.where(take[:, None], warped, cur_t.reshape(-1, 3).to(ft)).reshape(H, W, 3)
    known = torch.where(take, torch.ones((), dtype=torch.uint8), known_t.reshape(-1)).reshape(H, W)
    return cur, known, take.to(torch.uint8).reshape(H, W), near.reshape(H, W)


def prop_combine(orig, a, b, fa, fb, hole, mean3, ft=F32):
    """[H,W,3] x 3, u8 maps [H,W] x 3, mean3 [3] -> (out u8 [H,W,3], filled u8 [H,W]): mean of both sweeps | the one that filled | mean colour in an unfilled hole |
    the original, then clamp(floor(v + 0.5), 0, 255)"""
    A, B, Hh = (fa != 0)[..., None], (fb != 0)[..., None], (hole != 0)[..., None]
    a, b = a.to(ft), b.to(ft)
    v = torch.where(Hh, mean3.to(ft).expand_as(a), orig.to(ft))
    v = torch.where(B, b, v)
    v = torch.where(A, a, v)
    v = torch.where(A & B, (a + b) * 0.5, v)
    v = torch.floor(v + 0.5).clamp(0.0, 255.0)
    return v.to(torch.uint8), (A | B)[..., 0].to(torch.uint8)


def masked_sum_u8(frame, hole):
    """u8 [n,3], u8 [n] -> int64 [4]: sums of r, g, b over the pixels with hole == 0, and their count"""
    keep = hole.reshape(-1) == 0
    s = frame.reshape(-1, 3)[keep].to(torch.int64).sum(0)
    return torch.cat([s, keep.sum()[None].to(torch.int64)])


def u8_is_zero(x):
    return (x == 0).to(torch.uint8)


def u8_to_f32(x):
    return x.to(F32)


def raft_prep(img, ft=F32):
    """u8 [..., 3] -> [..., 8] = 2 * (x / 255) - 1, channels 3.. zero (before the h16 rounding)"""
    out = torch.zeros(img.shape[:-1] + (8,), dtype=ft)
    out[..., :3] = 2.0 * (img.to(ft) / 255.0) - 1.0
    return out


# ---------------------------------------------------------------------------------------------------------------- vv_sam2.hip (exact)
def select_f32(a, b, flag):
    return a.clone() if int(flag) else b.clone()


def add_rowvec_unless(x, vec, score, ft=F32):
    """x [M,C] += vec [C] unless score > 0: a NaN score adds, as !(score > 0) says"""
    return x.to(ft) if float(score) > 0 else x.to(ft) + vec.to(ft)


def clamp_f32(x, lo, hi, ft=F32):
    return x.to(ft).clamp(cf(lo, ft), cf(hi, ft))


def sam_select(masks, iou, obj_logit, multimask, delta, thresh, ft=F32):
    """masks [nm,HW], iou [nm], obj_logit -> (sel [3], near bool [HW]): stability of mask 0 = #(v > delta) / #(v > -delta) (1 when the union is empty) against thresh;
    sel[0] = multimask or unstable ? the first best-iou mask among 1.. : 0, sel[1] = obj_logit > 0, sel[2] = multimask ? that best mask : 0; near: a value of mask 0
    within 8 fp32 ulps of +-delta but not on it (a value ON the band's edge is not above it, in any precision)"""
    v, d = masks[0].to(ft), cf(delta, ft)
    ai, au = (v > d).sum().to(ft), (v > -d).sum().to(ft)
    stable = bool((ai / au if au > 0 else torch.ones((), dtype=ft)) >= cf(thresh, ft))
    best = 1 + int(torch.argmax(iou[1:]))
    dist = torch.minimum((v - d).abs(), (v + d).abs())
    near = (dist > 0) & (dist <= 8 * U[F32] * d)
    return torch.tensor([best if multimask or not stable else 0, int(float(obj_logit) > 0), best if multimask else 0], dtype=torch.int32), near


SELECT_CASES = [(75, 100, 0.75, True), (74, 100, 0.75, False), (0, 0, 0.98, True), (1003, 1003, 1.0, True), (3, 4, 0.75, True)]      # ai, au, thresh, stable


def sam_select_inputs(HW, ai, au, delta, seed=95):
    """mask 0 with exactly ai values above delta and au above -delta, the others ON the edges of the band (delta and -delta themselves, which count for neither) or
    far below; masks 1.. random"""
    m = randn(seed, 4, HW)
    d = float(cf(delta, F32))
    m[0] = -1.0
    m[0, au::2] = -d
    m[0, :au] = 0.0
    m[0, ai:au:2] = d
    m[0, :ai] = 1.0
    return m[:, torch.randperm(HW, generator=gen(seed + 1))].contiguous()


def mask_mem_input(logits, binarize, scale, bias, ft=F32):
    """-> (m [n] = (binarize ? x > 0 : sigmoid(x)) * scale + bias, near bool [n]: a binarised logit within 8 fp32 ulps of 0, which no finite fp32 logit but 0 is)"""
    v = logits.to(ft)
    m = torch.where(v > 0, 1.0, 0.0).to(ft) if binarize else 1.0 / (1.0 + torch.exp(-v))
    return m * cf(scale, ft) + cf(bias, ft), torch.zeros(v.shape, dtype=torch.bool)


# ---------------------------------------------------------------------------------------------------------------- rounded kernels
def silu(x, ft=F64):
    v = x.to(ft)
    return v / (1.0 + torch.exp(-v))


def act(x, a, ft=F64):
    v = x.to(ft)
    if a == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if a == ACT_RELU:
        return v.clamp_min(0.0)
    if a == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-v))
    if a == ACT_SILU:
        return v / (1.0 + torch.exp(-v))
    return v


def raft_ctx_split(cn, ft=F64):
    """cn [M,256] -> (net = tanh(cn[:, :128]) [M,128], inp = relu(cn[:, 128:]) [M,128])"""
    v = cn.to(ft)
    return torch.tanh(v[:, :128]), v[:, 128:].clamp_min(0.0)


def gru_rh(zr, h, ft=F64):
    return (1.0 / (1.0 + torch.exp(-zr[:, 128:].to(ft)))) * h.to(ft)


def gru_update(zr, q, h, ft=F64):
    z = 1.0 / (1.0 + torch.exp(-zr[:, :128].to(ft)))
    return (1.0 - z) * h.to(ft) + z * torch.tanh(q.to(ft))


def corr_lookup(pyr, coords, ft=F64, mut=None):
    """pyr: 4 x [N, h_l, w_l], coords [N,2] (x, y) -> [N,324]: channel l * 81 + i * 9 + j = plane n of level l sampled at (x / 2^l + i - 4, y / 2^l + j - 4), zeros outside"""
    N = coords.shape[0]
    d = torch.arange(-4, 5).to(ft)
    out = []
    for l, lvl in enumerate(pyr):
        sc = 1.0 / float(1 << l)
        xs = (coords[:, 0].to(ft) * sc)[:, None, None] + d[None, :, None]
        ys = (coords[:, 1].to(ft) * sc)[:, None, None] + d[None, None, :]
        xs, ys = xs.expand(N, 9, 9).reshape(-1), ys.expand(N, 9, 9).reshape(-1)
        hp, wp = lvl.shape[1:]
        n = torch.arange(N).repeat_interleave(81) if mut != "plane_base" else torch.zeros(N * 81, dtype=torch.long)
        x0, y0 = torch.floor(xs), torch.floor(ys)
        wx, wy = xs - x0, ys - y0
        x0, y0 = x0.long(), y0.long()
        p = lvl.to(ft)

        def tap(yy, xx):
            ok = (xx >= 0) & (xx < wp) & (yy >= 0) & (yy < hp)
            return torch.where(ok, p[n, yy.clamp(0, hp - 1), xx.clamp(0, wp - 1)], torch.zeros((), dtype=ft))

        v = ((((1.0 - wx) * (1.0 - wy)) * tap(y0, x0) + (wx * (1.0 - wy)) * tap(y0, x0 + 1)) + ((1.0 - wx) * wy) * tap(y0 + 1, x0)) + (wx * wy) * tap(y0 + 1, x0 + 1)
        out.append(v.reshape(N, 81))
    return torch.cat(out, dim=1)


def convex_upsample(coords1, mask_rows, sel, Fr, h, w, ft=F64, mut=None):
    """coords1 [F*h*w, 2] absolute positions over F stacked h x w grids; mask_rows [len(sel), 576]: the rows `sel` of the mask (logit k * 64 + sy * 8 + sx) ->
    [len(sel), 64, 2]: sub-pixel (sy, sx) of coarse pixel p is sum_k softmax_k(mask) * 8 * (coords1 - grid)(neighbour k of p IN ITS OWN GRID, zero outside)"""
    c = coords1.to(ft).reshape(Fr, h, w, 2)
    gx = torch.arange(w).to(ft)[None, None, :]
    gy = torch.arange(h).to(ft)[None, :, None]
    flow8 = torch.stack([8.0 * (c[..., 0] - gx), 8.0 * (c[..., 1] - gy)], dim=-1)          # [F,h,w,2]
    f, y, x = sel // (h * w), (sel // w) % h, sel % w
    if mut == "frame_base":
        f = torch.zeros_like(f)
    m = torch.softmax(mask_rows.to(ft).reshape(-1, 9, 64), dim=1)                          # [n, 9, 64]
    out = torch.zeros((sel.numel(), 64, 2), dtype=ft)
    for k in range(9):
        yy, xx = y + k // 3 - 1, x + k % 3 - 1
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = torch.where(ok[:, None], flow8[f, yy.clamp(0, h - 1), xx.clamp(0, w - 1)], torch.zeros((), dtype=ft))      # [n, 2]
        out = out + m[:, k, :, None] * v[:, None, :]
    return out


def convex_gather(out, sel, Fr, h, w):
    """the [len(sel), 64, 2] values of an [F, 8h, 8w, 2] output that belong to the coarse pixels sel"""
    return out.reshape(Fr, h, 8, w, 8, 2).permute(0, 1, 3, 2, 4, 5).reshape(Fr * h * w, 64, 2)[sel]


def layernorm_ex(x, gamma, beta, eps, a=ACT_NONE, cpad=None, ft=F64, mut=None):
    """fp32 [M,C] -> [M,cpad]: act(F.layer_norm) in the first C columns, zeros behind; also returns max |x| into the activation (the GELU term of the bound)"""
    M, C = x.shape
    y = F.layer_norm(x.to(ft), (C,), gamma.to(ft), beta.to(ft), float(cf(eps, F64)))
    out = torch.zeros((M, C if cpad is None else cpad), dtype=ft)
    out[:, :C] = act(y, a, ft)
    if mut == "pad_tail" and cpad is not None and cpad > C:
        out[:, -4:] = SENTINEL          # the last padding chunk never written
    return out, y.abs().max().item()


def layernorm(x, gamma, beta, pe, rows_per_frame, ft=F64, mut=None):
    """fp32 [M,C] -> F.layer_norm (eps 1e-5) + pe[row / rows_per_frame]"""
    M, C = x.shape
    y = F.layer_norm(x.to(ft), (C,), gamma.to(ft), beta.to(ft), float(cf(1e-5, F64)))
    if pe is not None:
        rows = torch.arange(M) // (rows_per_frame + 1 if mut == "frame_index" else rows_per_frame)
        y = y + pe.to(ft)[rows.clamp_max(pe.shape[0] - 1)]
    return y


def u8_normalize(img, mean, std, cpad, s2d, ft=F64, mut=None):
    """u8 [H,W,3] -> [(H/s2d)(W/s2d), cpad]: channel (dy * s2d + dx) * 3 + c of block (Y, X) = ((x / 255) - mean[c]) * (1 / std[c]) of pixel (s2d Y + dy, s2d X + dx)"""
    H, W, _ = img.shape
    m = torch.tensor([float(v) for v in mean], dtype=F32).to(ft)
    s = torch.tensor([1.0 / float(v) for v in std], dtype=F32).to(ft)          # the wrapper hands the library 1 / std as a C float
    v = (img.to(ft) / 255.0 - m) * s
    order = (0, 2, 3, 1, 4) if mut == "s2d_order" else (0, 2, 1, 3, 4)          # the mutant: channel (dx * s2d + dy) * 3 + c
    v = v.reshape(H // s2d, s2d, W // s2d, s2d, 3).permute(*order).reshape((H // s2d) * (W // s2d), 3 * s2d * s2d)
    out = torch.zeros((v.shape[0], cpad), dtype=ft)
    out[:, :v.shape[1]] = v
    return out


def deform_raw(x, raw, flow, max_residue, dg, kh=3, kw=3, pad=1, ft=F64, mut=None):
    """x [B,H,W,C]; raw [B*H*W, 3*dg*K] = (o1 | o2 | mask logits) of DeformableAlignment's conv_offset; flow [B*H*W, 2] (dx, dy) or None -> col [B*H*W, K*C] (tap-major):
    offset = max_residue * tanh(cat(o1, o2)) + flow FLIPPED to (dy, dx), mask = sigmoid; sampling by torchvision's rule (oracle/deform_ref.py): a sample at or
    beyond -1 / H / W is 0, neighbours outside the image count as 0.  stride 1, dilation 1."""
    B, H, W, C = x.shape
    K, cpg, M = kh * kw, C // dg, B * H * W
    xf = x.to(ft)
    off = cf(max_residue, ft) * torch.tanh(raw[:, :2 * dg * K].to(ft))
    msk = 1.0 / (1.0 + torch.exp(-raw[:, 2 * dg * K:].to(ft)))
    m = torch.arange(M)
    b, oy, ox = m // (H * W), (m // W) % H, m % W
    col = torch.zeros((M, K, C), dtype=ft)
    for g in range(dg):
        for k in range(K):
            j = g * K + k
            dy, dx = off[:, 2 * j], off[:, 2 * j + 1]
            if flow is not None:
                fy, fx = (flow[:, 1], flow[:, 0]) if mut != "flow_not_flipped" else (flow[:, 0], flow[:, 1])
                dy, dx = dy + fy.to(ft), dx + fx.to(ft)
            py, px = (oy - pad + k // kw).to(ft) + dy, (ox - pad + k % kw).to(ft) + dx
            inside = (py > -1) & (py < H) & (px > -1) & (px < W)
            y0, x0 = torch.floor(py), torch.floor(px)
            lh, lw = (py - y0)[:, None], (px - x0)[:, None]
            y0, x0 = y0.long(), x0.long()
            acc = torch.zeros((M, cpg), dtype=ft)
            for t, wgt in enumerate(((1 - lh) * (1 - lw), (1 - lh) * lw, lh * (1 - lw), lh * lw)):
                yy, xx = y0 + (t >> 1), x0 + (t & 1)
                ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
                v = xf[b, yy.clamp(0, H - 1), xx.clamp(0, W - 1), g * cpg:(g + 1) * cpg]
                acc = acc + torch.where(ok[:, None], wgt * v, torch.zeros((), dtype=ft))
            col[:, k, g * cpg:(g + 1) * cpg] = acc * msk[:, j:j + 1]
    return col.reshape(M, K * C)


# ---- the mask path of the SAM 2 memory encoder ------------------------------------------------------------------------------------------
def _ln_gelu(y, g, be, eps, ft):
    """[n, C] -> GELU(LayerNorm over C); also max |x| into the GELU"""
    z = F.layer_norm(y, (y.shape[1],), g.to(ft), be.to(ft), float(cf(eps, F64)))
    return act(z, ACT_GELU, ft), z.abs().max().item()


def maskdown_input(logits, lo, S, binarize, scale, bias, ft=F64, td_m=None):
    """logits [lo*lo] -> (m [S,S] = (binarize ? v > 0 : sigmoid(v)) * scale + bias of v = F.interpolate(bilinear, align_corners=False) to S x S, near bool [S,S]:
    a binarised v within 8 fp32 ulps (of the largest logit) of 0).  td_m: the layer-by-layer path stores m as h16 (vv_mask_mem_input)"""
    v = F.interpolate(logits.to(ft).reshape(1, 1, lo, lo), size=(S, S), mode="bilinear", align_corners=False)[0, 0]
    near = (v.abs() <= 8 * U[F32] * logits.abs().max().item()) if binarize else torch.zeros_like(v, dtype=torch.bool)
    m = torch.where(v > 0, 1.0, 0.0).to(ft) if binarize else 1.0 / (1.0 + torch.exp(-v))
    return r16(m * cf(scale, ft) + cf(bias, ft), td_m), near


def maskdown_stage(x, w, b, g, be, eps, td, ft=F64):
    """x [H,W,Cin] -> ([ (H/2)(W/2), Cout ] = h16(GELU(LayerNorm2d(conv 3x3 / stride 2 / pad 1))), max |x| into the GELU); w [Cout,Cin,3,3]"""
    y = F.conv2d(x.to(ft).permute(2, 0, 1)[None], w.to(ft), b.to(ft), stride=2, padding=1)[0]
    o, gx = _ln_gelu(y.permute(1, 2, 0).reshape(-1, w.shape[0]), g, be, eps, ft)
    return r16(o, td), gx


def near_outputs(near):
    """[S,S] marks of the conv's input -> [(S/2)^2] marks of the 3x3 / stride 2 / pad 1 outputs that read a marked input"""
    return (F.max_pool2d(near.to(F32)[None, None], 3, stride=2, padding=1)[0, 0] > 0).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- the inputs both test files use
def randn(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen(seed)) * scale


def silu_inputs(n=4099):
    x = randn(1, n, scale=4.0)
    x[:8] = torch.tensor([0.0, -0.0, 30.0, -30.0, 20.0, -20.0, 1e-30, -87.0])
    return x


def raft_rows(seed, M):
    """(cn | zr [M,256], h [M,128], q [M,128]) of the recurrent update"""
    return randn(seed, M, 256, scale=3.0), randn(seed + 1, M, 128), randn(seed + 2, M, 128, scale=3.0)


CORR_SIZES = [(8, 8), (9, 12)]


def corr_inputs(h, w, pairs=2, seed=5):
    """`pairs` stacked pairs: N = pairs * h * w planes of h x w with a 4-level pyramid of independent values, and one lookup position per plane: on the grid, at -4,
    at w + 3.5, at half pixels, then random ones from -6 to w + 6"""
    N = pairs * h * w
    pyr = [randn(seed + l, N, h >> l, w >> l) for l in range(4)]
    coords = (torch.rand(N, 2, generator=gen(seed + 9)) * torch.tensor([w + 12.0, h + 12.0])) - 6.0
    edge = torch.tensor([[3.0, 4.0], [0.0, 0.0], [-4.0, 2.0], [2.0, -4.0], [w + 3.5, 1.5], [1.5, h + 3.5], [2.5, 3.5], [w - 0.5, h - 0.5], [w - 1.0, h - 1.0], [-4.5, -4.5]])
    coords[:len(edge)] = edge
    coords[N // 2:N // 2 + len(edge)] = edge          # the same positions in the second pair, over other planes
    return pyr, coords


def convex_inputs(Fr, h, w, seed=11, with_mask=True):
    """coords1 [F*h*w, 2] (grid + a flow that differs per frame), mask [F*h*w, 576]; row 5 of every frame has one logit 80 above the rest"""
    n = Fr * h * w
    m = torch.arange(n)
    grid = torch.stack([(m % w).float(), ((m // w) % h).float()], dim=1)
    coords1 = grid + randn(seed, n, 2, scale=2.0) + (m // (h * w)).float()[:, None] * 3.0
    if not with_mask:
        return coords1, None
    mask = randn(seed + 1, n, 576)
    for f in range(Fr):
        mask[f * h * w + 5, 4 * 64:5 * 64] += 80.0
    return coords1, mask


def device_mask(n_rows, device):
    """the big convex_upsample mask, made where it is used: logits k / 256 - 2 from an integer hash (exact in fp32, the same on any device)"""
    idx = torch.arange(n_rows * 576, dtype=torch.int64, device=device)
    return (((idx * 7919 + (idx >> 9) * 104729) % 1024).to(F32) * (1.0 / 256.0) - 2.0).reshape(n_rows, 576)


FRAME_T, FRAME_PER = 3, 700001          # window_average / decode_blend: 3 frames whose length does not divide the cap


def window_inputs():
    return randn(1, FRAME_T, FRAME_PER), torch.tensor([1.0, 3.0, 7.0])


def blend_inputs():
    """dec [T, HW, 4], weights 0 / 0.25 / 1, acc [T, HW, 3]"""
    return randn(2, FRAME_T, FRAME_PER, 4, scale=0.8), torch.tensor([0.0, 0.25, 1.0]), torch.rand(FRAME_T, FRAME_PER, 3, generator=gen(3))


BRUSH = dict(T=3, H=700, W=1001, Hm=1050, Wm=1502)          # 2 102 100 pixels: the last frame starts inside the first pass and ends in the second; mask 1.5 x the grid


def brushnet_inputs():
    d = BRUSH
    return (randn(3, d["T"], d["H"], d["W"], 4), randn(4, d["T"], d["H"], d["W"], 4),
            (torch.rand(d["T"], d["Hm"], d["Wm"], generator=gen(5)) < 0.5).to(torch.uint8))


LNX_C = [60, 64, 254, 256, 260, 768, 772, 1280, 1284, 2304, 2308]
LNX_PAD = [0, 4, 252, 256]
LNX_M = 9
LNX_EPS = 1e-6
OUTS = [("fp32", torch.float32), ("h16", None)]
ACT_LIST = [ACT_NONE, ACT_SILU, ACT_RELU, ACT_GELU, ACT_SIGMOID]


def lnx_form(C, cpad):
    """the kernel vv_layernorm_ex launches, restated from its dispatch: NCH of the register-resident form, or 0 for the generic kernel"""
    if C % 4 == 0 and cpad % 4 == 0 and C >= 64 and cpad - C <= 252:
        for nch, top in ((1, 256), (3, 768), (5, 1280), (9, 2304)):
            if C <= top:
                return nch
    return 0


def lnx_cases(C):
    """(cpad, act, out name) of the launches tested at C: the four paddings, every activation and both output kinds over the list of C"""
    i = LNX_C.index(C)
    return [(C + d, ACT_LIST[(i + j) % 5], OUTS[(i + j) % 2][0]) for j, d in enumerate(LNX_PAD)] + [(C + LNX_PAD[(i + 1) % 3], ACT_LIST[(i + 4) % 5], OUTS[(i + 1) % 2][0])]


def ln_inputs(C, M=LNX_M, seed=21, offset=False):
    """x [M,C], gamma, beta; offset: rows of mean 20 and std 1, the last two rows constant (variance 0: the output is beta)"""
    x = randn(seed + C, M, C, scale=2.0)
    if offset:
        x = randn(seed + C, M, C) + 20.0
        x[-2:] = torch.tensor([[3.25], [-20.0]])
    return x, 1.0 + 0.5 * randn(seed + C + 1, C), 0.3 * randn(seed + C + 2, C)


LN_C = [512, 516, 1284, 2048]
ACT_N = [1000, 1003]
ACT_OFFS = [0, 1, 8]          # elements into the allocation: 2 and 16 bytes for h16


ACT_SETS = ["wide", "narrow"]


def act_inputs(n, kind="wide", seed=31):
    """wide: values to +-30 (the tails of exp); narrow: |x| <= 4, where max |ref| is small enough for the h16 bounds to bind on the shape of the function near 0"""
    if kind == "narrow":
        return randn(seed + 1, n, scale=1.5).clamp(-4.0, 4.0)
    x = randn(seed, n, scale=3.0)
    x[:6] = torch.tensor([0.0, -0.0, 12.0, -12.0, 30.0, -30.0])
    return x


DEFORM = dict(B=2, C=32, H=9, W=13, dg=4, max_residue=5.0)


def deform_inputs(seed=41):
    d = DEFORM
    M, K = d["B"] * d["H"] * d["W"], 9
    x = randn(seed, d["B"], d["H"], d["W"], d["C"])
    raw = randn(seed + 1, M, 3 * d["dg"] * K, scale=1.5)
    raw[::7, ::5] = 20.0
    raw[3::7, 1::5] = -20.0
    flow = randn(seed + 2, M, 2, scale=2.5)
    flow[:, 0] += 1.5          # x and y of the flow differ on average: an unflipped flow shows
    return x, raw, flow


MASKDOWN = [(64, 16), (36, 10)]          # (S, lo)
MD_SCALE, MD_BIAS, MD_EPS = 20.0, -10.0, 1e-6


def maskdown_inputs(S, lo, seed=51):
    """logits [lo*lo] (a blob: positive inside, negative outside, smooth in between so that few upsampled values lie near 0), l1 / l2 = (w, b, gamma, beta) with
    weights that bf16 and fp16 hold exactly (the layer-by-layer path packs them as h16)"""
    yy, xx = torch.meshgrid(torch.arange(lo).float(), torch.arange(lo).float(), indexing="ij")
    logits = (6.0 - 1.7 * torch.sqrt((yy - lo / 2.3) ** 2 + (xx - lo / 1.9) ** 2)) + 0.3 * randn(seed, lo, lo)
    q = lambda t: t.to(torch.bfloat16).float()
    l1 = (q(randn(seed + 1, 4, 1, 3, 3, scale=0.3)), randn(seed + 2, 4, scale=0.1), 1.0 + 0.2 * randn(seed + 3, 4), 0.1 * randn(seed + 4, 4))
    l2 = (q(randn(seed + 5, 16, 4, 3, 3, scale=0.3)), randn(seed + 6, 16, scale=0.1), 1.0 + 0.2 * randn(seed + 7, 16), 0.1 * randn(seed + 8, 16))
    return logits.reshape(-1), l1, l2


U8N = [(1, 8), (2, 16), (4, 56)]          # (s2d, cpad): cpad larger than 3 s2d^2
U8N_MEAN, U8N_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def u8_image(H, W, seed=61):
    img = torch.randint(0, 256, (H, W, 3), generator=gen(seed), dtype=torch.uint8)
    img[0, 0], img[0, 1] = 0, 255
    return img


def flow_edge_inputs(H=9, W=13, seed=71):
    """one frame of the propagation kernels at its edges: flows landing exactly on x.5 (the floor(s + 0.5) rounding), on -0.5, on W - 0.5, far outside, and random ones
    -> dict(f_ab, f_ba, cur_t, cur_nb, known_t, known_nb, valid, flow)"""
    n = H * W
    flow = randn(seed, H, W, 2, scale=2.0)
    fl = flow.reshape(n, 2)
    xs, ys = _pixel_grid(H, W, F32)
    fl[0::6, 0] = torch.round(fl[0::6, 0]) + 0.5                      # lands on x.5
    fl[1::6, 1] = torch.round(fl[1::6, 1]) - 0.5
    fl[2::12] = torch.stack([-0.5 - xs[2::12], 0.5 - ys[2::12]], 1)   # source (-0.5, 0.5): floor(0) = 0, in bounds by the rounding
    fl[5::12] = torch.stack([W - 0.5 - xs[5::12], H - 0.5 - ys[5::12]], 1)      # source (W - 0.5, H - 0.5): rounds to W, outside
    fl[8::24] = torch.tensor([500.0, -700.0])
    g = gen(seed + 1)
    known_nb = (torch.rand(H, W, generator=g) < 0.7).to(torch.uint8)
    known_t = (torch.rand(H, W, generator=g) < 0.4).to(torch.uint8)
    valid = (torch.rand(H, W, generator=g) < 0.8).to(torch.uint8)
    f_ab = randn(seed + 2, H, W, 2, scale=1.5)
    f_ba = -f_ab + randn(seed + 3, H, W, 2, scale=0.45)
    f_ab.reshape(n, 2)[4::9] = fl[4::9]
    return dict(f_ab=f_ab, f_ba=f_ba, flow=flow, cur_t=randn(seed + 4, H, W, 3, scale=60.0) + 128.0, cur_nb=randn(seed + 5, H, W, 3, scale=60.0) + 128.0,
                known_t=known_t, known_nb=known_nb, valid=valid)


def combine_inputs(H=9, W=13, seed=81):
    """all four A / B / hole branches, values that round to -1 and 256 before the clamp, and exact x.5 values"""
    g = gen(seed)
    mk = lambda p: (torch.rand(H, W, generator=g) < p).to(torch.uint8)
    fa, fb, hole = mk(0.5), mk(0.5), mk(0.6)
    orig, a, b = (torch.rand(H, W, 3, generator=g) * 255.0 for _ in range(3))
    a.reshape(-1)[0::5], a.reshape(-1)[1::5], a.reshape(-1)[2::5] = -0.75, 255.6, 100.5
    b.reshape(-1)[0::5], b.reshape(-1)[1::5], b.reshape(-1)[2::5] = -0.75, 255.6, 101.5
    orig.reshape(-1)[3::7] = 12.5
    return dict(orig=orig, a=a, b=b, fa=fa, fb=fb, hole=hole, mean3=torch.tensor([100.49999, 0.5, 254.5]))
