"""fp64 host reference of the stages of ProPainter's inpainting generator (videovanish_amd/inpaintgen.py), the cases and inputs of
tests/test_gen_stages_gpu.py, and the mutants that prove the comparison would notice a structural mistake.  Plain torch in float64 on the CPU, in the
torch.roll / F.unfold / F.fold / grouped F.conv2d form of the published architecture: nothing here reads inpaintgen._window_tables, the tap-major permutations or
the dense weight rewrites.  Shared by tests/test_genref_cpu.py and tests/test_gen_stages_gpu.py, not a conftest.

Every stage takes a weight source with the .conv / .linear / .norm interface of oracle.model_ref.Params, the parameter name prefix, fp32 activations as NHWC rows
(frames-major, the product's layout) and the h16 type `td` (torch.float32 = nothing is rounded: the tie to oracle/inpaintgen_ref.py).  Weights are always rounded
to td.  `rounded=True` also rounds the activations fp32 -> td, to nearest even, exactly where the product stores or loads h16; `rounded=False` is the same
arithmetic without those roundings.  Each stage returns (out float64, {name: intermediate}).

Rounding points (the statement of inpaintgen.py / hip.py / deform.py each one restates)
  encoder (inpaintgen._Encoder.__call__)
    layer input               inpaintgen.py 99    hip.conv_gemm(dt, x0 if skip else out, ...): the fp32 gen_input rows are rounded when vv_conv_gemm loads them
    layers 0 .. 7             inpaintgen.py 100   out_dtype = h16 after LeakyReLU(0.2); the last layer stores fp32
  feature_propagation (inpaintgen._FeaturePropagation.__call__, deform.DeformableAlignment)
    warped                    inpaintgen.py 143   hip.deform_im2col (1 x 1 tap, offset = flow) allocates h16 (hip.py 601)
    cond / backbone / fuse    inpaintgen.py 145, 147, 154   fp32 concatenations, rounded when vv_conv_gemm loads them
    offset stack              deform.py 56        three h16 layers (LeakyReLU 0.1), the last one fp32: tanh / sigmoid / + flow in fp32 inside vv_deform_im2col
    deformed columns          deform.py 25        mask * bilinear(x) stored h16; the 1 x 1 GEMM over them stores fp32 (deform.py 27, out_dtype of 58)
    backbone.0 / fuse.0       inpaintgen.py 147, 154   h16 after LeakyReLU(0.2); backbone.2 / fuse.2 add the fp32 residual and store fp32 (148, 155)
  soft_split (InpaintGenerator.soft_split)
    7 x 7 patches             inpaintgen.py 332   hip.deform_im2col allocates h16: the fp32 features are rounded once; the embedding stores fp32 (333)
  attention_half (_TransformerBlock.attention_half)
    norm1                     inpaintgen.py 237   hip.layernorm allocates h16 (hip.py 525); the padding rows are zero rows of it (238)
    q | k | v                 inpaintgen.py 239   self.qkv(xp): _Linear stores h16 (inpaintgen.py 66)
    pooled tokens             inpaintgen.py 243   self.poolw(pcol): the 4 x 4 gather copies h16 (241), the pool GEMM stores h16
    pooled q | k | v          inpaintgen.py 243   self.qkv(...) of the h16 pooled tokens, h16
    P, o                      vv_attention        P = 2^(s - m) rounded before P V, scores and the row sum in fp32; o h16 (inpaintgen.py 249, 256)
    proj                      inpaintgen.py 261   res0 = the fp32 x; fp32
  ffn_half (_TransformerBlock.ffn_half)
    norm2                     inpaintgen.py 266   h16
    fc1                       inpaintgen.py 267   h16, tap-major
    folded grid               inpaintgen.py 268   hip.fold_patches: overlap-add, / count and GELU in fp32, stored h16; the unfold gather copies h16 (269)
    fc2                       inpaintgen.py 270   res0 = the fp32 x; fp32
  soft_comp (InpaintGenerator.soft_comp)
    embedding                 inpaintgen.py 369   self.sc(tok): fp32 tokens rounded at the load, h16 result
    fold                      inpaintgen.py 369   overlap-add in fp32, stored h16
    bias_conv                 inpaintgen.py 370   res0 = the fp32 features; fp32
  decoder (InpaintGenerator.decoder)
    first upsample            inpaintgen.py 376   hip.upsample2x_bilinear keeps the dtype of x (hip.py 625): fp32, rounded when decoder.0 loads it
    decoder.0 / .2 / .4       inpaintgen.py 376-378   h16 after LeakyReLU(0.2); the second upsample interpolates h16 in fp32 and stores h16
    decoder.6                 inpaintgen.py 379   fp32, before tanh
GELU is the exact erf form, LayerNorm eps 1e-5, bilinear x2 with align_corners=True.

Noise floor N = max |ref(rounded) - ref(unrounded)| / (u max(1, max |ref(rounded)|)), u = 2^-11 (fp16) / 2^-8 (bf16), the worst case per (stage, type) over CASES --
measured by tests/test_genref_cpu.py, which fails when NOISE goes stale -- and MARGIN = modref.margin_of(N); the GPU bound is B = MARGIN u max(1, max |ref|)
(every stage output is fp32).
"""
import functools
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fusedref import TD, U, _r, _Rn, _w  # noqa: E402
from modref import margin_of  # noqa: E402

from videovanish_amd.weights import SyntheticWeights  # noqa: E402

LOG2E = 1.4426950408889634
C, HIDDEN, HEADS, WS, POOL, MLP = 128, 512, 4, (5, 9), (4, 4), 1960
K7, S3, P3 = (7, 7), (3, 3), (3, 3)
ENC_SPEC = [(64, 2, 1), (64, 1, 1), (128, 2, 1), (256, 1, 1), (384, 1, 1), (512, 1, 2), (384, 1, 4), (256, 1, 8), (128, 1, 1)]
STAGES = ("encoder", "feature_propagation", "soft_split", "attention_half", "ffn_half", "block", "soft_comp", "decoder")

# measured noise floors, worst case per (stage, type) over CASES: tests/test_genref_cpu.py::test_noise_floor_and_margin
NOISE = {
    ("encoder", "fp16"): 0.757, ("encoder", "bf16"): 0.745,
    ("feature_propagation", "fp16"): 0.323, ("feature_propagation", "bf16"): 0.346,
    ("soft_split", "fp16"): 0.293, ("soft_split", "bf16"): 0.403,
    ("attention_half", "fp16"): 0.700, ("attention_half", "bf16"): 0.629,
    ("ffn_half", "fp16"): 0.471, ("ffn_half", "bf16"): 0.492,
    ("block", "fp16"): 0.955, ("block", "bf16"): 0.751,
    ("soft_comp", "fp16"): 0.974, ("soft_comp", "bf16"): 1.057,
    ("decoder", "fp16"): 1.571, ("decoder", "bf16"): 1.635,
}


def token_grid(h, w):
    return (h - 1) // 3 + 1, (w - 1) // 3 + 1


def _nchw(x, Fr, H, W):
    return x.view(Fr, H, W, -1).permute(0, 3, 1, 2)


def _rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def _conv(P, name, x, Fr, H, W, cout, td, stride=1, groups=1, gain=1.0):
    """rows [Fr * H * W, cin] -> rows: 3 x 3 convolution, padding 1, weights rounded to td"""
    w, b = P.conv(name, x.shape[1] // groups, cout, 3, gain)
    y = F.conv2d(_nchw(x, Fr, H, W), _w(w, td), b.double(), stride=stride, padding=1, groups=groups)
    return _rows(y), y.shape[2], y.shape[3]


def _lin(P, name, x, cout, td):
    w, b = P.linear(name, x.shape[-1], cout)
    return x @ _w(w, td).t() + b.double()


def _ln(P, name, x):
    g, b = P.norm(name, x.shape[-1])
    mean, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    return (x - mean) * torch.rsqrt(var + 1e-5) * g.double() + b.double()


def _lrelu(x, s=0.2):
    return F.leaky_relu(x, s)


# ---------------------------------------------------------------------------------------------------------------------------
def encoder(P, name, x, Fr, H, W, td, rounded=True, mut=None):
    """x [Fr * H * W, 5] (masked frame | mask_in | mask_updated) -> ([Fr * (H / 4) * (W / 4), 128], intermediates)"""
    on, it = rounded, {}
    out, x0 = _r(x.double(), td, on), None
    for li, (co, s, g) in enumerate(ENC_SPEC):
        i = 2 * li
        if i == 8 and mut != "x0_one_layer_late":
            x0 = out
        if i > 8:
            if x0 is None:          # (the mutant) the skip feature taken after layer 8 instead of before it: the first 256 of its 384 channels
                x0 = out[:, :256]
            if mut == "plain_concatenation":
                out = torch.cat([x0, out], 1)
            else:
                n = out.shape[0]
                out = torch.cat([x0.view(n, g, -1), out.view(n, g, -1)], 2).reshape(n, -1)
        out, H, W = _conv(P, f"{name}.layers.{i}", out, Fr, H, W, co, td, s, g)
        out = _r(_lrelu(out), td, on and li < len(ENC_SPEC) - 1)
        it[f"layer{i}"] = out
    return out, it


# ---------------------------------------------------------------------------------------------------------------------------
def _flow_warp(x, flow):
    """x [B, C, H, W], flow [B, 2, H, W] (dx, dy): zero-padded bilinear sample at p + flow"""
    from oracle.deform_ref import bilinear_zero
    H, W = x.shape[-2:]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=x.dtype), torch.arange(W, dtype=x.dtype), indexing="ij")
    return bilinear_zero(x, ys[None, None] + flow[:, 1:2], xs[None, None] + flow[:, 0:1])


def fb_valid(fp, fc):
    """forward-backward consistency of fp against fc: ([1, 1, H, W] of 0 / 1, the slack a1 mag + a2 - |d|^2 whose sign decides)"""
    wb = _flow_warp(fc, fp)
    d = fp + wb
    mag = (fp ** 2).sum(1, keepdim=True) + (wb ** 2).sum(1, keepdim=True)
    slack = 0.01 * mag + 0.5 - (d ** 2).sum(1, keepdim=True)
    return (slack > 0).to(fp.dtype), slack


def feature_propagation(P, name, x, flows_f, flows_b, masks2, T, H, W, td, rounded=True, mut=None, deform_groups=16):
    """x [T * H * W, C]; flows [T - 1, H, W, 2] (dx, dy) at this resolution; masks2 [T * H * W, 2] -> ([T * H * W, C], intermediates)"""
    from oracle.deform_ref import deform_columns
    on, it, HW = rounded, {}, H * W
    Cc = x.shape[1]
    xd = x.double()
    ff = flows_f.double().permute(0, 3, 1, 2)
    fb = flows_b.double().permute(0, 3, 1, 2)
    mk = _nchw(masks2.double(), T, H, W)
    rows = lambda z: _rows(z)
    feats = {"input": [_nchw(xd[i * HW:(i + 1) * HW], 1, H, W) for i in range(T)]}
    cache = ["input", "backward_1", "forward_1"]
    slack_min = float("inf")
    for p_i, mod in enumerate(("backward_1", "forward_1")):
        feats[mod] = []
        if mod == "backward_1":
            frame_idx = list(range(T))[::-1]
            flow_idx = frame_idx
            f_prop, f_check = ff, fb
        else:
            frame_idx = list(range(T))
            flow_idx = list(range(-1, T - 1))
            f_prop, f_check = fb, ff
        if mut == "flows_exchanged":
            f_prop, f_check = f_check, f_prop
        src = "input" if (mut == "forward_reads_input") else cache[p_i]
        prop = None
        for i, idx in enumerate(frame_idx):
            cur, mcur = feats[src][idx], mk[idx:idx + 1]
            if i == 0:
                prop = cur
            else:
                fi = flow_idx[i]
                if mut == "flow_index_off_by_one":
                    assert T >= 3, "with one flow (T = 2) the neighbouring index wraps onto the same flow: assign this mutant to a case with l_t >= 3"
                    fi = (fi + 1) % (T - 1)
                fp, fc = f_prop[fi:fi + 1], f_check[fi:fi + 1]
                valid, slack = fb_valid(fp, fc)
                slack_min = min(slack_min, slack.abs().min().item())
                if mut == "validity_inverted":
                    valid = 1.0 - valid
                fw_ = fp if mut != "flow_not_flipped" else fp.flip(1)
                warped = _r(_flow_warp(prop, fw_), td, on)
                h = _r(torch.cat([cur, warped, fp, valid, mcur], 1), td, on)
                an = f"{name}.deform_align.{mod}"
                for j, co in enumerate([Cc, Cc, Cc, 27 * deform_groups]):
                    hr, _, _ = _conv(P, f"{an}.conv_offset.{2 * j}", rows(h), 1, H, W, co, td, gain=0.1 if j == 3 else 1.0)
                    h = _nchw(hr, 1, H, W)
                    if j < 3:
                        h = _r(_lrelu(h, 0.1), td, on)
                o1, o2, m = torch.chunk(h, 3, dim=1)
                offset = 3.0 * torch.tanh(torch.cat([o1, o2], 1))
                offset = offset + (fp.flip(1) if mut != "flow_not_flipped" else fp).repeat(1, offset.shape[1] // 2, 1, 1)
                col = _r(deform_columns(prop, offset, torch.sigmoid(m), 3, 3, 1, 1, 1, deform_groups), td, on)
                w, b = P.conv(an, Cc, Cc, 3)
                prop = torch.einsum("ok,bkyx->boyx", _w(w, td).permute(0, 2, 3, 1).reshape(Cc, 9 * Cc), col) + b.double().view(1, -1, 1, 1)
            feat = _r(torch.cat([cur, prop, mcur], 1), td, on)
            hr, _, _ = _conv(P, f"{name}.backbone.{mod}.0", rows(feat), 1, H, W, Cc, td)
            hr = _r(_lrelu(hr), td, on)
            prop = prop + _nchw(_conv(P, f"{name}.backbone.{mod}.2", hr, 1, H, W, Cc, td)[0], 1, H, W)
            feats[mod].append(prop)
        if mod == "backward_1" and mut != "backward_not_reversed":
            feats[mod] = feats[mod][::-1]
    ob, of = torch.cat(feats["backward_1"], 0), torch.cat(feats["forward_1"], 0)
    it["backward"], it["forward"] = rows(ob), rows(of)
    it["min |validity slack|"] = torch.tensor(slack_min)
    hr, _, _ = _conv(P, f"{name}.fuse.0", rows(_r(torch.cat([ob, of, mk], 1), td, on)), T, H, W, Cc, td)
    hr = _r(_lrelu(hr), td, on)
    out = _conv(P, f"{name}.fuse.2", hr, T, H, W, Cc, td)[0] + xd
    return out, it


# ---------------------------------------------------------------------------------------------------------------------------
def _tap_major(cm, ch):
    """patch vectors [..., ch * 49] channel-major (F.unfold's c * 49 + k) -> tap-major (k * ch + c)"""
    return cm.reshape(*cm.shape[:-1], ch, 49).transpose(-1, -2).reshape(cm.shape)


def _channel_major(tm, ch):
    return tm.reshape(*tm.shape[:-1], 49, ch).transpose(-1, -2).reshape(tm.shape)


def soft_split(P, name, x, t, h, w, td, rounded=True, mut=None, hidden=HIDDEN):
    """x [t * h * w, C] -> (tokens [t * fh * fw, hidden], intermediates)"""
    col = F.unfold(_nchw(_r(x.double(), td, rounded), t, h, w), K7, stride=S3, padding=P3).permute(0, 2, 1)        # [t, n, C * 49] channel-major
    col = col.reshape(-1, col.shape[-1])
    if mut == "tap_major_omitted":          # tap-major patches against the published (channel-major) columns of the weights
        col = _tap_major(col, x.shape[1])
    return _lin(P, f"{name}.embedding", col, hidden, td), {"patches": col}


def soft_comp(P, name, tok, enc, t, h, w, td, rounded=True, mut=None):
    """tok [t * fh * fw, hidden], enc [t * h * w, C] -> (enc + bias_conv(fold(embedding(tok))), intermediates)"""
    on, Cc = rounded, enc.shape[1]
    feat = _r(_lin(P, f"{name}.embedding", _r(tok.double(), td, on), 49 * Cc, td), td, on)
    if mut == "tap_major_omitted":          # the published (channel-major) rows read as tap-major by the fold
        feat = _channel_major(feat, Cc)
    grid = F.fold(feat.view(t, -1, 49 * Cc).permute(0, 2, 1), (h, w), K7, stride=S3, padding=P3)
    grid = _r(_rows(grid), td, on)
    out = _conv(P, f"{name}.bias_conv", grid, t, h, w, Cc, td)[0] + enc.double()
    return out, {"embedding": feat, "fold": grid}


# ---------------------------------------------------------------------------------------------------------------------------
def _attn(q, k, v, heads, td, on, key_ok=None, d_major=False):
    """softmax(q k^T / sqrt(D)) v per head in the log2 domain: q [B, Nq, c], k / v [B, Nk, c] (float64 holding h16 values) -> R(o) [B, Nq, c]; key_ok [B, Nk] bool"""
    B, Nq, c = q.shape
    D = c // heads

    def split(z):
        if d_major:
            return z.reshape(z.shape[0], z.shape[1], D, heads).permute(0, 3, 1, 2)
        return z.reshape(z.shape[0], z.shape[1], heads, D).transpose(1, 2)
    s = (split(q) @ split(k).transpose(-1, -2)) * (float(D) ** -0.5 * LOG2E)
    if key_ok is not None:
        s = s.masked_fill(~key_ok[:, None, None, :], float("-inf"))
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    o = _r((_r(p, td, on) @ split(v)) / p.sum(-1, keepdim=True), td, on)
    return (o.permute(0, 2, 3, 1) if d_major else o.transpose(1, 2)).reshape(B, Nq, c)


def _partition(a, ws):
    """[t, nh, nw, c] -> [nwin, t, wh * ww, c]"""
    t, nh, nw, c = a.shape
    a = a.view(t, nh // ws[0], ws[0], nw // ws[1], ws[1], c).permute(1, 3, 0, 2, 4, 5)
    return a.reshape(-1, t, ws[0] * ws[1], c)


def rolled_valid_index(ws):
    e = tuple((i + 1) // 2 for i in ws)
    m_tl = torch.ones(ws); m_tl[:-e[0], :-e[1]] = 0
    m_tr = torch.ones(ws); m_tr[:-e[0], e[1]:] = 0
    m_bl = torch.ones(ws); m_bl[e[0]:, :-e[1]] = 0
    m_br = torch.ones(ws); m_br[e[0]:, e[1]:] = 0
    return torch.stack((m_tl, m_tr, m_bl, m_br), 0).flatten().nonzero(as_tuple=False).view(-1), e


def window_hole_mask(mask, nh, nw, ws):
    """mask bool [frames, fh, fw] (the hole mask on the token grid) -> bool [nwin]: the window touches a hole in one of the frames"""
    m = F.pad(mask.double(), (0, nw - mask.shape[2], 0, nh - mask.shape[1]))
    return F.max_pool2d(m[:, None], ws, ws).sum(0).reshape(-1) > 0


def attention_half(P, name, x, t, fh, fw, mask, l_t, parity, td, rounded=True, mut=None, t_dilation=2, heads=HEADS, ws=WS, pool=POOL):
    """one block up to proj + residual.  x [t * fh * fw, c] (the fp32 residual stream); mask bool [t, fh, fw]: the hole mask of every frame on the token grid, of
    which the l_t local ones classify the windows; parity: the block index mod t_dilation -> (out [t * fh * fw, c], intermediates)"""
    on, c, it = rounded, x.shape[1], {}
    wh, ww = ws
    L = wh * ww
    xd = x.double()
    n_wh, n_ww = math.ceil(fh / wh), math.ceil(fw / ww)
    nh, nw = n_wh * wh, n_ww * ww
    y = _r(_ln(P, f"{name}.norm1", xd), td, on).view(t, fh, fw, c)
    it["norm1"] = y.reshape(-1, c)
    yp = F.pad(y, (0, 0, 0, nw - fw, 0, nh - fh))
    an = f"{name}.attention"
    q, k, v = (_r(_lin(P, f"{an}.{nm}", yp, c, td), td, on) for nm in ("query", "key", "value"))
    real = torch.zeros(t, nh, nw, 1, dtype=torch.bool)
    real[:, :fh, :fw] = True
    win_q, win_k, win_v, win_ok = _partition(q, ws), _partition(k, ws), _partition(v, ws), _partition(real, ws)
    valid, e = rolled_valid_index(ws)
    if mut == "corner_masks_dropped":
        valid = torch.arange(4 * L)
    shifts = [(-e[0], -e[1]), (-e[0], e[1]), (e[0], -e[1]), (e[0], e[1])]
    if mut == "corners_exchanged":
        shifts[1], shifts[2] = shifts[2], shifts[1]
    if mut == "rolls_negated":
        shifts = [(-a, -b) for a, b in shifts]
    roll = lambda a: torch.cat([_partition(torch.roll(a, shifts=sh, dims=(1, 2)), ws) for sh in shifts], 2)[:, :, valid]
    win_k, win_v, win_ok = torch.cat([win_k, roll(k)], 2), torch.cat([win_v, roll(v)], 2), torch.cat([win_ok, roll(real)], 2)
    # pooled (global) tokens: the depth-wise 4 x 4 convolution of the padded normalised tokens, then the key / value projections
    pw, pb = P.conv(f"{an}.pool_layer", 1, c, pool[0], 1.0)
    pw = _w(pw, td)
    if mut == "pool_taps_transposed":
        pw = pw.transpose(-1, -2)
    src = y if mut == "pooled_from_unpadded" else yp
    px = _r(F.conv2d(src.permute(0, 3, 1, 2), pw, pb.double(), stride=pool, groups=c).permute(0, 2, 3, 1), td, on)          # [t, ph, pw, c]
    it["pooled"] = px.reshape(-1, c)
    npool = px.shape[1] * px.shape[2]
    pk, pv = (_r(_lin(P, f"{an}.{nm}", px, c, td), td, on).reshape(t, npool, c) for nm in ("key", "value"))
    par = (parity + 1) % t_dilation if mut == "T_ind_other_parity" else parity
    T_ind = list(range(par, t, t_dilation))
    T_pool = list(range(t)) if mut == "pooled_all_frames" else T_ind
    nwin = n_wh * n_ww
    mw = window_hole_mask(mask if mut == "mask_from_all_frames" else mask[:l_t], nh, nw, ws)
    if mut == "masked_as_clean":
        mw = torch.zeros_like(mw)
    if mut == "clean_as_masked":
        mw = torch.ones_like(mw)
    it["masked windows"] = mw
    out = torch.zeros(nwin, t, L, c, dtype=torch.float64)
    mi, ui = mw.nonzero().view(-1), (~mw).nonzero().view(-1)
    if len(mi):
        nm = len(mi)
        kt = torch.cat([win_k[mi][:, T_ind].reshape(nm, -1, c), pk[T_pool].reshape(1, -1, c).expand(nm, -1, -1)], 1)
        vt = torch.cat([win_v[mi][:, T_ind].reshape(nm, -1, c), pv[T_pool].reshape(1, -1, c).expand(nm, -1, -1)], 1)
        ok = None
        if mut == "padding_keys_dropped":
            ok = torch.cat([win_ok[mi][:, T_ind].reshape(nm, -1), torch.ones(nm, len(T_pool) * npool, dtype=torch.bool)], 1)
        out[mi] = _attn(win_q[mi].reshape(nm, t * L, c), kt, vt, heads, td, on, ok, mut == "heads_d_major").view(nm, t, L, c)
    if len(ui):
        nu = len(ui)
        f = lambda a: a[ui][:, :, :L].reshape(nu * t, L, c)
        out[ui] = _attn(f(win_q), f(win_k), f(win_v), heads, td, on, None, mut == "heads_d_major").view(nu, t, L, c)
    o = out.view(n_wh, n_ww, t, wh, ww, c).permute(2, 0, 3, 1, 4, 5).reshape(t, nh, nw, c)[:, :fh, :fw].reshape(-1, c)
    it["attention"] = o
    return _lin(P, f"{an}.proj", o, c, td) + xd, it


def ffn_half(P, name, x, t, fh, fw, h, w, td, rounded=True, mut=None, hidden=MLP):
    """norm2 through fc2 + residual.  x [t * fh * fw, c] -> (out, intermediates)"""
    on, c, ch, it = rounded, x.shape[1], hidden // 49, {}
    xd = x.double()
    y = _r(_ln(P, f"{name}.norm2", xd), td, on)
    hm = _r(_lin(P, f"{name}.mlp.fc1.0", y, hidden, td), td, on)          # [n, ch * 49] channel-major, as published
    if mut == "fc1_channel_major":          # the fold reads the unpermuted rows as tap-major
        hm = _channel_major(hm, ch)
    it["fc1"] = hm
    fold = lambda z: F.fold(z.view(t, fh * fw, -1).permute(0, 2, 1), (h, w), K7, stride=S3, padding=P3)
    norm = fold(torch.ones(t * fh * fw, 49, dtype=torch.float64))
    g = fold(hm)
    if mut == "overlap_not_divided":
        g = F.gelu(g)
    elif mut == "gelu_before_normalisation":
        g = F.gelu(g) / norm
    else:
        g = F.gelu(g / norm)          # GELU on the grid: it commutes with the unfold gather (tests/test_genref_cpu.py)
    g = _r(g, td, on)
    it["grid"] = _rows(g)
    hc = F.unfold(g, K7, stride=S3, padding=P3).permute(0, 2, 1).reshape(-1, hidden)
    return _lin(P, f"{name}.mlp.fc2.1", hc, c, td) + xd, it


def block(P, name, x, t, fh, fw, h, w, mask, l_t, parity, td, rounded=True, mut=None):
    a, it = attention_half(P, name, x, t, fh, fw, mask, l_t, parity, td, rounded, mut)
    out, it2 = ffn_half(P, name, a, t, fh, fw, h, w, td, rounded, mut)
    return out, {**it, "attention_half": a, **it2}


# ---------------------------------------------------------------------------------------------------------------------------
def decoder(P, name, x, l_t, h, w, td, rounded=True, mut=None):
    """x [l_t * h * w, C] -> (the raw prediction [l_t * 4h * 4w, 3], before tanh; intermediates)"""
    on, it = rounded, {}
    ac = mut != "align_corners_false"
    up = lambda z, hh, ww: _rows(F.interpolate(_nchw(z, l_t, hh, ww), scale_factor=2, mode="bilinear", align_corners=ac))
    z = _r(up(x.double(), h, w), td, on)
    it["d0"] = z = _r(_lrelu(_conv(P, f"{name}.0.conv", z, l_t, 2 * h, 2 * w, 128, td)[0]), td, on)
    it["d2"] = z = _r(_lrelu(_conv(P, f"{name}.2", z, l_t, 2 * h, 2 * w, 64, td)[0]), td, on)
    z = _r(up(z, 2 * h, 2 * w), td, on)
    it["d4"] = z = _r(_lrelu(_conv(P, f"{name}.4.conv", z, l_t, 4 * h, 4 * w, 64, td)[0]), td, on)
    return _conv(P, f"{name}.6", z, l_t, 4 * h, 4 * w, 3, td)[0], it


# ---------------------------------------------------------------------------------------------------------------------------
# Cases: geometry x (t, l_t) x mask layout x parity; each item of the issue's lists occurs at least once.
#   a 80 x 144: 7 x 12 tokens, 2 x 2 windows on a 10 x 18 grid (padding both ways, 10 % 4 != 0), pooled 2 x 4
#   b 48 x 96:  4 x 8 tokens, one window (5 x 9): every roll wraps onto the window itself, pooled 1 x 2
#   c 56 x 208: 5 x 18 tokens, 1 x 2 windows, no padding, pooled 1 x 4
#   d 128 x 112: 11 x 10 tokens, 3 x 2 windows on 15 x 18, pooled 3 x 4 (the pooled grid drops three rows)
GEOM = {"a": (80, 144), "b": (48, 96), "c": (56, 208), "d": (128, 112)}
CASES = [
    dict(g="a", t=5, l_t=3, layout="mixed", parity=0),
    dict(g="a", t=5, l_t=3, layout="ref_only", parity=1),
    dict(g="b", t=2, l_t=2, layout="all", parity=1),           # parity 1 of t = 2: the masked windows see one key frame
    dict(g="b", t=4, l_t=4, layout="none", parity=0),
    dict(g="c", t=4, l_t=4, layout="mixed", parity=1),
    dict(g="d", t=2, l_t=2, layout="mixed", parity=0),
    dict(g="d", t=5, l_t=3, layout="all", parity=1),
    # the validity bit is one of 261 conditioning channels of the seeded offset stack: inverted, it moves the result by less than the bf16 bound.  This case draws
    # that channel's weights 30 times larger (LoudValidity)
    dict(g="b", t=2, l_t=2, layout="mixed", parity=0, weights="loud_validity"),
]
REF_FRAMES_CASE = 0          # the case of the composition's mutant "reference_frames_propagated" (t > l_t)
SEED = 21          # the weight seed of the cases


def dims(cs):
    H, W = GEOM[cs["g"]]
    h, w = H // 4, W // 4
    return H, W, h, w, *token_grid(h, w)


def hole_masks(cs):
    """bool [t, h, w]: the 1/4-resolution hole masks.  mixed: a hole whose last token column / row is the last one of window (0, 0) -- pixel x <= 23 marks token 8
    ([21, 27]) and not token 9 ([24, 30]); pixel y <= 11 marks token 4 and not token 5 -- moving from frame to frame inside that window"""
    _, _, h, w, _, _ = dims(cs)
    m = torch.zeros(cs["t"], h, w, dtype=torch.bool)
    if cs["layout"] == "mixed":
        for f in range(cs["l_t"]):
            m[f, 4 + f:min(12, h), 10 + 2 * f:24] = True
    elif cs["layout"] == "all":
        m[0] = True
    elif cs["layout"] == "ref_only":
        m[cs["l_t"], 4:12, 10:24] = True
    return m


def token_mask(m):
    """the 7 / 3 / 3 max pool of the 1/4-resolution masks: bool [t, fh, fw]"""
    return F.max_pool2d(m.double()[:, None], K7, S3, P3)[:, 0] > 0


def make_flows(rn, n, H, W):
    """completed flows [n, H, W, 2] (dx, dy) at full resolution, forward and backward: whole-pixel differences from frame to frame, x and y of different size,
    sub-pixel parts, vectors that leave the frame near the borders, and no mirror symmetry: the backward flow answers the forward one only on the left half, so the
    right half fails the forward-backward check in both orders"""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ff, fb = [], []
    for i in range(n):
        f = torch.stack([4.0 * (i + 1) + 0.37 + 0.02 * yy, -8.0 * (i + 1) + 0.61 + 0.01 * xx], -1) + 0.1 * rn(H, W, 2)
        b = -f + 0.1 * rn(H, W, 2)
        b[:, W // 2:, 0] += 12.0 + 4.0 * i
        b[:, W // 2:, 1] -= 8.0
        ff.append(f)
        fb.append(b)
    return torch.stack(ff), torch.stack(fb)


def flow_down4(f):
    return F.interpolate(f.permute(0, 3, 1, 2), scale_factor=0.25, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous() / 4.0


class LoudValidity(SyntheticWeights):
    """the seeded weights with the validity channel (2 C + 2 of [current | warped | flow | valid | masks]) of the first offset convolutions 30 times larger; also a
    Ctx(weights=) source"""

    def conv(self, name, cin, cout, k, gain=1.0):
        w, b = super().conv(name, cin, cout, k, gain)
        if name.endswith(".conv_offset.0"):
            w = w.clone()
            w[:, 2 * C + 2] *= 30.0
        return w, b


@functools.lru_cache(maxsize=None)
def _params(weights=None):
    from oracle.model_ref import Params
    P = Params(SEED)
    if weights == "loud_validity":
        P.src = LoudValidity(SEED)
    return P


@functools.lru_cache(maxsize=None)
def raw_inputs(case):
    """the generator's own inputs of one case: frames u8 [t, H, W, 3], masks u8 [t, H, W] x 2 (constant over each 4 x 4 cell), flows fp32 [l_t - 1, H, W, 2] x 2"""
    cs = CASES[case]
    H, W, h, w, _, _ = dims(cs)
    rn = _Rn(4000 + case)
    frames = torch.randint(0, 256, (cs["t"], H, W, 3), generator=rn.g, dtype=torch.uint8)
    m = hole_masks(cs)
    m_in = (m.repeat_interleave(4, 1).repeat_interleave(4, 2)).to(torch.uint8) * 255
    m_up = m_in.clone()
    m_up[:, ::8] = 0
    ff, fb = make_flows(rn, cs["l_t"] - 1, H, W)
    return dict(frames=frames, m_in=m_in, m_up=m_up, ff=ff, fb=fb, m4=m)


def chain(case, td, rounded=True, mut=None, stage_mut=None, depths=1, upto=None, parity0=None, inp=None, cs=None, base=None):
    """the stages composed: every stage runs on the output of the one before.  mut applies to stage `stage_mut` (None: to every stage that knows it).
    Block d runs at parity (parity0 + d) % 2, parity0 = the case's own unless given (the generator starts at 0).
    inp / cs: inputs and geometry of another clip than the case's (a dict like raw_inputs' and one like a row of CASES).
    -> {stage: (input dict, out, intermediates)}, plus "features": what enters the soft split, and "raw": the prediction before tanh"""
    cs, inp = CASES[case] if cs is None else cs, raw_inputs(case) if inp is None else inp
    P = _params(cs.get("weights"))
    H, W, h, w, fh, fw = dims(cs)
    t, l_t, hw = cs["t"], cs["l_t"], h * w
    m_of = lambda st: mut if (stage_mut in (None, st)) else None
    res = {}
    if base is not None and stage_mut not in (None, "encoder", "feature_propagation"):          # the stages before the mutated one: taken from the unmutated run
        res = {k: base[k] for k in ("encoder", "feature_propagation", "features")}
        return _chain_tail(res, res["features"], cs, inp, P, td, rounded, m_of, depths, parity0)
    x5 = torch.cat([inp["frames"].float().reshape(-1, 3) / 127.5 - 1.0, (inp["m_in"] > 0).float().reshape(-1, 1), (inp["m_up"] > 0).float().reshape(-1, 1)], 1)
    enc, it = encoder(P, "gen.encoder", x5, t, H, W, td, rounded, m_of("encoder"))
    res["encoder"] = (dict(x=x5), enc, it)
    if upto == "encoder":
        return res
    m_in4, m_up4 = inp["m4"], (inp["m_up"] > 0)[:, ::4, ::4]
    masks2 = torch.stack([m_in4[:l_t], m_up4[:l_t]], -1).float().reshape(l_t * hw, 2)
    f4, b4 = flow_down4(inp["ff"]), flow_down4(inp["fb"])
    fmut = m_of("feature_propagation")
    lt_p = t if fmut == "reference_frames_propagated" else l_t
    pin = dict(x=enc[:lt_p * hw].float(), ff=f4, fb=b4, masks2=masks2)
    if fmut == "reference_frames_propagated":          # the clip's remaining frames walk along, with the last flow and mask repeated
        rep = lambda z, n: torch.cat([z] + [z[-1:]] * n, 0)
        pin = dict(x=pin["x"], ff=rep(f4, t - l_t), fb=rep(b4, t - l_t), masks2=rep(masks2.view(l_t, hw, 2), t - l_t).reshape(-1, 2))
    local, it = feature_propagation(P, "gen.feat_prop_module", pin["x"], pin["ff"], pin["fb"], pin["masks2"], lt_p, h, w, td, rounded,
                                    None if fmut == "reference_frames_propagated" else fmut)
    res["feature_propagation"] = (pin, local, it)
    enc = torch.cat([local, enc[lt_p * hw:]], 0)
    res["features"] = enc
    if upto == "feature_propagation":
        return res
    return _chain_tail(res, enc, cs, inp, P, td, rounded, m_of, depths, parity0)


def _chain_tail(res, enc, cs, inp, P, td, rounded, m_of, depths, parity0):
    H, W, h, w, fh, fw = dims(cs)
    t, l_t, hw = cs["t"], cs["l_t"], h * w
    tok, it = soft_split(P, "gen.ss", enc.float(), t, h, w, td, rounded, m_of("soft_split"))
    res["soft_split"] = (dict(x=enc.float()), tok, it)
    tmask = token_mask(inp["m4"])
    for d in range(depths):
        par = ((cs["parity"] if parity0 is None else parity0) + d) % 2
        bn = f"gen.transformers.transformer.{d}"
        a, it = attention_half(P, bn, tok.float(), t, fh, fw, tmask, l_t, par, td, rounded, m_of("attention_half"))
        if d == 0:
            res["attention_half"] = (dict(x=tok.float(), mask=tmask), a, it)
        o, it2 = ffn_half(P, bn, a.float(), t, fh, fw, h, w, td, rounded, m_of("ffn_half"))
        if d == 0:
            res["ffn_half"] = (dict(x=a.float()), o, it2)
        tok = o
    comp, it = soft_comp(P, "gen.sc", tok.float(), enc.float(), t, h, w, td, rounded, m_of("soft_comp"))
    res["soft_comp"] = (dict(tok=tok.float(), enc=enc.float()), comp, it)
    raw, it = decoder(P, "gen.decoder", comp[:l_t * hw].float(), l_t, h, w, td, rounded, m_of("decoder"))
    res["decoder"] = (dict(x=comp[:l_t * hw].float()), raw, it)
    res["raw"] = raw
    return res


@functools.lru_cache(maxsize=None)
def stage_inputs(case, dname):
    """the fp32 input of every stage of one case: the output of the rounded reference run of the stage before it (the scale the seeded network produces there)"""
    with torch.no_grad():
        res = chain(case, TD[dname], True)
    d = {k: v[0] for k, v in res.items() if k not in ("raw", "features")}
    d["block"] = d["attention_half"]
    return d


def run(stage, case, inp, td, rounded=True, mut=None):
    """the reference of one stage of one case on the inputs `inp` (stage_inputs(...)[stage]) -> (out float64, intermediates)"""
    cs = CASES[case]
    P = _params(cs.get("weights"))
    H, W, h, w, fh, fw = dims(cs)
    t, l_t = cs["t"], cs["l_t"]
    b0 = "gen.transformers.transformer.0"
    if stage == "encoder":
        return encoder(P, "gen.encoder", inp["x"], t, H, W, td, rounded, mut)
    if stage == "feature_propagation":
        if mut == "reference_frames_propagated":
            raise RuntimeError("a mutant of the composition: chain(..., mut=..., stage_mut='feature_propagation')")
        return feature_propagation(P, "gen.feat_prop_module", inp["x"], inp["ff"], inp["fb"], inp["masks2"], l_t, h, w, td, rounded, mut)
    if stage == "soft_split":
        return soft_split(P, "gen.ss", inp["x"], t, h, w, td, rounded, mut)
    if stage == "attention_half":
        return attention_half(P, b0, inp["x"], t, fh, fw, inp["mask"], l_t, cs["parity"], td, rounded, mut)
    if stage == "ffn_half":
        return ffn_half(P, b0, inp["x"], t, fh, fw, h, w, td, rounded, mut)
    if stage == "block":
        return block(P, b0, inp["x"], t, fh, fw, h, w, inp["mask"], l_t, cs["parity"], td, rounded, mut)
    if stage == "soft_comp":
        return soft_comp(P, "gen.sc", inp["tok"], inp["enc"], t, h, w, td, rounded, mut)
    if stage == "decoder":
        return decoder(P, "gen.decoder", inp["x"], l_t, h, w, td, rounded, mut)
    raise KeyError(stage)


@functools.lru_cache(maxsize=None)
def reference(stage, case, dname, rounded=True):
    """(out, intermediates), computed once per process and shared; callers must not modify it"""
    with torch.no_grad():
        return run(stage, case, stage_inputs(case, dname)[stage], TD[dname], rounded)


def bound(stage, dname, ref):
    """B = MARGIN u max(1, max |ref|): every stage output is fp32"""
    return margin_of(NOISE[(stage, dname)]) * U[TD[dname]] * max(1.0, ref.abs().max().item())


def noise(stage, case, dname):
    a, b = reference(stage, case, dname, True)[0], reference(stage, case, dname, False)[0]
    return (a - b).abs().max().item() / (U[TD[dname]] * max(1.0, a.abs().max().item()))


# stage -> mutant -> index of the case (CASES) assigned to it: tests/test_genref_cpu.py holds every one at least 2 B from the unmutated reference
MUTANTS = {
    "attention_half": {"corners_exchanged": 0, "rolls_negated": 0, "corner_masks_dropped": 0, "pooled_all_frames": 0, "T_ind_other_parity": 0, "masked_as_clean": 0,
                       "clean_as_masked": 0, "mask_from_all_frames": 1, "padding_keys_dropped": 0, "pool_taps_transposed": 0, "pooled_from_unpadded": 0,
                       "heads_d_major": 0},
    "ffn_half": {"fc1_channel_major": 0, "overlap_not_divided": 0, "gelu_before_normalisation": 0},
    "encoder": {"plain_concatenation": 2, "x0_one_layer_late": 2},
    "feature_propagation": {"flow_index_off_by_one": 0, "flows_exchanged": 0, "flow_not_flipped": 0, "backward_not_reversed": 0, "forward_reads_input": 0,
                            "validity_inverted": 7},
    "soft_split": {"tap_major_omitted": 2},
    "soft_comp": {"tap_major_omitted": 2},
    "decoder": {"align_corners_false": 2},
}


# the mutants whose shift of the fp32 prediction (after tanh, the clip of tests/test_inpaintgen_gpu.py::test_generator_matches_oracle, 2 blocks) stays inside that
# test's tolerance, 3.6e-3 (fp16) / 2.5e-2 (bf16), as "stage:mutant": what the end-to-end comparison alone could not see.  Kept current by
# tests/test_genref_cpu.py::test_mutants_against_the_end_to_end_tolerance
E2E_INVISIBLE = {      # shifts: mask_from_all_frames 0 (that clip has a hole in every frame), validity_inverted 1.5e-3, flow_index_off_by_one 9.3e-3
    "fp16": ["attention_half:mask_from_all_frames", "feature_propagation:validity_inverted"],
    "bf16": ["attention_half:mask_from_all_frames", "feature_propagation:validity_inverted", "feature_propagation:flow_index_off_by_one"],
    # the test's third row, fp16 at 8 blocks against 6e-3: measured once with test_genref_cpu.e2e_shifts(8), not recomputed by the test (validity inverted 3.1e-3,
    # every other mutant 2.7e-2 or more)
    "fp16, 8 blocks": ["attention_half:mask_from_all_frames", "feature_propagation:validity_inverted"],
}


def diagnose(stage, case, dname, got):
    """failure messages: the size of the reference's intermediates, and the mutants of this stage that `got` (float64, CPU) meets within B"""
    ref, it = reference(stage, case, dname)
    B = bound(stage, dname, ref)
    near = []
    for mut in ({**MUTANTS["attention_half"], **MUTANTS["ffn_half"]} if stage == "block" else MUTANTS.get(stage, {})):
        try:
            with torch.no_grad():
                m = run(stage, case, stage_inputs(case, dname)[stage], TD[dname], True, mut)[0]
        except (RuntimeError, IndexError):
            continue
        if m.shape == ref.shape and (m - ref).abs().max().item() >= 2.0 * B and (got - m).abs().max().item() <= B:
            near.append(mut)
    return f"equals mutant(s) {near or 'none'}; reference intermediates max |.|: " + ", ".join(
        f"{k} {v.double().abs().max().item():.3g}" for k, v in it.items() if torch.is_tensor(v))
