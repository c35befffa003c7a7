"""fp64 host reference of the stages of ProPainter's recurrent flow-completion network (videovanish_amd/flowcomplete.py), the cases and inputs of
tests/test_fc_stages_gpu.py, the table of its vv_conv_gemm launches, and the mutants that prove the comparison would notice a structural mistake.  Plain torch in
float64 on the CPU in the published form -- F.conv3d for the (1, k, k) and (3, 1, 1) kernels, F.conv2d, F.interpolate(align_corners=True), and torchvision's
deformable sampling written out (_bilinear_zero, _deform_columns) -- nothing here reads flowcomplete.py, deform.py or packing.py.  Shared by tests/test_fcref_cpu.py
and tests/test_fc_stages_gpu.py, not a conftest.

Every stage takes a weight source with the .conv / .linear / .norm interface of oracle.model_ref.Params (.src.normal for the temporal kernels), fp32 activations
as NHWC rows (frames-major, the product's layout) and the h16 type `td` (torch.float32 = nothing is rounded: the tie to oracle/flowcomplete_ref.py).  Weights are
always rounded to td.  `rounded=True` also rounds the activations fp32 -> td, to nearest even, exactly where the product stores or loads h16; `rounded=False` is the
same arithmetic without those roundings.  Each stage returns (out float64, {name: intermediate}).

Rounding points (the statement of flowcomplete.py / deform.py / hip.py each one restates)
  down (FlowCompleteNet.input_stage)
    network input             flowcomplete.py input_stage   hip.fc_input allocates fp32 (hip.py fc_input); vv_conv_gemm rounds the rows when it loads them
    downsample.0              flowcomplete.py _Conv.__call__   out_dtype defaults to ctx.h16, after LeakyReLU(0.2)
  encoder1 / encoder2 (_P3D.__call__, _TemporalConv.__call__)
    conv1                     _P3D.__call__   self.conv1(..., act=0.2, out=buf[2 HW:(T + 2) HW]): buf is h16 (torch.zeros(..., dtype=ctx.h16)), its outer frames zero
    temporal sum              _TemporalConv.__call__   the first GEMM stores fp32 (out_dtype=torch.float32), the second adds into it (res0=y, out=y): no rounding
    third tap                 _TemporalConv.__call__   res0=y, out_dtype=ctx.h16, act=LRELU: LeakyReLU of the whole sum, then one h16 store
  mid_dilation (FlowCompleteNet.middle, _DilatedConv.__call__)
    columns                   hip.deform_im2col allocates h16 (hip.py deform_im2col): with zero offsets a column is a copy of the h16 input or zero, exact
    layers 0, 1               middle: out_dtype = ctx.h16 after LeakyReLU(0.2); layer 2 stores fp32 (torch.float32 if i == 2)
  alignment (_SecondOrderAlignment.__call__, deform.DeformConv2d.__call__)
    conditioning stack        _BidirectionalPropagation.__call__   torch.cat([prop, cur, n2], 1) is fp32, rounded when vv_conv_gemm loads it
    offset layers 0 .. 2      _SecondOrderAlignment.__call__   out_dtype = ctx.h16 after LeakyReLU(0.1); the last one stores fp32 (torch.float32 if last)
    tanh / sigmoid            videovanish_amd/csrc/vv_deform.hip   fp32, from the fp32 raw rows; the deformed input torch.cat([prop, n2], 1) is read as fp32, not rounded
    deformed columns          deform.py DeformConv2d.__call__   hip.deform_im2col allocates h16: mask * bilinear(x) rounded once; the 1 x 1 GEMM stores fp32
  propagation (_BidirectionalPropagation.__call__)
    backbone input            torch.cat(parts, 1) is fp32, rounded at the load; backbone.0 stores h16 after LeakyReLU(0.1) (_Conv default)
    backbone.2                res0=prop, out_dtype=torch.float32: the propagated feature stays fp32 from step to step
    fusion                    self.fusion(bwd, ..., x1=fwd, res0=x, out_dtype=torch.float32): both fp32 halves rounded at the load, the residual and the store fp32
  decoder (FlowCompleteNet.decoder)
    decoder2.0                the fp32 propagation output rounded at the load; h16 after LeakyReLU(0.2)
    bilinear x2               hip.upsample2x_bilinear keeps the dtype of x (hip.py upsample2x_bilinear): h16 in, interpolated in fp32, h16 out
    decoder2.2                out_dtype=torch.float32 after LeakyReLU(0.2): `d22` stores fp32 before the skip; hip.add_inplace adds the h16 encoder1 rows in fp32
    decoder1.0                the fp32 sum rounded at the load; h16.  decoder1.2, upsample.0: h16 in (upsampled), h16 out
    upsample.2                out_dtype=torch.float32, no activation
Outputs: down, encoder1 and encoder2 are h16; every other stage stores fp32.

Noise floor N = max |ref(rounded) - ref(unrounded)| / (u max(1, max |ref(rounded)|)), u = 2^-11 (fp16) / 2^-8 (bf16), the worst case per (stage, type) over CASES --
measured by tests/test_fcref_cpu.py, which fails when NOISE goes stale -- and MARGIN = modref.margin_of(N); the GPU bound is B = MARGIN u max(1, max |ref|), plus
u max |ref| where the stage's output is itself h16 (one more rounding, of the product's own value).
"""
import functools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fusedref import TD, U, _r, _Rn, _w  # noqa: E402
from modref import margin_of  # noqa: E402

WIDTH, DG, SEED, NAME = (32, 64, 128), 16, 11, "fc"
MAX_RESIDUE = 5.0
# The seeded weights shrink the signal from layer to layer: flows of a few pixels leave features of about 0.1 at 1/8 resolution, where the offsets (5 tanh of a layer
# drawn with gain 0.1) stay below a hundredth of a pixel and B, which never falls below u, is a tenth of the signal: no mistake in the offsets could be seen.  So the
# flows are FLOW_SCALE times those of tests/test_flowcomplete_gpu.py (up to 30 pixels, as at 720p), and the stages `propagation` and `alignment` are given the
# reference's features PROP_GAIN and ALIGN_GAIN times larger (features of order 10, offsets that reach whole pixels and the flat part of tanh, as a trained
# network's).  Every other stage runs at the scale the seeded network produces.
FLOW_SCALE = 4.0
PROP_GAIN = 32.0
ALIGN_GAIN = 256.0
STAGES = ("down", "encoder1", "encoder2", "mid_dilation", "alignment", "propagation", "decoder", "complete")
H16_OUT = ("down", "encoder1", "encoder2")

# measured noise floors, worst case per (stage, type) over CASES: tests/test_fcref_cpu.py::test_noise_floor_and_margin
NOISE = {
    ("down", "fp16"): 1.220, ("down", "bf16"): 1.173,
    ("encoder1", "fp16"): 1.450, ("encoder1", "bf16"): 1.285,
    ("encoder2", "fp16"): 1.001, ("encoder2", "bf16"): 0.969,
    ("mid_dilation", "fp16"): 0.155, ("mid_dilation", "bf16"): 0.139,
    ("alignment", "fp16"): 0.822, ("alignment", "bf16"): 0.740,
    ("propagation", "fp16"): 0.308, ("propagation", "bf16"): 0.308,
    ("decoder", "fp16"): 1.418, ("decoder", "bf16"): 1.284,
    ("complete", "fp16"): 1.882, ("complete", "bf16"): 2.004,
}


def _nchw(x, Fr, H, W):
    return x.view(Fr, H, W, -1).permute(0, 3, 1, 2)


def _rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def _ncthw(x, T, H, W):
    """rows [T * H * W, C] -> [1, C, T, H, W]"""
    return x.view(T, H, W, -1).permute(3, 0, 1, 2)[None]


def _rows5(x):
    return x[0].permute(1, 2, 3, 0).reshape(-1, x.shape[1])


def _lrelu(x, s=0.2):
    return F.leaky_relu(x, s)


def _conv_1kk(P, name, x, T, H, W, cout, td, k=3, stride=1, pad=1, dil=1):
    """Conv3d with a (1, k, k) kernel on rows [T * H * W, cin] -> (rows, Ho, Wo)"""
    w, b = P.conv(name, x.shape[1], cout, k, 1.0)
    y = F.conv3d(_ncthw(x, T, H, W), _w(w, td)[:, :, None], b.double(), stride=(1, stride, stride), padding=(0, pad, pad), dilation=(1, dil, dil))
    return _rows5(y), y.shape[3], y.shape[4]


def _conv2(P, name, x, Fr, H, W, cout, td, k=3, pad=1, gain=1.0):
    w, b = P.conv(name, x.shape[1], cout, k, gain)
    return _rows(F.conv2d(_nchw(x, Fr, H, W), _w(w, td), b.double(), padding=pad))


def _temporal_weights(P, name, c):
    key = name + "#t"          # the key of oracle.flowcomplete_ref._wt: one draw per name
    if key not in P.cache:
        P.cache[key] = (P.src.normal(name + ".weight", (c, c, 3), std=1.0 / float(3 * c) ** 0.5), P.src.normal(name + ".bias", (c,), std=0.02))
    return P.cache[key]


# ---------------------------------------------------------------------------------------------------------------------------
def down(P, name, flow, mask_u8, td, rounded=True, mut=None, width=WIDTH):
    """flow fp32 [T, H, W, 2], mask u8 [T, H, W] (non-zero = hole) -> (h16-valued rows [T * (H / 2) * (W / 2), c1], intermediates)"""
    T, H, W, _ = flow.shape
    m = (mask_u8 > 0).double()[..., None]
    inp = torch.cat([flow.double() * (1.0 - m), (1.0 - m) if mut == "mask_inverted" else m], -1).permute(3, 0, 1, 2)[None]          # [1, 3, T, H, W]
    inp = F.pad(inp, (2, 2, 2, 2, 0, 0), mode="constant" if mut == "zero_padding" else "replicate")
    x = _r(_rows5(inp), td, rounded)
    y, H2, W2 = _conv_1kk(P, f"{name}.downsample.0", x, T, H + 4, W + 4, width[0], td, 5, 2, 0)
    assert (H2, W2) == (H // 2, W // 2)
    return _r(_lrelu(y), td, rounded), {"input": x}


def p3d(P, name, x, T, H, W, cout, stride, td, rounded=True, mut=None):
    """Conv3d (1,3,3) + LeakyReLU(0.2), Conv3d (3,1,1) padding (2,0,0) dilation (2,1,1), + the LeakyReLU(0.2) that follows every P3D -> (rows, Ho, Wo, conv1)"""
    h, Ho, Wo = _conv_1kk(P, name + ".conv1.0", x, T, H, W, cout, td, 3, stride, 1)
    h = _r(_lrelu(h), td, rounded)
    w, b = _temporal_weights(P, name + ".conv2.0", cout)
    w = _w(w, td)
    if mut == "temporal_taps_reversed":
        w = w.flip(2)
    h5 = _ncthw(h, T, Ho, Wo)
    if mut == "temporal_dilation_1":
        y = F.conv3d(h5, w[:, :, :, None, None], b.double(), padding=(1, 0, 0))
    elif mut == "temporal_wrap":          # the frames beyond either end are the clip's own, taken round, not zero frames
        idx = torch.arange(-2, T + 2) % T
        y = F.conv3d(h5[:, :, idx], w[:, :, :, None, None], b.double(), dilation=(2, 1, 1))
    else:
        y = F.conv3d(h5, w[:, :, :, None, None], b.double(), padding=(2, 0, 0), dilation=(2, 1, 1))
    return _r(_lrelu(_rows5(y)), td, rounded), Ho, Wo, h


def encoder(P, name, x, T, H, W, cout, td, rounded=True, mut=None):
    """encoder1 / encoder2 (`name` ends in the one meant): P3D(c, c), P3D(c, cout, stride 2) -> (h16-valued rows at half the resolution, intermediates)"""
    a, _, _, c1a = p3d(P, name + ".0", x.double(), T, H, W, x.shape[1], 1, td, rounded, mut)
    b, Ho, Wo, c1b = p3d(P, name + ".2", a, T, H, W, cout, 2, td, rounded, mut)
    assert (Ho, Wo) == (H // 2, W // 2)
    return b, {"p3d0.conv1": c1a, "p3d0": a, "p3d2.conv1": c1b}


def mid_dilation(P, name, x, T, H, W, td, rounded=True, mut=None):
    """three (1,3,3) convolutions of dilation 3, 2, 1 + LeakyReLU(0.2) -> (fp32 rows, intermediates)"""
    it, h = {}, x.double()
    for i, d in enumerate((1, 2, 3) if mut == "dilations_1_2_3" else (3, 2, 1)):
        h, _, _ = _conv_1kk(P, f"{name}.mid_dilation.{2 * i}", h, T, H, W, x.shape[1], td, 3, 1, d, d)
        it[f"layer{2 * i}"] = h = _r(_lrelu(h), td, rounded and i < 2)
    return h, it


# ---------------------------------------------------------------------------------------------------------------------------
def _bilinear_zero(img, py, px):
    """torchvision's deform_conv2d sampling rule (bilinear_interpolate): img [G, c, H, W], positions [G, 1, H, W] -> [G, c, H, W].  A sample at or beyond -1 / H (W)
    is 0; else the four neighbours are blended with (1 - lh)(1 - lw) ..., a neighbour outside the image counting as 0"""
    G, c, H, W = img.shape
    inside = (py > -1) & (py < H) & (px > -1) & (px < W)
    y0, x0 = torch.floor(py), torch.floor(px)
    lh, lw = py - y0, px - x0
    y0, x0 = y0.long(), x0.long()
    flat = img.reshape(G, c, H * W)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(G, 1, -1).expand(G, c, -1)
        return torch.gather(flat, 2, idx).reshape(G, c, *yy.shape[2:]) * ok.to(img.dtype)
    val = (1 - lh) * (1 - lw) * tap(y0, x0) + (1 - lh) * lw * tap(y0, x0 + 1) + lh * (1 - lw) * tap(y0 + 1, x0) + lh * lw * tap(y0 + 1, x0 + 1)
    return val * inside.to(img.dtype)


def _deform_columns(x, offset, mask, dg):
    """x [Cin, H, W]; offset [2 * dg * 9, H, W] with channel 2 (g 9 + k) = dy and the next one dx of group g, tap k = ky 3 + kx; mask [dg * 9, H, W]
    -> [9, Cin, H, W]: mask * bilinear(x, p + tap - 1 + offset), 3 x 3, stride 1, padding 1, dilation 1"""
    Cin, H, W = x.shape
    xg = x.view(dg, Cin // dg, H, W)
    off, mk = offset.view(dg, 9, 2, H, W), mask.view(dg, 9, 1, H, W)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=x.dtype), torch.arange(W, dtype=x.dtype), indexing="ij")
    cols = []
    for k in range(9):
        ky, kx = divmod(k, 3)
        v = _bilinear_zero(xg, ys + (ky - 1) + off[:, k, 0:1], xs + (kx - 1) + off[:, k, 1:2])
        cols.append((v * mk[:, k]).reshape(Cin, H, W))
    return torch.stack(cols)


def alignment(P, name, prop, cur, n2, H, W, td, rounded=True, mut=None, dg=DG):
    """SecondOrderDeformableAlignment without flow guidance: prop, cur, n2 fp32 rows [H * W, C] (one frame) -> (aligned rows [H * W, C] fp32, intermediates)"""
    on, C = rounded, prop.shape[1]
    prop, cur, n2 = prop.double(), cur.double(), n2.double()
    h = _r(torch.cat([cur, prop, n2] if mut == "cond_cur_prop_n2" else [prop, cur, n2], 1), td, on)
    for i, co in enumerate([C, C, C, 27 * dg]):
        h = _conv2(P, f"{name}.conv_offset.{2 * i}", h, 1, H, W, co, td, gain=0.1 if i == 3 else 1.0)
        if i < 3:
            h = _r(_lrelu(h, 0.1), td, on)
    raw = _nchw(h, 1, H, W)[0].contiguous()          # [27 dg, H, W]
    if mut == "raw_interleaved":          # (o1, o2, m) of nine channels each per group, not three chunks of 9 dg
        g3 = raw.view(dg, 3, 9, H, W)
        o1, o2, m = (g3[:, j].reshape(9 * dg, H, W) for j in range(3))
    else:
        o1, o2, m = torch.chunk(raw, 3, dim=0)
    offset = (3.0 if mut == "max_residue_3" else MAX_RESIDUE) * torch.tanh(torch.cat([o1, o2], 0))
    x2 = torch.cat([n2, prop] if mut == "prop_n2_exchanged" else [prop, n2], 1)
    col = _r(_deform_columns(_nchw(x2, 1, H, W)[0].contiguous(), offset.contiguous(), torch.sigmoid(m).contiguous(), dg), td, on)          # [9, 2C, H, W]
    w, b = P.conv(name, 2 * C, C, 3, 1.0)
    out = torch.einsum("ock,kchw->ohw", _w(w, td).reshape(C, 2 * C, 9), col) + b.double().view(-1, 1, 1)
    return out.permute(1, 2, 0).reshape(H * W, C), {"raw": h, "max |offset|": offset.abs().max()}


def propagation(P, name, x, T, H, W, td, rounded=True, mut=None, dg=DG):
    """BidirectionalPropagation: x fp32 rows [T * H * W, C] -> (rows of the same shape, intermediates)"""
    on, C, HW = rounded, x.shape[1], H * W
    xd = x.double()
    spatial = [xd[t * HW:(t + 1) * HW] for t in range(T)]
    feats = {}
    for mod in ("backward_", "forward_"):
        feats[mod] = []
        order = list(range(T))[::-1] if mod == "backward_" else list(range(T))
        prop = torch.zeros(HW, C, dtype=torch.float64)
        for i, idx in enumerate(order):
            cur = spatial[idx]
            if i > 0:
                n2 = torch.zeros_like(prop)
                if i > 1:
                    n2 = feats[mod][-1 if mut == "second_order_one_back" else -2]
                prop = alignment(P, f"{name}.deform_align.{mod}", prop, cur, n2, H, W, td, on, mut, dg)[0]
            parts = [cur] + ([feats["backward_"][idx]] if mod == "forward_" else []) + [prop]
            if mut == "forward_input_cur_prop_backward" and mod == "forward_":
                parts = [parts[0], parts[2], parts[1]]
            h = _r(_lrelu(_conv2(P, f"{name}.backbone.{mod}.0", _r(torch.cat(parts, 1), td, on), 1, H, W, C, td), 0.1), td, on)
            prop = prop + _conv2(P, f"{name}.backbone.{mod}.2", h, 1, H, W, C, td)
            feats[mod].append(prop)
        if mod == "backward_" and mut != "backward_not_reversed":
            feats[mod] = feats[mod][::-1]
    bwd, fwd = torch.cat(feats["backward_"], 0), torch.cat(feats["forward_"], 0)
    al = torch.cat([fwd, bwd] if mut == "fusion_halves_exchanged" else [bwd, fwd], 1)
    out = _conv2(P, f"{name}.fusion", _r(al, td, on), T, H, W, C, td, 1, 0) + xd
    return out, {"backward": bwd, "forward": fwd}


def decoder(P, name, prop, e1, T, H, W, td, rounded=True, mut=None, width=WIDTH):
    """decoder2 + the encoder1 skip, decoder1, upsample: prop fp32 rows at 1/8, e1 h16-valued rows at 1/4 -> (the flow, fp32 rows [T * H * W, 2], intermediates)"""
    on, it = rounded, {}
    c1, c2, c3 = width
    H2, W2, H4, W4, H8, W8 = H // 2, W // 2, H // 4, W // 4, H // 8, W // 8
    ac = mut != "align_corners_false"
    up = lambda z, hh, ww: _r(_rows(F.interpolate(_nchw(z, T, hh, ww), scale_factor=2, mode="bilinear", align_corners=ac)), td, on)
    z = _r(_lrelu(_conv2(P, f"{name}.decoder2.0", _r(prop.double(), td, on), T, H8, W8, c3, td)), td, on)
    z = _conv2(P, f"{name}.decoder2.2.conv", up(z, H8, W8), T, H4, W4, c2, td)
    it["d2"] = z = _lrelu(z + e1.double()) if mut == "skip_before_lrelu" else _lrelu(z) + e1.double()
    z = _r(_lrelu(_conv2(P, f"{name}.decoder1.0", _r(z, td, on), T, H4, W4, c2, td)), td, on)
    it["d1"] = z = _r(_lrelu(_conv2(P, f"{name}.decoder1.2.conv", up(z, H4, W4), T, H2, W2, c1, td)), td, on)
    it["up"] = z = _r(_lrelu(_conv2(P, f"{name}.upsample.0", z, T, H2, W2, c1, td)), td, on)
    return _conv2(P, f"{name}.upsample.2.conv", up(z, H2, W2), T, H, W, 2, td), it


# stage -> the stage-level mutants it knows (chain hands a mutant only to these)
STAGE_MUTANTS = {
    "down": ("zero_padding", "mask_inverted"),
    "encoder1": ("temporal_taps_reversed", "temporal_dilation_1", "temporal_wrap"),
    "encoder2": ("temporal_taps_reversed", "temporal_dilation_1", "temporal_wrap"),
    "mid_dilation": ("dilations_1_2_3",),
    "alignment": ("cond_cur_prop_n2", "prop_n2_exchanged", "raw_interleaved", "max_residue_3"),
    "propagation": ("cond_cur_prop_n2", "prop_n2_exchanged", "raw_interleaved", "max_residue_3", "second_order_one_back", "backward_not_reversed",
                    "forward_input_cur_prop_backward", "fusion_halves_exchanged"),
    "decoder": ("skip_before_lrelu", "align_corners_false"),
}


def chain(P, flow, mask_u8, td, rounded=True, mut=None, stage_mut=None, name=NAME, dg=DG, width=WIDTH):
    """`complete`: the stages composed, every stage on the output of the one before.  mut applies to stage `stage_mut` (None: to every stage that knows it)
    -> {stage: (input dict, out, intermediates)} and "pred": the flow, rows [T * H * W, 2]"""
    T, H, W, _ = flow.shape
    assert H % 8 == 0 and W % 8 == 0
    c1, c2, c3 = width
    m_of = lambda st: mut if (stage_mut in (None, st) and mut in STAGE_MUTANTS[st]) else None
    res = {}
    x, it = down(P, name, flow, mask_u8, td, rounded, m_of("down"), width)
    res["down"] = (dict(flow=flow, mask=mask_u8), x, it)
    e1, it = encoder(P, f"{name}.encoder1", x.float(), T, H // 2, W // 2, c2, td, rounded, m_of("encoder1"))
    res["encoder1"] = (dict(x=x.float()), e1, it)
    e2, it = encoder(P, f"{name}.encoder2", e1.float(), T, H // 4, W // 4, c3, td, rounded, m_of("encoder2"))
    res["encoder2"] = (dict(x=e1.float()), e2, it)
    mid, it = mid_dilation(P, name, e2.float(), T, H // 8, W // 8, td, rounded, m_of("mid_dilation"))
    res["mid_dilation"] = (dict(x=e2.float()), mid, it)
    pr, it = propagation(P, f"{name}.feat_prop_module", mid.float(), T, H // 8, W // 8, td, rounded, m_of("propagation"), dg)
    res["propagation"] = (dict(x=(PROP_GAIN * mid).float()), pr, it)
    HW = (H // 8) * (W // 8)          # one alignment call (alignment_pair) on features the propagation produced: the last backward one, a frame, the first forward one
    g = lambda z: (ALIGN_GAIN * z).float()
    res["alignment"] = (dict(prop=g(it["backward"][(T - 1) * HW:]), cur=g(mid[max(T - 2, 0) * HW:(max(T - 2, 0) + 1) * HW]), n2=g(it["forward"][:HW])), None, None)
    pred, it = decoder(P, name, pr.float(), e1.float(), T, H, W, td, rounded, m_of("decoder"), width)
    res["decoder"] = (dict(prop=pr.float(), e1=e1.float()), pred, it)
    res["complete"] = (dict(flow=flow, mask=mask_u8), pred, {})
    res["pred"] = pred
    return res


def alignment_pair(P, name, prop, cur, n2, H, W, td, rounded=True, mut=None, dg=DG):
    """the stage `alignment`: one _SecondOrderAlignment call with n2 = 0 (the second step of a direction) and one with n2 != 0, the two results stacked
    -> ([2 * H * W, C], intermediates)"""
    a, ia = alignment(P, name, prop, cur, torch.zeros_like(n2), H, W, td, rounded, mut, dg)
    b, ib = alignment(P, name, prop, cur, n2, H, W, td, rounded, mut, dg)
    return torch.cat([a, b], 0), {"raw, n2 = 0": ia["raw"], "raw": ib["raw"], "max |offset|": torch.maximum(ia["max |offset|"], ib["max |offset|"])}


def bidirect(P, fw, bw, masks_u8, td, rounded=True, mut=None, **kw):
    """forward_bidirect_flow + combine_flow: flows fp32 [T, H, W, 2] (t -> t + 1 / t + 1 -> t), masks u8 [T + 1, H, W]
    -> (pred_fw, pred_bw, comb_fw, comb_bw), each float64 [T, H, W, 2]"""
    T, H, W, _ = fw.shape
    pf = chain(P, fw, masks_u8[:-1], td, rounded, mut, **kw)["pred"].view(T, H, W, 2)
    if mut == "backward_not_flipped":
        pb = chain(P, bw, masks_u8[1:], td, rounded, None, **kw)["pred"].view(T, H, W, 2)
    else:
        pb = chain(P, bw.flip(0), masks_u8[1:].flip(0), td, rounded, mut, **kw)["pred"].view(T, H, W, 2).flip(0)
    hole = lambda m: (m > 0)[..., None]
    return pf, pb, torch.where(hole(masks_u8[:-1]), pf, fw.double()), torch.where(hole(masks_u8[1:]), pb, bw.double())


# ---------------------------------------------------------------------------------------------------------------------------
# Cases (T counts flows; the clip has T + 1 frames), width (32, 64, 128), 16 deformable groups:
#   a 3 x 64 x 128: the scales 32 x 64, 16 x 32 and 8 x 16 are exact covers of 8 x 16 patches: every eligible 3 x 3 launch takes the halo loader, as at 720p
#   b 5 x 24 x 40:  grids 12 x 20, 6 x 10, 3 x 5: ragged, no halo launch; the temporal taps t +- 2 reach real frames on both sides
#   c 2 x 16 x 24:  both outer temporal taps fall in the zero frames; propagation without a second-order term
#   d 1 x 8 x 16:   a 1 x 2 grid at 1/8: every dilated tap but the centre is out of bounds; bilinear x2 from a 1-pixel row
CASES = [dict(T=3, H=64, W=128), dict(T=5, H=24, W=40), dict(T=2, H=16, W=24), dict(T=1, H=8, W=16)]


@functools.lru_cache(maxsize=None)
def params(width=WIDTH, seed=SEED):
    """the seeded weights; one source per width, since a Params caches by layer name alone"""
    from oracle.model_ref import Params
    return Params(seed)


def make_masks(T, H, W):
    """u8 [T + 1, H, W]: frame 0 a hole that touches the top and the left border (the replicate padding replicates mask = 1 and zeroed flow), frame 1 none, frame 2
    all hole where the clip has at least five frames (case b), every other frame an interior hole that moves"""
    m = torch.zeros(T + 1, H, W, dtype=torch.uint8)
    m[0, :H // 2, :W // 3] = 255
    for t in range(2, T + 1):
        if t == 2 and T + 1 >= 5:
            m[t] = 255
        else:
            m[t, H // 4:H // 2 + 2, W // 4 + t:W // 2 + t] = 255
    return m


@functools.lru_cache(maxsize=None)
def raw_inputs(case):
    """(fw, bw fp32 [T, H, W, 2], masks u8 [T + 1, H, W]): a smooth ramp plus noise, as _case of tests/test_flowcomplete_gpu.py, FLOW_SCALE times larger"""
    cs = CASES[case]
    T, H, W = cs["T"], cs["H"], cs["W"]
    rn = _Rn(7000 + case)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    fw = FLOW_SCALE * (torch.stack([torch.stack([2.0 + 0.05 * yy + 0.3 * t, -1.0 + 0.04 * xx], -1) for t in range(T)]) + 0.2 * rn(T, H, W, 2))
    bw = -fw + FLOW_SCALE * 0.1 * rn(T, H, W, 2)
    return fw, bw, make_masks(T, H, W)


@functools.lru_cache(maxsize=None)
def stage_inputs(case, dname):
    """the fp32 input of every stage of one case: the output of the rounded reference run of the stage before it (the scale the seeded network produces there)"""
    fw, _, m = raw_inputs(case)
    with torch.no_grad():
        res = chain(params(), fw, m[:-1], TD[dname], True)
    return {k: v[0] for k, v in res.items() if k != "pred"}


def run(stage, case, inp, td, rounded=True, mut=None, P=None):
    """the reference of one stage of one case on the inputs `inp` (stage_inputs(...)[stage]) -> (out float64, intermediates)"""
    cs, P = CASES[case], params() if P is None else P
    T, H, W = cs["T"], cs["H"], cs["W"]
    c1, c2, c3 = WIDTH
    if stage == "down":
        return down(P, NAME, inp["flow"], inp["mask"], td, rounded, mut)
    if stage == "encoder1":
        return encoder(P, f"{NAME}.encoder1", inp["x"], T, H // 2, W // 2, c2, td, rounded, mut)
    if stage == "encoder2":
        return encoder(P, f"{NAME}.encoder2", inp["x"], T, H // 4, W // 4, c3, td, rounded, mut)
    if stage == "mid_dilation":
        return mid_dilation(P, NAME, inp["x"], T, H // 8, W // 8, td, rounded, mut)
    if stage == "alignment":
        return alignment_pair(P, f"{NAME}.feat_prop_module.deform_align.forward_", inp["prop"], inp["cur"], inp["n2"], H // 8, W // 8, td, rounded, mut)
    if stage == "propagation":
        return propagation(P, f"{NAME}.feat_prop_module", inp["x"], T, H // 8, W // 8, td, rounded, mut)
    if stage == "decoder":
        return decoder(P, NAME, inp["prop"], inp["e1"], T, H, W, td, rounded, mut)
    if stage == "complete":
        return chain(P, inp["flow"], inp["mask"], td, rounded, mut)["pred"], {}
    raise KeyError(stage)


@functools.lru_cache(maxsize=None)
def reference(stage, case, dname, rounded=True):
    """(out, intermediates), computed once per process and shared; callers must not modify it"""
    with torch.no_grad():
        return run(stage, case, stage_inputs(case, dname)[stage], TD[dname], rounded)


@functools.lru_cache(maxsize=None)
def reference_bidirect(case, dname):
    fw, bw, m = raw_inputs(case)
    with torch.no_grad():
        return bidirect(params(), fw, bw, m, TD[dname], True)


def bound(stage, dname, ref):
    """B = MARGIN u max(1, max |ref|), plus u max |ref| where the stage's output is h16"""
    u, mx = U[TD[dname]], ref.abs().max().item()
    return margin_of(NOISE[(stage, dname)]) * u * max(1.0, mx) + (u * mx if stage in H16_OUT else 0.0)


def noise(stage, case, dname):
    a, b = reference(stage, case, dname, True)[0], reference(stage, case, dname, False)[0]
    return (a - b).abs().max().item() / (U[TD[dname]] * max(1.0, a.abs().max().item()))


# stage -> mutant -> index of the case (CASES) assigned to it: tests/test_fcref_cpu.py holds every one at least 2 B from the unmutated reference.
# ("complete": "backward_not_flipped" is a mutant of forward_bidirect_flow, held on the backward prediction against the bound of `complete`)
MUTANTS = {
    "down": {"zero_padding": 0, "mask_inverted": 0},
    "encoder1": {"temporal_taps_reversed": 1, "temporal_dilation_1": 1, "temporal_wrap": 1},
    "encoder2": {"temporal_taps_reversed": 0, "temporal_dilation_1": 0, "temporal_wrap": 0},
    "mid_dilation": {"dilations_1_2_3": 0},
    "alignment": {"cond_cur_prop_n2": 0, "prop_n2_exchanged": 0, "raw_interleaved": 0, "max_residue_3": 0},
    "propagation": {"second_order_one_back": 1, "backward_not_reversed": 1, "forward_input_cur_prop_backward": 1, "fusion_halves_exchanged": 1, "prop_n2_exchanged": 0},
    "decoder": {"skip_before_lrelu": 0, "align_corners_false": 0},
    "complete": {"backward_not_flipped": 1},
}

# the mutants whose shift of the fp32 predictions of forward_bidirect_flow, at the clip and width of tests/test_flowcomplete_gpu.py::
# test_flow_completion_matches_oracle (T = 5 frames of 32 x 48, width (16, 32, 64), 8 groups), stays inside that test's tolerance, 2e-3 (fp16) / 2.2e-2 (bf16) of
# max |ref|, as "stage:mutant": what the end-to-end comparison alone could not see.  Kept current by tests/test_fcref_cpu.py::test_mutants_against_the_end_to_end_tolerance
E2E_INVISIBLE = {      # shifts: conditioning order 1.2e-4, max_residue = 3 1.3e-3, raw channels interleaved 3.4e-3, the temporal kernels of encoder2 7e-3 .. 8e-3,
    # the second-order feature one step back 2.1e-2, dilations 1, 2, 3 2.19e-2; every other mutant moves the prediction by 5e-2 .. 0.8 of max |ref|
    "fp16": ["alignment:cond_cur_prop_n2", "alignment:max_residue_3"],
    "bf16": ["alignment:cond_cur_prop_n2", "alignment:max_residue_3", "alignment:raw_interleaved", "encoder2:temporal_dilation_1", "encoder2:temporal_taps_reversed",
             "encoder2:temporal_wrap", "mid_dilation:dilations_1_2_3", "propagation:second_order_one_back"],
}


def run_mutant(stage, mut, case, dname):
    """the mutated reference of (stage, mutant) on `case`, rounded, in the shape of reference(stage, case, dname)[0]"""
    with torch.no_grad():
        if stage == "complete":
            fw, bw, m = raw_inputs(case)
            return bidirect(params(), fw, bw, m, TD[dname], True, mut)[1].reshape(-1, 2)
        return run(stage, case, stage_inputs(case, dname)[stage], TD[dname], True, mut)[0]


def diagnose(stage, case, dname, got):
    """failure messages: the size of the reference's intermediates, and the mutants of this stage that `got` (float64, CPU) meets within B"""
    ref, it = reference(stage, case, dname)
    B = bound(stage, dname, ref)
    near = []
    for mut in ([m for s in STAGE_MUTANTS.values() for m in s] if stage == "complete" else STAGE_MUTANTS.get(stage, ())):
        try:
            with torch.no_grad():
                m = run(stage, case, stage_inputs(case, dname)[stage], TD[dname], True, mut)[0]
        except (RuntimeError, IndexError):
            continue
        if m.shape == ref.shape and (m - ref).abs().max().item() >= 2.0 * B and (got - m).abs().max().item() <= B and mut not in near:
            near.append(mut)
    return f"equals mutant(s) {near or 'none'}; reference intermediates max |.|: " + ", ".join(
        f"{k} {v.double().abs().max().item():.3g}" for k, v in it.items() if torch.is_tensor(v))


# ---------------------------------------------------------------------------------------------------------------------------
# The vv_conv_gemm launches of FlowCompleteNet.complete, layer by layer, as shapes: what tests/test_fcref_cpu.py routes through hip.conv_gemm_route at 720 x 1280 and
# at the cases, and what tests/test_fc_stages_gpu.py compares with the launches the product makes.  A tensor is ("f32" | "h16", shape).
def _npad(N):
    """the row padding of the packed weights ([Npad][Kpad] h16, Kpad % 64 == 0): N itself at a multiple of 160 or 128, a multiple of 16 up to 64, else of 128"""
    if N % 160 == 0 or N % 128 == 0:
        return N
    return (N + 15) // 16 * 16 if N <= 64 else (N + 127) // 128 * 128


def _launch(layer, x0, cin, cout, F_, H, W, k=3, stride=1, pad=None, act=0.0, out="h16", res0=False, x1=False, own_out=False, lin=False):
    pad = k // 2 if pad is None else pad
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    cpad = (cin + 7) // 8 * 8
    K = k * k * cpad * (2 if x1 else 1)
    M = F_ * Ho * Wo
    d = dict(layer=layer, x0=(x0, (F_ * H * W, cpad)), weight=("h16", (_npad(cout), (K + 63) // 64 * 64)), N=cout, K=K, x1=(x0, (F_ * H * W, cpad)) if x1 else None, F=F_,
             Hin=H, Win=W, Hout=Ho, Wout=Wo, ksize=k, stride=stride, pad_t=pad, pad_l=pad, bias=("f32", (cout,)), res0=("f32", (M, cout)) if res0 else None,
             out=(out, (M, cout)) if own_out else None, out_dtype=out, act="lrelu" if act else None, act_slope=float(act))
    if lin:          # the GEMMs the product launches without naming the convolution's geometry: hip.conv_gemm's defaults
        d.update(Hout=None, Wout=None)
    return d


def _p3d_launches(layer, cin, cout, stride, T, H, W):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    n = T * Ho * Wo
    t = lambda i, **kw: dict(_launch(f"{layer}.conv2.0[{i}]", "h16", cout, cout, 1, 1, n, k=1, lin=True, **kw), pad_t=0, pad_l=0)
    t0, t1, t2 = t(0, out="f32"), dict(t(1, out="f32", res0=True, own_out=True), bias=None), dict(t(2, act=0.2, res0=True), bias=None)
    t1["out_dtype"] = None
    return [_launch(f"{layer}.conv1.0", "h16", cin, cout, T, H, W, stride=stride, act=0.2, own_out=True), t0, t1, t2]


def _align_launches(layer, C, dg, H, W):
    ls, cin = [], 3 * C
    for i, co in enumerate([C, C, C, 27 * dg]):
        ls.append(_launch(f"{layer}.conv_offset.{2 * i}", "f32" if i == 0 else "h16", cin, co, 1, H, W, act=0.0 if i == 3 else 0.1, out="f32" if i == 3 else "h16"))
        cin = co
    return ls + [_dcn_launch(layer, 2 * C, C, 1, H, W, 0.0, "f32")]


def _dcn_launch(layer, cin, cout, F_, H, W, act, out):
    return dict(_launch(layer, "h16", 9 * cin, cout, F_, H, W, k=1, act=act, out=out), Hout=None, Wout=None)


def stage_launches(stage, T, H, W, width=WIDTH, dg=DG):
    """the vv_conv_gemm launches of one stage at T flows of H x W, in order"""
    c1, c2, c3 = width
    H2, W2, H4, W4, H8, W8 = H // 2, W // 2, H // 4, W // 4, H // 8, W // 8
    fp = f"{NAME}.feat_prop_module"
    if stage == "down":
        return [_launch(f"{NAME}.downsample.0", "f32", 3, c1, T, H + 4, W + 4, k=5, stride=2, pad=0, act=0.2)]
    if stage == "encoder1":
        return _p3d_launches(f"{NAME}.encoder1.0", c1, c1, 1, T, H2, W2) + _p3d_launches(f"{NAME}.encoder1.2", c1, c2, 2, T, H2, W2)
    if stage == "encoder2":
        return _p3d_launches(f"{NAME}.encoder2.0", c2, c2, 1, T, H4, W4) + _p3d_launches(f"{NAME}.encoder2.2", c2, c3, 2, T, H4, W4)
    if stage == "mid_dilation":
        return [_dcn_launch(f"{NAME}.mid_dilation.{2 * i}", c3, c3, T, H8, W8, 0.2, "f32" if i == 2 else "h16") for i in range(3)]
    if stage == "alignment":
        return 2 * _align_launches(f"{fp}.deform_align.forward_", c3, dg, H8, W8)
    if stage == "propagation":
        ls = []
        for di, mod in enumerate(("backward_", "forward_")):
            for i in range(T):
                if i > 0:
                    ls += _align_launches(f"{fp}.deform_align.{mod}", c3, dg, H8, W8)
                ls.append(_launch(f"{fp}.backbone.{mod}.0", "f32", (2 + di) * c3, c3, 1, H8, W8, act=0.1))
                ls.append(_launch(f"{fp}.backbone.{mod}.2", "h16", c3, c3, 1, H8, W8, out="f32", res0=True))
        return ls + [_launch(f"{fp}.fusion", "f32", c3, c3, T, H8, W8, k=1, pad=0, out="f32", res0=True, x1=True)]
    if stage == "decoder":
        return [_launch(f"{NAME}.decoder2.0", "f32", c3, c3, T, H8, W8, act=0.2), _launch(f"{NAME}.decoder2.2.conv", "h16", c3, c2, T, H4, W4, act=0.2, out="f32"),
                _launch(f"{NAME}.decoder1.0", "f32", c2, c2, T, H4, W4, act=0.2), _launch(f"{NAME}.decoder1.2.conv", "h16", c2, c1, T, H2, W2, act=0.2),
                _launch(f"{NAME}.upsample.0", "h16", c1, c1, T, H2, W2, act=0.2), _launch(f"{NAME}.upsample.2.conv", "h16", c1, 2, T, H, W, out="f32")]
    if stage == "complete":
        return [l for st in ("down", "encoder1", "encoder2", "mid_dilation", "propagation", "decoder") for l in stage_launches(st, T, H, W, width, dg)]
    raise KeyError(stage)


def launch_key(d):
    """a launch without its layer name: what two launches must share to be the same launch"""
    return tuple((k, v) for k, v in sorted(d.items()) if k != "layer")


def route_of(d, dname):
    """hip.conv_gemm_route of a launch of the table, in type `dname`: the ROUTE_* code (negative: the launch would be refused)"""
    from videovanish_amd import hip
    h16 = TD[dname]
    ty = lambda t: torch.float32 if t == "f32" else h16
    ten = lambda v: None if v is None else torch.empty(v[1], dtype=ty(v[0]), device="meta")
    kw = {k: v for k, v in d.items() if k not in ("layer", "x0", "weight", "N", "K", "x1", "bias", "res0", "out", "out_dtype", "act") and v is not None}
    kw["act"] = hip.ACT_LRELU if d["act"] else hip.ACT_NONE
    return hip.conv_gemm_route(hip.F16 if dname == "fp16" else hip.BF16, ten(d["x0"]), ten(d["weight"]), d["N"], d["K"], x1=ten(d["x1"]), bias=ten(d["bias"]),
                               res0=ten(d["res0"]), out=ten(d["out"]), out_dtype=None if d["out_dtype"] is None else ty(d["out_dtype"]), **kw)


def describe_call(args, kw):
    """the arguments of one hip.conv_gemm call of the product in the form of the table (without the layer name)"""
    from videovanish_amd import hip
    ten = lambda t: None if t is None else ("f32" if t.dtype == torch.float32 else "h16", tuple(t.shape))
    dtype, x0, weight, N, K = args
    assert kw.get("act", hip.ACT_NONE) in (hip.ACT_NONE, hip.ACT_LRELU)
    od = kw.get("out_dtype")
    d = dict(x0=ten(x0), weight=ten(weight), N=N, K=K, x1=ten(kw.get("x1")), F=kw.get("F", 1), Hin=kw.get("Hin", 1), Win=kw.get("Win", 1), Hout=kw.get("Hout"),
             Wout=kw.get("Wout"), ksize=kw.get("ksize", 1), stride=kw.get("stride", 1), pad_t=kw.get("pad_t", 0), pad_l=kw.get("pad_l", 0), bias=ten(kw.get("bias")),
             res0=ten(kw.get("res0")), out=ten(kw.get("out")), out_dtype=None if od is None else ("f32" if od == torch.float32 else "h16"), act="lrelu" if kw.get("act", 0) else None,
             act_slope=float(kw.get("act_slope", 0.0)))
    extra = set(kw) - {"x1", "F", "Hin", "Win", "Hout", "Wout", "ksize", "stride", "pad_t", "pad_l", "bias", "res0", "out", "out_dtype", "act", "act_slope"}
    assert not extra, f"hip.conv_gemm arguments the launch table does not hold: {sorted(extra)}"
    return d
