"""fp64 host references of the layer-by-layer modules of videovanish_amd/nn.py (ResBlock, SpatialTransformer, MotionModule) and of vae._MidAttn: the
composition of kernels that runs wherever no fused kernel exists (C = 640 / 1280, the fallback conditions at C = 320, the VAE), the inputs and case tables of
tests/test_modules_gpu.py, and the mutants that prove the comparison would notice a structural mistake.  Plain torch in float64 on the CPU; shared by
tests/test_modref_cpu.py and tests/test_modules_gpu.py, not a conftest.

Every function takes a weight source with the .conv / .linear / .norm interface of oracle.model_ref.Params (Params(0) draws the weights of Ctx(..., weight_seed=0)),
the parameter name prefix, fp32 activations as rows [F * H * W, C] (frames-major NHWC, the product's layout), and the h16 type `td` (torch.float32 = nothing is
rounded at all: the tie to oracle/model_ref.py).  Weights are always rounded to td (not in the `precise` forms, whose split-3 GEMM carries hi + lo of both
operands: an unrounded GEMM here).  `rounded=True` also rounds the activations fp32 -> td, to nearest even, exactly where the product path stores or loads h16;
`rounded=False` is the same arithmetic without those roundings.  Each function returns (out float64, {name: intermediate}) for failure messages.

Rounding points (the statement of nn.py / hip.py each one restates)
  ResBlock (nn.ResBlock.__call__)
    norm1 / norm2 output      nn.py 284, 296   self.norm1(x0, F, HW, x1=x1, silu=True) / self.norm2(h, ...): hip.groupnorm allocates h16 (hip.py 432)
    time_emb_proj operand     nn.py 273        self.temb(silu_temb, res0=res): an fp32 operand is rounded when vv_conv_gemm loads it; the result is fp32
    shortcut operand          nn.py 298        self.short(x0, F, H, W, x1=x1): x0 | x1 fp32, rounded at the load
    conv1 output              nn.py 295        out_dtype fp32 (H16_MID is False): not rounded
    block output              nn.py 302        conv2(..., res0=xs, res1=res1, out_dtype=out_dtype): fp32, or h16 when asked
    precise (VAE)             nn.py 109-112    GroupNorm emits the split operand, Conv(precise=True) runs hi / lo of both operands: nothing is rounded here
  SpatialTransformer (nn.SpatialTransformer.__call__, the path below the fused one)
    GroupNorm output          nn.py 455        h16; proj_in (456) stores fp32
    LN1 / LN2 / LN3           nn.py 457-459    hip.layernorm allocates h16 (hip.py 476)
    q | k | v                 nn.py 342        self.qkv(n, out_dtype=h16, split=...); the query weights carry 40^-1/2 log2 e before their rounding at D = 40 only (415)
    text K | V                nn.py 377        kvp(text_h16, out_dtype=h16): h16 text, h16 [77, 2C] result, once at build time
    cross-attention q         nn.py 383        self.q(n, out_dtype=h16)
    P, o                      vv_attention     P = 2^(s - m) rounded before P V, scores and the row sum l in fp32 (tests/attnref.py attention_core); o h16 (nn.py 348 / 384)
    GEGLU product             nn.py 398        self.proj(n, out_dtype=h16)
    feed-forward + residual   nn.py 398        self.out(..., res0=res, out_dtype=h16): the trunk is h16 from here
    proj_out                  nn.py 460        res0 = the fp32 x; fp32 or h16 output
  MotionModule (nn.MotionModule._run, the path below the fused one)
    GroupNorm output          nn.py 519        pool_frames=True: statistics over the clip; h16
    LN1 / LN2 + pe            nn.py 521-522    pe[row // HW] is added in fp32 before the one rounding (vv_norm.hip layernorm_kernel: per = pe + (row / rows_per_frame) * C)
    q | k | v                 nn.py 360        row-major h16 [F * HW, 3C]; the core gathers a pixel's frames with row stride HW * 3C (363)
    trunk                     nn.py 364        self.out(o, res0=res): fp32 until the feed-forward (523), h16 after it
    proj_out                  nn.py 524        res0 = x, res1; fp32 or h16 output
  vae._MidAttn (vae.py 15, nn.SelfAttention.spatial)
    plain                     GroupNorm h16, q | k | v (with bias) h16, P, o h16, out projection + the fp32 x
    precise                   nn.py 328-334    unrounded GroupNorm and projections around the h16 core: q | k | v rounded once (hip.split_f32 hi), P, o h16
GELU is the exact erf form, LayerNorm eps 1e-5, GroupNorm statistics fp64.

Noise floor N = max |ref(rounded) - ref(unrounded)| / (u max(1, max |ref(rounded)|)), u = 2^-11 (fp16) / 2^-8 (bf16), the worst case per (module, width, type) of
the tables below -- measured by tests/test_modref_cpu.py, which fails when NOISE goes stale -- and MARGIN = max(1, ceil(4 N)); the GPU bound is
B = MARGIN u max(1, max |ref|), plus u max |ref| where the output itself is h16.  The floor of 1: the precise ResBlock has no rounding point here (N = 0), and what the
split-3 GEMM drops is far below one u: operands good to 2^-(2p) each and the lo x lo product, over K <= 2304 terms, against u = 2^-p.
"""
import functools
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fusedref import TD, U, _r, _Rn, _w, gn_affine  # noqa: E402

from videovanish_amd.weights import SyntheticWeights  # noqa: E402

LOG2E = 1.4426950408889634
HEADS, GROUPS, TEXT_LEN, CROSS, TEMB = 8, 32, 77, 768, 1280

# measured noise floors, worst case per (module, width, type): tests/test_modref_cpu.py::test_noise_floor_and_margin
NOISE = {
    ("resblock", 256, "fp16"): 0.000, ("resblock", 256, "bf16"): 0.000,          # the precise (VAE) form
    ("resblock", 320, "fp16"): 0.411, ("resblock", 320, "bf16"): 0.424,
    ("resblock", 640, "fp16"): 0.780, ("resblock", 640, "bf16"): 0.789,          # (the h16-output case: its own rounding is 0.5 of it)
    ("resblock", 1280, "fp16"): 0.5001, ("resblock", 1280, "bf16"): 0.510,        # (fp16: 0.500024, just past the step of ceil(4 N) from 2 to 3)
    ("spatial", 320, "fp16"): 1.448, ("spatial", 320, "bf16"): 1.421,
    ("spatial", 640, "fp16"): 1.392, ("spatial", 640, "bf16"): 1.605,
    ("spatial", 1280, "fp16"): 1.693, ("spatial", 1280, "bf16"): 1.683,
    ("motion", 320, "fp16"): 0.791, ("motion", 320, "bf16"): 0.767,
    ("motion", 640, "fp16"): 0.905, ("motion", 640, "bf16"): 0.924,
    ("motion", 1280, "fp16"): 0.770, ("motion", 1280, "bf16"): 0.773,
    ("vae_attn", 512, "fp16"): 0.409, ("vae_attn", 512, "bf16"): 0.366,
}


def margin_of(n):
    return max(1, int(math.ceil(4.0 * n)))


def _ln(t, gb):
    g, b = gb
    mean, var = t.mean(-1, keepdim=True), t.var(-1, unbiased=False, keepdim=True)
    return (t - mean) * torch.rsqrt(var + 1e-5) * g.double() + b.double()


def _lin(P, name, x, cin, cout, td, bias=True, w_scale=1.0, precise=False):
    w, b = P.linear(name, cin, cout, 1.0, bias)
    w = w * w_scale if w_scale != 1.0 else w
    y = x @ (w.double() if precise else _w(w, td)).t()
    return y + b.double() if bias else y


def _conv(P, name, x, Fr, H, W, cin, cout, k, td, precise=False, bias=True):
    """rows [Fr * H * W, cin] -> rows [Fr * H * W, cout]: k x k convolution, padding k // 2"""
    w, b = P.conv(name, cin, cout, k)
    w = w.double() if precise else _w(w, td)
    if k == 1:
        y = x @ w.reshape(cout, cin).t()
    else:
        y = F.conv2d(x.view(Fr, H, W, cin).permute(0, 3, 1, 2), w, None, padding=k // 2).permute(0, 2, 3, 1).reshape(Fr * H * W, cout)
    return y + b.double() if bias else y


def _attn(q, k, v, heads, td, on, cq, d_major=False):
    """softmax(q k^T) v per head: q [B, Nq, C], k / v [B or 1, Nk, C] (float64 holding h16 values) -> R(o) [B, Nq, C].  cq multiplies the scores in the log2
    domain.  d_major: the (mutant) split channel = d * heads + head"""
    B, Nq, C = q.shape
    D = C // heads

    def split(z):
        if d_major:
            return z.reshape(z.shape[0], z.shape[1], D, heads).permute(0, 3, 1, 2)
        return z.reshape(z.shape[0], z.shape[1], heads, D).transpose(1, 2)
    s = (split(q) @ split(k).transpose(-1, -2)) * cq
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    o = _r((_r(p, td, on) @ split(v)) / p.sum(-1, keepdim=True), td, on)
    return (o.permute(0, 2, 3, 1) if d_major else o.transpose(1, 2)).reshape(B, Nq, C)


def _feed_forward(P, b, t, td, on, mut, res=None):
    """R(res + ff(R(LN3(t)))): the GEGLU product and the result are stored as h16"""
    C = t.shape[-1]
    n3 = _r(_ln(t, P.norm(b + ".norm3", C)), td, on)
    h = _lin(P, b + ".ff.net.0.proj", n3, C, 8 * C, td)
    v, g = h[..., :4 * C], h[..., 4 * C:]
    if mut == "geglu_value_gate_exchanged":
        v, g = g, v
    hp = _r(v * F.gelu(g), td, on)
    return _r((t if res is None else res) + _lin(P, b + ".ff.net.2", hp, 4 * C, C, td), td, on)


# ---------------------------------------------------------------------------------------------------------------------------
def resblock(P, name, x0, Fr, H, W, td, cout, groups=GROUPS, eps=1e-5, x1=None, silu_temb=None, row=0, res1=None, out16=False, precise=False, rounded=True,
             mut=None):
    """nn.ResBlock: x0 (| x1) [M, C0 (+ C1)], silu_temb [S, temb_dim] (the block takes row `row`), res1 [M, cout] -> (out [M, cout], intermediates)"""
    on, HW = rounded and not precise, H * W
    it = {}
    xs = [x0.double()] + ([x1.double()] if x1 is not None else [])
    if mut == "halves_exchanged":
        xs = xs[::-1]
    x = torch.cat(xs, 1)
    cin = x.shape[1]

    def norm(nm, z, stats_of=None):
        g, b = P.norm(nm, z.shape[1])
        a_, b_ = gn_affine((g, b, groups, eps), z if stats_of is None else stats_of, Fr, HW, pool=False)
        y = z.view(Fr, HW, -1) * a_[:, None] + b_[:, None]
        return _r(F.silu(y).reshape(Fr * HW, -1), td, on)
    it["norm1"] = h = norm(name + ".norm1", x)
    c1 = _conv(P, name + ".conv1", h, Fr, H, W, cin, cout, 3, td, precise, bias=False)
    b1 = P.conv(name + ".conv1", cin, cout, 3)[1].double()
    pre = c1 + b1
    if silu_temb is not None:
        r = row if mut != "temb_other_row" else (row + 1) % silu_temb.shape[0]
        b1 = b1 + _lin(P, name + ".time_emb_proj", _r(silu_temb[r].double(), td, on), silu_temb.shape[1], cout, td)
    if mut == "conv1_bias_twice":
        b1 = b1 + P.conv(name + ".conv1", cin, cout, 3)[1].double()
    it["conv1"] = h = c1 + b1
    it["norm2"] = h = norm(name + ".norm2", h, pre if mut == "norm2_stats_before_temb" else None)
    if cin != cout:
        sc = _conv(P, name + ".conv_shortcut", _r(x, td, on), Fr, H, W, cin, cout, 1, td, precise)
        if mut == "shortcut_skipped":
            sc = torch.zeros_like(sc)
    else:
        sc = x
    it["shortcut"] = sc
    out = _conv(P, name + ".conv2", h, Fr, H, W, cout, cout, 3, td, precise) + sc
    if res1 is not None and mut != "res1_dropped":
        out = out + res1.double()
    return _r(out, td, on and out16), it


# ---------------------------------------------------------------------------------------------------------------------------
def spatial_transformer(P, name, x, Fr, H, W, td, text, heads=HEADS, groups=GROUPS, out16=False, rounded=True, mut=None):
    """nn.SpatialTransformer, layer by layer: x [M, C], text [77, cross] fp32 -> (out [M, C], intermediates)"""
    on, HW, C = rounded, H * W, x.shape[1]
    D = C // heads
    it = {}
    g, b_ = P.norm(name + ".norm", C)
    a, b = gn_affine((g, b_, groups, 1e-5 if mut == "gn_eps_1e-5" else 1e-6), x, Fr, HW, pool=False)
    xd = x.double()
    it["norm"] = h = _r((xd.view(Fr, HW, C) * a[:, None] + b[:, None]).reshape(Fr * HW, C), td, on)
    it["proj_in"] = t = _conv(P, name + ".proj_in", h, Fr, H, W, C, C, 1, td)
    blk = name + ".transformer_blocks.0"
    # attn1: the query weights carry 40^-1/2 log2 e (before their rounding) at D = 40; elsewhere the core applies the factor to the scores
    pres = D == 40 or mut == "prescale_at_other_D"
    c = float(D) ** -0.5 * LOG2E
    n1 = _r(_ln(t, P.norm(blk + ".norm1", C)), td, on)
    q = _r(_lin(P, blk + ".attn1.to_q", n1, C, C, td, False, c if pres else 1.0), td, on)
    k = _r(_lin(P, blk + ".attn1.to_k", n1, C, C, td, False), td, on)
    v = _r(_lin(P, blk + ".attn1.to_v", n1, C, C, td, False), td, on)
    cq = 1.0 if D == 40 else c          # (the mutant: prescaled weights under a core that scales too)
    o = _attn(q.view(Fr, HW, C), k.view(Fr, HW, C), v.view(Fr, HW, C), heads, td, on, cq, d_major=mut == "heads_split_d_major").reshape(Fr * HW, C)
    it["attn1"] = t1 = t + _lin(P, blk + ".attn1.to_out.0", o, C, C, td)
    # attn2: the text K | V [77, 2C] projected once, h16, shared by every frame (k_bs = 0)
    n2 = _r(_ln(t1, P.norm(blk + ".norm2", C)), td, on)
    q = _r(_lin(P, blk + ".attn2.to_q", n2, C, C, td, False), td, on)
    tx = _r(text.double(), td, on)
    kt = _r(_lin(P, blk + ".attn2.to_k", tx, text.shape[1], C, td, False), td, on)
    vt = _r(_lin(P, blk + ".attn2.to_v", tx, text.shape[1], C, td, False), td, on)
    if mut == "cross_k_v_exchanged":
        kt, vt = vt, kt
    kt, vt = kt[None], vt[None]
    if mut == "text_per_frame_stride":          # a batch stride of one row: frame f reads rows f .. f + 76 of the [77, 2C] tensor, zeros behind it
        sh = lambda z: torch.stack([torch.cat([z[0, f:], torch.zeros(f, C, dtype=z.dtype)]) for f in range(Fr)])
        kt, vt = sh(kt), sh(vt)
    o = _attn(q.view(Fr, HW, C), kt, vt, heads, td, on, c).reshape(Fr * HW, C)
    it["attn2"] = t2 = t1 + _lin(P, blk + ".attn2.to_out.0", o, C, C, td)
    it["ff"] = t3 = _feed_forward(P, blk, t2, td, on, mut, res=t1 if mut == "ff_residual_before_attn2" else None)
    out = _conv(P, name + ".proj_out", t3, Fr, H, W, C, C, 1, td) + (t3 if mut == "proj_out_residual_t" else xd)
    return _r(out, td, on and out16), it


# ---------------------------------------------------------------------------------------------------------------------------
def motion_module(P, name, x, Fr, H, W, td, pe, heads=HEADS, groups=GROUPS, res1=None, out16=False, rounded=True, mut=None):
    """nn.MotionModule._run, layer by layer: x [Fr * HW, C] (rows frame-major), pe [max_seq, C] -> (out [Fr * HW, C], intermediates)"""
    on, HW, C = rounded, H * W, x.shape[1]
    M, D = Fr * HW, x.shape[1] // heads
    it = {}
    g, b_ = P.norm(name + ".norm", C)
    a, b = gn_affine((g, b_, groups, 1e-6), x, Fr, HW, pool=mut != "gn_per_frame")
    xd = x.double()
    it["norm"] = h = _r((xd.view(Fr, HW, C) * a[:, None] + b[:, None]).reshape(M, C), td, on)
    it["proj_in"] = t = _lin(P, name + ".proj_in", h, C, C, td)
    blk = name + ".transformer_blocks.0"
    rows = torch.arange(M)
    c = float(D) ** -0.5 * LOG2E
    n_first = None
    for i, an in enumerate(("attn1", "attn2")):
        n = _ln(t, P.norm(f"{blk}.norm{i + 1}", C))
        if not (mut == "pe_left_out_of_ln2" and i == 1):
            n = n + pe.double()[(rows % Fr) if mut == "pe_by_token" else (rows // HW)]
        n = _r(n, td, on)
        if i == 0:
            n_first = n
        elif mut == "attn2_reads_attn1_input":
            n = n_first
        q, k, v = (_r(_lin(P, f"{blk}.{an}.{nm}", n, C, C, td, False), td, on) for nm in ("to_q", "to_k", "to_v"))
        if mut == "gather_transposed":          # batch = row // F, sequence = row % F: the rows taken as [HW][F]
            seq = lambda z: z.view(HW, Fr, C)
            o = _attn(seq(q), seq(k), seq(v), heads, td, on, c).reshape(M, C)
        else:                                   # batch = pixel, sequence = frame: row = frame * HW + pixel
            seq = lambda z: z.view(Fr, HW, C).transpose(0, 1)
            o = _attn(seq(q), seq(k), seq(v), heads, td, on, c).transpose(0, 1).reshape(M, C)
        it[an] = t = t + _lin(P, f"{blk}.{an}.to_out.0", o, C, C, td)
    it["ff"] = t = _feed_forward(P, blk, t, td, on, mut)
    out = _lin(P, name + ".proj_out", t, C, C, td) + xd
    if res1 is not None and mut != "res1_dropped":
        out = out + res1.double()
    return _r(out, td, on and out16), it


# ---------------------------------------------------------------------------------------------------------------------------
def vae_mid_attn(P, name, x, Fr, H, W, td, groups=GROUPS, precise=False, rounded=True, mut=None):
    """vae._MidAttn: one head over C channels, projections with bias: x [M, C] -> (out [M, C], intermediates)"""
    on, HW, C = rounded, H * W, x.shape[1]
    it = {}
    g, b_ = P.norm(name + ".group_norm", C)
    a, b = gn_affine((g, b_, groups, 1e-6), x, Fr, HW, pool=False)
    xd = x.double()
    h = (xd.view(Fr, HW, C) * a[:, None] + b[:, None]).reshape(Fr * HW, C)
    if mut == "gn_with_silu":
        h = F.silu(h)
    it["norm"] = h = _r(h, td, on and not precise)
    q, k, v = (_r(_lin(P, f"{name}.{nm}", h, C, C, td, True, precise=precise), td, on).view(Fr, HW, C) for nm in ("to_q", "to_k", "to_v"))
    it["o"] = o = _attn(q, k, v, 1, td, on, float(C) ** -0.5 * LOG2E).reshape(Fr * HW, C)
    out = _lin(P, name + ".to_out.0", o, C, C, td, precise=precise)
    if mut != "residual_dropped":
        out = out + xd
    return out, it


# ---------------------------------------------------------------------------------------------------------------------------
# the tables of the GPU test and their inputs.  `path`: how the GPU test makes sure the layer path ran ("width": no fused kernel at this width;
# "switch": the class switch FUSED = False; "own": the module's own fallback condition with FUSED = True).
# The attention routes these sizes take (hip.attention_route, either type), none of them degenerate -- every one has a ragged last query and K/V tile:
#   spatial  150 tokens, D = 80: reg80 self / reg80 cross;  78 tokens, D = 160: w4x32 for both;  150 tokens, D = 40: mfma32-d40 ragged / dma64 cross;  8 tokens: short / dma64 cross
#   motion   short (short-2w at C = 1280, F = 32)          vae  d512-w4
# and both 3x3 convolutions of the 32 x 64 ResBlock run halo+gn 128x160 (hip.conv_gemm_route; asserted by the GPU test)
L0, L1, L2 = "unet.down_blocks.0", "unet.down_blocks.1", "unet.down_blocks.2"
SPATIAL_CASES = [      # token counts 150 / 78 / 8: no multiple of 64, ragged query and K/V tiles
    dict(name=L1 + ".attentions.0", C=640, F=2, H=10, W=15, out16=False, path="width", amp=0.004),      # var(x) about 1e-5: the GroupNorm eps is visible
    dict(name=L1 + ".attentions.0", C=640, F=2, H=10, W=15, out16=True, path="width", amp=1.0),
    dict(name=L2 + ".attentions.0", C=1280, F=2, H=6, W=13, out16=False, path="width", amp=0.1),
    dict(name=L2 + ".attentions.0", C=1280, F=1, H=6, W=13, out16=True, path="width", amp=0.1),
    dict(name=L0 + ".attentions.0", C=320, F=2, H=10, W=15, out16=False, path="switch", amp=0.1),
    dict(name=L0 + ".attentions.0", C=320, F=2, H=2, W=4, out16=False, path="own", amp=0.1),             # HW = 8 < hip.CHAIN_FRONT_MIN_HW
]
MOTION_CASES = [
    dict(name=L1 + ".motion_modules.0", C=640, F=32, H=3, W=4, res1=False, out16=False, path="width", amp=0.1),
    dict(name=L1 + ".motion_modules.0", C=640, F=22, H=1, W=5, res1=True, out16=True, path="width", amp=0.1),
    dict(name=L1 + ".motion_modules.0", C=640, F=1, H=1, W=7, res1=False, out16=False, path="width", amp=1.0),
    dict(name=L2 + ".motion_modules.0", C=1280, F=32, H=2, W=3, res1=False, out16=False, path="width", amp=0.1),
    dict(name=L2 + ".motion_modules.0", C=1280, F=3, H=4, W=5, res1=True, out16=False, path="width", amp=1.0),
    dict(name=L0 + ".motion_modules.0", C=320, F=15, H=2, W=4, res1=False, out16=False, path="own", amp=0.1),          # F < 16
    dict(name=L0 + ".motion_modules.0", C=320, F=32, H=2, W=3, res1=True, out16=False, path="own", amp=0.1),           # HW % 4 != 0
    dict(name=L0 + ".motion_modules.0", C=320, F=32, H=2, W=4, res1=False, out16=False, path="own", amp=0.1, x16=True),  # an h16 x
]
RES_CASES = [      # C0 (| C1) -> cout
    dict(name=L1 + ".resnets.0", C0=320, C1=0, cout=640, F=2, H=7, W=9, temb=True, res1=False, out16=False),
    dict(name="unet.up_blocks.3.resnets.0", C0=640, C1=320, cout=320, F=2, H=7, W=9, temb=True, res1=False, out16=False),
    dict(name="unet.up_blocks.1.resnets.0", C0=1280, C1=1280, cout=1280, F=1, H=4, W=5, temb=True, res1=False, out16=False),
    dict(name=L1 + ".resnets.1", C0=640, C1=0, cout=640, F=2, H=5, W=6, temb=True, res1=True, out16=True),
    dict(name=L0 + ".resnets.0", C0=320, C1=0, cout=320, F=1, H=32, W=64, temb=True, res1=False, out16=False, want_gn=True),      # H W = 2048, exact 8 x 16 cover: GroupNorm partials from conv1 and conv2
    dict(name=L0 + ".resnets.0", C0=320, C1=0, cout=320, F=1, H=31, W=64, temb=True, res1=False, out16=False, want_gn=True),      # below the threshold: gn is None
    dict(name="vae.encoder.down_blocks.1.resnets.0", C0=128, C1=0, cout=256, F=1, H=9, W=11, temb=False, res1=False, out16=False, eps=1e-6, precise=True),
    # the model's convolution biases are N(0, 0.02^2): one counted twice stays below the bf16 bound.  This case draws them 50 times larger (BigBias), small x
    dict(name=L1 + ".resnets.0", C0=320, C1=0, cout=640, F=1, H=4, W=5, temb=True, res1=False, out16=False, amp=0.2, weights="big_bias"),
]
VAE_NAME = "vae.decoder.mid_block.attentions.0"
VAE_CASES = [dict(name=VAE_NAME, C=512, F=1, H=8, W=10, precise=True), dict(name=VAE_NAME, C=512, F=1, H=8, W=10, precise=False),
             dict(name=VAE_NAME, C=512, F=1, H=10, W=15, precise=True), dict(name=VAE_NAME, C=512, F=1, H=10, W=15, precise=False)]
CASES = {"resblock": RES_CASES, "spatial": SPATIAL_CASES, "motion": MOTION_CASES, "vae_attn": VAE_CASES}
TEMB_ROW = 1          # the row of the two-row silu_temb the ResBlock cases use


def width(kind, cs):
    return cs["cout"] if kind == "resblock" else cs["C"]


def frame_x(rn, Fr, HW, C, amp):
    """x whose frames differ in mean and spread (per-frame against pooled statistics)"""
    s = torch.tensor([0.5, 1.5, 1.0, 2.5])[torch.arange(Fr) % 4]
    m = torch.tensor([-1.0, 2.0, 0.5, -2.0])[torch.arange(Fr) % 4]
    return ((rn(Fr, HW, C) * s[:, None, None] + m[:, None, None]) * amp).reshape(Fr * HW, C).contiguous()


def pos_table(C, n=32):
    from oracle.model_ref import sinusoidal_pos_emb
    return sinusoidal_pos_emb(n, C)


def edge_inputs(kind, case, td, seed=0):
    """the activations of one case of CASES[kind] -> dict of fp32 tensors (an `x16` x holds td values)"""
    cs = CASES[kind][case]
    rn = _Rn(1000 * seed + 31 * case + {"resblock": 5, "spatial": 6, "motion": 7, "vae_attn": 8}[kind])
    Fr, HW = cs["F"], cs["H"] * cs["W"]
    if kind == "resblock":
        d = dict(x0=frame_x(rn, Fr, HW, cs["C0"], cs.get("amp", 1.0)))
        d["x1"] = frame_x(rn, Fr, HW, cs["C1"], 3.0) if cs["C1"] else None          # the two sources differ in scale
        d["temb"] = rn(2, TEMB) * torch.tensor([[1.0], [2.0]]) + torch.tensor([[0.5], [-0.5]]) if cs["temb"] else None      # two timesteps: rows differ
        d["silu_temb"] = F.silu(d["temb"]) if cs["temb"] else None
        d["res1"] = rn(Fr * HW, cs["cout"]) if cs["res1"] else None
        return d
    if kind == "spatial":
        scale = 0.5 + 1.5 * torch.rand(TEXT_LEN, 1, generator=rn.g)          # text rows of different size; row 0 the largest: it holds mass a shifted read would lose
        scale[0] = 3.0
        return dict(x=frame_x(rn, Fr, HW, cs["C"], cs["amp"]), text=rn(TEXT_LEN, CROSS) * scale)
    if kind == "motion":
        x = frame_x(rn, Fr, HW, cs["C"], cs["amp"])
        if cs.get("x16"):
            x = x.to(td).float()
        return dict(x=x, res1=cs["amp"] * rn(Fr * HW, cs["C"]) if cs["res1"] else None)
    return dict(x=frame_x(rn, Fr, HW, cs["C"], 1.0))


def run(kind, case, inp, td, rounded=True, mut=None, P=None):
    """the reference of one case on the inputs `inp` -> (out float64, intermediates)"""
    P = _params(CASES[kind][case].get("weights")) if P is None else P
    cs = CASES[kind][case]
    Fr, H, W = cs["F"], cs["H"], cs["W"]
    if kind == "resblock":
        return resblock(P, cs["name"], inp["x0"], Fr, H, W, td, cs["cout"], eps=cs.get("eps", 1e-5), x1=inp["x1"], silu_temb=inp["silu_temb"], row=TEMB_ROW,
                        res1=inp["res1"], out16=cs["out16"], precise=cs.get("precise", False), rounded=rounded, mut=mut)
    if kind == "spatial":
        return spatial_transformer(P, cs["name"], inp["x"], Fr, H, W, td, inp["text"], out16=cs["out16"], rounded=rounded, mut=mut)
    if kind == "motion":
        return motion_module(P, cs["name"], inp["x"], Fr, H, W, td, pos_table(cs["C"]), res1=inp["res1"], out16=cs["out16"], rounded=rounded, mut=mut)
    return vae_mid_attn(P, cs["name"], inp["x"], Fr, H, W, td, precise=cs["precise"], rounded=rounded, mut=mut)


class BigBias(SyntheticWeights):
    """the model's seeded weights with convolution biases 50 times larger (N(0, 1)); also a Ctx(weights=) source"""

    def conv(self, name, cin, cout, k, gain=1.0):
        w, b = super().conv(name, cin, cout, k, gain)
        return w, 50.0 * b


@functools.lru_cache(maxsize=None)
def _params(weights=None):
    from oracle.model_ref import Params
    P = Params(0)
    if weights == "big_bias":
        P.src = BigBias(0)
    return P


@functools.lru_cache(maxsize=None)
def inputs(kind, case, dname):
    return edge_inputs(kind, case, TD[dname])


@functools.lru_cache(maxsize=None)
def reference(kind, case, dname, rounded=True):
    """(out, intermediates), computed once per process and shared; callers must not modify it"""
    with torch.no_grad():
        return run(kind, case, inputs(kind, case, dname), TD[dname], rounded)


def bound(kind, case, dname, ref):
    """B = MARGIN u max(1, max |ref|), + u max |ref| for an h16 output (its own rounding)"""
    cs = CASES[kind][case]
    u, top = U[TD[dname]], ref.abs().max().item()
    return margin_of(NOISE[(kind, width(kind, cs), dname)]) * u * max(1.0, top) + (u * top if cs.get("out16") else 0.0)


def noise(kind, case, dname):
    a, b = reference(kind, case, dname, True)[0], reference(kind, case, dname, False)[0]
    return (a - b).abs().max().item() / (U[TD[dname]] * max(1.0, a.abs().max().item()))


# mutant -> index of the case (CASES) assigned to it: tests/test_modref_cpu.py holds every one at least 2 B from the unmutated reference
MUTANTS = {
    "motion": {"gn_per_frame": 0, "pe_by_token": 0, "pe_left_out_of_ln2": 0, "gather_transposed": 0, "attn2_reads_attn1_input": 0, "res1_dropped": 1},
    "spatial": {"gn_eps_1e-5": 0, "cross_k_v_exchanged": 2, "text_per_frame_stride": 2, "heads_split_d_major": 2, "prescale_at_other_D": 2,
                "geglu_value_gate_exchanged": 2, "ff_residual_before_attn2": 2, "proj_out_residual_t": 2},
    "resblock": {"halves_exchanged": 1, "shortcut_skipped": 0, "temb_other_row": 0, "conv1_bias_twice": 7, "norm2_stats_before_temb": 0, "res1_dropped": 3},
    "vae_attn": {"residual_dropped": 1, "gn_with_silu": 1},
}


def diagnose(kind, case, dname, got):
    """failure messages: the size of the reference's intermediates, and the mutants of this case that `got` (float64, CPU) meets within B -- a wrong result that equals
    a mutant names the mistake"""
    ref, it = reference(kind, case, dname)
    B = bound(kind, case, dname, ref)
    near = []
    for mut in MUTANTS[kind]:
        try:
            with torch.no_grad():
                m = run(kind, case, inputs(kind, case, dname), TD[dname], True, mut)[0]
        except (RuntimeError, IndexError):          # a mutant that does not apply to this case's shape
            continue
        if (m - ref).abs().max().item() >= 2.0 * B and (got - m).abs().max().item() <= B:          # (a mutant that changes nothing on this case says nothing)
            near.append(mut)
    return f"equals mutant(s) {near or 'none'}; reference intermediates max |.|: " + ", ".join(f"{k} {v.abs().max().item():.3g}" for k, v in it.items())
