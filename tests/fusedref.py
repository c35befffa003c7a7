"""fp64 host references of the three fused level-0 kernels (csrc/vv_chain.hip: chain_front_rs_c320_kernel, chain_rs_c320_kernel; csrc/vv_motion.hip:
motion_c320_kernel), inputs that turn each structural mistake of those kernels into an O(1) error, and the mutants that prove it.  Plain torch in
float64 on the CPU; shared by tests/test_fusedref_cpu.py and tests/test_fused_kernels_gpu.py, not a conftest.

Every function takes the LOGICAL weight dict of packing.pack_chain_front_stream / pack_chain_stream / pack_motion_stream (the keys assembled in
nn.SpatialTransformer.__init__ / nn.MotionModule.__init__), fp32 tensors, and the h16 type `td` of the kernel (torch.float16 / torch.bfloat16;
torch.float32 = nothing is rounded at all: the tie to oracle/model_ref.py).  Weights are always rounded to td.  `rounded=True` also rounds the
activations to td exactly where the kernels do (fp32 -> h16, round to nearest even); `rounded=False` is the same arithmetic without those roundings.

Rounding points (file:line of the statement each one restates)
  front (vv_chain.hip)
    weights                  packing._slab: out.to(h16)
    GroupNorm-applied x      429  own[rb][tt] = make_uint4(pack2<T>(x0.x * g0.x + b0.x, ...
    t = Win a + bin          457  stored as fp32: not rounded
    LN1 output               497  own[rb][tt] = rs_frag<T>(y[0], y[1])
    q | k | v store          524  *(uint2*)(qkv + tokbase[tt] + off) = make_uint2(pack2<T>(acc...
  tail (vv_chain.hip; LayerNorm in vv_chain_rs.h)
    weights, text K / V      packing._slab
    o                        92   read as h16 (the attention core's output)
    LN2 / LN3 output         vv_chain_rs.h 158  own[rb][tt] = rs_frag<T>(y[0], y[1])
    q                        181  q0 = frag(qa[0], qa[1]), q1 = frag(qa[2], z4)
    scores                   203  exp2(sT * sc - mc) on fp32 scores, sc = 40^-1/2 log2 e: not rounded; l sums the fp32 values
    P before normalisation   206  pf0 = frag(sT[0], sT[1]) ...
    per-head O after * inv   219  *(uint4*)dst = frag(oT[0], oT[1])
    GEGLU product            274  hown[tt] = frag(hv[0], hv[1])
    trunk before proj_out    294  own[rb][tt] = frag(t[2 * rb][tt], t[2 * rb + 1][tt])
    h16 output               337  pack2<T>(v0, v1)
  motion (vv_motion.hip)
    weights                  packing._slab
    GroupNorm-applied x      90   a[s][tt] = make_uint4(pack2<T>(x0.x * a0.x + b0.x, ...
    LN1 / LN2 (+ pe) / LN3   195  a[s2][tt] = frag(y[0], y[1])
    q, k                     219-220  qf / kf = frag(qa.. / ka..)
    v                        261  vf = frag(va[dt][0], va[dt][1])
    scores                   251  exp2 on fp32 scores: not rounded; l sums the fp32 values
    P before normalisation   254  pf[qt] = frag(sT[0][qt], sT[1][qt])
    per-head O after * inv   270  of[tt][0] = frag(oT[0][tt], oT[1][tt])
    GEGLU product            314  hf0[tt] = frag(hv[0], hv[1])
    trunk before proj_out    326  a[s2][tt] = frag(t[2 * s2][tt], t[2 * s2 + 1][tt])
    h16 output               365  pack2<T>(v0, v1)
GELU is the exact erf form.  GroupNorm statistics are fp64 over x (per frame: front; pooled over the clip: motion), the affine is that of
vv_gn_affine(_frames): a = rstd gamma, b = beta - mean a.

Noise floor N = max |ref(rounded) - ref(unrounded)| / (u max(1, max |ref(rounded)|)), u = 2^-11 (fp16) / 2^-8 (bf16), the worst case of each kernel's
table below (measured by tests/test_fusedref_cpu.py, which fails when these figures go stale), and the factor K = ceil(4 N) of the GPU bound
B = K u max(1, max |ref|):
            fp16 N   K     bf16 N   K
    front   0.987    4     0.950    4
    tail    1.041    5     0.941    4
    motion  2.341   10     2.404   10      (marker keys that share a query's mass: a rounding of k at a score of 36 shifts that share; k accounts for half of N)
These are NOISE and MARGIN below.
"""
import functools
import math

import torch
import torch.nn.functional as F

C, HEADS, D, NKEY = 320, 8, 40, 77
SCALE = float(D) ** -0.5
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TD = {"fp16": torch.float16, "bf16": torch.bfloat16}
SENTINEL = 1000.0          # exact in fp32, fp16 and bf16

# measured noise floors (worst case of each table) and the margins derived from them: B = MARGIN u max(1, max |ref|)
NOISE = {("front", "fp16"): 0.987, ("front", "bf16"): 0.950, ("tail", "fp16"): 1.041, ("tail", "bf16"): 0.941, ("motion", "fp16"): 2.341, ("motion", "bf16"): 2.404}
MARGIN = {("front", "fp16"): 4, ("front", "bf16"): 4, ("tail", "fp16"): 5, ("tail", "bf16"): 4, ("motion", "fp16"): 10, ("motion", "bf16"): 10}

HI = (torch.arange(C) % 64) >= 32          # the channels the hf = 1 wave of a row-split pair owns (vv_chain_rs.h rs_chan)


def _w(t, td):
    return t.to(td).double() if td in U else t.double()


def _r(t, td, on):
    """fp32 -> td, round to nearest even, as pack2<T> does"""
    return t.float().to(td).double() if (on and td in U) else t


def _ln(t, g, b, merged_without_between=False):
    if merged_without_between:          # the pair merge of rs_layer_norm without 80 dm^2: M2 of the two 160-channel halves only
        lo, hi = t[..., ~HI], t[..., HI]
        m0, m1 = lo.mean(-1, keepdim=True), hi.mean(-1, keepdim=True)
        mean = 0.5 * (m0 + m1)
        var = (((lo - m0) ** 2).sum(-1, keepdim=True) + ((hi - m1) ** 2).sum(-1, keepdim=True)) / C
    else:
        mean, var = t.mean(-1, keepdim=True), t.var(-1, unbiased=False, keepdim=True)
    return (t - mean) * torch.rsqrt(var + 1e-5) * g + b


def gn_affine(gn, x, Fr, HW, pool):
    """(a, b) [Fr, C] float64 of the GroupNorm gn = (gamma, beta, groups, eps) over x [Fr * HW, C]: statistics per frame, or pooled over the clip"""
    gamma, beta, groups, eps = gn
    Cc = x.shape[-1]          # (any width: tests/modref.py shares this)
    xd = x.double().view(Fr, HW, groups, Cc // groups)
    dims = (0, 1, 3) if pool else (1, 3)
    mean = xd.mean(dim=dims, keepdim=True).expand(Fr, 1, groups, 1)
    var = xd.var(dim=dims, unbiased=False, keepdim=True).expand(Fr, 1, groups, 1)
    rstd = torch.rsqrt(var + eps)
    a = rstd.expand(Fr, 1, groups, Cc // groups).reshape(Fr, Cc) * gamma.double()
    b = beta.double() - mean.expand(Fr, 1, groups, Cc // groups).reshape(Fr, Cc) * a
    return a, b


def _geglu(n3, w, td, on, mut):
    """R(value * gelu(gate)) [M, 1280] of ff1; the GEGLU mutants act on 16-unit groups (packing: rows interleaved per 16 hidden units)"""
    inner = 4 * C
    b1 = w["ff1.b"].double().clone()
    if mut == "ff1_bias_next_chunk":          # the bias of group G1 read from the chunk behind it (64 hidden units on)
        for base in (0, inner):
            b1[base + 16 * G1:base + 16 * G1 + 16] = w["ff1.b"].double()[base + 16 * G1 + 64:base + 16 * G1 + 80]
    hfull = n3 @ _w(w["ff1.w"], td).t() + b1
    v, g = hfull[..., :inner].clone(), hfull[..., inner:].clone()
    if mut == "value_gate_exchanged":
        s = slice(16 * G1, 16 * G1 + 16)
        v[..., s], g[..., s] = hfull[..., inner:][..., s], hfull[..., :inner][..., s]
    h = v * F.gelu(g)
    if mut == "geglu_groups_swapped":
        a, b = slice(16 * G1, 16 * G1 + 16), slice(16 * G2, 16 * G2 + 16)
        h2 = h.clone()
        h2[..., a], h2[..., b] = h[..., b], h[..., a]
        h = h2
    return _r(h, td, on)


G1, G2 = 5, 6          # the two 16-unit GEGLU groups of the mutants: neighbours inside chunk 1 (units 80..95 and 96..111: row halves hf = 0 / 1 of the tail)
MH = 2                 # the head of the per-head mutants
NEG_HEAD = 5           # tail: the head whose real scores all lie far below 0 (a phantom key would take the mass)


# ---------------------------------------------------------------------------------------------------------------------------
# front
def front(w, gn, x, Fr, HW, td, rounded=True, mut=None):
    """-> (t [M, C], qkv [Fr][3][8][HW][40]) float64"""
    M = Fr * HW
    a, b = gn_affine(gn, x, Fr, HW, pool=False)
    fr = torch.arange(M) // HW
    fa = fr.clone()
    if mut in ("gn_affine_prev_frame", "gn_affine_next_frame"):          # tokens behind / before a frame boundary inside a 128-token block take the neighbour's affine
        blk = (torch.arange(M) // 128) * 128
        if mut == "gn_affine_prev_frame":
            fa = torch.where(fr > blk // HW, fr - 1, fr)
        else:
            fa = torch.where(fr < torch.clamp(blk + 127, max=M - 1) // HW, fr + 1, fr)
    h = _r(x.double() * a[fa] + b[fa], td, rounded)
    t = h @ _w(w["in.w"], td).t() + w["in.b"].double()
    n1 = _r(_ln(t, w["ln1.g"].double(), w["ln1.b"].double(), mut == "ln1_merge_term_omitted"), td, rounded)
    qkv = _r(n1 @ _w(w["qkv.w"], td).t(), td, rounded)                     # [M, 3C]: q | k | v, channel = head * 40 + d
    out = qkv.view(Fr, HW, 3, HEADS, D).permute(0, 2, 3, 1, 4).contiguous()
    if mut == "token_in_next_frame_slot":          # the last token of every frame but the last lands in the following frame's slot (same token index), which loses its own
        out[1:, :, :, HW - 1] = out[:-1, :, :, HW - 1].clone()
        out[0, :, :, HW - 1] = 0.0
    elif mut == "planes_permuted":
        out = out[:, [1, 2, 0]].contiguous()
    elif mut == "head_piece_off_by_one":           # channels 40..43 (head 1, d = 0..3) decomposed as head 0, d = 40..43 = head 0, next token, d = 0..3
        flat = out.clone()
        flat[:, :, 0, 1:, 0:4] = out[:, :, 1, :-1, 0:4]
        flat[:, :, 1, :, 0:4] = 0.0
        out = flat
    return t, out


# ---------------------------------------------------------------------------------------------------------------------------
# tail
def o_head_major(o, o_hw):
    """logical o [M, C] -> the head-major buffer [M / o_hw][8][o_hw][40] vv_attention writes (o_hs = o_hw * 40)"""
    M = o.shape[0]
    return o.view(M // o_hw, o_hw, HEADS, D).permute(0, 2, 1, 3).contiguous()


def tail(w, o, t_in, x, res1, td, rounded=True, mut=None, out_h16=False, o_hw=0):
    """-> out [M, C] float64.  o: the LOGICAL [M, C] attention output (h16 values); o_hw only matters to the head-major mutant"""
    M = t_in.shape[0]
    od = o.double()
    if mut == "o_frame_offset_of_group":          # head-major o: the frame of a 32-token group's first row used for all its rows (token offset runs past the frame)
        assert o_hw > 0
        buf = o_head_major(od, o_hw).reshape(-1)
        r = torch.arange(M)
        fr = ((r // 32) * 32) // o_hw
        tk = r - fr * o_hw
        c = torch.arange(C)
        idx = (fr * o_hw * C)[:, None] + ((c // D) * o_hw * D + c % D)[None, :] + (tk * D)[:, None]
        od = buf[idx.clamp(max=buf.numel() - 1)]
    t = t_in.double() + od @ _w(w["o1.w"], td).t() + w["o1.b"].double()
    nomerge = mut == "ln_merge_term_omitted"
    n2 = _r(_ln(t, w["ln2.g"].double(), w["ln2.b"].double(), nomerge), td, rounded)
    q = _r(n2 @ _w(w["q2.w"], td).t(), td, rounded).view(M, HEADS, D).transpose(0, 1)          # [8, M, 40]
    K = _w(w["k2"], td).view(NKEY, HEADS, D).permute(1, 0, 2)
    V = _w(w["v2"], td).view(NKEY, HEADS, D).permute(1, 0, 2)
    s = q @ K.transpose(1, 2)                                                                      # [8, M, 77]
    if mut == "key76_dropped":
        s[MH, :, 76] = -float("inf")
    m = s.amax(-1, keepdim=True)
    extra = torch.zeros_like(m)
    if mut == "phantom_key77":                     # a zero K row: score 0, a zero V row: it only joins the maximum and the denominator
        m[NEG_HEAD] = m[NEG_HEAD].clamp(min=0.0)
    p = torch.exp((s - m) * SCALE)
    if mut == "phantom_key77":
        extra[NEG_HEAD] = torch.exp((0.0 - m[NEG_HEAD]) * SCALE)
    l = p.sum(-1, keepdim=True) + extra
    O = _r((_r(p, td, rounded) @ V) / l, td, rounded)                                            # [8, M, 40]
    if mut == "head_o_in_next_head":
        O = O.clone()
        O[[MH, MH + 1]] = O[[MH + 1, MH]]
    t = t + O.transpose(0, 1).reshape(M, C) @ _w(w["o2.w"], td).t() + w["o2.b"].double()
    n3 = _r(_ln(t, w["ln3.g"].double(), w["ln3.b"].double(), nomerge), td, rounded)
    t = t + _geglu(n3, w, td, rounded, mut) @ _w(w["ff2.w"], td).t() + w["ff2.b"].double()
    out = _r(t, td, rounded) @ _w(w["out.w"], td).t() + w["out.b"].double() + x.double()
    if res1 is not None and mut != "res1_omitted":
        out = out + res1.double()
    if mut == "last_row_duplicated":
        out = out.clone()
        out[M - 2] = out[M - 1]
    return _r(out, td, rounded and out_h16)


# ---------------------------------------------------------------------------------------------------------------------------
# motion module
def motion(w, gn, x, res1, Fr, HW, td, rounded=True, mut=None, out_h16=False):
    """-> out [Fr * HW, C] float64 (rows frame-major, as the kernel's)"""
    a, b = gn_affine(gn, x, Fr, HW, pool=mut != "gn_per_frame")
    h = _r(x.double().view(Fr, HW, C) * a[:, None] + b[:, None], td, rounded)
    t = h @ _w(w["proj_in.w"], td).t() + w["proj_in.b"].double()                                  # [Fr, HW, C]
    pe = w["pe"][:32].double()
    fidx = torch.arange(Fr)
    if mut == "pe_next_frame":
        fidx = (fidx + 1).clamp(max=31)
    elif mut == "pe_prev_frame":
        fidx = (fidx - 1).clamp(min=0)
    pe = pe[fidx][:, None]                                                                          # [Fr, 1, C]
    names = ("attn1", "attn2") if mut != "attn_weights_exchanged" else ("attn2", "attn1")
    for i, a_ in enumerate(names):
        g_, b_ = w[f"ln{i + 1}.g"].double(), w[f"ln{i + 1}.b"].double()
        n = _ln(t, g_, b_)
        if not (mut == "pe_left_out_of_ln2" and i == 1):
            n = n + pe
        n = _r(n, td, rounded)
        heads = lambda z: _r(z, td, rounded).view(Fr, HW, HEADS, D).permute(1, 2, 0, 3)          # [HW, 8, Fr, 40]
        q, k, v = (heads(n @ _w(w[f"{a_}.{nm}"], td).t()) for nm in ("q", "k", "v"))
        if mut == "d32_dropped_in_scores" and i == 0:
            q = q.clone()
            q[:, MH, :, 32:] = 0.0
        s = q @ k.transpose(-1, -2)                                                                # [HW, 8, Fr(query), Fr(key)]
        if mut == "key_mask_at_F_plus_1" and Fr < 32:          # row F of the wave repeats frame F - 1: one more copy of that key
            s = torch.cat([s, s[..., -1:]], -1)
            v = torch.cat([v, v[..., -1:, :]], -2)
        m = s.amax(-1, keepdim=True)
        p = torch.exp((s - m) * SCALE)
        O = _r((_r(p, td, rounded) @ v) / p.sum(-1, keepdim=True), td, rounded)                   # [HW, 8, Fr, 40]
        if mut == "d32_dropped_in_out_proj" and i == 0:
            O = O.clone()
            O[:, MH, :, 32:] = 0.0
        t = t + O.permute(2, 0, 1, 3).reshape(Fr, HW, C) @ _w(w[f"{a_}.o"], td).t() + w[f"{a_}.ob"].double()
    n3 = _r(_ln(t, w["ln3.g"].double(), w["ln3.b"].double()), td, rounded)
    t = t + _geglu(n3, w, td, rounded, mut) @ _w(w["ff2.w"], td).t() + w["ff2.b"].double()
    out = _r(t, td, rounded) @ _w(w["proj_out.w"], td).t() + w["proj_out.b"].double() + x.double().view(Fr, HW, C)
    if res1 is not None:
        out = out + res1.double().view(Fr, HW, C)
    return _r(out.reshape(Fr * HW, C), td, rounded and out_h16)


# ---------------------------------------------------------------------------------------------------------------------------
# the tables of the GPU test and their inputs
TAIL_CASES = [      # M, o_hw, res1, h16 output, large residuals
    dict(M=128, o_hw=0, res1=False, out16=False),          # one whole block
    dict(M=126, o_hw=0, res1=True, out16=False),           # ragged inside the last pair group
    dict(M=97, o_hw=0, res1=False, out16=True),            # ragged at a pair-group edge + 1, h16 output
    dict(M=1, o_hw=0, res1=True, out16=False),
    dict(M=129, o_hw=0, res1=False, out16=False),
    dict(M=384, o_hw=0, res1=True, out16=True),
    dict(M=200, o_hw=50, res1=True, out16=False),          # head-major o, frame boundaries inside 32-token groups
    dict(M=648, o_hw=9, res1=False, out16=False),
    dict(M=126, o_hw=0, res1=True, out16=True, big=True),  # large x and res1: the residual add itself, ragged h16 store
]
FRONT_CASES = [dict(F=72, HW=9), dict(F=2, HW=64), dict(F=3, HW=42), dict(F=1, HW=384), dict(F=5, HW=27), dict(F=1, HW=9)]
MOTION_CASES = [      # F, HW, res1, h16 output
    dict(F=32, HW=20, res1=False, out16=False), dict(F=31, HW=8, res1=True, out16=False), dict(F=22, HW=4, res1=False, out16=True),
    dict(F=17, HW=8, res1=True, out16=True), dict(F=16, HW=4, res1=True, out16=False), dict(F=15, HW=20, res1=False, out16=False),
    dict(F=2, HW=4, res1=True, out16=True), dict(F=1, HW=8, res1=False, out16=False),
    dict(F=22, HW=4, res1=True, out16=False, big=True),
]
CASES = {"front": FRONT_CASES, "tail": TAIL_CASES, "motion": MOTION_CASES}

SEL = (8, 40, 72, 104)            # tail: trunk channels that select a token's marker key (two in each half of a row-split pair)
BIAS_CH = 136                     # tail: LN2 output channel that is 1 for every token (gamma 0, beta 1)
MARK = (0, 63, 64, 76)            # tail: marker text keys (first, the two sides of the 64 + 16 key-slab boundary, last)
MARK_D = (1, 13, 27, 36)          # tail: head dim each marker lives on (36: the second k step of the head's 64-wide operand)
NEG_D = 38


def tail_marker(r, M):
    """marker index (0..3) of token r, or -1: tokens at the 16-token tile edges of a block, rotated so that every marker meets 16- and 32-token edges; the last two rows"""
    if r == M - 1:
        return 3
    pos = r % 128
    if pos % 16 in (0, 15):
        return (pos // 16 * 2 + (pos % 16 == 15) + pos // 32) % 4
    return 2 if r == M - 2 else -1


def _geglu_weights(rn, w):
    """ff1 / ff2 with every 16-unit group distinct at O(1): group means of the value and gate biases, and a coherent +-0.03 pattern per group in ff2's columns,
    whose token-independent part ff2.b cancels"""
    inner, ng = 4 * C, 4 * C // 16
    # value mean and gate mean of a group have opposite signs, so value * gelu(gate) and gate * gelu(value) differ by more than 1 in every group
    # (which sign: alternates between neighbouring groups and between a group and the one 64 units on, so a swap or a neighbouring chunk's bias always crosses it)
    gi = torch.arange(ng)
    neg = (gi + gi // 4) % 2 == 0
    vb = (0.8 + 1.2 * torch.rand(ng, generator=rn.g)) * torch.where(neg, -1.0, 1.0)
    gb = torch.where(neg, 1.0 + 1.5 * torch.rand(ng, generator=rn.g), -1.5 + 1.0 * torch.rand(ng, generator=rn.g))
    w["ff1.w"] = 0.5 * rn(2 * inner, C) / C ** 0.5
    w["ff1.b"] = torch.cat([vb.repeat_interleave(16), gb.repeat_interleave(16)]) + 0.1 * rn(2 * inner)
    sign = (torch.randint(0, 2, (C, ng), generator=rn.g) * 2 - 1).float()
    w["ff2.w"] = rn(C, inner) / inner ** 0.5 + 0.02 * sign.repeat_interleave(16, 1)
    z = torch.linspace(-6.0, 6.0, 241, dtype=torch.float64)          # E gelu(gb + 0.51 z), z ~ N(0, 1): the gate of a unit is its group mean + ff1.w n3 + the bias jitter
    pz = torch.exp(-0.5 * z * z)
    eg = (F.gelu(gb.double()[:, None] + 0.51 * z[None, :]) * pz).sum(1) / pz.sum()
    w["ff2.b"] = 0.1 * rn(C) - 0.02 * 16 * (sign @ (vb * eg.float()))


class _Rn:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def __call__(self, *shape):
        return torch.randn(*shape, generator=self.g)


def _frame_x(rn, Fr, HW, scale):
    """x whose frames differ in mean and spread (per-frame against pooled statistics, the neighbour's affine)"""
    s = torch.tensor([0.5, 1.5, 1.0, 2.5])[torch.arange(Fr) % 4]
    m = torch.tensor([-1.0, 2.0, 0.5, -2.0])[torch.arange(Fr) % 4]
    return ((rn(Fr, HW, C) * s[:, None, None] + m[:, None, None]) * scale).reshape(Fr * HW, C).contiguous()


def _gn(rn):
    return (1.0 + 0.2 * rn(C), 0.2 * rn(C), 32, 1e-6)


def edge_inputs(kind, case, td, seed=0):
    """weights and activations of one case of CASES[kind] (case: its index) -> dict.  o (tail) holds td values."""
    cs = CASES[kind][case]
    rn = _Rn(1000 * seed + 17 * case + {"front": 1, "tail": 2, "motion": 3}[kind])
    w = {}
    if kind == "front":
        from videovanish_amd.hip import attention_q_scale
        Fr, HW = cs["F"], cs["HW"]
        w["in.w"], w["in.b"] = rn(C, C) / C ** 0.5, 0.1 * rn(C) + 3.0 * HI          # LN1 sees halves of different mean
        w["ln1.g"], w["ln1.b"] = 1.0 + 0.1 * rn(C), 0.1 * rn(C)
        qkv = rn(3 * C, C) / C ** 0.5
        qkv[:C] *= attention_q_scale(D)
        w["qkv.w"] = qkv
        return dict(w=w, gn=_gn(rn), x=_frame_x(rn, Fr, HW, 1.0), F=Fr, HW=HW)
    if kind == "tail":
        M, big = cs["M"], cs.get("big", False)
        w["o1.w"], w["o1.b"] = rn(C, C) / C ** 0.5, 0.1 * rn(C) + 3.0 * HI          # LN2 and LN3 see halves of different mean
        g2, b2 = 1.0 + 0.1 * rn(C), 0.1 * rn(C)
        g2[list(SEL)], b2[list(SEL)] = 1.0, 0.0
        g2[BIAS_CH], b2[BIAS_CH] = 0.0, 1.0
        w["ln2.g"], w["ln2.b"] = g2, b2
        q2, k2 = 0.5 * rn(C, C) / C ** 0.5, 0.5 * rn(NKEY, C)
        for h in range(HEADS):
            if h == NEG_HEAD:          # q[NEG_D] = 4 for every token, k[NEG_D] = -16 for every key: all real scores shift by -64 (x 40^-1/2 = -10), the softmax does not move
                q2[h * D + NEG_D, BIAS_CH] += 4.0
                k2[:, h * D + NEG_D] = -16.0
                continue
            for j in range(4):         # a token whose trunk has 8 in channel SEL[j] (about 4 after LN2): q[MARK_D[j]] about 8, marker key 6 there: 48 x 40^-1/2 = 7.6 above the rest
                q2[h * D + MARK_D[j], SEL[j]] += 2.0
                k2[MARK[j], h * D + MARK_D[j]] += 6.0
        v2 = rn(NKEY, C)
        v2[:, NEG_HEAD * D:(NEG_HEAD + 1) * D] += 1.5          # the head's O is about 1.5 everywhere: a phantom key that takes the mass sends it to 0
        w["q2.w"], w["k2"], w["v2"] = q2, k2, v2
        o2 = rn(C, C) / C ** 0.5
        o2.view(C, HEADS, D)[:, :, 32:] *= 3.0          # d = 32..39 (the second k step of a head's O operand) carries weight
        w["o2.w"], w["o2.b"] = o2, 0.1 * rn(C)
        w["ln3.g"], w["ln3.b"] = 1.0 + 0.1 * rn(C), 0.1 * rn(C)
        _geglu_weights(rn, w)
        w["out.w"] = rn(C, C) / C ** 0.5
        w["out.b"] = 0.1 * rn(C) - w["out.w"] @ (3.0 * HI.float())          # the +3 of the hf = 1 channels does not reach the output
        t_in = 0.5 * rn(M, C)
        for r in range(M):
            j = tail_marker(r, M)
            if j >= 0:
                t_in[r, list(SEL)] = 0.0
                t_in[r, SEL[j]] = 8.0
        amp = 4.0 if big else 0.1
        return dict(w=w, o=(0.5 * rn(M, C)).to(td).float(), t_in=t_in, x=amp * rn(M, C), res1=amp * rn(M, C) if cs["res1"] else None, M=M, o_hw=cs["o_hw"],
                    out16=cs["out16"])
    Fr, HW, big = cs["F"], cs["HW"], cs.get("big", False)
    w["proj_in.w"], w["proj_in.b"] = rn(C, C) / C ** 0.5, 0.1 * rn(C)
    w["proj_out.w"], w["proj_out.b"] = rn(C, C) / C ** 0.5, 0.1 * rn(C)
    pe = 0.3 * rn(32, C)
    # attn i: LN output channels QCH[i] / KCH[i] / VCH[i] are pe alone (gamma = beta = 0); a designated query frame carries 3 in QCH, a marker key frame 3 in KCH, and head h
    # joins them on dim 36 (even heads: the second k step) or 5: q = 12, k = 3 (the large factor on the side both marker keys share, so its rounding moves them alike), 36 x 40^-1/2 = 5.7 above the rest.  Marker keys: an earlier frame and F - 1, which share the
    # mass and carry -2 / +2 in VCH, which the value projection spreads over d = 7 and 33: their values differ at O(1).
    QCH, KCH, VCH = (10, 200), (50, 300), (120, 260)
    keys = (sorted({(Fr - 1) // 2, Fr - 1}), sorted({0, Fr - 1}))
    queries = sorted({0, 15, 16, Fr // 3, Fr - 1} & set(range(Fr)))
    for i, a in enumerate(("attn1", "attn2")):
        g_, b_ = 1.0 + 0.1 * rn(C), 0.1 * rn(C)
        for ch in (QCH[i], KCH[i], VCH[i]):
            g_[ch], b_[ch] = 0.0, 0.0
        w[f"ln{i + 1}.g"], w[f"ln{i + 1}.b"] = g_, b_
        pe[:, QCH[i]], pe[:, KCH[i]], pe[:, VCH[i]] = 0.0, 0.0, 0.0
        pe[queries, QCH[i]] = 3.0
        pe[keys[i], KCH[i]] = 3.0
        pe[keys[i][0], VCH[i]] = -2.0
        pe[keys[i][-1], VCH[i]] = 2.0
        for nm in ("q", "k", "v", "o"):
            w[f"{a}.{nm}"] = rn(C, C) / C ** 0.5
        for h in range(HEADS):
            d = 36 if h % 2 == 0 else 5
            w[f"{a}.q"][h * D + d, QCH[i]] += 4.0
            w[f"{a}.k"][h * D + d, KCH[i]] += 1.0
            w[f"{a}.v"][[h * D + 7, h * D + 33], VCH[i]] += 1.5
        w[f"{a}.o"].view(C, HEADS, D)[:, :, 32:] *= 3.0
        w[f"{a}.ob"] = 0.1 * rn(C)
    w["ln3.g"], w["ln3.b"] = 1.0 + 0.1 * rn(C), 0.1 * rn(C)
    _geglu_weights(rn, w)
    w["pe"] = pe
    amp = 3.0 if big else 0.1
    return dict(w=w, gn=_gn(rn), x=_frame_x(rn, Fr, HW, amp), res1=amp * rn(Fr * HW, C) if cs["res1"] else None, F=Fr, HW=HW, out16=cs["out16"])


def run(kind, inp, td, rounded=True, mut=None):
    """the reference of one edge_inputs dict -> tuple of float64 outputs (front: (t, qkv); tail, motion: (out,))"""
    if kind == "front":
        return front(inp["w"], inp["gn"], inp["x"], inp["F"], inp["HW"], td, rounded, mut)
    if kind == "tail":
        return (tail(inp["w"], inp["o"], inp["t_in"], inp["x"], inp["res1"], td, rounded, mut, out_h16=inp["out16"], o_hw=inp["o_hw"]),)
    return (motion(inp["w"], inp["gn"], inp["x"], inp["res1"], inp["F"], inp["HW"], td, rounded, mut, out_h16=inp["out16"]),)


@functools.lru_cache(maxsize=None)
def inputs(kind, case, dname):
    return edge_inputs(kind, case, TD[dname])


@functools.lru_cache(maxsize=None)
def reference(kind, case, dname, rounded=True):
    """computed once per process and shared; callers must not modify it"""
    with torch.no_grad():
        return run(kind, inputs(kind, case, dname), TD[dname], rounded)


def bound(kind, dname, ref):
    """B = ceil(4 N) u max(1, max |ref|)"""
    return MARGIN[(kind, dname)] * U[TD[dname]] * max(1.0, ref.abs().max().item())


def noise(kind, case, dname):
    """N of one case: the largest over the kernel's outputs"""
    return max(((a - b).abs().max().item() / (U[TD[dname]] * max(1.0, a.abs().max().item())))
               for a, b in zip(reference(kind, case, dname, True), reference(kind, case, dname, False)))


def margin_of(n):
    return int(math.ceil(4.0 * n))


# ---------------------------------------------------------------------------------------------------------------------------
# GroupNorm statistics at the geometries the fused kernels consume (vv_groupnorm_stats -> vv_gn_affine(_frames))
def gn_geom(HW, Cc):
    """csrc/vv_norm.hip gn_geom restated -> dict(C8, krows, threads, rows_per_split, nsplit)"""
    C8 = Cc // 8
    krows = 1 if C8 >= 256 else 256 // C8
    rows = max(32768 // Cc, krows)
    rows = (rows + krows - 1) // krows * krows
    ns = (HW + rows - 1) // rows
    if ns > 128:
        ns = 128
        rows = ((HW + ns - 1) // ns + krows - 1) // krows * krows
        ns = (HW + rows - 1) // rows
    return dict(C8=C8, krows=krows, threads=krows * C8, rows_per_split=rows, nsplit=ns)


GN_CASES = [      # C, HW, F, pooled; what the geometry has to show
    dict(C=320, HW=13057, F=1, pool=False, geom=dict(krows=6, threads=240, rows_per_split=108, nsplit=121)),      # the ns > 128 cap: 102-row splits would be 129; last split 97 rows
    dict(C=2560, HW=1537, F=1, pool=False, geom=dict(krows=1, threads=320, rows_per_split=13, nsplit=119)),       # cap taken at krows = 1, 320 threads
    dict(C=960, HW=70, F=2, pool=False, geom=dict(krows=2, threads=240, nsplit=3)),                               # C / 8 = 120: idle lanes, krows = 2
    dict(C=1920, HW=70, F=1, pool=False, geom=dict(krows=1, threads=240, nsplit=5)),                              # C / 8 = 240: idle lanes, krows = 1
    dict(C=320, HW=820, F=32, pool=True, geom=dict(nsplit=9)),          # 9 x 32 = 288 partials: the strided loop of gn_finalize_pooled_kernel runs twice for 32 threads
    dict(C=320, HW=820, F=32, pool=False, geom=dict(nsplit=9)),         # gn_finalize_kernel: 8 lanes per group over 9 partials
]
