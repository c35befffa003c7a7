"""fp64 host reference of the vv_attn_params contract (include/vvhip.h, vv_attention / vv_attention_merge), and adversarial inputs that turn an
off-by-one at a key-tile or query-tile edge into an O(1) error.  Plain torch in float64 on the CPU; shared by the kernel tests, not a conftest.

The contract, restated:
  * element (b, h, i, c) of q lives at q[q_off + b * q_bs + h * q_hs + i * q_rs + c] of the flat buffer, q_hs = D when 0; the same for k, v and o.
  * s[i][j] = cq * sum_c q[i][c] k[j][c] in the log2 domain: cq = scale * log2(e), or 1 with q_prescaled (q then already carries the factor).
  * o[i] = sum_j 2^(s[i][j] - m_i) v[j] / l_i,  m_i = max_j s[i][j],  l_i = sum_j 2^(s[i][j] - m_i);  lse[b][h][i] = m_i + log2(l_i).
  * `requant` (an h16 torch dtype): the 32x32x16 routes without q_prescaled form their operand as h16(fp32(q) * fp32(scale * 1.4426950408889634f)) and
    use it with cq = 1 (a32_scale_q in vv_attn32.hip); the reference then does the same before it goes on in fp64.
  * `p_round` (an h16 torch dtype): the h16 MODEL of a kernel -- P = 2^(s - m) rounded to h16, numerator and denominator summed in fp32 -- used to
    show that a bound leaves the kernels room (tests/test_attnref_cpu.py), never as the reference.
  * merge: out[q][h * D + c] = sum_s w_s parts[s][q][h * D + c] / sum_s w_s, w_s = 2^(lse[s][h][q] - max_s lse[s][h][q]).
"""
import dataclasses
import math

import numpy as np
import torch

LOG2E = 1.4426950408889634
SENTINEL = 0x5A5A          # bit pattern the output allocation is prefilled with (finite in both h16 formats)
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # unit roundoff, as the DT table of tests/test_kernels_gpu.py


def index(off, bs, hs, rs, B, heads, rows, D):
    """flat element index [B][heads][len(rows)][D] of a tensor laid out by (off, bs, hs (0 = D), rs); rows: int64 tensor of row numbers (may be negative: guards)"""
    b = torch.arange(B, dtype=torch.int64).view(B, 1, 1, 1)
    h = torch.arange(heads, dtype=torch.int64).view(1, heads, 1, 1)
    c = torch.arange(D, dtype=torch.int64).view(1, 1, 1, D)
    return off + b * bs + h * (hs if hs else D) + rows.view(1, 1, -1, 1) * rs + c


def _rows(n):
    return torch.arange(n, dtype=torch.int64)


def attention_core(q, k, v, *, B, heads, Nq, Nkv, D, q_bs, k_bs, v_bs, q_rs, k_rs, v_rs, q_off=0, k_off=0, v_off=0, q_hs=0, k_hs=0, v_hs=0, scale=None,
                   q_prescaled=False, requant=None, p_round=None, **_):
    """(o [B][heads][Nq][D], lse [B][heads][Nq]) in float64 from the flat buffers q / k / v (any float dtype)."""
    scale = float(D) ** -0.5 if scale is None else float(scale)
    qd = q.reshape(-1)[index(q_off, q_bs, q_hs, q_rs, B, heads, _rows(Nq), D)]
    kd = k.reshape(-1)[index(k_off, k_bs, k_hs, k_rs, B, heads, _rows(Nkv), D)].double()
    vd = v.reshape(-1)[index(v_off, v_bs, v_hs, v_rs, B, heads, _rows(Nkv), D)].double()
    if q_prescaled:
        qd, cq = qd.double(), 1.0
    elif requant is not None:
        f = np.float32(scale) * np.float32(LOG2E)                   # the kernel's fp32 factor
        qd, cq = (qd.float() * float(f)).to(requant).double(), 1.0
    else:
        qd, cq = qd.double(), float(np.float32(scale) * np.float32(LOG2E))
    s = (qd @ kd.transpose(-1, -2)) * cq
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - m)
    if p_round is not None:
        ph = p.to(p_round).float()
        o = (ph @ vd.float()).double() / ph.sum(-1, keepdim=True).double()
        l = ph.sum(-1, keepdim=True).double()
    else:
        l = p.sum(-1, keepdim=True)
        o = (p @ vd) / l
    return o, (m + torch.log2(l)).squeeze(-1)


def place(o, numel, *, B, heads, Nq, D, o_bs, o_rs, o_hs=0, o_off=0, row_shift=None, **_):
    """the [B][heads][Nq][D] output placed in a flat float64 buffer of `numel` elements through o_off / o_bs / o_hs / o_rs (NaN where nothing is written);
    row_shift: {row: new row}, for tests that misplace a row on purpose"""
    rows = _rows(Nq)
    for a, b in (row_shift or {}).items():
        rows[a] = b
    buf = torch.full((numel,), float("nan"), dtype=torch.float64)
    buf[index(o_off, o_bs, o_hs, o_rs, B, heads, rows, D)] = o
    return buf


def attention(q, k, v, numel, **kw):
    """(output placed through o_off / o_bs / o_hs / o_rs in a flat float64 buffer of numel elements, NaN elsewhere; lse [B][heads][Nq])"""
    o, lse = attention_core(q, k, v, **kw)
    return place(o, numel, **kw), lse


def merge(parts, lse, *, S, heads, Nq, D, ld):
    """vv_attention_merge in float64: parts [S][Nq][ld], lse [S][heads][Nq] -> [Nq][heads * D]"""
    w = torch.exp2(lse.double() - lse.double().amax(0, keepdim=True))                    # [S][heads][Nq]
    x = parts.double().reshape(S, Nq, ld)[:, :, :heads * D].reshape(S, Nq, heads, D)
    wq = w.permute(0, 2, 1).unsqueeze(-1)                                                 # [S][Nq][heads][1]
    return ((wq * x).sum(0) / wq.sum(0)).reshape(Nq, heads * D)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# adversarial inputs

LAYOUTS = ("fused", "hm", "hm_o", "shared", "temporal")
#   fused    : rows of one [B][N][3C + 8] QKV matrix with column offsets (Nq == Nkv; otherwise q rows of their own and a fused [Nkv][2C] K|V matrix); row-major o
#   hm       : head-major q / k / v ([B][heads][N][D], hs = N * D, rs = D), row-major o
#   hm_o     : head-major q / k / v and head-major o through o_hs (one spare head slot per batch)
#   shared   : one K|V matrix for every batch (k_bs = v_bs = 0), row-major q and o
#   temporal : b = pixel, i = frame of a [frames][pixels][3C] matrix (q_bs = 3C, q_rs = pixels * 3C); Nq == Nkv
# every tensor has G guard rows before and after each batch's rows; row-major o has 8 spare columns (o_rs = C + 8).


@dataclasses.dataclass
class Case:
    """inputs of one launch, and what the generator knows about its markers"""
    bufs: dict           # {buffer name: flat h16 tensor} of q / k / v (a fused buffer holds several)
    names: dict          # {"q" | "k" | "v" | "o": buffer name}
    kw: dict             # the hip.attention keywords (o_off apart: the launch passes out[o_off:])
    out_numel: int       # elements of the output allocation, guards and spare columns included
    dtype: torch.dtype
    KVT: int
    G: int               # guard rows before and after every batch's rows
    markers: list        # marker keys
    designated: list     # designated queries; query designated[t] belongs to marker t mod len(markers)
    gamma: float
    fill: str
    layout: str


def marker_keys(Nkv, KVT):
    m = {0, Nkv - 1}
    for j in range(KVT, Nkv, KVT):
        m.update((j - 1, j))
    return sorted(m)


def designated_queries(Nq, want):
    d = {0, Nq - 1}
    for b in range(16, Nq, 16):
        d.update((b - 1, b))
    i = 1
    while len(d) < min(want, Nq):      # more markers than query-tile edges: further queries, so that every marker has its query while queries last
        d.add(i)
        i += 1
    return sorted(d)


def _spec(layout, B, heads, Nq, Nkv, D, G):
    """{tensor: (buffer name, off, bs, hs, rs)}, {buffer name: numel} of a layout"""
    C = heads * D
    Rq, Rk = Nq + 2 * G, Nkv + 2 * G
    sizes, sp = {}, {}
    if layout in ("hm", "hm_o"):
        for t, R, N in (("q", Rq, Nq), ("k", Rk, Nkv), ("v", Rk, Nkv)):
            sizes[t] = B * heads * R * D
            sp[t] = (t, G * D, heads * R * D, R * D, D)
    elif layout == "temporal":
        assert Nq == Nkv
        W = 3 * C
        sizes["qkv"] = Rq * B * W
        for i, t in enumerate("qkv"):
            sp[t] = ("qkv", G * B * W + i * C, W, 0, B * W)
    elif layout == "fused" and Nq == Nkv:
        W = 3 * C + 8
        sizes["qkv"] = B * Rq * W
        for i, t in enumerate("qkv"):
            sp[t] = ("qkv", G * W + i * C, Rq * W, 0, W)
    else:      # fused with Nq != Nkv, shared
        W, Wk = C + 8, 2 * C
        Bk = 1 if layout == "shared" else B
        sizes["q"], sizes["kv"] = B * Rq * W, Bk * Rk * Wk
        sp["q"] = ("q", G * W, Rq * W, 0, W)
        for i, t in enumerate("kv"):
            sp[t] = ("kv", G * Wk + i * C, 0 if layout == "shared" else Rk * Wk, 0, Wk)
    if layout == "hm_o":
        sizes["o"] = B * (heads + 1) * Rq * D
        sp["o"] = ("o", G * D, (heads + 1) * Rq * D, Rq * D, D)
    elif layout == "temporal":
        sizes["o"] = Rq * B * C
        sp["o"] = ("o", G * B * C, C, 0, B * C)
    else:
        Wo = C + 8
        sizes["o"] = B * Rq * Wo
        sp["o"] = ("o", G * Wo, Rq * Wo, 0, Wo)
    return sp, sizes


def edge_case(B, heads, Nq, Nkv, D, KVT, dtype, seed, *, layout="hm", fill="nan", scale=None, q_prescaled=False, lead=16.0, markers=None):
    """Inputs that make an error at a tile edge an O(1) error of the output while max|ref| stays <= 1.

    Marker keys: 0, Nkv - 1 and both sides of every key-tile boundary (KVT j - 1, KVT j), or the list `markers` (a key sequence that is launched in
    chunks has its tile edges elsewhere).  Designated queries: 0, Nq - 1, both sides of every multiple of
    16 (which covers the 32- and 64-query boundaries), and further queries while there are more markers than those.  Designated query t belongs to marker
    t mod (number of markers).  For each (b, head) marker m has a random sign vector u_m in {-1, +1}^D: its designated queries are q = u_m, its key is
    k = gamma u_m, and its value a sign vector of its own; gamma is the smallest power of two for which, over all (b, head), the marker of every
    designated query leads every other score of that query by `lead` binary orders (measured on the stored, rounded operands; the issue asks for 12, the
    rest is room for the re-rounded operand of the 32x32x16 routes).  All other queries are N(0, 1), all other keys N(0, 1/4), all other values uniform in
    [-1, 1], so |o| <= 1.
    Guards: G = max(KVT, 64) rows before and after every batch's rows of q, k, v and o.  fill = "nan": q / k / v guards and every spare element are NaN.
    fill = "ghost": k guard row Nkv holds 2 gamma u of the LAST marker with v = -(its value), row -1 the same for marker 0, the other guard rows cycle
    over the markers; q guards are N(0, 1) and spare elements 0.  The output allocation is prefilled with SENTINEL."""
    assert layout in LAYOUTS and fill in ("nan", "ghost")
    g = torch.Generator().manual_seed(seed)
    G = max(KVT, 64)
    shared = layout == "shared"
    Bk = 1 if shared else B
    scale = float(D) ** -0.5 if scale is None else float(scale)
    c = float(np.float32(scale) * np.float32(LOG2E))
    M = marker_keys(Nkv, KVT) if markers is None else sorted(markers)
    nM = len(M)
    Dq = designated_queries(Nq, nM)
    own = [t % nM for t in range(len(Dq))]
    Mi, Di, Oi = torch.tensor(M), torch.tensor(Dq), torch.tensor(own)

    def signs(*shape):
        return torch.randint(0, 2, shape, generator=g).double() * 2 - 1

    u = signs(Bk, heads, nM, D)
    w = signs(Bk, heads, nM, D)
    q = torch.randn(B, heads, Nq, D, generator=g, dtype=torch.float64)
    q[:, :, Di] = u[:, :, Oi].expand(B, heads, len(Dq), D)
    if q_prescaled:
        q = q * c
    q = q.to(dtype)
    kbase = (torch.randn(Bk, heads, Nkv, D, generator=g, dtype=torch.float64) * 0.5)
    v = torch.rand(Bk, heads, Nkv, D, generator=g, dtype=torch.float64) * 2 - 1
    v[:, :, Mi] = w
    v = v.to(dtype)
    gamma = 2.0 ** -3
    while True:
        k = kbase.clone()
        k[:, :, Mi] = gamma * u
        k = k.to(dtype)
        s = (q[:, :, Di].double() @ k.double().transpose(-1, -2)) * (1.0 if q_prescaled else c)       # [B][heads][designated][Nkv]
        mine = s.gather(-1, Mi[Oi].view(1, 1, -1, 1).expand(B, heads, len(Dq), 1))
        rest = s.scatter(-1, Mi[Oi].view(1, 1, -1, 1).expand(B, heads, len(Dq), 1), -1e30).amax(-1, keepdim=True)
        if Nkv == 1 or float((mine - rest).min()) >= lead:
            break
        gamma *= 2
        assert gamma <= 2.0 ** 8, "edge_case: no gamma gives the markers their lead"

    sp, sizes = _spec(layout, B, heads, Nq, Nkv, D, G)
    nan = fill == "nan"
    bufs = {n: torch.full((sz,), float("nan") if nan else 0.0, dtype=dtype) for n, sz in sizes.items() if n != "o"}
    gq = torch.cat([_rows(G) - G, _rows(G) + Nq])
    gk = torch.cat([_rows(G) - G, _rows(G) + Nkv])
    if not nan:      # ("nan": the buffers are NaN already, guards and spare elements included)
        gm = gk % nM
        gm[gk == Nkv] = nM - 1
        gm[gk == -1] = 0
        bufs[sp["q"][0]][index(*sp["q"][1:], B, heads, gq, D)] = torch.randn(B, heads, 2 * G, D, generator=g).to(dtype)
        bufs[sp["k"][0]][index(*sp["k"][1:], Bk, heads, gk, D)] = (2 * gamma * u[:, :, gm]).to(dtype)
        bufs[sp["v"][0]][index(*sp["v"][1:], Bk, heads, gk, D)] = (-w[:, :, gm]).to(dtype)
    bufs[sp["q"][0]][index(*sp["q"][1:], B, heads, _rows(Nq), D)] = q
    bufs[sp["k"][0]][index(*sp["k"][1:], Bk, heads, _rows(Nkv), D)] = k
    bufs[sp["v"][0]][index(*sp["v"][1:], Bk, heads, _rows(Nkv), D)] = v

    kw = dict(B=B, heads=heads, Nq=Nq, Nkv=Nkv, D=D, scale=scale, q_prescaled=q_prescaled)
    for t in "qkvo":
        _, off, bs, hs, rs = sp[t]
        kw.update({f"{t}_off": off, f"{t}_bs": bs, f"{t}_hs": hs, f"{t}_rs": rs})
    return Case(bufs=bufs, names={t: sp[t][0] for t in "qkvo"}, kw=kw, out_numel=sizes["o"], dtype=dtype, KVT=KVT, G=G, markers=M, designated=Dq, gamma=gamma,
                fill=fill, layout=layout)


def reference(cs, **over):
    """(o [B][heads][Nq][D], lse) of a case from its own buffers; over: keywords to replace (Nkv, requant, p_round, v=...)"""
    kw = dict(cs.kw)
    bufs = {t: over.pop(t, cs.bufs[cs.names[t]]) for t in "qkv"}
    kw.update(over)
    return attention_core(bufs["q"], bufs["k"], bufs["v"], **kw)


def sentinel_buffer(cs):
    return torch.full((cs.out_numel,), SENTINEL, dtype=torch.int16).view(cs.dtype)


def launch_kw(cs):
    """the keywords of hip.attention for a case (the output is passed as out[o_off:])"""
    return {k: v for k, v in cs.kw.items() if k != "o_off"}


def check_output(cs, got, ref):
    """(max |got - ref| over the elements the contract writes -- inf when one of them is not finite --, number of OTHER elements of the output allocation that
    no longer hold SENTINEL); got: the flat h16 output allocation (CPU), ref: [B][heads][Nq][D] float64"""
    kw = cs.kw
    idx = index(kw["o_off"], kw["o_bs"], kw["o_hs"], kw["o_rs"], kw["B"], kw["heads"], _rows(kw["Nq"]), kw["D"])
    val = got.reshape(-1)[idx].double()
    err = float((val - ref).abs().max()) if bool(torch.isfinite(val).all()) else math.inf
    outside = torch.ones(cs.out_numel, dtype=torch.bool)
    outside[idx.reshape(-1)] = False
    bits = got.reshape(-1).view(torch.int16)
    return err, int((bits[outside] != SENTINEL).sum())


def written(cs, o, row_shift=None):
    """what a kernel that computed `o` leaves in the output allocation: SENTINEL everywhere, o rounded to h16 at its place"""
    buf = sentinel_buffer(cs)
    p = place(o, cs.out_numel, row_shift=row_shift, **cs.kw)
    at = ~torch.isnan(place(torch.zeros_like(o), cs.out_numel, row_shift=row_shift, **cs.kw))
    buf[at] = p[at].to(cs.dtype)
    return buf
