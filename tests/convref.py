"""fp64 host reference of the vv_conv_params contract (include/vvhip.h, vv_conv_gemm): the output rows of ONE launch, evaluated from that launch's
own operands.  Plain torch in float64 on whatever device the operands live on; shared by the kernel tests, not a conftest.

    ref = conv_rows(dtype, rows, x0, weight, N, K, **kw)      # the conv_gemm keyword arguments of the launch
    pos = out_positions(rows, N, K, **kw)                     # where those values sit in `out` (flat element index)
    got = out.reshape(-1)[pos]

The contract, restated:
  * A[m][k], k = (ky * KW + kx) * Cin + c over the channel concat of x0 (C0) and x1 (C1), KW = ksize_w or ksize;  row m = (f, y, x) of the
    Hout x Wout grid;  tap (yv, xv) = (y * stride - pad_t + ky, x * stride - pad_l + kx) is inside the VIRTUAL Hv x Wv image or zero, and reads
    source pixel ((yv * Hin) // Hv, (xv * Win) // Wv) (the fused nearest resize);  fp32 sources are rounded to the operand dtype (as staged).
  * weight: the packed h16 [Npad][Kpad] as stored; column k < K of row n.
  * value = (A W^T + bias) * out_scale + rowvec[f] + res0 + res1, then RELU / LRELU; residuals are [rows][N] (leading dimension N, not ldo) and
    are read at the row the value is stored at (the scatter row below).
  * GEGLU: weight rows interleaved in blocks of 16 ([v0..15 g0..15 v16..]): out column j = (v + bv) * gelu_erf(g + bg), N / 2 columns.
  * store: row r * ldo + out_col + n, r = m or, with the scatter, (f * sc_oh + y * sc_sy + sc_oy) * sc_ow + x * sc_sx + sc_ox;
    split_heads: out[(((b * 3 + which) * heads + head) * tokens + token) * dim + d] + out_col with n = (which * heads + head) * dim + d and
    (b, token) = divmod(m, tokens), or for split_tokens < 0 (token-major rows) (token, b) = divmod(m, M / tokens).
"""
import math

import torch

EPI_NONE, EPI_GEGLU = 0, 1
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 2, 3


def _geom(F, Hin, Win, Hv, Wv, Hout, Wout):
    Hv = Hin if Hv is None else Hv
    Wv = Win if Wv is None else Wv
    Hout = Hv if Hout is None else Hout
    Wout = Wv if Wout is None else Wout
    return Hv, Wv, Hout, Wout


def im2col_rows(h16, rows, x0, x1=None, *, F=1, Hin=1, Win=1, Hv=None, Wv=None, Hout=None, Wout=None, ksize=1, ksize_w=0, stride=1, pad_t=0,
                pad_l=0, C0=None):
    """float64 A[rows][K] (K = ksize * KW * Cin, k = (ky * KW + kx) * Cin + c) of the launch rows `rows` (int64 tensor)."""
    Hv, Wv, Hout, Wout = _geom(F, Hin, Win, Hv, Wv, Hout, Wout)
    KW = ksize_w if ksize_w else ksize
    C0 = x0.shape[-1] if C0 is None else C0
    srcs = [x0.reshape(-1, C0)] + ([x1.reshape(-1, x1.shape[-1])] if x1 is not None else [])
    rows = rows.to(srcs[0].device)
    HWo = Hout * Wout
    f, rem = rows // HWo, rows % HWo
    y, x = rem // Wout, rem % Wout
    cols = []
    for ky in range(ksize):
        for kx in range(KW):
            yv, xv = y * stride - pad_t + ky, x * stride - pad_l + kx
            ok = (yv >= 0) & (yv < Hv) & (xv >= 0) & (xv < Wv)
            ys, xs = (yv.clamp(0, Hv - 1) * Hin) // Hv, (xv.clamp(0, Wv - 1) * Win) // Wv
            pix = (f * Hin + ys) * Win + xs
            for s in srcs:      # gathered in the stored dtype; an fp32 source rounded to the operand dtype (the kernel's staging); taps outside: zero
                v = s[pix]
                v = (v.to(h16) if v.dtype == torch.float32 else v).double()
                cols.append(torch.where(ok[:, None], v, torch.zeros((), dtype=v.dtype, device=v.device)))
    return torch.cat(cols, 1)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def scatter_rows(rows, F=1, Hout=1, Wout=1, scatter=None):
    """the row of `out` (and of the residuals) that launch row m is stored at"""
    if scatter is None:
        return rows
    OH, OW, sy, sx, oy, ox = scatter
    HWo = Hout * Wout
    f, rem = rows // HWo, rows % HWo
    y, x = rem // Wout, rem % Wout
    return (f * OH + y * sy + oy) * OW + x * sx + ox


def conv_rows(h16, rows, x0, weight, N, K, *, x1=None, F=1, Hin=1, Win=1, Hv=None, Wv=None, Hout=None, Wout=None, ksize=1, stride=1, pad_t=0,
              pad_l=0, bias=None, rowvec=None, res0=None, res1=None, epilogue=EPI_NONE, out_scale=1.0, C0=None, C1=0, ksize_w=0, act=ACT_NONE,
              act_slope=0.0, scatter=None, chunk=2048, **_store):
    """float64 [len(rows)][Nout] of launch rows `rows` (int64): the value vv_conv_gemm stores for them, before the cast to out_dtype.  The store-only
    arguments of conv_gemm (out, out_dtype, ldo / out_col, split_*, tile_hint, gn_partials) are accepted and ignored; see out_positions."""
    Hv, Wv, Hout, Wout = _geom(F, Hin, Win, Hv, Wv, Hout, Wout)
    dev = weight.device
    rows = torch.as_tensor(rows, dtype=torch.int64).to(dev)
    W = weight[:N, :K].double()
    parts = []
    for i in range(0, rows.numel(), chunk):      # bounded im2col working set
        r = rows[i:i + chunk]
        A = im2col_rows(h16, r, x0, x1, F=F, Hin=Hin, Win=Win, Hv=Hv, Wv=Wv, Hout=Hout, Wout=Wout, ksize=ksize, ksize_w=ksize_w, stride=stride,
                        pad_t=pad_t, pad_l=pad_l, C0=C0)
        assert A.shape[1] == K, f"K = {K} but ksize * KW * Cin = {A.shape[1]}"
        parts.append(A.to(dev) @ W.t())
    acc = torch.cat(parts, 0) if parts else torch.zeros(0, N, dtype=torch.float64, device=dev)
    if bias is not None:
        acc = acc + bias.double().to(dev)[:N]
    if epilogue == EPI_GEGLU:
        j = torch.arange(N // 2, device=dev)
        vrow = (j // 16) * 32 + j % 16
        return acc[:, vrow] * gelu_erf(acc[:, vrow + 16])
    v = acc * out_scale
    if rowvec is not None:
        v = v + rowvec.double().to(dev).reshape(-1, N)[rows // (Hout * Wout)]
    srow = scatter_rows(rows, F, Hout, Wout, scatter)
    for r in (res0, res1):
        if r is not None:
            v = v + r.double().to(dev).reshape(-1, N)[srow]
    if act == ACT_RELU:
        v = v.clamp(min=0.0)
    elif act == ACT_LRELU:
        v = torch.where(v > 0, v, v * act_slope)
    return v


def out_positions(rows, N, K=None, *, F=1, Hin=1, Win=1, Hv=None, Wv=None, Hout=None, Wout=None, epilogue=EPI_NONE, out=None, ldo=None, out_col=0,
                  split_heads=0, split_dim=0, split_tokens=0, scatter=None, **_):
    """int64 [len(rows)][Nout]: flat element index into `out` (as conv_gemm got it) of every value conv_rows returns.  ldo = out.shape[-1] unless given."""
    Hv, Wv, Hout, Wout = _geom(F, Hin, Win, Hv, Wv, Hout, Wout)
    rows = torch.as_tensor(rows, dtype=torch.int64)
    nout = N // 2 if epilogue == EPI_GEGLU else N
    n = torch.arange(nout, dtype=torch.int64)
    if split_heads > 0:
        M = F * Hout * Wout
        stok = abs(split_tokens)
        if split_tokens > 0:
            b, tok = rows // stok, rows % stok
        else:
            snb = M // stok
            tok, b = rows // snb, rows % snb
        wh, d = n // split_dim, n % split_dim
        return (((b[:, None] * 3 * split_heads + wh[None]) * stok + tok[:, None]) * split_dim + d[None]) + out_col
    ldo = out.shape[-1] if ldo is None else ldo
    srow = scatter_rows(rows, F, Hout, Wout, scatter)
    return srow[:, None] * ldo + out_col + n[None]


def bound(ref, out_dtype, h16):
    """the kernel-test bound of the project (tests/test_kernels_gpu.py): fp32 output 3e-4 * max(1, max|ref|); h16 output 2 ulp * max|ref|"""
    m = ref.abs().max().item() if ref.numel() else 0.0
    if out_dtype == torch.float32:
        return 3e-4 * max(1.0, m)
    return 2 * (2.0 ** -8 if h16 == torch.bfloat16 else 2.0 ** -11) * m
