"""GPU parity tests of the individual HIP kernels (through the C ABI) against plain fp32 torch on the CPU.

Operands are pre-rounded to the MFMA operand type (bf16 / fp16) on both sides, so the comparison isolates the
kernel's indexing and accumulation: tolerance = fp32 accumulation-order noise (+ one h16 rounding when the kernel
stores h16)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = [("bf16", torch.bfloat16, 2 ** -8), ("fp16", torch.float16, 2 ** -11)]


def _r(t, td):
    return t.to(td).float()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("dname,td,ulp", DT)
@pytest.mark.parametrize("case", [
    dict(F=2, H=9, W=11, cin=64, cout=160, k=3, stride=1),
    dict(F=3, H=12, W=10, cin=128, cout=128, k=3, stride=2),
    dict(F=2, H=7, W=5, cin=320, cout=320, k=1, stride=1),
    dict(F=1, H=6, W=6, cin=64, cout=4, k=3, stride=1),           # tiny-N tile (conv_out)
    dict(F=2, H=5, W=6, cin=8, cout=64, k=3, stride=1),           # padded conv_in style (K=72 -> 128)
    dict(F=1, H=17, W=19, cin=64, cout=320, k=3, stride=1, f32in=True),
    dict(F=2, H=33, W=29, cin=192, cout=96, k=3, stride=1),       # N padded to 128, several M tiles
    dict(F=2, H=13, W=21, cin=128, cout=160, k=1, stride=1, f32in=True),   # fp32 A tile by LDS-DMA (FAST32), several M tiles
    dict(F=2, H=12, W=10, cin=192, cout=128, k=3, stride=2, f32in=True),
    dict(F=1, H=9, W=9, cin=64, cout=4, k=3, stride=1, f32in=True),
    dict(F=1, H=9, W=9, cin=72, cout=64, k=3, stride=1, f32in=True),       # C % 64 != 0 -> register-staged fp32 loader
    dict(F=2, H=16, W=32, cin=64, cout=160, k=3, stride=1),                # 3x3 halo-tile path: exact 8x16 patches
    dict(F=3, H=23, W=47, cin=128, cout=128, k=3, stride=1),               # halo path, ragged patches on both edges
    dict(F=1, H=40, W=31, cin=192, cout=320, k=3, stride=1),               # halo path, 3 channel chunks, 2 N tiles
    dict(F=2, H=31, W=48, cin=128, cout=160, k=3, stride=1),                # halo path, 16-row-aligned shapes: ragged bottom edge
    dict(F=1, H=32, W=47, cin=320, cout=320, k=3, stride=1),                # 5 chunks (odd), 2 N tiles, ragged right edge
    dict(F=1, H=48, W=32, cin=64, cout=128, k=3, stride=1),                 # one chunk, 128-wide N tile
])
def test_conv_gemm(gpu, dname, td, ulp, case):
    from videovanish_amd import hip, packing
    dt = hip.dtype_id(dname)
    g = torch.Generator().manual_seed(1)
    Fr, H, W, cin, cout, k, stride = (case[x] for x in ("F", "H", "W", "cin", "cout", "k", "stride"))
    x = torch.randn(Fr, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g)
    f32in = case.get("f32in", False)
    ref = F.conv2d(_r(x, td), _r(w, td), b, stride=stride, padding=k // 2)
    Ho, Wo = ref.shape[-2:]
    wp, K = packing.pack_conv(w, td)
    xin = _nhwc(x).to(gpu) if f32in else _nhwc(x).to(td).to(gpu)
    out = hip.conv_gemm(dt, xin, wp.to(gpu), cout, K, F=Fr, Hin=H, Win=W, Hout=Ho, Wout=Wo, ksize=k, stride=stride, pad_t=k // 2,
                        pad_l=k // 2, bias=b.to(gpu), out_dtype=torch.float32)
    got = out.cpu().reshape(Fr, Ho, Wo, cout).permute(0, 3, 1, 2)
    tol = 2e-4
    assert (got - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("dname,td,ulp", DT)
def test_conv_gemm_epilogues(gpu, dname, td, ulp):
    """concat input + fused nearest upsample + temb rowvec + two residuals + h16 output; asymmetric pad; GEGLU."""
    from videovanish_amd import hip, packing
    dt = hip.dtype_id(dname)
    g = torch.Generator().manual_seed(2)
    Fr, h, w, H, W, c0, c1, cout = 2, 6, 5, 11, 9, 64, 128, 160
    a = torch.randn(Fr, c0, h, w, generator=g)
    s = torch.randn(Fr, c1, h, w, generator=g)
    wt = torch.randn(cout, c0 + c1, 3, 3, generator=g) / math.sqrt((c0 + c1) * 9)
    bias = torch.randn(cout, generator=g)
    temb = torch.randn(Fr, cout, generator=g)
    r0 = torch.randn(Fr, cout, H, W, generator=g)
    r1 = torch.randn(Fr, cout, H, W, generator=g)
    xin = torch.cat([_r(a, td), _r(s, td)], 1)
    up = F.interpolate(xin, size=(H, W), mode="nearest")
    ref = F.conv2d(up, _r(wt, td), bias, padding=1) + temb[:, :, None, None] + r0 + r1
    wp, K = packing.pack_conv(wt, td)
    kw = dict(x1=_nhwc(s).to(td).to(gpu), F=Fr, Hin=h, Win=w, Hv=H, Wv=W, ksize=3, pad_t=1, pad_l=1, bias=bias.to(gpu))
    out = hip.conv_gemm(dt, _nhwc(a).to(td).to(gpu), wp.to(gpu), cout, K, rowvec=temb.to(gpu), res0=_nhwc(r0).to(gpu),
                        res1=_nhwc(r1).to(gpu), out_dtype=torch.float32, **kw)
    got = out.cpu().reshape(Fr, H, W, cout).permute(0, 3, 1, 2)
    assert (got - ref).abs().max().item() <= 3e-4 * ref.abs().max().item()
    # h16 output path
    out16 = hip.conv_gemm(dt, _nhwc(a).to(td).to(gpu), wp.to(gpu), cout, K, **kw)
    ref16 = F.conv2d(up, _r(wt, td), bias, padding=1)
    got16 = out16.float().cpu().reshape(Fr, H, W, cout).permute(0, 3, 1, 2)
    assert (got16 - ref16).abs().max().item() <= 2 * ulp * ref16.abs().max().item()
    # fp32 concat input + fused nearest upsample (VAE decoder / up-block shortcut style): same result as pre-rounded operands
    out32 = hip.conv_gemm(dt, _nhwc(_r(a, td)).to(gpu), wp.to(gpu), cout, K, **{**kw, "x1": _nhwc(_r(s, td)).to(gpu)}, out_dtype=torch.float32)
    got32 = out32.cpu().reshape(Fr, H, W, cout).permute(0, 3, 1, 2)
    assert (got32 - ref16).abs().max().item() <= 3e-4 * ref16.abs().max().item()
    # halo-tile 3x3 path with concat input (chunks from two sources) + rowvec + two residuals, fp32 and h16 outputs
    Hh, Wh = 24, 47
    ah, sh = torch.randn(Fr, c0, Hh, Wh, generator=g), torch.randn(Fr, c1, Hh, Wh, generator=g)
    r0h, r1h = torch.randn(Fr, cout, Hh, Wh, generator=g), torch.randn(Fr, cout, Hh, Wh, generator=g)
    refh = F.conv2d(torch.cat([_r(ah, td), _r(sh, td)], 1), _r(wt, td), bias, padding=1)
    kwh = dict(x1=_nhwc(sh).to(td).to(gpu), F=Fr, Hin=Hh, Win=Wh, ksize=3, pad_t=1, pad_l=1, bias=bias.to(gpu))
    outh = hip.conv_gemm(dt, _nhwc(ah).to(td).to(gpu), wp.to(gpu), cout, K, rowvec=temb.to(gpu), res0=_nhwc(r0h).to(gpu), res1=_nhwc(r1h).to(gpu),
                         out_dtype=torch.float32, **kwh)
    goth = outh.cpu().reshape(Fr, Hh, Wh, cout).permute(0, 3, 1, 2)
    refh_full = refh + temb[:, :, None, None] + r0h + r1h
    assert (goth - refh_full).abs().max().item() <= 3e-4 * refh_full.abs().max().item()
    outh16 = hip.conv_gemm(dt, _nhwc(ah).to(td).to(gpu), wp.to(gpu), cout, K, **kwh)
    assert (outh16.float().cpu().reshape(Fr, Hh, Wh, cout).permute(0, 3, 1, 2) - refh).abs().max().item() <= 2 * ulp * refh.abs().max().item()
    # the same at 32 x 46 (whole 8-row patches, a ragged last patch column)
    Hh, Wh = 32, 46
    ah, sh = torch.randn(Fr, c0, Hh, Wh, generator=g), torch.randn(Fr, c1, Hh, Wh, generator=g)
    r0h, r1h = torch.randn(Fr, cout, Hh, Wh, generator=g), torch.randn(Fr, cout, Hh, Wh, generator=g)
    refh = F.conv2d(torch.cat([_r(ah, td), _r(sh, td)], 1), _r(wt, td), bias, padding=1)
    kwh = dict(x1=_nhwc(sh).to(td).to(gpu), F=Fr, Hin=Hh, Win=Wh, ksize=3, pad_t=1, pad_l=1, bias=bias.to(gpu))
    outh = hip.conv_gemm(dt, _nhwc(ah).to(td).to(gpu), wp.to(gpu), cout, K, rowvec=temb.to(gpu), res0=_nhwc(r0h).to(gpu), res1=_nhwc(r1h).to(gpu),
                         out_dtype=torch.float32, **kwh)
    goth = outh.cpu().reshape(Fr, Hh, Wh, cout).permute(0, 3, 1, 2)
    refh_full = refh + temb[:, :, None, None] + r0h + r1h
    assert (goth - refh_full).abs().max().item() <= 3e-4 * refh_full.abs().max().item()
    outh16 = hip.conv_gemm(dt, _nhwc(ah).to(td).to(gpu), wp.to(gpu), cout, K, **kwh)
    assert (outh16.float().cpu().reshape(Fr, Hh, Wh, cout).permute(0, 3, 1, 2) - refh).abs().max().item() <= 2 * ulp * refh.abs().max().item()
    # VAE-encoder style downsample: pad (0,1,0,1), stride 2, pad 0
    x = torch.randn(2, 64, 10, 12, generator=g)
    wd = torch.randn(128, 64, 3, 3, generator=g) / 24.0
    refd = F.conv2d(F.pad(_r(x, td), (0, 1, 0, 1)), _r(wd, td), None, stride=2)
    wpd, Kd = packing.pack_conv(wd, td)
    outd = hip.conv_gemm(dt, _nhwc(x).to(td).to(gpu), wpd.to(gpu), 128, Kd, F=2, Hin=10, Win=12, Hout=5, Wout=6, ksize=3, stride=2,
                         pad_t=0, pad_l=0, out_dtype=torch.float32)
    gotd = outd.cpu().reshape(2, 5, 6, 128).permute(0, 3, 1, 2)
    assert (gotd - refd).abs().max().item() <= 3e-4 * refd.abs().max().item()
    # GEGLU linear
    M, C = 300, 64
    x = torch.randn(M, C, generator=g)
    w8 = torch.randn(8 * C, C, generator=g) / math.sqrt(C)
    b8 = torch.randn(8 * C, generator=g)
    hfull = F.linear(_r(x, td), _r(w8, td), b8)
    v, gate = hfull.chunk(2, -1)
    refg = v * F.gelu(gate)
    wi, bi = packing.geglu_interleave(w8, b8)
    wpk = packing.pack_matrix(wi, td, geglu=True)
    outg = hip.conv_gemm(dt, x.to(td).to(gpu), wpk.to(gpu), 8 * C, C, F=1, Hin=M, Win=1, bias=bi.to(gpu), epilogue=hip.EPI_GEGLU,
                         out_dtype=torch.float32)
    assert outg.shape == (M, 4 * C)
    assert (outg.cpu() - refg).abs().max().item() <= 3e-4 * refg.abs().max().item()


@pytest.mark.parametrize("dname,td,ulp", DT)
@pytest.mark.parametrize("C,groups,HW,Fr,pool,f32in", [(320, 32, 150, 2, False, True), (64, 8, 37, 3, True, True),
                                                       (640, 32, 90, 2, False, False), (2560, 32, 20, 1, False, True)])
def test_groupnorm(gpu, dname, td, ulp, C, groups, HW, Fr, pool, f32in):
    from videovanish_amd import hip
    dt = hip.dtype_id(dname)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(Fr, HW, C, generator=g) * 2 + 0.5
    if not f32in:
        x = _r(x, td)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    xc = x.permute(0, 2, 1)  # [F,C,HW]
    if pool:
        ref = F.group_norm(xc.permute(1, 0, 2).reshape(1, C, Fr * HW), groups, gamma, beta, 1e-6).reshape(C, Fr, HW).permute(1, 0, 2)
    else:
        ref = F.group_norm(xc, groups, gamma, beta, 1e-6)
    ref = F.silu(ref).permute(0, 2, 1)
    half = C // 2 // 8 * 8
    xg = x.to(gpu) if f32in else x.to(td).to(gpu)
    for split in (False, True):
        if split:
            out = hip.groupnorm(dt, xg[..., :half].contiguous(), gamma.to(gpu), beta.to(gpu), groups, 1e-6, x1=xg[..., half:].contiguous(),
                                F=Fr, HW=HW, silu=True, pool_frames=pool, out_dtype=torch.float32)
        else:
            out = hip.groupnorm(dt, xg, gamma.to(gpu), beta.to(gpu), groups, 1e-6, F=Fr, HW=HW, silu=True, pool_frames=pool,
                                out_dtype=torch.float32)
        assert (out.cpu().reshape(Fr, HW, C) - ref).abs().max().item() <= 2e-4 * max(1.0, ref.abs().max().item())
    out16 = hip.groupnorm(dt, xg, gamma.to(gpu), beta.to(gpu), groups, 1e-6, F=Fr, HW=HW, silu=True, pool_frames=pool)
    assert (out16.float().cpu().reshape(Fr, HW, C) - ref).abs().max().item() <= 2 * ulp * ref.abs().max().item()


@pytest.mark.parametrize("dname,td,ulp", DT)
@pytest.mark.parametrize("M,C,rpf", [(37, 320, 5), (10, 1280, 2), (9, 64, 3)])
def test_layernorm(gpu, dname, td, ulp, M, C, rpf):
    from videovanish_amd import hip
    dt = hip.dtype_id(dname)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(M, C, generator=g) * 3 + 1
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    pe = torch.randn((M + rpf - 1) // rpf, C, generator=g)
    ref = F.layer_norm(x, (C,), gamma, beta, 1e-5)
    out = hip.layernorm(dt, x.to(gpu), gamma.to(gpu), beta.to(gpu))
    assert (out.float().cpu() - ref).abs().max().item() <= 2 * ulp * ref.abs().max().item()
    ref2 = ref + pe.repeat_interleave(rpf, 0)[:M]
    out2 = hip.layernorm(dt, x.to(gpu), gamma.to(gpu), beta.to(gpu), pe=pe.to(gpu), rows_per_frame=rpf)
    assert (out2.float().cpu() - ref2).abs().max().item() <= 2 * ulp * ref2.abs().max().item()


def _attn_ref(q, k, v):
    d = q.shape[-1]
    s = (q @ k.transpose(-1, -2)) * d ** -0.5
    return torch.softmax(s, -1) @ v


@pytest.mark.parametrize("dname,td,ulp", DT)
@pytest.mark.parametrize("B,heads,Nq,Nkv,D", [(2, 8, 200, 200, 40), (1, 8, 130, 130, 80), (2, 8, 70, 70, 160), (1, 1, 150, 150, 512),
                                              (2, 2, 100, 77, 32), (3, 8, 64, 77, 40), (1, 2, 129, 129, 64)])
def test_attention_spatial(gpu, dname, td, ulp, B, heads, Nq, Nkv, D):
    """fused-QKV layout for self attention; separate K/V with batch stride 0 for cross attention (Nq != Nkv)."""
    from videovanish_amd import hip
    dt = hip.dtype_id(dname)
    taken = hip.attention_route(dt, (1,), (1,), (1,), (1,), B=B, heads=heads, Nq=Nq, Nkv=Nkv, D=D, q_bs=8, k_bs=8, v_bs=8, o_bs=8, q_rs=8, k_rs=8, v_rs=8, o_rs=8)
    assert hip.attn_route_name(taken) == {(200, 40): "mfma32-d40 ragged", (130, 80): "reg80 self", (70, 160): "w4x32", (150, 512): "d512-w4", (100, 32): "dma64 cross",
                                          (64, 40): "dma64 cross", (129, 64): "dma64 self"}[(Nq, D)]        # (strides do not enter the route)
    g = torch.Generator().manual_seed(5)
    C = heads * D
    q = _r(torch.randn(B, Nq, heads, D, generator=g), td)
    shared_kv = Nq != Nkv
    kb = 1 if shared_kv else B
    k = _r(torch.randn(kb, Nkv, heads, D, generator=g) * 1.5, td)
    v = _r(torch.randn(kb, Nkv, heads, D, generator=g), td)
    ref = _attn_ref(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2)      # [B,Nq,heads,D]
    out = torch.empty(B, Nq, C, dtype=td, device=gpu)
    if shared_kv:
        kv = torch.cat([k.reshape(1, Nkv, C), v.reshape(1, Nkv, C)], -1).to(td).to(gpu)           # [1,Nkv,2C]
        qd = q.reshape(B, Nq, C).to(td).to(gpu)
        hip.attention(dt, qd, kv, kv, out, B=B, heads=heads, Nq=Nq, Nkv=Nkv, D=D, q_bs=Nq * C, k_bs=0, v_bs=0, o_bs=Nq * C, q_rs=C,
                      k_rs=2 * C, v_rs=2 * C, o_rs=C, v_off=C)
    else:
        qkv = torch.cat([q.reshape(B, Nq, C), k.reshape(B, Nkv, C), v.reshape(B, Nkv, C)], -1).to(td).to(gpu)   # [B,N,3C]
        hip.attention(dt, qkv, qkv, qkv, out, B=B, heads=heads, Nq=Nq, Nkv=Nkv, D=D, q_bs=Nq * 3 * C, k_bs=Nq * 3 * C, v_bs=Nq * 3 * C,
                      o_bs=Nq * C, q_rs=3 * C, k_rs=3 * C, v_rs=3 * C, o_rs=C, k_off=C, v_off=2 * C)
    got = out.float().cpu().reshape(B, Nq, heads, D)
    assert (got - ref).abs().max().item() <= 4 * ulp * max(1.0, ref.abs().max().item())
    if not shared_kv:
        # head-major layout [b][q|k|v][head][token][D] (what vv_conv_gemm's split_heads store writes): same result bit for bit
        hm = torch.stack([q, k, v], 1).permute(0, 1, 3, 2, 4).contiguous().to(td).to(gpu)      # [B,3,heads,N,D]
        out2 = torch.empty_like(out)
        hip.attention(dt, hm, hm, hm, out2, B=B, heads=heads, Nq=Nq, Nkv=Nkv, D=D, q_bs=3 * Nq * C, k_bs=3 * Nq * C, v_bs=3 * Nq * C,
                      o_bs=Nq * C, q_rs=D, k_rs=D, v_rs=D, o_rs=C, k_off=Nq * C, v_off=2 * Nq * C, q_hs=Nq * D, k_hs=Nq * D, v_hs=Nq * D)
        assert torch.equal(out2.cpu(), out.cpu())


@pytest.mark.parametrize("dname,td,ulp", DT)
@pytest.mark.parametrize("M,K,N,flags", [(3000, 640, 640, "res f32out"), (2900, 640, 640, "f32out"), (1000, 1280, 1280, "res f32out p8"), (2600, 640, 1920, "split80"),
                                         (777, 640, 640, "h16out"), (2048, 640, 1280, "geglu"), (1500, 2560, 640, "res f32out scale")])
def test_gemm_tile_forms_agree_on_every_epilogue(gpu, dname, td, ulp, M, K, N, flags):
    """The epilogue forms of vv_gemm_epilogue.h (round 5: lean -- bias folded into the accumulators --, staged -- fp32 strips through a wave-private LDS tile, read /
    written row-major --, and the old tile-by-tile form of the 128-row loaders) compute the same arithmetic in the same order: a linear layer run on the 128-row tile
    (tile_hint 1), the 2-phase 256-row kernel (tile_hint 2: lean + staged) and the 8-phase one (tile_hint 3: lean; N % 256 == 0) gives the same bits, ragged last
    row tile included, and matches fp32 torch on the rounded operands."""
    from videovanish_amd import hip, packing
    dt = hip.dtype_id(dname)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    geglu, res = "geglu" in flags, "res" in flags
    f32out = "f32out" in flags
    scale = 0.5 if "scale" in flags else 1.0
    if geglu:
        wi, bi = packing.geglu_interleave(w, b)
        wp, bias = packing.pack_matrix(wi, td, geglu=True).to(gpu), bi.to(gpu)
    else:
        wp, bias = packing.pack_matrix(w, td).to(gpu), b.to(gpu)
    r = torch.randn(M, N, generator=g) if res else None
    kw = dict(F=1, Hin=M, Win=1, bias=bias, res0=r.to(gpu) if res else None, epilogue=hip.EPI_GEGLU if geglu else hip.EPI_NONE, out_scale=scale)
    if "split80" in flags:
        kw.update(split_heads=N // 3 // 80, split_dim=80, split_tokens=M // 2)      # two batch elements
    xg = x.to(td).to(gpu)
    outs = {}
    # the kernel each hint names is the kernel that runs (vv_conv_gemm_route): an ineligible case would silently compare the 128-row tile with itself
    want = {1: lambda r: 0 < r < hip.ROUTE_256x320_LIN,
            2: lambda r: r == (hip.ROUTE_256x320_LIN if (N % 320 == 0 and not geglu) else hip.ROUTE_256x256_LIN),
            3: lambda r: r == hip.ROUTE_256P8_LIN}
    for hint in (1, 2) + ((3,) if (N % 256 == 0 and ("p8" in flags or geglu)) else ()):
        out = torch.zeros(M, N // 2 if geglu else N, dtype=torch.float32 if f32out else td, device=gpu)
        route = hip.conv_gemm_route(dt, xg, wp, N, K, out=out, tile_hint=hint, **kw)
        assert route > 0 and want[hint](route), f"tile_hint {hint} runs {hip.route_name(route) if route > 0 else route}"
        hip.conv_gemm(dt, xg, wp, N, K, out=out, tile_hint=hint, **kw)
        outs[hint] = out.float().cpu()
    for hint, o in outs.items():
        assert torch.equal(o, outs[1]), f"tile_hint {hint} differs from the 128-row tile"
    if "split80" not in flags:
        y = _r(x, td) @ _r(w, td).t() + b
        if geglu:
            y = y[:, : N // 2] * F.gelu(y[:, N // 2:])
        ref = y * scale + (r if res else 0.0)
        tol = (3e-4 if f32out else 2 * ulp) * max(1.0, ref.abs().max().item())
        assert (outs[1] - ref).abs().max().item() <= tol


@pytest.mark.parametrize("dname,td,ulp", DT)
@pytest.mark.parametrize("Fr,H,W,Hv,Wv,C,N,f32in,precise", [(2, 9, 12, 18, 24, 64, 64, False, False), (2, 9, 12, 17, 24, 64, 96, False, False),
                                                           (1, 5, 8, 10, 16, 128, 64, True, False), (3, 2, 4, 3, 8, 64, 64, False, False),
                                                           (2, 23, 40, 45, 80, 64, 160, False, False), (1, 6, 7, 11, 13, 64, 64, False, False),
                                                           (2, 8, 14, 15, 27, 64, 64, False, False), (1, 5, 7, 10, 13, 64, 64, True, False),
                                                           (1, 2, 2, 3, 3, 64, 64, False, False), (1, 6, 7, 12, 15, 64, 64, False, False),
                                                           (1, 7, 9, 14, 18, 64, 32, True, True), (1, 7, 9, 13, 17, 64, 32, True, True),
                                                           (1, 16, 32, 32, 64, 64, 128, False, False), (2, 15, 32, 30, 64, 128, 160, False, False),      # patch grids the halo loader takes (round 5: 2x2 taps + scatter)
                                                           (1, 16, 16, 32, 32, 64, 128, True, True), (1, 8, 16, 16, 32, 64, 64, False, False)])
def test_upconv2x_parity_phases(gpu, dname, td, ulp, Fr, H, W, Hv, Wv, C, N, f32in, precise):
    """nn.UpConv2x: the 3x3 convolution of an Upsample2D layer as four 2x2 convolutions over the SOURCE image (taps on the same source pixel summed,
    scattered store, ABI 9) against torch's interpolate(nearest) + conv2d with exact weights -- even sizes, Hv = 2 H - 1 and / or Wv = 2 W - 1 (the
    last row / column / corner have their own launches; 45 x 80 from 23 x 40 is UNet level 2 -> 1 at 720p, 15 x 27 from 8 x 14 is c2's level 3 -> 2),
    a width outside the family (15 from 7: fallback to the fused-gather form), fp32 and h16 sources, bias + residual, split precision (the VAE
    decoder) -- and against the fused-gather form itself."""
    from videovanish_amd import hip
    from videovanish_amd.nn import Ctx, UpConv2x
    ctx = Ctx(gpu, dname, weight_seed=7)
    g = torch.Generator().manual_seed(31)
    up = UpConv2x(ctx, "test.upsamplers.0.conv", C, N, precise=precise)
    w, b = ctx.src.conv("test.upsamplers.0.conv", C, N, 3, 1.0)
    x = torch.randn(Fr, C, H, W, generator=g)
    xr = x if precise else _r(x, td)
    res = torch.randn(Fr, N, Hv, Wv, generator=g)
    ref = F.conv2d(F.interpolate(xr, size=(Hv, Wv), mode="nearest"), w.float(), b.float(), padding=1) + res
    xin = (_nhwc(xr).to(gpu) if f32in else _nhwc(xr).to(td).to(gpu)).reshape(-1, C)          # [M, C], as the layers hand it over
    out, ho, wo = up(xin, Fr, H, W, Hv=Hv, Wv=Wv, res1=_nhwc(res).to(gpu))
    assert (ho, wo) == (Hv, Wv) and out.dtype == torch.float32
    got = out.cpu().reshape(Fr, Hv, Wv, N).permute(0, 3, 1, 2)
    scale = max(1.0, (ref - res).abs().max().item())
    err = (got - ref).abs().max().item()
    tol = ((2.0 ** -16 if td == torch.float16 else 2.0 ** -10) if precise else 3 * ulp) * scale      # split precision: ~2x the operand's bits
    assert err <= tol, (err, tol)
    old, _, _ = up.fallback()(xin, Fr, H, W, Hv=Hv, Wv=Wv, res1=_nhwc(res).to(gpu))          # the fused-gather 3x3 form (9 taps, weights rounded one by one)
    assert (old - out).abs().max().item() <= tol
    if Wv > 2 * W:
        assert torch.equal(old, out)                                                          # ... which IS the path sizes outside the family take


def test_conv_gemm_scatter_arguments(gpu):
    """vv_conv_params.sc_* (ABI 9): a grid that does not hold the launch's rows, a missing output tensor, GEGLU / rowvec with a scatter are refused by name;
    a 1x1 launch scattered with step 1 / origin 0 into its own grid equals the plain launch bit for bit (also through a 256-row-eligible shape, which
    must stay on the 128-row kernels)."""
    from videovanish_amd import hip, packing
    td, dt = torch.float16, hip.F16
    g = torch.Generator().manual_seed(41)
    Fr, H, W, C, N = 2, 6, 8, 64, 320
    x = torch.randn(Fr * H * W, C, generator=g).to(td).to(gpu)
    w = packing.pack_matrix(torch.randn(N, C, generator=g) / 8.0, td).to(gpu)
    plain = hip.conv_gemm(dt, x, w, N, C, F=Fr, Hin=H, Win=W, out_dtype=torch.float32)
    out = torch.zeros(Fr * H * W, N, dtype=torch.float32, device=gpu)
    hip.conv_gemm(dt, x, w, N, C, F=Fr, Hin=H, Win=W, out=out, scatter=(H, W, 1, 1, 0, 0))
    assert torch.equal(out, plain)
    big = torch.zeros(Fr * 2 * H * 2 * W, N, dtype=torch.float32, device=gpu)
    hip.conv_gemm(dt, x, w, N, C, F=Fr, Hin=H, Win=W, out=big, scatter=(2 * H, 2 * W, 2, 2, 1, 0))
    assert torch.equal(big.view(Fr, 2 * H, 2 * W, N)[:, 1::2, 0::2].reshape(-1, N), plain) and big.view(Fr, 2 * H, 2 * W, N)[:, 0::2].abs().max().item() == 0.0
    with pytest.raises(RuntimeError, match="scatter"):
        hip.conv_gemm(dt, x, w, N, C, F=Fr, Hin=H, Win=W, out=big, scatter=(2 * H - 1, 2 * W, 2, 2, 1, 0))       # row 2 (H - 1) + 1 does not exist
    with pytest.raises(RuntimeError, match="scatter"):
        hip.conv_gemm(dt, x, w, N, C, F=Fr, Hin=H, Win=W, scatter=(2 * H, 2 * W, 2, 2, 0, 0))                    # no output tensor
    with pytest.raises(RuntimeError, match="scatter"):
        hip.conv_gemm(dt, x, w, N, C, F=Fr, Hin=H, Win=W, out=big, rowvec=torch.zeros(Fr, N, device=gpu), scatter=(2 * H, 2 * W, 2, 2, 0, 0))


@pytest.mark.parametrize("dname,td,ulp", DT)
def test_conv_gemm_split_heads(gpu, dname, td, ulp):
    """fused QKV projection with the head-major store: out[b][which][head][token][d] == linear(x)[b*T+token][which*C + head*D + d]."""
    from videovanish_amd import hip, packing
    dt = hip.dtype_id(dname)
    g = torch.Generator().manual_seed(15)
    B, T, heads, D = 3, 70, 8, 40
    C = heads * D
    x = torch.randn(B * T, C, generator=g)
    w = torch.randn(3 * C, C, generator=g) / math.sqrt(C)
    wp = packing.pack_matrix(w, td).to(gpu)
    plain = hip.conv_gemm(dt, x.to(td).to(gpu), wp, 3 * C, C, F=1, Hin=B * T, Win=1)
    split = hip.conv_gemm(dt, x.to(td).to(gpu), wp, 3 * C, C, F=1, Hin=B * T, Win=1, split_heads=heads, split_dim=D, split_tokens=T)
    want = plain.cpu().reshape(B, T, 3, heads, D).permute(0, 2, 3, 1, 4).contiguous()
    assert torch.equal(split.cpu().reshape(B, 3, heads, T, D), want)
    ref = F.linear(_r(x, td), _r(w, td))
    assert (plain.float().cpu() - ref).abs().max().item() <= 2 * ulp * ref.abs().max().item()
    with pytest.raises(RuntimeError):
        hip.conv_gemm(dt, x.to(td).to(gpu), wp, 3 * C, C, F=1, Hin=B * T, Win=1, split_heads=heads, split_dim=D, split_tokens=T, out_dtype=torch.float32)
    # token-major rows (temporal attention: row = frame*HW + pixel, batch element = pixel): split_tokens < 0
    tm = hip.conv_gemm(dt, x.to(td).to(gpu), wp, 3 * C, C, F=1, Hin=B * T, Win=1, split_heads=heads, split_dim=D, split_tokens=-B)
    want_tm = plain.cpu().reshape(B, T, 3, heads, D).permute(1, 2, 3, 0, 4).contiguous()       # rows = (token=B index, b=T index)
    assert torch.equal(tm.cpu().reshape(T, 3, heads, B, D), want_tm)


@pytest.mark.parametrize("dname,td,ulp", DT)
@pytest.mark.parametrize("Fr,HW,heads,D", [(32, 50, 8, 40), (8, 33, 8, 80), (22, 20, 8, 160), (5, 12, 2, 32)])
def test_attention_temporal(gpu, dname, td, ulp, Fr, HW, heads, D):
    """b = pixel, i = frame: rows of the [F*HW, 3C] QKV matrix are gathered with stride HW*3C."""
    from videovanish_amd import hip
    dt = hip.dtype_id(dname)
    taken = hip.attention_route(dt, (1,), (1,), (1,), (1,), B=HW, heads=heads, Nq=Fr, Nkv=Fr, D=D, q_bs=8, k_bs=8, v_bs=8, o_bs=8, q_rs=8, k_rs=8, v_rs=8, o_rs=8)
    assert hip.attn_route_name(taken) == {40: "short", 80: "short", 160: "short-2w", 32: "short"}[D]
    g = torch.Generator().manual_seed(6)
    C = heads * D
    qkv = _r(torch.randn(Fr, HW, 3, heads, D, generator=g), td)
    q, k, v = (qkv[:, :, i].permute(1, 2, 0, 3) for i in range(3))       # [HW,heads,F,D]
    ref = _attn_ref(q, k, v).permute(2, 0, 1, 3)                          # [F,HW,heads,D]
    buf = qkv.reshape(Fr * HW, 3 * C).to(td).to(gpu)
    out = torch.empty(Fr * HW, C, dtype=td, device=gpu)
    hip.attention(dt, buf, buf, buf, out, B=HW, heads=heads, Nq=Fr, Nkv=Fr, D=D, q_bs=3 * C, k_bs=3 * C, v_bs=3 * C, o_bs=C, q_rs=HW * 3 * C,
                  k_rs=HW * 3 * C, v_rs=HW * 3 * C, o_rs=HW * C, k_off=C, v_off=2 * C)
    got = out.float().cpu().reshape(Fr, HW, heads, D)
    assert (got - ref).abs().max().item() <= 4 * ulp * max(1.0, ref.abs().max().item())


def test_attention_online_softmax_rescale(gpu):
    """Force the running max to jump at a late KV tile (guide rule 26): spike one key far above the rest."""
    from videovanish_amd import hip
    td, dt = torch.bfloat16, hip.BF16
    g = torch.Generator().manual_seed(7)
    B, heads, N, D = 1, 8, 400, 40
    C = heads * D
    q = _r(torch.randn(B, N, heads, D, generator=g), td)
    k = _r(torch.randn(B, N, heads, D, generator=g), td)
    v = _r(torch.randn(B, N, heads, D, generator=g), td)
    k[0, 333] = q[0, 17] * 6.0          # key 333 (6th tile) dominates for query 17 and shifts many maxima
    k[0, 5] = -q[0, 200] * 6.0
    ref = _attn_ref(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2)
    qkv = torch.cat([q.reshape(B, N, C), k.reshape(B, N, C), v.reshape(B, N, C)], -1).to(td).to(gpu)
    out = torch.empty(B, N, C, dtype=td, device=gpu)
    hip.attention(dt, qkv, qkv, qkv, out, B=B, heads=heads, Nq=N, Nkv=N, D=D, q_bs=N * 3 * C, k_bs=N * 3 * C, v_bs=N * 3 * C, o_bs=N * C,
                  q_rs=3 * C, k_rs=3 * C, v_rs=3 * C, o_rs=C, k_off=C, v_off=2 * C)
    got = out.float().cpu().reshape(B, N, heads, D)
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() <= 2 ** -6 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("N", [64 * 9 - 37, 64 * 9, 64 * 18 - 37, 64 * 17])      # 32 queries per wave (N < 1024) / 64 queries per wave, each with a ragged and a whole last tile
@pytest.mark.parametrize("D", [40, 80])                                   # d = 80: attn80_kernel (N >= 512; the reference enters through the MFMA's C operand)
@pytest.mark.parametrize("dname,td,ulp", [("bf16", torch.bfloat16, 2 ** -8), ("fp16", torch.float16, 2 ** -11)])
def test_attention_d40_lazy_reference_maximum(gpu, dname, td, ulp, N, D):
    """The d = 40 spatial kernels subtract a softmax reference ON THE MATRIX PIPE (vv_attn32.hip attn40_kernel / attn40q2_kernel / attn80_kernel: the reference is
    fixed once from a 64-key sample, P may exceed 1, a block whose denominator overflows repeats its keys with the exact maximum): exercise
    what that adds -- q_prescaled (scale * log2 e folded into q before its one rounding), maxima that creep up tile after tile, maxima that
    jump by hundreds in a late tile (fp16: overflow -> the exact-maximum repeat), a first tile far BELOW the rest, a ragged last tile,
    rows past Nq."""
    from videovanish_amd import hip
    dt = hip.dtype_id(dname)
    g = torch.Generator().manual_seed(11)
    B, heads = 2, 8
    C = heads * D
    c = hip.attention_q_scale(D)
    q = torch.randn(B, N, heads, D, generator=g)
    k = torch.randn(B, N, heads, D, generator=g)
    v = _r(torch.randn(B, N, heads, D, generator=g), td)
    u = q[:, :1].mean(2, keepdim=True) * 0 + torch.randn(B, 1, heads, D, generator=g)      # a common direction per (b, head)
    q = q + 2.0 * u                                                                          # every query likes keys along u
    ramp = torch.linspace(-3.0, 3.0, N).view(1, N, 1, 1)                                     # key affinity creeps up tile after tile
    k = k * 0.3 + u * ramp / (u * u).sum(-1, keepdim=True) * 4.0
    k[:, :64] -= 3.0 * u[:, :1] * 1.0                                                        # first tile far below the rest
    k[0, 500] = q[0, 17] * 5.0                                                               # one late key dominates some rows by a wide margin
    k = _r(k, td)
    for prescaled in (True, False):
        qs = _r(q * c, td) if prescaled else _r(q, td)
        s = torch.einsum("bqhd,bkhd->bhqk", qs.double(), k.double()) * (1.0 if prescaled else c)
        pr = torch.exp2(s - s.amax(-1, keepdim=True))
        ref = torch.einsum("bhqk,bkhd->bqhd", pr / pr.sum(-1, keepdim=True), v.double()).float()
        hm = torch.stack([qs, k, v], 1).permute(0, 1, 3, 2, 4).contiguous().to(td).to(gpu)      # head-major, as the pipeline stores it
        out = torch.empty(B, N, C, dtype=td, device=gpu)
        hip.attention(dt, hm, hm, hm, out, B=B, heads=heads, Nq=N, Nkv=N, D=D, q_bs=3 * N * C, k_bs=3 * N * C, v_bs=3 * N * C, o_bs=N * C,
                      q_rs=D, k_rs=D, v_rs=D, o_rs=C, k_off=N * C, v_off=2 * N * C, q_hs=N * D, k_hs=N * D, v_hs=N * D, q_prescaled=prescaled)
        got = out.float().cpu().reshape(B, N, heads, D)
        assert torch.isfinite(got).all()
        spread = float((s.amax(-1) - s.amin(-1)).max())
        assert spread > 60                                  # the case really spans far more than the h16 exponent range would forgive
        # without q_prescaled the kernel re-rounds c*q: the scores (|s| up to hundreds here) then carry that second rounding
        tol = (6 if prescaled else 64) * ulp * max(1.0, ref.abs().max().item())
        assert (got - ref).abs().max().item() <= tol, (prescaled, (got - ref).abs().max().item(), tol)


def test_elementwise(gpu):
    from videovanish_amd import hip
    g = torch.Generator().manual_seed(8)
    x, e, z = (torch.randn(5, 7, 9, 4, generator=g) for _ in range(3))
    out = hip.axpby(x.to(gpu), e.to(gpu), 0.3, 0.7).cpu()
    assert torch.equal(out, np.float32(0.3) * x + np.float32(0.7) * e)
    sa, sb, c0, c1, c2 = 0.9, 0.43, 0.95, 0.31, 0.2
    ref = np.float32(c0) * ((x - np.float32(sb) * e) / np.float32(sa)) + np.float32(c1) * e
    assert torch.equal(hip.sched_step(x.to(gpu), e.to(gpu), None, sa, sb, c0, c1).cpu(), ref)
    assert torch.equal(hip.sched_step(x.to(gpu), e.to(gpu), z.to(gpu), sa, sb, c0, c1, c2).cpu(), ref + np.float32(c2) * z)
    y = torch.randn(5, 7, 9, 4, generator=g)
    xa = x.clone().to(gpu)
    hip.add_inplace(hip.BF16, xa, y.to(gpu))
    assert torch.equal(xa.cpu(), x + y)
    xb = x.clone().to(gpu)
    hip.add_inplace(hip.BF16, xb, y.to(torch.bfloat16).to(gpu))
    assert torch.equal(xb.cpu(), x + y.to(torch.bfloat16).float())
    # pad_channels / brushnet_input / preprocess / decode_blend
    lat = torch.randn(2, 5, 6, 4, generator=g)
    pc = hip.pad_channels(hip.BF16, lat.to(gpu), 8, 1.0).float().cpu()
    assert torch.equal(pc[..., :4], lat.to(torch.bfloat16).float()) and (pc[..., 4:] == 0).all()
    cond = torch.randn(2, 5, 6, 4, generator=g)
    mask = (torch.rand(2, 40, 48, generator=g) > 0.5).to(torch.uint8) * 255
    bi = hip.brushnet_input(hip.BF16, lat.to(gpu), cond.to(gpu), mask.to(gpu), 40, 48).float().cpu()
    mref = F.interpolate((mask > 0).float()[:, None], size=(5, 6), mode="nearest")[:, 0]
    assert torch.equal(bi[..., :4], lat.to(torch.bfloat16).float()) and torch.equal(bi[..., 4:8], cond.to(torch.bfloat16).float())
    assert torch.equal(bi[..., 8], mref) and (bi[..., 9:] == 0).all()
    fr = torch.randint(0, 256, (2, 40, 48, 3), generator=g, dtype=torch.uint8)
    img, msk = hip.preprocess(hip.F16, fr.to(gpu), mask.to(gpu))
    iref = (fr.float() / 127.5 - 1.0)
    assert torch.equal(img.float().cpu()[..., :3], iref.to(torch.float16).float()) and (img.float().cpu()[..., 3:] == 0).all()
    assert torch.equal(msk.float().cpu()[..., :3], (iref * (1 - (mask > 0).float()[..., None])).to(torch.float16).float())
    dec = torch.randn(2, 40, 48, 16, generator=g)
    acc = torch.rand(2, 40, 48, 3, generator=g)
    w = torch.tensor([0.25, 1.0])
    pix = (dec[..., :3] / 2 + 0.5).clamp(0, 1)
    refb = acc * (1.0 - w)[:, None, None, None] + pix * w[:, None, None, None]
    got = hip.decode_blend(dec.to(gpu), w.to(gpu), acc.clone().to(gpu)).cpu()
    assert torch.equal(got, refb)


def test_image_kernels_bit_exact(gpu):
    from oracle import imageops_ref as I
    from videovanish_amd import hip, imageops
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_intree.npz"))
    masks = torch.from_numpy(fx["masks"]).to(gpu)
    for k in (0, 1, 3, 8):
        got = hip.mask_collapse_dilate(masks, k).cpu().numpy()
        assert (got == fx[f"dilated_k{k}"]).all(), k
    empty = torch.zeros_like(masks)
    assert (hip.mask_collapse_dilate(empty, 0).cpu().numpy() == 0).all()
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    for (Hd, Wd) in [(40, 56), (24, 31), (37, 53), (111, 80)]:
        got = hip.resize_u8(torch.from_numpy(img).to(gpu), Hd, Wd).cpu().numpy()
        ref = np.stack([I.resize_bilinear_u8(f, Wd, Hd) for f in img])
        assert (got == ref).all(), (Hd, Wd)
        gotn = hip.resize_u8(torch.from_numpy(img).to(gpu), Hd, Wd, mode="nearest").cpu().numpy()
        refn = np.stack([I.resize_nearest_u8(f, Wd, Hd) for f in img])
        assert (gotn == refn).all(), (Hd, Wd)
    # chamfer DT inside the window radius + feather composite
    m = (rng.random((2, 45, 50)) < 0.3).astype(np.uint8) * 255
    m[0, 10:30, 10:35] = 255
    R = 5
    got = hip.chamfer_dt(torch.from_numpy(m).to(gpu), R).cpu().numpy()
    for t in range(2):
        ref = I.distance_transform_l2_5(m[t])
        sel = ref <= R
        assert (got[t][sel] == ref[sel]).all()
        assert (got[t][~sel] > R).all()
    inp = rng.integers(0, 256, (2, 45, 50, 3), dtype=np.uint8)
    orig = rng.integers(0, 256, (2, 45, 50, 3), dtype=np.uint8)
    for feather in (3.0, 1.0, 0.0, 2.5):
        got = hip.feather_composite(torch.from_numpy(inp).to(gpu), torch.from_numpy(orig).to(gpu), torch.from_numpy(m).to(gpu), feather).cpu().numpy()
        ref = np.stack([I.composite(inp[t], orig[t], I.feather_alpha(m[t], feather)) for t in range(2)])
        assert (got == ref).all(), feather
    pix = rng.random((2, 45, 50, 3), dtype=np.float32)
    got = hip.blur_compose(torch.from_numpy(pix).to(gpu), torch.from_numpy(orig).to(gpu), torch.from_numpy(m).to(gpu),
                           imageops.gaussian_taps_21()).cpu().numpy()
    ref = np.stack([I.blur_compose(pix[t], orig[t], m[t]) for t in range(2)])
    assert (got == ref).all()


@pytest.mark.parametrize("dname,tol", [("fp16", 3e-6), ("bf16", 1.5e-4)])
def test_precise_split_conv_and_linear(gpu, dname, tol):
    """Split-precision layers (hi*wh + lo*wh + hi*wl as ONE K-concatenated MFMA launch: hip.split3 / nn.split3_weight) against an fp64 reference on
    UN-rounded fp32 operands: the error must sit orders of magnitude below the one-pass h16 layer (5e-4 fp16 / 4e-3 bf16)."""
    from videovanish_amd import nn as vnn
    g = torch.Generator().manual_seed(31)
    Fr, H, W, cin, cout = 2, 12, 20, 64, 128

    class Src:
        def conv(self, name, ci, co, k, gain=1.0):
            return torch.randn(co, ci, k, k, generator=g) / math.sqrt(ci * k * k), torch.randn(co, generator=g)

        def linear(self, name, ci, co, gain=1.0, bias=True):
            return torch.randn(co, ci, generator=g) / math.sqrt(ci), torch.randn(co, generator=g)

    ctx = vnn.Ctx("cuda:0", dname, 0, weights=Src())
    x = torch.randn(Fr, cin, H, W, generator=g)
    res = torch.randn(Fr, cout, H, W, generator=g)
    for precise in (False, True):
        g.manual_seed(32)
        conv = vnn.Conv(ctx, "c", cin, cout, k=3, precise=precise)
        g.manual_seed(32)
        w, b = Src().conv("c", cin, cout, 3)
        ref = F.conv2d(x.double(), w.double(), b.double(), padding=1) + res.double()
        xin = _nhwc(x).reshape(-1, cin).to(gpu)
        if not precise:
            xin = xin.to(ctx.h16)
        out, _, _ = conv(xin, Fr, H, W, res0=_nhwc(res).reshape(-1, cout).to(gpu))
        got = out.cpu().reshape(Fr, H, W, cout).permute(0, 3, 1, 2).double()
        err = ((got - ref).abs().max() / ref.abs().max()).item()
        print(f"conv3 {dname} precise={precise}: rel max err {err:.2e}")
        assert err <= (tol if precise else 1e-2)
        if precise:
            assert err <= tol
    g.manual_seed(33)
    lin = vnn.Linear(ctx, "l", cin, cout, precise=True)
    g.manual_seed(33)
    w, b = Src().linear("l", cin, cout)
    xm = torch.randn(300, cin, generator=g)
    ref = xm.double() @ w.double().t() + b.double()
    got = lin(xm.to(gpu)).cpu().double()
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"linear {dname} precise: rel max err {err:.2e}")
    assert err <= tol


@pytest.mark.parametrize("hs,vs", [(1, 1), (1, 0), (0, 0), (2, 0)])
def test_ycbcr_to_rgb_gpu_equals_host(gpu, hs, vs, tmp_path):
    """row n3, GPU-side colour conversion: vv_ycbcr_to_rgb is bit for bit the host routine vvio_ycbcr_to_rgb (and through it the numpy
    restatement in tests/test_frameio_cpu.py); the frame loader takes the GPU path when a device is visible."""
    from videovanish_amd import frameio as FIO
    from videovanish_amd import hip
    rng = np.random.default_rng(11)
    T, H, W = 3, 37, 53
    ch, cw = (H + (1 << vs) - 1) >> vs, (W + (1 << hs) - 1) >> hs
    y, cb, cr = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((T, H, W), (T, ch, cw), (T, ch, cw)))
    for full in (False, True):
        host = FIO.ycbcr_to_rgb(y, cb, cr, hs, vs, full, device=False)
        dev = hip.ycbcr_to_rgb(torch.from_numpy(y).to(gpu), torch.from_numpy(cb).to(gpu), torch.from_numpy(cr).to(gpu), hs, vs, full).cpu().numpy()
        assert np.array_equal(dev, host)
        assert np.array_equal(FIO.ycbcr_to_rgb(y, cb, cr, hs, vs, full, device=True), host)          # the loader's explicit GPU path
    if (hs, vs) == (1, 1):
        p = str(tmp_path / "clip.y4m")
        with open(p, "wb") as f:
            f.write(b"YUV4MPEG2 W%d H%d F25:1 C420jpeg\n" % (W, H))
            for t in range(T):
                f.write(b"FRAME\n" + y[t].tobytes() + cb[t].tobytes() + cr[t].tobytes())
        frames, fps = FIO.load_video_frames_from_path(p)
        assert fps == 25.0 and all(np.array_equal(a, b) for a, b in zip(frames, FIO.ycbcr_to_rgb(y, cb, cr, 1, 1, False, device=False)))


@pytest.mark.parametrize("D", [40, 80])
@pytest.mark.parametrize("orders", [12, 13, 16, 20])
def test_attention_d40_heavy_tail(gpu, orders, D):
    """The shape real softmax logits take and random-init weights never produce: N = 14400 keys, ONE key -- a member of the kernel's 64-key sample
    (keys 0, 225, 450, ...) -- 12 .. 20 binary orders above a bulk of thousands of keys that still carries part of the softmax mass (12 / 13 orders:
    78 % / 64 % of it; 16: 18 %; 20: 1.4 %).  The optimistic reference of attn40 / attn40q2 is fixed from the sample maximum: with P = 2^-4 there
    (round 3) the bulk went subnormal / to zero in fp16; with P = 2^4 (round 4) it keeps full precision.  fp16, 6 ulp of the output range, against
    an fp64 softmax; both kernels (N >= 1024 -> 64 queries per wave; the first 640 queries through a second, short launch -> 32 per wave)."""
    from videovanish_amd import hip
    td, dt, ulp = torch.float16, hip.F16, 2 ** -11
    g = torch.Generator().manual_seed(100 + orders)
    B, heads, N = 1, 8, 14400
    C = heads * D
    u = torch.nn.functional.normalize(torch.randn(B, 1, heads, D, generator=g), dim=-1)
    q = 3.0 * u + 0.05 * torch.randn(B, N, heads, D, generator=g)                 # every query looks along u: c q.u ~ 3 (log2 units after the scale below)
    k = 0.3 * torch.randn(B, N, heads, D, generator=g)                            # the bulk: scores within a few binary orders of 0
    v = torch.randn(B, N, heads, D, generator=g)
    k[:, 225 * 7] = u[:, 0] * (orders / 3.0)                                      # the outlier (sampled: key 1575): c q.k ~ orders above the bulk
    v[:, 225 * 7] = 5.0                                                           # ... with a value the bulk must pull away from
    qs, k, v = (t.to(td).float() for t in (q, k, v))                              # q is used pre-scaled: scores = q.k directly, in log2 units
    s = torch.einsum("bqhd,bkhd->bhqk", qs.double(), k.double())
    gap = (s[..., 225 * 7] - s[..., :225].median(-1).values).min()               # the outlier against the TYPICAL bulk key (the bulk itself spreads +- 3.5 orders)
    assert gap > orders - (1.5 if D == 40 else 2.0)                               # the construction holds for every query
    pr = torch.exp2(s - s.amax(-1, keepdim=True))
    bulk_share = 1.0 - (pr[..., 225 * 7] / pr.sum(-1)).mean().item()
    ref = torch.einsum("bhqk,bkhd->bqhd", pr / pr.sum(-1, keepdim=True), v.double()).float()
    hm = torch.stack([qs, k, v], 1).permute(0, 1, 3, 2, 4).contiguous().to(td).to(gpu)
    out = torch.empty(B, N, C, dtype=td, device=gpu)
    args = dict(B=B, heads=heads, Nkv=N, D=D, q_bs=3 * N * C, k_bs=3 * N * C, v_bs=3 * N * C, o_bs=N * C, q_rs=D, k_rs=D, v_rs=D, o_rs=C, k_off=N * C,
                v_off=2 * N * C, q_hs=N * D, k_hs=N * D, v_hs=N * D, q_prescaled=True)
    hip.attention(dt, hm, hm, hm, out, Nq=N, **args)
    got = out.float().cpu().reshape(B, N, heads, D)
    out32 = torch.empty(B, N, C, dtype=td, device=gpu)
    hip.attention(dt, hm, hm, hm, out32, Nq=640, **args)                          # Nq < 1024: the 32-queries-per-wave kernel (no own-key sample: Nq != Nkv)
    got32 = out32.float().cpu().reshape(B, N, heads, D)[:, :640]
    tol = 6 * ulp * max(1.0, ref.abs().max().item())
    e64, e32 = (got - ref).abs().max().item(), (got32 - ref[:, :640]).abs().max().item()
    print(f"attention d{D} heavy tail [{orders} orders, bulk share {bulk_share:.3f}]: max-abs {e64:.2e} (64 q / wave), {e32:.2e} (32 q / wave), tol {tol:.2e}")
    assert torch.isfinite(got).all() and e64 <= tol and e32 <= tol
