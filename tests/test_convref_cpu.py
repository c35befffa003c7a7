"""CPU tests of tests/convref.py (the fp64 reference of vv_conv_params) pinned against torch -- F.conv2d, F.linear, F.interpolate(nearest), F.gelu --
one test per feature of the contract, so the reference is pinned by torch and not by the kernel it judges; and of vv_conv_gemm_route, the
dispatcher's own answer to "which kernel runs", on the host without a GPU over a table of launch descriptors."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convref as R  # noqa: E402

H16 = [torch.bfloat16, torch.float16]
TOL = 1e-9       # fp64 against fp64 torch: summation-order noise only


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _all(Fr, Ho, Wo):
    return torch.arange(Fr * Ho * Wo)


def _vs(ref_nchw):
    return _nhwc(ref_nchw).reshape(-1, ref_nchw.shape[1])


def _pack(w, td):
    from videovanish_amd import packing
    return packing.pack_conv(w, td)


def _close(a, b):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= TOL * max(1.0, b.abs().max().item())


def _case(seed, Fr, cin, cout, H, W, kh, kw, td, c1=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Fr, cin, H, W, generator=g).to(td)
    x1 = torch.randn(Fr, c1, H, W, generator=g).to(td) if c1 else None
    w = (torch.randn(cout, cin + c1, kh, kw, generator=g) / math.sqrt((cin + c1) * kh * kw)).to(td)
    b = torch.randn(cout, generator=g)
    return g, x, x1, w, b


@pytest.mark.parametrize("td", H16)
@pytest.mark.parametrize("k,stride,pad", [(3, 1, 1), (3, 2, 1), (3, 2, 0), (1, 1, 0), (1, 2, 0), (5, 1, 2), (7, 2, 3)])
def test_plain_conv_matches_conv2d(td, k, stride, pad):
    """k = (ky * ks + kx) * Cin + c, stride, symmetric padding, bias; the packed weight read as stored"""
    Fr, cin, cout, H, W = 2, 16, 24, 9, 11
    _, x, _, w, b = _case(1, Fr, cin, cout, H, W, k, k, td)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad)
    Ho, Wo = ref.shape[-2:]
    wp, K = _pack(w.float(), td)
    got = R.conv_rows(td, _all(Fr, Ho, Wo), _nhwc(x), wp, cout, K, F=Fr, Hin=H, Win=W, Hout=Ho, Wout=Wo, ksize=k, stride=stride, pad_t=pad, pad_l=pad,
                      bias=b)
    _close(got, _vs(ref))


@pytest.mark.parametrize("td", H16)
def test_concat_two_sources(td):
    """Cin = C0 + C1 over x0 then x1"""
    Fr, c0, c1, cout, H, W = 2, 16, 8, 32, 7, 6
    _, x, x1, w, b = _case(2, Fr, c0, cout, H, W, 3, 3, td, c1=c1)
    ref = F.conv2d(torch.cat([x, x1], 1).double(), w.double(), b.double(), padding=1)
    wp, K = _pack(w.float(), td)
    got = R.conv_rows(td, _all(Fr, H, W), _nhwc(x), wp, cout, K, x1=_nhwc(x1), F=Fr, Hin=H, Win=W, ksize=3, pad_t=1, pad_l=1, bias=b)
    _close(got, _vs(ref))


@pytest.mark.parametrize("td", H16)
@pytest.mark.parametrize("h,w,Hv,Wv", [(5, 6, 10, 12), (5, 6, 9, 11), (4, 7, 11, 13), (6, 6, 6, 13)])
def test_fused_nearest_resize(td, h, w, Hv, Wv):
    """source pixel (yv * Hin) // Hv: torch's nearest map"""
    Fr, cin, cout = 2, 16, 16
    _, x, _, wt, b = _case(3, Fr, cin, cout, h, w, 3, 3, td)
    up = F.interpolate(x.double(), size=(Hv, Wv), mode="nearest")
    ref = F.conv2d(up, wt.double(), b.double(), padding=1)
    wp, K = _pack(wt.float(), td)
    got = R.conv_rows(td, _all(Fr, Hv, Wv), _nhwc(x), wp, cout, K, F=Fr, Hin=h, Win=w, Hv=Hv, Wv=Wv, ksize=3, pad_t=1, pad_l=1, bias=b)
    _close(got, _vs(ref))


@pytest.mark.parametrize("td", H16)
@pytest.mark.parametrize("kh,kw,pt,pl", [(2, 2, 0, 0), (2, 2, 1, 1), (2, 2, 1, 0), (1, 5, 0, 2), (5, 1, 2, 0), (3, 1, 1, 0)])
def test_ksize_w_and_explicit_geometry(td, kh, kw, pt, pl):
    """ksize_w, asymmetric pad_t / pad_l with explicit Hout / Wout (bottom / right padding implied by the bounds)"""
    Fr, cin, cout, H, W = 2, 8, 16, 8, 9
    _, x, _, w, b = _case(4, Fr, cin, cout, H, W, kh, kw, td)
    Ho, Wo = H + pt - kh + 1 + (1 if pt else 0), W + pl - kw + 1 + (1 if pl else 0)      # one implied row / column of bottom / right padding where padded
    xp = F.pad(x.double(), (pl, pl, pt, pt))
    ref = F.conv2d(xp, w.double(), b.double())[..., :Ho, :Wo]
    assert ref.shape[-2:] == (Ho, Wo)
    wp, K = _pack(w.float(), td)
    got = R.conv_rows(td, _all(Fr, Ho, Wo), _nhwc(x), wp, cout, K, F=Fr, Hin=H, Win=W, Hout=Ho, Wout=Wo, ksize=kh, ksize_w=kw, pad_t=pt, pad_l=pl,
                      bias=b)
    _close(got, _vs(ref))


@pytest.mark.parametrize("td", H16)
def test_fp32_source_rounded_as_staged(td):
    """an fp32 source enters as its rounding to the operand dtype"""
    Fr, cin, cout, H, W = 1, 16, 8, 5, 5
    g = torch.Generator().manual_seed(5)
    x = torch.randn(Fr, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g).to(td)
    ref = F.conv2d(x.to(td).double(), w.double(), None, padding=1)
    wp, K = _pack(w.float(), td)
    got = R.conv_rows(td, _all(Fr, H, W), _nhwc(x), wp, cout, K, F=Fr, Hin=H, Win=W, ksize=3, pad_t=1, pad_l=1)
    _close(got, _vs(ref))
    assert (got - _vs(F.conv2d(x.double(), w.double(), None, padding=1))).abs().max().item() > 1e-6      # the rounding is really there


@pytest.mark.parametrize("td", H16)
@pytest.mark.parametrize("rdt", [torch.float32, "h16"])
def test_epilogue_order(td, rdt):
    """bias, then out_scale on (acc + bias), then rowvec[f(m)], res0, res1 (fp32 or h16, leading dimension N), RELU / LRELU last -- F.linear"""
    g = torch.Generator().manual_seed(6)
    Fr, HW, Kc, N = 3, 7, 64, 48
    M = Fr * HW
    x = torch.randn(M, Kc, generator=g).to(td)
    w = torch.randn(N, Kc, generator=g).to(td)
    b, rv = torch.randn(N, generator=g), torch.randn(Fr, N, generator=g)
    r0, r1 = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    if rdt == "h16":
        r0, r1 = r0.to(td), r1.to(td)
    from videovanish_amd import packing
    wp = packing.pack_matrix(w.float(), td)
    lin = F.linear(x.double(), w.double(), b.double())
    for act, slope in ((R.ACT_NONE, 0.0), (R.ACT_RELU, 0.0), (R.ACT_LRELU, 0.2)):
        pre = lin * 0.75 + rv.double().repeat_interleave(HW, 0) + r0.double() + r1.double()
        ref = pre if act == R.ACT_NONE else (F.relu(pre) if act == R.ACT_RELU else F.leaky_relu(pre, slope))
        got = R.conv_rows(td, torch.arange(M), x, wp, N, Kc, F=Fr, Hin=HW, Win=1, bias=b, rowvec=rv, res0=r0, res1=r1, out_scale=0.75, act=act,
                          act_slope=slope)
        _close(got, ref)


@pytest.mark.parametrize("td", H16)
def test_geglu_interleaved_exact_gelu(td):
    """GEGLU: rows interleaved in blocks of 16, value * gelu_erf(gate) -- F.linear + F.gelu(approximate='none')"""
    from videovanish_amd import packing
    g = torch.Generator().manual_seed(7)
    M, Kc, inner = 40, 64, 48
    x = torch.randn(M, Kc, generator=g).to(td)
    w = torch.randn(2 * inner, Kc, generator=g).to(td).float()
    b = torch.randn(2 * inner, generator=g)
    h = F.linear(x.double(), w.double(), b.double())
    ref = h[:, :inner] * F.gelu(h[:, inner:])
    wi, bi = packing.geglu_interleave(w, b)
    wp = packing.pack_matrix(wi, td, geglu=True)
    got = R.conv_rows(td, torch.arange(M), x, wp, 2 * inner, Kc, F=1, Hin=M, Win=1, bias=bi, epilogue=R.EPI_GEGLU)
    _close(got, ref)


def test_ldo_out_col_positions():
    """row-major store at r * ldo + out_col + n"""
    out = torch.zeros(10, 50)
    pos = R.out_positions(torch.tensor([0, 3, 9]), 16, F=1, Hin=10, Win=1, out=out, out_col=20)
    ref = torch.arange(500).reshape(10, 50)[[0, 3, 9]][:, 20:36]
    assert torch.equal(pos, ref)


@pytest.mark.parametrize("stok", [6, -6])
def test_split_heads_positions(stok):
    """head-major store of both signs of split_tokens: torch's reshape / permute of the [M][3 * heads * dim] product"""
    heads, dim = 2, 4
    N, M = 3 * heads * dim, 24
    val = torch.arange(M * N).reshape(M, N)
    if stok > 0:      # [b][token][which][head][d] -> [b][which][head][token][d]
        ref = val.reshape(M // stok, stok, 3, heads, dim).permute(0, 2, 3, 1, 4).reshape(-1)
    else:             # token-major rows m = token * B + b
        B = M // -stok
        ref = val.reshape(-stok, B, 3, heads, dim).permute(1, 2, 3, 0, 4).reshape(-1)
    pos = R.out_positions(torch.arange(M), N, F=1, Hin=M, Win=1, split_heads=heads, split_dim=dim, split_tokens=stok)
    store = torch.full((M * N,), -1, dtype=torch.int64)
    store[pos.reshape(-1)] = val.reshape(-1)
    assert torch.equal(store, ref)


@pytest.mark.parametrize("td", H16)
def test_scatter_rows_and_residual(td):
    """sc_*: a 2x2 parity launch of a convolution over the nearest-2x image lands on its parity rows; the residual is read at the same rows"""
    Fr, cin, cout, H, W = 1, 8, 16, 4, 5
    g, x, _, _, b = _case(8, Fr, cin, cout, H, W, 3, 3, td)
    w3 = torch.randint(-4, 5, (cout, cin, 3, 3), generator=g).float() / 16      # the per-phase tap sums stay exact in h16: the fp64 tolerance holds
    Hv, Wv = 2 * H, 2 * W
    res = torch.randn(Fr * Hv * Wv, cout, generator=g)
    full = F.conv2d(F.interpolate(x.double(), size=(Hv, Wv), mode="nearest"), w3.double(), b.double(), padding=1)
    full = _vs(full) + res.double()
    from videovanish_amd import packing
    got = torch.full((Fr * Hv * Wv, cout), float("nan"), dtype=torch.float64)
    for py in (0, 1):
        for px in (0, 1):
            wp, K = packing.pack_conv(packing.upconv2x_phase_weight(w3.float(), py, px), td)
            kw = dict(F=Fr, Hin=H, Win=W, Hout=H, Wout=W, ksize=2, pad_t=1 - py, pad_l=1 - px, bias=b, res1=res, scatter=(Hv, Wv, 2, 2, py, px))
            rows = _all(Fr, H, W)
            val = R.conv_rows(td, rows, _nhwc(x), wp, cout, K, **kw)
            pos = R.out_positions(rows, cout, K, ldo=cout, **kw)
            got.reshape(-1)[pos.reshape(-1)] = val.reshape(-1)
    assert not torch.isnan(got).any()
    _close(got, full)


# ----------------------------------------------------------------------------------------------------------------------------------------------
# vv_conv_gemm_route on the host: no GPU, no device pointer is dereferenced (tensors given as shapes)

def _route(**kw):
    from videovanish_amd import hip
    return hip.conv_gemm_route(hip.F16 if kw.pop("dt", "fp16") == "fp16" else hip.BF16, **kw)


def _resconv(F_, H, W, cin, cout, **kw):
    K = 9 * cin
    return dict(x0=(F_ * H * W, cin), weight=(cout, K), N=cout, K=K, F=F_, Hin=H, Win=W, ksize=3, pad_t=1, pad_l=1, bias=(cout,), **kw)


# level 2 of the UNet / BrushNet: 23 x 40 at 720p, 34 x 60 at 1080p; ResBlock conv1 (Cin -> 1280, fp32 out, temb folded into the bias) and conv2
# (1280 -> 1280, the shortcut as res0, res1 where the model passes one)
LEVEL2 = {"720p": (23, 40), "1080p": (34, 60)}
CONV1_CIN = [640, 1280, 2560, 1920]


@pytest.mark.parametrize("geo", ["720p", "1080p"])
@pytest.mark.parametrize("frames", [32, 28])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_route_level2_convs_take_the_256x320_conv_kernel(geo, frames, dt):
    from videovanish_amd import hip
    H, W = LEVEL2[geo]
    M = frames * H * W
    for cin in CONV1_CIN:
        for od in (torch.float32, torch.float16 if dt == "fp16" else torch.bfloat16):
            r = _route(dt=dt, **_resconv(frames, H, W, cin, 1280, out_dtype=od))
            assert r == hip.ROUTE_256x320_CONV, (geo, frames, cin, hip.route_name(r) if r > 0 else r)
    for res1 in (None, (M, 1280)):
        r = _route(dt=dt, **_resconv(frames, H, W, 1280, 1280, res0=(M, 1280), res1=res1))
        assert r == hip.ROUTE_256x320_CONV
    if frames == 28 and geo == "720p":
        assert M % 256 == 160       # the ragged last row tile of a 28-frame 720p clip


@pytest.mark.parametrize("geo", ["720p", "1080p"])
def test_route_level2_convs_at_two_frames_stay_on_128_rows(geo):
    from videovanish_amd import hip
    H, W = LEVEL2[geo]
    for cin in CONV1_CIN + [1280]:
        r = _route(**_resconv(2, H, W, cin, 1280))
        assert 0 < r < hip.ROUTE_256x320_LIN, hip.route_name(r)


@pytest.mark.parametrize("geo", ["720p", "1080p"])
def test_route_tile_hint_1_never_takes_a_256_row_kernel(geo):
    from videovanish_amd import hip
    H, W = LEVEL2[geo]
    for cin in CONV1_CIN:
        r = _route(tile_hint=1, **_resconv(32, H, W, cin, 1280))
        assert 0 < r < hip.ROUTE_256x320_LIN, hip.route_name(r)
    r = _route(tile_hint=1, x0=(29440, 5120), weight=(1280, 5120), N=1280, K=5120, F=1, Hin=29440, Win=1)     # a linear the 256-row kernel takes at hint 0
    assert r == hip.ROUTE_LIN + hip.ROUTE_TILE_128x160
    assert _route(x0=(29440, 5120), weight=(1280, 5120), N=1280, K=5120, F=1, Hin=29440, Win=1) == hip.ROUTE_256x320_LIN


def test_route_forced_forms_and_their_fallback():
    from videovanish_amd import hip
    kw = _resconv(2, 9, 13, 64, 1280)
    assert _route(tile_hint=2, **kw) == hip.ROUTE_256x320_CONV
    assert _route(tile_hint=3, **kw) == hip.ROUTE_256P8_CONV
    assert _route(tile_hint=4, **kw) == hip.ROUTE_256P8A_CONV
    kw = _resconv(2, 9, 13, 64, 640)
    assert _route(tile_hint=2, **kw) == hip.ROUTE_256x320_CONV
    assert _route(tile_hint=3, **kw) == hip.ROUTE_FAST9 + hip.ROUTE_TILE_128x160     # 8-phase needs N % 256 == 0: silent fallback (9 x 13: too ragged for the halo tile)
    kw = _resconv(2, 9, 13, 64, 512)
    assert _route(tile_hint=2, **kw) == hip.ROUTE_256x256_CONV
    lin = dict(x0=(300, 640), weight=(1280, 640), N=1280, K=640, F=1, Hin=300, Win=1)
    assert _route(tile_hint=2, **lin) == hip.ROUTE_256x320_LIN
    assert _route(tile_hint=3, **lin) == hip.ROUTE_256P8_LIN
    assert _route(tile_hint=2, epilogue=hip.EPI_GEGLU, **lin) == hip.ROUTE_256x256_LIN
    assert _route(tile_hint=2, **{**kw, "Hv": 18, "Wv": 26, "Hout": 18, "Wout": 26}) < hip.ROUTE_256x320_LIN       # fused resize: not eligible
    f32 = torch.empty(2 * 9 * 13, 64, dtype=torch.float32, device="meta")
    assert _route(tile_hint=2, **{**kw, "x0": f32}) == hip.ROUTE_FAST32 + hip.ROUTE_TILE_128x128                 # fp32 source: not eligible


def test_route_scatter_and_gn_partials():
    from videovanish_amd import hip
    # nn.UpConv2x parity launch (2x2, scattered store): the halo loader of the 128-row kernels, whatever tile_hint says
    up = dict(x0=(2 * 23 * 40, 1280), weight=(1280, 4 * 1280), N=1280, K=4 * 1280, F=2, Hin=23, Win=40, Hout=23, Wout=40, ksize=2, pad_t=1, pad_l=1,
              bias=(1280,), out=torch.empty(2 * 45 * 80, 1280, dtype=torch.float32, device="meta"), scatter=(45, 80, 2, 2, 0, 0))
    up32 = dict(up, x0=(2 * 32 * 64, 1280), Hin=32, Win=64, Hout=32, Wout=64, out=torch.empty(2 * 64 * 128, 1280, dtype=torch.float32, device="meta"),
                scatter=(64, 128, 2, 2, 1, 0))
    for hint in (0, 2, 3):
        assert _route(tile_hint=hint, **up) == hip.ROUTE_FAST9 + hip.ROUTE_TILE_128x160      # 23 x 40: too ragged for the 8 x 16 patches
        assert _route(tile_hint=hint, **up32) == hip.ROUTE_HALO + hip.ROUTE_TILE_128x160
    # GroupNorm partials: the 128 x 160 halo kernel, also where the 256-row kernel would run otherwise
    gn = _resconv(32, 23, 40, 640, 640, out_dtype=torch.float32)
    assert _route(gn_partials=True, **gn) == hip.ROUTE_HALO_GN
    assert _route(gn_partials=True, **_resconv(2, 64, 64, 320, 320, out_dtype=torch.float32)) == hip.ROUTE_HALO_GN
    assert _route(gn_partials=True, **{**gn, "out_dtype": torch.float16}) == -2                     # VV_E_UNSUPPORTED, as vv_conv_gemm


def test_route_of_refused_launches_is_the_launch_error(tmp_path):
    """the route query refuses exactly what vv_conv_gemm refuses, with the same code and message (without a GPU: vv_conv_gemm validates first)"""
    import ctypes
    from videovanish_amd import hip
    lib = hip.lib()
    base = _resconv(2, 9, 13, 64, 320)
    bad = [dict(base, K=100),                                                     # K != kh * kw * Cin
           dict(base, stride=3),
           dict(base, ksize=4, K=16 * 64, weight=(320, 1024)),
           dict(base, act=hip.ACT_SILU),
           dict(base, x0=(2 * 9 * 13, 60), K=540, weight=(320, 576)),           # C0 % 8
           dict(base, weight=(320, 600)),                                        # Kpad % 64
           dict(base, epilogue=hip.EPI_GEGLU, res0=(234, 320)),
           dict(base, epilogue=hip.EPI_GEGLU, out_scale=0.5),                   # GEGLU has no scale step: refused, not dropped
           dict(base, weight=(300, 576), N=300)]                                 # Npad 300: no tile
    for kw in bad:
        r = _route(**kw)
        assert r < 0, kw
        msg = lib.vv_last_error()
        # the same parameters through vv_conv_gemm itself, with null-free fake pointers it never dereferences (it refuses before any launch)
        p = hip.ConvParams()
        ctypes.memmove(ctypes.byref(p), ctypes.byref(_params(**kw)), ctypes.sizeof(p))
        assert lib.vv_conv_gemm(ctypes.byref(p), hip.F16, None) == r
        assert lib.vv_last_error() == msg


def _params(**kw):
    """the ConvParams hip.conv_gemm_route builds (pointers = 1)"""
    from videovanish_amd import hip
    seen = {}
    orig = hip.lib().vv_conv_gemm_route

    class Spy:
        def __getattr__(self, name):
            return getattr(hip.lib(), name)

        def vv_conv_gemm_route(self, pp, dt):
            seen["p"] = hip.ConvParams.from_buffer_copy(pp._obj)
            return orig(pp, dt)
    saved = hip.CORE.dll
    hip.CORE.dll = Spy()
    try:
        _route(**kw)
    finally:
        hip.CORE.dll = saved
    return seen["p"]
