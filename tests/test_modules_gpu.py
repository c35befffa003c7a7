"""The layer-by-layer modules of videovanish_amd/nn.py (ResBlock, SpatialTransformer, MotionModule) and vae._MidAttn, built by name on the model's seeded weights and run
once, against the fp64 references of tests/modref.py that round where the product path rounds: every output element within B = MARGIN u max(1, max |ref|)
(+ u max |ref| for an h16 output; MARGIN = ceil(4 N), N the reference's own rounding noise: tests/test_modref_cpu.py), finite, and the launches recorded
through hip.PROFILE show that the path under test is the one that ran (no fused level-0 kernel)."""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modref as R  # noqa: E402

from videovanish_amd.config import UNetConfig  # noqa: E402

pytestmark = pytest.mark.gpu
REPORT = os.environ.get("VV_PARITY_REPORT")
DNAMES = ["fp16", "bf16"]


def _log(msg):
    print(msg)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(msg + "\n")


@contextlib.contextmanager
def _launches():
    """the profile keys of every launch inside the block (hip.PROFILE: one record per kernel launch of the wrappers)"""
    from videovanish_amd import hip
    keys, prev = [], hip.PROFILE
    hip.PROFILE = []
    try:
        yield keys
    finally:
        keys.extend(r[0] for r in hip.PROFILE)
        hip.PROFILE = prev


def _ctx(dname, cs):
    from videovanish_amd import nn as vnn
    if cs.get("weights") == "big_bias":
        return vnn.Ctx("cuda:0", dname, weights=R.BigBias(0))
    return vnn.Ctx("cuda:0", dname, 0)


def _check(kind, case, dname, path, got, keys=()):
    cs, (ref, _) = R.CASES[kind][case], R.reference(kind, case, dname)
    got = got.cpu().double()
    assert got.shape == ref.shape
    diff = (got - ref).abs()
    err, B = diff.max().item(), R.bound(kind, case, dname, ref)
    desc = {k: v for k, v in cs.items() if k not in ("name", "path", "amp")}
    _log(f"module {kind} [{dname}] case {case} {desc}: path {path}, max |got - ref| {err:.3e} = {err / B:.3f} B (B = {B:.3e}, max |ref| {ref.abs().max().item():.2f})")
    assert torch.isfinite(got).all()
    assert not any("fused" in k for k in keys), f"a fused level-0 kernel ran: {sorted(set(keys))}"
    r, c = divmod(int(diff.argmax()), ref.shape[1])
    if err > B:
        pytest.fail(f"{err / B:.2f} B; worst element: row {r} (frame {r // (cs['H'] * cs['W'])}, pixel {r % (cs['H'] * cs['W'])}), channel {c}: got {got[r, c].item():.6f}, "
                    f"ref {ref[r, c].item():.6f}; {R.diagnose(kind, case, dname, got)}")


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("case", range(len(R.SPATIAL_CASES)))
def test_spatial_transformer_against_fp64(gpu, dname, case):
    from videovanish_amd import hip, nn as vnn
    cs, inp = R.SPATIAL_CASES[case], R.inputs("spatial", case, dname)
    ctx = _ctx(dname, cs)
    mod = vnn.SpatialTransformer(ctx, cs["name"], cs["C"], UNetConfig(), ctx.dev(inp["text"], ctx.h16))
    Fr, H, W = cs["F"], cs["H"], cs["W"]
    x = inp["x"].to(gpu)
    od = ctx.h16 if cs["out16"] else torch.float32
    assert vnn.SpatialTransformer.FUSED
    if cs["path"] == "width":
        assert mod.fused is None
    else:
        assert mod.fused is not None
    with _launches() as keys:
        if cs["path"] == "switch":
            vnn.SpatialTransformer.FUSED = False
            try:
                out = mod(x, Fr, H, W, out_dtype=od)
            finally:
                vnn.SpatialTransformer.FUSED = True
        else:
            if cs["path"] == "own":
                assert H * W < hip.CHAIN_FRONT_MIN_HW
            out = mod(x, Fr, H, W, out_dtype=od)
    assert out.dtype == od and sum(k == "layernorm" for k in keys) == 3
    _check("spatial", case, dname, cs["path"], out, keys)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("case", range(len(R.MOTION_CASES)))
def test_motion_module_against_fp64(gpu, dname, case):
    from videovanish_amd import nn as vnn
    cs, inp = R.MOTION_CASES[case], R.inputs("motion", case, dname)
    ctx = _ctx(dname, cs)
    mod = vnn.MotionModule(ctx, cs["name"], cs["C"], UNetConfig(), ctx.dev(R.pos_table(cs["C"])))
    Fr, H, W = cs["F"], cs["H"], cs["W"]
    x = inp["x"].to(gpu)
    if cs.get("x16"):
        x = x.to(ctx.h16)
    res1 = inp["res1"].to(gpu) if inp["res1"] is not None else None
    od = ctx.h16 if cs["out16"] else torch.float32
    assert vnn.MotionModule.FUSED and (mod.fused is None) == (cs["path"] == "width")
    if cs["path"] == "own":          # the module's own conditions send this shape down the layer path
        assert Fr < 16 or (H * W) % 4 != 0 or x.dtype != torch.float32
    with _launches() as keys:
        out = mod(x, Fr, H, W, res1=res1, out_dtype=od)
    assert out.dtype == od and sum(k == "motion:layernorm" for k in keys) == 3
    _check("motion", case, dname, cs["path"], out, keys)


def test_motion_module_refuses_a_clip_longer_than_the_positional_table(gpu):
    from videovanish_amd import nn as vnn
    ctx = vnn.Ctx("cuda:0", "fp16", 0)
    C = 640
    mod = vnn.MotionModule(ctx, R.MOTION_CASES[0]["name"], C, UNetConfig(), ctx.dev(R.pos_table(C)))
    with pytest.raises(RuntimeError, match="exceeds the positional table"):
        mod(torch.zeros((33 * 4, C), device=gpu), 33, 2, 2)


# ---------------------------------------------------------------------------------------------------------------------------
def _resblock(ctx, cs):
    from videovanish_amd import nn as vnn
    return vnn.ResBlock(ctx, cs["name"], cs["C0"] + cs["C1"], cs["cout"], R.GROUPS, cs.get("eps", 1e-5), R.TEMB if cs["temb"] else None, precise=cs.get("precise", False))


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("case", range(len(R.RES_CASES)))
def test_resblock_against_fp64(gpu, dname, case):
    from videovanish_amd import hip
    cs, inp = R.RES_CASES[case], R.inputs("resblock", case, dname)
    ctx = _ctx(dname, cs)
    blk = _resblock(ctx, cs)
    Fr, H, W, cout = cs["F"], cs["H"], cs["W"], cs["cout"]
    M = Fr * H * W
    dev = lambda t: t.to(gpu) if t is not None else None
    x0, x1, res1, st = dev(inp["x0"]), dev(inp["x1"]), dev(inp["res1"]), dev(inp["silu_temb"])
    od = ctx.h16 if cs["out16"] else torch.float32
    want_gn = cs.get("want_gn", False)
    assert (blk.short is not None) == (cs["C0"] + cs["C1"] != cout)
    kw = dict(x1=x1, res1=res1, out_dtype=od, want_gn=want_gn)
    row = st[R.TEMB_ROW:R.TEMB_ROW + 1] if st is not None else None
    with _launches() as keys:
        ret = blk(x0, Fr, H, W, silu_temb=row, **kw)
    out, gn = ret if want_gn else (ret, None)
    assert out.dtype == od
    path = "layers"
    if st is not None:          # the hoisted form: this block's row of a table made for two timesteps at once is the one-row launch bit for bit
        table = blk.temb_bias(st)
        assert table.shape == (2, cout)
        ret2 = blk(x0, Fr, H, W, silu_temb={id(blk): table[R.TEMB_ROW]}, **kw)
        assert torch.equal(ret2[0] if want_gn else ret2, out), "silu_temb as a tensor and as the hoisted dict differ"
    if want_gn:
        dt = ctx.dt
        routes = [hip.conv_gemm_route(dt, (M, cout), c.w, cout, c.K, F=Fr, Hin=H, Win=W, ksize=3, pad_t=1, pad_l=1, bias=(cout,), res0=r0, out_dtype=torch.float32,
                                      gn_partials=True) for c, r0 in ((blk.conv1, None), (blk.conv2, (M, cout)))]
        if H * W >= 2048:
            assert blk.wants_gn_partials(H, W, None, torch.float32) and gn is not None
            assert all(r > 0 and (r & ~15) == hip.ROUTE_HALO_GN for r in routes), routes
            path = "layers, " + " / ".join(hip.route_name(r) for r in routes)
            fin = gn.finalize(R.GROUPS, 1e-6).cpu().double()
            o = out.double().cpu().view(Fr, H * W, R.GROUPS, cout // R.GROUPS)
            mean, var = o.mean(dim=(1, 3)), o.var(dim=(1, 3), unbiased=False)
            e_m = (fin[..., 0] - mean).abs().max().item()
            e_r = ((fin[..., 1] - (var + 1e-6).rsqrt()).abs() / (var + 1e-6).rsqrt()).max().item()
            _log(f"module resblock [{dname}] case {case}: GroupNorm partials of the output: mean {e_m:.2e}, rstd rel {e_r:.2e}")
            assert e_m <= 2e-6 * max(1.0, mean.abs().max().item()) + 2e-6 and e_r <= 2e-5          # the bound of test_chain_gpu.py::test_groupnorm_partials_from_the_conv_epilogue
        else:
            assert not blk.wants_gn_partials(H, W, None, torch.float32) and gn is None
            path = "layers, no partials"
    _check("resblock", case, dname, path, out, keys)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("case", range(len(R.VAE_CASES)))
def test_vae_mid_attention_against_fp64(gpu, dname, case):
    from videovanish_amd import nn as vnn
    from videovanish_amd.vae import _MidAttn
    cs, inp = R.VAE_CASES[case], R.inputs("vae_attn", case, dname)
    ctx = vnn.Ctx("cuda:0", dname, 0)
    mod = _MidAttn(ctx, cs["name"], cs["C"], R.GROUPS, precise=cs["precise"])
    assert mod.attn.heads == 1 and mod.attn.precise == cs["precise"] and not mod.attn.prescale_q
    with _launches() as keys:
        out = mod(inp["x"].to(gpu), cs["F"], cs["H"], cs["W"])
    assert out.dtype == torch.float32 and ("split3" in keys or not cs["precise"]) and sum(k.startswith("attention[spatial,d512]") for k in keys) == 1
    _check("vae_attn", case, dname, "precise" if cs["precise"] else "plain", out, keys)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_comparison_sees_a_wrong_module_and_the_mutants_model_it(gpu, dname):
    """three mistakes made on purpose from outside the modules -- the text K | V halves exchanged, the two sources of a concat ResBlock passed in the other order, res1
    not passed -- leave results at least 2 B from the reference and within B of the mutant of tests/modref.py that models each: the mutants of
    tests/test_modref_cpu.py are what a wrong module computes"""
    from videovanish_amd import nn as vnn
    td = R.TD[dname]

    def held(kind, mut, got):
        case = R.MUTANTS[kind][mut]
        ref = R.reference(kind, case, dname)[0]
        with torch.no_grad():
            m = R.run(kind, case, R.inputs(kind, case, dname), td, True, mut)[0]
        B, got = R.bound(kind, case, dname, ref), got.cpu().double()
        d_ref, d_mut = (got - ref).abs().max().item() / B, (got - m).abs().max().item() / B
        _log(f"module {kind} [{dname}] case {case} made wrong ({mut}): {d_ref:.1f} B from the reference, {d_mut:.3f} B from the mutant")
        assert d_ref >= 2.0 and d_mut <= 1.0

    case = R.MUTANTS["spatial"]["cross_k_v_exchanged"]
    cs, inp = R.SPATIAL_CASES[case], R.inputs("spatial", case, dname)
    ctx = _ctx(dname, cs)
    mod = vnn.SpatialTransformer(ctx, cs["name"], cs["C"], UNetConfig(), ctx.dev(inp["text"], ctx.h16))
    C = cs["C"]
    mod.attn2.kv = torch.cat([mod.attn2.kv[:, C:], mod.attn2.kv[:, :C]], 1).contiguous()
    held("spatial", "cross_k_v_exchanged", mod(inp["x"].to(gpu), cs["F"], cs["H"], cs["W"]))

    case = R.MUTANTS["resblock"]["halves_exchanged"]
    cs, inp = R.RES_CASES[case], R.inputs("resblock", case, dname)
    blk = _resblock(_ctx(dname, cs), cs)
    held("resblock", "halves_exchanged", blk(inp["x1"].to(gpu), cs["F"], cs["H"], cs["W"], x1=inp["x0"].to(gpu), silu_temb=inp["silu_temb"][R.TEMB_ROW:R.TEMB_ROW + 1].to(gpu)))

    case = R.MUTANTS["motion"]["res1_dropped"]
    cs, inp = R.MOTION_CASES[case], R.inputs("motion", case, dname)
    ctx = _ctx(dname, cs)
    mod = vnn.MotionModule(ctx, cs["name"], cs["C"], UNetConfig(), ctx.dev(R.pos_table(cs["C"])))
    held("motion", "res1_dropped", mod(inp["x"].to(gpu), cs["F"], cs["H"], cs["W"], res1=None, out_dtype=ctx.h16))
