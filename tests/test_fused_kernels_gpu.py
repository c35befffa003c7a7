"""The three fused level-0 kernels (vv_spatial_chain_front_c320, vv_spatial_chain_c320, vv_motion_module_c320), called directly with streams packed from the
edge dicts of tests/fusedref.py, against the fp64 reference that rounds where the kernels round: |got - ref| <= B = ceil(4 N) u max(1, max |ref|) (N: the
reference's own rounding noise, tests/test_fusedref_cpu.py), finite, and every element of the output allocations outside the contract still a sentinel.
Then the GroupNorm statistics those kernels take their affine from, at the geometries of gn_geom no other test reaches."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fusedref as R  # noqa: E402

pytestmark = pytest.mark.gpu
REPORT = os.environ.get("VV_PARITY_REPORT")
DNAMES = ["fp16", "bf16"]
GUARD = 144          # guard rows around [M, 320] outputs: more than one 128-token block behind the last row


def _log(msg):
    print(msg)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(msg + "\n")


def _guarded(rows, width, dtype, gpu, before=GUARD, after=GUARD):
    """(sentinel-filled buffer [before + rows + after, width], the contiguous view of the middle rows)"""
    buf = torch.full((before + rows + after, width), R.SENTINEL, dtype=dtype, device=gpu)
    return buf, buf[before:before + rows]


def _guards_intact(buf, rows, before=GUARD):
    b = buf.cpu()
    return bool((b[:before] == R.SENTINEL).all()) and bool((b[before + rows:] == R.SENTINEL).all())


def _check(kind, dname, label, got, ref):
    err = (got - ref).abs().max().item()
    B = R.bound(kind, dname, ref)
    _log(f"fused {kind} [{dname}] {label}: max |got - ref| {err:.3e} = {err / B:.3f} B (B = {B:.3e}, max |ref| {ref.abs().max().item():.2f})")
    assert torch.isfinite(got).all()
    assert err <= B


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("case", range(len(R.TAIL_CASES)))
def test_tail_against_fp64(gpu, dname, case):
    from videovanish_amd import hip, packing
    td, dt = R.TD[dname], hip.dtype_id(dname)
    inp, (ref,) = R.inputs("tail", case, dname), R.reference("tail", case, dname)
    stream, prm = packing.pack_chain_stream(inp["w"], td)
    M, o_hw = inp["M"], inp["o_hw"]
    o = inp["o"].to(td)
    if o_hw:
        o = R.o_head_major(o, o_hw)
    buf, out = _guarded(M, R.C, td if inp["out16"] else torch.float32, gpu)
    res1 = inp["res1"].to(gpu) if inp["res1"] is not None else None
    ret = hip.spatial_chain_c320(dt, o.to(gpu), inp["t_in"].to(gpu), inp["x"].to(gpu), stream.to(gpu), prm.to(gpu), res1=res1, o_hw=o_hw, out=out)
    assert ret.data_ptr() == out.data_ptr()
    _check("tail", dname, str(R.TAIL_CASES[case]), out.cpu().double(), ref)
    assert _guards_intact(buf, M), "the tail stored outside its M rows"


def _front_call(hip, dt, td, gpu, inp, stream, prm, x, partials=None):
    Fr, HW = inp["F"], inp["HW"]
    M = Fr * HW
    gamma, beta, groups, eps = inp["gn"]
    tbuf, t_out = _guarded(M, R.C, torch.float32, gpu)
    qbuf = torch.full((Fr + 2, 3, 8, HW, 40), R.SENTINEL, dtype=td, device=gpu)          # a guard frame on each side
    t, qkv = hip.spatial_chain_front_c320(dt, x, gamma.to(gpu), beta.to(gpu), groups, eps, stream.to(gpu), prm.to(gpu), F=Fr, HW=HW, partials=partials,
                                          t_out=t_out, qkv_out=qbuf[1:Fr + 1])
    assert t.data_ptr() == t_out.data_ptr() and qkv.data_ptr() == qbuf[1:Fr + 1].data_ptr()
    q = qbuf.cpu()
    intact = _guards_intact(tbuf, M) and bool((q[0] == R.SENTINEL).all()) and bool((q[Fr + 1] == R.SENTINEL).all())
    return t_out.cpu().double(), q[1:Fr + 1].double(), intact


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("case", range(len(R.FRONT_CASES)))
def test_front_against_fp64(gpu, dname, case):
    from videovanish_amd import hip, packing
    td, dt = R.TD[dname], hip.dtype_id(dname)
    inp, (t_ref, qkv_ref) = R.inputs("front", case, dname), R.reference("front", case, dname)
    stream, prm = packing.pack_chain_front_stream(inp["w"], td)
    t, qkv, intact = _front_call(hip, dt, td, gpu, inp, stream, prm, inp["x"].to(gpu))
    _check("front", dname, f"{R.FRONT_CASES[case]} t", t, t_ref)
    _check("front", dname, f"{R.FRONT_CASES[case]} qkv", qkv, qkv_ref)
    assert intact, "the front stored outside t's rows or qkv's frames"


@pytest.mark.parametrize("dname", DNAMES)
def test_front_with_groupnorm_partials_from_the_producing_convolution(gpu, dname):
    """x comes out of a 3x3 convolution that leaves its GroupNorm partials (conv_gemm(gn_partials=): the 128 x 160 halo-tile kernel, 2 frames of 9 x 13, ragged patches);
    the front takes its affine from them and meets the same reference, computed from the x the convolution stored"""
    from videovanish_amd import hip, packing
    td, dt = R.TD[dname], hip.dtype_id(dname)
    Fr, H, W, cin = 2, 9, 13, 64
    g = torch.Generator().manual_seed(31)
    a = torch.randn(Fr, H, W, cin, generator=g)
    a[1] = a[1] * 2.0 + 0.5                                  # the frames' statistics differ
    wc = torch.randn(R.C, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    wp, K = packing.pack_conv(wc, td)
    parts = hip.GNPartials(Fr, H, W, R.C, gpu)
    x = hip.conv_gemm(dt, a.to(td).to(gpu), wp.to(gpu), R.C, K, F=Fr, Hin=H, Win=W, ksize=3, pad_t=1, pad_l=1, bias=torch.randn(R.C, generator=g).to(gpu),
                      out_dtype=torch.float32, gn_partials=parts)
    base = R.inputs("front", 1, dname)
    inp = dict(base, x=x.cpu(), F=Fr, HW=H * W)
    with torch.no_grad():
        t_ref, qkv_ref = R.front(inp["w"], inp["gn"], inp["x"], Fr, H * W, td)
    stream, prm = packing.pack_chain_front_stream(inp["w"], td)
    t, qkv, intact = _front_call(hip, dt, td, gpu, inp, stream, prm, x, partials=parts)
    _check("front", dname, "partials 2 x 9 x 13 t", t, t_ref)
    _check("front", dname, "partials 2 x 9 x 13 qkv", qkv, qkv_ref)
    assert intact


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("case", range(len(R.MOTION_CASES)))
def test_motion_against_fp64(gpu, dname, case):
    from videovanish_amd import hip, packing
    td, dt = R.TD[dname], hip.dtype_id(dname)
    inp, (ref,) = R.inputs("motion", case, dname), R.reference("motion", case, dname)
    stream, prm = packing.pack_motion_stream(inp["w"], td)
    Fr, HW = inp["F"], inp["HW"]
    gamma, beta, groups, eps = inp["gn"]
    # behind the clip: the rows of frames F .. 31 (where a wave's masked token rows would land) and a guard frame more
    buf, out = _guarded(Fr * HW, R.C, td if inp["out16"] else torch.float32, gpu, before=GUARD, after=(33 - Fr) * HW + GUARD)
    res1 = inp["res1"].to(gpu) if inp["res1"] is not None else None
    ret = hip.motion_module_c320(dt, inp["x"].to(gpu), stream.to(gpu), prm.to(gpu), gamma.to(gpu), beta.to(gpu), groups, eps, F=Fr, HW=HW, res1=res1, out=out)
    assert ret.data_ptr() == out.data_ptr()
    _check("motion", dname, str(R.MOTION_CASES[case]), out.cpu().double(), ref)
    assert _guards_intact(buf, Fr * HW), "the motion module stored outside the clip's frames"


def test_wrappers_refuse_outputs_of_another_shape_or_type(gpu):
    from videovanish_amd import hip, packing
    inp = R.inputs("tail", 3, "fp16")
    stream, prm = packing.pack_chain_stream(inp["w"], torch.float16)
    args = (hip.dtype_id("fp16"), inp["o"].half().to(gpu), inp["t_in"].to(gpu), inp["x"].to(gpu), stream.to(gpu), prm.to(gpu))
    with pytest.raises(RuntimeError, match="contiguous"):
        hip.spatial_chain_c320(*args, out=torch.empty((2, R.C), device=gpu))
    with pytest.raises(RuntimeError, match="contiguous"):
        hip.spatial_chain_c320(*args, out=torch.empty((1, 2 * R.C), device=gpu)[:, ::2])


# ---------------------------------------------------------------------------------------------------------------------------
# GroupNorm statistics at the geometries the fused kernels consume
def _gn_run(hip, gpu, dname, x, gamma, beta, groups, eps, Fr, HW, pool):
    """-> (fin [F, groups, 2] as vv_groupnorm_stats leaves it, fp32 output of vv_groupnorm)"""
    dt = hip.dtype_id(dname)
    Cc = x.shape[-1]
    xg, gg, bg = x.to(gpu), gamma.to(gpu), beta.to(gpu)
    _, ws = hip._gn_stats(dt, xg, gg, bg, groups, eps, Fr, HW, int(pool))
    nsplit = R.gn_geom(HW, Cc)["nsplit"]
    assert ws.numel() == Fr * (nsplit + 1) * groups * 2
    fin = ws[Fr * nsplit * groups * 2:].view(Fr, groups, 2).cpu().double()
    out = hip.groupnorm(dt, xg, gg, bg, groups, eps, F=Fr, HW=HW, pool_frames=pool, out_dtype=torch.float32)
    return fin, out.cpu().double().view(Fr, HW, Cc)


def _gn_ref(x, gamma, beta, groups, eps, Fr, HW, pool):
    Cc = x.shape[-1]
    xd = x.double().view(Fr, HW, groups, Cc // groups)
    dims = (0, 1, 3) if pool else (1, 3)
    mean = xd.mean(dim=dims, keepdim=True).expand(Fr, 1, groups, 1)
    var = xd.var(dim=dims, unbiased=False, keepdim=True).expand(Fr, 1, groups, 1)
    ref = ((xd - mean) * torch.rsqrt(var + eps)).reshape(Fr, HW, Cc) * gamma.double() + beta.double()
    return mean.reshape(Fr, groups), torch.rsqrt(var + eps).reshape(Fr, groups), ref


@pytest.mark.parametrize("case", range(len(R.GN_CASES)))
def test_groupnorm_statistics_at_fused_geometries(gpu, case, dname="fp16"):
    """x is fp32, as the fused kernels' is: the h16 type of the launch does not enter the statistics (one type is run).  Bounds: those of test_kernels_gpu.py::test_groupnorm (fp32 output: 2e-4 max(1, max |ref|)) and, for (mean, rstd), of the conv-epilogue partials test in
    test_chain_gpu.py (2e-6 max(1, |mean|) + 2e-6; 2e-5 relative)"""
    from videovanish_amd import hip
    cs = R.GN_CASES[case]
    Cc, HW, Fr, pool = cs["C"], cs["HW"], cs["F"], cs["pool"]
    g = torch.Generator().manual_seed(40 + case)
    x = torch.randn(Fr * HW, Cc, generator=g) * 2 + 0.5
    if Fr > 1:          # frames differ: per-frame and pooled statistics are not the same numbers
        x = (x.view(Fr, HW, Cc) * (1.0 + 0.1 * (torch.arange(Fr) % 5))[:, None, None] + 0.2 * (torch.arange(Fr) % 3)[:, None, None]).reshape(Fr * HW, Cc).contiguous()
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    fin, out = _gn_run(hip, gpu, dname, x, gamma, beta, 32, 1e-6, Fr, HW, pool)
    mean, rstd, ref = _gn_ref(x, gamma, beta, 32, 1e-6, Fr, HW, pool)
    e_m = (fin[..., 0] - mean).abs().max().item()
    e_r = ((fin[..., 1] - rstd).abs() / rstd).max().item()
    e_o = (out - ref).abs().max().item()
    _log(f"groupnorm statistics [{dname}] {dict((k, cs[k]) for k in ('C', 'HW', 'F', 'pool'))}: mean {e_m:.2e}, rstd rel {e_r:.2e}, output {e_o:.2e}")
    assert torch.isfinite(out).all()
    assert e_m <= 2e-6 * max(1.0, mean.abs().max().item()) + 2e-6
    assert e_r <= 2e-5
    assert e_o <= 2e-4 * max(1.0, ref.abs().max().item())


def test_groupnorm_statistics_at_mean_twenty_times_std(gpu, dname="fp16"):
    """x = 20 + N(0, 1): what fp32 (sum, sum of squares) partials can deliver, from the partial sizes of gn_geom.  C = 320, HW = 150, 2 frames: krows = 6, two splits of
    102 and 48 rows, so a thread adds at most 102 / 6 = 17 rows into its per-channel fp32 sums and one thread per group then adds krows * (C / groups) = 60 of them,
    every addition good to 2^-24 of a running sum of positive terms (x > 0 here) that never exceeds the total, and each square rounded once more:
        |ds| / s <= (17 + 60) 2^-24 = 4.6e-6,   |dq| / q <= (17 + 60 + 1) 2^-24 = 4.7e-6      (what follows is in double: vv_norm.hip gn_finalize_kernel)
    var = q / n - mean^2 with q / n = mean^2 + var = 401 var:   |dvar| / var <= 401 dq + 2 x 400 ds = 5.6e-3,   |drstd| / rstd <= half of it = 2.8e-3,
    and |dmean| <= mean ds = 9.2e-5 (in units of the std: the same).  The output (x - mean) rstd gamma + beta then moves by at most
    (max |xhat| drstd / rstd + dmean / std) max |gamma|.  The generic 2e-5 / 2e-4 of the other cases is NOT what this formulation promises here."""
    from videovanish_amd import hip
    Cc, HW, Fr = 320, 150, 2
    geom = R.gn_geom(HW, Cc)
    assert geom["krows"] == 6 and geom["rows_per_split"] == 102 and geom["nsplit"] == 2
    adds = geom["rows_per_split"] // geom["krows"] + geom["krows"] * (Cc // 32)
    ds, dq = adds * 2.0 ** -24, (adds + 1) * 2.0 ** -24
    g = torch.Generator().manual_seed(47)
    x = torch.randn(Fr * HW, Cc, generator=g) + 20.0
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    fin, out = _gn_run(hip, gpu, dname, x, gamma, beta, 32, 1e-6, Fr, HW, False)
    mean, rstd, ref = _gn_ref(x, gamma, beta, 32, 1e-6, Fr, HW, False)
    ratio2 = (mean ** 2 * rstd ** 2).max().item()                                   # mean^2 / var, about 400
    b_rstd = 0.5 * ((ratio2 + 1.0) * dq + 2.0 * ratio2 * ds)
    b_mean = mean.abs().max().item() * ds + 2.0 ** -24 * mean.abs().max().item()     # + the fp32 store of the mean
    xhat = ((x.double().view(Fr, HW, 32, 10) - mean.view(Fr, 1, 32, 1)) * rstd.view(Fr, 1, 32, 1)).abs().max().item()
    b_out = (xhat * b_rstd + b_mean * rstd.max().item()) * gamma.abs().max().item() + 1e-5 * ref.abs().max().item()      # + the apply pass's own fp32 arithmetic
    e_m = (fin[..., 0] - mean).abs().max().item()
    e_r = ((fin[..., 1] - rstd).abs() / rstd).max().item()
    e_o = (out - ref).abs().max().item()
    _log(f"groupnorm statistics [{dname}] mean / std = 20: mean {e_m:.2e} (bound {b_mean:.2e}), rstd rel {e_r:.2e} (bound {b_rstd:.2e}), output {e_o:.2e} (bound {b_out:.2e})")
    assert 2.5e-3 <= b_rstd <= 3.2e-3
    assert torch.isfinite(out).all()
    assert e_m <= b_mean and e_r <= b_rstd and e_o <= b_out


@pytest.mark.parametrize("dname", DNAMES)
def test_comparison_sees_a_mispacked_bias_and_the_mutant_models_it(gpu, dname):
    """the kernel run on a stream packed from a dict whose ff1.b of one 16-unit group comes from the chunk behind it: the comparison above fails by more than 2 B, and the
    result is the reference's own `ff1_bias_next_chunk` mutant to within B -- the mutants of tests/test_fusedref_cpu.py model what a wrong kernel would compute"""
    from videovanish_amd import hip, packing
    td, dt = R.TD[dname], hip.dtype_id(dname)
    case = 1
    inp, (ref,) = R.inputs("tail", case, dname), R.reference("tail", case, dname)
    w = dict(inp["w"])
    b1 = w["ff1.b"].clone()
    for base in (0, 4 * R.C):
        b1[base + 16 * R.G1:base + 16 * R.G1 + 16] = w["ff1.b"][base + 16 * R.G1 + 64:base + 16 * R.G1 + 80]
    w["ff1.b"] = b1
    stream, prm = packing.pack_chain_stream(w, td)
    got = hip.spatial_chain_c320(dt, inp["o"].to(td).to(gpu), inp["t_in"].to(gpu), inp["x"].to(gpu), stream.to(gpu), prm.to(gpu), res1=inp["res1"].to(gpu)).cpu().double()
    with torch.no_grad():
        (mut,) = R.run("tail", inp, td, True, "ff1_bias_next_chunk")
    B = R.bound("tail", dname, ref)
    assert (got - ref).abs().max().item() >= 2.0 * B
    assert (got - mut).abs().max().item() <= B
