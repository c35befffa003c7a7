"""The stages of ProPainter's recurrent flow-completion network (videovanish_amd/flowcomplete.py: input + downsample, the two P3D encoders, the dilated middle, one
second-order deformable alignment, the bidirectional propagation, the decoder, and complete() as a whole), built once per type on the seeded weights at the shipped
width (32, 64, 128) with 16 deformable groups and run each on the reference's input for that stage, against the fp64 references of tests/fcref.py that round where
the product rounds: every output element finite and within B = MARGIN u max(1, max |ref|) (+ u max |ref| for an h16 output; MARGIN = ceil(4 N), N the reference's own
rounding noise: tests/test_fcref_cpu.py).  Every vv_conv_gemm launch of a stage is compared, argument by argument, with the launch table of fcref, and its route with
what hip.conv_gemm_route answers for the table's shapes: the routes tests/test_fcref_cpu.py lists are the ones that ran."""
import contextlib
import copy
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fcref as R  # noqa: E402

pytestmark = pytest.mark.gpu
REPORT = os.environ.get("VV_PARITY_REPORT")
DNAMES = ["fp16", "bf16"]
NCASE = len(R.CASES)
DEVICE = "cuda:0"


def _log(msg):
    print(msg)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(msg + "\n")


@contextlib.contextmanager
def _launches():
    """every hip.conv_gemm call inside the block as (its arguments in the form of fcref's launch table, the route hip.conv_gemm_route gives the same arguments)"""
    from videovanish_amd import hip
    orig, seen = hip.conv_gemm, []

    def recording(*args, **kw):
        if not kw.get("_route"):          # (hip.conv_gemm_route itself goes through hip.conv_gemm)
            seen.append((R.describe_call(args, kw), hip.conv_gemm_route(*args, **kw)))
        return orig(*args, **kw)
    hip.conv_gemm = recording
    try:
        yield seen
    finally:
        hip.conv_gemm = orig


@functools.lru_cache(maxsize=None)
def _net(dname):
    from videovanish_amd import nn
    from videovanish_amd.flowcomplete import FlowCompleteNet
    return FlowCompleteNet(nn.Ctx(DEVICE, dname, R.SEED))          # the defaults flowprop._flow_net builds: width (32, 64, 128), 16 groups


def _run_product(stage, case, dname, inp, net=None, align=None):
    """one stage of the product on the fp32 inputs `inp` of the reference -> (out on the device, [(launch, route)])"""
    cs, dev = R.CASES[case], torch.device(DEVICE)
    net = _net(dname) if net is None else net
    T, H, W = cs["T"], cs["H"], cs["W"]
    H8, W8 = H // 8, W // 8
    d = lambda z: z.contiguous().to(dev)
    h = lambda z: z.contiguous().to(dev).to(net.ctx.h16)          # h16 inputs: the reference's values are h16 values, the conversion is exact
    with _launches() as seen:
        if stage == "down":
            out = net.input_stage(d(inp["flow"]), d(inp["mask"]))
        elif stage == "encoder1":
            out = net.encoder1(h(inp["x"]), T, H // 2, W // 2)
        elif stage == "encoder2":
            out = net.encoder2(h(inp["x"]), T, H // 4, W // 4)
        elif stage == "mid_dilation":
            out = net.middle(h(inp["x"]), T, H8, W8)
        elif stage == "alignment":
            al = net.prop.align["forward_"] if align is None else align
            prop, cur, n2 = d(inp["prop"]), d(inp["cur"]), d(inp["n2"])
            out = torch.cat([al(torch.cat([prop, z], 1), torch.cat([prop, cur, z], 1), H8, W8) for z in (torch.zeros_like(n2), n2)], 0)
        elif stage == "propagation":
            out = net.prop(d(inp["x"]), T, H8, W8)
        elif stage == "decoder":
            out = net.decoder(d(inp["prop"]), h(inp["e1"]), T, H, W)
        elif stage == "complete":
            out = net.complete(d(inp["flow"]), d(inp["mask"]))
        else:
            raise KeyError(stage)
        torch.cuda.synchronize()
    return out, seen


def _h16_inputs_are_exact(stage, inp, td):
    for k in {"encoder1": ("x",), "encoder2": ("x",), "mid_dilation": ("x",), "decoder": ("e1",)}.get(stage, ()):
        assert torch.equal(inp[k].to(td).float(), inp[k])


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("case", range(NCASE))
@pytest.mark.parametrize("stage", R.STAGES)
def test_stage_against_fp64(gpu, stage, case, dname):
    from videovanish_amd import hip
    cs = R.CASES[case]
    T, H, W = cs["T"], cs["H"], cs["W"]
    ref, _ = R.reference(stage, case, dname)
    inp = R.stage_inputs(case, dname)[stage]
    _h16_inputs_are_exact(stage, inp, R.TD[dname])
    out, seen = _run_product(stage, case, dname, inp)
    assert out.dtype == (R.TD[dname] if stage in R.H16_OUT else torch.float32)
    got = out.float().cpu().double()
    assert got.shape == ref.shape
    diff = (got - ref).abs()
    err, B = diff.max().item(), R.bound(stage, dname, ref)
    _log(f"fc stage {stage} [{dname}] case {'abcd'[case]} {cs}: max |got - ref| {err:.3e} = {err / B:.3f} B (B = {B:.3e}, max |ref| {ref.abs().max().item():.2f})")
    assert torch.isfinite(got).all()
    # the launches the stage made are the launches of the table, and they took the routes the table's shapes take
    table = R.stage_launches(stage, T, H, W)
    assert len(seen) == len(table), (len(seen), len(table))
    for (call, route), row in zip(seen, table):
        assert R.launch_key(call) == R.launch_key(row), (row["layer"], call, row)
        assert route > 0 and route == R.route_of(row, dname), (row["layer"], hip.route_name(route))
    if err > B:
        frames = 2 if stage == "alignment" else T
        per = ref.shape[0] // frames
        r, c = divmod(int(diff.argmax()), ref.shape[1])
        pytest.fail(f"{err / B:.2f} B; worst element: row {r} (frame {r // per}, pixel {r % per}), channel {c}: got {got[r, c].item():.6f}, ref {ref[r, c].item():.6f}; "
                    f"{R.diagnose(stage, case, dname, got)}")


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("case", range(NCASE))
def test_bidirect_and_complete_flows(gpu, case, dname):
    """forward_bidirect_flow: both directions within the bound of `complete`, the backward one re-flipped (the reference that leaves the time flip out lies 15 B and
    more away at T = 5: tests/test_fcref_cpu.py); complete_flows: the prediction inside the holes, outside them the measured flow bit for bit"""
    net, dev = _net(dname), torch.device(DEVICE)
    fw, bw, m = R.raw_inputs(case)
    rf, rb, _, _ = R.reference_bidirect(case, dname)
    pf, pb = net.forward_bidirect_flow(fw.to(dev), bw.to(dev), m.to(dev))
    gf, gb = net.complete_flows(fw.to(dev), bw.to(dev), m.to(dev))
    torch.cuda.synchronize()
    for label, got, ref, comb, src, mk in (("forward", pf, rf, gf, fw, m[:-1]), ("backward", pb, rb, gb, bw, m[1:])):
        got, comb = got.cpu(), comb.cpu()
        assert got.shape == ref.shape == comb.shape == src.shape and torch.isfinite(got).all()
        err, B = (got.double() - ref).abs().max().item(), R.bound("complete", dname, ref)
        _log(f"fc forward_bidirect_flow {label} [{dname}] case {'abcd'[case]}: max |got - ref| {err:.3e} = {err / B:.3f} B (B = {B:.3e})")
        assert err <= B, f"{label}: {err / B:.2f} B"
        assert torch.equal(comb[mk == 0], src[mk == 0])          # outside the holes: the measured flow, untouched
        if (mk > 0).any():          # inside: the prediction (case d's second frame has no hole)
            assert (comb[mk > 0].double() - ref[mk > 0]).abs().max().item() <= B


@pytest.mark.parametrize("dname", DNAMES)
def test_comparison_sees_a_wrong_product_and_the_mutants_model_it(gpu, dname):
    """three mistakes made on purpose in the test's own copies of the product's modules -- a _SecondOrderAlignment built with the generator's max_residue = 3, the
    _TemporalConvs of encoder1 with their three packed weights in reverse order, and the dilated middle run with dilations 1, 2, 3 -- leave results at least 2 B from
    the reference and within B of the mutant of tests/fcref.py that models each: the mutants of tests/test_fcref_cpu.py are what a wrong product computes"""
    from videovanish_amd.flowcomplete import _SecondOrderAlignment
    net = _net(dname)

    def held(stage, mut, **kw):
        case = R.MUTANTS[stage][mut]
        out, _ = _run_product(stage, case, dname, R.stage_inputs(case, dname)[stage], **kw)
        ref, m = R.reference(stage, case, dname)[0], R.run_mutant(stage, mut, case, dname)
        B, got = R.bound(stage, dname, ref), out.float().cpu().double()
        d_ref, d_mut = (got - ref).abs().max().item() / B, (got - m).abs().max().item() / B
        _log(f"fc stage {stage} [{dname}] case {'abcd'[case]} made wrong ({mut}): {d_ref:.1f} B from the reference, {d_mut:.3f} B from the mutant")
        assert d_ref >= 2.0 and d_mut <= 1.0

    held("alignment", "max_residue_3", align=_SecondOrderAlignment(net.ctx, "fc.feat_prop_module.deform_align.forward_", R.WIDTH[2], R.DG, max_residue=3.0))

    wrong = copy.copy(net)
    for attr in ("e10", "e12"):
        p3d = copy.copy(getattr(net, attr))
        p3d.conv2 = copy.copy(p3d.conv2)
        p3d.conv2.w = p3d.conv2.w[::-1]
        setattr(wrong, attr, p3d)
    held("encoder1", "temporal_taps_reversed", net=wrong)
    assert net.e10.conv2.w[0] is wrong.e10.conv2.w[2] and net.e10 is not wrong.e10

    wrong = copy.copy(net)
    wrong.mid = [copy.copy(c) for c in net.mid]
    for c, dil in zip(wrong.mid, (1, 2, 3)):
        c.dil, c.zero = dil, None
    held("mid_dilation", "dilations_1_2_3", net=wrong)
    assert [c.dil for c in net.mid] == [3, 2, 1]
