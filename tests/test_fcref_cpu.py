"""tests/fcref.py is right and its cases are sensitive (no GPU): with nothing rounded every stage and the composition equal the matching function of
oracle/flowcomplete_ref.py on the seeded weights; the noise floor N behind the GPU bound B = MARGIN u max(1, max |ref|) is measured here (fcref.NOISE fails this file
when it goes stale); every mutant of the network's structure lies at least 2 B from the unmutated reference in both types on the case assigned to it; and the table
of vv_conv_gemm launches of FlowCompleteNet.complete takes, at the four cases, every route it takes at 720 x 1280 (hip.conv_gemm_route: the built library, no GPU).

What the end-to-end comparison of tests/test_flowcomplete_gpu.py::test_flow_completion_matches_oracle could not see (test_mutants_against_the_end_to_end_tolerance
below: the shift of the fp32 predictions at that test's clip and width; its tolerances are 2e-3 (fp16) and 2.2e-2 (bf16) of max |ref|): see fcref.E2E_INVISIBLE."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fcref as R  # noqa: E402

from oracle import flowcomplete_ref as FC  # noqa: E402

# fp32 noise of the oracle against the float64 restatement, as derived in tests/test_genref_cpu.py: one fp32 layer with K <= 6912 terms leaves about 80 * 2^-24 of its
# size (here K <= 9 * 384), and a stage of n layers that follow one another is held to sqrt(n) * 80 * 2^-24 of max(1, max |oracle|).  Nothing of the GPU enters.
TIE_LAYER = 80 * 2.0 ** -24
DNAMES = ["fp16", "bf16"]
NCASE = len(R.CASES)


def tie_layers(stage, T):
    """fp32 layers (convolutions, the deformable sampling, interpolations) that follow one another in a stage"""
    n = dict(down=1, encoder1=4, encoder2=4, mid_dilation=3, alignment=5, decoder=9)
    n["propagation"] = 2 * T * 7 + 1          # per direction and frame: four offset convolutions, the deformable one, two of the backbone; then the fusion
    n["complete"] = sum(n.values())
    return n[stage]


def tie_bound(stage, T):
    return math.sqrt(tie_layers(stage, T)) * TIE_LAYER


def _tie(label, out, ref, bound):
    err = (out - ref.double()).abs().max().item() / max(1.0, ref.abs().max().item())
    print(f"{label} vs oracle: max err {err:.2e} of max(1, max |ref| = {ref.abs().max().item():.3g}) = {err / 2.0 ** -24:.0f} x 2^-24")
    assert out.shape == ref.shape and err <= bound, f"{label}: {err / 2.0 ** -24:.0f} x 2^-24 against {bound / 2.0 ** -24:.0f}"


def _to5(f):
    """[T, H, W, c] -> [1, T, c, H, W]"""
    return f.permute(0, 3, 1, 2)[None]


def _mask5(m):
    return (m > 0).float()[None, :, None]


# ------------------------------------------------------------------------------------------------------------------ a. the tie to the oracle
@pytest.mark.parametrize("case", range(NCASE))
def test_every_stage_equals_the_oracle_function(case):
    """each stage on its own input (the fp32 input of the rounded reference run) against the oracle function of the same layer names"""
    cs, si, P = R.CASES[case], R.stage_inputs(case, "fp16"), R.params()
    T, H, W = cs["T"], cs["H"], cs["W"]
    c1, c2, c3 = R.WIDTH
    H2, W2, H4, W4, H8, W8 = H // 2, W // 2, H // 4, W // 4, H // 8, W // 8
    cthw = lambda r, hh, ww: r.view(T, hh, ww, -1).permute(3, 0, 1, 2)[None].contiguous()          # rows -> [1, C, T, H, W]
    rows5 = lambda z: z[0].permute(1, 2, 3, 0).reshape(-1, z.shape[1])
    nchw = lambda r, n, hh, ww: r.view(n, hh, ww, -1).permute(0, 3, 1, 2).contiguous()
    rows = lambda z: z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])
    ref = lambda st: R.run(st, case, si[st], torch.float32, rounded=False)[0]
    lr = lambda z: F.leaky_relu(z, 0.2)
    with torch.no_grad():
        d = si["down"]
        m = (d["mask"] > 0).float()[..., None]
        inp = torch.cat([d["flow"] * (1 - m), m], -1).permute(3, 0, 1, 2)[None]
        _tie("down", ref("down"), rows5(lr(FC.conv_1kk(P, "fc.downsample.0", inp, c1, 5, 2, 2, replicate=True))), tie_bound("down", T))
        x = cthw(si["encoder1"]["x"], H2, W2)
        e1 = lr(FC.p3d(P, "fc.encoder1.2", lr(FC.p3d(P, "fc.encoder1.0", x, c1, 1)), c2, 2))
        _tie("encoder1", ref("encoder1"), rows5(e1), tie_bound("encoder1", T))
        x = cthw(si["encoder2"]["x"], H4, W4)
        _tie("encoder2", ref("encoder2"), rows5(lr(FC.p3d(P, "fc.encoder2.2", lr(FC.p3d(P, "fc.encoder2.0", x, c2, 1)), c3, 2))), tie_bound("encoder2", T))
        x = cthw(si["mid_dilation"]["x"], H8, W8)
        for i, dil in enumerate((3, 2, 1)):
            x = lr(FC.conv_1kk(P, f"fc.mid_dilation.{2 * i}", x, c3, 3, 1, dil, dil))
        _tie("mid_dilation", ref("mid_dilation"), rows5(x), tie_bound("mid_dilation", T))
        a = si["alignment"]
        pr, cur, n2 = (nchw(a[k], 1, H8, W8) for k in ("prop", "cur", "n2"))
        an = "fc.feat_prop_module.deform_align.forward_"
        outs = [FC.second_order_alignment(P, an, torch.cat([pr, z], 1), torch.cat([pr, cur, z], 1), c3, R.DG) for z in (torch.zeros_like(n2), n2)]
        _tie("alignment", ref("alignment"), torch.cat([rows(o) for o in outs], 0), tie_bound("alignment", T))
        x = si["propagation"]["x"].view(T, H8, W8, c3).permute(0, 3, 1, 2)[None].contiguous()          # [1, T, C, H, W]
        o = FC.bidirectional_propagation(P, "fc.feat_prop_module", x, c3, R.DG)
        _tie("propagation", ref("propagation"), rows(o[0]), tie_bound("propagation", T))
        dd = si["decoder"]
        z = lr(FC.conv2(P, "fc.decoder2.0", nchw(dd["prop"], T, H8, W8), c3))
        z = lr(FC.deconv(P, "fc.decoder2.2", z, c2)) + nchw(dd["e1"], T, H4, W4)
        z = lr(FC.deconv(P, "fc.decoder1.2", lr(FC.conv2(P, "fc.decoder1.0", z, c2)), c1))
        z = FC.deconv(P, "fc.upsample.2", lr(FC.conv2(P, "fc.upsample.0", z, c1)), 2)
        _tie("decoder", ref("decoder"), rows(z), tie_bound("decoder", T))
        o = FC.complete(P, _to5(d["flow"] * (1 - m)), _mask5(d["mask"]))
        _tie("complete", ref("complete"), rows(o[0]), tie_bound("complete", T))


@pytest.mark.parametrize("case", range(NCASE))
def test_bidirect_and_combine_equal_the_oracle(case):
    fw, bw, m = R.raw_inputs(case)
    T = R.CASES[case]["T"]
    with torch.no_grad():
        pf, pb, cf, cb = R.bidirect(R.params(), fw, bw, m, torch.float32, False)
        rf, rb = FC.forward_bidirect_flow(R.params(), _to5(fw), _to5(bw), _mask5(m))
        qf, qb = FC.combine_flow(_to5(fw), _to5(bw), rf, rb, _mask5(m))
    back = lambda t5: t5[0].permute(0, 2, 3, 1)
    for label, got, ref in (("pred fw", pf, rf), ("pred bw", pb, rb), ("combined fw", cf, qf), ("combined bw", cb, qb)):
        _tie(f"{label} case {case}", got, back(ref), tie_bound("complete", T))
    for got, src, mk in ((cf, fw, m[:-1]), (cb, bw, m[1:])):
        assert torch.equal(got[mk == 0], src.double()[mk == 0])


def test_deformable_sampling_written_out_equals_a_convolution_and_a_shift():
    """_deform_columns pinned without the operator: zero offsets and a unit mask give the 3 x 3 im2col of F.unfold; a whole-pixel offset gives the columns of the
    shifted image; a sample at -1 or at H is zero"""
    g = torch.Generator().manual_seed(5)
    C, H, W, dg = 32, 5, 7, 4
    x = torch.randn(C, H, W, generator=g, dtype=torch.float64)
    one = torch.ones(dg * 9, H, W, dtype=torch.float64)
    col = R._deform_columns(x, torch.zeros(2 * dg * 9, H, W, dtype=torch.float64), one, dg)
    want = F.unfold(x[None], 3, padding=1).view(C, 9, H, W).permute(1, 0, 2, 3)
    assert torch.equal(col, want)
    off = torch.zeros(dg, 9, 2, H, W, dtype=torch.float64)
    off[:, :, 0], off[:, :, 1] = 1.0, -2.0          # dy = 1, dx = -2
    col = R._deform_columns(x, off.view(-1, H, W), one, dg)
    shifted = torch.zeros_like(x)
    shifted[:, :H - 1, 2:] = x[:, 1:, :W - 2]          # shifted[y, x] = x[y + 1, x - 2]
    assert torch.equal(col[4], shifted)          # the centre tap; tap (ky, kx) reads the image at (y + ky, x + kx - 3)
    for k in range(9):
        ky, kx = divmod(k, 3)
        want = torch.zeros_like(x)
        want[:, :H - ky, max(3 - kx, 0):] = x[:, ky:, max(kx - 3, 0):W - 3 + kx]
        assert torch.equal(col[k], want), k
    img = torch.ones(1, 1, H, W, dtype=torch.float64)
    at = lambda py, px: R._bilinear_zero(img, torch.full((1, 1, 1, 1), py, dtype=torch.float64), torch.full((1, 1, 1, 1), px, dtype=torch.float64)).item()
    assert at(-1.0, 2.0) == 0 and at(float(H), 2.0) == 0 and at(2.0, -1.0) == 0 and at(2.0, float(W)) == 0
    assert at(-0.5, 2.0) == 0.5 and at(H - 0.75, W - 0.5) == 0.375 and at(1.5, 2.25) == 1.0


# ------------------------------------------------------------------------------------------------------------------ b. noise floors
@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("stage", R.STAGES)
def test_noise_floor_and_margin(stage, dname):
    """N of every case; the worst one per (stage, type) is the figure fcref.NOISE carries, and MARGIN follows from it"""
    ns = [R.noise(stage, i, dname) for i in range(NCASE)]
    worst = max(ns)
    print(f"{stage} [{dname}]: N per case {[round(n, 3) for n in ns]}, worst {worst:.3f}, MARGIN = {R.margin_of(worst)}")
    assert all(torch.isfinite(R.reference(stage, i, dname)[0]).all() for i in range(NCASE))
    assert abs(worst - R.NOISE[(stage, dname)]) <= 5e-3, "the noise floor recorded in fcref.NOISE is stale"
    assert R.margin_of(worst) == R.margin_of(R.NOISE[(stage, dname)])


# ------------------------------------------------------------------------------------------------------------------ c. mutants
@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("stage,mut", [(s, m) for s in R.MUTANTS for m in R.MUTANTS[s]])
def test_mutant_is_at_least_two_bounds_away(stage, mut, dname):
    case = R.MUTANTS[stage][mut]
    ref = R.reference_bidirect(case, dname)[1].reshape(-1, 2) if stage == "complete" else R.reference(stage, case, dname)[0]
    got = R.run_mutant(stage, mut, case, dname)
    dist = (got - ref).abs().max().item() / R.bound(stage, dname, ref)
    print(f"{stage} [{dname}] mutant {mut} on case {case}: {dist:.1f} B")
    assert got.shape == ref.shape and dist >= 2.0


def test_the_mutants_the_issue_names_are_all_held():
    held = {m for s in R.MUTANTS.values() for m in s}
    assert held >= {"temporal_taps_reversed", "temporal_dilation_1", "temporal_wrap", "dilations_1_2_3", "zero_padding", "mask_inverted", "cond_cur_prop_n2",
                    "prop_n2_exchanged", "raw_interleaved", "max_residue_3", "second_order_one_back", "backward_not_reversed", "forward_input_cur_prop_backward",
                    "fusion_halves_exchanged", "skip_before_lrelu", "align_corners_false", "backward_not_flipped"}
    for s, muts in R.MUTANTS.items():          # every stage-level mutant is one its stage implements
        assert s == "complete" or set(muts) <= set(R.STAGE_MUTANTS[s])


def test_cases_hold_what_the_stages_need():
    assert [(c["T"], c["H"], c["W"]) for c in R.CASES] == [(3, 64, 128), (5, 24, 40), (2, 16, 24), (1, 8, 16)]
    for i, c in enumerate(R.CASES):
        fw, bw, m = R.raw_inputs(i)
        T, H, W = c["T"], c["H"], c["W"]
        assert fw.shape == bw.shape == (T, H, W, 2) and m.shape == (T + 1, H, W) and H % 8 == 0 and W % 8 == 0
        hole = m > 0
        assert hole[0, 0, :].any() and hole[0, :, 0].any() and not hole[0].all()          # a hole on the border: the padding replicates mask = 1 and zeroed flow
        assert not hole[1].any()          # a frame without a hole
        assert hole[:-1].any() and (T == 1 or hole[1:].any())          # both directions of forward_bidirect_flow see a hole
        if i == 1:
            assert hole[2].all()          # a frame that is all hole, among the frames of both directions
        assert (fw + bw).abs().max().item() > 0          # the backward flow is no mirror image
        assert fw.abs().max().item() <= 40.0


# ------------------------------------------------------------------------------------------------------------------ d. the end-to-end comparison, judged
E2E_WIDTH, E2E_DG = (16, 32, 64), 8


def e2e_clip():
    """the clip of tests/test_flowcomplete_gpu.py::test_flow_completion_matches_oracle, _case(5, 32, 48, 3), restated"""
    T, H, W = 5, 32, 48
    g = torch.Generator().manual_seed(3)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    fw = torch.stack([torch.stack([2.0 + 0.05 * yy + 0.3 * t, -1.0 + 0.04 * xx], -1) for t in range(T - 1)]) + 0.2 * torch.randn(T - 1, H, W, 2, generator=g)
    bw = -fw + 0.1 * torch.randn(T - 1, H, W, 2, generator=g)
    m = torch.zeros(T, H, W, dtype=torch.uint8)
    for t in range(T):
        m[t, H // 4: H // 2 + 2, W // 4 + t: W // 2 + t] = 255
    return fw, bw, m


def e2e_shifts():
    """{(stage, mutant): the larger of the two directions' max |shift| / max |ref|} of the fp32 predictions at e2e_clip(); the unmutated run is first tied to the oracle"""
    fw, bw, m = e2e_clip()
    P = R.params(E2E_WIDTH)
    back = lambda t5: t5[0].permute(0, 2, 3, 1)
    with torch.no_grad():
        base = R.bidirect(P, fw, bw, m, torch.float32, False, dg=E2E_DG, width=E2E_WIDTH)[:2]
        rf, rb = FC.forward_bidirect_flow(P, _to5(fw), _to5(bw), _mask5(m), width=E2E_WIDTH, deform_groups=E2E_DG)
        for got, ref in zip(base, (rf, rb)):
            _tie("forward_bidirect_flow at the end-to-end clip", got, back(ref), tie_bound("complete", 4))
        shifts = {}
        for stage, muts in R.MUTANTS.items():
            for mut in muts:
                # (a mutant of the alignment acts inside the propagation, in every alignment call of both directions)
                got = R.bidirect(P, fw, bw, m, torch.float32, False, mut, stage_mut="propagation" if stage == "alignment" else stage, dg=E2E_DG, width=E2E_WIDTH)[:2]
                shifts[(stage, mut)] = max(((g_ - b_).abs().max() / b_.abs().max()).item() for g_, b_ in zip(got, base))
                print(f"end to end: {stage} mutant {mut}: shift {shifts[(stage, mut)]:.3e} of max |ref|")
    return shifts


def test_mutants_against_the_end_to_end_tolerance():
    """every mutant through the whole fp32 reference at the clip, width (16, 32, 64) and 8 groups of tests/test_flowcomplete_gpu.py::
    test_flow_completion_matches_oracle: the shift of the raw predictions as that test measures it, max |.| / max |ref| per direction.  A mutant whose shift is below
    the test's tolerance (2e-3 fp16, 2.2e-2 bf16) can pass it; fcref.E2E_INVISIBLE records them, and this test fails when the record goes stale."""
    shifts = e2e_shifts()
    for dname, tol in (("fp16", 2e-3), ("bf16", 2.2e-2)):
        inside = sorted(f"{s}:{m}" for (s, m), v in shifts.items() if v <= tol)
        print(f"inside the {dname} tolerance {tol}: {inside}")
        assert inside == sorted(R.E2E_INVISIBLE[dname])


# ------------------------------------------------------------------------------------------------------------------ e. routes
# A 720p clip of 16 frames: T = 15 flows of 720 x 1280.
GEO_720 = (15, 720, 1280)
# routes taken at 720p that no case can take, with the reason (none: every 720p route is reached)
UNREACHABLE = {}


def _routes(T, H, W, dname):
    """[(layer, route name)] of the launches of complete() at T flows of H x W"""
    from videovanish_amd import hip
    out = []
    for l in R.stage_launches("complete", T, H, W):
        r = R.route_of(l, dname)
        assert r > 0, (l["layer"], r, hip.lib().vv_last_error())
        out.append((l["layer"], hip.route_name(r)))
    return out


@pytest.mark.parametrize("dname", DNAMES)
def test_routes_of_720p_are_reached_by_the_cases(dname):
    """the launches of complete(), layer by layer: every route name that occurs at 720 x 1280 occurs in at least one case, and case a takes the halo loader in every
    layer that takes it at 720p"""
    big = _routes(*GEO_720, dname)
    small = [_routes(c["T"], c["H"], c["W"], dname) for c in R.CASES]
    per_layer = lambda rs: {layer: {n for l2, n in rs if l2 == layer} for layer, _ in rs}
    for layer, names in per_layer(big).items():
        print(f"{layer}: 720p {sorted(names)}; cases {[sorted(per_layer(s).get(layer, ())) for s in small]}")
    names_big = {n for _, n in big}
    names_small = {n for s in small for _, n in s}
    missing = names_big - names_small - set(UNREACHABLE)
    assert not missing, f"routes of 720p no case reaches: {sorted(missing)}"
    assert not set(UNREACHABLE) & names_small and set(UNREACHABLE) <= names_big, "UNREACHABLE is stale"
    a = per_layer(small[0])
    halo = {layer for layer, names in per_layer(big).items() if any(n.startswith("halo") for n in names)}
    assert halo, "no launch takes the halo loader at 720p"
    for layer in halo:
        assert per_layer(big)[layer] == a[layer], (layer, per_layer(big)[layer], a[layer])
    for s in small[1:]:          # cases b, c, d: ragged grids, no halo launch
        assert not any(n.startswith("halo") for _, n in s)
    # the launches differ from case to case in size only: the same layers in the same order, frame by frame of the propagation
    assert [l for l, _ in small[0]] == [l["layer"] for l in R.stage_launches("complete", 3, 64, 128)]


def test_launch_table_shape():
    """the number of launches of complete(): 1 + 2 * 8 + 3 + (2 T * 2 + 2 (T - 1) * 5 + 1) + 6"""
    for c in R.CASES:
        T = c["T"]
        assert len(R.stage_launches("complete", T, c["H"], c["W"])) == 1 + 16 + 3 + 4 * T + 10 * (T - 1) + 1 + 6
