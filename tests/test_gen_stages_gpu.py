"""The stages of ProPainter's inpainting generator (videovanish_amd/inpaintgen.py: encoder, feature propagation, soft split, a transformer block as a whole and as its
two halves, soft composition, decoder), built once per type on the seeded weights and run each on the reference's input for that stage, against the fp64 references
of tests/genref.py that round where the product rounds: every output element finite and within B = MARGIN u max(1, max |ref|) (MARGIN = ceil(4 N), N the
reference's own rounding noise: tests/test_genref_cpu.py), and the launches recorded through hip.PROFILE show which attention paths ran."""
import contextlib
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import genref as R  # noqa: E402

pytestmark = pytest.mark.gpu
REPORT = os.environ.get("VV_PARITY_REPORT")
DNAMES = ["fp16", "bf16"]
SLACK = 1e-4          # |a1 mag + a2 - |d|^2| of the forward-backward check: its terms are below 100 here, which fp32 evaluates to about 1e-5


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


@functools.lru_cache(maxsize=None)
def _gen(dname):
    from videovanish_amd import nn
    from videovanish_amd.inpaintgen import InpaintGenerator
    return InpaintGenerator(nn.Ctx("cuda:0", dname, R.SEED), depths=2, t_dilation=2)


@functools.lru_cache(maxsize=None)
def _prop(dname, weights):
    """the propagation module of the generator, or one built on another weight source (genref.LoudValidity)"""
    if weights is None:
        return _gen(dname).prop
    from videovanish_amd import nn
    from videovanish_amd.inpaintgen import _FeaturePropagation
    assert weights == "loud_validity"
    return _FeaturePropagation(nn.Ctx("cuda:0", dname, weights=R.LoudValidity(R.SEED)), "gen.feat_prop_module", R.C, 16)


def _exchange_corner_shifts(pp, t, parity):
    """a copy of one parity's tables whose m_k is mis-built: the top-right and bottom-left rolled key blocks take each other's shift under their own corner mask
    (exchanging the two blocks as they are would only permute the keys of a softmax)"""
    tb = pp["tabs"]
    nh, nw, L = tb["nh"], tb["nw"], R.WS[0] * R.WS[1]
    valid, e = R.rolled_valid_index(R.WS)
    k = pp["m_k"].cpu().numpy().reshape(pp["nm"], len(range(parity, t, 2)), -1).copy()
    own = k[:, :, :L]          # the window's own tokens: (frame * nh + y) * nw + x
    f, oy, ox = own // (nh * nw), (own // nw) % nh, own % nw
    start = L
    for c, (sy, sx) in enumerate(((-e[0], -e[1]), (e[0], -e[1]), (-e[0], e[1]), (e[0], e[1]))):          # the shifts with corners 1 and 2 exchanged
        sel = (valid[(valid >= c * L) & (valid < (c + 1) * L)] - c * L).numpy()
        if c in (1, 2):
            k[:, :, start:start + len(sel)] = (f[:, :, sel] * nh + (oy[:, :, sel] - sy) % nh) * nw + (ox[:, :, sel] - sx) % nw
        start += len(sel)
    return dict(pp, m_k=torch.from_numpy(np.ascontiguousarray(k.reshape(-1)).astype(np.int32)).to(pp["m_k"].device))


def _run_product(stage, case, dname, inp, gen=None, blk=None, parity=None, wrong_tables=None):
    """one stage of the product on the fp32 inputs `inp` of the reference -> (out on the device, profile keys)"""
    cs, dev = R.CASES[case], torch.device("cuda:0")
    gen = _gen(dname) if gen is None else gen
    blk = gen.blocks[0] if blk is None else blk
    H, W, h, w, fh, fw = R.dims(cs)
    t, l_t = cs["t"], cs["l_t"]
    d = lambda z: z.contiguous().to(dev)
    with _launches() as keys:
        if stage == "encoder":
            out, ho, wo = gen.encoder(d(F.pad(inp["x"], (0, 3))), t, H, W)          # gen_input's rows: five channels and three zero ones
            assert (ho, wo) == (h, w)
        elif stage == "feature_propagation":
            out = _prop(dname, cs.get("weights"))(d(inp["x"]), d(inp["ff"]), d(inp["fb"]), d(inp["masks2"]), l_t, h, w)
        elif stage == "soft_split":
            out = gen.soft_split(d(inp["x"]), t, h, w)[0]
        elif stage in ("attention_half", "ffn_half", "block"):
            zero7 = torch.zeros((t * fh * fw, 2 * 49), dtype=torch.float32, device=dev)
            x = d(inp["x"])
            if stage == "ffn_half":
                out = blk.ffn_half(x, t, fh, fw, h, w, zero7)
            else:
                m4 = R.raw_inputs(case)["m4"]
                pp = gen.window_masks(m4[:l_t].numpy(), t, fh, fw, dev)[cs["parity"] if parity is None else parity]
                if wrong_tables is not None:
                    pp = wrong_tables(pp, t, cs["parity"])
                zero4 = gen.zero4(t, pp["tabs"], dev)
                if stage == "attention_half":
                    out = blk.attention_half(x, t, pp["tabs"], pp, zero4)
                else:
                    out = blk(x, t, fh, fw, h, w, pp["tabs"], pp, zero7, zero4)
        elif stage == "soft_comp":
            out = gen.soft_comp(d(inp["tok"]), d(inp["enc"]), t, fh, fw, h, w)
        elif stage == "decoder":
            out = gen.decoder(d(inp["x"]), l_t, h, w)
        else:
            raise KeyError(stage)
        torch.cuda.synchronize()
    return out, keys


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("case", range(len(R.CASES)))
@pytest.mark.parametrize("stage", R.STAGES)
def test_stage_against_fp64(gpu, stage, case, dname):
    cs = R.CASES[case]
    ref, it = R.reference(stage, case, dname)
    out, keys = _run_product(stage, case, dname, R.stage_inputs(case, dname)[stage])
    assert out.dtype == torch.float32
    got = out.cpu().double()
    assert got.shape == ref.shape
    diff = (got - ref).abs()
    err, B = diff.max().item(), R.bound(stage, dname, ref)
    _log(f"gen stage {stage} [{dname}] case {case} {cs}: max |got - ref| {err:.3e} = {err / B:.3f} B (B = {B:.3e}, max |ref| {ref.abs().max().item():.2f})")
    assert torch.isfinite(got).all()
    if stage == "feature_propagation":          # no pixel of the reference sits on the threshold of the forward-backward check
        assert it["min |validity slack|"].item() >= SLACK
    if stage in ("attention_half", "block"):          # masked windows: queries of all frames; clean windows: frame by frame
        n_att = sum(k.startswith("attention[") for k in keys)
        masked = it["masked windows"]
        want = 2 if (cs["layout"] == "mixed" and cs["g"] != "b") else 1          # (geometry b has one window: one launch in every layout)
        assert bool(masked.any() and not masked.all()) == (want == 2)
        assert n_att == want, keys
    if err > B:
        frames = cs["l_t"] if stage in ("feature_propagation", "decoder") else cs["t"]
        per = ref.shape[0] // frames
        r, c = divmod(int(diff.argmax()), ref.shape[1])
        pytest.fail(f"{err / B:.2f} B; worst element: row {r} (frame {r // per}, {'token' if ref.shape[1] == R.HIDDEN else 'pixel'} {r % per}), channel {c}: "
                    f"got {got[r, c].item():.6f}, ref {ref[r, c].item():.6f}; {R.diagnose(stage, case, dname, got)}")


@pytest.mark.parametrize("dname", DNAMES)
def test_comparison_sees_a_wrong_product_and_the_mutants_model_it(gpu, dname):
    """three mistakes made on purpose in the test's copy of the tables and of the block -- the rolled keys of two corners built with each other's shift, the gather
    tables of the other parity (k_idx built for the wrong T_ind), and fc1 left in the published channel-major row order under a fold that reads tap-major -- leave results at least 2 B from the reference and within B of the mutant of
    tests/genref.py that models each: the mutants of tests/test_genref_cpu.py are what a wrong product computes"""
    from videovanish_amd.inpaintgen import _Linear
    gen = _gen(dname)
    td = R.TD[dname]

    def held(stage, mut, got):
        case = R.MUTANTS[stage][mut]
        ref = R.reference(stage, case, dname)[0]
        with torch.no_grad():
            m = R.run(stage, case, R.stage_inputs(case, dname)[stage], td, True, mut)[0]
        B, got = R.bound(stage, dname, ref), got.cpu().double()
        d_ref, d_mut = (got - ref).abs().max().item() / B, (got - m).abs().max().item() / B
        _log(f"gen stage {stage} [{dname}] case {case} made wrong ({mut}): {d_ref:.1f} B from the reference, {d_mut:.3f} B from the mutant")
        assert d_ref >= 2.0 and d_mut <= 1.0

    case = R.MUTANTS["attention_half"]["corners_exchanged"]
    out, _ = _run_product("attention_half", case, dname, R.stage_inputs(case, dname)["attention_half"], wrong_tables=_exchange_corner_shifts)
    held("attention_half", "corners_exchanged", out)

    case = R.MUTANTS["attention_half"]["T_ind_other_parity"]
    out, _ = _run_product("attention_half", case, dname, R.stage_inputs(case, dname)["attention_half"], parity=1 - R.CASES[case]["parity"])
    held("attention_half", "T_ind_other_parity", out)

    case = R.MUTANTS["ffn_half"]["fc1_channel_major"]
    blk = copy.copy(gen.blocks[0])
    w1, b1 = gen.ctx.src.linear("gen.transformers.transformer.0.mlp.fc1.0", R.HIDDEN, R.MLP)
    blk.fc1 = _Linear(gen.ctx, w1, b1)          # rows c * 49 + k, not permuted
    out, _ = _run_product("ffn_half", case, dname, R.stage_inputs(case, dname)["ffn_half"], blk=blk)
    held("ffn_half", "fc1_channel_major", out)
    assert gen.blocks[0].fc1 is not blk.fc1
