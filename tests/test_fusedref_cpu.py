"""tests/fusedref.py is right and its tables are sensitive (no GPU): the references tie to oracle/model_ref.py on the model's own weights, the noise floor N behind the
GPU bound B = ceil(4 N) u max(1, max |ref|) is measured here (the figures in fusedref.py fail this file when they go stale), every mutant of the kernels' structure lies
at least 2 B from the unmutated reference in both types on the case designed for it, and the packers accept the edge dicts."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fusedref as R  # noqa: E402

from videovanish_amd import hip, packing  # noqa: E402
from videovanish_amd.config import UNetConfig  # noqa: E402

C = 320


def _spatial_dicts(P, name, cfg):
    """the two dicts of nn.SpatialTransformer.__init__ (fp32 text projection instead of the h16 one the device makes)"""
    from oracle import model_ref as M
    src, b = P.src, name + ".transformer_blocks.0"
    w, f = {}, {}
    w["o1.w"], w["o1.b"] = src.linear(b + ".attn1.to_out.0", C, C)
    w["ln2.g"], w["ln2.b"] = src.norm(b + ".norm2", C)
    w["q2.w"], _ = src.linear(b + ".attn2.to_q", C, C, 1.0, False)
    text = M.text_states(P, cfg)[0]
    wk, _ = src.linear(b + ".attn2.to_k", cfg.cross_dim, C, 1.0, False)
    wv, _ = src.linear(b + ".attn2.to_v", cfg.cross_dim, C, 1.0, False)
    w["k2"], w["v2"] = (text.double() @ wk.double().t()), (text.double() @ wv.double().t())
    w["o2.w"], w["o2.b"] = src.linear(b + ".attn2.to_out.0", C, C)
    w["ln3.g"], w["ln3.b"] = src.norm(b + ".norm3", C)
    w["ff1.w"], w["ff1.b"] = src.linear(b + ".ff.net.0.proj", C, 8 * C)
    w["ff2.w"], w["ff2.b"] = src.linear(b + ".ff.net.2", 4 * C, C)
    wo, w["out.b"] = src.conv(name + ".proj_out", C, C, 1)
    w["out.w"] = wo.reshape(C, C)
    wi, f["in.b"] = src.conv(name + ".proj_in", C, C, 1)
    f["in.w"] = wi.reshape(C, C)
    f["ln1.g"], f["ln1.b"] = src.norm(b + ".norm1", C)
    wq, _ = src.linear(b + ".attn1.to_q", C, C, 1.0, False)
    wk1, _ = src.linear(b + ".attn1.to_k", C, C, 1.0, False)
    wv1, _ = src.linear(b + ".attn1.to_v", C, C, 1.0, False)
    f["qkv.w"] = torch.cat([wq.double() * hip.attention_q_scale(C // cfg.heads), wk1.double(), wv1.double()], 0)
    return f, w


def _motion_dict(P, name, cfg):
    from oracle import model_ref as M
    src, b = P.src, name + ".transformer_blocks.0"
    w = {}
    w["proj_in.w"], w["proj_in.b"] = src.linear(name + ".proj_in", C, C)
    w["proj_out.w"], w["proj_out.b"] = src.linear(name + ".proj_out", C, C)
    for a in ("attn1", "attn2"):
        for nm, key in (("q", "to_q"), ("k", "to_k"), ("v", "to_v")):
            w[f"{a}.{nm}"], _ = src.linear(f"{b}.{a}.{key}", C, C, 1.0, False)
        w[f"{a}.o"], w[f"{a}.ob"] = src.linear(f"{b}.{a}.to_out.0", C, C)
    for i in (1, 2, 3):
        w[f"ln{i}.g"], w[f"ln{i}.b"] = src.norm(f"{b}.norm{i}", C)
    w["ff1.w"], w["ff1.b"] = src.linear(b + ".ff.net.0.proj", C, 8 * C)
    w["ff2.w"], w["ff2.b"] = src.linear(b + ".ff.net.2", 4 * C, C)
    w["pe"] = M.sinusoidal_pos_emb(cfg.motion_max_seq, C)
    return w


def _rows(x):          # [F, C, H, W] -> [F * H * W, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


# fp32 noise of the oracle: a chain of about a dozen 320..1280-term fp32 dot products, LayerNorms and softmaxes, each good to a few 2^-24 sqrt(terms) of its
# operands; 2e-5 of max |ref| is 300 fp32 ulps, two orders below anything the fp64 reference could get structurally wrong
TIE = 2e-5


def test_front_core_tail_equal_the_oracle_spatial_transformer():
    from oracle import model_ref as M
    cfg = UNetConfig()
    name = "unet.down_blocks.0.attentions.0"
    P = M.Params(0)
    Fr, H, W = 2, 5, 7
    g = torch.Generator().manual_seed(23)
    x = torch.randn(Fr, C, H, W, generator=g) * 1.3 + 0.1
    with torch.no_grad():
        ref = M.spatial_transformer(P, name, x, M.text_states(P, cfg), cfg)
    f, w = _spatial_dicts(P, name, cfg)
    gn = P.src.norm(name + ".norm", C) + (cfg.groups, 1e-6)
    xr = _rows(x)
    t, qkv = R.front(f, gn, xr, Fr, H * W, torch.float32, rounded=False)
    assert qkv.shape == (Fr, 3, 8, H * W, 40)
    q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]          # [F, 8, HW, 40]; q carries 40^-1/2 log2 e
    s = q @ k.transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    o = (p @ v) / p.sum(-1, keepdim=True)
    o = o.permute(0, 2, 1, 3).reshape(Fr * H * W, C)
    out = R.tail(w, o, t, xr, None, torch.float32, rounded=False)
    err = (out - _rows(ref).double()).abs().max().item() / ref.abs().max().item()
    print(f"front -> core -> tail vs oracle spatial_transformer: rel max {err:.2e}")
    assert err <= TIE


@pytest.mark.parametrize("Fr", [32, 22, 5])
def test_motion_equals_the_oracle_motion_module(Fr):
    from oracle import model_ref as M
    cfg = UNetConfig()
    name = "unet.down_blocks.0.motion_modules.0"
    P = M.Params(0)
    H, W = 2, 4
    g = torch.Generator().manual_seed(17)
    x = torch.randn(Fr, C, H, W, generator=g) * 1.5 + 0.2
    with torch.no_grad():
        ref = M.motion_module(P, name, x, cfg)
    gn = P.src.norm(name + ".norm", C) + (cfg.groups, 1e-6)
    res1 = torch.randn(Fr * H * W, C, generator=g)
    out = R.motion(_motion_dict(P, name, cfg), gn, _rows(x), res1, Fr, H * W, torch.float32, rounded=False)
    err = (out - (_rows(ref) + res1).double()).abs().max().item() / ref.abs().max().item()
    print(f"motion vs oracle motion_module [F = {Fr}]: rel max {err:.2e}")
    assert err <= TIE


@pytest.mark.parametrize("dname", ["fp16", "bf16"])
@pytest.mark.parametrize("kind", ["front", "tail", "motion"])
def test_noise_floor_and_margin(kind, dname):
    """N of every case of the GPU table; the worst one fixes ceil(4 N), which must be the figure fusedref.py carries (and its docstring states)"""
    ns = [R.noise(kind, c, dname) for c in range(len(R.CASES[kind]))]
    worst = max(ns)
    print(f"{kind} [{dname}]: N per case {[round(n, 3) for n in ns]}, worst {worst:.3f}, ceil(4 N) = {R.margin_of(worst)}")
    assert all(torch.isfinite(o).all() for c in range(len(R.CASES[kind])) for o in R.reference(kind, c, dname))
    assert abs(worst - R.NOISE[(kind, dname)]) <= 5e-3, "the noise floor recorded in fusedref.NOISE is stale"
    assert R.margin_of(worst) == R.MARGIN[(kind, dname)]


# mutant -> index of the case (fusedref.CASES) designed for it
MUTANTS = {
    "tail": {"key76_dropped": 1, "phantom_key77": 1, "geglu_groups_swapped": 1, "value_gate_exchanged": 1, "ff1_bias_next_chunk": 1, "ln_merge_term_omitted": 1,
             "head_o_in_next_head": 1, "o_frame_offset_of_group": 6, "res1_omitted": 8, "last_row_duplicated": 1},
    "front": {"gn_affine_prev_frame": 2, "gn_affine_next_frame": 4, "token_in_next_frame_slot": 2, "planes_permuted": 1, "head_piece_off_by_one": 2,
              "ln1_merge_term_omitted": 5},
    "motion": {"key_mask_at_F_plus_1": 2, "pe_next_frame": 3, "pe_prev_frame": 2, "pe_left_out_of_ln2": 2, "gn_per_frame": 2, "geglu_groups_swapped": 2,
               "attn_weights_exchanged": 2, "d32_dropped_in_scores": 2, "d32_dropped_in_out_proj": 2},
}


@pytest.mark.parametrize("dname", ["fp16", "bf16"])
@pytest.mark.parametrize("kind,mut", [(k, m) for k in MUTANTS for m in MUTANTS[k]])
def test_mutant_is_at_least_two_bounds_away(kind, mut, dname):
    case = MUTANTS[kind][mut]
    ref = R.reference(kind, case, dname)
    with torch.no_grad():
        got = R.run(kind, R.inputs(kind, case, dname), R.TD[dname], True, mut)
    dist = max((g - a).abs().max().item() / R.bound(kind, dname, a) for g, a in zip(got, ref))
    print(f"{kind} [{dname}] mutant {mut} on case {R.CASES[kind][case]}: {dist:.1f} B")
    assert dist >= 2.0


def test_off_by_one_key_mask_is_invisible_without_a_shared_last_frame():
    """why the motion inputs make frame F - 1 share the mass: at F = 1 the extra key is a copy of the only key, and the mutant computes the same thing"""
    case = next(i for i, c in enumerate(R.MOTION_CASES) if c["F"] == 1)
    ref = R.reference("motion", case, "fp16")[0]
    got = R.run("motion", R.inputs("motion", case, "fp16"), torch.float16, True, "key_mask_at_F_plus_1")[0]
    assert (got - ref).abs().max().item() <= R.bound("motion", "fp16", ref)


def test_packers_accept_the_edge_dicts():
    for kind, pack, slabs, params in (("front", packing.pack_chain_front_stream, 100, 960), ("tail", packing.pack_chain_stream, 462, 5120),
                                      ("motion", packing.pack_motion_stream, 670, 16320)):
        for td in (torch.float16, torch.bfloat16):
            stream, prm = pack(R.inputs(kind, 0, "fp16")["w"], td)
            assert stream.shape == (slabs, 64, 64) and stream.dtype == td and prm.shape == (params,) and prm.dtype == torch.float32
            assert torch.isfinite(stream.float()).all() and torch.isfinite(prm).all()


def test_tables_hold_the_cases_the_kernels_need():
    assert {c["M"] for c in R.TAIL_CASES} >= {128, 126, 97, 1, 129, 384, 200, 648}
    assert any(c["o_hw"] == 50 and c["M"] == 200 for c in R.TAIL_CASES) and any(c["o_hw"] == 9 and c["M"] == 648 for c in R.TAIL_CASES)
    assert any(c["res1"] for c in R.TAIL_CASES) and any(not c["res1"] for c in R.TAIL_CASES)
    assert any(c["out16"] and c["M"] % 128 for c in R.TAIL_CASES) and any(c.get("big") for c in R.TAIL_CASES)
    assert {(c["F"], c["HW"]) for c in R.FRONT_CASES} >= {(72, 9), (2, 64), (3, 42), (1, 384), (5, 27), (1, 9)}
    assert {c["F"] for c in R.MOTION_CASES} >= {32, 31, 22, 17, 16, 15, 2, 1} and {c["HW"] for c in R.MOTION_CASES} == {4, 8, 20}
    assert any(c.get("big") for c in R.MOTION_CASES)
    # tail markers: each of the four marker keys is met at a 16-token and at a 32-token tile edge of a block
    for j in range(4):
        pos = [r for r in range(128) if R.tail_marker(r, 10 ** 6) == j]
        assert any(p % 32 in (0, 31) for p in pos) and any(p % 32 in (15, 16) for p in pos), (j, pos)


def test_groupnorm_nsplit_matches_the_restated_geometry():
    """vv_groupnorm_nsplit against fusedref.gn_geom (csrc/vv_norm.hip gn_geom restated), and the table's cases reach the paths they are there for"""
    for cs in R.GN_CASES + [dict(C=320, HW=14400, F=1, geom=dict(nsplit=127, rows_per_split=114)), dict(C=320, HW=150, F=2, geom=dict(nsplit=2, krows=6, rows_per_split=102))]:
        g = R.gn_geom(cs["HW"], cs["C"])
        assert hip.lib().vv_groupnorm_nsplit(cs["HW"], cs["C"]) == g["nsplit"], cs
        for k, v in cs["geom"].items():
            assert g[k] == v, (cs, k, g)
    g = R.gn_geom(13057, 320)
    assert (13057 + 101) // 102 > 128 and 13057 - (g["nsplit"] - 1) * g["rows_per_split"] == 97
    assert 32 * R.gn_geom(820, 320)["nsplit"] == 288 > 256
