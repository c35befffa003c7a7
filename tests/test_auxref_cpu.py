"""The references of tests/auxref.py checked on the CPU: each against an independent formulation (torch's functional form or the oracle's), the fp32 restatement of
every exact kernel anchored to fp64, the rounding noise N of every rounded kernel measured on the GPU test's own inputs (auxref.NOISE fails here when stale), the share
of threshold elements left out, and every indexing mutant shown to fail at the shapes the GPU test uses."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import auxref as R  # noqa: E402

F32, F64 = torch.float32, torch.float64
H16 = [("fp16", torch.float16), ("bf16", torch.bfloat16)]


# ---------------------------------------------------------------------------------------------------------------- independent formulations
def test_pool_lookup_upsample_equal_the_oracle():
    from oracle import flowprop_ref as O
    x = R.randn(1, 3, 9, 13)
    assert torch.equal(R.avgpool2(x, F64), F.avg_pool2d(x.double()[:, None], 2)[:, 0])
    for h, w in R.CORR_SIZES:
        pyr, coords = R.corr_inputs(h, w)
        assert (R.corr_lookup(pyr, coords, F32) - O.corr_lookup(pyr, coords)).abs().max().item() <= 4 * R.U[F32] * 8
    Fr, h, w = 2, 8, 12
    coords1, mask = R.convex_inputs(Fr, h, w)
    sel = torch.arange(Fr * h * w)
    mine = R.convex_upsample(coords1, mask, sel, Fr, h, w, F64)
    for f in range(Fr):
        c = coords1[f * h * w:(f + 1) * h * w].double().reshape(h, w, 2)
        grid = torch.stack(torch.meshgrid(torch.arange(h).double(), torch.arange(w).double(), indexing="ij")[::-1], dim=-1)
        flow = (c - grid).permute(2, 0, 1)[None]
        up = O.convex_upsample(flow, mask[f * h * w:(f + 1) * h * w].double().reshape(h, w, 576).permute(2, 0, 1)[None])[0].permute(1, 2, 0)      # [8h, 8w, 2]
        got = R.convex_gather(up[None], torch.arange(h * w), 1, h, w)
        assert (got - mine[f * h * w:(f + 1) * h * w]).abs().max().item() <= 1e-12 * 64


def test_consistency_and_warp_equal_the_oracle():
    from oracle import flowprop_ref as O
    d = R.flow_edge_inputs()
    v, _ = R.fb_valid(d["f_ab"], d["f_ba"], F32)
    assert torch.equal(v.bool(), O.fb_consistency(d["f_ab"].permute(2, 0, 1), d["f_ba"].permute(2, 0, 1)))
    cur, known, filled, _ = R.prop_fill(d["cur_t"], d["cur_nb"], d["known_t"], d["known_nb"], d["valid"], d["flow"], F32)
    w = O.warp_frame(d["cur_nb"].permute(2, 0, 1), d["flow"].permute(2, 0, 1)).permute(1, 2, 0)
    assert filled.sum() > 10 and torch.equal(cur[filled.bool()], w[filled.bool()]) and torch.equal(cur[~filled.bool()], d["cur_t"][~filled.bool()])
    assert torch.equal(known, d["known_t"] | filled)


def test_raw_deform_columns_equal_the_oracle():
    from oracle import deform_ref as O
    d = R.DEFORM
    x, raw, flow = R.deform_inputs()
    B, H, W, dg, K = d["B"], d["H"], d["W"], d["dg"], 9
    nchw = lambda t: t.double().reshape(B, H, W, -1).permute(0, 3, 1, 2)
    r = nchw(raw)
    o1, o2, m = torch.chunk(r, 3, dim=1)
    for fl in (flow, None):
        off = d["max_residue"] * torch.tanh(torch.cat([o1, o2], 1))
        if fl is not None:
            off = off + nchw(fl).flip(1).repeat(1, off.shape[1] // 2, 1, 1)
        col = O.deform_columns(nchw(x), off, torch.sigmoid(m), 3, 3, 1, 1, 1, dg).permute(0, 2, 3, 1).reshape(B * H * W, -1)
        assert (R.deform_raw(x, raw, fl, d["max_residue"], dg) - col).abs().max().item() <= 1e-12


def test_norms_activations_and_the_mask_path_equal_torch():
    x, g, b = R.ln_inputs(260)
    y, _ = R.layernorm_ex(x, g, b, 1e-6, R.ACT_GELU, 264)
    xd = x.double()
    z = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + float(R.cf(1e-6, F64))) * g.double() + b.double()
    assert (y[:, :260] - F.gelu(z)).abs().max().item() <= 1e-12 and bool((y[:, 260:] == 0).all())
    for a, fn in ((R.ACT_SILU, F.silu), (R.ACT_RELU, F.relu), (R.ACT_SIGMOID, torch.sigmoid), (R.ACT_GELU, F.gelu)):
        assert (R.act(x, a) - fn(xd)).abs().max().item() <= 1e-12
    pe = R.randn(3, 5, 260)
    assert (R.layernorm(x, g, b, pe, 2) - (F.layer_norm(xd, (260,), g.double(), b.double(), float(R.cf(1e-5, F64))) + pe.double().repeat_interleave(2, 0)[:9])).abs().max() <= 1e-12
    # the mask path, per output pixel from its definition: 3x3 taps of the upsampled map, stride 2, zero padding
    S, lo = 36, 10
    logits, l1, _ = R.maskdown_inputs(S, lo)
    m, _ = R.maskdown_input(logits, lo, S, False, R.MD_SCALE, R.MD_BIAS)
    mid, _ = R.maskdown_stage(m[..., None], *l1, R.MD_EPS, None)
    mp = F.pad(m, (1, 1, 1, 1))
    for oy, ox in ((0, 0), (17, 17), (5, 11)):
        acc = torch.stack([(mp[2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3] * l1[0][c, 0].double()).sum() + l1[1][c].double() for c in range(4)])
        zz = (acc - acc.mean()) / torch.sqrt(acc.var(unbiased=False) + float(R.cf(R.MD_EPS, F64))) * l1[2].double() + l1[3].double()
        assert (mid[oy * (S // 2) + ox] - F.gelu(zz)).abs().max().item() <= 1e-12
    img = R.u8_image(8, 12)
    for s2d, cpad in R.U8N:
        ref = R.u8_normalize(img, R.U8N_MEAN, R.U8N_STD, cpad, s2d)
        v = (img.double() / 255.0 - torch.tensor(R.U8N_MEAN, dtype=F32).double()) * torch.tensor([1.0 / s for s in R.U8N_STD], dtype=F32).double()
        un = F.pixel_unshuffle(v.permute(2, 0, 1)[None], s2d)[0]          # channel c * s2d^2 + dy * s2d + dx
        un = un.reshape(3, s2d * s2d, -1).permute(2, 1, 0).reshape(-1, 3 * s2d * s2d)
        assert torch.equal(ref[:, :3 * s2d * s2d], un) and bool((ref[:, 3 * s2d * s2d:] == 0).all())


def test_split_forms_rebuild_their_input():
    x = R.randn(2, 64, 8, scale=3.0)
    for _, td in H16:
        hi, lo = R.split_f32(x, 1024.0, td)
        assert (hi + lo / 1024.0 - x).abs().max().item() <= 4 * R.U[td] ** 2 * 16
        s3 = R.split3(x, td)
        assert torch.equal(s3[:, :8], hi) and torch.equal(s3[:, 16:], R.r16(hi * 2.0 ** -10, td))
        assert bool((R.split3(x.to(td), td)[:, 8:16] == 0).all())          # an h16 input is its own hi


# ---------------------------------------------------------------------------------------------------------------- exact kernels: fp32 anchored to fp64
def _anchor(f, ops):
    v32, v64 = f(F32), f(F64)
    v32, v64 = (v32, v64) if isinstance(v32, torch.Tensor) else (torch.cat([t.reshape(-1).double() for t in v32]), torch.cat([t.reshape(-1) for t in v64]))
    assert (v32.double() - v64).abs().max().item() <= 2 * ops * R.U[F32] * max(1.0, v64.abs().max().item())


def test_fp32_restatements_of_the_exact_kernels_agree_with_fp64():
    x, y, z = R.randn(1, 5000), R.randn(2, 5000), R.randn(3, 5000)
    _anchor(lambda ft: R.axpby(x, y, 0.7, -1.3, ft), 3)
    _anchor(lambda ft: R.sched_step(x, y, z, 0.8, 0.6, 0.9, 0.3, 0.2, ft), 7)
    _anchor(lambda ft: R.add_inplace(x, y, ft), 1)
    _anchor(lambda ft: R.pad_channels(x.reshape(-1, 5), 8, 0.18215, ft), 1)
    _anchor(lambda ft: R.decode_blend(R.randn(4, 3, 50, 4), torch.tensor([0.0, 0.25, 1.0]), torch.rand(3, 50, 3, generator=R.gen(5)), ft), 6)
    _anchor(lambda ft: R.window_average(R.randn(6, 3, 50), torch.tensor([1.0, 2.0, 3.0]), ft), 1)
    u8 = torch.randint(0, 256, (2, 5, 7, 3), generator=R.gen(7), dtype=torch.uint8)
    _anchor(lambda ft: R.preprocess(u8, u8[..., 0] // 128, ft), 3)
    _anchor(lambda ft: R.raft_prep(u8, ft), 3)
    _anchor(lambda ft: R.avgpool2(R.randn(8, 3, 9, 13), ft), 4)
    _anchor(lambda ft: R.raft_flow_prep(R.randn(9, 3 * 37 * 41, 2, scale=20.0), 41, 37, ft), 1)
    _anchor(lambda ft: R.add_relu(x, y, ft), 1)
    _anchor(lambda ft: R.add_flow(x.reshape(-1, 2), y.reshape(-1, 2), ft), 1)
    _anchor(lambda ft: R.clamp_f32(x, -0.5, 0.7, ft), 1)
    _anchor(lambda ft: R.add_rowvec_unless(x.reshape(-1, 8), y[:8], torch.tensor(float("nan")), ft), 1)
    d = R.flow_edge_inputs()
    _anchor(lambda ft: R.prop_fill(d["cur_t"], d["cur_nb"], d["known_t"], d["known_nb"], d["valid"], d["flow"], ft)[0], 12)      # 3 ops per tap weight and product, 3 sums
    lat = R.randn(10, 2, 5, 7, 4)
    _anchor(lambda ft: R.brushnet_input(lat, lat * 2, u8[..., 0], 5, 7, ft), 1)
    # the kernels that decide: the fp32 and the fp64 decision agree on these inputs, element by element (for fb_valid outside the marked ones, of which there are none)
    c = R.combine_inputs()
    o32, o64 = R.prop_combine(**c, ft=F32), R.prop_combine(**c, ft=F64)
    assert torch.equal(o32[0], o64[0]) and torch.equal(o32[1], o64[1])
    v32, v64 = R.fb_valid(d["f_ab"], d["f_ba"], F32), R.fb_valid(d["f_ab"], d["f_ba"], F64)
    assert torch.equal(v32[0][~v64[1]], v64[0][~v64[1]]) and 0 < int(v64[0].sum()) < v64[0].numel()
    for _, td in H16:
        _anchor(lambda ft: R.split_f32(x[:4096], 1024.0, td, ft), 1)
        _anchor(lambda ft: R.split3(x[:4096].reshape(-1, 8), td, ft), 1)


# ---------------------------------------------------------------------------------------------------------------- thresholds
def test_threshold_elements_left_out_stay_under_half_a_percent():
    """the exact kernels decide in fp32 as their restatement does, so the GPU test leaves nothing out there; this shows that the fp64 decision differs from the fp32 one
    only on marked elements, and how few those are.  The binarised mask path is compared against fp64, marked outputs left out."""
    shares = {}
    for name, d in (("edge 9 x 13", R.flow_edge_inputs()), ("random 64 x 96", R.flow_edge_inputs(64, 96, seed=171))):
        v32, _ = R.fb_valid(d["f_ab"], d["f_ba"], F32)
        v64, near = R.fb_valid(d["f_ab"], d["f_ba"], F64)
        assert torch.equal(v32[~near], v64[~near])
        shares[f"fb_valid {name}"] = near.float().mean().item()
        o32 = R.prop_fill(d["cur_t"], d["cur_nb"], d["known_t"], d["known_nb"], d["valid"], d["flow"], F32)
        o64 = R.prop_fill(d["cur_t"], d["cur_nb"], d["known_t"], d["known_nb"], d["valid"], d["flow"], F64)
        assert torch.equal(o32[2][~o64[3]], o64[2][~o64[3]])
        shares[f"prop_fill {name}"] = o64[3].float().mean().item()
    for S, lo in R.MASKDOWN:
        logits, _, _ = R.maskdown_inputs(S, lo)
        m32, _ = R.maskdown_input(logits, lo, S, True, R.MD_SCALE, R.MD_BIAS, F32)
        m64, near = R.maskdown_input(logits, lo, S, True, R.MD_SCALE, R.MD_BIAS, F64)
        assert torch.equal(m32.double()[~near], m64[~near])
        assert 0.1 < (m64 > 0).float().mean().item() < 0.9, "the blob must cross 0 inside the map"
        shares[f"maskdown binarise S={S}"] = R.near_outputs(near).float().mean().item()
        shares[f"mask_mem_input binarise S={S}"] = R.mask_mem_input(logits, True, R.MD_SCALE, R.MD_BIAS)[1].float().mean().item()
    for ai, au, thresh, stable in R.SELECT_CASES:
        m = R.sam_select_inputs(1003, ai, au, 0.05)
        s32, near = R.sam_select(m, torch.tensor([0.1, 0.3, 0.9, 0.2]), 1.0, False, 0.05, thresh, F32)
        s64, _ = R.sam_select(m, torch.tensor([0.1, 0.3, 0.9, 0.2]), 1.0, False, 0.05, thresh, F64)
        assert torch.equal(s32, s64) and int(s32[0]) == (0 if stable else 2)
        shares[f"sam_select {ai} / {au} >= {thresh}"] = near.float().mean().item()
    for k, v in shares.items():
        print(f"threshold elements left out, {k}: {100 * v:.3f} %")
        assert v <= 0.005


# ---------------------------------------------------------------------------------------------------------------- noise
def _h(v32, v64, td):
    return R.noise_of(R.r16(v32, td), R.r16(v64, td), td)


def measure_noise():
    N = {}

    def put(key, out, v):
        k = f"{key}:{out}"
        N[k] = max(N.get(k, 0.0), v)

    x = R.silu_inputs()
    put("silu", "fp32", R.noise_of(R.silu(x, F32), R.silu(x, F64), F32))
    cn, h, q = R.raft_rows(3, 300)
    n32, n64 = R.raft_ctx_split(cn, F32), R.raft_ctx_split(cn, F64)
    put("ctx_split", "fp32", R.noise_of(n32[0], n64[0], F32))
    put("gru_update", "fp32", R.noise_of(R.gru_update(cn, q, h, F32), R.gru_update(cn, q, h, F64), F32))
    c1, mk = R.convex_inputs(2, 8, 12)
    sel = torch.arange(c1.shape[0])
    put("convex_upsample", "fp32", R.noise_of(R.convex_upsample(c1, mk, sel, 2, 8, 12, F32), R.convex_upsample(c1, mk, sel, 2, 8, 12, F64), F32))
    dx, raw, fl = R.deform_inputs()
    img = R.u8_image(8, 12)
    for dn, td in H16:
        put("ctx_split", dn, max(_h(n32[0], n64[0], td), _h(n32[1], n64[1], td)))
        put("gru_rh", dn, _h(R.gru_rh(cn, h, F32), R.gru_rh(cn, h, F64), td))
        put("gru_update", dn, _h(R.gru_update(cn, q, h, F32), R.gru_update(cn, q, h, F64), td))
        for hh, ww in R.CORR_SIZES:
            pyr, co = R.corr_inputs(hh, ww)
            put("corr_lookup", dn, _h(R.corr_lookup(pyr, co, F32), R.corr_lookup(pyr, co, F64), td))
        for xin in (dx, dx.to(td)):
            put("deform_raw", dn, _h(R.deform_raw(xin, raw, fl, R.DEFORM["max_residue"], R.DEFORM["dg"], ft=F32), R.deform_raw(xin, raw, fl, R.DEFORM["max_residue"], R.DEFORM["dg"]), td))
        for s2d, cpad in R.U8N:
            put("u8_normalize", dn, _h(R.u8_normalize(img, R.U8N_MEAN, R.U8N_STD, cpad, s2d, F32), R.u8_normalize(img, R.U8N_MEAN, R.U8N_STD, cpad, s2d), td))
        for C in R.LN_C:
            xx, g, b = R.ln_inputs(C)
            pe = R.randn(C, 5, C)
            put("layernorm", dn, _h(R.layernorm(xx, g, b, pe, 2, F32), R.layernorm(xx, g, b, pe, 2), td))
        for S, lo in R.MASKDOWN:
            logits, l1, l2 = R.maskdown_inputs(S, lo)
            for binz in (True, False):
                m32, _ = R.maskdown_input(logits, lo, S, binz, R.MD_SCALE, R.MD_BIAS, F32)
                m64, near = R.maskdown_input(logits, lo, S, binz, R.MD_SCALE, R.MD_BIAS, F64)
                keep = ~R.near_outputs(near)
                if not binz:
                    put("mask_mem_sigmoid", dn, _h(m32, m64, td))
                a32, a64 = R.maskdown_stage(m32[..., None], *l1, R.MD_EPS, td, F32)[0], R.maskdown_stage(m64[..., None], *l1, R.MD_EPS, td)[0]
                put("maskdown_mid", dn, R.noise_of(a32[keep], a64[keep], td))
                mid = a64.reshape(S // 2, S // 2, 4)          # the second stage is compared from ONE mid: the kernel's own
                put("maskdown_out", dn, R.noise_of(R.maskdown_stage(mid, *l2, R.MD_EPS, td, F32)[0], R.maskdown_stage(mid, *l2, R.MD_EPS, td)[0], td))
    for C in R.LNX_C:
        for offset in (False, True):
            xx, g, b = R.ln_inputs(C, offset=offset)
            key = "layernorm_ex_offset" if offset else "layernorm_ex"
            for a in R.ACT_LIST:
                y32, y64 = R.layernorm_ex(xx, g, b, R.LNX_EPS, a, ft=F32)[0], R.layernorm_ex(xx, g, b, R.LNX_EPS, a)[0]
                put(key, "fp32", R.noise_of(y32, y64, F32))
                for dn, td in H16:
                    put(key, dn, _h(y32, y64, td))
    for n, kind in ((n, k) for n in R.ACT_N for k in R.ACT_SETS):
        xx = R.act_inputs(n, kind)
        for a in R.ACT_LIST:
            put("act", "fp32", R.noise_of(R.act(xx, a, F32), R.act(xx, a), F32))
            for dn, td in H16:
                xh = xx.to(td)
                put("act", dn, _h(R.act(xh, a, F32), R.act(xh, a), td))
    return N


def test_noise_floor():
    N = measure_noise()
    for k in sorted(N):
        print(f"N[{k}] = {N[k]:.3f}   (recorded {R.NOISE.get(k)}; bound factor ceil(4 max(1, N)) = {math.ceil(4 * max(1.0, N[k]))})")
    assert set(N) == set(R.NOISE), "auxref.NOISE does not list the kernels measured here"
    for k, v in N.items():
        assert abs(v - R.NOISE[k]) <= 0.02 + 0.02 * v, f"the noise floor recorded in auxref.NOISE[{k!r}] is stale: measured {v:.3f}"


# ---------------------------------------------------------------------------------------------------------------- mutants
def _far(got, ref, B):
    return (got.double() - ref.double()).abs().max().item() > 2 * B


def test_every_indexing_mutant_fails_at_the_tested_shapes():
    # the per-frame table of the grid-stride kernels, at the second-pass shapes (values: the frame's index, so a wrong frame is a whole unit off)
    # on the GPU test's own inputs.  i / (HW + 1) names another frame only for the first k elements of frame k (3 elements here, all before the cap), which is why the
    # GPU test compares every element and not the second pass alone; a dropped frame base shows in every later frame, the second pass included
    dec, w, acc = R.blend_inputs()
    ref, mut = R.decode_blend(dec, w, acc).reshape(-1, 3), R.decode_blend(dec, w, acc, mut="frame_index").reshape(-1, 3)
    assert int((ref != mut).any(1).sum()) == 3 and torch.equal(ref[:R.FRAME_PER], mut[:R.FRAME_PER])          # the first frame alone cannot show it
    value, count = R.window_inputs()
    ref, mut = R.window_average(value, count).reshape(-1), R.window_average(value, count, mut="frame_index").reshape(-1)
    assert int((ref != mut).sum()) == 3 and torch.equal(ref[:R.FRAME_PER], mut[:R.FRAME_PER])
    lat, cond, mask = R.brushnet_inputs()
    ref, mut = (R.brushnet_input(lat, cond, mask, R.BRUSH["Hm"], R.BRUSH["Wm"], mut=m).reshape(-1, 16) for m in (None, "frame_base"))
    assert int((ref[R.ELEM_CAP:] != mut[R.ELEM_CAP:]).sum()) > 1000 and torch.equal(ref[:R.BRUSH["H"] * R.BRUSH["W"]], mut[:R.BRUSH["H"] * R.BRUSH["W"]])
    img = R.u8_image(8, 12)
    for s2d, cpad in R.U8N:
        ref, mut = R.u8_normalize(img, R.U8N_MEAN, R.U8N_STD, cpad, s2d), R.u8_normalize(img, R.U8N_MEAN, R.U8N_STD, cpad, s2d, mut="s2d_order")
        assert torch.equal(ref, mut) if s2d == 1 else _far(mut, ref, 8 * R.U[torch.bfloat16] * ref.abs().max().item())          # s2d = 1 has no order to get wrong
    c = R.randn(9, 3 * 37 * 41, 2, scale=20.0)
    assert not torch.equal(R.raft_flow_prep(c, 41, 37, mut="frame_base"), R.raft_flow_prep(c, 41, 37))
    assert torch.equal(R.raft_flow_prep(c, 41, 37, mut="frame_base")[:37 * 41], R.raft_flow_prep(c, 41, 37)[:37 * 41]), "one grid alone cannot show a dropped frame base"
    for h, ww in R.CORR_SIZES:
        pyr, co = R.corr_inputs(h, ww)
        ref = R.corr_lookup(pyr, co)
        assert _far(R.corr_lookup(pyr, co, mut="plane_base"), ref, 8 * R.U[torch.bfloat16] * ref.abs().max().item())
    c1, mk = R.convex_inputs(2, 8, 12)
    sel = torch.arange(c1.shape[0])
    ref = R.convex_upsample(c1, mk, sel, 2, 8, 12)
    mut = R.convex_upsample(c1, mk, sel, 2, 8, 12, mut="frame_base")
    assert torch.equal(mut[:96], ref[:96]) and _far(mut[96:], ref[96:], 1e-3 * ref.abs().max().item())          # F = 1 cannot show it, F = 2 does
    x, g, b = R.ln_inputs(256)
    for cpad in (260, 508):
        assert _far(R.layernorm_ex(x, g, b, 1e-6, cpad=cpad, mut="pad_tail")[0], R.layernorm_ex(x, g, b, 1e-6, cpad=cpad)[0], 1.0)
    pe = R.randn(5, 5, 256)
    assert _far(R.layernorm(x, g, b, pe, 2, mut="frame_index"), R.layernorm(x, g, b, pe, 2), 8 * R.U[torch.bfloat16] * 8)
    dx, raw, fl = R.deform_inputs()
    ref = R.deform_raw(dx, raw, fl, 5.0, 4)
    assert _far(R.deform_raw(dx, raw, fl, 5.0, 4, mut="flow_not_flipped"), ref, 8 * R.U[torch.bfloat16] * ref.abs().max().item())


def test_dispatch_restated_for_layernorm_ex_reaches_every_form():
    forms = {R.lnx_form(C, cpad) for C in R.LNX_C for cpad, _, _ in R.lnx_cases(C)}
    assert forms == {0, 1, 3, 5, 9}
    assert all(R.lnx_form(C, C + 252) in (1, 3, 5, 9) and R.lnx_form(C, C + 256) == 0 for C in R.LNX_C if C % 4 == 0 and 64 <= C <= 2304)
    assert {a for C in R.LNX_C for _, a, _ in R.lnx_cases(C)} == set(R.ACT_LIST) and {o for C in R.LNX_C for _, _, o in R.lnx_cases(C)} == {"fp32", "h16"}
