"""The references of tests/aux2ref.py checked on the CPU: each against an independent formulation (torch's functional form, the oracle's, or the definition written
out), the fp32 restatement of every exact kernel anchored to fp64, the rounding noise N of every rounded kernel measured on the GPU test's own inputs (aux2ref.NOISE
fails here when stale), the share of vv_gen_compose's values left out on the reference alone, the properties the inputs are built to have (frames past the grid cap,
every kind of frame there, the hole shapes), and every indexing mutant shown to miss at the shapes the GPU test uses."""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aux2ref as R  # noqa: E402

F32, F64 = torch.float32, torch.float64
H16 = [("fp16", torch.float16), ("bf16", torch.bfloat16)]
BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------- the image inputs past the cap
def test_image_cases_put_whole_distinct_frames_of_every_kind_past_the_cap():
    T, H, W = R.CLIP["T"], R.CLIP["H"], R.CLIP["W"]
    assert R.IMAGE_CAP == 16384 * 256 and R.frames_past_cap(T, H * W) >= 2 and R.frames_past_cap(T, R.RESIZE_DST[0] * R.RESIZE_DST[1]) >= 2
    assert R.DIST_BIG_F == 8192.0
    first = T - R.frames_past_cap(T, H * W)
    for ch in (1, 3):
        m = R.clip_masks(ch)
        kinds = [int((m[t] > 0).any(-1).sum()) for t in range(first, T)]
        assert 0 in kinds and 1 in kinds and max(kinds) > 1000, kinds          # empty, one set pixel and blocks, all in the second pass
        full = [t for t in range(T) if t % 4 >= 1]
        assert len({m[t].tobytes() for t in full}) == len(full), "the non-empty frames must differ"
        # the whole-frame fill of iters < 1: the oracle fills exactly the frames that hold a set pixel
        out0 = R.collapse_dilate(m, 0)
        assert all(int(out0[t].min()) == int(out0[t].max()) == (255 if (m[t] > 0).any() else 0) for t in range(T))
    for hs, vs in R.YCC_MODES:
        y, cb, cr = R.ycc_inputs(hs, vs)
        assert len({y[t].tobytes() for t in range(T)}) == T and cb.shape == (T, (H + (1 << vs) - 1) >> vs, (W + (1 << hs) - 1) >> hs)
    for kind in ("up", "down"):
        s = R.resize_inputs(kind, 3)
        assert (s.shape[1] < R.RESIZE_DST[0]) == (kind == "up") and (s.shape[2] < R.RESIZE_DST[1]) == (kind == "up")
        assert s.shape[1] % R.RESIZE_DST[0] and R.RESIZE_DST[0] % s.shape[1], "a non-integer ratio"


def test_c_distance_transform_equals_the_numpy_oracle_on_whole_frames():
    from oracle import imageops_ref as I
    m = R.clip_masks(1, T=4, H=31, W=37, seed=5)[..., 0]
    m[3, 4:20, 6:30] = 255
    m[3, 10, 12] = 0
    mb = np.where(m > 0, 255, 0).astype(np.uint8)
    got = R.dt_frames(mb)
    for t in range(4):
        assert np.array_equal(got[t], I.distance_transform_l2_5(mb[t]))
    d = R.chamfer_dt(m, 5)
    assert set(np.unique(d[3])) >= {0.0, 1.0, 2.0, np.float32(R.DIST_BIG_F)} and float(d[d < 8000].max()) <= 5.0


def test_small_blur_case_folds_more_than_once():
    """9 x 6 is below the 11 pixels one reflection of a 10-pixel reach needs: the oracle clamps after one reflection, which is what vv_blur_compose restates"""
    inp, orig, pix, mask = R.compose_inputs(3, 9, 6)
    out = R.blur_compose(pix, orig, mask)
    assert out.shape == (3, 9, 6, 3) and 0 < int((mask > 0).sum()) < mask.size
    idx = np.abs(np.arange(6)[:, None] + np.arange(21)[None, :] - 10)          # pixel x, tap j
    assert (np.where(idx >= 6, 10 - idx, idx) < 0).any(), "one reflection must leave the image at this size"


# ---------------------------------------------------------------------------------------------------------------- independent formulations
def _nchw(x):
    return x.permute(0, 3, 1, 2)


def test_flow_completion_and_generator_helpers_equal_torch():
    flow, mask = R.fc_inputs()
    for pad in R.FC_PADS:
        mm = (mask != 0).double()
        ref = torch.cat([flow.double() * (1 - mm)[..., None], mm[..., None]], dim=-1)
        ref = F.pad(_nchw(ref), (pad,) * 4, mode="replicate").permute(0, 2, 3, 1)
        got = R.fc_input(flow, mask, pad, F64)
        assert torch.equal(got[..., :3], ref) and bool((got[..., 3:] == 0).all())
    for B, H, W, C in R.UP2_CASES:
        x = R.up2_inputs(B, H, W, C)
        ref = F.interpolate(_nchw(x.double()), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        assert (R.upsample2x(x) - ref).abs().max().item() <= 1e-12
    for T, H, W in R.DOWN4_SHAPES:
        f = R.randn(7, T, H, W, 2, scale=5.0)
        ref = F.interpolate(_nchw(f.double()), scale_factor=0.25, mode="bilinear", align_corners=False).permute(0, 2, 3, 1) / 4
        assert (R.flow_down4(f, F64) - ref).abs().max().item() <= 1e-12
    for k, s, p, h, w in R.FOLD_GEOM:
        fh, fw = R.fold_grid(k, s, p, h, w)
        x = R.fold_inputs(k, s, p, h, w, 8)
        cols = x.double().reshape(R.FOLD_B, fh * fw, k * k, 8).permute(0, 3, 2, 1).reshape(R.FOLD_B, 8 * k * k, fh * fw)          # F.fold: channel-major columns
        ref = F.fold(cols, (h, w), k, padding=p, stride=s).permute(0, 2, 3, 1).reshape(-1, 8)
        cnt = F.fold(torch.ones(1, k * k, fh * fw, dtype=F64), (h, w), k, padding=p, stride=s)[0, 0].reshape(-1).repeat(R.FOLD_B)
        assert (R.fold_patches(x, R.FOLD_B, 8, h, w, k, s, p, False, False)[0] - ref).abs().max().item() <= 1e-12
        mine = R.fold_patches(x, R.FOLD_B, 8, h, w, k, s, p, True, True)[0]
        assert (mine[cnt > 0] - F.gelu(ref[cnt > 0] / cnt[cnt > 0, None])).abs().max().item() <= 1e-12
        assert bool((mine[cnt == 0] == 0).all()) and bool(torch.isnan(ref[cnt == 0] / cnt[cnt == 0, None]).all())          # 0 by contract where F.fold / count is NaN
        assert (int((cnt == 0).sum()) > 0) == (p == 0)
    pred, ori, mask, acc = R.gen_compose_inputs(8)
    img = ((torch.tanh(pred[:, :3].double()) + 1) / 2 * 255).clamp(0, 255).to(torch.uint8)
    v = torch.where((mask != 0)[:, None], img, ori)
    assert torch.equal(R.gen_compose(pred, ori, mask, acc, True).to(torch.uint8), v)
    assert torch.equal(R.gen_compose(pred, ori, mask, acc, False).to(torch.uint8), ((acc.to(torch.int32) + v.to(torch.int32)) // 2).to(torch.uint8))
    fr = torch.randint(0, 256, (R.PIX_N, 3), generator=R.gen(3), dtype=torch.uint8)
    gi = R.gen_input(fr, mask[:R.PIX_N], ori[:R.PIX_N, 0], F64)
    assert torch.equal(gi[:, :3], fr.double() / 127.5 - 1) and torch.equal(gi[:, 3], (mask[:R.PIX_N] > 0).double()) and bool((gi[:, 5:] == 0).all())


def test_sam2_helpers_equal_torch_and_the_oracle():
    from oracle import sam2_ref
    d = R.POOL
    buf = R.pool_inputs()
    per = d["H"] * d["W"] * d["C"]
    imgs = torch.stack([buf[d["x_off"] + b * (per + d["gap"]):][:per] for b in range(d["B"])]).reshape(d["B"], d["H"], d["W"], d["C"])
    assert torch.equal(R.maxpool2x2(buf), F.max_pool2d(_nchw(imgs), 2, 2).permute(0, 2, 3, 1).reshape(-1, d["C"])) and bool((buf < 0).all())
    for c in R.ROPE_CASES:
        x, cs = R.rope_inputs(c, torch.float16)
        got = R.rope_apply(x, cs, c, None)
        rr, D, c0 = c["rows_rope"], c["D"], c["col0"]
        z = torch.view_as_complex(x.double()[:rr, c0:c0 + D].reshape(rr, D // 2, 2).contiguous()) * torch.view_as_complex(cs.double())[torch.arange(rr) % c["n_table"]]
        assert (got[:rr, c0:c0 + D] - torch.view_as_real(z).reshape(rr, D)).abs().max().item() <= 1e-12 and torch.equal(got[~R.rope_region(c)], x.double()[~R.rope_region(c)])
    k, C, H, W = 7, 24, 9, 11
    x, w, b = R.dw_inputs(k, C, H, W)
    xp = F.pad(x.double().reshape(H, W, C), (0, 0, 3, 3, 3, 3))
    ref = b.double() + sum(xp[dy:dy + H, dx:dx + W] * w.double()[:, dy, dx] for dy in range(k) for dx in range(k))
    assert (R.dwconv(x, H, W, w, b) - ref.reshape(H * W, C)).abs().max().item() <= 1e-12
    # ConvTranspose2d(k 2, s 2) = a GEMM and the pixel shuffle
    h, ww, cout, cin = R.PS["h"], R.PS["w"], R.PS["C"], 16
    xi, wt = R.randn(1, 1, cin, h, ww), R.randn(2, cin, cout, 2, 2)
    y, bias, add = R.ps_inputs()
    yy = (xi.double().permute(0, 2, 3, 1).reshape(-1, cin) @ wt.double().permute(2, 3, 1, 0).reshape(-1, cin).T).contiguous()
    ref = F.gelu(F.conv_transpose2d(xi.double(), wt.double(), bias.double(), stride=2)[0].permute(1, 2, 0).reshape(-1, cout) + add.double())
    assert (R.pixel_shuffle2(yy, bias, add, h, ww, R.ACT_GELU)[0] - ref).abs().max().item() <= 1e-12
    for Hs, Ws, Hd, Wd, C in R.RESIZE_F32:
        s = R.resize_f32_inputs(Hs, Ws, C)
        ref = F.interpolate(s.double().reshape(1, Hs, Ws, C).permute(0, 3, 1, 2), size=(Hd, Wd), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).reshape(-1, C)
        assert (R.resize_bilinear_f32(s, Hs, Ws, Hd, Wd) - ref).abs().max().item() <= 1e-12
    for D in R.PP_D:
        coords, labels, gauss, table = R.pp_inputs(D)
        assert sorted(set(labels.tolist())) == [-1, 0, 1, 2, 3] and len(labels) * D > 256
        c = (2 * ((coords.double() + 0.5) / R.PP_SIZE) - 1) @ gauss.double() * (2 * math.pi)
        ref = torch.cat([torch.sin(c), torch.cos(c)], dim=-1)
        ref[labels == -1] = 0.0
        assert (R.prompt_points(coords, labels, 1.0 / R.PP_SIZE, gauss, table) - (ref + table.double()[(labels + 1).long()])).abs().max().item() <= 1e-12
    for dim in R.SINE_DIMS:
        assert (R.sine_pe_1d(R.SINE_POS["small"], dim, ft=F32) - sam2_ref.sine_pe_1d(R.SINE_POS["small"], dim)).abs().max().item() <= 1e-5          # the oracle is fp32
        j = torch.arange(dim // 2)
        t = 10000.0 ** (2 * (j // 2).double() / (dim // 2))
        for pos in R.SINE_POS.values():
            assert (R.sine_pe_1d(pos, dim)[:, :dim // 2] - torch.sin(pos.double()[:, None] / t)).abs().max().item() <= 1e-9
        assert float(R.SINE_POS["large"].abs().max()) > 1e4 and bool((R.SINE_POS["small"] == 0).any()) and bool((R.SINE_POS["small"] < 0).any())
    masks = R.hyper_masks(*R.hyper_inputs(4))
    for sel in ([3, 1, 0], [3, 0, 0]):
        out = R.sam_pick(masks.float(), torch.tensor(sel), -1024.0)
        assert torch.equal(out, masks.float()[3]) if sel[1] else bool((out == -1024.0).all())


def test_hole_masks_hold_the_shapes_they_are_built_for():
    sp = R._spiral(15)
    assert int(sp.sum()) > 64
    from scipy import ndimage
    lab, n = ndimage.label(sp, structure=np.ones((3, 3), dtype=bool))
    assert n == 1 and int(ndimage.label(~sp, structure=np.ones((3, 3), dtype=bool))[1]) == 1          # one corridor, one wall
    for A_ in R.HOLE_AREAS:
        m = R.holes_mask(A_)
        f = R.fill_holes(m, A_)
        bg = lambda t: bool((t <= 0).all())
        filled = lambda t: bool((t == 0.1).all())
        assert bg(m[2, 2:2 + A_]) and bool((m[2, 1] > 0) & (m[2, 2 + A_] > 0)) and bool((m[1, 1:3 + A_] > 0).all()) and bool((m[3, 1:3 + A_] > 0).all())      # a closed straight snake
        assert filled(f[2, 2:2 + A_]) and bg(f[5, 2:3 + A_]) and bg(f[16:31, 2:17][torch.from_numpy(sp)])
        assert filled(f[-1:, -1:]) and (filled(f[0, 30:32]) if A_ >= 2 else bg(f[0, 30:32]))
        if A_ >= 2:
            a1 = (A_ + 1) // 2
            assert filled(f[8, 2:2 + a1]) and filled(f[9, 2 + a1:2 + A_]) and bool(m[9, 1 + a1] > 0) and bool(m[8, 2 + a1] > 0)          # joined by the diagonal alone
        assert bg(f[12, 2:2 + (A_ + 2) // 2]) and bg(f[13, 2 + (A_ + 2) // 2:3 + A_])
        assert bool((m == 0).any()) and int((f == 0.1).sum()) > 10 and int((f <= 0).sum()) > 100
    for v, A_ in ((-1.0, 8), (-1.0, 64), (0.0, 64), (1.0, 8)):
        m = torch.full((5, 7), v)
        f = R.fill_holes(m, A_)
        assert torch.equal(f, torch.full((5, 7), 0.1) if v <= 0 and A_ >= 35 else m)


# ---------------------------------------------------------------------------------------------------------------- exact kernels: fp32 anchored to fp64
def test_fp32_restatements_of_the_exact_kernels_agree_with_fp64():
    def anchor(f, ops):
        v32, v64 = f(F32), f(F64)
        assert (v32.double() - v64).abs().max().item() <= 2 * ops * R.U[F32] * max(1.0, v64.abs().max().item())

    flow, mask = R.fc_inputs()
    for pad in R.FC_PADS:
        assert torch.equal(R.fc_input(flow, mask, pad, F32).double(), R.fc_input(flow, mask, pad, F64))
    for T, H, W in R.DOWN4_SHAPES:
        f = R.randn(7, T, H, W, 2, scale=5.0)
        anchor(lambda ft: R.flow_down4(f, ft), 3)
    fr = torch.randint(0, 256, (R.PIX_N, 3), generator=R.gen(3), dtype=torch.uint8)
    m = R.mask_0_1_255(R.PIX_N, 4)
    anchor(lambda ft: R.gen_input(fr, m, m, ft), 2)
    y, bias, add = R.ps_inputs()
    for a in (R.ACT_NONE, R.ACT_RELU):
        anchor(lambda ft: R.pixel_shuffle2(y, bias, add, R.PS["h"], R.PS["w"], a, ft)[0], 2)


# ---------------------------------------------------------------------------------------------------------------- vv_gen_compose: the values left out
def test_gen_compose_leaves_out_at_most_a_thousandth_on_the_reference_alone():
    for ld in R.LD_PRED["gen_compose"]:
        pred, ori, mask, acc = R.gen_compose_inputs(ld)
        t64 = R.gen_compose_t(pred)
        band = R.bound("gen_compose:fp32", F32, t64)
        keep = R.gen_compose_keep(pred, mask, band)
        share = (~keep).float().mean().item()
        print(f"gen_compose ld {ld}: band {band:.3e}, {int((~keep).sum())} of {keep.numel()} values left out ({100 * share:.4f} %)")
        assert share <= R.GC_CAP and float(pred.abs().max()) > 10 and not bool(keep[0, 0]) and bool(keep[1:4, 0].all())          # tanh(12) rounds to 1 in fp32, not in fp64; tanh(25) is 1 in both: 255 is compared
        assert float(R.gen_compose_t(pred)[2, 0]) == 255.0 and float(R.gen_compose(pred, ori, mask, acc, True)[2, 0]) == 255.0
        assert {int(v) for v in mask.unique()} == {0, 1, 255}
        for first in (True, False):          # on the values kept, the fp32 evaluation on the CPU already agrees with fp64
            assert torch.equal(R.gen_compose(pred, ori, mask, acc, first, F32).double()[keep], R.gen_compose(pred, ori, mask, acc, first)[keep])


# ---------------------------------------------------------------------------------------------------------------- noise
def _h(v32, v64, td):
    return R.noise_of(R.r16(v32, td), R.r16(v64, td), td)


def measure_noise():
    N = {}

    def put(key, out, v):
        k = f"{key}:{out}"
        N[k] = max(N.get(k, 0.0), v)

    def both(key, f, h16=True, f32=True):
        """f(ft) -> the value; its noise as an fp32 output and as either h16 output"""
        v32, v64 = f(F32), f(F64)
        if f32:
            put(key, "fp32", R.noise_of(v32, v64, F32))
        if h16:
            for dn, td in H16:
                put(key, dn, _h(v32, v64, td))

    for B, H, W, C in R.UP2_CASES:
        x = R.up2_inputs(B, H, W, C)
        both("upsample2x", lambda ft: R.upsample2x(x, ft), h16=False)
        for dn, td in H16:
            put("upsample2x", dn, _h(R.upsample2x(x.to(td), F32), R.upsample2x(x.to(td)), td))
    for ld in R.LD_PRED["gen_compose"]:
        pred = R.gen_compose_inputs(ld)[0]
        both("gen_compose", lambda ft: R.gen_compose_t(pred, ft), h16=False)
    for k, s, p, h, w in R.FOLD_GEOM:
        for C in R.FOLD_C:
            x = R.fold_inputs(k, s, p, h, w, C)
            for nrm, gl in R.FOLD_FLAGS:
                both("fold", lambda ft: R.fold_patches(x, R.FOLD_B, C, h, w, k, s, p, nrm, gl, ft)[0])
                for dn, td in H16:
                    put("fold", dn, _h(R.fold_patches(x.to(td), R.FOLD_B, C, h, w, k, s, p, nrm, gl, F32)[0], R.fold_patches(x.to(td), R.FOLD_B, C, h, w, k, s, p, nrm, gl)[0], td))
    for c in R.ROPE_CASES:
        for dn, td in H16:
            x, cs = R.rope_inputs(c, td)
            put("rope", dn, R.noise_of(R.rope_apply(x, cs, c, td, F32), R.rope_apply(x, cs, c, td), td))
    for k, C, H, W in R.DW_CASES:
        x, w, b = R.dw_inputs(k, C, H, W)
        both("dwconv", lambda ft: R.dwconv(x, H, W, w, b, ft), h16=False)
    y, bias, add = R.ps_inputs()
    for a in R.PS_ACTS:
        for ad in (add, None):
            both("pixel_shuffle", lambda ft: R.pixel_shuffle2(y, bias, ad, R.PS["h"], R.PS["w"], a, ft)[0])
    for Hs, Ws, Hd, Wd, C in R.RESIZE_F32:
        s = R.resize_f32_inputs(Hs, Ws, C)
        both("resize_f32", lambda ft: R.resize_bilinear_f32(s, Hs, Ws, Hd, Wd, ft), h16=False)
    for D in R.PP_D:
        coords, labels, gauss, table = R.pp_inputs(D)
        both("prompt_points", lambda ft: R.prompt_points(coords, labels, 1.0 / R.PP_SIZE, gauss, table, ft), h16=False)
    for dim in R.SINE_DIMS:
        for kind, pos in R.SINE_POS.items():
            both(f"sine_pe_{kind}", lambda ft: R.sine_pe_1d(pos, dim, ft=ft), h16=False)
    for nm in R.HYPER["nms"]:
        hy, up = R.hyper_inputs(nm)
        both("hyper_masks", lambda ft: R.hyper_masks(hy, up, ft), h16=False)
    return N


def test_noise_floor():
    N = measure_noise()
    for k in sorted(N):
        print(f"N[{k}] = {N[k]:.3f}   (recorded {R.NOISE.get(k)}; bound factor ceil(4 max(1, N)) = {math.ceil(4 * max(1.0, N[k]))})")
    assert set(N) == set(R.NOISE), "aux2ref.NOISE does not list the kernels measured here"
    for k, v in N.items():
        assert abs(v - R.NOISE[k]) <= 0.02 + 0.02 * v, f"the noise floor recorded in aux2ref.NOISE[{k!r}] is stale: measured {v:.3f}"


# ---------------------------------------------------------------------------------------------------------------- mutants
def _far(got, ref, B):
    return (got.double() - ref.double()).abs().max().item() > 2 * B


def test_image_mutants_differ_past_the_cap():
    T, H, W = R.CLIP["T"], R.CLIP["H"], R.CLIP["W"]
    first = T - R.frames_past_cap(T, H * W)
    for ch in (1, 3):
        m = R.clip_masks(ch)
        ref, mut = R.collapse_dilate(m, 0), R.collapse_dilate(m, 0, mut="frame_index")
        assert (ref[first:] != mut[first:]).any() and np.array_equal(ref[0], mut[0])          # one frame alone cannot show it
        for it in (1, 2):
            assert (R.collapse_dilate(m, it)[first:] != R.collapse_dilate(m, it, mut="no_frame_edge")[first:]).any()
    f2 = T - R.frames_past_cap(T, R.RESIZE_DST[0] * R.RESIZE_DST[1])
    for kind in ("up", "down"):
        s = R.resize_inputs(kind, 1)[f2 - 1:]          # the frames of the second pass (and one before) are enough to show it
        for mode in ("bilinear", "nearest"):
            ref, mut = R.resize_u8(s, *R.RESIZE_DST, mode), R.resize_u8(s, *R.RESIZE_DST, mode, mut="frame_base")
            assert all((ref[t] != mut[t]).any() for t in range(1, len(s)))
    inp, orig, pix, mask = (a[first:] for a in R.compose_inputs())
    for Rr in (1, 5):
        assert (R.chamfer_dt(mask, Rr) != R.chamfer_dt(mask, Rr, mut="frame_base")).any()
    for fe in (0.0, 1.0, 2.5):
        assert (R.feather_composite(inp, orig, mask, fe) != R.feather_composite(inp, orig, mask, fe, mut="frame_base")).any()
    assert (R.blur_compose(pix, orig, mask) != R.blur_compose(pix, orig, mask, mut="frame_base")).any()


def test_every_indexing_mutant_misses_at_the_tested_shapes():
    flow, mask = R.fc_inputs()
    for pad in R.FC_PADS:
        assert not torch.equal(R.fc_input(flow, mask, pad), R.fc_input(flow, mask, pad, mut="frame_base"))
    for B, H, W, C in R.UP2_CASES:
        x = R.up2_inputs(B, H, W, C)
        ref = R.upsample2x(x)
        lim = R.bound("upsample2x:bf16", BF, ref)
        assert _far(R.upsample2x(x, mut="batch_out"), ref, lim) and torch.equal(R.upsample2x(x, mut="batch_out")[0], ref[0])          # B = 1 cannot show it
        assert _far(R.upsample2x(x, mut="xy_swap"), ref, lim) == (H != W)          # a square image cannot show it
    pred, fl, m = R.randn(1, R.PIX_N, 8), R.randn(2, R.PIX_N, 2), R.mask_0_1_255(R.PIX_N, 3)
    assert not torch.equal(R.flow_combine(pred, fl, m), R.flow_combine(pred, fl, m, mut="ld_min")) and torch.equal(R.flow_combine(pred[:, :2].contiguous(), fl, m, mut="ld_min"),
                                                                                                                    R.flow_combine(pred[:, :2].contiguous(), fl, m))
    pred, ori, mask, acc = R.gen_compose_inputs(8)
    for first in (True, False):
        assert _far(R.gen_compose(pred, ori, mask, acc, first, mut="ld_min"), R.gen_compose(pred, ori, mask, acc, first), 1.0)
    for td in (torch.float16, BF):
        src = R.randn(5, R.GATHER_ROWS, 24).to(td)
        idx = R.gather_idx("mixed")
        assert not torch.equal(R.gather_rows(src, idx, mut="neg_wraps"), R.gather_rows(src, idx)) and int((idx == R.GATHER_ROWS - 1).sum()) >= 2 and int((idx == 5).sum()) >= 2
        assert bool((R.gather_rows(src, R.gather_idx("all -1")) == 0).all()) and (R.GATHER_N * 3) % 256 and R.GATHER_N % 256
    for k, s, p, h, w in R.FOLD_GEOM:
        for C in R.FOLD_C:
            x = R.fold_inputs(k, s, p, h, w, C)
            for nrm, gl in R.FOLD_FLAGS:
                ref = R.fold_patches(x, R.FOLD_B, C, h, w, k, s, p, nrm, gl)[0]
                lim = R.bound("fold:bf16", BF, ref)
                for mut in ("tap_order", "fw_for_fh", "py_lo"):
                    assert _far(R.fold_patches(x, R.FOLD_B, C, h, w, k, s, p, nrm, gl, mut=mut)[0], ref, lim), (k, C, nrm, gl, mut)
    buf = R.pool_inputs()
    assert not torch.equal(R.maxpool2x2(buf, "zero_init"), R.maxpool2x2(buf)) and not torch.equal(R.maxpool2x2(buf, "batch_contig"), R.maxpool2x2(buf))
    for c in R.ROPE_CASES:
        assert c["ld"] > c["col0"] + c["D"] and c["col0"] and c["n_table"] < c["rows_rope"] < c["rows"] and c["rows_rope"] * c["D"] // 2 > 256
        for dn, td in H16:
            x, cs = R.rope_inputs(c, td)
            ref = R.rope_apply(x, cs, c, td)
            for mut in ("swap", "no_wrap", "dense"):
                assert _far(R.rope_apply(x, cs, c, td, mut=mut), ref, R.bound(f"rope:{dn}", td, ref)), (c["D"], dn, mut)
    for k, C, H, W in R.DW_CASES:
        x, w, b = R.dw_inputs(k, C, H, W)
        ref = R.dwconv(x, H, W, w, b)
        for mut in ("w_layout", "xy_swap"):
            assert _far(R.dwconv(x, H, W, w, b, mut=mut), ref, R.bound("dwconv:fp32", F32, ref)), (k, C, H, W, mut)
    y, bias, add = R.ps_inputs()
    for a in R.PS_ACTS:
        ref = R.pixel_shuffle2(y, bias, add, R.PS["h"], R.PS["w"], a)[0]
        for mut in ("yx_swap", "w_for_2w"):
            assert _far(R.pixel_shuffle2(y, bias, add, R.PS["h"], R.PS["w"], a, mut=mut)[0], ref, R.bound("pixel_shuffle:bf16", BF, ref))
    for nm in R.HYPER["nms"]:
        hy, up = R.hyper_inputs(nm)
        ref = R.hyper_masks(hy, up)
        assert _far(R.hyper_masks(hy, up, mut="pj_layout"), ref, R.bound("hyper_masks:fp32", F32, ref)) == (nm > 1) and R.HYPER["HW"] % 256          # one mask has one layout
    for A_ in R.HOLE_AREAS:
        m = R.holes_mask(A_)
        assert m.shape[0] != m.shape[1] and not torch.equal(R.fill_holes(m, A_, mut="rows_of_H"), R.fill_holes(m, A_))
