"""Second-pass direct tests of the image kernels (vv_image.hip), the flow-completion and generator helpers (vv_deform.hip) and the SAM 2 helpers (vv_sam2.hip), called
through their hip.py wrappers against tests/aux2ref.py: the image kernels on a clip of many small frames that reaches past the grid cap (the second pass of the
grid-stride loops, where the frame index is used), the others at the block boundary, the second batch, every template instantiation and launcher branch.  Exact kernels
must EQUAL the fp32 restatement or the oracle; rounded kernels meet |got - ref| <= B = ceil(4 N) u max(1, max |ref|) against fp64 (N: tests/test_aux2ref_cpu.py).
Every output lives between sentinel guards that must stay untouched, every output is finite, every case logs one line."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aux2ref as R  # noqa: E402
import test_aux_kernels_gpu as AUX  # noqa: E402
from test_aux_kernels_gpu import Guarded, DNAMES  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64, U8 = torch.float32, torch.float64, torch.uint8
ONAMES = ["fp32"] + DNAMES


def _exact(name, label, got, ref, *guards):
    AUX._exact(name, label, got, ref, *guards, tag="aux2")


def _close(name, key, label, got, ref, out_dtype, *guards, **kw):
    return AUX._close(name, key, label, got, ref, out_dtype, *guards, table=R.NOISE, tag="aux2", **kw)


def _np(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _types(hip, oname):
    """(library dtype id, torch type of an `oname` output): an fp32 output goes through the fp16 instantiation"""
    return (hip.F16, F32) if oname == "fp32" else (hip.dtype_id(oname), R.TD[oname])


# ================================================================================================================ vv_image.hip past its grid cap
@pytest.mark.parametrize("hs,vs", R.YCC_MODES)
def test_ycbcr_to_rgb_converts_every_frame_of_a_clip_past_the_grid_cap(gpu, hs, vs):
    """80 frames of 245 x 245: ten whole frames lie past 16384 x 256 pixels.  Before the kernel walked a grid-stride loop those stayed as the allocation left them."""
    from videovanish_amd import hip
    T, H, W = R.CLIP["T"], R.CLIP["H"], R.CLIP["W"]
    y, cb, cr = R.ycc_inputs(hs, vs)
    yg, cbg, crg = (_np(a, gpu) for a in (y, cb, cr))
    for full in (False, True):
        o = Guarded((T, H, W, 3), U8, gpu)
        hip.ycbcr_to_rgb(yg, cbg, crg, hs, vs, full, out=o.t)
        _exact("ycbcr_to_rgb", f"{T} x {H} x {W}, shifts ({hs}, {vs}), {'full' if full else 'limited'} range, against the host routine", o.t, torch.from_numpy(R.ycc_host(y, cb, cr, hs, vs, full)), o)
    assert torch.equal(hip.ycbcr_to_rgb(yg[:2], cbg[:2], crg[:2], hs, vs, True), o.t[:2]), "without out= the wrapper returns a fresh tensor with the same bytes"


@pytest.mark.parametrize("ch", [1, 3])
def test_mask_collapse_dilate_indexes_its_frame_past_the_cap(gpu, ch):
    from videovanish_amd import hip
    T, H, W = R.CLIP["T"], R.CLIP["H"], R.CLIP["W"]
    m = R.clip_masks(ch)
    mg = _np(m, gpu)
    for iters, path in ((0, "whole-frame fill by flag"), (1, "odd: copied back"), (2, "even: no copy")):
        o = Guarded((T, H, W), U8, gpu)
        hip.mask_collapse_dilate(mg, iters, out=o.t)
        _exact("mask_collapse_dilate", f"{T} x {H} x {W} x {ch}, iters {iters} ({path})", o.t, torch.from_numpy(R.collapse_dilate(m, iters)), o)


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("kind", ["up", "down"])
def test_resize_u8_destination_past_the_cap(gpu, kind, ch):
    from videovanish_amd import hip
    Hd, Wd = R.RESIZE_DST
    src = R.resize_inputs(kind, ch)
    sg = _np(src, gpu)
    for mode in ("bilinear", "nearest"):
        o = Guarded((src.shape[0], Hd, Wd, ch), U8, gpu)
        hip.resize_u8(sg, Hd, Wd, mode=mode, out=o.t)
        _exact(f"resize_{mode}_u8", f"{src.shape[0]} x {src.shape[1]} x {src.shape[2]} x {ch} -> {Hd} x {Wd} ({kind}scale)", o.t, torch.from_numpy(R.resize_u8(src, Hd, Wd, mode)), o)


def test_chamfer_dt_and_feather_composite_past_the_cap(gpu):
    """the distance transform of the reference by the C form of the oracle (oracle/imageops_c.py), frame by frame"""
    from videovanish_amd import hip
    T, H, W = R.CLIP["T"], R.CLIP["H"], R.CLIP["W"]
    inp, orig, _, mask = R.compose_inputs()
    ig, og, mg = (_np(a, gpu) for a in (inp, orig, mask))
    for Rr in (1, 5):
        o = Guarded((T, H, W), F32, gpu)
        hip.chamfer_dt(mg, Rr, out=o.t)
        _exact("chamfer_dt", f"{T} x {H} x {W}, R {Rr} (C oracle)", o.t, torch.from_numpy(R.chamfer_dt(mask, Rr)), o)
    for feather in (0.0, 1.0, 2.5):
        o = Guarded((T, H, W, 3), U8, gpu)
        hip.feather_composite(ig, og, mg, feather, out=o.t)
        _exact("feather_composite", f"{T} x {H} x {W}, feather {feather} (C oracle for the distances)", o.t, torch.from_numpy(R.feather_composite(inp, orig, mask, feather)), o)


@pytest.mark.parametrize("T,H,W", [(R.CLIP["T"], R.CLIP["H"], R.CLIP["W"]), (3, 9, 6)])
def test_blur_compose_past_the_cap_and_where_the_reflection_folds_twice(gpu, T, H, W):
    """9 x 6: below 11 pixels refl101 leaves the image after one reflection and clamps, as the oracle's does"""
    from videovanish_amd import hip, imageops
    _, orig, pix, mask = R.compose_inputs(T, H, W)
    o = Guarded((T, H, W, 3), U8, gpu)
    hip.blur_compose(_np(pix, gpu), _np(orig, gpu), _np(mask, gpu), imageops.gaussian_taps_21(), out=o.t)
    _exact("blur_compose", f"{T} x {H} x {W} (numpy oracle)", o.t, torch.from_numpy(R.blur_compose(pix, orig, mask)), o)


# ================================================================================================================ vv_deform.hip: flow completion and generator helpers
def test_fc_input_replicates_the_border_of_its_own_frame(gpu):
    from videovanish_amd import hip
    T, H, W = R.FC_SHAPE
    flow, mask = R.fc_inputs()
    for pad in R.FC_PADS:
        o = Guarded((T, H + 2 * pad, W + 2 * pad, 8), F32, gpu)
        hip.fc_input(flow.to(gpu), mask.to(gpu), pad, out=o.t)
        _exact("fc_input", f"{T} x {H} x {W}, pad {pad}", o.t, R.fc_input(flow, mask, pad), o)
        assert bool((o.t[..., 3:] == 0).all()), "channels 3 .. 7 must be zero"


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("B,H,W,C", R.UP2_CASES)
def test_upsample2x_bilinear_every_input_type(gpu, dname, B, H, W, C):
    from videovanish_amd import hip
    td, dt = R.TD[dname], hip.dtype_id(dname)
    x = R.up2_inputs(B, H, W, C)
    for xin, oname, od in ((x, "fp32", F32), (x.to(td), dname, td)):
        o = Guarded((B * 4 * H * W, C), od, gpu)
        hip.upsample2x_bilinear(dt, xin.reshape(-1, C).to(gpu), B, H, W, out=o.t)
        ref = R.upsample2x(xin).reshape(-1, C)
        _close("upsample2x_bilinear", f"upsample2x:{oname}", f"[{dname}] {oname} in, B {B}, {H} x {W}, C {C}", o.t, R.r16(ref, None if od == F32 else td), od, o)


def test_flow_combine_and_gen_input_at_a_block_boundary(gpu):
    from videovanish_amd import hip
    n = R.PIX_N
    flow, mask = R.randn(2, n, 2), R.mask_0_1_255(n, 3)
    assert {int(v) for v in mask.unique()} == {0, 1, 255}
    for ld in R.LD_PRED["flow_combine"]:
        pred = R.randn(1, n, ld)
        o = Guarded((n, 2), F32, gpu)
        hip.flow_combine(pred.to(gpu), flow.to(gpu), mask.to(gpu), out=o.t)
        _exact("flow_combine", f"npx {n}, ld_pred {ld}, mask values 0 / 1 / 255", o.t, R.flow_combine(pred, flow, mask), o)
    frames = torch.randint(0, 256, (n, 3), generator=R.gen(4), dtype=U8)
    m_up = R.mask_0_1_255(n, 5)
    o = Guarded((n, 8), F32, gpu)
    hip.gen_input(frames.to(gpu), mask.to(gpu), m_up.to(gpu), out=o.t)
    _exact("gen_input", f"npx {n}", o.t, R.gen_input(frames, mask, m_up), o)


@pytest.mark.parametrize("ld", R.LD_PRED["gen_compose"])
def test_gen_compose_first_visit_and_mean_of_two(gpu, ld):
    """the floor of a rounded tanhf: values whose fp64 (tanh + 1) 127.5 lies within the band of an integer are left out (at most 0.1 %, tests/test_aux2ref_cpu.py)"""
    from videovanish_amd import hip
    pred, ori, mask, acc = R.gen_compose_inputs(ld)
    keep = R.gen_compose_keep(pred, mask, R.bound("gen_compose:fp32", F32, R.gen_compose_t(pred)))
    assert (~keep).float().mean().item() <= R.GC_CAP
    for first in (True, False):
        o = Guarded((R.GC_N, 3), F32, gpu, init=acc.to(gpu))
        hip.gen_compose(pred.to(gpu), ori.to(gpu), mask.to(gpu), o.t, first)
        _close("gen_compose", "gen_compose:fp32", f"npx {R.GC_N}, ld_pred {ld}, {'first visit' if first else 'mean with the first visit'}, {int((~keep).sum())} of {keep.numel()} values left out",
               o.t, R.gen_compose(pred, ori, mask, acc, first), F32, o, keep=keep)


@pytest.mark.parametrize("dname", DNAMES)
def test_gather_rows_negative_repeated_and_last_indices(gpu, dname):
    from videovanish_amd import hip
    td = R.TD[dname]
    for C in (8, 24):          # 16 and 48 bytes per row
        src = R.randn(5 + C, R.GATHER_ROWS, C).to(td)
        for kind in ("all -1", "mixed"):
            idx = R.gather_idx(kind)
            o = Guarded((R.GATHER_N, C), td, gpu)
            hip.gather_rows(src.to(gpu), idx.to(gpu), out=o.t)
            _exact("gather_rows", f"[{dname}] {R.GATHER_N} rows of {2 * C} bytes out of {R.GATHER_ROWS}, indices {kind}", o.t, R.gather_rows(src, idx), o)


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("k,s,p,h,w", R.FOLD_GEOM)
def test_fold_patches_every_instantiation(gpu, dname, k, s, p, h, w):
    from videovanish_amd import hip
    td, dt = R.TD[dname], hip.dtype_id(dname)
    fh, fw = R.fold_grid(k, s, p, h, w)
    for C in R.FOLD_C:
        x = R.fold_inputs(k, s, p, h, w, C)
        for xin, iname in ((x, "fp32"), (x.to(td), dname)):
            for od, oname in ((F32, "fp32"), (td, dname)):
                for nrm, gl in R.FOLD_FLAGS:
                    o = Guarded((R.FOLD_B * h * w, C), od, gpu)
                    hip.fold_patches(dt, xin.to(gpu), R.FOLD_B, fh, fw, C, h, w, k=k, stride=s, pad=p, normalise=nrm, gelu=gl, out_dtype=od, out=o.t)
                    ref, gx = R.fold_patches(xin, R.FOLD_B, C, h, w, k, s, p, nrm, gl)
                    _close("fold_patches", f"fold:{oname}", f"[{dname}] {iname} in, {oname} out, k {k} s {s} p {p}, {h} x {w}, C {C}, normalise {int(nrm)}, gelu {int(gl)}", o.t,
                           R.r16(ref, None if od == F32 else td), od, o, gelu_x=gx if gl else None)


def test_flow_down4(gpu):
    from videovanish_amd import hip
    for T, H, W in R.DOWN4_SHAPES:
        f = R.randn(7, T, H, W, 2, scale=5.0)
        o = Guarded((T, H // 4, W // 4, 2), F32, gpu)
        hip.flow_down4(f.to(gpu), out=o.t)
        _exact("flow_down4", f"{T} x {H} x {W}", o.t, R.flow_down4(f), o)


# ================================================================================================================ vv_sam2.hip helpers
@pytest.mark.parametrize("oname", ONAMES)
def test_maxpool2x2_strided_batches_of_negative_values(gpu, oname):
    from videovanish_amd import hip
    d = R.POOL
    td = F32 if oname == "fp32" else R.TD[oname]
    buf = R.pool_inputs().to(td)
    o = Guarded((d["B"] * (d["H"] // 2) * (d["W"] // 2), d["C"]), td, gpu)
    hip.maxpool2x2(buf.to(gpu), d["B"], d["H"], d["W"], Cc=d["C"], in_bs=d["H"] * d["W"] * d["C"] + d["gap"], x_off=d["x_off"], out=o.t)
    _exact("maxpool2x2", f"[{oname}] B {d['B']}, {d['H']} x {d['W']} x {d['C']}, in_bs = image + {d['gap']}, x_off {d['x_off']}, all values negative", o.t, R.maxpool2x2(buf), o)


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("c", R.ROPE_CASES, ids=lambda c: f"D{c['D']}")
def test_rope_apply_leaves_everything_outside_its_block_alone(gpu, dname, c):
    from videovanish_amd import hip
    td, dt = R.TD[dname], hip.dtype_id(dname)
    x, cs = R.rope_inputs(c, td)
    o = Guarded((c["rows"], c["ld"]), td, gpu, init=x.to(gpu))
    hip.rope_apply(dt, o.t, c["rows_rope"], cs.to(gpu), c["D"], col0=c["col0"], ld=c["ld"])
    tag = f"[{dname}] D {c['D']}, rows {c['rows_rope']} of {c['rows']}, columns {c['col0']} .. {c['col0'] + c['D']} of {c['ld']}, table of {c['n_table']} rows"
    _close("rope_apply", f"rope:{dname}", tag, o.t, R.rope_apply(x, cs, c, td), td, o)
    out = ~R.rope_region(c)
    _exact("rope_apply", f"{tag}: the elements outside the block", o.t.cpu()[out], x[out], o)


def test_dwconv_small_images_and_both_kernel_sizes(gpu):
    from videovanish_amd import hip
    for k, C, H, W in R.DW_CASES:
        x, w, b = R.dw_inputs(k, C, H, W)
        o = Guarded((H * W, C), F32, gpu)
        hip.dwconv(x.to(gpu), H, W, w.to(gpu), b.to(gpu), out=o.t)
        _close("dwconv", "dwconv:fp32", f"k {k}, C {C}, {H} x {W}", o.t, R.dwconv(x, H, W, w, b), F32, o)


@pytest.mark.parametrize("oname", ONAMES)
def test_pixel_shuffle2_every_output_type_and_activation(gpu, oname):
    from videovanish_amd import hip
    dt, od = _types(hip, oname)
    h, w, C = R.PS["h"], R.PS["w"], R.PS["C"]
    y, bias, add = R.ps_inputs()
    for ad, atag in ((add, "with add"), (None, "without add")):
        for a in R.PS_ACTS:
            o = Guarded((4 * h * w, C), od, gpu)
            hip.pixel_shuffle2(dt, y.to(gpu), bias.to(gpu), h, w, add=None if ad is None else ad.to(gpu), act=a, out_dtype=od, out=o.t)
            tag = f"[{oname}] {h} x {w} x {C}, {atag}, act {a}"
            if a in (R.ACT_NONE, R.ACT_RELU):          # sums alone: nothing for a contraction to change
                _exact("pixel_shuffle2", tag, o.t, R.pixel_shuffle2(y, bias, ad, h, w, a, F32)[0].to(od), o)
            else:
                ref, gx = R.pixel_shuffle2(y, bias, ad, h, w, a)
                _close("pixel_shuffle2", f"pixel_shuffle:{oname}", tag, o.t, R.r16(ref, None if od == F32 else od), od, o, gelu_x=gx if a == R.ACT_GELU else None)
    with pytest.raises(RuntimeError, match="vv_pixel_shuffle2"):
        hip.pixel_shuffle2(dt, y.to(gpu), bias.to(gpu), h, w, act=hip.ACT_LRELU)
    AUX._log(f"aux2 pixel_shuffle2 [{oname}] LRELU: refused with an argument error")


def test_resize_bilinear_f32_degenerate_identity_up_and_down(gpu):
    from videovanish_amd import hip
    for Hs, Ws, Hd, Wd, C in R.RESIZE_F32:
        s = R.resize_f32_inputs(Hs, Ws, C)
        o = Guarded((Hd * Wd, C), F32, gpu)
        hip.resize_bilinear_f32(s.to(gpu), Hs, Ws, Hd, Wd, out=o.t)
        _close("resize_bilinear_f32", "resize_f32:fp32", f"{Hs} x {Ws} -> {Hd} x {Wd}, C {C}", o.t, R.resize_bilinear_f32(s, Hs, Ws, Hd, Wd), F32, o)


def test_prompt_points_and_sine_pe(gpu):
    from videovanish_amd import hip
    for D in R.PP_D:
        coords, labels, gauss, table = R.pp_inputs(D)
        o = Guarded((labels.numel(), D), F32, gpu)
        hip.prompt_points(coords.to(gpu), labels.to(gpu), 1.0 / R.PP_SIZE, gauss.to(gpu), table.to(gpu), out=o.t)
        _close("prompt_points", "prompt_points:fp32", f"P {labels.numel()}, D {D}, labels -1 .. 3, coordinates 0 and {R.PP_SIZE - 1}", o.t,
               R.prompt_points(coords, labels, 1.0 / R.PP_SIZE, gauss, table), F32, o)
    for dim in R.SINE_DIMS:
        for kind, pos in R.SINE_POS.items():
            o = Guarded((pos.numel(), dim), F32, gpu)
            hip.sine_pe_1d(pos.to(gpu), dim, out=o.t)
            _close("sine_pe_1d", f"sine_pe_{kind}:fp32", f"dim {dim}, {kind} positions (max |pos| {pos.abs().max().item():.1f})", o.t, R.sine_pe_1d(pos, dim), F32, o)


@pytest.mark.parametrize("nm", R.HYPER["nms"])
def test_hyper_masks_and_sam_pick(gpu, nm):
    from videovanish_amd import hip
    HW = R.HYPER["HW"]
    hy, up = R.hyper_inputs(nm)
    o = Guarded((nm, HW), F32, gpu)
    hip.hyper_masks(hy.to(gpu), up.to(gpu), out=o.t)
    _close("hyper_masks", "hyper_masks:fp32", f"nm {nm}, HW {HW}, C {R.HYPER['C']}", o.t, R.hyper_masks(hy, up), F32, o)
    masks = R.hyper_masks(hy, up, F32).contiguous()
    for sel in ([nm - 1, 1, 0], [nm - 1, 0, 0], [0, 1, 0]):
        o = Guarded((HW,), F32, gpu)
        hip.sam_pick(masks.to(gpu), torch.tensor(sel, dtype=torch.int32, device=gpu), -1024.0, out=o.t)
        _exact("sam_pick", f"nm {nm}, HW {HW}, sel {sel}", o.t, R.sam_pick(masks, sel, -1024.0), o)


@pytest.mark.parametrize("max_area", R.HOLE_AREAS)
def test_fill_holes_on_a_non_square_mask(gpu, max_area):
    """a snake of exactly max_area pixels (filled) and one pixel longer (kept), segments joined by a diagonal, a spiral, border and corner holes, against scipy's
    8-connected labelling; the workspace is guarded too"""
    from videovanish_amd import hip
    H, W = R.HOLES["H"], R.HOLES["W"]
    cases = [(R.holes_mask(max_area), f"{H} x {W}")] + [(torch.full((5, 7), v), f"5 x 7, all {v}") for v in (-1.0, 0.0, 1.0)]
    for m, tag in cases:
        h, w = m.shape
        o, ws = Guarded((h * w,), F32, gpu, init=m.reshape(-1).to(gpu)), Guarded((3 * h * w,), torch.int32, gpu)
        hip.fill_holes(o.t, h, w, max_area, ws=ws.t)
        _exact("fill_holes", f"{tag}, max_area {max_area}", o.t, R.fill_holes(m, max_area).reshape(-1), o, ws)
