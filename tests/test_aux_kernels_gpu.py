"""The helper kernels of vv_elem.hip, vv_flow.hip, vv_sam2.hip, vv_deform.hip (raw mode) and the LayerNorms, called directly through their hip.py wrappers, against
tests/auxref.py: at sizes just over the grid cap (the second pass of the grid-stride loops, where the per-frame tables are indexed) and at the small shapes that select
each launcher branch.  Exact kernels must EQUAL the fp32 restatement; rounded kernels meet |got - ref| <= B = ceil(4 N) u max(1, max |ref|) against fp64 (N:
tests/test_auxref_cpu.py).  Every output lives between sentinel guards that must stay untouched, every output is finite, every case logs one line."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auxref as R  # noqa: E402

pytestmark = pytest.mark.gpu
REPORT = os.environ.get("VV_PARITY_REPORT")
DNAMES = ["fp16", "bf16"]
F32, F64 = torch.float32, torch.float64
GUARD = 4096          # guard elements on each side of an output (a multiple of 16 bytes for every type)


def _log(msg):
    print(msg)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(msg + "\n")


class Guarded:
    """an output (or an in-place operand) of `shape` inside a sentinel-filled allocation"""

    def __init__(self, shape, dtype, gpu, init=None):
        self.n = math.prod(shape)
        self.sent = R.SENTINEL if dtype.is_floating_point else R.SENTINEL_INT
        self.buf = torch.full((GUARD + self.n + GUARD,), self.sent, dtype=dtype, device=gpu)
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        return bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[GUARD + self.n:] == self.sent).all())


def _exact(name, label, got, ref, *guards, tag="aux"):
    """got (on the GPU) must equal ref (CPU) bit for bit; compared where the data is; tag: the first word of the logged line"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    r = ref.to(got.device)
    bad = int((got != r).sum().item())
    fin = bool(torch.isfinite(got).all()) if got.dtype.is_floating_point else True
    ok = all(g.intact() for g in guards)
    _log(f"{tag} {name} {label}: " + ("exact" if bad == 0 else f"{bad} of {got.numel()} elements differ") + ("" if ok else ", GUARDS TOUCHED") + ("" if fin else ", NOT FINITE"))
    assert bad == 0 and fin and ok


def _close(name, key, label, got, ref, out_dtype, *guards, gelu_x=None, keep=None, table=None, tag="aux"):
    """rounded kernel: got (GPU) against the fp64 ref (CPU), B from auxref.NOISE[key] (or table[key]); keep: the elements compared (threshold elements are left out)"""
    g = got.detach().cpu().double()
    assert g.shape == ref.shape, (g.shape, ref.shape)
    fin = bool(torch.isfinite(g).all())
    B = R.bound(key, out_dtype, ref, gelu_x, table)
    d = (g - ref).abs()
    if keep is not None:
        d = d[keep]
    err = d.max().item()
    ok = all(x.intact() for x in guards)
    _log(f"{tag} {name} {label}: max |got - ref| {err:.3e} = {err / B:.3f} B (B = {B:.3e}, max |ref| {ref.abs().max().item():.2f})" + ("" if ok else ", GUARDS TOUCHED")
         + ("" if fin else ", NOT FINITE"))
    assert fin and ok and err <= B
    return err / B


# ================================================================================================================ second pass of the grid-stride loops
def test_elem_flat_kernels_second_pass(gpu):
    from videovanish_amd import hip
    n = R.ELEM_CAP + 1000
    x, y, z = R.randn(1, n), R.randn(2, n), R.randn(3, n)
    xg, yg, zg = x.to(gpu), y.to(gpu), z.to(gpu)
    o = Guarded((n,), F32, gpu)
    hip.axpby(xg, yg, 0.7, -1.3, out=o.t)
    _exact("axpby", f"n = cap + 1000 = {n}", o.t, R.axpby(x, y, 0.7, -1.3), o)
    for zz, zc, tag in ((zg, z, "with z"), (None, None, "without z")):
        o = Guarded((n,), F32, gpu)
        hip.sched_step(xg, yg, zz, 0.8, 0.6, 0.9, 0.3, 0.2, out=o.t)
        _exact("sched_step", f"{tag}, n = {n}", o.t, R.sched_step(x, y, zc, 0.8, 0.6, 0.9, 0.3, 0.2), o)
    xs = R.silu_inputs(n)
    o = Guarded((n,), F32, gpu)
    hip.silu(xs.to(gpu), out=o.t)
    _close("silu", "silu:fp32", f"n = {n}", o.t, R.silu(xs), F32, o)
    o = Guarded((n,), F32, gpu, init=xg)
    hip.add_inplace(hip.F16, o.t, yg)
    _exact("add_inplace", f"fp32 y, n = {n}", o.t, R.add_inplace(x, y), o)
    rows = n // 8 + 1
    xr = R.randn(4, rows, 3)
    o = Guarded((rows, 8), F32, gpu)
    hip.pad_channels_f32(xr.to(gpu), 8, 0.18215, out=o.t)
    _exact("pad_channels_f32", f"{rows} x 3 -> 8", o.t, R.pad_channels(xr, 8, 0.18215), o)


@pytest.mark.parametrize("dname", DNAMES)
def test_elem_h16_kernels_second_pass(gpu, dname):
    from videovanish_amd import hip
    td, dt = R.TD[dname], hip.dtype_id(dname)
    n = R.ELEM_CAP + 1000
    x, y = R.randn(1, n), R.randn(2, n).to(td)
    o = Guarded((n,), F32, gpu, init=x.to(gpu))
    hip.add_inplace(dt, o.t, y.to(gpu))
    _exact("add_inplace", f"[{dname}] y, n = {n}", o.t, R.add_inplace(x, y), o)
    rows = n // 8 + 1
    xr = R.randn(4, rows, 3)
    o = Guarded((rows, 8), td, gpu)
    hip.pad_channels(dt, xr.to(gpu), 8, 0.18215, out=o.t)
    _exact("pad_channels", f"[{dname}] {rows} x 3 -> 8", o.t, R.pad_channels(xr, 8, 0.18215).to(td), o)
    n4 = 4 * n                                   # one thread splits four values
    xs = R.randn(5, n4, scale=3.0)
    hi, lo = Guarded((n4,), td, gpu), Guarded((n4,), td, gpu)
    hip.split_f32(dt, xs.to(gpu), 1024.0, hi=hi.t, lo=lo.t)
    rh, rl = R.split_f32(xs, 1024.0, td)
    _exact("split_f32", f"[{dname}] hi, n = 4 (cap + 1000)", hi.t, rh.to(td), hi)
    _exact("split_f32", f"[{dname}] lo, n = 4 (cap + 1000)", lo.t, rl.to(td), lo)
    M = n // 2                                   # C = 8: two threads per row
    x3 = xs[:M * 8].reshape(M, 8)
    o = Guarded((M, 24), td, gpu)
    hip.split3(dt, x3.to(gpu), out=o.t)
    _exact("split3", f"[{dname}] fp32 in, {M} x 8", o.t, R.split3(x3, td).to(td), o)


def test_window_average_and_decode_blend_index_their_frame_in_the_second_pass(gpu):
    from videovanish_amd import hip
    T, per = R.FRAME_T, R.FRAME_PER
    value, count = R.window_inputs()
    o = Guarded((T, per), F32, gpu)
    hip.window_average(value.to(gpu), count.to(gpu), out=o.t)
    _exact("window_average", f"frames {T}, per_frame {per}", o.t, R.window_average(value, count), o)
    dec, w, acc = R.blend_inputs()
    o = Guarded((T, per, 1, 3), F32, gpu, init=acc.reshape(T, per, 1, 3).to(gpu))
    hip.decode_blend(dec.reshape(T, per, 1, 4).to(gpu), w.to(gpu), o.t)
    _exact("decode_blend", f"T {T}, HW {per}, ld 4, weights 0 / 0.25 / 1", o.t, R.decode_blend(dec, w, acc).reshape(T, per, 1, 3), o)


@pytest.mark.parametrize("dname", DNAMES)
def test_preprocess_and_brushnet_input_cross_a_frame_in_the_second_pass(gpu, dname):
    from videovanish_amd import hip
    td, dt = R.TD[dname], hip.dtype_id(dname)
    T, H, W = R.BRUSH["T"], R.BRUSH["H"], R.BRUSH["W"]          # 2 102 100 pixels: the last frame starts inside the first pass and ends in the second
    frames = torch.randint(0, 256, (T, H, W, 3), generator=R.gen(1), dtype=torch.uint8)
    mask = (torch.rand(T, H, W, generator=R.gen(2)) < 0.3).to(torch.uint8) * 255
    img, msk = Guarded((T, H, W, 8), td, gpu), Guarded((T, H, W, 8), td, gpu)
    hip.preprocess(dt, frames.to(gpu), mask.to(gpu), img=img.t, masked=msk.t)
    ri, rm = R.preprocess(frames, mask)
    _exact("preprocess", f"[{dname}] img, {T} x {H} x {W}", img.t, ri.to(td), img)
    _exact("preprocess", f"[{dname}] masked, {T} x {H} x {W}", msk.t, rm.to(td), msk)
    Hm, Wm = R.BRUSH["Hm"], R.BRUSH["Wm"]          # mask 1.5 x the latent grid: a non-integer nearest ratio
    lat, cond, m2 = R.brushnet_inputs()
    o = Guarded((T, H, W, 16), td, gpu)
    hip.brushnet_input(dt, lat.to(gpu), cond.to(gpu), m2.to(gpu), Hm, Wm, out=o.t)
    _exact("brushnet_input", f"[{dname}] {T} x {H} x {W}, mask {Hm} x {Wm}", o.t, R.brushnet_input(lat, cond, m2, Hm, Wm).to(td), o)


def test_flow_flat_kernels_second_pass(gpu):
    from videovanish_amd import hip
    n = R.FLOW_CAP + 1000
    a, b = R.randn(1, n), R.randn(2, n)
    o = Guarded((n,), F32, gpu)
    hip.add_relu(a.to(gpu), b.to(gpu), out=o.t)
    _exact("add_relu", f"n = cap + 1000 = {n}", o.t, R.add_relu(a, b), o)
    u = torch.randint(0, 4, (n,), generator=R.gen(3), dtype=torch.uint8) * 85
    o = Guarded((n,), torch.uint8, gpu)
    hip.u8_is_zero(u.to(gpu), out=o.t)
    _exact("u8_is_zero", f"n = {n}", o.t, R.u8_is_zero(u), o)
    o = Guarded((n,), F32, gpu)
    hip.u8_to_f32(u.to(gpu), out=o.t)
    _exact("u8_to_f32", f"n = {n}", o.t, R.u8_to_f32(u), o)
    frame = torch.randint(0, 256, (n, 3), generator=R.gen(4), dtype=torch.uint8)
    for hole, tag in ((u, "a quarter kept"), (torch.ones(n, dtype=torch.uint8), "every pixel a hole")):
        o = Guarded((4,), torch.int64, gpu)
        hip.masked_sum_u8(frame.to(gpu), hole.to(gpu), out=o.t)
        _exact("masked_sum_u8", f"{tag}, n = {n}", o.t, R.masked_sum_u8(frame, hole), o)
    M = R.FLOW_CAP // 2 + 500
    c1 = R.randn(5, M, 2, scale=30.0)
    for ld in (2, 8):
        df = R.randn(6 + ld, M, ld)
        o = Guarded((M, 2), F32, gpu, init=c1.to(gpu))
        hip.add_flow(o.t, df.to(gpu))
        _exact("add_flow", f"ld {ld}, M = {M}", o.t, R.add_flow(c1, df), o)


@pytest.mark.parametrize("dname", DNAMES)
def test_raft_elementwise_kernels_second_pass(gpu, dname):
    from videovanish_amd import hip
    td, dt = R.TD[dname], hip.dtype_id(dname)
    M = 32800                                    # 128 M = cap + 4096
    cn, h, q = R.raft_rows(3, M)
    net, net16, xbuf = Guarded((M, 128), F32, gpu), Guarded((M, 128), td, gpu), Guarded((M, 256), td, gpu)
    hip.raft_ctx_split(dt, cn.to(gpu), net.t, net16.t, xbuf.t)
    rn, ri = R.raft_ctx_split(cn)
    _close("raft_ctx_split", "ctx_split:fp32", f"[{dname}] net, M = {M}", net.t, rn, F32, net)
    _close("raft_ctx_split", f"ctx_split:{dname}", f"[{dname}] net16", net16.t, R.r16(rn, td), td, net16)
    _close("raft_ctx_split", f"ctx_split:{dname}", f"[{dname}] xbuf[:, :128]", xbuf.t[:, :128], R.r16(ri, td), td, xbuf)
    assert bool((xbuf.t[:, 128:] == R.SENTINEL).all()), "raft_ctx_split wrote the columns of xbuf it does not own"
    rh = Guarded((M, 128), td, gpu)
    hip.gru_rh(dt, cn.to(gpu), h.to(gpu), rh.t)
    _close("gru_rh", f"gru_rh:{dname}", f"[{dname}] M = {M}", rh.t, R.r16(R.gru_rh(cn, h), td), td, rh)
    hh, h16o = Guarded((M, 128), F32, gpu, init=h.to(gpu)), Guarded((M, 128), td, gpu)
    hip.gru_update(dt, cn.to(gpu), q.to(gpu), hh.t, h16o.t)
    ref = R.gru_update(cn, q, h)
    _close("gru_update", "gru_update:fp32", f"[{dname}] h, M = {M}", hh.t, ref, F32, hh)
    _close("gru_update", f"gru_update:{dname}", f"[{dname}] h16", h16o.t, R.r16(ref, td), td, h16o)
    npix = R.FLOW_CAP + 1000
    img = torch.randint(0, 256, (npix, 3), generator=R.gen(7), dtype=torch.uint8)
    o = Guarded((npix, 8), td, gpu)
    hip.raft_prep(dt, img.to(gpu), out=o.t)
    _exact("raft_prep", f"[{dname}] npix = cap + 1000", o.t, R.raft_prep(img).to(td), o)


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("w,h,grids", [(41, 37, 3), (4099, 1024, 1)])
def test_raft_flow_prep_subtracts_the_position_in_its_own_grid(gpu, dname, w, h, grids):
    """3 stacked grids of 37 x 41 (the row index wraps per grid), and one grid of 4099 x 1024 = cap + 3072 rows for the second pass"""
    from videovanish_amd import hip
    td, dt = R.TD[dname], hip.dtype_id(dname)
    M = grids * h * w
    m = torch.arange(M)
    coords1 = torch.stack([(m % w).float(), ((m // w) % h).float()], 1) + R.randn(9, M, 2, scale=4.0)
    flow8, xbuf = Guarded((M, 8), td, gpu), Guarded((M, 256), td, gpu)
    hip.raft_flow_prep(dt, coords1.to(gpu), w, h, flow8.t, xbuf.t)
    ref = R.raft_flow_prep(coords1, w, h).to(td)
    ref8 = torch.zeros((M, 8), dtype=td)
    ref8[:, :2] = ref
    _exact("raft_flow_prep", f"[{dname}] flow8, {grids} x {h} x {w}", flow8.t, ref8, flow8)
    _exact("raft_flow_prep", f"[{dname}] xbuf[:, 254:], {grids} x {h} x {w}", xbuf.t[:, 254:], ref, xbuf)
    assert bool((xbuf.t[:, :254] == R.SENTINEL).all()), "raft_flow_prep wrote the columns of xbuf it does not own"


def _corr_case(gpu, hip, dname, pyr, coords, cpad, label):
    td, dt = R.TD[dname], hip.dtype_id(dname)
    N = coords.shape[0]
    o = Guarded((N, cpad), td, gpu)
    hip.corr_lookup(dt, [p.to(gpu) for p in pyr], coords.to(gpu), cpad=cpad, out=o.t)
    ref = torch.zeros((N, cpad), dtype=F64)
    ref[:, :324] = R.r16(R.corr_lookup(pyr, coords), td)
    _close("corr_lookup", f"corr_lookup:{dname}", f"[{dname}] {label}", o.t, ref, td, o)
    assert bool((o.t[:, 324:] == 0).all()), "corr_lookup: the channels behind 324 must be zero"


@pytest.mark.parametrize("dname", DNAMES)
def test_corr_lookup_second_pass(gpu, dname):
    from videovanish_amd import hip
    N = 11000                                    # 384 N = cap + 29 696
    pyr = [R.randn(5 + l, N, 8 >> l, 8 >> l) for l in range(4)]
    coords = torch.rand(N, 2, generator=R.gen(14)) * 14.0 - 3.0
    _corr_case(gpu, hip, dname, pyr, coords, 384, f"N = {N} planes of 8 x 8, cpad 384")


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("h,w", R.CORR_SIZES)
def test_corr_lookup_edges(gpu, dname, h, w):
    """two stacked pairs, positions on the grid, at -4, at w + 3.5, at half pixels; cpad = 328"""
    from videovanish_amd import hip
    pyr, coords = R.corr_inputs(h, w)
    _corr_case(gpu, hip, dname, pyr, coords, 328, f"2 pairs of {h} x {w}, cpad 328")


def test_convex_upsample_second_pass(gpu):
    from videovanish_amd import hip
    Fr, h, w = 3, 150, 150                       # 64 F h w = cap + 125 696: the last 1964 coarse pixels of frame 2 run in the second pass
    coords1, _ = R.convex_inputs(Fr, h, w, seed=15, with_mask=False)
    mask = R.device_mask(Fr * h * w, gpu)
    o = Guarded((Fr, 8 * h, 8 * w, 2), F32, gpu)
    hip.convex_upsample(coords1.to(gpu), mask, h, w, F=Fr, out=o.t)
    first = R.FLOW_CAP // 64
    sel = torch.cat([torch.arange(first - 200, Fr * h * w), torch.arange(0, first - 200, 97), torch.arange(h * w - 160, h * w + 160)]).unique()
    ref = R.convex_upsample(coords1, mask[sel.to(gpu)].cpu(), sel, Fr, h, w)
    _close("convex_upsample", "convex_upsample:fp32", f"F {Fr}, {h} x {w}: the second pass, the frame boundary and every 97th pixel", R.convex_gather(o.t, sel.to(gpu), Fr, h, w), ref, F32, o)
    assert bool(torch.isfinite(o.t).all())


def test_convex_upsample_two_frames_and_a_dominant_logit(gpu):
    from videovanish_amd import hip
    Fr, h, w = 2, 8, 12
    coords1, mask = R.convex_inputs(Fr, h, w)
    sel = torch.arange(Fr * h * w)
    o = Guarded((Fr, 8 * h, 8 * w, 2), F32, gpu)
    hip.convex_upsample(coords1.to(gpu), mask.to(gpu), h, w, F=Fr, out=o.t)
    _close("convex_upsample", "convex_upsample:fp32", f"F {Fr}, {h} x {w}, one logit 80 above the rest", R.convex_gather(o.t, sel.to(gpu), Fr, h, w),
           R.convex_upsample(coords1, mask, sel, Fr, h, w), F32, o)


def _propagation(gpu, hip, d, label):
    H, W, _ = d["flow"].shape
    g = {k: v.to(gpu) for k, v in d.items()}
    o = Guarded((H, W), torch.uint8, gpu)
    hip.fb_valid(g["f_ab"], g["f_ba"], out=o.t)
    _exact("fb_valid", label, o.t, R.fb_valid(d["f_ab"], d["f_ba"])[0], o)
    cur, known, filled = Guarded((H, W, 3), F32, gpu, init=g["cur_t"]), Guarded((H, W), torch.uint8, gpu, init=g["known_t"]), Guarded((H, W), torch.uint8, gpu)
    hip.prop_fill(cur.t, g["cur_nb"], known.t, g["known_nb"], g["valid"], g["flow"], filled.t)
    rc, rk, rf, _ = R.prop_fill(d["cur_t"], d["cur_nb"], d["known_t"], d["known_nb"], d["valid"], d["flow"])
    _exact("prop_fill", f"{label}, filled", filled.t, rf, filled)
    _exact("prop_fill", f"{label}, known after the commit", known.t, rk, known)
    _exact("prop_fill", f"{label}, pixels", cur.t, rc, cur)
    return int(rf.sum())


def test_propagation_kernels_at_their_rounding_edges(gpu):
    from videovanish_amd import hip
    d = R.flow_edge_inputs()
    assert _propagation(gpu, hip, d, "9 x 13, flows on x.5, -0.5, W - 0.5 and far outside") > 10
    c = R.combine_inputs()
    g = {k: v.to(gpu) for k, v in c.items()}
    ro, rf = R.prop_combine(**c)
    assert {(int(a), int(b), int(hh)) for a, b, hh in zip(c["fa"].reshape(-1), c["fb"].reshape(-1), c["hole"].reshape(-1))} == {(a, b, hh) for a in (0, 1) for b in (0, 1) for hh in (0, 1)}
    assert int(ro.min()) == 0 and int(ro.max()) == 255
    out, filled = Guarded((9, 13, 3), torch.uint8, gpu), Guarded((9, 13), torch.uint8, gpu)
    hip.prop_combine(g["orig"], g["a"], g["b"], g["fa"], g["fb"], g["hole"], g["mean3"], out=out.t, filled=filled.t)
    _exact("prop_combine", "9 x 13, every A / B / hole branch, -0.75 and 255.6 before the clamp", out.t, ro, out)
    _exact("prop_combine", "9 x 13, filled", filled.t, rf, filled)
    out = Guarded((9, 13, 3), torch.uint8, gpu)
    assert hip.prop_combine(g["orig"], g["a"], g["b"], g["fa"], g["fb"], g["hole"], g["mean3"], out=out.t, want_filled=False)[1] is None
    _exact("prop_combine", "9 x 13, filled = NULL", out.t, ro, out)


def test_propagation_kernels_second_pass(gpu):
    from videovanish_amd import hip
    H = W = 2050                                 # 4 202 500 pixels = cap + 8196
    d = R.flow_edge_inputs(H, W, seed=91)
    _propagation(gpu, hip, d, f"{H} x {W}")
    c = R.combine_inputs(H, W, seed=92)
    g = {k: v.to(gpu) for k, v in c.items()}
    out, filled = Guarded((H, W, 3), torch.uint8, gpu), Guarded((H, W), torch.uint8, gpu)
    hip.prop_combine(g["orig"], g["a"], g["b"], g["fa"], g["fb"], g["hole"], g["mean3"], out=out.t, filled=filled.t)
    ro, rf = R.prop_combine(**c)
    _exact("prop_combine", f"{H} x {W}", out.t, ro, out)
    _exact("prop_combine", f"{H} x {W}, filled", filled.t, rf, filled)


# ================================================================================================================ edges at small shapes
def test_avgpool2_drops_an_odd_last_row_and_column(gpu):
    from videovanish_amd import hip
    x = R.randn(1, 3, 9, 13)
    o = Guarded((3, 4, 6), F32, gpu)
    hip.avgpool2(x.to(gpu), out=o.t)
    _exact("avgpool2", "3 x 9 x 13 -> 3 x 4 x 6", o.t, R.avgpool2(x), o)


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("S,lo", R.MASKDOWN)
@pytest.mark.parametrize("binarize", [True, False])
def test_sam2_maskdown_stage_by_stage_and_the_layer_by_layer_path(gpu, dname, S, lo, binarize):
    from videovanish_amd import hip, packing
    td, dt = R.TD[dname], hip.dtype_id(dname)
    tag = f"[{dname}] S {S}, lo {lo}, {'binarise' if binarize else 'sigmoid'}"
    logits, l1, l2 = R.maskdown_inputs(S, lo)
    dev = lambda ts: tuple(t.contiguous().to(gpu) for t in ts)
    H1, H2 = S // 2, S // 4
    m_ref, near = R.maskdown_input(logits, lo, S, binarize, R.MD_SCALE, R.MD_BIAS)
    keep = ~R.near_outputs(near)
    assert (~keep).float().mean().item() <= 0.005
    # the fused kernel: mid against fp64, out against the fp64 second stage run from the GPU's own mid
    mid, out = Guarded((H1 * H1, 8), td, gpu), Guarded((H2 * H2, 16), td, gpu)
    hip.sam2_maskdown(dt, logits.to(gpu), lo, S, binarize, R.MD_SCALE, R.MD_BIAS, dev(l1), dev(l2), eps=R.MD_EPS, mid=mid.t, out=out.t)
    ref_mid, _ = R.maskdown_stage(m_ref[..., None], *l1, R.MD_EPS, td)
    _close("sam2_maskdown", f"maskdown_mid:{dname}", f"{tag}, mid", mid.t[:, :4], ref_mid, td, mid, keep=keep)
    assert bool((mid.t[:, 4:] == 0).all()), "channels 4 .. 7 of mid must be zero"
    ref_out, _ = R.maskdown_stage(mid.t[:, :4].cpu().double().reshape(H1, H1, 4), *l2, R.MD_EPS, td)
    _close("sam2_maskdown", f"maskdown_out:{dname}", f"{tag}, out from the kernel's own mid", out.t, ref_out, td, out)
    # the layer-by-layer path of sam2_model.py on the same weights, each layer from the GPU's own input
    high = hip.resize_bilinear_f32(logits.reshape(lo * lo, 1).to(gpu), lo, lo, S, S)
    m = Guarded((S * S, 8), td, gpu)
    hip.mask_mem_input(dt, high, binarize, R.MD_SCALE, R.MD_BIAS, out=m.t)
    rm, _ = R.mask_mem_input(high.cpu().reshape(-1), binarize, R.MD_SCALE, R.MD_BIAS, F32 if binarize else F64)
    if binarize:
        _exact("mask_mem_input", f"{tag}", m.t[:, 0], rm.to(td), m)
    else:
        _close("mask_mem_input", f"mask_mem_sigmoid:{dname}", tag, m.t[:, 0], R.r16(rm, td), td, m)
    assert bool((m.t[:, 1:] == 0).all()), "channels 1 .. 7 of the memory-encoder input must be zero"
    # ... and against the SAME first step as the fused kernel (F.interpolate in fp64), stored as h16 as this path stores it
    m_ref16, _ = R.maskdown_input(logits, lo, S, binarize, R.MD_SCALE, R.MD_BIAS, td_m=td)
    if binarize:
        bad = int(((m.t[:, 0].cpu().double().reshape(S, S) != m_ref16) & ~near).sum())
        _log(f"aux mask_mem_input {tag}, against the fp64 upsampling: " + ("exact" if bad == 0 else f"{bad} elements differ"))
        assert bad == 0
    else:
        _close("mask_mem_input", f"mask_mem_sigmoid:{dname}", f"{tag}, against the fp64 upsampling", m.t[:, 0], m_ref16.reshape(-1), td, m)
    x, Hc = m.t, S
    stages = []
    for (w, b, ga, be), cout, key in ((l1, 4, "maskdown_mid"), (l2, 16, "maskdown_out")):
        wp, K = packing.pack_conv(w, td, 8)
        y = hip.conv_gemm(dt, x, wp.to(gpu), cout, K, F=1, Hin=Hc, Win=Hc, Hout=Hc // 2, Wout=Hc // 2, ksize=3, stride=2, pad_t=1, pad_l=1, bias=b.to(gpu), out_dtype=F32)
        o = Guarded((y.shape[0], max(8, cout)), td, gpu)
        hip.layernorm_ex(dt, y, ga.to(gpu), be.to(gpu), R.MD_EPS, act=hip.ACT_GELU, cpad=max(8, cout), out=o.t)
        cin = w.shape[1]
        ref, _ = R.maskdown_stage(x[:, :cin].cpu().double().reshape(Hc, Hc, cin), w, b, ga, be, R.MD_EPS, td)
        _close("sam2_maskdown", f"{key}:{dname}", f"{tag}, layer by layer, {cin} -> {cout} from its own input", o.t[:, :cout], ref, td, o)
        if cin == 1:          # the first stage also from the reference's mask input: the path as a whole meets the fp64 reference the fused kernel meets
            ref1, _ = R.maskdown_stage(m_ref16[..., None], w, b, ga, be, R.MD_EPS, td)
            _close("sam2_maskdown", f"{key}:{dname}", f"{tag}, layer by layer, 1 -> 4 from the fp64 mask input", o.t[:, :cout], ref1, td, keep=keep)
        stages.append(o.t[:, :cout].cpu().double())
        x, Hc = o.t, Hc // 2
    # the two paths against each other.  Each mid lies within B of its fp64 reference, and the references differ only by the h16 rounding of the mask input that the
    # layer-by-layer path stores (none with binarise: -10 and 10 are exact): limit = 2 B + max |stage(m) - stage(h16(m))|, all of it from the references
    B = R.bound(f"maskdown_mid:{dname}", td, ref_mid)
    limit = 2 * B + (ref_mid - R.maskdown_stage(m_ref16[..., None], *l1, R.MD_EPS, td)[0]).abs()[keep].max().item()
    gap = (stages[0] - mid.t[:, :4].cpu().double()).abs()[keep].max().item()
    _log(f"aux sam2_maskdown {tag}: fused mid against the layer-by-layer mid: max gap {gap:.3e} = {gap / R.U[td]:.2f} u = {gap / limit:.3f} of the limit {limit:.3e}")
    assert gap <= limit


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("C", R.LNX_C)
def test_layernorm_ex_every_form_and_padding(gpu, dname, C):
    from videovanish_amd import hip
    td, dt = R.TD[dname], hip.dtype_id(dname)
    x, g, b = R.ln_inputs(C)
    for cpad, a, oname in R.lnx_cases(C):
        od = F32 if oname == "fp32" else td
        o = Guarded((R.LNX_M, cpad), od, gpu)
        hip.layernorm_ex(dt, x.to(gpu), g.to(gpu), b.to(gpu), R.LNX_EPS, act=a, out_dtype=od, cpad=cpad, out=o.t)
        ref, gx = R.layernorm_ex(x, g, b, R.LNX_EPS, a, cpad)
        form = R.lnx_form(C, cpad)
        _close("layernorm_ex", f"layernorm_ex:{oname if oname == 'fp32' else dname}", f"[{dname}] C {C}, cpad {cpad}, act {a}, out {oname}, {'NCH = %d' % form if form else 'generic'}",
               o.t, R.r16(ref, None if od == F32 else td), od, o, gelu_x=gx if a == R.ACT_GELU else None)
        assert bool((o.t[:, C:] == 0).all()), "the padding columns must be zero"


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("C", [256, 772])
def test_layernorm_ex_rows_far_from_zero_and_constant_rows(gpu, dname, C):
    from videovanish_amd import hip
    td, dt = R.TD[dname], hip.dtype_id(dname)
    x, g, b = R.ln_inputs(C, offset=True)
    for oname, od in (("fp32", F32), (dname, td)):
        o = Guarded((R.LNX_M, C + 4), od, gpu)
        hip.layernorm_ex(dt, x.to(gpu), g.to(gpu), b.to(gpu), R.LNX_EPS, out_dtype=od, cpad=C + 4, out=o.t)
        ref, _ = R.layernorm_ex(x, g, b, R.LNX_EPS, cpad=C + 4)
        _close("layernorm_ex", f"layernorm_ex_offset:{oname}", f"[{dname}] C {C}, rows of mean 20 and std 1, two constant rows, out {oname}", o.t, R.r16(ref, None if od == F32 else td), od, o)


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("C", R.LN_C)
def test_layernorm_every_form_with_and_without_pe(gpu, dname, C):
    from videovanish_amd import hip
    td, dt = R.TD[dname], hip.dtype_id(dname)
    x, g, b = R.ln_inputs(C)
    pe = R.randn(C, 5, C)
    for p, tag in ((pe, "pe, rows_per_frame 2"), (None, "no pe")):
        o = Guarded((R.LNX_M, C), td, gpu)
        hip.layernorm(dt, x.to(gpu), g.to(gpu), b.to(gpu), pe=None if p is None else p.to(gpu), rows_per_frame=2, out=o.t)
        _close("layernorm", f"layernorm:{dname}", f"[{dname}] C {C} (NCH = {2 if C <= 512 else 5 if C <= 1280 else 8}), M 9, {tag}", o.t, R.r16(R.layernorm(x, g, b, p, 2), td), td, o)


@pytest.mark.parametrize("dname", ["fp32"] + DNAMES)
@pytest.mark.parametrize("n", R.ACT_N)
@pytest.mark.parametrize("kind", R.ACT_SETS)
def test_act_vector_and_scalar_forms(gpu, dname, n, kind):
    """n % 8 and the pointer's alignment choose between the 16-byte form and the scalar one: views 0, 2 and 16 bytes into an allocation.  Two input sets: values to
    +-30, and |x| <= 4 where B (proportional to max |ref|) is small enough to hold the h16 forms to the shape of each function near 0"""
    from videovanish_amd import hip
    td = F32 if dname == "fp32" else R.TD[dname]
    x = R.act_inputs(n, kind).to(td)
    for off in ([0, 4] if td == F32 else R.ACT_OFFS):
        form = "vector" if td != F32 and n % 8 == 0 and (off * 2) % 16 == 0 else "scalar"
        for a in R.ACT_LIST:
            buf = torch.full((GUARD + off + n + GUARD,), R.SENTINEL, dtype=td, device=gpu)
            view = buf[GUARD + off:GUARD + off + n]
            view.copy_(x)
            hip.act_inplace(view, a)
            assert bool((buf[:GUARD + off] == R.SENTINEL).all()) and bool((buf[GUARD + off + n:] == R.SENTINEL).all()), "vv_act wrote outside its n elements"
            _close("act", f"act:{dname}", f"[{dname}] n {n}, {kind} inputs, {off * x.element_size()} bytes in, act {a}, {form} form", view, R.r16(R.act(x, a), None if td == F32 else td), td,
                   gelu_x=x.abs().max().item() if a == R.ACT_GELU else None)


def test_leaky_relu_is_refused_where_there_is_no_slope(gpu):
    """vv_layernorm_ex and vv_act take no act_slope: VV_ACT_LRELU is an argument error, not a silent identity"""
    from videovanish_amd import hip
    x, g, b = (t.to(gpu) for t in R.ln_inputs(64))
    with pytest.raises(RuntimeError, match="vv_layernorm_ex"):
        hip.layernorm_ex(hip.F16, x, g, b, R.LNX_EPS, act=hip.ACT_LRELU)
    y = x.clone()
    with pytest.raises(RuntimeError, match="vv_act"):
        hip.act_inplace(y, hip.ACT_LRELU)
    assert torch.equal(y, x), "a refused launch must leave its operand alone"
    _log("aux act / layernorm_ex LRELU: refused with an argument error")


def test_select_clamp_and_add_rowvec_unless(gpu):
    from videovanish_amd import hip
    a, b = R.randn(1, 1003), R.randn(2, 1003)
    o = Guarded((1003,), F32, gpu)
    hip.clamp_f32(a.to(gpu), -0.5, 0.7, out=o.t)
    _exact("clamp_f32", "n 1003, [-0.5, 0.7]", o.t, R.clamp_f32(a, -0.5, 0.7), o)
    for flag in (0, 1):
        o = Guarded((1003,), F32, gpu)
        hip.select_f32(a.to(gpu), b.to(gpu), torch.tensor([flag], dtype=torch.int32, device=gpu), out=o.t)
        _exact("select_f32", f"flag {flag}", o.t, R.select_f32(a, b, flag), o)
    x, vec = R.randn(3, 37, 65), R.randn(4, 65)
    for score in (1.5, 0.0, -2.0, float("nan")):
        o = Guarded((37, 65), F32, gpu, init=x.to(gpu))
        hip.add_rowvec_unless(o.t, vec.to(gpu), torch.tensor([score], device=gpu))
        ref = R.add_rowvec_unless(x, vec, score)
        assert torch.equal(ref, x) == (score > 0)
        _exact("add_rowvec_unless", f"score {score}", o.t, ref, o)


def test_sam_select_on_the_edges_of_the_delta_band_and_at_the_stability_threshold(gpu):
    """values exactly on +-delta count for neither side; a stability score exactly at the threshold is stable (>=); an empty union is stable"""
    from videovanish_amd import hip
    HW, delta = 1003, 0.05
    iou = torch.tensor([0.1, 0.3, 0.9, 0.2])
    for ai, au, thresh, stable in R.SELECT_CASES:
        m = R.sam_select_inputs(HW, ai, au, delta)
        for multimask, obj in ((False, 1.0), (True, -0.5)):
            ref, near = R.sam_select(m, iou, obj, multimask, delta, thresh)
            assert not bool(near.any()) and int(ref[0]) == (2 if multimask or not stable else 0)
            o = Guarded((4,), torch.int32, gpu)
            hip.sam_select(m.to(gpu), iou.to(gpu), torch.tensor([obj], device=gpu), multimask, delta, thresh, out=o.t)
            _exact("sam_select", f"{ai} above delta, {au} above -delta of {HW}, thresh {thresh}, multimask {multimask}, object logit {obj}", o.t[:3], ref, o)


@pytest.mark.parametrize("dname", DNAMES)
def test_deform_im2col_raw_mode_against_fp64(gpu, dname):
    from videovanish_amd import hip
    td, dt = R.TD[dname], hip.dtype_id(dname)
    d = R.DEFORM
    x, raw, flow = R.deform_inputs()
    M = d["B"] * d["H"] * d["W"]
    for xin, xt in ((x, "fp32 x"), (x.to(td), f"{dname} x")):
        for fl, ft in ((flow, "with flow"), (None, "without flow")):
            o = Guarded((M, 9 * d["C"]), td, gpu)
            hip.deform_im2col(dt, xin.reshape(M, d["C"]).to(gpu), B=d["B"], H=d["H"], W=d["W"], deform_groups=d["dg"], raw=raw.to(gpu), flow=None if fl is None else fl.to(gpu),
                              max_residue=d["max_residue"], out=o.t)
            ref = R.r16(R.deform_raw(xin, raw, fl, d["max_residue"], d["dg"]), td)
            _close("deform_im2col", f"deform_raw:{dname}", f"[{dname}] raw mode, {xt}, {ft}, B 2, C 32, 9 x 13, dg 4", o.t, ref, td, o)


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("s2d,cpad", R.U8N)
def test_u8_normalize_zeroes_its_padding(gpu, dname, s2d, cpad):
    from videovanish_amd import hip
    td, dt = R.TD[dname], hip.dtype_id(dname)
    img = R.u8_image(8, 12)
    o = Guarded(((8 // s2d) * (12 // s2d), cpad), td, gpu)
    hip.u8_normalize(dt, img.to(gpu), R.U8N_MEAN, R.U8N_STD, cpad=cpad, s2d=s2d, out=o.t)
    _close("u8_normalize", f"u8_normalize:{dname}", f"[{dname}] 8 x 12, s2d {s2d}, cpad {cpad}", o.t, R.r16(R.u8_normalize(img, R.U8N_MEAN, R.U8N_STD, cpad, s2d), td), td, o)
    assert bool((o.t[:, 3 * s2d * s2d:] == 0).all()), "the padding channels must be zero"


@pytest.mark.parametrize("dname", DNAMES)
def test_split_forms_at_the_ends_of_the_h16_range(gpu, dname):
    """values in the fp16 subnormal range and at 65504; an h16 input is its own hi, so the lo group is exactly zero"""
    from videovanish_amd import hip
    td, dt = R.TD[dname], hip.dtype_id(dname)
    x = R.randn(1, 64, 8)
    x[0] = torch.tensor([65504.0, -65504.0, 65503.0, 2.0 ** -24, 3.3e-6, -5.1e-7, 2.0 ** -14, 6.1e-5])
    x[1] = x[0] * 0.5
    x[2] = torch.tensor([0.0, -0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12, 2.0 ** -25, 1e-8, -1e-8])
    hi, lo = Guarded((64, 8), td, gpu), Guarded((64, 8), td, gpu)
    hip.split_f32(dt, x.to(gpu), 1024.0, hi=hi.t, lo=lo.t)
    rh, rl = R.split_f32(x, 1024.0, td)
    _exact("split_f32", f"[{dname}] hi, subnormals and 65504", hi.t, rh.to(td), hi)
    _exact("split_f32", f"[{dname}] lo, subnormals and 65504", lo.t, rl.to(td), lo)
    for xin, tag in ((x, "fp32 in"), (x.to(td), f"{dname} in")):
        o = Guarded((64, 24), td, gpu)
        hip.split3(dt, xin.to(gpu), out=o.t)
        _exact("split3", f"[{dname}] {tag}, subnormals and 65504", o.t, R.split3(xin, td).to(td), o)
    assert bool((o.t[:, 8:16] == 0).all()), "an h16 input is its own hi: the lo group must be zero"
