"""tests/attnref.py (the fp64 restatement of the vv_attn_params contract) against torch, vv_attention_route over a table that pins every threshold of the
dispatcher on both sides, the product's attention shapes against the GPU case table, and the proof that the GPU cases are sharp: no GPU anywhere."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attnref as R  # noqa: E402
import test_attn_routes_gpu as G  # noqa: E402  (the case table; importing it touches no device)

DT = [("bf16", torch.bfloat16), ("fp16", torch.float16)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the reference against torch

def _sdpa(q, k, v, scale=None):
    return F.scaled_dot_product_attention(q.double(), k.double(), v.double(), scale=scale)


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _plain(B, heads, Nq, Nkv, D):
    """q / k / v [B][heads][N][D] and the keywords of the plain head-major layout"""
    q, k, v = _rand(B, heads, Nq, D, seed=1), _rand(B, heads, Nkv, D, seed=2), _rand(B, heads, Nkv, D, seed=3)
    kw = dict(B=B, heads=heads, Nq=Nq, Nkv=Nkv, D=D, q_bs=heads * Nq * D, k_bs=heads * Nkv * D, v_bs=heads * Nkv * D, q_rs=D, k_rs=D, v_rs=D,
              q_hs=Nq * D, k_hs=Nkv * D, v_hs=Nkv * D)
    return q, k, v, kw


def _close(a, b):
    # (1e-7, not 1e-12: the reference scales by the kernel's fp32 factor scale * log2(e), 6e-8 off the fp64 one)
    assert float((a - b).abs().max()) <= 1e-7 * max(1.0, float(b.abs().max()))


def test_ref_head_major_layout():
    q, k, v, kw = _plain(2, 3, 7, 5, 8)
    o, _ = R.attention_core(q, k, v, **kw)
    _close(o, _sdpa(q, k, v))


def test_ref_row_layout_with_offsets_in_a_fused_qkv_matrix():
    B, heads, N, D = 2, 3, 6, 8
    C = heads * D
    q, k, v, _ = _plain(B, heads, N, N, D)
    rows = torch.cat([t.permute(0, 2, 1, 3).reshape(B, N, C) for t in (q, k, v)], -1)                  # [B][N][3C]: q_hs = 0 means heads D apart inside a row
    pad = torch.cat([_rand(5, seed=4), rows.reshape(-1)])                                                # ... behind 5 foreign elements
    o, _ = R.attention_core(pad, pad, pad, B=B, heads=heads, Nq=N, Nkv=N, D=D, q_bs=N * 3 * C, k_bs=N * 3 * C, v_bs=N * 3 * C, q_rs=3 * C, k_rs=3 * C,
                            v_rs=3 * C, q_off=5, k_off=5 + C, v_off=5 + 2 * C)
    _close(o, _sdpa(q, k, v))


def test_ref_batch_stride_zero_shares_k_and_v():
    q, _, _, kw = _plain(3, 2, 4, 9, 8)
    k, v = _rand(1, 2, 9, 8, seed=5), _rand(1, 2, 9, 8, seed=6)
    o, _ = R.attention_core(q, k, v, **dict(kw, k_bs=0, v_bs=0))
    _close(o, _sdpa(q, k.expand(3, -1, -1, -1), v.expand(3, -1, -1, -1)))


def test_ref_temporal_gather():
    Fr, HW, heads, D = 5, 3, 2, 8
    C = heads * D
    x = _rand(Fr, HW, 3, heads, D, seed=7)
    q, k, v = (x[:, :, i].permute(1, 2, 0, 3) for i in range(3))                                          # [HW][heads][F][D]
    buf = x.reshape(-1)
    o, _ = R.attention_core(buf, buf, buf, B=HW, heads=heads, Nq=Fr, Nkv=Fr, D=D, q_bs=3 * C, k_bs=3 * C, v_bs=3 * C, q_rs=HW * 3 * C, k_rs=HW * 3 * C,
                            v_rs=HW * 3 * C, k_off=C, v_off=2 * C)
    _close(o, _sdpa(q, k, v))


def test_ref_q_hs_apart_from_k_hs():
    B, heads, Nq, Nkv, D = 1, 2, 4, 6, 8
    q, k, v, kw = _plain(B, heads, Nq, Nkv, D)
    qwide = torch.zeros(B, heads, Nq + 3, D, dtype=torch.float64)                                        # q heads Nq + 3 rows apart
    qwide[:, :, :Nq] = q
    o, _ = R.attention_core(qwide, k, v, **dict(kw, q_hs=(Nq + 3) * D, q_bs=heads * (Nq + 3) * D))
    _close(o, _sdpa(q, k, v))


def test_ref_output_placement_row_major_and_o_hs():
    B, heads, Nq, D = 2, 3, 4, 8
    C = heads * D
    o = _rand(B, heads, Nq, D, seed=8)
    kw = dict(B=B, heads=heads, Nq=Nq, D=D)
    row = R.place(o, 3 + B * Nq * (C + 8), o_bs=Nq * (C + 8), o_rs=C + 8, o_off=3, **kw)
    want = torch.full((B, Nq, C + 8), float("nan"), dtype=torch.float64)
    want[:, :, :C] = o.permute(0, 2, 1, 3).reshape(B, Nq, C)
    assert torch.equal(torch.nan_to_num(row[3:], nan=7.0), torch.nan_to_num(want.reshape(-1), nan=7.0)) and bool(row[:3].isnan().all())
    hm = R.place(o, B * (heads + 1) * Nq * D, o_bs=(heads + 1) * Nq * D, o_hs=Nq * D, o_rs=D, **kw).reshape(B, heads + 1, Nq, D)
    assert torch.equal(hm[:, :heads], o) and bool(hm[:, heads].isnan().all())


def test_ref_scale():
    q, k, v, kw = _plain(1, 2, 5, 7, 8)
    o, _ = R.attention_core(q, k, v, scale=0.2, **kw)
    assert float((o - _sdpa(q, k, v, scale=0.2)).abs().max()) <= 1e-7        # (the reference uses the kernel's fp32 factor scale * log2(e))


def test_ref_q_prescaled():
    q, k, v, kw = _plain(1, 2, 5, 7, 8)
    c = 8 ** -0.5 * R.LOG2E
    o, _ = R.attention_core(q * c, k, v, q_prescaled=True, scale=123.0, **kw)                             # scale is ignored then
    _close(o, _sdpa(q, k, v))


def test_ref_requant_rounds_the_scaled_operand_once_more():
    q, k, v, kw = _plain(1, 1, 5, 7, 8)
    q, k, v = (t.to(torch.bfloat16) for t in (q, k, v))
    o, _ = R.attention_core(q, k, v, requant=torch.bfloat16, **kw)
    q2 = (q.float() * (8 ** -0.5 * R.LOG2E)).to(torch.bfloat16)
    assert not torch.equal(q2.double(), q.double() * (8 ** -0.5 * R.LOG2E))
    assert float((o - _sdpa(q2, k, v, scale=math.log(2.0))).abs().max()) <= 1e-7


def test_ref_lse_is_log2_of_the_sum_of_exp2():
    q, k, v, kw = _plain(2, 2, 5, 7, 8)
    _, lse = R.attention_core(q, k, v, **kw)
    s = (q @ k.transpose(-1, -2)) * 8 ** -0.5
    assert float((lse - torch.logsumexp(s, -1) / math.log(2.0)).abs().max()) <= 1e-6


def test_ref_merge_of_split_keys_is_the_unsplit_attention():
    heads, Nq, Nkv, D, S = 2, 5, 12, 8, 3
    q, k, v, kw = _plain(1, heads, Nq, Nkv, D)
    whole, _ = R.attention_core(q, k, v, **kw)
    ch = Nkv // S
    kw = dict(kw, B=S, Nkv=ch, q_bs=0, k_bs=ch * D, v_bs=ch * D)                                          # the chunks as batches: head h of chunk s at s * ch * D + h * Nkv * D
    o, lse = R.attention_core(q, k, v, **kw)
    ld = heads * D + 8
    parts = torch.zeros(S, Nq, ld, dtype=torch.float64)
    parts[:, :, :heads * D] = o.permute(0, 2, 1, 3).reshape(S, Nq, heads * D)
    m = R.merge(parts, lse, S=S, heads=heads, Nq=Nq, D=D, ld=ld)
    _close(m, whole[0].permute(1, 0, 2).reshape(Nq, heads * D))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the route query

@pytest.fixture(scope="module")
def hip():
    from videovanish_amd import hip
    hip.lib()
    return hip


def _route(hip, D, Nq, Nkv, B=1, heads=1, dt=None, **kw):
    C = heads * D
    base = dict(B=B, heads=heads, Nq=Nq, Nkv=Nkv, D=D, q_bs=Nq * C, k_bs=Nkv * C, v_bs=Nkv * C, o_bs=Nq * C, q_rs=C, k_rs=C, v_rs=C, o_rs=C)
    base.update(kw)
    q, k, v, o = (base.pop(n, (1,)) for n in ("q", "k", "v", "o"))
    return hip.attention_route(hip.BF16 if dt is None else dt, q, k, v, o, **base)


S, S2, DMA, REG, W4, W8, V4, V8, M40, Q2, M80 = ("SHORT", "SHORT_2W", "DMA64", "REG80", "W4x32", "W8x16", "D512_W4", "D512_W8", "MFMA32_D40", "MFMA32_D40_Q2",
                                                 "MFMA32_D80")
CROSS, RAGGED = 1, 2
# (D, Nq, Nkv, B, heads) -> (route, flags): every threshold of the dispatcher on both sides
ROUTES = [
    # short: Nq 32 / 33 and Nkv 32 / 33
    ((32, 32, 32, 1, 1), (S, 0)), ((32, 33, 32, 1, 1), (DMA, CROSS)), ((32, 32, 33, 1, 1), (DMA, CROSS)), ((32, 33, 33, 1, 1), (DMA, 0)),
    ((80, 32, 32, 1, 1), (S, 0)), ((80, 33, 32, 1, 1), (REG, CROSS)), ((40, 32, 32, 1, 1), (S, 0)), ((40, 33, 33, 1, 1), (DMA, 0)),
    ((512, 32, 32, 1, 1), (V4, 0)),                                          # no short form at D = 512
    # D >= 128: Nq 16 / 17
    ((128, 16, 32, 1, 1), (S, 0)), ((128, 17, 32, 1, 1), (S2, 0)), ((160, 16, 16, 1, 1), (S, 0)), ((160, 17, 17, 1, 1), (S2, 0)),
    ((256, 16, 32, 1, 1), (S, 0)), ((256, 17, 32, 1, 1), (S2, 0)), ((80, 17, 32, 1, 1), (S, 0)), ((128, 33, 32, 1, 1), (W4, 0)),
    # D = 40: Nkv 63 / 64
    ((40, 63, 63, 1, 1), (DMA, 0)), ((40, 64, 64, 1, 1), (M40, 0)), ((40, 200, 63, 1, 1), (DMA, CROSS)),
    # cross: Nkv 127 / 128 with Nq != Nkv
    ((40, 200, 127, 1, 1), (DMA, CROSS)), ((40, 200, 128, 1, 1), (M40, 0)), ((40, 127, 127, 1, 1), (M40, RAGGED)),
    ((64, 200, 127, 1, 1), (DMA, CROSS)), ((64, 200, 128, 1, 1), (DMA, 0)), ((80, 200, 127, 1, 1), (REG, CROSS)), ((80, 200, 128, 1, 1), (REG, 0)),
    ((80, 600, 127, 1, 1), (REG, CROSS)), ((80, 600, 128, 1, 1), (M80, 0)),
    # D = 160 and D = 512: Nq 255 / 256
    ((160, 255, 255, 1, 1), (W4, 0)), ((160, 256, 256, 1, 1), (W8, 0)), ((160, 255, 77, 1, 1), (W4, 0)), ((160, 256, 77, 1, 1), (W8, 0)),
    ((512, 255, 255, 1, 1), (V4, 0)), ((512, 256, 256, 1, 1), (V8, 0)), ((128, 256, 256, 1, 1), (W4, 0)),
    # D = 80: Nq 511 / 512
    ((80, 511, 511, 1, 1), (REG, 0)), ((80, 512, 512, 1, 1), (M80, 0)), ((80, 512, 77, 1, 1), (REG, CROSS)),
    # D = 40: Nq 1023 / 1024
    ((40, 1023, 1023, 1, 1), (M40, RAGGED)), ((40, 1024, 1024, 1, 1), (Q2, 0)), ((40, 1024, 77, 1, 1), (DMA, CROSS)),
    # D = 256: 128 / 129 blocks of 128 queries
    ((256, 128, 64, 128, 1), (W8, 0)), ((256, 129, 64, 64, 1), (W8, 0)), ((256, 128, 64, 129, 1), (W4, 0)), ((256, 129, 64, 65, 1), (W4, 0)),
    ((256, 40, 65, 43, 3), (W4, 0)), ((256, 40, 65, 42, 3), (W8, 0)),
    # the ragged bit: Nkv % 64
    ((40, 200, 192, 1, 1), (M40, 0)), ((40, 200, 193, 1, 1), (M40, RAGGED)), ((40, 200, 255, 1, 1), (M40, RAGGED)), ((40, 2000, 256, 1, 1), (Q2, 0)),
    ((40, 2000, 257, 1, 1), (Q2, RAGGED)), ((80, 600, 640, 1, 1), (M80, 0)), ((80, 600, 641, 1, 1), (M80, RAGGED)),
]


def _name(hip, r):
    return hip.attn_route_name(r) if r > 0 else f"{r}: {hip.lib().vv_last_error().decode()}"


@pytest.mark.parametrize("shape,want", ROUTES, ids=[f"d{s[0]}-{s[1]}x{s[2]}-b{s[3]}h{s[4]}" for s, _ in ROUTES])
def test_route_table(hip, shape, want):
    D, Nq, Nkv, B, heads = shape
    for dt in (hip.BF16, hip.F16):
        r = _route(hip, D, Nq, Nkv, B, heads, dt=dt)
        assert r == (getattr(hip, "ATTN_ROUTE_" + want[0]) | want[1]), _name(hip, r)


def test_route_refusals_by_code(hip):
    E_ARG, E_UNSUPPORTED = -1, -2
    for D in (8, 48, 72, 96, 320, 1024):
        assert _route(hip, D, 64, 64) == E_UNSUPPORTED and b"not built" in hip.lib().vv_last_error()
    for name in ("q_rs", "k_rs", "v_rs", "q_bs", "k_bs", "v_bs", "q_hs", "k_hs", "v_hs"):
        assert _route(hip, 64, 100, 100, **{name: 64 * 100 + 4}) == E_ARG and b"multiples of 8" in hip.lib().vv_last_error(), name
    for name in ("o_rs", "o_bs", "o_hs"):
        assert _route(hip, 64, 100, 100, **{name: 64 * 100 + 2}) == E_ARG and b"multiple" in hip.lib().vv_last_error(), name
        assert _route(hip, 64, 100, 100, **{name: 64 * 100 + 4}) > 0, name                                 # o: 4 elements are enough
    assert _route(hip, 40, 100, 100, lse=(1,)) == E_UNSUPPORTED and b"lse" in hip.lib().vv_last_error()
    assert _route(hip, 40, 20, 20, lse=(1,)) == E_UNSUPPORTED                                              # ... on every D = 40 route
    assert _route(hip, 80, 600, 600, lse=(1,)) == hip.ATTN_ROUTE_MFMA32_D80 | RAGGED and _route(hip, 64, 100, 100, lse=(1,)) == hip.ATTN_ROUTE_DMA64
    for Nq, Nkv, B, heads in ((100, 100, 0, 1), (100, 100, 1, 0), (0, 100, 1, 1), (100, 0, 1, 1), (-1, 100, 1, 1)):
        assert _route(hip, 64, Nq, Nkv, B, heads) == E_ARG and b"empty" in hip.lib().vv_last_error(), (Nq, Nkv, B, heads)
    for ptr in "qkvo":
        assert _route(hip, 64, 100, 100, **{ptr: None}) == E_ARG and b"null" in hip.lib().vv_last_error()
    assert _route(hip, 64, 100, 100, dt=hip.F32) == E_ARG
    assert hip.lib().vv_attention_route(None, hip.BF16) == E_ARG


def test_route_query_takes_tensors_on_any_device(hip):
    t = torch.zeros(4, dtype=torch.bfloat16)
    assert _route(hip, 64, 100, 100, q=t, k=t, v=t, o=torch.empty(4, device="meta")) == hip.ATTN_ROUTE_DMA64


def test_route_names_are_distinct_and_only_for_route_codes(hip):
    names ={hip.attn_route_name(getattr(hip, "ATTN_ROUTE_" + r) | f) for r in G.KVT for f in (0, 1, 2)
             if not (f == 1 and r not in (DMA, REG)) and not (f == 2 and not r.startswith("MFMA32"))}
    assert len(names) == 11 + 2 + 3
    with pytest.raises(ValueError):
        hip.attn_route_name(hip.ATTN_ROUTE_SHORT | CROSS)


def test_profile_label_follows_the_route(hip):
    """the profile keys attention[spatial|cross|temporal,dD] (bench.py's kernel_times_s) are made from a copy of the short / cross rules in hip.py: over the
    route table and the GPU cases, label temporal <=> a SHORT* route for D < 512, and label cross <=> the cross kind where the route has one"""
    shapes = [s for s, _ in ROUTES] + [(c["D"], c["Nq"], c["Nkv"], c["B"], c["heads"]) for c in G.CASES]
    for D, Nq, Nkv, B, heads in shapes:
        r, label = _route(hip, D, Nq, Nkv, B, heads), hip.attention_label(Nq, Nkv)
        assert label in ("temporal", "cross", "spatial")
        if D < 512:
            assert (label == "temporal") == (r & ~15 in (hip.ATTN_ROUTE_SHORT, hip.ATTN_ROUTE_SHORT_2W)), (D, Nq, Nkv, label, _name(hip, r))
        if r & ~15 in (hip.ATTN_ROUTE_DMA64, hip.ATTN_ROUTE_REG80):
            assert (label == "cross") == bool(r & CROSS), (D, Nq, Nkv, label, _name(hip, r))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the product's shapes

def _product_shapes():
    """(what, D, Nq, Nkv, B, heads) of the vv_attention launches of the product at the 720p bench geometry (latent 90 x 160; 32 and 22 frames), from the
    configs: UNet spatial self / 77-key cross / temporal at every level that has them and the mid block, the VAE mid block, SAM 2's trunk and memory attention"""
    from videovanish_amd.config import UNetConfig, VAEConfig
    from videovanish_amd.sam2_config import Sam2Config, hiera_blocks
    from videovanish_amd.sam2_model import _HEAD_DIMS
    out = []
    u = UNetConfig()
    H, W = 720 // 8, 1280 // 8
    for Fr in (32, 22):
        h, w = H, W
        for lvl, ch in enumerate(u.block_out):
            D = ch // u.heads
            if u.attn_levels[lvl] or lvl == len(u.block_out) - 1:                  # the last level's resolution is the mid block's (which has attention)
                out.append((f"unet L{lvl} self F{Fr}", D, h * w, h * w, Fr, u.heads))
                out.append((f"unet L{lvl} cross F{Fr}", D, h * w, u.text_len, Fr, u.heads))
                out.append((f"unet L{lvl} temporal F{Fr}", D, Fr, Fr, h * w, u.heads))
            if lvl + 1 < len(u.block_out):
                h, w = (h + 1) // 2, (w + 1) // 2
    out.append(("vae mid", VAEConfig().block_out[-1], H * W, H * W, 4, 1))
    s = Sam2Config()
    blocks, _ = hiera_blocks(s)
    side = s.image_size // 4
    for i, L in enumerate(blocks):
        dp = min(d for d in _HEAD_DIMS if d >= L["dim_out"] // L["heads"])
        N = L["window"] ** 2 if L["window"] else side * side
        B = (side // L["window"]) ** 2 if L["window"] else 1
        out.append((f"sam2 trunk block {i}", dp, N // 4 if L["q_stride"] else N, N, B, L["heads"]))
        if L["q_stride"]:
            side //= 2
    n = s.feat_size ** 2
    out.append(("sam2 memory self (4 key chunks)", s.d_model, n, n // 4, 4, 1))
    out.append(("sam2 memory cross (4 key chunks)", s.d_model, n, s.num_maskmem * n // 4, 4, 1))
    return out


def test_every_product_shape_takes_a_route_of_the_gpu_case_table(hip):
    covered = {G.route_code(hip, c) for c in G.CASES}
    shapes = _product_shapes()
    assert len(shapes) > 30
    seen = set()
    for what, D, Nq, Nkv, B, heads in shapes:
        r = _route(hip, D, Nq, Nkv, B, heads)
        assert r > 0, (what, _name(hip, r))
        assert r in covered, (what, D, Nq, Nkv, hip.attn_route_name(r))
        seen.add(r & ~15)
    # the 720p product runs the forms the kernel tests used not to launch
    for form in (hip.ATTN_ROUTE_D512_W8, hip.ATTN_ROUTE_W8x16, hip.ATTN_ROUTE_MFMA32_D40_Q2, hip.ATTN_ROUTE_MFMA32_D80, hip.ATTN_ROUTE_SHORT_2W):
        assert form in seen, hip.attn_route_name(form)


def test_case_table_lists_every_route_and_two_layouts_each(hip):
    by_route = {}
    for c in G.CASES:
        by_route.setdefault(G.route_code(hip, c), set()).add(c["layout"])
    want = {getattr(hip, "ATTN_ROUTE_" + r) | f for r in G.KVT for f in (0, 1, 2) if not (f == 1 and r not in (DMA, REG)) and not (f == 2 and not r.startswith("MFMA32"))}
    assert set(by_route) == want
    assert all(len(l) >= 2 for l in by_route.values()), by_route
    assert {(c["B"], c["heads"]) for c in G.CASES} >= {(1, 1), (2, 3), (3, 8)}
    assert {l for ls in by_route.values() for l in ls} == set(R.LAYOUTS)
    for c in G.CASES:                                                             # the table's expectation is the dispatcher's answer (asserted again before each launch)
        assert _route(hip, c["D"], c["Nq"], c["Nkv"], c["B"], c["heads"]) == G.route_code(hip, c), c["id"]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# sharpness of the GPU cases, on the CPU

@pytest.mark.parametrize("dname,td", DT)
@pytest.mark.parametrize("c", G.CASES, ids=[c["id"] for c in G.CASES])
def test_gpu_case_is_sharp_and_leaves_the_kernel_room(dname, td, c):
    """On the case's own inputs four mutants of the reference -- the last key dropped, one guard key counted (both guard fills), keys KVT j - 1 and KVT j
    swapped in V only (the last two keys where there is one tile), the last query row written one row late -- each miss the case's check, and an h16 model
    of the kernel (P rounded to h16, fp32 sums, output rounded to h16) stays within HALF the bound."""
    cs = G.build(c, td, "nan")
    ref, _ = G.reference(c, cs, td)
    bound, _ = G.bounds(c, td, ref)
    Nq, Nkv = c["Nq"], c["Nkv"]
    assert float(ref.abs().max()) <= 1.0 + 1e-9
    rq = dict(requant=td) if c["mfma32"] and not c["q_prescaled"] else {}

    def missed(cs_, o, **kw):
        err, clobbered = R.check_output(cs_, R.written(cs_, o, **kw), ref)
        return not err <= bound or clobbered > 0

    model, _ = R.reference(cs, p_round=td, **rq)
    err, clobbered = R.check_output(cs, R.written(cs, model), ref)
    assert clobbered == 0 and err <= bound / 2, (err, bound)
    assert not missed(cs, ref)
    if Nkv > 1:
        assert missed(cs, R.reference(cs, Nkv=Nkv - 1, **rq)[0]), "last key dropped"
        v = cs.bufs[cs.names["v"]].clone()
        kw = cs.kw
        edges = list(range(cs.KVT, Nkv, cs.KVT)) or [Nkv - 1]
        Bk = 1 if kw["v_bs"] == 0 else kw["B"]
        for j in edges:
            a, b = (R.index(kw["v_off"], kw["v_bs"], kw["v_hs"], kw["v_rs"], Bk, kw["heads"], torch.tensor([r]), kw["D"]) for r in (j - 1, j))
            v[a], v[b] = cs.bufs[cs.names["v"]][b], cs.bufs[cs.names["v"]][a]
        assert missed(cs, R.reference(cs, v=v, **rq)[0]), "keys swapped in V"
    assert missed(cs, R.reference(cs, Nkv=Nkv + 1, **rq)[0]), "one guard key counted (nan fill)"
    ghost = G.build(c, td, "ghost")
    assert missed(ghost, R.reference(ghost, Nkv=Nkv + 1, **rq)[0]), "one guard key counted (ghost fill)"
    assert not missed(ghost, R.reference(ghost, **rq)[0])
    assert missed(cs, ref, row_shift={Nq - 1: Nq}), "last query row written one row late"
