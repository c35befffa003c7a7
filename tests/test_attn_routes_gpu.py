"""Every vv_attention route (vv_attention_route: include/vvhip.h VV_ATTN_ROUTE_*) against the fp64 reference of tests/attnref.py at its tile edges,
in both operand types.  One table (CASES) holds every case; a case first asserts the route the dispatcher reports, then launches twice -- guard fill
"nan" (no lse) and guard fill "ghost" (with lse where the route writes one) -- and checks the output, that every other element of the output allocation
still holds the sentinel, and lse.  The inputs are attnref.edge_case: marker keys at 0, Nkv - 1 and both sides of every key-tile boundary, each the
dominant key of designated queries at the query-tile edges, so one key dropped, one key too many, two keys swapped or a row misplaced is an O(1) error;
tests/test_attnref_cpu.py proves that on the CPU for every case of this table, and that an h16 model of the kernels sits within half the bound.

Shapes whose route is not the one a reader of the shape might expect: the dispatcher's cross rule is Nkv < 128 && Nq != Nkv, so (100, 64), (100, 65),
(129, 127), (100, 40) at D <= 80 take the CROSS instantiation of DMA64 / REG80, and (1023, 64), (1024, 64), (1025, 65) at D = 40 and (513, 65), (600, 64)
at D = 80 take DMA64 / REG80 cross, not the 32x32x16 kernels.  They stay in the table under the route they take; (64, 64), (65, 65), (127, 127) put the
same key-tile edges on the SELF instantiations and (1023, 128), (1024, 128), (1025, 129), (513, 129), (600, 128) put the same query thresholds on the
32x32x16 kernels.

Bounds (the project's own): generic routes 4 u max(1, max|ref|) (test_attention_spatial); MFMA32_* routes 6 u max(1, max|ref|)
(test_attention_d40_lazy_reference_maximum; for both q_prescaled settings, the reference re-rounds the operand as the kernel does); lse
2 u + 2^-20 max(1, |ref|): the denominator is a sum of h16-rounded P of relative error <= u, so its log2 is off by <= u / ln 2 = 1.45 u, the second
term covers the fp32 rounding of the value; merged output 4 u max(1, max|ref|).  u = 2^-8 (bf16), 2^-11 (fp16).  max|ref| <= 1 by construction."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attnref as R  # noqa: E402

REPORT = os.environ.get("VV_PARITY_REPORT")
DT = [("bf16", torch.bfloat16), ("fp16", torch.float16)]

# route -> (key tile of the kernel body, writes lse)
KVT = {"SHORT": 32, "SHORT_2W": 32, "DMA64": 64, "REG80": 64, "W4x32": 64, "W8x16": 64, "D512_W4": 32, "D512_W8": 32, "MFMA32_D40": 64, "MFMA32_D40_Q2": 64,
       "MFMA32_D80": 64}
# (route, head dims, [(Nq, Nkv, flag)]): flag "s" / "c" = the self / cross kind of DMA64 and REG80, "w" / "r" = the whole / ragged bit of MFMA32_*, "" = none
TABLE = [
    ("SHORT", (32, 40, 64, 80), [(32, 32, ""), (22, 22, ""), (7, 31, ""), (1, 1, "")]),
    ("SHORT", (128, 160, 256), [(16, 32, ""), (5, 7, "")]),
    ("SHORT_2W", (128, 160, 256), [(17, 32, ""), (32, 32, ""), (22, 22, ""), (32, 9, "")]),
    ("DMA64", (32, 64), [(100, 64, "c"), (100, 65, "c"), (129, 127, "c"), (129, 128, "s"), (130, 129, "s"), (100, 40, "c"),
                         (64, 64, "s"), (65, 65, "s"), (127, 127, "s"), (40, 40, "s")]),
    ("DMA64", (40,), [(40, 40, "s"), (63, 63, "s"), (1023, 64, "c"), (1024, 64, "c"), (1025, 65, "c")]),
    ("DMA64", (32, 40, 64), [(129, 77, "c"), (300, 33, "c"), (64, 127, "c")]),
    ("REG80", (80,), [(100, 64, "c"), (130, 65, "c"), (129, 127, "c"), (511, 129, "s"), (100, 40, "c"), (64, 64, "s"), (65, 65, "s"), (127, 127, "s"),
                      (40, 40, "s"), (129, 77, "c"), (515, 77, "c"), (513, 65, "c"), (600, 64, "c")]),
    ("W4x32", (128,), [(33, 40, ""), (129, 64, ""), (130, 129, ""), (200, 77, "")]),
    ("W4x32", (160,), [(70, 70, ""), (255, 77, ""), (255, 129, "")]),
    ("W4x32", (256,), [(40, 65, "")]),                    # B = 43, heads = 3: a 129-block grid
    ("W8x16", (160,), [(256, 256, ""), (257, 77, ""), (300, 129, "")]),
    ("W8x16", (256,), [(200, 64, ""), (130, 129, "")]),
    ("D512_W4", (512,), [(33, 31, ""), (150, 33, ""), (255, 64, "")]),
    ("D512_W8", (512,), [(256, 32, ""), (290, 97, ""), (257, 65, "")]),
    ("MFMA32_D40", (40,), [(64, 64, "w"), (65, 65, "r"), (127, 127, "r"), (128, 128, "w"), (129, 129, "r"), (200, 300, "r"), (40, 128, "w"), (20, 200, "r"),
                           (1023, 128, "w")]),
    ("MFMA32_D40_Q2", (40,), [(1024, 128, "w"), (1025, 129, "r"), (1030, 193, "r"), (1088, 1088, "w")]),
    ("MFMA32_D80", (80,), [(512, 512, "w"), (513, 129, "r"), (600, 128, "w"), (520, 129, "r")]),
]
BH = [(2, 3), (3, 8), (1, 1)]
FLAGS = {"": 0, "s": 0, "c": 1, "w": 0, "r": 2}


def _cases():
    out, per_route = [], {}
    for route, dims, shapes in TABLE:
        for D in dims:
            for Nq, Nkv, flag in shapes:
                i = per_route.get(route, 0)
                per_route[route] = i + 1
                B, heads = BH[i % 3]
                if Nq * Nkv > 300000:
                    B, heads = (2, 3) if i % 2 else (1, 1)
                if route == "W4x32" and D == 256:
                    B, heads = 43, 3
                layouts = [l for l in R.LAYOUTS if l != "temporal" or (Nq == Nkv and B * heads * D * Nq < 400000)]
                layout = layouts[i % len(layouts)]
                mf = route.startswith("MFMA32")
                for pre in ((False, True) if mf else (i % 4 == 3,)):
                    out.append(dict(route=route, flag=flag, D=D, Nq=Nq, Nkv=Nkv, B=B, heads=heads, layout=layout, q_prescaled=pre,
                                    scale=0.7 * D ** -0.5 if i == 0 else None, mfma32=mf, lse=D != 40, seed=1000 + len(out),
                                    id=f"{route}{'-' + flag if flag else ''}-d{D}-{Nq}x{Nkv}-b{B}h{heads}-{layout}{'-pre' if pre else ''}"))
    return out


CASES = _cases()


def route_code(hip, c):
    return getattr(hip, "ATTN_ROUTE_" + c["route"]) | FLAGS[c["flag"]]


def build(c, td, fill):
    return R.edge_case(c["B"], c["heads"], c["Nq"], c["Nkv"], c["D"], KVT[c["route"]], td, c["seed"], layout=c["layout"], fill=fill, scale=c["scale"],
                       q_prescaled=c["q_prescaled"])


def reference(c, cs, td):
    """the fp64 reference of a case; the 32x32x16 routes without q_prescaled re-round their operand (attnref: requant)"""
    return R.reference(cs, requant=td if c["mfma32"] and not c["q_prescaled"] else None)


def bounds(c, td, ref):
    u = R.U[td]
    return (6 if c["mfma32"] else 4) * u * max(1.0, float(ref.abs().max())), u


def _log(msg):
    print(msg)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(msg + "\n")


@pytest.fixture(scope="module", autouse=True)
def wall_time_of_this_file():
    """logs what this file adds to -m gpu: from its first test to its last, whatever ran before it"""
    t0 = time.time()
    yield
    _log(f"attn_routes: {len(CASES)} cases x 2 operand types x 2 guard fills, wall time of the file {time.time() - t0:.1f} s")


@pytest.mark.gpu
@pytest.mark.parametrize("dname,td", DT)
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_route_against_fp64(gpu, dname, td, c):
    from videovanish_amd import hip
    dt = hip.dtype_id(dname)
    want = route_code(hip, c)
    ref = lse_ref = None
    for fill in ("nan", "ghost"):
        cs = build(c, td, fill)
        if ref is None:
            ref, lse_ref = reference(c, cs, td)
            bound, u = bounds(c, td, ref)
        dev = {n: b.to(gpu) for n, b in cs.bufs.items()}
        out = R.sentinel_buffer(cs).to(gpu)
        with_lse = c["lse"] and fill == "ghost"
        lse = torch.full((c["B"], c["heads"], c["Nq"]), float("nan"), dtype=torch.float32, device=gpu) if with_lse else None
        kw = R.launch_kw(cs)
        args = (dt, dev[cs.names["q"]], dev[cs.names["k"]], dev[cs.names["v"]], out[cs.kw["o_off"]:])
        route = hip.attention_route(*args, lse=lse, **kw)
        assert route == want, (hip.attn_route_name(route) if route > 0 else route, hip.attn_route_name(want))
        hip.attention(*args, lse=lse, **kw)
        err, clobbered = R.check_output(cs, out.cpu(), ref)
        msg = f"attn_routes {c['id']} [{dname}] {fill}: {hip.attn_route_name(route)}, gamma {cs.gamma:g}, err {err:.3e}, err/bound {err / bound:.3f}"
        if with_lse:
            lerr = (lse.cpu().double() - lse_ref).abs()
            lbound = 2 * u + 2.0 ** -20 * lse_ref.abs().clamp(min=1.0)
            lratio = float((lerr / lbound).max()) if bool(torch.isfinite(lerr).all()) else float("inf")
            msg += f", lse err {float(lerr.max()):.3e}, lse err/bound {lratio:.3f}"
        _log(msg + f", outside {clobbered}")
        assert clobbered == 0, f"{clobbered} elements outside the output were written"
        assert err <= bound, (err, bound)
        if with_lse:
            assert lratio <= 1.0, (float(lerr.max()), lratio)


@pytest.mark.gpu
@pytest.mark.parametrize("dname,td", DT)
@pytest.mark.parametrize("want,heads,Nq,Nkv,D,S", [("MFMA32_D80", 2, 640, 4 * 129, 80, 4), ("W8x16", 1, 300, 3 * 130, 256, 3), ("W4x32", 2, 100, 2 * 77, 128, 2)])
def test_split_kv_against_unsplit_fp64(gpu, dname, td, want, heads, Nq, Nkv, D, S):
    """hip.attention_split_kv (S chunks as S batches + vv_attention_merge) against the UNSPLIT fp64 reference; the chunk launch lands on `want`.  The marker
    keys sit where the chunk launch has its edges: the first and last key of every chunk and both sides of every 64-key boundary counted from the chunk's
    start.  The operands are handed over as plain [N][heads * D] matrices, as attention_split_kv takes them: guard rows and the sentinel are the table's
    business (test_route_against_fp64 runs the same kernels with B > 1), what is checked here is the split and the merge."""
    from videovanish_amd import hip
    dt = hip.dtype_id(dname)
    u = R.U[td]
    chunk = Nkv // S
    markers = [s * chunk + m for s in range(S) for m in R.marker_keys(chunk, 64)]
    cs = R.edge_case(1, heads, Nq, Nkv, D, 64, td, 77, layout="fused", fill="ghost", markers=markers)
    C = heads * D
    sel = lambda t: cs.bufs[cs.names[t]][R.index(cs.kw[t + "_off"], 0, 0, cs.kw[t + "_rs"], 1, 1, torch.arange(Nq if t == "q" else Nkv), C)].reshape(-1, C)
    q, k, v = (sel(t).contiguous().to(gpu) for t in "qkv")
    route = hip.attention_route(dt, q, k, v, (1,), B=S, heads=heads, Nq=Nq, Nkv=chunk, D=D, q_bs=0, k_bs=chunk * C, v_bs=chunk * C, o_bs=Nq * C, q_rs=C, k_rs=C, v_rs=C,
                                o_rs=C, lse=(1,))
    assert route & ~15 == getattr(hip, "ATTN_ROUTE_" + want), hip.attn_route_name(route)
    out = torch.empty(Nq, C, dtype=td, device=gpu)
    hip.attention_split_kv(dt, q, k, v, out, heads=heads, Nq=Nq, Nkv=Nkv, D=D, S=S, q_rs=C, k_rs=C, v_rs=C, o_rs=C)
    ref, _ = R.reference(cs, requant=td if want.startswith("MFMA32") else None)
    ref = ref[0].permute(1, 0, 2).reshape(Nq, C)
    err, bound = float((out.cpu().double() - ref).abs().max()), 4 * u * max(1.0, float(ref.abs().max()))
    _log(f"attn_routes split_kv d{D} {Nq}x{Nkv} S{S} [{dname}]: {hip.attn_route_name(route)}, err {err:.3e}, err/bound {err / bound:.3f}")
    assert err <= bound, (err, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("dname,td", DT)
@pytest.mark.parametrize("S", [1, 3, 4])
def test_merge_alone(gpu, dname, td, S):
    """vv_attention_merge against its fp64 reference: ld > heads * D, lse spread over +-60 between the parts; columns past heads * D keep their sentinel"""
    from videovanish_amd import hip
    dt = hip.dtype_id(dname)
    heads, Nq, D, ld = 3, 37, 40, 3 * 40 + 8
    g = torch.Generator().manual_seed(5 + S)
    parts = (torch.rand(S, Nq, ld, generator=g) * 2 - 1).to(td)
    lse = (torch.rand(S, heads, Nq, generator=g) * 120 - 60).float()
    lse[:, :, ::5] = lse[:1, :, ::5] + torch.rand(S, heads, (Nq + 4) // 5, generator=g)       # ... and some queries whose parts weigh alike
    out = torch.full((Nq, ld), R.SENTINEL, dtype=torch.int16).view(td).to(gpu)
    pd, ld_ = parts.to(gpu), lse.to(gpu)
    rc = hip.lib().vv_attention_merge(pd.data_ptr(), ld_.data_ptr(), S, heads, Nq, D, ld, out.data_ptr(), dt, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    got = out.cpu()
    ref = R.merge(parts, lse, S=S, heads=heads, Nq=Nq, D=D, ld=ld)
    err, bound = float((got[:, :heads * D].double() - ref).abs().max()), 4 * R.U[td] * max(1.0, float(ref.abs().max()))
    _log(f"attn_routes merge S{S} [{dname}]: err {err:.3e}, err/bound {err / bound:.3f}")
    assert err <= bound, (err, bound)
    assert bool((got[:, heads * D:].contiguous().view(torch.int16) == R.SENTINEL).all())
