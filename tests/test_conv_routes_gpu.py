"""vv_conv_gemm route by route against the fp64 reference of its contract (tests/convref.py), each case first tied to the kernel that runs by the
dispatcher's own answer (vv_conv_gemm_route): a case the query calls ineligible fails -- it would otherwise compare the fallback with itself.

  * forced forms on synthetic shapes: tile_hint 1 (128-row tiles), 2 (2-phase 256-row kernel) and 3 (8-phase, N % 256 == 0), CONV mode of the
    256-row kernels -- 3x3 with and without a concat split on a k-tile start, stride 2 with pad 1 / 0, 1x1 taking the CONV branch, 2x2, 1x5, 5x1,
    M < 256, ragged M % 256, frames smaller than a tile -- and every epilogue (bias, rowvec, res0 + res1 fp32 / h16, out_scale, RELU / LRELU, h16 /
    fp32 output, ldo > N through out_col);
  * the production shapes with tile_hint 0: UNet / BrushNet level-2 ResBlock convolutions at 720p (32 and 28 frames) and 1080p, which the
    dispatcher sends to the 256 x 320 CONV kernel;
  * every conv_gemm launch of real evaluations with the full-width fp16 model: one Denoiser evaluation at 720p F = 32, 720p F = 28 and 1080p
    F = 32, VAE encode + decode (precise decoder) at 720p -- checked rows of each launch, checked launches == launched launches;
  * the PROFILE label (bench.py's kernel_times_s keys) is the tile of the route that runs.

Bounds (the project's vv_conv_gemm kernel-test bounds, over the checked rows of one launch): fp32 output 3e-4 * max(1, max|ref|), h16 output
2 ulp * max|ref|.  fp32 accumulation over K <= 23 040 sits orders of magnitude below them; one 64-channel chunk dropped or misplaced at K = 23 040
moves outputs by ~ sqrt(64 / 23040) = 5 % of their rms, far above."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convref as R  # noqa: E402

pytestmark = pytest.mark.gpu
REPORT = os.environ.get("VV_PARITY_REPORT")
DT = [("bf16", torch.bfloat16), ("fp16", torch.float16)]
SENTINEL = 1000.0       # exact in bf16 and fp16: columns outside [out_col, out_col + N) must keep it


def _log(msg):
    print(msg)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(msg + "\n")


def _geometry(c):
    k, kw = c["k"], c.get("kw", c["k"])
    pt, pl, s = c.get("pt", k // 2), c.get("pl", kw // 2), c.get("stride", 1)
    Ho = c.get("Ho", (c["H"] + 2 * pt - k) // s + 1)
    Wo = c.get("Wo", (c["W"] + 2 * pl - kw) // s + 1)
    return k, kw, pt, pl, s, Ho, Wo


def _launch(gpu, dname, td, c, epi, seed, hint):
    """operands of case c with epilogue epi on the GPU -> (conv_gemm keyword arguments, weight, x0, K)"""
    from videovanish_amd import hip, packing
    g = torch.Generator(device=gpu).manual_seed(seed)
    k, kw, pt, pl, s, Ho, Wo = _geometry(c)
    Fr, H, W, C0, C1, N = c["F"], c["H"], c["W"], c["C0"], c.get("C1", 0), c["N"]
    M = Fr * Ho * Wo
    x0 = torch.randn(Fr, H, W, C0, device=gpu, generator=g).to(td)
    x1 = torch.randn(Fr, H, W, C1, device=gpu, generator=g).to(td) if C1 else None
    w = torch.randn(N, k, kw, C0 + C1, device=gpu, generator=g) * (k * kw * (C0 + C1)) ** -0.5
    K = k * kw * (C0 + C1)
    wp = packing.pack_matrix(w.reshape(N, K).cpu(), td).to(gpu)      # k = (ky * kw + kx) * Cin + c
    rdt = torch.float32 if epi.get("res") == "f32" else td
    odt = torch.float32 if epi.get("out") == "f32" else td
    kwargs = dict(x1=x1, F=Fr, Hin=H, Win=W, Hout=Ho, Wout=Wo, ksize=k, ksize_w=kw if kw != k else 0, stride=s, pad_t=pt, pad_l=pl,
                  bias=torch.randn(N, device=gpu, generator=g), out_scale=epi.get("scale", 1.0), act=epi.get("act", hip.ACT_NONE),
                  act_slope=0.2 if epi.get("act") == hip.ACT_LRELU else 0.0, tile_hint=hint)
    if epi.get("rowvec"):
        kwargs["rowvec"] = torch.randn(Fr, N, device=gpu, generator=g)
    if epi.get("res"):
        kwargs["res0"] = torch.randn(M, N, device=gpu, generator=g).to(rdt)
        if epi.get("res1", True):
            kwargs["res1"] = torch.randn(M, N, device=gpu, generator=g).to(rdt)
    col = epi.get("out_col", 0)
    kwargs["out"] = torch.full((M, N + col + epi.get("ldo_pad", 0)), SENTINEL, dtype=odt, device=gpu)
    kwargs["out_col"] = col
    return kwargs, wp, x0, K


def _check_rows(td, rows, x0, wp, N, K, kw, label):
    """compare the rows `rows` of the launch's output with conv_rows; returns (max error, bound)"""
    out = kw["out"]
    ref = R.conv_rows(td, rows, x0, wp, N, K, **kw)
    pos = R.out_positions(rows.cpu(), N, K, **kw).to(out.device)
    got = out.reshape(-1)[pos].double()
    tol = R.bound(ref, out.dtype, td)
    err = (got - ref).abs().max().item()
    assert torch.isfinite(got).all(), f"{label}: non-finite output"
    assert err <= tol, f"{label}: max error {err:.3e} > bound {tol:.3e}"
    return err, tol


def _expected(Npad, hint, route):
    from videovanish_amd import hip
    if hint == 1:
        return 0 < route < hip.ROUTE_256x320_LIN
    if hint == 2:
        return route == (hip.ROUTE_256x320_CONV if Npad % 320 == 0 else hip.ROUTE_256x256_CONV)
    return route == hip.ROUTE_256P8_CONV


# ---------------------------------------------------------------------------------------------------------------------------------------------
# forced forms, synthetic shapes
EPI = {
    "bias": dict(out="f32"),
    "rowvec+res f32": dict(out="f32", rowvec=True, res="f32"),
    "res h16, scale, h16 out": dict(out="h16", res="h16", scale=0.5),
    "lrelu, h16 out, ldo": dict(out="h16", act=3, out_col=16, ldo_pad=8),
    "relu, rowvec, ldo": dict(out="f32", act=2, rowvec=True, out_col=64),
    "res0 f32 (staged)": dict(out="f32", res="f32", res1=False),
    "res0 f32, h16 out, scale (staged)": dict(out="h16", res="f32", res1=False, scale=2.0),
}
CASES = [
    ("3x3 M<256", dict(F=2, H=9, W=13, C0=64, N=320, k=3), "bias"),
    ("3x3 M%256=100", dict(F=3, H=20, W=23, C0=128, N=256, k=3), "rowvec+res f32"),
    ("3x3 concat 64+64, frames < tile", dict(F=2, H=11, W=17, C0=64, C1=64, N=512, k=3), "res h16, scale, h16 out"),
    ("3x3 concat 640+1280", dict(F=1, H=6, W=7, C0=640, C1=1280, N=1280, k=3), "res0 f32 (staged)"),
    ("3x3 concat 1280+640", dict(F=2, H=5, W=9, C0=1280, C1=640, N=640, k=3), "lrelu, h16 out, ldo"),
    ("3x3 s2 p1", dict(F=2, H=17, W=30, C0=128, N=320, k=3, stride=2), "relu, rowvec, ldo"),
    ("3x3 s2 p0 (VAE downsample)", dict(F=2, H=20, W=26, C0=128, N=256, k=3, stride=2, pt=0, pl=0, Ho=10, Wo=13), "res0 f32, h16 out, scale (staged)"),
    ("1x1 s2", dict(F=2, H=14, W=22, C0=192, N=320, k=1, stride=2), "rowvec+res f32"),
    ("1x1 concat", dict(F=1, H=19, W=29, C0=128, C1=64, N=256, k=1), "res0 f32 (staged)"),
    ("2x2 p0", dict(F=3, H=12, W=15, C0=64, N=320, k=2, pt=0, pl=0), "res h16, scale, h16 out"),
    ("2x2 p1", dict(F=2, H=10, W=13, C0=64, N=256, k=2, pt=1, pl=1, Ho=10, Wo=13), "lrelu, h16 out, ldo"),
    ("1x5", dict(F=2, H=9, W=31, C0=64, N=320, k=1, kw=5, pt=0, pl=2), "bias"),
    ("5x1", dict(F=2, H=21, W=8, C0=128, N=512, k=5, kw=1, pt=2, pl=0), "relu, rowvec, ldo"),
    ("3x3 N=1280, 8 row tiles", dict(F=4, H=16, W=30, C0=64, N=1280, k=3), "res0 f32, h16 out, scale (staged)"),
]


@pytest.mark.parametrize("dname,td", DT)
@pytest.mark.parametrize("name,case,epi", CASES, ids=[c[0] for c in CASES])
def test_forced_forms_against_the_reference(gpu, dname, td, name, case, epi):
    """every row of every forced form against the fp64 reference; whether forms 2 / 3 are bit-equal to form 1 is logged, not asserted"""
    from videovanish_amd import hip
    dt = hip.dtype_id(dname)
    N = case["N"]
    hints = (1, 2) + ((3,) if N % 256 == 0 else ())
    outs = {}
    for hint in hints:
        kw, wp, x0, K = _launch(gpu, dname, td, case, EPI[epi], 100 + len(name), hint)
        route = hip.conv_gemm_route(dt, x0, wp, N, K, **kw)
        assert route > 0 and _expected(wp.shape[0], hint, route), f"{name} tile_hint {hint}: the dispatcher runs {hip.route_name(route) if route > 0 else route}"
        if hint >= 2:
            assert route >= hip.ROUTE_256x320_LIN and route & 1, "a CONV-mode 256-row route"
        hip.conv_gemm(dt, x0, wp, N, K, **kw)
        out = kw["out"]
        M = out.shape[0]
        col, width = kw["out_col"], out.shape[1]
        err, tol = _check_rows(td, torch.arange(M, device=gpu), x0, wp, N, K, kw, f"{name} [{dname}, hint {hint}]")
        outside = torch.cat([out[:, :col], out[:, col + N:]], 1)
        assert torch.equal(outside, torch.full_like(outside, SENTINEL)), f"{name} hint {hint}: columns outside [out_col, out_col + N) written"
        outs[hint] = out.clone()
        _log(f"conv_routes forced {name} [{dname}] {epi}: hint {hint} -> {hip.route_name(route)}, M {M} N {N} K {K}, max err {err:.3e} <= {tol:.3e}")
    for hint in hints[1:]:
        _log(f"conv_routes forced {name} [{dname}]: hint {hint} bit-equal to hint 1: {torch.equal(outs[hint], outs[1])}")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# production shapes, tile_hint 0: UNet / BrushNet level-2 ResBlock convolutions (nn.ResBlock: conv1 reads norm1's h16 output of Cin channels, bias =
# conv1 bias + time embedding, fp32 or h16 output; conv2 1280 -> 1280, the shortcut as res0 (fp32), res1 where the model passes one)
LEVEL2 = {"720p": (23, 40), "1080p": (34, 60)}
PROD = [("720p", 32), ("1080p", 32), ("720p", 28)]
LAYERS = [("conv1 640", 640, dict(out="f32")), ("conv1 1280", 1280, dict(out="h16")), ("conv1 2560", 2560, dict(out="f32")),
          ("conv1 1920", 1920, dict(out="f32")), ("conv2 res0", 1280, dict(out="f32", res="f32", res1=False)),
          ("conv2 res0+res1", 1280, dict(out="f32", res="f32"))]


def _tile_crossing_frame(Fr, HW):
    """a frame (not the first or last) whose rows cross a 256-row tile boundary in their interior"""
    for f in range(Fr // 2, Fr - 1):
        if (f * HW) // 256 != ((f + 1) * HW - 1) // 256 and (f * HW) % 256:
            return f
    raise AssertionError("no interior frame crosses a tile boundary")


@pytest.mark.parametrize("geo,frames", PROD, ids=[f"{g}-F{f}" for g, f in PROD])
def test_level2_resblock_convs_on_the_256x320_conv_kernel(gpu, geo, frames):
    from videovanish_amd import hip
    t0 = time.time()
    H, W = LEVEL2[geo]
    HW, M, N = H * W, frames * H * W, 1280
    fmid = _tile_crossing_frame(frames, HW)
    rows = torch.cat([torch.arange(f * HW, (f + 1) * HW) for f in (0, fmid, frames - 1)]).to(gpu)
    for i, (name, cin, epi) in enumerate(LAYERS):
        c = dict(F=frames, H=H, W=W, C0=cin, N=N, k=3)
        kw, wp, x0, K = _launch(gpu, "fp16", torch.float16, c, epi, 7 + i, 0)
        route = hip.conv_gemm_route(hip.F16, x0, wp, N, K, **kw)
        assert route == hip.ROUTE_256x320_CONV, f"{geo} F{frames} {name}: {hip.route_name(route) if route > 0 else route}"
        hip.conv_gemm(hip.F16, x0, wp, N, K, **kw)
        err, tol = _check_rows(torch.float16, rows, x0, wp, N, K, kw, f"{geo} F{frames} {name}")
        _log(f"conv_routes level2 {geo} F{frames} {name}: M {M} N {N} K {K} (M % 256 = {M % 256}, frames 0/{fmid}/{frames - 1}) -> "
             f"{hip.route_name(route)}, max err {err:.3e} <= {tol:.3e}")
        del kw, wp, x0
    torch.cuda.synchronize()
    _log(f"conv_routes level2 {geo} F{frames}: {time.time() - t0:.1f} s")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# every vv_conv_gemm launch of real evaluations at the benchmarked geometry: hip.conv_gemm wrapped (nn looks it up through the module on every call)

def _checked_rows(M, Fr, Hout, Wout, seed):
    """the rows checked of one launch: all rows of the first and last 256-row tile; in the first frame, the last frame and one frame whose rows cross a
    256-row boundary every row with m % 256 in {0, 127, 128, 255} and every image-edge pixel (images only: a linear launch is one column of rows);
    64 seeded random rows"""
    T = (M + 255) // 256
    sel = [torch.arange(0, min(256, M)), torch.arange((T - 1) * 256, M)]
    HW = Hout * Wout
    frames = {0, Fr - 1}
    for f in range(Fr // 2, Fr - 1):
        if f > 0 and (f * HW) // 256 != ((f + 1) * HW - 1) // 256:
            frames.add(f)
            break
    for f in sorted(frames):
        m = torch.arange(f * HW, (f + 1) * HW)
        sel.append(m[(m % 256 == 0) | (m % 256 == 127) | (m % 256 == 128) | (m % 256 == 255)])
        if Wout > 1:
            b = f * HW
            sel += [b + torch.arange(Wout), b + (Hout - 1) * Wout + torch.arange(Wout), b + torch.arange(Hout) * Wout, b + torch.arange(Hout) * Wout + Wout - 1]
    sel.append(torch.randint(0, M, (64,), generator=torch.Generator().manual_seed(seed)))
    return torch.unique(torch.cat(sel))


class LaunchChecker:
    """wraps hip.conv_gemm: before each launch the operands it reads are copied on the launch's stream (out may alias a residual), after it the checked
    rows are compared with conv_rows.  Counts the launches that reach the library (vv_conv_gemm) separately from the launches checked."""

    def __init__(self, monkeypatch, tag, route_at=None):
        from videovanish_amd import hip
        self.hip, self.tag, self.route_at = hip, tag, route_at
        self.real = hip.conv_gemm
        self.records, self.launched = [], 0
        lib = hip.lib()
        real_c = lib.vv_conv_gemm

        def counted(*a):
            self.launched += 1
            return real_c(*a)
        monkeypatch.setattr(lib, "vv_conv_gemm", counted)
        monkeypatch.setattr(hip, "conv_gemm", self)

    def __call__(self, dtype, x0, weight, N, K, **kw):
        hip = self.hip
        if kw.get("_route"):
            return self.real(dtype, x0, weight, N, K, **kw)
        route = hip.conv_gemm_route(dtype, x0, weight, N, K, **kw)
        if self.route_at is not None:
            self.route_at(dtype, x0, weight, N, K, kw, route)
        snap = {k: (v.clone() if isinstance(v, torch.Tensor) and k in ("x1", "bias", "rowvec", "res0", "res1") else v) for k, v in kw.items()}
        x0c = x0.clone()
        out = self.real(dtype, x0, weight, N, K, **kw)
        h16 = hip.h16(dtype)
        Fr, Hin, Win = kw.get("F", 1), kw.get("Hin", 1), kw.get("Win", 1)
        Hv, Wv = kw.get("Hv") or Hin, kw.get("Wv") or Win
        Hout, Wout = kw.get("Hout") or Hv, kw.get("Wout") or Wv
        M = Fr * Hout * Wout
        rows = _checked_rows(M, Fr, Hout, Wout, len(self.records)).to(out.device)
        snap["out"] = out
        ref = R.conv_rows(h16, rows, x0c, weight, N, K, **snap)
        pos = R.out_positions(rows.cpu(), N, K, **snap).to(out.device)
        got = out.reshape(-1)[pos].double()
        tol = R.bound(ref, out.dtype, h16)
        err = (got - ref).abs().max().item() if torch.isfinite(got).all() else float("inf")
        self.records.append(dict(M=M, N=N, K=K, route=route, err=err, tol=tol, rows=rows.numel()))
        _log(f"{self.tag} #{len(self.records)}: M {M} N {N} K {K} k{kw.get('ksize', 1)} -> {hip.route_name(route)}, rows {rows.numel()}, "
             f"max err {err:.3e} tol {tol:.3e}")
        return out

    def finish(self):
        """-> {route name: (launches, worst err / tol)}; asserts checked == launched and every launch within its bound"""
        hip = self.hip
        hist = {}
        for r in self.records:
            n, w = hist.get(hip.route_name(r["route"]), (0, 0.0))
            hist[hip.route_name(r["route"])] = (n + 1, max(w, r["err"] / r["tol"] if r["tol"] > 0 else (0.0 if r["err"] == 0 else float("inf"))))
        _log(f"{self.tag}: {len(self.records)} launches checked of {self.launched} launched; route histogram (launches, max err / tol):")
        for k in sorted(hist):
            _log(f"{self.tag}:   {k}: {hist[k][0]}, {hist[k][1]:.3f}")
        assert self.launched > 0 and len(self.records) == self.launched, f"{len(self.records)} launches checked, {self.launched} launched"
        bad = [r for r in self.records if not r["err"] <= r["tol"]]
        assert not bad, f"{len(bad)} launches over their bound, first: {bad[0]}"
        return hist


@pytest.fixture(scope="module")
def full_model(gpu):
    """the full-width fp16 Denoiser (UNet + BrushNet + motion modules) with seeded weights and the full VAE with the precise decoder, built once for the
    module (~45 s) and shared by the evaluations below"""
    from videovanish_amd.config import UNetConfig, VAEConfig
    from videovanish_amd.nn import Ctx
    from videovanish_amd.unet import Denoiser
    from videovanish_amd.vae import VAE
    ucfg = UNetConfig()
    ctx = Ctx("cuda:0", "fp16", 0)
    den = Denoiser(ctx, ucfg, ctx.src.normal("text_states", (1, ucfg.text_len, ucfg.cross_dim)))
    vae = VAE(ctx, VAEConfig(), precise_decoder=True)
    yield ctx, den, vae
    del den, vae
    torch.cuda.empty_cache()


EVALS = [("720p", 32), ("720p", 28), ("1080p", 32)]
LATENT = {"720p": (90, 160), "1080p": (135, 240)}


@pytest.mark.parametrize("geo,frames", EVALS, ids=[f"{g}-F{f}" for g, f in EVALS])
def test_every_launch_of_a_denoiser_evaluation(gpu, full_model, monkeypatch, geo, frames):
    """(a) / (b) / (c): one Denoiser evaluation (UNet + BrushNet + motion modules) at 720p F = 32, 720p F = 28 (ragged last row tile) and 1080p F = 32,
    every conv_gemm launch checked.  One stream (Denoiser.OVERLAP off): the same launches as the two-stream schedule, with the operand copies ordered."""
    from videovanish_amd import hip
    from videovanish_amd.unet import Denoiser
    ctx, den, _ = full_model
    monkeypatch.setattr(Denoiser, "OVERLAP", False)
    t0 = time.time()
    h, w = LATENT[geo]
    g = torch.Generator().manual_seed(frames)
    lat, cond = torch.randn(frames, h, w, 4, generator=g).to(gpu), torch.randn(frames, h, w, 4, generator=g).to(gpu)
    mask = torch.zeros(frames, h * 8, w * 8, dtype=torch.uint8)
    mask[:, h * 2:h * 5, w * 3:w * 6] = 255
    chk = LaunchChecker(monkeypatch, f"conv_routes eval {geo} F{frames}")
    with torch.no_grad():
        eps = den(lat, cond, mask.to(gpu), 501, frames, h, w, h * 8, w * 8)
    torch.cuda.synchronize()
    assert torch.isfinite(eps).all()
    hist = chk.finish()
    c256 = hip.route_name(hip.ROUTE_256x320_CONV)
    assert c256 in hist, "the level-2 convolutions take the 256 x 320 CONV kernel"
    if frames == 28:
        assert any(r["route"] == hip.ROUTE_256x320_CONV and r["M"] % 256 for r in chk.records), "a 256 x 320 CONV launch with a ragged last row tile"
    _log(f"conv_routes eval {geo} F{frames}: {time.time() - t0:.1f} s")


def test_every_launch_of_vae_encode_decode(gpu, full_model, monkeypatch):
    """(d): VAE encode + decode (precise decoder) at 720p on 4 frames -- the pipeline's VAE batch (pipeline.vae_batch), so these are the launches a
    32-frame chunk makes, batch by batch; each launch's route is also asserted equal to the route of the same launch over 32 frames."""
    from videovanish_amd import hip
    ctx, _, vae = full_model
    t0 = time.time()
    Fv, H, W = 4, 720, 1280

    def route_at(dtype, x0, weight, N, K, kw, route):
        k2 = dict(kw)
        Fr = kw.get("F", 1)
        if Fr == Fv:
            k2["F"] = 32
        else:                       # a linear layer over the rows of all frames (F = 1, Hin = M)
            assert Fr == 1 and kw.get("Win", 1) == 1 and kw["Hin"] % Fv == 0, f"launch geometry {Fr} x {kw.get('Hin')} x {kw.get('Win')}"
            k2["Hin"] = kw["Hin"] // Fv * 32
            if kw.get("split_tokens", 0) < 0:
                k2["split_tokens"] = -32
        if kw.get("out") is not None:
            o = kw["out"]
            k2["out"] = torch.empty((o.shape[0] // Fv * 32, o.shape[1]), dtype=o.dtype, device="meta")
        for r in ("res0", "res1"):
            if kw.get(r) is not None:
                k2[r] = torch.empty((kw[r].shape[0] // Fv * 32,) + tuple(kw[r].shape[1:]), dtype=kw[r].dtype, device="meta")
        r32 = hip.conv_gemm_route(dtype, x0, weight, N, K, **k2)
        assert r32 == route, f"route {hip.route_name(route)} at F = {Fv}, {hip.route_name(r32) if r32 > 0 else r32} at F = 32 (M {Fr * (kw.get('Hin'))})"

    g = torch.Generator().manual_seed(4)
    fr = torch.randint(0, 256, (Fv, H, W, 3), generator=g, dtype=torch.uint8)
    chk = LaunchChecker(monkeypatch, "conv_routes vae 720p F4", route_at=route_at)
    with torch.no_grad():
        img8, _ = hip.preprocess(ctx.dt, fr.to(gpu), None, want_masked=False)
        z = vae.encode(img8.view(Fv * H * W, 8), Fv, H, W)
        d = vae.decode(z.contiguous(), Fv, H // 8, W // 8)
    torch.cuda.synchronize()
    assert torch.isfinite(d).all()
    chk.finish()
    _log(f"conv_routes vae 720p F4: {time.time() - t0:.1f} s")


def test_profile_label_is_the_route(gpu, monkeypatch):
    """hip.conv_gemm's PROFILE key names the tile of the kernel that runs (vv_conv_gemm_route).  Regression: the Python mirror of the dispatch rules it
    replaces labelled a gn_partials launch the 256-row kernel would otherwise take "256x320"; gn_partials forces the 128 x 160 halo-tile kernel."""
    from videovanish_amd import hip
    monkeypatch.setattr(hip, "PROFILE", [])
    cases = [(dict(F=28, H=48, W=48, C0=640, N=640, k=3), dict(out="f32"), True, hip.ROUTE_HALO_GN, "conv_gemm[128x160,h16in,k3]"),
             (dict(F=28, H=48, W=48, C0=640, N=640, k=3), dict(out="f32"), False, hip.ROUTE_256x320_CONV, "conv_gemm[256x320,h16in,k3]"),
             (dict(F=2, H=23, W=40, C0=1280, N=1280, k=3), dict(out="f32"), False, hip.ROUTE_FAST9 + hip.ROUTE_TILE_128x160, "conv_gemm[128x160,h16in,k3]")]
    for i, (c, epi, gn, want_route, want_key) in enumerate(cases):
        kw, wp, x0, K = _launch(gpu, "fp16", torch.float16, c, epi, 50 + i, 0)
        route = hip.conv_gemm_route(hip.F16, x0, wp, c["N"], K, gn_partials=gn, **kw)
        assert route == want_route, hip.route_name(route)
        hip.conv_gemm(hip.F16, x0, wp, c["N"], K, gn_partials=hip.GNPartials(c["F"], kw["Hout"], kw["Wout"], c["N"], gpu) if gn else None, **kw)
        assert hip.PROFILE[-1][0] == want_key
    torch.cuda.synchronize()
