"""Seam detail matching on the CPU: the settings, the binding of include/detailmatch.h, the product's integer fit against the restatement's
fractions, the invariants of the restated rules (tests/detailmatch_ref.py), the rule on the synthetic clips, infill.finish with the device
functions replaced by the restatements, configuration and CLI."""
import ctypes
import dataclasses
import inspect
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abiref  # noqa: E402
import deflicker_ref as FR  # noqa: E402
import detailmatch_ref as R  # noqa: E402
import seamblend_ref as BR  # noqa: E402
import tonematch_ref as TR  # noqa: E402

from videovanish_amd import detailmatch as M  # noqa: E402
from videovanish_amd.detailmatch import DetailMatchConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFS1 = np.zeros((1, 2), np.int32)


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_spellings_and_config():
    assert M.SPELLINGS == ("on",)
    for off in (None, False, "off", "none", "", " OFF "):
        assert M.as_config(off) is None
    d = DetailMatchConfig()
    assert dataclasses.asdict(d) == R.DEFAULTS
    assert M.as_config("on") == M.as_config(" On ") == M.as_config(True) == d
    assert M.as_config("ring=8,edge=12,smooth=2,min_pixels=256,max_sharpen=2.0,max_soften=1.0,dead=0.06,overshoot=4,strength=1.0") == d
    assert M.as_config(" ring = 32 , edge=255,smooth=16,min_pixels=2147483647,max_sharpen=4,max_soften=1,dead=1,overshoot=255,strength=1 ") == \
        DetailMatchConfig(32, 255, 16, 2 ** 31 - 1, 4.0, 1.0, 1.0, 255, 1.0)
    assert M.as_config("ring=1,edge=0,smooth=0,min_pixels=1,max_sharpen=0,max_soften=0,dead=0,overshoot=0,strength=0") == DetailMatchConfig(1, 0, 0, 1, 0.0, 0.0, 0.0, 0, 0.0)
    assert M.as_config("strength=0.5").strength == 0.5 and M.as_config("edge=20") == DetailMatchConfig(edge=20)
    cfg = DetailMatchConfig(ring=4)
    assert M.as_config(cfg) is cfg
    with pytest.raises(Exception):
        cfg.ring = 5                                                                                 # frozen
    for bad in ("yes", "sharpen", "ring", "ring=", "ring=x", "ring=-3", "ring=1.5", "ring=3,ring=4", "size=3", "ring=3;edge=1", "ring=0", "ring=33",
                "edge=256", "edge=-1", "smooth=17", "min_pixels=0", "min_pixels=2147483648", "max_sharpen=4.5", "max_sharpen=-1", "max_soften=1.5",
                "dead=1.5", "dead=-0.1", "overshoot=256", "overshoot=1.5", "strength=1.5", "strength=-0.1", "strength=nan", "strength=inf", "on,ring=3",
                "ring=3,", "mode=luma", 3, 1.0, ("on",)):
        with pytest.raises(ValueError):
            M.as_config(bad)
    with pytest.raises(ValueError, match="'on', 'off', 'ring=N,edge=N,smooth=N,min_pixels=N,max_sharpen=X,max_soften=X,dead=X,overshoot=N,strength=X'"):
        M.as_config("sometimes")
    for kw in (dict(ring=0), dict(ring=33), dict(ring=4.0), dict(ring=True), dict(edge=256), dict(edge="12"), dict(smooth=-1), dict(smooth=17),
               dict(min_pixels=0), dict(min_pixels=2 ** 31), dict(max_sharpen=4.01), dict(max_sharpen=None), dict(max_soften=1.01), dict(max_soften=-0.5),
               dict(dead=-0.01), dict(dead=float("nan")), dict(overshoot=-1), dict(overshoot=256), dict(overshoot=4.0), dict(strength=1.01), dict(strength="1")):
        with pytest.raises(ValueError):
            DetailMatchConfig(**kw)
    assert "build-defined" in DetailMatchConfig.__doc__ and "nobody has run real checkpoints through it" in DetailMatchConfig.__doc__
    # the caps keep every amount inside the kernel's limit
    assert M.q8_of(4) == M.MAX_AMOUNT == 1024 and M.q8_of(0.06) == 15 and M.q8_of(1.0) == 256 and M.q8_of(0) == 0


# ---- binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_detailmatch_header():
    """detailmatch_bind.SIGNATURES declares every function of include/detailmatch.h with the header's types and in its order, lib() has applied
    it, the version and the limits agree (abiref.check_binding); the arguments are refused before any device work, each refusal naming its
    function; the vvd_ prefix and every name belong to no part of abiref.parts() (what test_abi_cpu.py's walk does for the parts of its table)."""
    from videovanish_amd import detailmatch_bind as B
    loaded, define = abiref.check_binding(B, 4)
    assert B.EXPORTS == ["vvd_abi_version", "vvd_last_error", "vvd_ring_detail_stats", "vvd_sharpen"] and define("VVD_ABI_VERSION") == 1
    assert (define("VVD_MAX_RING"), define("VVD_MAX_EDGE"), define("VVD_MAX_OVERSHOOT"), define("VVD_MAX_AMOUNT"), define("VVD_MAX_PIXELS"), define("VVD_NQ"),
            define("VVD_NSUM")) == (B.MAX_RING, B.MAX_EDGE, B.MAX_OVERSHOOT, B.MAX_AMOUNT, B.MAX_PIXELS, B.NQ, B.NSUM) == \
        (M.MAX_RING, M.MAX_EDGE, M.MAX_OVERSHOOT, M.MAX_AMOUNT, M.MAX_PIXELS, M.NQ, M.NSUM) == (32, 255, 255, 1024, 1 << 24, 4, 12)
    raw = open(os.path.join(ROOT, "include", "detailmatch.h")).read()
    for formula in ("H(I)(p) = 16 I(p) -", "a = (8192 P + Q) // (2 Q)", "(4096 x_c + a_t H(x_c)(p) + 2048) >> 12", "lo_c - overshoot, hi_c + overshoot",
                    "2^24 * 73440^2 < 2^57 < 2^63", "1. Statistic", "2. Fit", "3. Apply"):
        assert formula in raw, formula                                                               # the rules are part of the ABI
    # Nothing can be launched here: every pointer is host memory and every call below is refused before the first device call.
    buf = (ctypes.c_char * 64)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 32
    stats = lambda patch=a, orig=a, mask=a, offs=a, sums=a, Hm=4, Wm=4, T=1, H0=8, W0=8, h=4, w=4, ring=4, edge=12: \
        loaded.vvd_ring_detail_stats(patch, Hm, Wm, orig, mask, offs, T, H0, W0, h, w, ring, edge, sums, None)
    sharp = lambda patch=a, amount=a, out=b, Hm=4, Wm=4, T=1, h=4, w=4, overshoot=4: loaded.vvd_sharpen(patch, Hm, Wm, amount, T, h, w, overshoot, out, None)
    for kw in (dict(patch=None), dict(orig=None), dict(mask=None), dict(offs=None), dict(sums=None), dict(Hm=0), dict(Wm=-1), dict(T=0), dict(H0=0), dict(W0=0),
               dict(h=0), dict(w=0), dict(h=9), dict(w=9)):
        assert stats(**kw) == -1 and loaded.vvd_last_error().startswith(b"vvd_ring_detail_stats:"), kw
    for kw in (dict(ring=0), dict(ring=33), dict(edge=-1), dict(edge=256), dict(H0=4097, W0=4096, h=4097, w=4096), dict(H0=1 << 15, W0=1 << 15, h=1 << 15, w=1 << 15)):
        assert stats(**kw) == -2 and loaded.vvd_last_error().startswith(b"vvd_ring_detail_stats:"), kw
    assert stats(ring=0, T=0) == -1                                                                  # a bad argument before an unsupported one
    assert b"2^24" in (stats(H0=4097, W0=4096, h=4097, w=4096), loaded.vvd_last_error())[1]
    for kw in (dict(patch=None), dict(amount=None), dict(out=None), dict(Hm=0), dict(Wm=0), dict(T=0), dict(T=-1), dict(h=0), dict(w=-2), dict(out=a)):
        assert sharp(**kw) == -1 and loaded.vvd_last_error().startswith(b"vvd_sharpen:"), kw
    assert b"out is not patch" in loaded.vvd_last_error()                                            # never in place
    for kw in (dict(overshoot=-1), dict(overshoot=256), dict(h=4097, w=4096)):
        assert sharp(**kw) == -2 and loaded.vvd_last_error().startswith(b"vvd_sharpen:"), kw
    with pytest.raises(ctypes.ArgumentError):
        sharp(overshoot=2.0)
    import torch
    z, m = torch.zeros((2, 4, 4, 3), dtype=torch.uint8), torch.zeros((2, 4, 4), dtype=torch.uint8)
    offs, amount = torch.zeros((2, 2), dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for call in (lambda: B.ring_detail_stats(z, z, m, offs, 4, 4, 8, 12), lambda: B.sharpen(z, amount, 4, 4, 4), lambda: B.ring_detail_stats(z, z, None, offs, 4, 4, 8, 12)):
        with pytest.raises(RuntimeError):                                                            # no CPU fallback
            call()
    # the part stands outside abiref.PARTS: its prefix, header and names are checked against every part here
    assert "detailmatch_bind" not in abiref.PARTS and abiref.part_of(B) is B.PART and B.PART.header == "detailmatch.h"
    assert re.fullmatch(r"vv[a-z]_", B.PART.prefix)
    from videovanish_amd import platetone_bind
    names = set(B.SIGNATURES)
    for module, part in abiref.parts() + [(platetone_bind, platetone_bind.PART)]:
        assert part.prefix != B.PART.prefix and part.header != B.PART.header, module.__name__
        assert not names & set(module.SIGNATURES), module.__name__
        assert not [n for n in module.SIGNATURES if n.startswith(B.PART.prefix)], module.__name__
    assert all(n.startswith("vvd_") for n in names)


def test_product_sources_of_the_feature():
    """The kernels live in a unit of their own, in the one recipe with the header among the dependencies; no environment; the ring and the window's
    pixel are the shared statements, the 5 x 5 gate is the unit's own; the settings import no torch; importing the drop-in and asking for the
    setting resolves no vvd_ symbol."""
    kernel, txt = abiref.check_sources("vv_detail", "detailmatch.h", "detailmatch")
    for fn in ("vvd_ring_detail_stats", "vvd_sharpen"):
        assert f'extern "C" int {fn}(' in kernel
    for shared in ('#include "vv_ring_bits.h"', '#include "vv_paste_px.h"', '#include "vv_wave_bytes.h"', "vvring::ring_bits<false>(", "window_px(", "wave_sum64(",
                   "store_px<VEC>("):
        assert shared in kernel, shared
    ring = open(os.path.join(abiref.CSRC, "vv_ring_bits.h")).read()
    assert "near[j - (r - 1)]" in ring and "wide" not in ring                                        # the shared header keeps its radius-1 `near`
    assert "import ctypes" not in txt
    code = ("import diffuerase; from videovanish_amd import detailmatch_bind, tone_hip, hip; "
            "assert detailmatch_bind.PART.dll is None and tone_hip.PART.dll is None and hip.CORE.dll is None; "
            "assert diffuerase.detail_match_config() is None and diffuerase.last_detail_match is None")
    env = {k: v for k, v in os.environ.items() if k != "VV_DETAIL_MATCH"}
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)


# ---- the fit --------------------------------------------------------------------------------------------------------------------------------
def _row(count, P, Q, DD=0):
    """One frame's sums with everything in channel 0 but the count, which is spread (rule 2 pools the channels)."""
    return [count - 2 * (count // 3), P, Q, DD, count // 3, 0, 0, 0, count // 3, 0, 0, 0]


def test_the_fit_rounds_half_up_and_respects_caps_dead_zone_and_support():
    cfg = DetailMatchConfig(smooth=0, min_pixels=1)
    one = lambda P, Q, count=3, **kw: M.amount_q8(P, Q, count, dataclasses.replace(cfg, **kw))
    # a = floor(4096 P / Q + 1/2): ties go up, also below zero
    assert one(1, 8192) == (0, False, True)                                                          # 0.5 -> 1, inside the dead zone
    assert one(1, 8192, dead=0.0) == (1, False, False) and one(-1, 8192, dead=0.0) == (0, False, False)      # -0.5 -> 0
    assert one(3, 8192, dead=0.0)[0] == 2 and one(-3, 8192, dead=0.0)[0] == -1                       # 1.5 -> 2, -1.5 -> -1
    assert one(100, 4096)[0] == 100 and one(-100, 4096)[0] == -100 and one(99, 4096 * 2, dead=0.0)[0] == 50
    # caps, by integer comparison on the q8
    assert one(600, 4096) == (512, True, False) and one(512, 4096) == (512, False, False) and one(-300, 4096) == (-256, True, False)
    assert one(5000, 4096, max_sharpen=4.0) == (1024, True, False) and one(-5000, 4096, max_soften=0.5) == (-128, True, False)
    assert one(600, 4096, max_sharpen=0.0) == (0, True, True) and one(-600, 4096, max_soften=0.0) == (0, True, True)
    # the dead zone: |a| < q(dead)
    assert one(14, 4096) == (0, False, True) and one(15, 4096) == (15, False, False) and one(-14, 4096) == (0, False, True) and one(-15, 4096)[0] == -15
    # strength, after the clamp: (a q(strength) + 128) >> 8, an arithmetic shift
    assert one(100, 4096, strength=0.5)[0] == 50 and one(-100, 4096, strength=0.5)[0] == -50 and one(101, 4096, strength=0.5)[0] == 51
    assert one(-101, 4096, strength=0.5)[0] == -50 and one(600, 4096, strength=0.0) == (0, True, False)
    # support and Q = 0
    assert one(100, 4096, count=3 * 256 - 1, min_pixels=256) == (0, False, False) and one(100, 4096, count=3 * 256, min_pixels=256)[0] == 100
    assert one(100, 0) == (0, False, False)
    # the product against the restatement in fractions, pooled over frames
    rng = np.random.default_rng(3)
    s = np.stack([_row(int(rng.integers(0, 900)), int(rng.integers(-10 ** 12, 10 ** 12)), int(rng.integers(1, 10 ** 13)), int(rng.integers(0, 10 ** 9))) for _ in range(40)])
    s[5] = 0
    s[11, 2] = 0
    for kw in ({}, dict(smooth=0), dict(smooth=4, min_pixels=900), dict(dead=0.0, strength=0.3), dict(max_sharpen=0.5, max_soften=0.25), dict(min_pixels=1, max_sharpen=4.0)):
        f = M.fit(s, DetailMatchConfig(**kw))
        amounts, clamped, dead = R.fit(s, **dict(R.DEFAULTS, **kw))
        assert M.q8(f.amount).tolist() == amounts and f.clamped.tolist() == clamped and f.dead.tolist() == dead, kw
        assert f.amount.dtype == np.float64 and M.q8(f.amount).dtype == np.int32 and np.abs(M.q8(f.amount)).max() <= 1024
        assert (f.n == s[:, [0, 4, 8]].sum(1) // 3).all() and f.n.dtype == np.int64 and f.n[5] == 0 and f.residual[5] == 0.0
        assert np.allclose(f.residual[f.n > 0], (s[:, 3] / np.maximum(f.n, 1))[f.n > 0], rtol=1e-12, atol=0)
    assert len(set(amounts)) > 20 and min(amounts) == -256 and max(amounts) > 256 and any(clamped)   # the last setting: fits of both signs, the soften cap
    assert M.fit(np.zeros((0, 12), np.int64), cfg).amount.shape == (0,)
    # the largest sums rule 1 allows stay exact
    big = M.fit([_row(3 << 24, -(1 << 24) * 6120 * 73440, (1 << 24) * 73440 ** 2)], DetailMatchConfig(min_pixels=1))
    assert M.q8(big.amount).tolist() == [-256] and big.clamped.tolist() == [True]                    # 4096 * -6120 / 73440 = -341.3


# ---- the restated rules: invariants ---------------------------------------------------------------------------------------------------------
def test_restatement_invariants():
    """No byte leaves [lo - overshoot, hi + overshoot] of its own neighbourhood; amount 0 is the identity; for a fixed neighbourhood the output is
    monotone in the amount; a negative amount down to -256 stays inside [lo, hi] by itself; a constant image has no high-pass."""
    from scipy import ndimage
    rng = np.random.default_rng(11)
    x = rng.integers(0, 256, (1, 24, 31, 3)).astype(np.uint8)
    x[0, :6] = np.where(rng.integers(0, 2, (6, 31, 3)) > 0, 255, 0)                                   # extremes
    lo = ndimage.minimum_filter(x[0].astype(np.int64), size=(3, 3, 1), mode="nearest")
    hi = ndimage.maximum_filter(x[0].astype(np.int64), size=(3, 3, 1), mode="nearest")
    assert (R.sharpen(x, [0], 24, 31, 4) == x).all()
    prev = None
    for a in (-1024, -512, -256, -100, -1, 0, 1, 100, 256, 512, 1024, 5000):
        for ov in (0, 4, 255):
            out = R.sharpen(x, [a], 24, 31, ov)[0].astype(np.int64)
            assert (out >= np.maximum(lo - ov, 0)).all() and (out <= np.minimum(hi + ov, 255)).all(), (a, ov)
            if -256 <= a <= 0:
                assert (out >= lo).all() and (out <= hi).all(), a
        out = R.sharpen(x, [a], 24, 31, 4)[0].astype(np.int64)
        if prev is not None:                                                                         # monotone in a: up where H > 0, down where H < 0
            h = R.highpass(x[0].astype(np.int64), "nearest")
            assert ((out - prev) * np.sign(h) >= 0).all(), a
        prev = out
    assert (R.sharpen(x, [5000], 24, 31, 4) == R.sharpen(x, [1024], 24, 31, 4)).all()                 # the kernel's clamp of the amount
    flat = np.full((1, 9, 9, 3), 77, np.uint8)
    assert (R.sharpen(flat, [1024], 9, 9, 4) == flat).all() and not R.highpass(flat[0].astype(np.int64), "nearest").any()
    # the statistic: x = y gives D = 0 and the count of the structured ring; a mask-free frame, and a window no 5 x 5 fits in, give zeros
    orig, model, mask, _ = R.detail_clip("same", 0)
    s = R.sums(orig, orig, mask, OFFS1, R.H, R.W, 8, 12).reshape(3, 4)
    assert (s[:, 0] > 500).all() and not s[:, 1].any() and not s[:, 3].any() and (s[:, 2] > 0).all()
    assert not R.sums(orig, orig, 0 * mask, OFFS1, R.H, R.W, 8, 12).any()
    assert not R.sums(orig[:, :4], orig, mask, np.array([[18, 0]], np.int32), 4, R.W, 8, 0).any()
    # edge = 0 counts every gated ring pixel, in all three channels alike: the ring of the box less the 5 x 5 gate
    s0 = R.sums(orig, orig, mask, OFFS1, R.H, R.W, 8, 0).reshape(3, 4)
    y0, x0, y1, x1 = R.BOX
    assert s0[:, 0].tolist() == [(y1 - y0 + 16) * (x1 - x0 + 16) - (y1 - y0 + 4) * (x1 - x0 + 4)] * 3


# ---- the rule on synthetic clips, the restatement alone ---------------------------------------------------------------------------------------
# DESIGN.md section 24 holds the table these figures come from (seeds 0 - 3, grain 0 / 4 / 8 on the original, +-1 level of noise on the model) and
# the reason for each margin.
SOFT_RATIO = 0.80           # measured 0.747 .. 0.753 of the error before; the margin is eight times the spread between the seeds
CRISP_Q8 = 10               # measured within 6 q8 of -256 (at grain 8); the margin is the spread again
CRISP_RMS = 0.56            # sqrt(2/3 * 36/256 + 1/12 + 1/12) = 0.51 levels: the model's noise through the binomial, two roundings; plus 10 %
SAME_Q8 = 5                 # measured within 3 q8 of 0, a third of the dead zone (15)
GRAIN_SOFT = 0.05           # the unclamped amount (about 830 q8) moves by at most 18 q8 = 2.2 % between grain 0, 4 and 8 at one seed
GRAIN_Q8 = 10               # crisp: at most 6 q8; same: at most 2


def _raw(s):
    """The unclamped fit of one frame's sums."""
    return R.fit(s, smooth=0, min_pixels=1, max_sharpen=1e6, max_soften=1e6, dead=0.0)[0][0]


@pytest.mark.parametrize("seed", range(4))
def test_the_rule_on_synthetic_clips(seed):
    raws = {}
    for kind in ("soft", "crisp", "same"):
        for grain in (0, 4, 8):
            orig, model, mask, truth = R.detail_clip(kind, seed, grain)
            out, s, (a,), (clamped,), (dead,) = R.apply(model, orig, mask, OFFS1, R.H, R.W)
            raw = raws[kind, grain] = _raw(s)
            before, after = R.rms(model[0], truth), R.rms(out[0], truth)
            n = int(s.reshape(3, 4)[:, 0].sum()) // 3
            print(f"{kind} clip, seed {seed}, grain {grain}: n {n}, unclamped {raw} q8, applied {a} q8 (clamped {clamped}, dead {dead}), "
                  f"rms error against the clean truth {before:.3f} -> {after:.3f}")
            assert n >= 256
            if kind == "soft":              # the inverse of a binomial blur is at least the whole high-pass at every frequency
                assert raw >= 256 and 256 <= a <= 512 and after <= SOFT_RATIO * before
            elif kind == "crisp":
                assert abs(raw + 256) <= CRISP_Q8 and a == max(raw, -256) and after <= CRISP_RMS and after < 0.1 * before
            else:
                assert abs(raw) <= SAME_Q8 and a == 0 and dead and (out == model).all()
    for grain in (4, 8):                    # grain on the original is uncorrelated with the model's high-pass: the fit moves little
        assert abs(raws["soft", grain] - raws["soft", 0]) <= GRAIN_SOFT * raws["soft", 0]
        assert abs(raws["crisp", grain] - raws["crisp", 0]) <= GRAIN_Q8 and abs(raws["same", grain] - raws["same", 0]) <= GRAIN_Q8


# ---- infill.finish with the kernels replaced by the restatements ----------------------------------------------------------------------------
def _stand_ins(monkeypatch, calls, on):
    """tests/test_seamblend_cpu.py's stand-ins of the paste and seam entry points (a stage that is not in `on` raises), plus this feature's and
    the deflicker's; calls gets (name, frames) per call."""
    import test_seamblend_cpu as SB
    from videovanish_amd import detailmatch_bind, flicker_hip
    SB._all_stand_ins(monkeypatch, calls, on)

    def said(name, fn):
        def f(patch, *a, **k):
            calls.append((name, len(patch)))
            return fn(patch, *a, **k)
        return f

    monkeypatch.setattr(detailmatch_bind, "ring_detail_stats", said("ring_detail_stats", R.hip_ring_detail_stats))
    monkeypatch.setattr(detailmatch_bind, "sharpen", said("sharpen", R.hip_sharpen))
    monkeypatch.setattr(flicker_hip, "window_pixels", FR.hip_window_pixels)
    monkeypatch.setattr(flicker_hip, "hold", said("hold", FR.hip_hold))


def _soft_clip(T=3, H=64, W=96):
    """(orig [T,H,W,3] u8, mask [T,H,W]): T renderings of detailmatch_ref's texture with its box mask; the last frame has no mask."""
    orig = np.stack([np.clip(np.rint(R.texture(20 + t, H, W)), 0, 255).astype(np.uint8) for t in range(T)])
    mask = np.stack([R.box_mask(H, W)] * (T - 1) + [np.zeros((H, W), np.uint8)])
    return orig, mask


def _soft(frames):
    """The frames as a soft model renders them: their 3 x 3 binomial blur."""
    return np.stack([np.clip(np.rint(R.blur(f.astype(np.float64))), 0, 255).astype(np.uint8) for f in frames])


CFG = dict(ring=8, edge=12, smooth=1, min_pixels=64, overshoot=4)


def test_finish_runs_the_stage_after_the_deflicker_and_before_tone_grain_and_blend(monkeypatch):
    """The full frame with every seam stage and the deflicker on: the calls in order, and the bytes of the chained restatements, in which tone,
    grain and membrane measure the sharpened rendering of the filtered pixels."""
    import torch
    from videovanish_amd import infill
    from videovanish_amd.deflicker import DeflickerConfig
    from videovanish_amd.grainmatch import GrainMatchConfig
    from videovanish_amd.seamblend import SeamBlendConfig
    from videovanish_amd.tonematch import ToneMatchConfig
    calls = []
    _stand_ins(monkeypatch, calls, ("tone", "grain", "blend"))
    orig, mask = _soft_clip()
    T, H, W = mask.shape
    x = _soft(orig)
    monkeypatch.setattr("videovanish_amd.seamblend.groups", lambda T, h, w: [(0, T)])
    rows, got = [], {}
    kw = dict(tone=ToneMatchConfig(), tone_out=[], grain=GrainMatchConfig(seed=5, min_count=64), grain_out=[], frame0=7,
              blend=SeamBlendConfig(strength=0.75), blend_out=[], flicker=DeflickerConfig(radius=1, tol=12), flicker_out=[])
    out = np.stack(infill.finish([list(x)], list(orig), torch.from_numpy(mask), [], 3, True, "cpu", detail=DetailMatchConfig(**CFG), detail_out=rows, **kw))
    names = [c[0] for c in calls]
    assert names == ["hold", "ring_detail_stats", "sharpen", "ring_stats", "ring_grain_stats", "solve", "paste_blend_composite"] and all(c[1] == T for c in calls)
    offs = np.zeros((T, 2), np.int32)
    held = FR.hold(x, offs, mask, 1, 12)[0]
    sharp, s, amounts, clamped, dead = R.apply(held, orig, mask, offs, H, W, **CFG)
    want = BR.apply(sharp, orig, mask, offs, H, W, 3.0, frame_ids=[7, 8, 9], strength=0.75, tone=dict(ring=12), grain=dict(seed=5, min_count=64))[0]
    assert (out == want).all() and any(a > 0 for a in amounts) and (sharp != held).any()
    rep, = rows
    assert isinstance(rep, infill.DetailMatchReport) and rep._fields == ("n", "amount", "residual", "clamped", "dead")
    assert rep.n.shape == rep.amount.shape == rep.residual.shape == rep.clamped.shape == rep.dead.shape == (1, T)
    assert rep.n.dtype == np.int64 and rep.amount.dtype == rep.residual.dtype == np.float64 and rep.clamped.dtype == rep.dead.dtype == bool
    assert (rep.amount[0] * 256).tolist() == amounts and rep.clamped[0].tolist() == clamped and rep.dead[0].tolist() == dead
    assert (rep.n[0] == s.reshape(T, 3, 4)[:, :, 0].sum(1) // 3).all() and rep.n[0, 2] == 0 and rep.n[0, 0] > 64 and rep.residual[0, 0] > 0


def test_finish_detail_alone_on_the_full_frame_and_on_two_windows(monkeypatch):
    """The stage alone: the full frame takes the window loop as (0, 0, H0, W0) and ends in the plain window paste; two windows, the second pasted
    into the first's output, a frame another rank holds stays None with zero rows; no other stage's binding is touched (their stand-ins raise)."""
    import torch
    from videovanish_amd import hip, infill
    calls = []
    _stand_ins(monkeypatch, calls, ())
    monkeypatch.setattr(hip, "resize_u8", lambda x, H, W, mode: torch.from_numpy(np.stack([TR.window_image(f, H, W) for f in x.numpy()])))
    orig, mask = _soft_clip(T=4)
    T, H, W = mask.shape
    offs = np.zeros((T, 2), np.int32)
    ident = np.broadcast_to(BR.IDENT, (T, 3, 256))
    cfg = DetailMatchConfig(**CFG)
    # the full frame, the model at half the size: the stage materialises the resize
    small = np.stack([TR.window_image(f, H // 2, W // 2) for f in _soft(orig)])
    for keep, feather in ((True, 3.0), (False, -1.0)):
        del calls[:]
        rows = []
        out = np.stack(infill.finish([list(small)], list(orig), torch.from_numpy(mask), [], 3, keep, "cpu", detail=cfg, detail_out=rows))
        assert calls == [("ring_detail_stats", T), ("sharpen", T), ("roi_paste_composite", T)]
        sharp, s, amounts, _, _ = R.apply(small, orig, mask, offs, H, W, **CFG)
        assert (out == TR.composite(sharp, orig, mask, offs, ident, H, W, feather)).all() and sharp.shape == (T, H, W, 3) and any(amounts)
        assert rows[0].n.shape == (1, T) and (rows[0].amount[0] * 256).tolist() == amounts
    # strength 0: the resize is materialised and pasted as it is -- the bytes of the call without the option
    del calls[:]
    out = infill.finish([list(small)], list(orig), torch.from_numpy(mask), [], 3, True, "cpu", detail=DetailMatchConfig(strength=0.0, **CFG))
    plain = infill.finish([list(small)], list(orig), torch.from_numpy(mask), [], 3, True, "cpu")
    assert (np.stack(out) == np.stack(plain)).all() and [c[0] for c in calls] == ["ring_detail_stats", "sharpen", "roi_paste_composite", "feather_composite"]
    # two windows; frame 2 is another rank's
    wins = [((0, 0), (44, 52)), ((14, 54), (50, 42))]                                               # disjoint
    mask2 = np.zeros((T, H, W), np.uint8)
    mask2[:, 12:30, 15:40] = 255
    mask2[:, 30:48, 64:84] = 255
    plans, outs = [], []
    for (oy, ox), (h, w) in wins:
        place = np.tile(np.array([[oy, ox]], np.int32), (T, 1))
        plans.append(types.SimpleNamespace(size=(h, w), offsets=place))
        outs.append(list(_soft(orig[:, oy:oy + h, ox:ox + w])))
    idx = [0, 1, 3]
    for o in outs:
        o[2] = None
    del calls[:]
    rows = []
    got = infill.finish(outs, list(orig), torch.from_numpy(mask2), plans, 3, True, "cpu", detail=cfg, detail_out=rows)
    assert got[2] is None and calls == [("ring_detail_stats", 3), ("sharpen", 3), ("roi_paste_composite", 3)] * 2
    want = orig[idx]
    rep, = rows
    assert rep.n.shape == (2, T)
    for k, (plan, o) in enumerate(zip(plans, outs)):
        h, w = plan.size
        patch = np.stack([o[i] for i in idx])
        s = np.zeros((T, 12), np.int64)
        s[idx] = R.sums(patch, want, mask2[idx], plan.offsets[idx], h, w, CFG["ring"], CFG["edge"])
        amounts, clamped, dead = R.fit(s, **dict(R.DEFAULTS, **CFG))
        sharp = R.sharpen(patch, [amounts[i] for i in idx], h, w, CFG["overshoot"])
        want = TR.composite(sharp, want, mask2[idx], plan.offsets[idx], ident[:3], h, w, 3.0)
        assert (rep.amount[k, idx] * 256).tolist() == [amounts[i] for i in idx] and (rep.n[k, idx] > 0).all() and any(amounts[i] for i in idx)
        assert not any(f[k, 2] for f in rep)                                                         # a zero row, whatever its neighbours pooled
    assert (np.stack([got[i] for i in idx]) == want).all() and (want != orig[idx]).any()
    # a rank that holds no frame of the clip: zero rows
    rows = []
    none = infill.finish([[None] * T, [None] * T], list(orig), torch.from_numpy(mask2), plans, 3, True, "cpu", detail=cfg, detail_out=rows)
    assert none == [None] * T and rows[0].n.shape == (2, T) and not any(f.any() for f in rows[0])


def test_detail_report_assembles_spans_and_windows_and_finish_keeps_its_signature():
    from videovanish_amd import infill
    one = lambda K, T, v: infill.DetailMatchReport(np.full((K, T), v, np.int64), np.full((K, T), v / 256.0), np.full((K, T), float(v)), np.ones((K, T), bool),
                                                   np.zeros((K, T), bool))
    rep = infill.detail_report([one(1, 3, 5), one(2, 2, 7)], [(1, 4), (6, 8)], 9)
    assert rep.n.tolist() == [[0, 5, 5, 5, 0, 0, 7, 7, 0], [0, 0, 0, 0, 0, 0, 7, 7, 0]] and (rep.amount * 256 == rep.n).all() and (rep.residual == rep.n).all()
    assert (rep.clamped == (rep.n > 0)).all() and not rep.dead.any() and rep.clamped.dtype == rep.dead.dtype == bool and rep.n.dtype == np.int64
    empty = infill.detail_report([], [], 4)
    assert empty.n.shape == (1, 4) and not any(f.any() for f in empty) and infill.detail_report([], [], 4, K=3).amount.shape == (3, 4)
    names = list(inspect.signature(infill.finish).parameters)
    assert names[-2:] == ["detail", "detail_out"] and names[names.index("flicker_align_out") + 1] == "detail"
    assert all(inspect.signature(infill.finish).parameters[k].default is None for k in names[-2:])


def test_finish_without_the_option_calls_nothing_of_the_feature(monkeypatch):
    import torch
    from videovanish_amd import detailmatch_bind, infill
    from videovanish_amd.tonematch import ToneMatchConfig
    calls = []
    _stand_ins(monkeypatch, calls, ("tone",))
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("a detail matching call without detail_match="))
    for name in ("ring_detail_stats", "sharpen", "lib"):
        monkeypatch.setattr(detailmatch_bind, name, boom)
    orig, mask = _soft_clip()
    x = _soft(orig)
    out = np.stack(infill.finish([list(x)], list(orig), torch.from_numpy(mask), [], 3, True, "cpu", tone=ToneMatchConfig()))
    assert (out == TR.apply(x, orig, mask, np.zeros((3, 2), np.int32), 64, 96, 3.0)[0]).all()
    assert [c[0] for c in calls] == ["ring_stats", "paste_lut_composite"]
    np.stack(infill.finish([list(x)], list(orig), torch.from_numpy(mask), [], 3, True, "cpu"))
    assert calls[-1][0] == "feather_composite"                                                       # no stage: the full-frame path as before


# ---- configuration and CLI ----------------------------------------------------------------------------------------------------------------
def test_the_call_passes_the_keywords_only_when_the_option_is_set(monkeypatch):
    import torch

    import diffuerase
    from videovanish_amd import hip, infill
    for o in diffuerase.ALL_OPTIONS:
        monkeypatch.delenv(o.env, raising=False)
    T = 3
    frames = [np.zeros((8, 8, 3), np.uint8) for _ in range(T)]
    log = []
    part = infill.detail_report([], [], T)
    part.amount[0, 1] = 0.5

    def run_clip(f, d, *a, **kw):
        log.append(kw)
        if "detail_out" in kw:
            kw["detail_out"].append(part)
        return list(f)

    monkeypatch.setattr(diffuerase, "get_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(hip, "mask_collapse_dilate", lambda m, it: torch.zeros((T, 8, 8), dtype=torch.uint8))
    monkeypatch.setattr(infill, "run_clip", run_clip)
    diffuerase.configure()
    diffuerase.last_detail_match = "stale"
    diffuerase.run_infill_on_frames(frames, frames)
    assert log == [{}] and diffuerase.last_detail_match is None
    diffuerase.run_infill_on_frames(frames, frames, detail_match="ring=4")
    assert set(log[-1]) == {"detail", "detail_out"} and log[-1]["detail"] == DetailMatchConfig(ring=4)
    rep = diffuerase.last_detail_match
    assert isinstance(rep, infill.DetailMatchReport) and rep.amount.tolist() == [[0.0, 0.5, 0.0]]
    diffuerase.run_infill_on_frames(frames, frames, detail_match="on", tone_match="on")
    assert set(log[-1]) == {"detail", "detail_out", "tone", "tone_out"}
    diffuerase.run_infill_on_frames(frames, frames, detail_match="off")
    assert log[-1] == {} and diffuerase.last_detail_match is None


def test_precedence_argument_configure_environment_and_exclusions(monkeypatch):
    import diffuerase
    monkeypatch.delenv("VV_DETAIL_MATCH", raising=False)
    row = diffuerase._OPTION["detail_match"]
    assert row in diffuerase.MORE_OPTIONS and row not in diffuerase.OPTIONS and len(diffuerase.OPTIONS) == 10
    assert row.env == "VV_DETAIL_MATCH" and row.settings is M and row.phrase == "seam detail matching"
    assert [M.as_config(x) for x in row.metavar.split("|")] == [DetailMatchConfig()] * 2
    try:
        diffuerase.configure()
        assert diffuerase.detail_match_config() is None
        monkeypatch.setenv("VV_DETAIL_MATCH", "ring=5")
        assert diffuerase.detail_match_config() == DetailMatchConfig(ring=5)
        diffuerase.configure(detail_match="edge=20")
        assert diffuerase.detail_match_config() == DetailMatchConfig(edge=20) and diffuerase.detail_match_config("on") == DetailMatchConfig()
        assert diffuerase.detail_match_config("off") is None and diffuerase.detail_match_config(False) is None
        diffuerase.configure(detail_match="off")
        assert diffuerase.detail_match_config() is None                                                    # configure("off") beats the environment
        mine = DetailMatchConfig(overshoot=0)
        assert diffuerase.detail_match_config(mine) is mine
        diffuerase.configure()
        assert diffuerase.detail_match_config() == DetailMatchConfig(ring=5)                               # configure() resets
        with pytest.raises(ValueError):
            diffuerase.configure(detail_match="sometimes")
        f = [np.zeros((8, 8, 3), np.uint8)] * 2
        with pytest.raises(ValueError, match=r"detail_match= \(seam detail matching\) cannot be combined with compat_reference_early_return=True"):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True)                      # from the environment
        monkeypatch.delenv("VV_DETAIL_MATCH")
        for value in ("on", "ring=4", DetailMatchConfig(), True):
            with pytest.raises(ValueError, match="detail_match="):
                diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, detail_match=value)
        with pytest.raises(ValueError, match="1 <= ring <= 32"):
            diffuerase.run_infill_on_frames(f, f, detail_match="ring=33")
        with pytest.raises(TypeError):
            diffuerase.run_infill_on_frames(f, f, detailmatch="on")
        diffuerase.last_detail_match = "stale"
        with pytest.raises(ValueError):
            diffuerase.run_infill_on_frames(f, f, compat_reference_early_return=True, detail_match="on")
        assert diffuerase.last_detail_match is None                                                        # reset at the start of every call
        monkeypatch.setenv("VV_DETAIL_MATCH", "sometimes")
        with pytest.raises(ValueError):
            diffuerase.detail_match_config()
    finally:
        diffuerase.configure()
    for fn in (diffuerase.run_infill_on_frames, diffuerase.configure):
        names = list(inspect.signature(fn).parameters)
        p = inspect.signature(fn).parameters["detail_match"]
        assert names[names.index("seam_blend") + 1] == "detail_match" and names[names.index("deflicker") + 1] == "deflicker_align"
        assert names[names.index("shadow_mask") + 1] == "plate_tone" and names[-3:] == ["plate_grain", "plate_align", "plate_fill"]
        assert p.default is None and (fn is diffuerase.configure or p.kind is inspect.Parameter.KEYWORD_ONLY)


def test_cli_detail_match_reaches_the_call_and_prints_one_line(monkeypatch, tmp_path, capsys):
    import diffuerase
    from videovanish_amd import infill
    calls = []
    videos = {"mask.mkv": [np.zeros((16, 24, 3), np.uint8)] * 4}
    tools = types.ModuleType("tools")
    tools.load_video_frames_from_path = lambda path, start=0, max_frames=-1: ([f.copy() for f in videos[path]], 24.0)
    tools.write_video_frames_to_path = lambda *a: None
    monkeypatch.setitem(sys.modules, "tools", tools)
    rep = infill.detail_report([], [], 4, K=2)
    rep.amount[0] = (1.25, 0.0, -0.5, 0.0)
    rep.amount[1] = (0.0, 0.0, -0.75, 0.0)
    rep.dead[:, 1] = True

    def fake(frames, masks, **kw):
        calls.append(kw)
        diffuerase.last_detail_match = rep if "detail_match" in kw else None
        return [f.copy() for f in frames]

    monkeypatch.setattr(diffuerase, "run_infill_on_frames", fake)
    color = tmp_path / "in.mkv"
    color.write_bytes(b"x")
    videos[str(color)] = [np.zeros((16, 24, 3), np.uint8)] * 4
    argv = ["diffuerase.py", "--color_video", str(color), "--mask_video", "mask.mkv"]
    monkeypatch.setattr(sys, "argv", argv)
    diffuerase.main()
    assert calls[-1] == {"propainer_frames": None} and capsys.readouterr().out == ""                      # a default call passes no keyword, prints nothing
    for value in ("on", "ring=4,strength=0.5"):
        monkeypatch.setattr(sys, "argv", argv + ["--detail-match", value, "--roi", "static"])
        diffuerase.main()
        assert calls[-1] == {"propainer_frames": None, "detail_match": value, "roi": "static"}
        out = capsys.readouterr().out
        assert out == "detail match: 2 of 4 frames matched, largest sharpen 1.250, largest soften 0.750, 1 frames unfit\n"
    for bad in ("off", "yes", "ring=x", "ring=33", "strength=2"):
        monkeypatch.setattr(sys, "argv", argv + ["--detail-match", bad])
        with pytest.raises(SystemExit):
            diffuerase.main()
    monkeypatch.setattr(diffuerase, "last_detail_match", None)
