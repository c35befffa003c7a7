"""CPU tests of the C-ABI library: it loads and exports every symbol include/vvhip.h declares (no compute calls)."""
import ctypes
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abiref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "videovanish_amd", "csrc", "libvvhip.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(LIB)


def _declared():
    src = open(os.path.join(ROOT, "include", "vvhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vv_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported(lib):
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/vvhip.h but not exported"


def _header():
    """include/vvhip.h without its comments"""
    return abiref.code(open(os.path.join(ROOT, "include", "vvhip.h")).read())


def test_binding_lists_match_header(lib):
    """hip.SIGNATURES declares every function of include/vvhip.h with the header's return and parameter types, and hip.lib() has applied it: an int64_t
    or float parameter passed without its declaration would be truncated / passed as garbage silently."""
    from videovanish_amd import hip
    protos = abiref.prototypes("vvhip.h", "vv_")[1]
    assert sorted(protos) == _declared() and len(protos) == 88
    assert sorted(hip.EXPORTS) == _declared()
    abiref.check_binding(hip, 88)
    assert sum(ctypes.c_int64 in a for _, a in protos.values()) == 34 and sum(ctypes.c_float in a for _, a in protos.values()) == 16
    assert lib.vv_abi_version() == hip.ABI_VERSION == 10


def test_parts_of_the_library_share_no_name():
    """The parts of libvvhip.so (abiref.PARTS) are hip and every videovanish_amd/*_hip.py, their headers every include/vv*.h but the codec's; the
    prefixes differ pairwise, every name of a part carries its own prefix, and no name is declared by two parts."""
    import glob
    found = ["hip"] + [os.path.basename(f)[:-3] for f in glob.glob(os.path.join(ROOT, "videovanish_amd", "*_hip.py"))]
    assert sorted(abiref.PARTS) == sorted(found) and len(set(abiref.PARTS)) == len(abiref.PARTS)
    parts = abiref.parts()
    headers = {os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "include", "vv*.h"))} - {"vvio.h"}
    assert sorted(p.header for _, p in parts) == sorted(headers)
    prefixes = [p.prefix for _, p in parts]
    assert len(set(prefixes)) == len(prefixes) and all(re.fullmatch(r"vv[a-z]?_", x) for x in prefixes) and parts[0][1].prefix == "vv_"
    seen = {}
    for mod, part in parts:
        assert part.signatures is mod.SIGNATURES and list(mod.SIGNATURES) == mod.EXPORTS, mod.__name__
        for name in mod.SIGNATURES:
            assert name.startswith(part.prefix), (mod.__name__, name)
            assert seen.setdefault(name, mod.__name__) == mod.__name__, (name, seen[name], mod.__name__)
        for other in prefixes:      # a name of one part cannot be taken for another's either: no other prefix starts it
            assert other == part.prefix or not any(name.startswith(other) for name in mod.SIGNATURES), (mod.__name__, other)


def test_wrong_kind_of_argument_is_refused_at_the_call():
    """with the declared signatures a float where the header says int, or a Python object where it says pointer, raises ctypes.ArgumentError instead of
    passing garbage.  vv_layernorm validates before it touches a device and every pointer is null: nothing could be launched even if a call went through."""
    from videovanish_amd import hip
    fn = hip.lib().vv_layernorm
    assert fn(None, 1, 4, None, None, None, 1, None, 0, None) == -1      # the same call with well-typed arguments reaches the library (and is refused there)
    with pytest.raises(ctypes.ArgumentError):
        fn(None, 1.0, 4, None, None, None, 1, None, 0, None)             # float for `int M`
    with pytest.raises(ctypes.ArgumentError):
        fn(object(), 1, 4, None, None, None, 1, None, 0, None)           # an object (e.g. a tensor instead of its address) for `const float* x`
    with pytest.raises(ctypes.ArgumentError):
        hip.lib().vv_conv_gemm(ctypes.byref(hip.ConvParams()), 0.0, None)      # float for `int dtype` (all-null parameters: refused by the library otherwise)


def test_integration_md_binding_snippet_version_check(lib):
    """The reference-side ctypes snippet of INTEGRATION.md section 2 is executed up to (and including) its ABI assert, against the library as built:
    a stale version number in the document fails here."""
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = next(b for b in re.findall(r"```python\n(.*?)```", md, flags=re.S) if "vv_abi_version" in b)
    head = block.split("def dilate_masks")[0]
    assert "ctypes.CDLL" in head and "assert lib.vv_abi_version() ==" in head
    cwd = os.getcwd()
    os.chdir(ROOT)      # the snippet loads the library by its path relative to the app directory
    try:
        exec(compile(head, "INTEGRATION.md", "exec"), {})
    finally:
        os.chdir(cwd)
    hdr = open(os.path.join(ROOT, "include", "vvhip.h")).read()
    ver = re.search(r"#define VV_ABI_VERSION (\d+)", hdr).group(1)
    assert "vv_abi_version() == " + ver in head


def test_vvio_header_symbols_are_exported():
    """include/vvio.h (frame codec, libvvio.so): every declared entry point is exported and the ABI versions agree."""
    src = open(os.path.join(ROOT, "include", "vvio.h")).read()
    ver = int(re.search(r"#define VVIO_ABI_VERSION (\d+)", src).group(1))
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(vvio_[a-z0-9_]+)\s*\(", src)))
    assert names == ["vvio_abi_version", "vvio_ffv1_config_record", "vvio_ffv1_decode_frame", "vvio_ffv1_decode_frame_yuv", "vvio_ffv1_decoder_close",
                     "vvio_ffv1_decoder_decode", "vvio_ffv1_decoder_info", "vvio_ffv1_decoder_open", "vvio_ffv1_encode_frame", "vvio_ffv1_stream_info",
                     "vvio_ycbcr_to_rgb"]
    io = ctypes.CDLL(os.path.join(ROOT, "videovanish_amd", "csrc", "libvvio.so"))
    for n in names:
        assert hasattr(io, n), f"{n} declared in include/vvio.h but not exported"
    assert io.vvio_abi_version() == ver


def test_argument_validation_without_gpu(lib):
    """Launchers validate arguments before touching the device: bad args -> negative code + message."""
    from videovanish_amd import hip
    lib.vv_last_error.restype = ctypes.c_char_p
    p = hip.ConvParams()
    assert lib.vv_conv_gemm(ctypes.byref(p), 0, None) == -1 and b"null tensor" in lib.vv_last_error()
    a = hip.AttnParams()
    assert lib.vv_attention(ctypes.byref(a), 0, None) == -1
    assert lib.vv_layernorm(None, 1, 4, None, None, None, 1, None, 0, None) == -1
    assert lib.vv_groupnorm_nsplit(14400, 320) >= 1


def test_product_path_has_no_cpu_fallback():
    """hip wrappers refuse CPU tensors; the product package never imports oracle/."""
    import torch
    from videovanish_amd import hip
    with pytest.raises(RuntimeError):
        hip.axpby(torch.zeros(4), torch.zeros(4), 1.0, 1.0)
    pkg = os.path.join(ROOT, "videovanish_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f
    txt = open(os.path.join(ROOT, "diffuerase.py")).read() if os.path.isfile(os.path.join(ROOT, "diffuerase.py")) else ""
    assert "oracle" not in txt


def test_chain_stream_layout_is_part_of_the_abi(lib):
    """ABI 10: vv_spatial_chain_c320 refuses a weight stream whose `layout` is not the order its kernel consumes -- the orders have equal slab
    and parameter counts, so only the id can tell a stream packed the pre-round-5 way from the current one.  Checked before anything touches a device."""
    from videovanish_amd import hip, packing
    lib.vv_last_error.restype = ctypes.c_char_p
    assert hip.CHAIN_LAYOUT_IDS[packing.CHAIN_LAYOUT] == 1
    hdr = open(os.path.join(ROOT, "include", "vvhip.h")).read()
    for name, val in (("TOKENS", 0), ("ROWSPLIT", 1), ("COLUMNS", 2)):
        assert re.search(rf"#define VV_CHAIN_LAYOUT_{name}\s+{val}\b", hdr)
    buf = (ctypes.c_char * 64)()
    addr = ctypes.addressof(buf)
    base = dict(o=addr, t_in=addr, x=addr, res1=0, out=addr, out_dtype=hip.F32, stream=addr, params=addr, M=128, C=320, heads=8, text_len=77, n_slabs=462, n_params=5120)
    for stale in (0, 2, 7):
        cp = hip.ChainParams(layout=stale, **base)
        assert lib.vv_spatial_chain_c320(ctypes.byref(cp), hip.F16, None) == -1
        msg = lib.vv_last_error()
        assert b"layout" in msg and str(stale).encode() in msg, msg


def test_product_sources_carry_no_timing_probes():
    """VERDICT r5 hygiene 10: switches that make a kernel compute wrong results (timing probes) live in tools/lab/*.patch, never in csrc/.  Since the lab
    build was retired the same holds for every A/B switch it carried: one form per kernel, no environment variable read, in EVERY file of the directory."""
    csrc = os.path.join(ROOT, "videovanish_amd", "csrc")
    sources = [f for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".c"))]
    assert "vv_chain.hip" in sources and "vv_motion.hip" in sources
    assert not [f for f in sources if f.endswith(("lab.hip", "lab.h"))]      # no lab-only translation unit or header comes back
    retired = ("VV_AB", "VV_AB_ENV", "VV_AB_INT", "getenv", "VV_ATTN_VARIANT", "VV_CHAIN_FORM", "VV_CHAIN_TT", "VV_CHAIN_LAG", "VV_CHAIN_AHEAD", "VV_CHAIN_PIN",
               "VV_FRONT_FORM", "VV_FRONT_BURST", "VV_MOTION_FORM", "VV_GELU_SCALAR", "VV_GELU_ERFF", "VV_GELU2", "VV_GELU2_POLY", "VV_NO_STAGE_F32",
               "VV_ROUTE_HALO256", "VV_ROUTE_TILE_128x320")
    for f in sources:
        txt = open(os.path.join(csrc, f)).read()
        for tok in ("VV_PROBE_", "VV_CHAIN_PROBE_", "VV_MOTION_NO_PIN"):
            assert tok not in txt, (f, tok)
        for tok in retired:      # whole words: VV_ABI_VERSION is not VV_AB
            assert not re.search(rf"\b{tok}\b", txt), (f, tok)
    hdr = open(os.path.join(ROOT, "include", "vvhip.h")).read()
    assert "VV_ROUTE_HALO256" not in hdr and "VV_ROUTE_TILE_128x320" not in hdr and "lab build" not in hdr
    assert os.path.isfile(os.path.join(ROOT, "tools", "lab", "r5_chain_probes.patch"))


def test_one_build_recipe():
    """The library's sources and per-file flags are listed once, in csrc/build.sh: the variant recipe of the A/B tools (tools/build_variant.sh) is a call of
    it and names no source or compiler of its own, so a variant cannot miss a translation unit (it once lacked vv_roi).  Text only: nothing is compiled."""
    csrc = os.path.join(ROOT, "videovanish_amd", "csrc")
    code = lambda p: "\n".join(l.split("#", 1)[0] for l in open(p).read().splitlines()[1:])      # without comments
    recipe, variant = code(os.path.join(csrc, "build.sh")), code(os.path.join(ROOT, "tools", "build_variant.sh"))
    listed = set(re.findall(r"\bvv_[a-z0-9]+\b", recipe)) - {"vv_ffv1"}
    units = {f[:-4] for f in os.listdir(csrc) if f.endswith(".hip")}
    assert listed == units, (sorted(listed - units), sorted(units - listed))      # every translation unit in the directory is in the one list, and nothing else
    assert "build.sh" in variant and "--out" in variant
    assert not re.search(r"\bvv_[a-z0-9]+\b", variant) and "hipcc" not in variant and ".hip" not in variant
    assert "--out" in recipe and "--src" in recipe
    for f in os.listdir(os.path.join(ROOT, "tools")):      # and no other tool compiles the library's sources itself
        if f.endswith(".sh") and f != "build_variant.sh":
            assert not re.search(r"hipcc[^\n]*csrc", open(os.path.join(ROOT, "tools", f)).read()), f


def _struct_members(name):
    """member names of `typedef struct { ... } name;` in include/vvhip.h, in order"""
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", _header()).group(1)
    names = []
    for decl in body.split(";"):
        if decl.strip():      # `type a, b, c` / `const type* a`: the declarators are the last word of each comma-separated piece
            names += [re.search(r"(\w+)\s*$", d).group(1) for d in decl.split(",")]
    return names


def test_struct_layouts_match_header(tmp_path):
    """the seven parameter structs of include/vvhip.h == their ctypes mirrors in hip.py: the same member names in the same order, and sizeof / offsetof of
    EVERY member as gcc compiles the header."""
    import subprocess
    from videovanish_amd import hip
    mirrors = {"vv_conv_params": hip.ConvParams, "vv_deform_params": hip.DeformParams, "vv_attn_params": hip.AttnParams,
               "vv_groupnorm_params": hip.GroupNormParams, "vv_chain_params": hip.ChainParams, "vv_motion_params": hip.MotionParams,
               "vv_chain_front_params": hip.ChainFrontParams}
    assert sorted(mirrors) == sorted(re.findall(r"\}\s*(vv_\w+_params)\s*;", _header()))      # every struct of the header is probed
    probes = {name: (cls, [f[0] for f in cls._fields_]) for name, cls in mirrors.items()}
    for name, (cls, fields) in probes.items():
        assert fields == _struct_members(name), (name, fields, _struct_members(name))
    assert len(probes["vv_conv_params"][1]) == 45
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "vvhip.h"', "int main(void) {"]
    for name, (_, fields) in probes.items():
        src.append(f'  printf("{name} %zu", sizeof({name}));')
        for f in fields:
            src.append(f'  printf(" %zu", offsetof({name}, {f}));')
        src.append('  printf("\\n");')
    src += ["  return 0;", "}"]
    c = tmp_path / "probe.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(out) == len(probes)
    for line in out:
        parts = line.split()
        cls, fields = probes[parts[0]]
        want = [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
        assert [int(x) for x in parts[1:]] == want, (parts[0], parts[1:], want)


def test_tcd_timesteps_match_diffusers_schedule():
    """diffusers TCDScheduler.set_timesteps (original_inference_steps 50): floor(linspace(0, 50, n, endpoint=False)) into [999, 979, ...]."""
    from oracle import model_ref as M
    from videovanish_amd.pipeline import ddim_timesteps, tcd_timesteps
    assert tcd_timesteps(2) == [999, 499] and tcd_timesteps(4) == [999, 759, 499, 259] and tcd_timesteps(3) == [999, 679, 339]
    assert tcd_timesteps(1) == [999] and tcd_timesteps(50) == [20 * k - 1 for k in range(50, 0, -1)]
    for n in (1, 2, 3, 4, 5, 8, 10, 25, 50):
        assert tcd_timesteps(n) == M.tcd_timesteps(n) and ddim_timesteps(n) == M.ddim_timesteps(n)


def test_normalize_device():
    """str / torch.device / int are all accepted and keep their index (one process per GPU passes cuda:<LOCAL_RANK>)."""
    import pytest
    import torch
    from videovanish_amd.nn import normalize_device
    assert normalize_device("cuda:3") == torch.device("cuda", 3)
    assert normalize_device(torch.device("cuda", 5)) == torch.device("cuda", 5)
    assert normalize_device(2) == torch.device("cuda", 2)
    with pytest.raises(RuntimeError):
        normalize_device("cpu")
