"""tests/abi_direct.py names, for every export of libvvhip.so that launches something, one GPU test that calls it directly.  Checked here by reading text, without a
GPU: the table covers hip.EXPORTS exactly (minus the entries that launch nothing), each named test exists, and its source calls a hip.py wrapper that reaches the
export.  A new export without a direct test fails here."""
import ast
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_direct  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# exports that launch nothing: version / error / device queries and the dispatchers' route and geometry queries
LAUNCH_NOTHING = ["vv_abi_version", "vv_last_error", "vv_device_count", "vv_device_name", "vv_conv_gemm_route", "vv_attention_route", "vv_groupnorm_nsplit",
                  "vv_conv_gn_partial_blocks"]


def _functions(path):
    src = open(path).read()
    return {n.name: ast.get_source_segment(src, n) for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef)}


def _internal(path):
    """names a test cannot call as hip.<name>(: the methods of classes and the functions that start with an underscore"""
    tree = ast.parse(open(path).read())
    methods = {n.name for c in ast.walk(tree) if isinstance(c, ast.ClassDef) for n in c.body if isinstance(n, ast.FunctionDef)}
    return methods | {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("_")}


def _wrappers(funcs, export, internal=frozenset()):
    """the wrappers of `export`: the functions of hip.py whose own source calls it on the library.  Only where such a function is internal (a method or a
    private helper such as _gn_stats) do the functions that call IT stand in for it; a public wrapper is never replaced by its callers"""
    reach = {f for f, s in funcs.items() if re.search(r"\blib\(\)\.%s\b" % export, s)}
    seen = set()
    while reach & internal - seen:
        f = sorted(reach & internal - seen)[0]
        seen.add(f)
        reach |= {g for g, s in funcs.items() if g != f and re.search(r"\b%s\(" % f, s)}
    return reach          # an internal one stays: a test may call hip._gn_stats( itself


def test_the_table_covers_every_export_that_launches():
    from videovanish_amd import hip
    assert all(e in hip.EXPORTS for e in LAUNCH_NOTHING)
    assert sorted(abi_direct.DIRECT) == sorted(e for e in hip.EXPORTS if e not in LAUNCH_NOTHING)


def test_each_named_test_exists_and_calls_a_wrapper_of_its_export():
    funcs, internal = _functions(os.path.join(ROOT, "videovanish_amd", "hip.py")), _internal(os.path.join(ROOT, "videovanish_amd", "hip.py"))
    tests = {}
    for export, where in abi_direct.DIRECT.items():
        path, name = where.split("::")
        assert path.startswith("tests/") and os.path.isfile(os.path.join(ROOT, path)), f"{export}: no file {path}"
        if path not in tests:
            tests[path] = _functions(os.path.join(ROOT, path))
        assert name in tests[path] and name.startswith("test_"), f"{export}: {path} has no test {name}"
        wrappers = _wrappers(funcs, export, internal)
        assert wrappers, f"no function of hip.py calls {export}"
        body = tests[path][name]
        helpers = [s for f, s in tests[path].items() if not f.startswith("test_") and re.search(r"\b%s\(" % f, body)]          # module helpers the test calls
        assert any(re.search(r"\bhip\.%s\(" % w, t) for w in wrappers for t in [body] + helpers), f"{where} does not call a wrapper of {export} ({sorted(wrappers)})"


def test_a_wrapper_less_export_would_be_caught():
    funcs, internal = _functions(os.path.join(ROOT, "videovanish_amd", "hip.py")), _internal(os.path.join(ROOT, "videovanish_amd", "hip.py"))
    assert _wrappers(funcs, "vv_not_an_export", internal) == set()
    assert _wrappers(funcs, "vv_silu_f32", internal) == {"silu"} and _wrappers(funcs, "vv_axpby_f32", internal) == {"axpby"}          # a caller of axpby does not count
    assert "groupnorm" in _wrappers(funcs, "vv_gn_finalize_partials", internal) and "motion_module_c320" in _wrappers(funcs, "vv_groupnorm_stats", internal)
