"""The header checks the binding tests share: one parser of the prototypes of an include/vv*.h, the comparison of a hip.Part (videovanish_amd/hip.py and
every *_hip.py) with its header and with the library as built, and the text checks on a feature's product sources.  A feature's test calls
check_binding(module, count) and goes on with its own limits and refusals; tests/test_abi_cpu.py holds the rules between the parts over PARTS."""
import ctypes
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videovanish_amd", "csrc")
# every part of libvvhip.so, as modules of videovanish_amd (test_abi_cpu.py: exactly hip and every *_hip.py, and every header but vvio.h)
PARTS = ("hip", "spans_hip", "mask_hip", "tone_hip", "grain_hip", "blend_hip", "plate_hip", "align_hip", "flicker_hip", "flickalign_hip", "plategrain_hip",
         "shadow_hip")
CTYPE_OF = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
RET_OF = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}


def part_of(module):
    """the hip.Part a binding module declares"""
    return module.CORE if module.__name__ == "videovanish_amd.hip" else module.PART


def parts():
    """[(module, its hip.Part)] over PARTS"""
    mods = [importlib.import_module("videovanish_amd." + name) for name in PARTS]
    return [(m, part_of(m)) for m in mods]


def code(raw):
    """a header without its comments"""
    return re.sub(r"/\*.*?\*/", "", raw, flags=re.S)


def prototypes(header, prefix):
    """include/<header> -> (its text, {name: (restype, [argtypes])} of every prototype whose name starts with prefix, in the header's order): any pointer
    parameter -> c_void_p, scalars by CTYPE_OF, the return type by RET_OF"""
    raw = open(os.path.join(ROOT, "include", header)).read()
    protos = {}
    for ret, name, args in re.findall(rf"^\s*(int|int64_t|const char\*)\s+({prefix}[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code(raw), flags=re.M):
        args = [" ".join(a.split()) for a in args.split(",")]
        args = [] if args in (["void"], [""]) else args
        # a parameter is `type name`; a pointer of any pointee is an address
        protos[name] = (RET_OF[ret], [ctypes.c_void_p if "*" in a else CTYPE_OF[a.rsplit(" ", 1)[0]] for a in args])
    return raw, protos


def built():
    """build the library first if a test runs before anything has"""
    if not os.path.isfile(os.path.join(CSRC, "libvvhip.so")):
        import __graft_entry__
        __graft_entry__.build()


def check_binding(module, count):
    """module.SIGNATURES declares every function of the module's header -- `count` of them -- with the header's types and in its order, EXPORTS lists
    the same names, the header declares no function outside its own prefix, module.lib() has applied the table, and the header's
    <PREFIX>ABI_VERSION, module.ABI_VERSION and <prefix>abi_version() agree.  -> (the loaded library, define(name) = the value of a #define of
    the header)."""
    part = part_of(module)
    built()
    raw, protos = prototypes(part.header, part.prefix)
    src = code(raw)
    declared = re.findall(rf"\b({part.prefix}[a-z0-9_]+)\s*\(", src)
    assert list(protos) == declared == list(module.SIGNATURES) == module.EXPORTS and len(protos) == count, (declared, list(module.SIGNATURES))
    assert part.signatures is module.SIGNATURES and part.version == module.ABI_VERSION
    assert not [n for n in re.findall(r"\b(vv[a-z]*_[a-z0-9_]+)\s*\(", src) if not n.startswith(part.prefix)]      # no other part's function
    loaded = module.lib()
    assert loaded is part.dll
    for name, (restype, argtypes) in protos.items():
        fn = getattr(loaded, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes, (name, fn.argtypes, argtypes)
        assert (restype, tuple(argtypes)) == (module.SIGNATURES[name][0], tuple(module.SIGNATURES[name][1])), name
    define = lambda name: eval(re.search(rf"^#define {name}\s+(.+)$", src, flags=re.M).group(1))
    assert getattr(loaded, part.prefix + "abi_version")() == define(part.prefix.upper() + "ABI_VERSION") == module.ABI_VERSION
    return loaded, define


def check_sources(unit, header, settings):
    """The product sources of a feature: csrc/<unit>.hip is in the one build recipe with include/<header> among the dependencies, reads no
    environment and includes the header; videovanish_amd/<settings>.py imports neither torch nor oracle.  -> (the kernel file's text, the
    settings module's text) for what the feature checks on top."""
    recipe = open(os.path.join(CSRC, "build.sh")).read()
    assert re.search(rf"\b{unit}\b", recipe) and "include/" + header in recipe
    kernel = open(os.path.join(CSRC, unit + ".hip")).read()
    assert "getenv" not in kernel and f'include/{header}"' in kernel
    txt = open(os.path.join(ROOT, "videovanish_amd", settings + ".py")).read()
    assert "import torch" not in txt and "from torch" not in txt and "oracle" not in txt
    return kernel, txt
