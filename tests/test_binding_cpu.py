"""The Python binding's tables against the C++ compiler (no GPU, no built library).

The header reader at the top of youku-mplug_amd/_lib.py derives every ctypes struct, every (restype, argtypes) entry and every integer
constant from include/mpv.h.  Here the host C++ compiler is the oracle for all of it: one generated translation unit includes the header and prints, for every struct
the reader found, sizeof and each field's offsetof / size / class; for every function, through a template on decltype(mpv_x), the number of
parameters and the size and class (pointer, floating, signed, unsigned, void) of the return type and of each parameter; and the value of
every constant.  decltype needs no definition, so nothing links.  A name the reader invented does not compile; a name it missed is caught
by comparing against the identifiers in the comment-stripped header text."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

PRELUDE = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "mpv.h"
template <class T> struct K {
  static void p() {
    std::printf(" %zu%c", sizeof(T), std::is_pointer<T>::value ? 'p' : std::is_floating_point<T>::value ? 'f'
                                     : std::is_signed<T>::value ? 'i' : std::is_unsigned<T>::value ? 'u' : '?');
  }
};
template <> struct K<void> { static void p() { std::printf(" 0v"); } };
template <class F> struct Sig;
template <class R, class... A> struct Sig<R(A...)> {
  static void p(const char* name) { std::printf("F %s %zu", name, sizeof...(A)); K<R>::p(); (K<A>::p(), ...); std::printf("\n"); }
};
int main() {
"""


def _compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [shutil.which(n) for n in ("c++", "g++", "clang++")] + [os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")]
    return next((p for p in found if p and os.path.isfile(p)), None)


def _kind(t):
    """a ctypes type as the translation unit prints a C type: size, then p / f / i / u / v"""
    if t is None:
        return "0v"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return f"{C.sizeof(t)}p"
    if t in (C.c_float, C.c_double):
        return f"{C.sizeof(t)}f"
    assert issubclass(t, C._SimpleCData) and isinstance(t(0).value, int), t
    return f"{C.sizeof(t)}{'i' if t(-1).value < 0 else 'u'}"


def _tables():
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    return _lib.CONSTANTS, _lib.STRUCTS, _lib._SIGS


def _stripped_header():
    with open(os.path.join(INCLUDE, "mpv.h")) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """what the compiler says about every name in the reader's tables: the printed lines, split into words"""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++, or the ROCm clang++)")
    constants, structs, sigs = _tables()
    body = [f'  std::printf("C {n} %lld\\n", (long long)({n}));' for n in constants]
    for s, cls in structs.items():
        body.append(f'  std::printf("S {s} %zu\\n", sizeof({s}));')
        for f, _ in cls._fields_:
            body.append(f'  std::printf("M {s} {f} %zu", offsetof({s}, {f})); K<decltype({s}::{f})>::p(); std::printf("\\n");')
    body += [f'  Sig<decltype({n})>::p("{n}");' for n in sigs]
    d = tmp_path_factory.mktemp("binding")
    src, exe = d / "layout.cpp", d / "layout"
    src.write_text(PRELUDE + "\n".join(body) + "\n  return 0;\n}\n")
    subprocess.run([cxx, "-std=c++17", "-O0", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
    return [line.split() for line in out.splitlines()]


def test_struct_layouts_match_the_compiler(compiled):
    _, structs, _ = _tables()
    assert set(re.findall(r"typedef\s+struct\s+(\w+)\s*\{", _stripped_header())) == set(structs) and len(structs) == 23
    sizes = {w[1]: int(w[2]) for w in compiled if w[0] == "S"}
    members = {(w[1], w[2]): (int(w[3]), w[4]) for w in compiled if w[0] == "M"}
    assert set(sizes) == set(structs) and len(members) == sum(len(c._fields_) for c in structs.values())
    for s, cls in structs.items():
        assert C.sizeof(cls) == sizes[s], f"{s}: ctypes {C.sizeof(cls)} bytes, the compiler {sizes[s]}"
        for f, t in cls._fields_:
            desc, (offset, kind) = getattr(cls, f), members[s, f]
            assert (desc.offset, desc.size, _kind(t)) == (offset, int(kind[:-1]), kind), \
                f"{s}.{f}: ctypes offset {desc.offset}, {desc.size} bytes, {_kind(t)}; the compiler {offset}, {kind}"


def test_signatures_match_the_compiler(compiled):
    _, _, sigs = _tables()
    text = _stripped_header()
    macros = set(re.findall(r"#[ \t]*define[ \t]+(\w+)\(", text))
    declared = set(re.findall(r"\b(mpv_[a-z0-9_]+)\s*\(", text)) - macros
    assert declared == set(sigs), declared ^ set(sigs)
    funcs = {w[1]: (int(w[2]), w[3], w[4:]) for w in compiled if w[0] == "F"}
    assert set(funcs) == set(sigs) and len(sigs) == 153
    for name, (restype, argtypes) in sigs.items():
        n, ret, args = funcs[name]
        assert (len(argtypes), _kind(restype)) == (n, ret), f"{name}: {len(argtypes)} parameters -> {_kind(restype)}, the compiler {n} -> {ret}"
        for i, t in enumerate(argtypes):
            assert _kind(t) == args[i], f"{name}, parameter {i}: ctypes {_kind(t)}, the compiler {args[i]}"


def test_constants_equal_the_defines(compiled):
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib, ops
    constants, _, _ = _tables()
    assert set(re.findall(r"#[ \t]*define[ \t]+(MPV_\w+)[ \t]+\S", _stripped_header())) == set(constants)     # every object-like macro is an integer
    assert {w[1]: int(w[2]) for w in compiled if w[0] == "C"} == constants
    names = {"MPV_W8_MAX_ROWS": _lib.W8_MAX_ROWS, "MPV_W8_TILED_MAX_ROWS": _lib.W8_TILED_MAX_ROWS,
             "MPV_CAPTION_OVERLAP_MAX_LEN": _lib.CAPTION_OVERLAP_MAX_LEN, "MPV_CAPTION_CIDER_ORDERS": _lib.CAPTION_CIDER_ORDERS,
             "MPV_LN_DPARAM_DEFER": ops.LN_DPARAM_DEFER, "MPV_ACT_NONE": ops.ACT_NONE, "MPV_ACT_GELU_ERF": ops.ACT_GELU_ERF,
             "MPV_ACT_GELU_TANH": ops.ACT_GELU_TANH, "MPV_ACT_RELU": ops.ACT_RELU, "MPV_ACT_DERIV": ops.ACT_DERIV}
    assert names == {k: constants[k] for k in names}
    assert (_lib.W8_MAX_ROWS, _lib.W8_TILED_MAX_ROWS, _lib.CAPTION_OVERLAP_MAX_LEN, _lib.CAPTION_CIDER_ORDERS, ops.LN_DPARAM_DEFER) == (96, 512, 255, 4, 2)
    assert (ops.ACT_NONE, ops.ACT_GELU_ERF, ops.ACT_GELU_TANH, ops.ACT_RELU, ops.ACT_DERIV) == (0, 1, 2, 3, 4)
    assert constants["MPV_E_SHAPE"] == -1 and constants["MPV_E_ARG"] == -5                                       # the parenthesised negatives


@pytest.mark.parametrize("what,text,named", [
    ("an array field", "typedef struct mpv_x { int n; float w[4]; } mpv_x;", "float w[4]"),
    ("a bit-field", "typedef struct mpv_x { unsigned on : 1; } mpv_x;", "unsigned on : 1"),
    ("an unknown type", "int mpv_f(const mpv_nope_desc* d, int n);", "int mpv_f(const mpv_nope_desc* d, int n)"),
    ("a function-pointer parameter", "int mpv_g(void (*done)(int), int n);", "int mpv_g(void (*done)(int), int n)"),
    ("a struct by value", "typedef struct mpv_x { int n; } mpv_x;\nint mpv_h(mpv_x d);", "int mpv_h(mpv_x d)"),
    ("an unknown field type", "typedef struct mpv_x { long n; } mpv_x;", "long n"),
])
def test_reader_raises_and_names_the_declaration(what, text, named):
    """raise, don't guess: whatever lies outside the header's narrow kind of C stops the import with the declaration in the message"""
    import youku_mplug_amd  # noqa: F401
    from youku_mplug_amd import _lib
    good = "typedef struct ihipStream_t* mpv_stream_t;\n#define MPV_OK 0\nint mpv_version(void);\n"
    constants, structs, functions = _lib.parse_header(good)
    assert (constants, structs, list(functions)) == ({"MPV_OK": 0}, {}, ["mpv_version"])
    with pytest.raises(_lib.HeaderError) as e:
        _lib.parse_header(good + text + "\nint mpv_after(mpv_stream_t stream);\n")
    assert named in str(e.value), f"{what}: {e.value}"
