"""ctypes binding of libmpv_hip.so (the C ABI declared in include/mpv.h).

The product path has NO CPU / PyTorch fallback: if the library is missing or a call fails
this module raises.  Build with `python __graft_entry__.py` (or `make -C youku-mplug_amd/csrc`).
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPV_LIB_PATH") or os.path.join(_HERE, "libmpv_hip.so")   # override: instrumented measurement builds only

# ------------------------------------------------------------------------------------------------------------------------------------------
# The header reader.  parse_header(text) returns (constants, structs, functions):
#   constants   MPV_NAME -> int, every `#define MPV_NAME <integer literal>` (parenthesised negatives included; macros with arguments are not)
#   structs     name -> ctypes.Structure subclass, every `typedef struct T { ... } T;`, fields in declaration order
#   functions   name -> (restype, [argtypes]), every prototype, in header order
#
# One type rule serves fields, parameters and return types: the scalars below map to their ctypes twins, an opaque handle
# (`typedef struct S* mpv_stream_t`) to c_void_p, `const char*` to c_char_p, a one-star pointer to a struct of the header to
# POINTER(that struct), a pointer to pointers to POINTER(c_void_p), every other pointer to c_void_p.  The header is plain C of that
# narrow kind; whatever lies outside it (an unknown type name, an array, a bit-field, a function pointer, a struct by value) raises
# HeaderError with the declaration in the message.  Nothing is guessed.
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mpv.h")

_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double, "int32_t": C.c_int32,
            "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8, "size_t": C.c_size_t}
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(MPV_\w+)[ \t]+(-?\d+|\(-?\d+\))[ \t]*$", re.M)
_CPLUSPLUS = re.compile(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*$", re.M | re.S)
_DIRECTIVE = re.compile(r"^[ \t]*#(?:\\\n|[^\n])*$", re.M)
_TOKEN, _NOT_PLAIN = re.compile(r"\w+|\*"), re.compile(r"[^\w\s*]")      # a declarator is words and stars, nothing else
_STATEMENT = re.compile(r"\s*(?:typedef\s+struct\s+(?P<tag>\w+)\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)"
                        r"|typedef\s+struct\s+\w+\s*\*\s*(?P<handle>\w+)"
                        r"|(?P<proto>[^;{}]+?))\s*;")


class HeaderError(ValueError):
    pass


def _declarators(decl: str, where: str):
    """`const void *q, *k` -> [("void", True, 1, "q"), ("void", True, 1, "k")]: (base type, const, stars, name) per declarator"""
    out, base = [], None
    for piece in decl.split(","):
        toks = _TOKEN.findall(piece)
        words = [t for t in toks if t not in ("*", "const")]
        if _NOT_PLAIN.search(piece) or len(words) != (1 if base else 2):
            raise HeaderError(f"not a plain `type name` declaration: `{' '.join(piece.split())}` in `{' '.join(where.split())}`")
        if base is None:
            base, const = words[0], "const" in toks[:(toks + ["*"]).index("*")]
        out.append((base, const, toks.count("*"), words[-1]))
    return out


def _ctype(types: dict, base: str, const: bool, stars: int, decl: str):
    if base not in types and base not in ("void", "char"):
        raise HeaderError(f"unknown type `{base}` in `{' '.join(decl.split())}`")
    t = types.get(base)
    struct = t is not None and issubclass(t, C.Structure)
    if stars == 0 and t is not None and not struct:
        return t
    if stars == 1:
        return C.c_char_p if (base == "char" and const) else C.POINTER(t) if struct else C.c_void_p
    if stars == 2:
        return C.POINTER(C.c_void_p)
    raise HeaderError(f"`{base}` with {stars} stars has no ctypes twin here (by value, or too deep): `{' '.join(decl.split())}`")


def parse_header(text: str):
    """-> (constants, structs, functions) of header text; see the reader's rules above"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {name: int(value.strip("()")) for name, value in _DEFINE.findall(text)}
    text = _DIRECTIVE.sub("", _CPLUSPLUS.sub("", text))
    types, structs, functions = dict(_SCALARS), {}, {}
    pos = 0
    while (m := _STATEMENT.match(text, pos)):
        pos = m.end()
        if m["handle"]:
            types[m["handle"]] = C.c_void_p
        elif m["struct"]:
            if m["tag"] != m["struct"]:
                raise HeaderError(f"struct tag and typedef name differ: `{m['tag']}` / `{m['struct']}`")
            fields = [(name, _ctype(types, base, const, stars, decl))
                      for decl in m["body"].split(";") if decl.strip()
                      for base, const, stars, name in _declarators(decl, decl)]
            types[m["struct"]] = structs[m["struct"]] = type(m["struct"], (C.Structure,), {"_fields_": fields})
        else:
            proto = m["proto"]
            f = re.fullmatch(r"([^()]*)\((.*)\)", proto, re.S)
            if not f or "," in f[1]:
                raise HeaderError(f"neither a struct typedef nor a prototype: `{' '.join(proto.split())}`")
            (base, const, stars, name), = _declarators(f[1], proto)
            restype = None if (base, stars) == ("void", 0) else _ctype(types, base, const, stars, proto)
            params = [] if f[2].strip() == "void" else f[2].split(",")
            functions[name] = (restype, [_ctype(types, *_declarators(p, proto)[0][:3], proto) for p in params])
    if text[pos:].strip():
        raise HeaderError(f"cannot read the declaration at `{' '.join(text[pos:].split())[:120]}`")
    return constants, structs, functions


# The structs, the signatures and the constants are READ from the header: a new entry point needs its declaration there and its wrapper in
# ops.py, nothing here.  What the header cannot say stays in this file: where the library is, the Python names of the descriptor structs,
# and how a failed call is reported.
with open(HEADER_PATH) as _f:
    CONSTANTS, STRUCTS, _SIGS = parse_header(_f.read())     # MPV_NAME -> int, struct name -> Structure, entry -> (restype, [argtypes])

GemmEpilogue = STRUCTS["mpv_gemm_epilogue"]
AttnDesc = STRUCTS["mpv_attn_desc"]
AttnPlanInfo = STRUCTS["mpv_attn_plan_info"]
AttnPrefixDesc = STRUCTS["mpv_attn_prefix_desc"]
AttnPrefixPackedDesc = STRUCTS["mpv_attn_prefix_packed_desc"]
AttnPrefixPackedBwdDesc = STRUCTS["mpv_attn_prefix_packed_bwd_desc"]
AttnDecodeSharedDesc = STRUCTS["mpv_attn_decode_shared_desc"]
SimSearchDesc = STRUCTS["mpv_sim_search_desc"]
SimBankDesc = STRUCTS["mpv_sim_bank_desc"]
MaxSimSearchDesc = STRUCTS["mpv_maxsim_search_desc"]
BeamAdvanceDesc = STRUCTS["mpv_beam_advance_desc"]
BeamAdvanceGroupsDesc = STRUCTS["mpv_beam_advance_groups_desc"]
SampleAdvanceDesc = STRUCTS["mpv_sample_advance_desc"]
LogitsConstrainDesc = STRUCTS["mpv_logits_constrain_desc"]
LogitsGuideDesc = STRUCTS["mpv_logits_guide_desc"]
LogitsTrieDesc = STRUCTS["mpv_logits_trie_desc"]
SampleScoreDesc = STRUCTS["mpv_sample_score_desc"]
CaptionOverlapDesc = STRUCTS["mpv_caption_overlap_desc"]
CaptionCiderDesc = STRUCTS["mpv_caption_cider_desc"]
GptLayerWeights = STRUCTS["mpv_gpt_layer_weights"]
GptWeights = STRUCTS["mpv_gpt_weights"]
GptLayerWeightsQ8 = STRUCTS["mpv_gpt_layer_weights_q8"]
GptWeightsQ8 = STRUCTS["mpv_gpt_weights_q8"]

CAPTION_OVERLAP_MAX_LEN = CONSTANTS["MPV_CAPTION_OVERLAP_MAX_LEN"]
CAPTION_CIDER_ORDERS = CONSTANTS["MPV_CAPTION_CIDER_ORDERS"]
W8_MAX_ROWS = CONSTANTS["MPV_W8_MAX_ROWS"]
W8_TILED_MAX_ROWS = CONSTANTS["MPV_W8_TILED_MAX_ROWS"]

EXPORTS = tuple(_SIGS)

_lib = None


class MpvError(RuntimeError):
    pass


def lib():
    """The loaded library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise MpvError(f"{LIB_PATH} not found: the HIP kernels are not built. "
                           "Run `python __graft_entry__.py` (build()) first; there is no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)      # AttributeError if a declared symbol is missing
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


n_calls = 0      # C-ABI calls checked so far (engine.graph_step: "has this graph segment captured anything yet?")


def check(rc: int, what: str = ""):
    global n_calls
    n_calls += 1
    if rc != 0:
        raise MpvError(f"{what} failed ({rc}): {lib().mpv_last_error().decode()}")
