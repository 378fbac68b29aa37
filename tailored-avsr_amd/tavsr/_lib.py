"""ctypes binding of libtavsr_hip.so (C ABI declared in include/tavsr.h).

The product path has NO fallback: if the shared library is missing or a call fails, a
``TavsrError`` is raised.  Device pointers are passed as raw addresses (``tensor.data_ptr()``) and
every call is enqueued on torch's current HIP stream, so the calls compose with torch's caching
allocator, stream semantics and HIP-graph capture.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# TAVSR_LIB selects another build of the same library (profiles/gemm_trace.py's instrumented one); never a fallback.
LIB_PATH = os.environ.get("TAVSR_LIB") or os.path.join(_HERE, "lib", "libtavsr_hip.so")


class TavsrError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------- the binding, read from the header
# include/tavsr.h is the only declaration of the C ABI: the descriptor classes, every entry point's argtypes / restype and the
# activation codes below are derived from it when this module is imported (no C parser: the header keeps to one regular dialect,
# and a declaration outside it is an error, not a guess).  tests/test_binding.py checks the layouts against the C compiler's.
HEADER_PATH = os.path.join(_HERE, "..", "..", "include", "tavsr.h")
_SCALARS = {"int": C.c_int, "uint8_t": C.c_uint8, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_POINTEES = set(_SCALARS) | {"void", "char"}
_DECL = re.compile(r"(\w+)\s*((?:\*\s*)*)(\w*)\s*(?:\[(\d+)\])?$")


def _class_name(struct):
    return "".join(w.capitalize() for w in struct.split("_")[1:])


def read_header(text):
    """(structs, prototypes, enums) of a header in the dialect of include/tavsr.h: ``typedef struct tavsr_x {...} tavsr_x;`` ->
    {"tavsr_x": Structure class}, ``ret tavsr_f(args);`` -> {"tavsr_f": (restype, [argtypes])}, enumerators -> {name: value}.
    Scalars map to their ctypes type, ``const char*`` to c_char_p, ``tavsr_stream_t`` and every data pointer to c_void_p; a
    pointer to a descriptor is POINTER(struct) as a field (assigning ``C.pointer(d)`` keeps ``d`` alive) and c_void_p as an
    argument (byref, a raw address or None).  Anything else raises TavsrError: a declaration is never skipped or guessed."""
    structs, protos, enums = {}, {}, {}

    def ctype(decl, where, field=False):
        m = _DECL.match(re.sub(r"\bconst\b", " ", decl).strip())
        if not m:
            raise TavsrError(f"include/tavsr.h: cannot read `{decl.strip()}` in {where}")
        base, stars, name, dim = m[1], m[2].count("*"), m[3], m[4]
        if field and not name:
            raise TavsrError(f"include/tavsr.h: field without a name `{decl.strip()}` in {where}")
        if base == "tavsr_stream_t":
            t = C.c_void_p
        elif stars == 0 and base in _SCALARS:
            t = _SCALARS[base]
        elif stars == 1 and base == "char":
            t = C.c_char_p
        elif stars == 1 and base in structs:
            t = C.POINTER(structs[base]) if field else C.c_void_p
        elif stars >= 1 and base in _POINTEES:
            t = C.c_void_p
        else:
            raise TavsrError(f"include/tavsr.h: unknown type in `{decl.strip()}` in {where}")
        return name, t * int(dim) if dim else t

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{|^\s*\}\s*$', " ", text, flags=re.M)
    text = text.replace("typedef void* tavsr_stream_t;", " ")

    def enum(m):
        for item in m[1].split(","):
            name, value = item.split("=")
            enums[name.strip()] = int(value)
        return " "

    def struct(m):
        fields = []
        for stmt in filter(str.strip, m[2].split(";")):
            first, *rest = stmt.split(",")          # `const float *q, *k, *v`: the later declarators repeat the first one's base type
            fields.append(ctype(first, m[1], field=True))
            base = re.match(r"\s*(?:const\s+)?\w+", first)[0]
            fields += [ctype(f"{base} {d}", m[1], field=True) for d in rest]
        structs[m[1]] = type(_class_name(m[1]), (C.Structure,), {"_fields_": fields, "__doc__": f"{m[1]} (include/tavsr.h)"})
        return " "

    text = re.sub(r"enum\s*\{([^}]*)\}\s*;", enum, text)
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{([^}]*)\}\s*\1\s*;", struct, text)
    for stmt in filter(str.strip, text.split(";")):
        m = re.match(r"\s*([\w\s\*]+?)\b(tavsr_\w+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if not m:
            raise TavsrError(f"include/tavsr.h: cannot read `{' '.join(stmt.split())}`")
        args = [] if m[3].strip() == "void" else [ctype(a, m[2])[1] for a in m[3].split(",")]
        protos[m[2]] = (ctype(m[1], m[2])[1], args)
    return structs, protos, enums


with open(HEADER_PATH) as _f:
    STRUCTS, PROTOTYPES, ENUMS = read_header(_f.read())
# GemmDesc, AttnDesc, FfnDesc, BfLayerDesc, BfLayerBwdDesc, TailoredStreamDesc, TailoredLayerDesc, CgmlpDesc, CgmlpBwdDesc,
# SubsampleDesc, SubsampleBwdDesc: tavsr_gemm_desc -> GemmDesc, ...
globals().update({cls.__name__: cls for cls in STRUCTS.values()})
ACT = {None: 0, **{k[len("TAVSR_ACT_"):].lower(): v for k, v in ENUMS.items() if k.startswith("TAVSR_ACT_")}}


_lib = None


def lib() -> C.CDLL:
    """Load (once) and return the shared library; fail loudly when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TavsrError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
        _lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(_lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        us = float(os.environ.get("TAVSR_RACE_PROBE", "0") or 0)
        if us > 0:      # race amplifier of the C-side sequencers (tests; ops/streams.py arms the Python-side scopes from the same variables)
            _lib.tavsr_race_probe(us, {"body": 0, "join": 1, "alt": 2}[os.environ.get("TAVSR_RACE_PROBE_MODE", "alt")])
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().tavsr_last_error_string().decode()
        raise TavsrError(f"{what} failed (rc={rc}): {msg}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream() -> int:
    """torch's current HIP stream of the current device as a raw handle (the fast private accessor when torch has it:
    torch.cuda.current_stream() builds a Stream object per call, ~9 us, and a step makes ~1100 calls)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------- stream safety
# Independent sections run on forked HIP streams (ops.BranchScope).  The two rules that make that safe against torch's per-stream
# caching allocator are stated at the head of tavsr/ops/streams.py and enforced HERE, at the one place where a tensor becomes a raw
# pointer (rule 1: ``ptr`` / ``addr`` -> ``_note``) and at the head of every autograd backward (rule 2: ``enter_node``), instead of by
# hand at the fork sites.
_FORKED = {}          # raw handle -> (torch.cuda.Stream forked, torch.cuda.Stream owner)
_CUR_FORK = None      # the forked stream launches currently go to (None: an owning / main stream), kept by the scopes below
_CUR_SEEN = None      # addresses already recorded in the innermost scope (a scope re-reads its operands many times)
SINGLE_STREAM = os.environ.get("TAVSR_SINGLE_STREAM", "0") == "1"      # every fork disabled: one queue, as the reference
RULES_OFF = False     # (tests only: switch both rules off to show that the race amplifier then catches the missing dependencies)


def register_fork(forked: "torch.cuda.Stream", owner: "torch.cuda.Stream") -> None:
    _FORKED[forked.cuda_stream] = (forked, owner)


def _note(t) -> None:
    """rule 1 for one tensor (parameters and other step-persistent tensors are never freed inside a step: skipped)"""
    if isinstance(t, torch.nn.Parameter) or RULES_OFF:
        return
    a = t.data_ptr()
    if _CUR_SEEN is not None:
        if a in _CUR_SEEN:
            return
        _CUR_SEEN.add(a)
    t.record_stream(_CUR_FORK)


def push_fork(forked) -> tuple:
    """launches go to ``forked`` from here (ops.BranchScope); returns the state ``pop_fork`` restores"""
    global _CUR_FORK, _CUR_SEEN
    prev = (_CUR_FORK, _CUR_SEEN)
    _CUR_FORK, _CUR_SEEN = forked, set()
    return prev


def pop_fork(prev: tuple) -> None:
    global _CUR_FORK, _CUR_SEEN
    _CUR_FORK, _CUR_SEEN = prev


def enter_node() -> tuple:
    """head of an autograd node's backward: autograd runs the node on the stream its forward ran on.  If that is a forked
    stream and no scope put us there, apply rule 2 (wait for the owner) and switch rule 1 on for the node's launches."""
    global _CUR_FORK, _CUR_SEEN
    prev = (_CUR_FORK, _CUR_SEEN)
    if _FORKED:
        ent = _FORKED.get(_raw_stream(torch.cuda.current_device()) if _raw_stream is not None
                          else torch.cuda.current_stream().cuda_stream)
        if ent is None:
            _CUR_FORK = _CUR_SEEN = None
        elif _CUR_FORK is not ent[0]:
            if not RULES_OFF:
                ent[0].wait_stream(ent[1])
            _CUR_FORK, _CUR_SEEN = ent[0], set()
    return prev


def guarded(fn):
    """decorator of every ``torch.autograd.Function.backward`` of the package (see enter_node)"""
    import functools

    @functools.wraps(fn)
    def wrapper(*args):
        prev = enter_node()
        try:
            return fn(*args)
        finally:
            pop_fork(prev)
    return wrapper


def ptr(t):
    """device address of ``t`` as a plain integer (every pointer parameter is declared c_void_p); None stays None (NULL)"""
    if t is None:
        return None
    if _CUR_FORK is not None:
        _note(t)
    return t.data_ptr()


def addr(t, off: int = 0):
    """``ptr`` as a plain integer (descriptor fields), ``off`` in 4-byte elements; None stays None"""
    if t is None:
        return None
    if _CUR_FORK is not None:
        _note(t)
    return t.data_ptr() + 4 * off


def param_ptrs(P):
    """storage addresses of a parameter list (None -> 0), as one tuple: the signature a cached descriptor template is valid for
    (a ``.to()`` or an optimizer that swaps ``.data`` changes it).  Parameters are not noted on a forked stream (``_note``)."""
    return tuple(0 if p is None else p.data_ptr() for p in P)


def cached_params(module, names):
    """[parameter or None for n in names] of ``module``, looked up once: the Parameter objects of a module never change
    identity (``.to()`` / ``load_state_dict`` / the fused optimizer swap ``.data``), while ``dict(named_parameters())`` per
    forward call costs ~1.5 ms of host time per step over the model's layers."""
    cache = module.__dict__.get("_tavsr_pcache")
    if cache is None or cache[0] is not names:
        sd = dict(module.named_parameters())
        cache = module.__dict__["_tavsr_pcache"] = (names, [sd.get(n) for n in names])
    return cache[1]


def require_cuda(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise TavsrError("tavsr ops run on the MI355X only: got a CPU tensor (no CPU fallback exists)")
