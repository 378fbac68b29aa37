"""CPU: the ctypes binding that tavsr/_lib.py derives from include/tavsr.h - descriptor layouts against the C compiler's,
the signatures set on the loaded library, the reader's refusal of what it does not know, and the activation codes."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from helpers import ROOT

HEADER = os.path.join(ROOT, "include", "tavsr.h")
PUBLIC = {"tavsr_gemm_desc": "GemmDesc", "tavsr_attn_desc": "AttnDesc", "tavsr_ffn_desc": "FfnDesc",
          "tavsr_bf_layer_desc": "BfLayerDesc", "tavsr_bf_layer_bwd_desc": "BfLayerBwdDesc",
          "tavsr_tailored_stream_desc": "TailoredStreamDesc", "tavsr_tailored_layer_desc": "TailoredLayerDesc",
          "tavsr_cgmlp_desc": "CgmlpDesc", "tavsr_cgmlp_bwd_desc": "CgmlpBwdDesc",
          "tavsr_subsample_desc": "SubsampleDesc", "tavsr_subsample_bwd_desc": "SubsampleBwdDesc"}


def _code():
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def test_descriptor_layouts_are_the_compilers(tmp_path):
    """sizeof and the offset of EVERY field of every descriptor struct, as the host C compiler lays the header out, against
    the derived ctypes classes (a field the reader dropped, reordered or mistyped moves a size or an offset; one it
    misnamed does not compile)"""
    from tavsr import _lib
    names = re.findall(r"typedef\s+struct\s+(\w+)\s*\{", _code())
    assert sorted(names) == sorted(PUBLIC) == sorted(_lib.STRUCTS)          # all 11, no skip list
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "tavsr.h"', 'int main(void) {']
    for s in names:
        cls = getattr(_lib, PUBLIC[s])
        assert cls is _lib.STRUCTS[s] and issubclass(cls, C.Structure)
        lines.append(f'  printf("{s} sizeof %zu\\n", sizeof({s}));')
        lines += [f'  printf("{s} {f} %zu\\n", offsetof({s}, {f}));' for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines()]
    want = []
    for s in names:
        cls = _lib.STRUCTS[s]
        want.append([s, "sizeof", str(C.sizeof(cls))])
        want += [[s, f, str(getattr(cls, f).offset)] for f, _ in cls._fields_]
    assert got == want
    sizes = {s: int(v) for s, f, v in got if f == "sizeof"}
    assert sizes["tavsr_gemm_desc"] == 304 and sizes["tavsr_bf_layer_desc"] == 864 and sizes["tavsr_tailored_stream_desc"] == 672
    # descriptor-pointer fields stay typed pointers: `b.fwd = C.pointer(d)` keeps d alive
    assert _lib.BfLayerBwdDesc._fields_[0] == ("fwd", C.POINTER(_lib.BfLayerDesc))
    assert dict(_lib.TailoredLayerDesc._fields_)["video"] is C.POINTER(_lib.TailoredStreamDesc)
    assert dict(_lib.CgmlpBwdDesc._fields_)["fwd"] is C.POINTER(_lib.CgmlpDesc)
    assert dict(_lib.SubsampleBwdDesc._fields_)["fwd"] is C.POINTER(_lib.SubsampleDesc)


def test_every_prototype_has_its_signature_on_the_loaded_library():
    from tavsr._lib import lib
    protos = re.findall(r"\b(tavsr_\w+)\s*\(([^()]*)\)\s*;", _code())
    assert len(protos) >= 151 and len({n for n, _ in protos}) == len(protos)
    L = lib()
    for name, args in protos:
        n = 0 if args.strip() == "void" else args.count(",") + 1
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, name
    for name in ("tavsr_gemm_ws", "tavsr_colsum_ws", "tavsr_layernorm_bwd_ws"):
        assert getattr(L, name).restype is C.c_int64, name
    assert L.tavsr_version.restype is C.c_int and L.tavsr_gemm.restype is C.c_int
    assert L.tavsr_last_error_string.restype is C.c_char_p
    ln = L.tavsr_layernorm_fwd.argtypes      # (x, ldx, gamma, beta, eps, y, ldy, mean, rstd, M, D, stream)
    assert ln[1] is C.c_int64 and ln[4] is C.c_float
    assert ln[0] is C.c_void_p and ln[9] is C.c_int32 and ln[11] is C.c_void_p
    assert L.tavsr_gemm.argtypes == [C.c_void_p, C.c_void_p]          # a descriptor pointer takes byref(), an address or None
    with pytest.raises(C.ArgumentError):                               # a cast of another width than the header's is an error now
        L.tavsr_layernorm_bwd_ws(C.c_int64(4), 256)


@pytest.mark.parametrize("text", [
    "int tavsr_f(long double x, tavsr_stream_t stream);",              # a scalar outside the vocabulary
    "int tavsr_f(const struct foo* p);",
    "int tavsr_f(float (*cb)(int));",
    "size_t tavsr_f(void);",                                           # ... as a return type
    "typedef struct tavsr_d { int32_t n; unsigned flags; } tavsr_d;",  # ... as a field
    "typedef struct tavsr_d { tavsr_other_desc* p; } tavsr_d;",        # a pointer to a struct that was never declared
    "typedef union tavsr_u { int32_t i; float f; } tavsr_u;",          # a statement of another kind
    "static inline int tavsr_f(int x) { return x; }",
])
def test_reader_raises_on_what_it_does_not_know(text):
    from tavsr._lib import TavsrError, read_header
    ok = "int tavsr_version(void);\n"
    structs, protos, _ = read_header(ok)
    assert not structs and protos == {"tavsr_version": (C.c_int, [])}
    with pytest.raises(TavsrError):
        read_header(ok + text + "\n")


def test_reader_takes_the_headers_awkward_declarators():
    from tavsr._lib import read_header
    structs, protos, enums = read_header("""
        enum { TAVSR_ACT_NONE = 0, TAVSR_ACT_RELU = 1 };
        typedef struct tavsr_a_desc { int32_t n; float *score, *pooled /* [4][B*T] */, *wts; const float* w[2]; uint64_t off[9]; } tavsr_a_desc;
        typedef struct tavsr_b_desc { const tavsr_a_desc *x, *y; tavsr_stream_t s; void *e0, *e1; } tavsr_b_desc;
        int64_t tavsr_ws(const tavsr_b_desc* b, const float* const* params, double f, tavsr_stream_t* out);
    """)
    a, b = structs["tavsr_a_desc"], structs["tavsr_b_desc"]
    assert a.__name__ == "ADesc" and [f for f, _ in a._fields_] == ["n", "score", "pooled", "wts", "w", "off"]
    assert a._fields_[4][1] is C.c_void_p * 2 and a._fields_[5][1] is C.c_uint64 * 9 and C.sizeof(a) == 8 + 3 * 8 + 16 + 72
    assert b._fields_ == [("x", C.POINTER(a)), ("y", C.POINTER(a)), ("s", C.c_void_p), ("e0", C.c_void_p), ("e1", C.c_void_p)]
    assert protos == {"tavsr_ws": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p])}
    assert enums == {"TAVSR_ACT_NONE": 0, "TAVSR_ACT_RELU": 1}


def test_act_codes_are_the_headers_enum():
    from tavsr._lib import ACT
    enum = dict(re.findall(r"TAVSR_ACT_(\w+)\s*=\s*(\d+)", _code()))
    assert len(enum) == 7
    assert ACT == {None: 0, **{k.lower(): int(v) for k, v in enum.items()}}
    assert ACT == {None: 0, "none": 0, "relu": 1, "swish": 2, "gelu": 3, "tanh": 4, "hardtanh": 5, "selu": 6}
