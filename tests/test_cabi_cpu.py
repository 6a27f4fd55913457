"""torch_points3d_amd/cabi.py: the ctypes bindings are read from include/tp3d_hip.h and include/tp3d_cpu.h.  The parsed
names are held against an independent regex, one declaration per type class against a literal, and everything outside
the supported C subset must be refused by name instead of bound with a guessed type.  Nothing is launched."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from torch_points3d_amd import _lib, cabi, torchpoints

_p, _i, _l, _f, _d, _z = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double,
                          ctypes.c_size_t)


def _header(name):
    return os.path.join(ROOT, "include", name)


def _declared(name, prefix):
    text = re.sub(r"/\*.*?\*/", "", open(_header(name)).read(), flags=re.S)
    return set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, text))


HIP = cabi.parse_header(_header("tp3d_hip.h"))[0]
CPU = cabi.parse_header(_header("tp3d_cpu.h"))[0]


def test_parsed_names_are_the_declared_names():
    hip, cpu = _declared("tp3d_hip.h", "tp3d_"), _declared("tp3d_cpu.h", "tp3d_cpu_")
    assert len(hip) >= 152 and len(cpu) == 7
    assert set(HIP) == hip and set(CPU) == cpu
    assert set(_lib.FUNCTIONS) == set(_lib.SIGNATURES) == set(_lib.MISC) == hip
    for name, (restype, argtypes) in _lib.FUNCTIONS.items():
        assert _lib.SIGNATURES[name] is argtypes and _lib.MISC[name] == (restype, argtypes)
    with pytest.raises(TypeError):  # the two views are read-only
        _lib.SIGNATURES["tp3d_fps_f32"] = []


@pytest.mark.parametrize("table,name,want", [
    (HIP, "tp3d_fps_f32", (_i, [_p, _i, _i, _i, _p, _p, _p])),
    (HIP, "tp3d_fgr_solve", (_i, [_l, _i, _d, _p, _p, _z, _p])),
    (HIP, "tp3d_instance_ap_match", (_i, [_p, _p, _p, _p, _l, _p, _p, _p, _p, _l, _d, _p, _p, _p])),
    (HIP, "tp3d_strerror", (ctypes.c_char_p, [_i])),
    (HIP, "tp3d_ball_query_workspace_bytes", (_z, [_i, _l, _i])),
    (CPU, "tp3d_cpu_grid_build", (_p, [_p, _l, _f])),
    (CPU, "tp3d_cpu_grid_free", (None, [_p])),
    (CPU, "tp3d_cpu_grow_clusters", (_l, [_p, _l, _i, _l, _p, _p])),
    (HIP, "tp3d_abi_version", (_i, [])),
], ids=lambda v: v if isinstance(v, str) else "")
def test_one_declaration_per_type_class(table, name, want):
    restype, argtypes = table[name]
    assert restype is want[0]
    assert len(argtypes) == len(want[1]) and all(a is b for a, b in zip(argtypes, want[1])), argtypes


def test_constants_are_the_header_defines():
    c = _lib.CONSTANTS
    assert c["TP3D_E_TOOBIG"] == -4 and c["TP3D_ABI_VERSION"] == 39 and c["TP3D_OK"] == 0
    assert "TP3D_HIP_H" not in c  # a define without an integer value is no constant
    assert _lib.ABI_VERSION == c["TP3D_ABI_VERSION"]
    assert torchpoints.FPS_MAX_REG_POINTS == c["TP3D_FPS_MAX_REG_POINTS"] == 32768
    assert torchpoints.BOX_NMS_MAX_BOXES == c["TP3D_BOX_NMS_MAX_BOXES"] == 4096
    assert torchpoints.PART_IOU_MAX_PARTS == c["TP3D_PART_IOU_MAX_PARTS"] == 16
    assert torchpoints.CLUSTER_BEST_WINDOW == c["TP3D_CLUSTER_BEST_WINDOW"] == 1024
    assert cabi.parse("#define A 7\n# define B (-12)  /* why */\n#define C 1.5\n#define D (2 + 3)\n")[1] == {"A": 7, "B": -12}


@pytest.mark.parametrize("text", [
    "int tp3d_bad(unsigned n);",
    "int tp3d_bad(long n);",
    "int tp3d_bad(unsigned int n);",
    "int tp3d_bad(struct tp3d_box box);",
    "int tp3d_bad(tp3d_box box);",
    "int tp3d_bad(const float *x, int);",
    "int tp3d_bad(const float *, int n);",
    "int tp3d_bad(int const);",
    "int tp3d_bad(float xyz[3]);",
    "int tp3d_bad(void (*done)(int), void *stream);",
    "int tp3d_bad(const char *fmt, ...);",
    "int tp3d_bad();",
    "int tp3d_bad(int n, );",
    "long tp3d_bad(int n);",
    "float *tp3d_bad(int n);",
    "tp3d_bad(int n);",
    "int tp3d_bad;",
    "typedef struct tp3d_bad tp3d_bad_t;",
    "struct tp3d_bad { int n; };",
    "int tp3d_bad(int n) { return n; }",
    "int tp3d_ok(int n);\nint tp3d_bad(int n)\n",
])
def test_outside_the_subset_is_refused_by_name(text):
    with pytest.raises(ValueError, match="tp3d_bad"):
        cabi.parse(text)


def test_layouts_the_headers_use():
    text = """
/* a comment with ; and ( in it, and a call-like tp3d_ghost(int x); inside */
#ifndef GUARD_H
#define GUARD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define LIMIT (-3)   /* trailing comment */
int tp3d_a(const int64_t *with_space, const int64_t* without_space, const int64_t*tight, int64_t n);
size_t
tp3d_b(const float *const *xs,
       unsigned char *arg,   /* ; ( */
       double
           tol);
void tp3d_c ( void ) ;
#ifdef __cplusplus
}
#endif
#endif /* GUARD_H */
"""
    functions, constants = cabi.parse(text)
    assert constants == {"LIMIT": -3}
    assert functions == {"tp3d_a": (_i, [_p, _p, _p, _l]), "tp3d_b": (_z, [_p, _p, _d]), "tp3d_c": (None, [])}
