"""CPU: the C-ABI of the capsule obstacles as far as it needs no GPU - the struct, the entry point and the refusals that
mi_gomp_scene_create_world decides before it looks at the handle."""
import ctypes as C
import os
import re

import numpy as np

import capsule_refs as K
import gomp_refs as G
import osqp_solver_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL


def test_struct_and_entry_point():
    with open(os.path.join(ROOT, "include", "mi_osqp.h")) as f:
        src = f.read()
    assert re.search(r"typedef struct \{ double a\[3\], b\[3\]; double radius; double margin; \} mi_gomp_capsule;", src)
    assert re.search(r"\bint mi_gomp_scene_create_world\(mi_gomp_scene \*\*out, mi_osqp_batch \*h, int64_t dims, int64_t waypoints,\s*"
                     r"const mi_gomp_chain \*chain, int64_t n_balls, const mi_gomp_ball \*balls,\s*"
                     r"int64_t n_lines, const mi_gomp_line \*lines, int64_t n_capsules, const mi_gomp_capsule \*capsules,\s*"
                     r"const double \*con_lo, const double \*con_hi\);", src)
    assert C.sizeof(K.Capsule) == 64
    assert hasattr(M.lib(), "mi_gomp_scene_create_world")


def test_refusals_that_need_no_handle():
    L = K.declare(M.lib())
    s = K.scene("K8")
    caps = s["capsules"]

    def refused(code, capsules=caps, why=None, **kw):
        rc, ptr = K.create_world(L, None, 8, 2, s["chain"], s["balls"], s["lines"], capsules, s["con_lo"], s["con_hi"], **kw)
        assert rc == code and not ptr, (rc, ptr, L.mi_osqp_last_error())
        if why:
            assert why in L.mi_osqp_last_error().decode(), L.mi_osqp_last_error()

    refused(NULL, null_capsules=True, why="no capsules")
    refused(INVALID, n_capsules=-1, why="negative")
    refused(INVALID, n_capsules=-(2 ** 40), null_capsules=True, why="negative")
    for key in ("a", "b"):
        for k in range(3):
            for bad in (np.nan, np.inf, -np.inf):
                c = dict(caps[0], a=list(caps[0]["a"]), b=list(caps[0]["b"]))
                c[key][k] = bad
                refused(INVALID, [caps[0], c], why="capsule 1 has a field that is not finite")
    for key in ("radius", "margin"):
        for bad in (np.nan, np.inf):
            refused(INVALID, [dict(caps[0], **{key: bad})], why="not finite")
        refused(INVALID, [dict(caps[0], **{key: -2.0 ** -1000})], why="negative")
    refused(INVALID, [dict(caps[0], radius=0.0, margin=0.0)] + [dict(caps[0], radius=-1.0)], why="capsule 1")
    refused(NULL)                                                             # all of it in order: the handle is missing
    refused(NULL, [])                                                         # no capsules at all: mi_gomp_scene_create_chain's answer
    out = C.c_void_p()
    cc = K.DH.c_chain(s["chain"])
    assert L.mi_gomp_scene_create_world(None, None, 8, 2, C.byref(cc), 1, G.c_balls(s["balls"]), 0, None, 1, K.c_capsules(caps), None, None) == NULL
    assert L.mi_gomp_scene_create_world(C.byref(out), None, 8, 2, C.byref(cc), 1, None, 0, None, 1, K.c_capsules(caps), None, None) == NULL and not out
