"""CPU: the C-ABI of the cuboid obstacles - the struct as the header states it, its size, the exported symbol, and every refusal
mi_gomp_scene_create_cuboids decides before it looks at the handle."""
import ctypes as C
import os
import re

import numpy as np

import cuboid_refs as X
import gomp_refs as G
import osqp_solver_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL


def test_header_struct_and_symbol():
    with open(os.path.join(ROOT, "include", "mi_osqp.h")) as f:
        text = f.read()
    assert "typedef struct { double centre[3]; double axes[9]; double half[3]; double radius; double margin; } mi_gomp_cuboid;" in text
    assert re.search(r"\bint mi_gomp_scene_create_cuboids\(mi_gomp_scene \*\*out, mi_osqp_batch \*h, int64_t dims, int64_t waypoints,\s*"
                     r"const mi_gomp_chain \*chain, int64_t n_balls, const mi_gomp_ball \*balls,\s*"
                     r"int64_t n_lines, const mi_gomp_line \*lines, int64_t n_capsules, const mi_gomp_capsule \*capsules,\s*"
                     r"int64_t n_cuboids, const mi_gomp_cuboid \*cuboids, const double \*con_lo, const double \*con_hi\);", text)
    assert C.sizeof(X.Cuboid) == 136
    assert hasattr(M.lib(), "mi_gomp_scene_create_cuboids")


def _create(cuboids, **kw):
    L = X.declare(M.lib())
    s = X.scene("X8")
    rc, ptr = X.create_cuboids(L, None, 8, 2, s["chain"], s["balls"], s["lines"], s["capsules"], cuboids, s["con_lo"], s["con_hi"], **kw)
    assert not ptr
    return rc, L.mi_osqp_last_error().decode()


def _with(base, **kw):
    c = dict(base, centre=list(base["centre"]), axes=list(base["axes"]), half=list(base["half"]))
    for k, v in kw.items():
        if isinstance(v, tuple):
            c[k][v[0]] = v[1]
        else:
            c[k] = v
    return c


def test_refusals_that_need_no_handle():
    base = X.scene("X8")["cuboids"][0]
    rc, why = _create([base], null_cuboids=True)
    assert rc == NULL and "no cuboids" in why
    rc, why = _create([base], n_cuboids=-1)
    assert rc == INVALID and "negative" in why
    for kw in (dict(centre=(1, np.nan)), dict(axes=(4, np.inf)), dict(half=(2, np.nan)), dict(radius=np.nan), dict(margin=-np.inf)):
        rc, why = _create([base, _with(base, **kw)])
        assert rc == INVALID and "cuboid 1" in why and "not finite" in why, (kw, why)
    for kw in (dict(half=(0, -0.01)), dict(half=(2, -2.0 ** -1000)), dict(radius=-0.01), dict(margin=-1e-300)):
        rc, why = _create([_with(base, **kw)])
        assert rc == INVALID and "cuboid 0" in why and "negative" in why, (kw, why)


def test_axes_must_be_orthonormal_to_1e_9():
    base = X.cuboid((0.1, 0.2, 0.3), (0.1, 0.2, 0.3), 0.01, 0.02)
    for kw in (dict(axes=(0, 1 + 1e-6)), dict(axes=(1, 1e-6)), dict(axes=(8, 1 - 1e-6)), dict(axes=(5, -1e-6))):
        rc, why = _create([base, base, _with(base, **kw)])
        assert rc == INVALID and "cuboid 2" in why and "orthonormal" in why, (kw, why)
    # accepted as far as the handle check (the handle is NULL here): off by 1e-12, a left-handed frame, a turned frame, zero half extents
    left = _with(base, axes=(8, -1.0))
    assert np.linalg.det(np.array(left["axes"]).reshape(3, 3)) == -1.0
    for c in (_with(base, axes=(0, 1 + 1e-12)), _with(base, axes=(1, 1e-12)), left, X.scene("X7")["cuboids"][0], _with(base, half=[0.0, 0.0, 0.0]),
              X.scene("XT")["cuboids"][1]):
        rc, why = _create([c])
        assert rc == NULL, (c, rc, why)


def test_refusals_before_the_handle_leave_out_null():
    L = X.declare(M.lib())
    s = X.scene("X8")
    out = C.c_void_p(1234)
    cc = X.DH.c_chain(s["chain"])
    bad = [_with(s["cuboids"][0], radius=-1.0)]
    rc = L.mi_gomp_scene_create_cuboids(C.byref(out), None, 8, 2, C.byref(cc), 1, G.c_balls(s["balls"]), 0, None, 0, None, 1, X.c_cuboids(bad), None, None)
    assert rc == INVALID and not out
    assert L.mi_gomp_scene_create_cuboids(None, None, 8, 2, C.byref(cc), 1, G.c_balls(s["balls"]), 0, None, 0, None, 1, X.c_cuboids(s["cuboids"]), None, None) == NULL
