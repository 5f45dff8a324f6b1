"""CPU: the C-ABI of the tilt limits - the struct and the definition as the header states them, the struct's size and field
offsets, the exported symbol, and every refusal mi_gomp_scene_create_tilts decides before it looks at the handle."""
import ctypes as C
import os
import re

import numpy as np

import dh_refs as DH
import gomp_refs as G
import osqp_solver_amd as M
import tilt_refs as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL


def test_header_struct_definition_and_symbol():
    with open(os.path.join(ROOT, "include", "mi_osqp.h")) as f:
        text = f.read()
    assert ("typedef struct { int32_t frame; int32_t reserved; double axis[3]; double ref[3]; double max_angle; double margin; } mi_gomp_tilt;"
            in text)
    assert re.search(r"\bint mi_gomp_scene_create_tilts\(mi_gomp_scene \*\*out, mi_osqp_batch \*h, int64_t dims, int64_t waypoints,\s*"
                     r"const mi_gomp_chain \*chain, int64_t n_balls, const mi_gomp_ball \*balls,\s*"
                     r"int64_t n_lines, const mi_gomp_line \*lines, int64_t n_capsules, const mi_gomp_capsule \*capsules,\s*"
                     r"int64_t n_cuboids, const mi_gomp_cuboid \*cuboids, int64_t n_pairs, const mi_gomp_pair \*pairs,\s*"
                     r"int64_t n_tilts, const mi_gomp_tilt \*tilts, const double \*con_lo, const double \*con_hi\);", text)
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", text))                     # the definition stands at the struct
    for piece in ("u_r = R_k[r][0] axis_0 + R_k[r][1] axis_1 + R_k[r][2] axis_2", "c = u_x ref_x + u_y ref_y + u_z ref_z",
                  "h_j = z_j x u; g_j = h_jx ref_x + h_jy ref_y + h_jz ref_z for j < k; g_j = 0 for j >= k",
                  "cos_lim = cos(max_angle); cos_act = cos(max(0, max_angle - margin)); cos_ok = cos(min(pi, max_angle + 1e-3))",
                  "active when c < cos_act", "l = (cos_lim - c) + sum_j g_j q_w[j], u = +1e30", "otherwise l = -1e30, u = +1e30",
                  "c >= cos_ok at every (tilt, waypoint)", "l = cos_lim + 1 > 0"):
        assert piece in flat, piece
    # two int32, eight doubles: 72 bytes, every double on a multiple of 8
    assert C.sizeof(T.Tilt) == 72
    assert [getattr(T.Tilt, n).offset for n, _ in T.Tilt._fields_] == [0, 4, 8, 32, 56, 64]
    assert "mi_gomp_tilt;   /* 72 bytes */" in text
    assert hasattr(M.lib(), "mi_gomp_scene_create_tilts")


def _create(tilts, chain=True, **kw):
    L = T.declare(M.lib())
    s = T.scene("T8")
    rc, ptr = T.create_tilts(L, None, 8, 2, s["chain"] if chain else None, s["balls"] if chain else [], [], [], [], [], tilts, None, None, **kw)
    assert not ptr                                                            # it was 1 before the call
    return rc, L.mi_osqp_last_error().decode()


def test_refusals_that_need_no_handle():
    ok = T.tilt(8, (0, 0, 1), (0, 0.6, 0.8), 0.5, 0.1)
    rc, why = _create([ok], null_tilts=True)
    assert rc == NULL and "no tilts" in why
    rc, why = _create([ok], chain=False)
    assert rc == NULL and "tilt 0" in why and "no chain" in why
    rc, why = _create([ok], n_tilts=-1)
    assert rc == INVALID and "negative" in why
    for frame in (0, -1, 9, 2 ** 31 - 1):
        rc, why = _create([ok, ok, dict(ok, frame=frame)])
        assert rc == INVALID and "tilt 2" in why and "frame" in why, (frame, why)
    for field in ("max_angle", "margin"):
        for v in (np.nan, np.inf, -np.inf):
            rc, why = _create([ok, dict(ok, **{field: v})])
            assert rc == INVALID and "tilt 1" in why and "not finite" in why, (field, v, why)
    for field in ("axis", "ref"):
        for i in range(3):
            vec = list(ok[field])
            vec[i] = np.nan
            rc, why = _create([dict(ok, **{field: vec})])
            assert rc == INVALID and "tilt 0" in why and "not finite" in why, (field, i, why)
        for vec in ((0, 0, 0), (0, 0, 1 + 2e-9), (0, 0, 1 - 2e-9), (1, 1, 0), (0.6, 0.8, 1e-4)):
            rc, why = _create([ok, dict(ok, **{field: [float(v) for v in vec]})])
            assert rc == INVALID and "tilt 1" in why and field in why and "unit" in why, (field, vec, why)
    for a in (0.0, -0.0, -1.0, np.pi, 3.2, 100.0):
        rc, why = _create([dict(ok, max_angle=a)])
        assert rc == INVALID and "tilt 0" in why and "max_angle" in why, (a, why)
    for mg in (-0.01, -2.0 ** -1000):
        rc, why = _create([ok, dict(ok, margin=mg)])
        assert rc == INVALID and "tilt 1" in why and "margin" in why, (mg, why)
    # accepted as far as the handle check (the handle is NULL here): every frame, the ends of (0, pi), margin 0, -0.0 and beyond
    # the cone's axis, vectors within 1e-9 of unit length
    for tls in ([ok], [dict(ok, frame=f) for f in range(1, 9)], [dict(ok, max_angle=2.0 ** -40)], [dict(ok, max_angle=float(np.nextafter(np.pi, 0)))],
                [dict(ok, margin=-0.0)], [dict(ok, margin=7.0)], [dict(ok, axis=[0.0, 0.0, 1 + 5e-10])], []):
        rc, why = _create(tls)
        assert rc == NULL, (tls, rc, why)


def test_refusals_before_the_handle_leave_out_null():
    L = T.declare(M.lib())
    s = T.scene("T8")
    out = C.c_void_p(1234)
    cc = DH.c_chain(s["chain"])
    bad = T.c_tilts([T.tilt(9, (0, 0, 1), (0, 0, 1), 0.5)])
    rc = L.mi_gomp_scene_create_tilts(C.byref(out), None, 8, 2, C.byref(cc), 1, G.c_balls(s["balls"]), 0, None, 0, None, 0, None, 0, None, 1, bad, None, None)
    assert rc == INVALID and not out
    good = T.c_tilts(s["tilts"])
    assert L.mi_gomp_scene_create_tilts(None, None, 8, 2, C.byref(cc), 1, G.c_balls(s["balls"]), 0, None, 0, None, 0, None, 0, None, 2, good, None, None) == NULL
