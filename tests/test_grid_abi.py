"""CPU: the C-ABI of the distance grids - the struct and the definition as the header states them, the struct's size and field
offsets, the exported symbols, and every refusal mi_gomp_scene_create_grids and mi_gomp_scene_update_grid decide before they
look at the handle or the scene."""
import ctypes as C
import os
import re

import numpy as np

import gomp_refs as G
import grid_refs as R
import osqp_solver_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL


def test_header_struct_definition_and_symbols():
    with open(os.path.join(ROOT, "include", "mi_osqp.h")) as f:
        text = f.read()
    assert re.search(r"typedef struct \{ double origin\[3\]; double cell; int32_t n\[3\]; int32_t reserved; double offset; double margin;\s*"
                     r"const double \*values; \} mi_gomp_grid;", text)
    assert re.search(r"\bint mi_gomp_scene_create_grids\(mi_gomp_scene \*\*out, mi_osqp_batch \*h, int64_t dims, int64_t waypoints, const mi_gomp_chain \*chain,\s*"
                     r"int64_t n_balls, const mi_gomp_ball \*balls, int64_t n_lines, const mi_gomp_line \*lines,\s*"
                     r"int64_t n_capsules, const mi_gomp_capsule \*capsules, int64_t n_cuboids, const mi_gomp_cuboid \*cuboids,\s*"
                     r"int64_t n_pairs, const mi_gomp_pair \*pairs, int64_t n_tilts, const mi_gomp_tilt \*tilts,\s*"
                     r"int64_t n_grids, const mi_gomp_grid \*grids, const double \*con_lo, const double \*con_hi\);", text)
    assert "int mi_gomp_scene_update_grid(mi_gomp_scene *sc, int64_t k, const double *values);" in text
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", text))                     # the definition stands at the struct
    for piece in ("f_k = (p_k - origin_k) * inv_cell", "f_k >= 0 and f_k <= n_k - 1", "i_k = min(n_k - 2, (int) floor(f_k)); t_k = f_k - i_k",
                  "e_bc = v_1bc - v_0bc; x_bc = v_0bc + t_0 * e_bc", "ey_c = x_1c - x_0c; y_c = x_0c + t_1 * ey_c", "ex_c = e_0c + t_1 * (e_1c - e_0c)",
                  "phi = y_0 + t_2 * (y_1 - y_0)", "G_x = (ex_0 + t_2 * (ex_1 - ex_0)) * inv_cell", "G_y = (ey_0 + t_2 * (ey_1 - ey_0)) * inv_cell",
                  "G_z = (y_1 - y_0) * inv_cell", "reach = offset + r; s = phi - reach", "g_j = G_x J[x][j] + G_y J[y][j] + G_z J[z][j]",
                  "l = (reach - phi) + sum_j g_j q_w[j], u = +1e30", "accepted only if s >= -1e-3", "V[(iz * n[1] + iy) * n[0] + ix]",
                  "primal infeasible"):
        assert piece in flat, piece
    # four doubles, four int32, two doubles, a pointer: 72 bytes, every double on a multiple of 8
    assert C.sizeof(R.Grid) == 72
    assert [getattr(R.Grid, n).offset for n, _ in R.Grid._fields_] == [0, 24, 32, 44, 48, 56, 64]
    assert "mi_gomp_grid;   /* 72 bytes" in text
    assert hasattr(M.lib(), "mi_gomp_scene_create_grids") and hasattr(M.lib(), "mi_gomp_scene_update_grid")


def _create(grids, **kw):
    L = R.declare(M.lib())
    s = R.scene("GT")
    rc, ptr = R.create_grids(L, None, 3, s["W"], None, s["balls"], [], [], [], [], [], grids, None, None, **kw)
    assert not ptr                                                            # it was 1 before the call
    return rc, L.mi_osqp_last_error().decode()


def test_refusals_that_need_no_handle():
    ok = R.scene("GT")["grids"][0]
    rc, why = _create([ok], null_grids=True)
    assert rc == NULL and "no grids" in why
    rc, why = _create([ok, ok], null_values=(1,))
    assert rc == NULL and "grid 1" in why and "values" in why
    rc, why = _create([ok], n_grids=-1)
    assert rc == INVALID and "negative" in why
    small = dict(ok, values=ok["values"][:8])
    for k in range(3):
        for bad in (1, 0, -3, 1025, 2 ** 31 - 1):
            n = [2, 2, 2]
            n[k] = bad
            rc, why = _create([ok, ok, dict(small, n=n)])
            assert rc == INVALID and "grid 2" in why and f"n[{k}]" in why, (k, bad, why)
    rc, why = _create([ok, dict(small, n=[1024, 1024, 17])])                 # each n[k] allowed, the product above 2^24 (refused before a value is read)
    assert rc == INVALID and "grid 1" in why and "2^24" in why
    for field in ("cell", "offset", "margin"):
        for v in (np.nan, np.inf, -np.inf):
            rc, why = _create([ok, dict(ok, **{field: v})])
            assert rc == INVALID and "grid 1" in why and "not finite" in why, (field, v, why)
    for v in (0.0, -0.0, -0.25):
        rc, why = _create([dict(ok, cell=v)])
        assert rc == INVALID and "grid 0" in why and "cell" in why, (v, why)
    for field in ("offset", "margin"):
        for v in (-0.01, -2.0 ** -1000):
            rc, why = _create([ok, dict(ok, **{field: v})])
            assert rc == INVALID and "grid 1" in why and field in why, (field, v, why)
    for i in range(3):
        for v in (np.nan, np.inf):
            o = list(ok["origin"])
            o[i] = v
            rc, why = _create([dict(ok, origin=o)])
            assert rc == INVALID and "grid 0" in why and "origin" in why and "not finite" in why, (i, v, why)
    for v in (np.nan, np.inf, -np.inf):
        vals = list(ok["values"])
        vals[(4 * 4 + 2) * 3 + 1] = v                                        # node (1, 2, 4) ...
        vals[-1] = np.nan                                                    # ... is the first of two
        rc, why = _create([ok, dict(ok, values=vals)])
        assert rc == INVALID and "grid 1" in why and "(1, 2, 4)" in why and "not finite" in why, (v, why)
    # accepted as far as the handle check (the handle is NULL here): the smallest and the largest n, offset and margin 0 and -0.0,
    # a tiny cell, negative and truncated values, no grids at all
    big = dict(ok, n=[1024, 2, 2], values=[0.0] * 4096)
    for grs in ([ok], [ok, ok], [small | dict(n=[2, 2, 2])], [big], [dict(ok, offset=-0.0, margin=-0.0)], [dict(ok, cell=2.0 ** -40)],
                [dict(ok, values=[-1.0] * 60)], []):
        rc, why = _create(grs)
        assert rc == NULL, (rc, why)


def test_refusals_before_the_handle_leave_out_null():
    L = R.declare(M.lib())
    s = R.scene("GT")
    out = C.c_void_p(1234)
    bad, keep = R.c_grids([dict(s["grids"][0], cell=-1.0)])
    rc = L.mi_gomp_scene_create_grids(C.byref(out), None, 3, 8, None, 1, G.c_balls(s["balls"]), 0, None, 0, None, 0, None, 0, None, 0, None, 1, bad, None, None)
    assert rc == INVALID and not out
    good, keep2 = R.c_grids(s["grids"])
    assert L.mi_gomp_scene_create_grids(None, None, 3, 8, None, 1, G.c_balls(s["balls"]), 0, None, 0, None, 0, None, 0, None, 0, None, 2, good, None, None) == NULL


def test_update_grid_without_a_scene():
    L = R.declare(M.lib())
    v = np.zeros(8)
    assert L.mi_gomp_scene_update_grid(None, 0, G._dp(v)) == NULL
