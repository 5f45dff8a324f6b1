"""CPU: the C-ABI of the self-collision pairs - the struct and the definition as the header states them, the struct's size, the
exported symbol, and every refusal mi_gomp_scene_create_pairs decides before it looks at the handle."""
import ctypes as C
import os
import re

import numpy as np

import dh_refs as DH
import gomp_refs as G
import osqp_solver_amd as M
import pair_refs as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL


def test_header_struct_definition_and_symbol():
    with open(os.path.join(ROOT, "include", "mi_osqp.h")) as f:
        text = f.read()
    assert "typedef struct { int32_t a, b; double margin; } mi_gomp_pair;" in text
    assert re.search(r"\bint mi_gomp_scene_create_pairs\(mi_gomp_scene \*\*out, mi_osqp_batch \*h, int64_t dims, int64_t waypoints,\s*"
                     r"const mi_gomp_chain \*chain, int64_t n_balls, const mi_gomp_ball \*balls,\s*"
                     r"int64_t n_lines, const mi_gomp_line \*lines, int64_t n_capsules, const mi_gomp_capsule \*capsules,\s*"
                     r"int64_t n_cuboids, const mi_gomp_cuboid \*cuboids, int64_t n_pairs, const mi_gomp_pair \*pairs,\s*"
                     r"const double \*con_lo, const double \*con_hi\);", text)
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", text))                     # the definition stands at the struct
    for piece in ("v = p_a - p_b;", "dist > 1e-12: n = v / dist; otherwise n = (0, 0, 1);", "reach = r_a + r_b;", "s = dist - reach;",
                  "l = (reach - dist) + sum_j g_j q_w[j], u = +1e30; otherwise l = -1e30, u = +1e30", "s >= -1e-3 at every (pair, waypoint)"):
        assert piece in flat, piece
    assert C.sizeof(P.Pair) == 16
    assert hasattr(M.lib(), "mi_gomp_scene_create_pairs")


def _create(pairs, balls=None, **kw):
    L = P.declare(M.lib())
    s = P.scene("P8")
    rc, ptr = P.create_pairs(L, None, 8, 2, s["chain"], s["balls"] if balls is None else balls, s["lines"], s["capsules"], s["cuboids"], pairs,
                             s["con_lo"], s["con_hi"], **kw)
    assert not ptr                                                            # it was 1 before the call
    return rc, L.mi_osqp_last_error().decode()


def test_refusals_that_need_no_handle():
    ok = P.pair(0, 1, 0.1)
    rc, why = _create([ok], null_pairs=True)
    assert rc == NULL and "no pairs" in why
    rc, why = _create([ok], n_pairs=-1)
    assert rc == INVALID and "negative" in why
    for margin in (np.nan, np.inf, -np.inf, -0.01, -2.0 ** -1000):
        rc, why = _create([ok, P.pair(1, 0, margin)])
        assert rc == INVALID and "pair 1" in why and "margin" in why, (margin, why)
    for a, b in ((-1, 1), (0, 2), (2, 0), (1, -1), (0, 2 ** 31 - 1)):
        rc, why = _create([ok, ok, P.pair(a, b, 0.0)])
        assert rc == INVALID and "pair 2" in why and "n_balls" in why, (a, b, why)
    rc, why = _create([P.pair(1, 1, 0.0)])
    assert rc == INVALID and "pair 0" in why and "itself" in why
    # two chain balls of one frame: their distance does not depend on the joints
    c8 = P.scene("P8")["chain"]
    balls = [DH.chain_ball(c8, 3, (0.1, 0, 0), 0, 0.05), DH.chain_ball(c8, 8, (0, 0, 0.02), 1, 0.04), DH.chain_ball(c8, 3, (0, 0.1, 0), 0, 0.05)]
    rc, why = _create([P.pair(0, 1, 0.0), P.pair(2, 0, 0.0)], balls=balls)
    assert rc == INVALID and "pair 1" in why and "one frame" in why
    # accepted as far as the handle check (the handle is NULL here): either order, margin 0 and -0.0, frames 3 and 8
    for prs in ([ok], [P.pair(1, 0, 0.0)], [P.pair(0, 1, -0.0)], [ok, ok], []):
        rc, why = _create(prs)
        assert rc == NULL, (prs, rc, why)
    assert _create([P.pair(0, 1), P.pair(2, 1)], balls=balls)[0] == NULL


def test_refusals_before_the_handle_leave_out_null():
    L = P.declare(M.lib())
    s = P.scene("P8")
    out = C.c_void_p(1234)
    cc = DH.c_chain(s["chain"])
    bad = P.c_pairs([P.pair(0, 0, 0.0)])
    rc = L.mi_gomp_scene_create_pairs(C.byref(out), None, 8, 2, C.byref(cc), 2, G.c_balls(s["balls"]), 0, None, 0, None, 0, None, 1, bad, None, None)
    assert rc == INVALID and not out
    good = P.c_pairs(s["pairs"])
    assert L.mi_gomp_scene_create_pairs(None, None, 8, 2, C.byref(cc), 2, G.c_balls(s["balls"]), 0, None, 0, None, 0, None, 1, good, None, None) == NULL
