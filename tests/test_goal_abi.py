"""CPU: the C-ABI of the grasp goals - the structs and the definition as the header states them, the structs' sizes and field
offsets, the exported symbols, and every refusal mi_gomp_scene_create_goals and mi_gomp_scene_set_goal_values decide before they
look at the handle or the scene.  (The refusals that need a handle - a matrix without the rows, an id out of range, values that
are not finite, a negative tol, a ref that is no unit vector, a max_angle outside (0, pi), a QP whose values were never set -
are in tests/test_gpu_goals.py.)"""
import ctypes as C
import os
import re

import numpy as np

import dh_refs as DH
import gomp_refs as G
import goal_refs as Q
import osqp_solver_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL


def test_header_struct_definitions_and_symbols():
    with open(os.path.join(ROOT, "include", "mi_osqp.h")) as f:
        text = f.read()
    assert "typedef struct { int32_t ball; int32_t waypoint; int32_t frame; int32_t reserved; double axis[3]; } mi_gomp_goal;" in text
    assert "typedef struct { double point[3]; double tol[3]; double ref[3]; double max_angle; } mi_gomp_goal_value;" in text
    assert re.search(r"\bint mi_gomp_scene_create_goals\(mi_gomp_scene \*\*out, mi_osqp_batch \*h, int64_t dims, int64_t waypoints, const mi_gomp_chain \*chain,\s*"
                     r"int64_t n_balls, const mi_gomp_ball \*balls, int64_t n_lines, const mi_gomp_line \*lines,\s*"
                     r"int64_t n_capsules, const mi_gomp_capsule \*capsules, int64_t n_cuboids, const mi_gomp_cuboid \*cuboids,\s*"
                     r"int64_t n_pairs, const mi_gomp_pair \*pairs, int64_t n_tilts, const mi_gomp_tilt \*tilts,\s*"
                     r"int64_t n_grids, const mi_gomp_grid \*grids, int64_t n_goals, const mi_gomp_goal \*goals,\s*"
                     r"const double \*con_lo, const double \*con_hi\);", text)
    assert "int mi_gomp_scene_set_goal_values(mi_gomp_scene *sc, int64_t n_ids, const int64_t *ids, const mi_gomp_goal_value *values);" in text
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", text))                     # the definition stands at the structs
    for piece in ("l = ((point_ax - tol_ax) - p_ax) + Jq_ax", "u = ((point_ax + tol_ax) - p_ax) + Jq_ax", "a free axis: l = -1e30, u = +1e30",
                  "fabs(p_ax - point_ax) <= tol_ax + 1e-3", "a NaN fails", "row 3, frame 0: zeros (written), l = -1e30, u = +1e30",
                  "l = (cos_lim - c) + sum_j g_j q_w[j]", "accepted only if c >= cos_ok", "cos_ok = cos(min(pi, max_angle + 1e-3))",
                  "primal infeasible", "seed on the right side", "first 3-D row + the rows of all ball blocks + waypoints * (n_pairs + n_tilts) + 4 k + r"):
        assert piece in flat, piece
    # four int32 and three doubles: 40 bytes; ten doubles: 80 bytes
    assert C.sizeof(Q.Goal) == 40 and [getattr(Q.Goal, n).offset for n, _ in Q.Goal._fields_] == [0, 4, 8, 12, 16]
    assert C.sizeof(Q.GoalValue) == 80 and [getattr(Q.GoalValue, n).offset for n, _ in Q.GoalValue._fields_] == [0, 24, 48, 72]
    assert "mi_gomp_goal;   /* 40 bytes */" in text and re.search(r"mi_gomp_goal_value;\s+/\* 80 bytes \*/", text)
    assert hasattr(M.lib(), "mi_gomp_scene_create_goals") and hasattr(M.lib(), "mi_gomp_scene_set_goal_values")


def _create(goals, chain="C8", **kw):
    L = Q.declare(M.lib())
    s = Q.scene("G8")
    rc, ptr = Q.create_goals(L, None, 8, 2, s["chain"] if chain == "C8" else chain, s["balls"], [], [], [], [], [], [], goals, None, None, **kw)
    if not kw.get("null_out"):
        assert not ptr                                                        # it was 1 before the call
    return rc, L.mi_osqp_last_error().decode()


def test_refusals_that_need_no_handle():
    ok = Q.scene("G8")["goals"]
    rc, why = _create(ok, null_goals=True)
    assert rc == NULL and "no goals" in why
    assert _create(ok, null_out=True)[0] == NULL
    for n in (-1, 5, 2 ** 40):
        rc, why = _create(ok, n_goals=n)
        assert rc == INVALID and "0 .. 4" in why, (n, why)
    for ball in (-1, 1, 2 ** 31 - 1):
        rc, why = _create([ok[0], dict(ok[1], ball=ball)])
        assert rc == INVALID and "goal 1" in why and "ball" in why, (ball, why)
    for w in (-1, 2, 40):
        rc, why = _create([dict(ok[0], waypoint=w)])
        assert rc == INVALID and "goal 0" in why and "waypoint" in why, (w, why)
    for frame in (-1, 9, 2 ** 31 - 1):
        rc, why = _create([ok[0], ok[1], dict(ok[1], frame=frame)])
        assert rc == INVALID and "goal 2" in why and "frame" in why, (frame, why)
    rc, why = _create([Q.goal(0, 1), ok[1]], chain=None)                      # a frame >= 1 without a chain (the chain ball is refused first)
    assert rc == NULL and "chain" in why
    for i in range(3):
        for v in (np.nan, np.inf, -np.inf):
            a = list(ok[0]["axis"])
            a[i] = v
            for frame in (0, 8):
                rc, why = _create([dict(ok[0], axis=a, frame=frame)])
                assert rc == INVALID and "goal 0" in why and "not finite" in why, (i, v, frame, why)
    for a in ((0.28, 0, 0.96 + 1e-8), (0, 0, 0), (2, 0, 0)):
        rc, why = _create([ok[0], dict(ok[1], axis=a)])
        assert rc == INVALID and "goal 1" in why and "unit" in why, (a, why)
    # accepted as far as the handle check (the handle is NULL here): no goals, four goals, a frame-0 goal whose axis is no unit
    # vector (it is not read), an axis within 1e-9 of a unit vector, the first and the last waypoint, frame = n_joints
    for gls in ([], ok, ok + ok, [dict(ok[0], frame=0, axis=(0, 0, 0))], [dict(ok[0], axis=(0.28, 0, 0.96 + 5e-10))], [Q.goal(0, 0, 8), Q.goal(0, 1, 1)]):
        rc, why = _create(gls)
        assert rc == NULL, (rc, why)


def test_a_table_scene_without_a_chain_takes_frame_0_only():
    L = Q.declare(M.lib())
    s = Q.scene("GX")
    rc, ptr = Q.create_goals(L, None, 3, s["W"], None, s["balls"], [], [], [], [], [], [], s["goals"], None, None)
    assert rc == NULL and not ptr and "goal 0" in L.mi_osqp_last_error().decode() and "no chain" in L.mi_osqp_last_error().decode()
    rc, ptr = Q.create_goals(L, None, 3, s["W"], None, s["balls"], [], [], [], [], [], [], [s["goals"][1]], None, None)
    assert rc == NULL and not ptr                                             # as far as the handle


def test_set_goal_values_without_a_scene():
    L = Q.declare(M.lib())
    ids, p = G._ids([0])
    vals = Q.c_values([[Q.value((0, 0, 0), (0, 0, 0))]])
    assert L.mi_gomp_scene_set_goal_values(None, 1, p, vals) == NULL
