"""GPU (-m gpu): grasp goals (mi_gomp_goal, the goal items of gomp_relinearise_kernel) through mi_gomp_scene_create_goals,
mi_gomp_scene_set_goal_values and every call that launches the kernel, against the mpmath reference of tests/goal_refs.py.

B = 8; every QP asks something else of the goals, and the id lists are permuted strict subsets ([5,2,7,0,3], [6,1,4]) with QP b
linearised around trajectory b: values read at the position in the list instead of at the QP's id would show in every scene.
Scene G7 (the 7-joint chain, 40 waypoints, 7 balls, 14 pairs, 7 tilts; goals at waypoints 37 - frame 7 - and 20 - position only),
scene G8 (8 joints, 2 waypoints, goals at waypoints 0 and 1 with frames 8 and 1: the last joint, a one-column gradient), scene GF
(the flips: a position error of tol + 1e-3 -+ 2^-20 on either side, the angle at max_angle + 1e-3 -+ 2^-20, a free axis,
tol = 0), scene GX (the TABLE model, identity rotations, dyadic values, compared BIT FOR BIT, with the zero row of frame 0 and the
antiparallel case) and scene GM (goals behind a gripper ball's rows, lines, a capsule, a cuboid, a grid, pairs and tilts, once
with the builder's over-allocated empty rows behind them: the row order).  Rows within 32 x the fp64 error of the formulas
themselves and never looser than 1e-13 (goal_refs.gpu_tolerance; tests/test_goal_refs.py holds the figures); no verdict is
excluded; joint-space entries, unlisted QPs and unpopulated rows bit for bit.  Run with -s to see the figures."""
import ctypes as C

import numpy as np
import pytest

import gomp_refs as G
import goal_refs as Q
import grid_refs as R
import osqp_solver_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu
B = Q.B
IDS_A, IDS_B = [5, 2, 7, 0, 3], [6, 1, 4]          # permuted strict subsets of the batch
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _why():
    return M.lib().mi_osqp_last_error().decode()


def _make(name, over=False, **kw):
    s, pr = Q.scene(name), Q.scene_batch(name, over)
    solver = _solver(pr, **kw)
    sc = Q.GoalScene(M.lib(), solver, s)
    assert sc.rc == 0, (sc.rc, _why())
    return solver, sc, pr


@pytest.fixture(scope="module")
def handles():
    """One handle and scene per (scene, settings), made on first use and kept for the module."""
    made = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = _make(name, **kw)
        return made[key]

    yield get
    for solver, sc, _ in made.values():
        sc.close()
        solver.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _check_rows(name, pr, got, ref, worst, exact=None):
    """The rows (A, l, u) read back for a listed QP against the reference `ref` of its trajectory and values and, outside the
    populated 3-D rows, against what set_rows wrote (got[3:])."""
    A, l, u, A0, l0, u0 = got
    r0, r1 = pr["row0"], pr["row0"] + pr["rows3d"]
    assert pr["rows3d"] == len(ref["l"])
    joint = np.ones(len(A), bool)
    joint[pr["aidx"].reshape(-1)] = False
    assert _same_bits(A[joint], A0[joint])                                    # joint-space entries
    assert _same_bits(l[:r0], l0[:r0]) and _same_bits(u[:r0], u0[:r0])
    assert _same_bits(l[r1:], l0[r1:]) and _same_bits(u[r1:], u0[r1:])        # unpopulated rows (behind the last goal row)
    vals = A[pr["aidx"]]
    tv, tb = Q.gpu_tolerance(name)
    assert not ref["near"].any() and not ref["verdict_excluded"]
    ev = float(np.max(np.abs(vals - ref["vals"])))
    worst["values"] = max(worst.get("values", 0.0), ev)
    bounds = []
    for side, dev in (("l", l[r0:r1]), ("u", u[r0:r1])):
        sc = ref[side + "_scale"]
        inf = sc == 0
        assert _same_bits(dev[inf], ref[side][inf])                           # an absent side, a free axis, the zero row: -+1e30 exactly
        fin = sc > 0
        eb = float(np.max(np.abs(dev[fin] - ref[side][fin]) / sc[fin], initial=0.0))
        worst["bounds"] = max(worst.get("bounds", 0.0), eb)
        bounds.append((side, eb))
    assert ev <= tv, (ev, tv)
    for side, eb in bounds:
        assert eb <= tb, (side, eb, tb)
    zero = np.array([c == "zero" for c in ref["cls"]])
    assert not vals[zero].any()                                               # the zeros are written (set_rows wrote ones)
    if name in Q.EXACT if exact is None else exact:                           # the exact scene: bit for bit
        assert np.array_equal(vals, ref["vals"]) and np.array_equal(l[r0:r1], ref["l"]) and np.array_equal(u[r0:r1], ref["u"])


def _check_verdicts(ok, refs):
    for j, r in enumerate(refs):
        assert ok[j] in (0, 1)
        assert not r["verdict_excluded"]
        assert bool(ok[j]) == r["ok"], j


def _rows_and_verdicts(name, sc, pr):
    s, ref = Q.scene(name), Q.scene_reference(name)
    worst = {}
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    before = [sc.get_rows(b) for b in range(B)]
    for ids in (IDS_A, IDS_B):                                                # the values too go in by permuted lists
        assert sc.set_goal_values(ids, [s["values"][b] for b in ids]) == 0, _why()
    assert all(_same_bits(x, y) for b in range(B) for x, y in zip(sc.get_rows(b), before[b]))     # kept rows are not touched
    rc, ok = sc.assemble_some(IDS_A, s["trajs"][IDS_A])                       # QP b is linearised around trajectory b
    assert rc == 0, _why()
    _check_verdicts(ok, [ref[b] for b in IDS_A])
    first = [sc.get_rows(b) for b in range(B)]
    for b in range(B):
        if b in IDS_A:
            _check_rows(name, pr, first[b] + before[b], ref[b], worst)
        else:
            assert all(_same_bits(x, y) for x, y in zip(first[b], before[b]))             # a QP not listed: untouched
    rc, ok = sc.assemble_some(IDS_B, s["trajs"][IDS_B])
    assert rc == 0
    _check_verdicts(ok, [ref[b] for b in IDS_B])
    for b in range(B):
        got = sc.get_rows(b)
        if b in IDS_B:
            _check_rows(name, pr, got + before[b], ref[b], worst)
        else:
            assert all(_same_bits(x, y) for x, y in zip(got, first[b]))
    tv, tb = Q.gpu_tolerance(name)
    print(f"\nscene {name}: worst device - reference: values {worst['values']:.3e} (tolerance {tv:.3e}),"
          f" bounds {worst['bounds']:.3e} of their term scale (tolerance {tb:.3e})")


@pytest.mark.parametrize("name,over", [("G7", False), ("G8", False), ("GF", False), ("GX", False), ("GM", False), ("GM", True)])
def test_rows_and_verdicts_of_permuted_id_lists(handles, name, over):
    solver, sc, pr = handles(name, over=over)
    if over:
        assert pr["m"] > pr["row0"] + pr["rows3d"]                            # empty rows behind the last goal row
    _rows_and_verdicts(name, sc, pr)


def test_the_flips_of_scene_GF_on_the_device(handles):
    """What tests/test_goal_refs.py pins in the reference, read from the device: 2^-20 decide the verdict, with write_rows 2
    (mi_gomp_relinearise_some) an accepted QP keeps its rows and a rejected one gets new ones."""
    solver, sc, pr = handles("GF", over=False)
    s, ref = Q.scene("GF"), Q.scene_reference("GF")
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    assert sc.set_goal_values(range(B), s["values"]) == 0
    rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
    assert rc == 0 and ok.tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    g0 = pr["row0"] + ref[0]["goal_rows0"]
    A, l, u = sc.get_rows(6)
    assert l[g0 + 4] == -G.INF and u[g0 + 4] == G.INF and A[pr["aidx"][ref[0]["goal_rows0"] + 4]].tolist() == [1.0, 0.0, 0.0]       # the free axis: the row is written
    A, l, u = sc.get_rows(7)
    assert np.array_equal(l[g0 + 4:g0 + 7], u[g0 + 4:g0 + 7])                 # tol = 0: equalities
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    rc, ok = sc.relinearise_some(list(range(B)), s["trajs"])
    assert rc == 0 and ok.tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    for b in range(B):
        got = sc.get_rows(b)
        if ok[b]:
            assert all(_same_bits(p, q) for p, q in zip(got, (pr["Ax"][b], pr["l"][b], pr["u"][b])))
        else:
            _check_rows("GF", pr, got + (pr["Ax"][b], pr["l"][b], pr["u"][b]), ref[b], {})


def test_new_values_give_the_rows_of_a_fresh_scene_made_with_them():
    """set_goal_values then assemble_some is bit-identical to a fresh scene given those values, and is the reference of the new
    values (scene GX stays exact: QP b gets what QP b + 1 asked)."""
    s, pr = Q.scene("GX"), Q.scene_batch("GX")
    new = [s["values"][(b + 1) % B] for b in range(B)]
    refs = [Q.reference(s, b, values=new[b]) for b in range(B)]
    assert [r["ok"] for r in refs] != [r["ok"] for r in Q.scene_reference("GX")]          # the new values change verdicts
    got = {}
    for which in ("updated", "fresh"):
        h = _solver(pr)
        sc = Q.GoalScene(M.lib(), h, s)
        assert sc.rc == 0 and sc.ptr
        assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
        if which == "updated":
            assert sc.set_goal_values(range(B), s["values"]) == 0
            rc, ok = sc.assemble_some(list(range(B)), s["trajs"])             # the old values first
            assert rc == 0 and ok.tolist() == [int(r["ok"]) for r in Q.scene_reference("GX")]
            kept = [sc.get_rows(b) for b in range(B)]
            bad = [dict(new[0][0], tol=[0.0, -1.0, 0.0])] + new[0][1:]
            assert sc.set_goal_values([3, 0], [new[3], bad]) == INVALID and "goal 0 of QP 0" in _why()      # refused: nothing changes, not QP 3 either
            rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
            assert rc == 0 and all(_same_bits(x, y) for b in range(B) for x, y in zip(sc.get_rows(b), kept[b]))
            assert sc.set_goal_values(IDS_A, [new[b] for b in IDS_A]) == 0 and sc.set_goal_values(IDS_B, [new[b] for b in IDS_B]) == 0
            assert all(_same_bits(x, y) for b in range(B) for x, y in zip(sc.get_rows(b), kept[b]))     # kept rows are not touched
        else:
            assert sc.set_goal_values(range(B), new) == 0
        rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
        assert rc == 0
        got[which] = (ok.tolist(), [sc.get_rows(b) for b in range(B)])
        if which == "fresh":
            for b in range(B):
                _check_rows("GX", pr, got[which][1][b] + (pr["Ax"][b], pr["l"][b], pr["u"][b]), refs[b], {})
        sc.close()
        h.close()
    assert got["updated"][0] == got["fresh"][0] == [int(r["ok"]) for r in refs]
    for a, b in zip(got["updated"][1], got["fresh"][1]):
        assert all(_same_bits(x, y) for x, y in zip(a, b))


def test_no_goals_is_the_grid_entry_point_bit_for_bit():
    """n_goals = 0 through mi_gomp_scene_create_goals against mi_gomp_scene_create_grids on scene GM without its goals; set_goal_values
    refuses a scene without goals, and such a scene needs no values."""
    L = Q.declare(M.lib())
    s, pr = Q.scene("GM"), Q.scene_batch("GM", with_goals=False)
    got = {}
    for which in ("grids", "goals"):
        h = _solver(pr)
        if which == "grids":
            sc = R.GridScene(L, h, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["pairs"], s["tilts"], s["grids"],
                             s["con_lo"], s["con_hi"])
        else:
            sc = Q.GoalScene(L, h, s, goals=[])
            assert sc.set_goal_values([0], [[]]) == INVALID and "no goals" in _why()
        assert sc.rc == 0 and sc.ptr
        assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
        rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
        assert rc == 0
        got[which] = (ok.tolist(), [sc.get_rows(b) for b in range(B)])
        sc.close()
        h.close()
    base = [R.with_obstacles(s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["pairs"], s["tilts"], s["grids"],
                             s["con_lo"], s["con_hi"], t) for t in s["trajs"]]
    assert got["grids"][0] == got["goals"][0] == [int(e["ok"]) for e in base]
    for a, b in zip(got["grids"][1], got["goals"][1]):
        assert all(_same_bits(x, y) for x, y in zip(a, b))


def test_relinearise_some_on_scene_GX_and_the_solves_that_follow(handles):
    solver, sc, pr = handles("GX", over=False, scaling=0)
    s, ref = Q.scene("GX"), Q.scene_reference("GX")
    ids = [5, 2, 7, 0, 3, 1, 4, 6]
    x = s["trajs"][ids]                                                      # QP b gets trajectory b, in the order of the list
    rejected = [b for b in range(B) if not ref[b]["ok"]]
    assert len(rejected) >= 4 and Q.GX_ANTI in rejected and len(rejected) < B
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    assert sc.set_goal_values(range(B), s["values"]) == 0
    rc, ok = sc.relinearise_some(ids, x)
    assert rc == 0, _why()
    _check_verdicts(ok, [ref[b] for b in ids])
    rows = {}
    for b in range(B):
        got = sc.get_rows(b)
        if b in rejected:                                                    # rewritten ...
            _check_rows("GX", pr, got + (pr["Ax"][b], pr["l"][b], pr["u"][b]), ref[b], {})
            rows[b] = got
        else:                                                                # accepted: as set_rows wrote
            assert all(_same_bits(p, q) for p, q in zip(got, (pr["Ax"][b], pr["l"][b], pr["u"][b])))
    # ... and updated: solved from the device's rows, against the oracle fed with the rows read back
    for b in rejected:
        solver.warm_start_x_some([b], s["trajs"][b])
    solver.solve_begin_some(rejected)
    for _ in range(400):
        if not solver.running():
            break
        solver.advance(1)
        solver.poll(True)
    assert not solver.running()
    infos, xs = solver.info_some(rejected), solver.primal_some(rejected)
    statuses = []
    for k, b in enumerate(rejected):
        Ax, l, u = rows[b]
        A = pr["A"].copy()
        A.data = Ax
        o = O.OracleQPSolver(pr["P"], None, pr["A"], pr["l"][b], pr["u"][b], scaling=0)
        o.update(l, A, u)
        o.set_warm_start(s["trajs"][b])
        st, xo = o.solve()
        print(f"\nscene GX, QP {b}: device status {infos[k].status_val} after {infos[k].iter} iterations, oracle {st} after {o.info().iter}")
        assert (infos[k].status_val, infos[k].iter) == (st, o.info().iter), b
        statuses.append(st)
        if st == 1:
            assert np.max(np.abs(xs[k] - xo)) <= 1e-6
    assert statuses[rejected.index(Q.GX_ANTI)] == -3                          # the antiparallel case: primal infeasible


def test_refusals_leave_the_handle_usable():
    L = Q.declare(M.lib())
    s, pr = Q.scene("G8"), Q.scene_batch("G8")
    h = _solver(pr)

    def refused(code, goals, why=None, **kw):
        rc, ptr = Q.create_goals(L, h._h, 8, 2, s["chain"], s["balls"], [], [], [], [], [], [], goals, None, None, **kw)
        assert rc == code and not ptr, (rc, ptr, _why())
        if why:
            assert why in _why(), _why()

    ok = s["goals"]
    refused(NULL, ok, null_goals=True, why="no goals")
    refused(INVALID, ok, n_goals=5, why="0 .. 4")
    refused(INVALID, [dict(ok[0], ball=1)], why="goal 0: ball")
    refused(INVALID, [dict(ok[0], waypoint=2)], why="goal 0: waypoint")
    refused(INVALID, [ok[0], dict(ok[1], frame=9)], why="goal 1: frame")
    refused(INVALID, [dict(ok[0], axis=(1, 1, 0))], why="unit")
    refused(INVALID, ok + [ok[0]], why="does not hold")                       # four rows more than the matrix has
    assert "(goal 2)" in _why()
    info = h.solve()                                                         # after all that the handle solves ...
    assert len(info) == B and all(i.iter > 0 for i in info)
    sc = Q.GoalScene(L, h, s)
    assert sc.rc == 0 and sc.ptr                                             # ... and takes a scene
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    kept = [sc.get_rows(b) for b in range(B)]
    # a QP whose values were never set is not linearised, whatever else the list holds
    for fn in (sc.assemble_some, sc.relinearise_some):
        rc, _ = fn([0], s["trajs"][:1])
        assert rc == INVALID and "QP 0" in _why() and "never set" in _why()
    assert sc.set_goal_values([2, 4], [s["values"][2], s["values"][4]]) == 0
    rc, _ = sc.assemble_some([4, 3, 2], s["trajs"][[4, 3, 2]])
    assert rc == INVALID and "QP 3" in _why()
    assert all(_same_bits(x, y) for b in range(B) for x, y in zip(sc.get_rows(b), kept[b]))
    good = s["values"][1]

    def values_refused(vals, why, ids=(1,)):
        assert sc.set_goal_values(list(ids), [vals]) == INVALID and why in _why(), _why()

    for i in range(3):
        for field in ("point", "tol", "ref"):
            for v in (np.nan, np.inf):
                bad = list(good[0][field])
                bad[i] = v
                values_refused([dict(good[0], **{field: bad}), good[1]], "not finite")
    values_refused([good[0], dict(good[1], max_angle=np.nan)], "goal 1 of QP 1")
    values_refused([dict(good[0], tol=[0.0, 0.0, -1e-300]), good[1]], "tol")
    values_refused([dict(good[0], ref=[0.6, 0.8, 1e-4]), good[1]], "ref")
    for ma in (0.0, -0.5, np.pi, 4.0):
        values_refused([good[0], dict(good[1], max_angle=ma)], "max_angle")
    values_refused(good, "id 8", ids=(8,))
    values_refused(good, "id -1", ids=(-1,))
    assert sc.L.mi_gomp_scene_set_goal_values(sc.ptr, 1, None, Q.c_values([good])) == NULL
    rc, _ = sc.assemble_some([1], s["trajs"][1:2])                            # none of that set QP 1's values
    assert rc == INVALID and "QP 1" in _why()
    _rows_and_verdicts("G8", sc, pr)                                         # the scene works
    refused(INVALID, ok, why="already has a scene")
    sc.close()
    h.close()


def test_struct_sizes_and_symbols():
    assert C.sizeof(Q.Goal) == 40 and C.sizeof(Q.GoalValue) == 80
    assert hasattr(M.lib(), "mi_gomp_scene_create_goals") and hasattr(M.lib(), "mi_gomp_scene_set_goal_values")
