"""GPU (-m gpu): capsule and sphere obstacles (mi_gomp_capsule, the loop over g.caps in gomp_relinearise_kernel) through
mi_gomp_scene_create_world and every call that launches the kernel, against the mpmath reference of tests/capsule_refs.py.

Scene K7 (the 7-joint chain of dh_refs, 40 waypoints, 7 balls = 280 (ball, waypoint) pairs: both sides of the 256-thread
stride; a line, a sphere, a vertical post and a slanted capsule reached with t clamped at 0, inside and clamped at 1), scene K8
(8 joints, 2 waypoints, one ball, one sphere, no line), scene KT (TABLE model, identity: every waypoint on an axis through the
sphere's centre at a dyadic distance, compared BIT FOR BIT - the +Z normal at dist == 0, the activity flips at s = margin -+
2^-20, the verdict flips at s = -1e-3 -+ 2^-20, margin 0, radius 0, a segment of length 2^-30) and scene KM (capsules beside a
gripper ball with a box and two lines: the row order).  Rows within 32 x the fp64 error of the formulas themselves
(capsule_refs.gpu_tolerance; tests/test_capsule_refs.py holds the figures), no row of the committed trajectories within 1e-9
of a threshold and no verdict excluded; joint-space entries and unpopulated rows bit for bit.  The re-linearised QPs of KT are
solved and compared with the oracle on the rows read back.
Observed on an MI355X: K7 values 1.7e-15 / bounds 5.5e-15 of their term scale (tolerance 5.2e-14 / 9.9e-14), K8 6.4e-16 /
4.9e-16, KT 0 / 0, KM 1.1e-15 / 6.4e-16; the re-linearised QPs of KT: device and oracle both infeasible after 100 (QP 0) and 125
(QP 4) iterations, optimal after 25 (QP 3); the planners on the device against the host callbacks (tests/test_gomp_capsule_cpp.py):
max |dx| 6.3e-11 (point robot) and 1.9e-12 (7-joint chain).  Run with -s to see the figures."""
import ctypes as C

import numpy as np
import pytest

import capsule_refs as K
import dh_refs as DH
import gomp_refs as G
import osqp_solver_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu
B = 8
IDS_A, IDS_B = [5, 2, 7, 0, 3], [6, 1, 4]          # permuted strict subsets of the batch
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


@pytest.fixture(scope="module")
def handles():
    """One handle and scene per (scene, settings), made on first use and kept for the module."""
    made = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in made:
            s, pr = K.scene(name), K.scene_batch(name)
            solver = _solver(pr, **kw)
            sc = K.WorldScene(M.lib(), solver, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["con_lo"], s["con_hi"])
            made[key] = (solver, sc, pr)
            assert sc.rc == 0, (sc.rc, M.lib().mi_osqp_last_error())
        return made[key]

    yield get
    for solver, sc, _ in made.values():
        sc.close()
        solver.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _check_rows(name, pr, got, ref, worst):
    """The rows (A, l, u) read back for a listed QP against the reference `ref` of its trajectory and, outside the populated
    3-D rows, against what set_rows wrote (got[3:])."""
    A, l, u, A0, l0, u0 = got
    r0, r1 = pr["row0"], pr["row0"] + pr["rows3d"]
    joint = np.ones(len(A), bool)
    joint[pr["aidx"].reshape(-1)] = False
    assert _same_bits(A[joint], A0[joint])                                    # joint-space entries
    assert _same_bits(l[:r0], l0[:r0]) and _same_bits(u[:r0], u0[:r0])
    assert _same_bits(l[r1:], l0[r1:]) and _same_bits(u[r1:], u0[r1:])        # unpopulated rows
    vals = A[pr["aidx"]]
    tv, tb = K.gpu_tolerance(name)
    assert not ref["near"].any()
    ev = float(np.max(np.abs(vals - ref["vals"])))
    worst["values"] = max(worst.get("values", 0.0), ev)
    assert ev <= tv, (ev, tv)
    for side, dev in (("l", l[r0:r1]), ("u", u[r0:r1])):
        sc = ref[side + "_scale"]
        inf = sc == 0
        assert _same_bits(dev[inf], ref[side][inf])                           # an absent side, a dummy row, an inactive capsule: -+1e30 exactly
        fin = sc > 0
        eb = float(np.max(np.abs(dev[fin] - ref[side][fin]) / sc[fin], initial=0.0))
        worst["bounds"] = max(worst.get("bounds", 0.0), eb)
        assert eb <= tb, (side, eb, tb)
    if name == "KT":                                                          # the exact cases: bit for bit
        assert np.array_equal(vals, ref["vals"]) and np.array_equal(l[r0:r1], ref["l"]) and np.array_equal(u[r0:r1], ref["u"])


def _check_verdicts(ok, refs):
    for j, r in enumerate(refs):
        assert ok[j] in (0, 1)
        assert not r["verdict_excluded"]
        assert bool(ok[j]) == r["ok"], j


def _rows_and_verdicts(name, sc, pr):
    s, ref = K.scene(name), K.scene_reference(name)
    worst = {}
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    before = [sc.get_rows(b) for b in range(B)]
    for b in range(B):
        assert all(_same_bits(x, y) for x, y in zip(before[b], (pr["Ax"][b], pr["l"][b], pr["u"][b])))
    rc, ok = sc.assemble_some(IDS_A, s["trajs"][:5])                         # trajectory j goes to QP IDS_A[j]
    assert rc == 0, M.lib().mi_osqp_last_error()
    _check_verdicts(ok, ref[:5])
    first = [sc.get_rows(b) for b in range(B)]
    for b in range(B):
        if b in IDS_A:
            _check_rows(name, pr, first[b] + before[b], ref[IDS_A.index(b)], worst)
        else:
            assert all(_same_bits(x, y) for x, y in zip(first[b], before[b]))             # a QP not listed: untouched
    rc, ok = sc.assemble_some(IDS_B, s["trajs"][5:])
    assert rc == 0
    _check_verdicts(ok, ref[5:])
    for b in range(B):
        got = sc.get_rows(b)
        if b in IDS_B:
            _check_rows(name, pr, got + before[b], ref[5 + IDS_B.index(b)], worst)
        else:
            assert all(_same_bits(x, y) for x, y in zip(got, first[b]))
    tv, tb = K.gpu_tolerance(name)
    print(f"\nscene {name}: worst device - reference: values {worst['values']:.3e} (tolerance {tv:.3e}),"
          f" bounds {worst['bounds']:.3e} of their term scale (tolerance {tb:.3e})")


@pytest.mark.parametrize("name", K.SCENES)
def test_rows_and_verdicts_of_permuted_id_lists(handles, name):
    solver, sc, pr = handles(name)
    _rows_and_verdicts(name, sc, pr)


def test_the_exact_cases_of_scene_KT_on_the_device(handles):
    """What tests/test_capsule_refs.py pins in the reference, read from the device's rows: the +Z normal at dist == 0, the
    activity flips at s = margin -+ 2^-20 (margin 1/8 and margin 0), the verdict flips at s = -1e-3 -+ 2^-20."""
    solver, sc, pr = handles("KT")
    s = K.scene("KT")
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
    assert rc == 0 and ok.tolist() == [0, 1, 1, 0, 0, 1, 1, 1]               # 2 | 3: the verdict flips
    W, nc = s["W"], 2

    def row(b, ball, w, cap):
        A, l, u = sc.get_rows(b)
        k = (ball * W + w) * nc + cap
        return A[pr["aidx"][k]].tolist(), l[pr["row0"] + k], u[pr["row0"] + k]

    c = K.KT_C
    for ball, r in ((0, K.KT_RB), (1, K.KT_RB1)):
        assert row(0, ball, 2, 0) == ([0.0, 0.0, 1.0], K.KT_R0 + r + c[2], G.INF)
        assert row(0, ball, 2, 1) == ([0.0, 0.0, 1.0], r + c[2], G.INF)
    x1, x4 = s["trajs"][1][3 * 1], s["trajs"][1][3 * 4]
    assert row(1, 0, 1, 0) == ([1.0, 0.0, 0.0], K.E20 - K.KT_M0 + x1, G.INF)
    assert row(1, 0, 4, 0) == ([1.0, 0.0, 0.0], -G.INF, G.INF)
    assert x4 - x1 == 2 * K.E20
    assert row(4, 0, 1, 1) == ([1.0, 0.0, 0.0], K.E20 + s["trajs"][4][3 * 1], G.INF)
    assert row(4, 0, 3, 1) == ([1.0, 0.0, 0.0], -G.INF, G.INF)
    assert row(5, 1, 0, 1)[0] == [0.0, 0.0, 1.0] and row(5, 1, 2, 1)[0] == [0.0, 0.0, -1.0]


def _drain(s, max_advances=400):
    for _ in range(max_advances):
        if not s.running():
            return
        s.advance(1)
        s.poll(True)
    raise AssertionError("continuous solve did not finish")


@pytest.mark.parametrize("name", ["KT", "K7"])
def test_relinearise_some_and_the_solves_that_follow(handles, name):
    solver, sc, pr = handles(name, scaling=0)
    s, ref = K.scene(name), K.scene_reference(name)
    ids = [5, 2, 7, 0, 3, 1, 4, 6]
    x = s["trajs"][ids]                                                      # QP b gets trajectory b, in the order of the list
    rejected = [b for b in range(B) if not ref[b]["ok"]]
    assert rejected == ([0, 3, 4] if name == "KT" else [0, 2, 4, 5, 7])
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    rc, ok = sc.relinearise_some(ids, x)
    assert rc == 0, M.lib().mi_osqp_last_error()
    _check_verdicts(ok, [ref[b] for b in ids])
    worst, rows = {}, {}
    for b in range(B):
        got = sc.get_rows(b)
        if b in rejected:                                                    # rewritten ...
            _check_rows(name, pr, got + (pr["Ax"][b], pr["l"][b], pr["u"][b]), ref[b], worst)
            rows[b] = got
        else:                                                                # accepted: as set_rows wrote
            assert all(_same_bits(p, q) for p, q in zip(got, (pr["Ax"][b], pr["l"][b], pr["u"][b])))
    if name != "KT":
        return
    # ... and updated: solved from the device's rows, against the oracle fed with the rows read back
    for b in rejected:
        solver.warm_start_x_some([b], s["trajs"][b])
    solver.solve_begin_some(rejected)
    _drain(solver)
    infos, xs = solver.info_some(rejected), solver.primal_some(rejected)
    solved = 0
    for k, b in enumerate(rejected):
        Ax, l, u = rows[b]
        A = pr["A"].copy()
        A.data = Ax
        o = O.OracleQPSolver(pr["P"], None, pr["A"], pr["l"][b], pr["u"][b], scaling=0)
        o.update(l, A, u)
        o.set_warm_start(s["trajs"][b])
        st, xo = o.solve()
        print(f"\nQP {b}: device status {infos[k].status_val} after {infos[k].iter} iterations, oracle {st} after {o.info().iter}")
        assert (infos[k].status_val, infos[k].iter) == (st, o.info().iter), b
        if st == 1:
            solved += 1
            assert np.max(np.abs(xs[k] - xo)) <= 1e-6
    assert solved == 1                                                       # QP 3; QPs 0 and 4 are pinned inside the sphere: infeasible


def test_no_capsules_is_the_chain_entry_point_bit_for_bit():
    """n_capsules = 0 through mi_gomp_scene_create_world against mi_gomp_scene_create_chain on scene C7 of dh_refs."""
    L = K.declare(M.lib())
    s, pr = DH.scene("C7"), DH.scene_batch("C7")
    got = {}
    for which in ("chain", "world"):
        h = _solver(pr)
        if which == "chain":
            sc = DH.ChainScene(L, h, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["con_lo"], s["con_hi"])
        else:
            sc = K.WorldScene(L, h, s["D"], s["W"], s["chain"], s["balls"], s["lines"], [], s["con_lo"], s["con_hi"])
        assert sc.rc == 0 and sc.ptr
        assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
        rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
        assert rc == 0
        got[which] = (ok.tolist(), [sc.get_rows(b) for b in range(B)])
        sc.close()
        h.close()
    assert got["chain"][0] == got["world"][0] == [int(e["ok"]) for e in DH.scene_reference("C7")]
    for a, b in zip(got["chain"][1], got["world"][1]):
        assert all(_same_bits(x, y) for x, y in zip(a, b))


def test_refusals_leave_the_handle_usable():
    L = K.declare(M.lib())
    s, pr = K.scene("K8"), K.scene_batch("K8")
    h = _solver(pr)
    caps = s["capsules"]

    def refused(code, capsules=caps, why=None, handle=h, **kw):
        rc, ptr = K.create_world(L, handle._h, 8, 2, s["chain"], s["balls"], s["lines"], capsules, s["con_lo"], s["con_hi"], **kw)
        assert rc == code and not ptr, (rc, ptr, L.mi_osqp_last_error())
        if why:
            assert why in L.mi_osqp_last_error().decode(), L.mi_osqp_last_error()

    refused(NULL, null_capsules=True, why="no capsules")
    refused(INVALID, n_capsules=-1, why="negative")
    for key, bad in (("a", np.nan), ("b", np.inf), ("radius", np.nan), ("margin", -np.inf)):
        c = dict(caps[0], a=list(caps[0]["a"]), b=list(caps[0]["b"]))
        if key in ("a", "b"):
            c[key][1] = bad
        else:
            c[key] = bad
        refused(INVALID, [c], why="not finite")
    refused(INVALID, [dict(caps[0], radius=-0.01)], why="negative")
    refused(INVALID, [dict(caps[0], margin=-1e-300)], why="negative")
    refused(INVALID, caps + caps, why="does not hold the 3-D rows")          # a row per (ball, waypoint) more than the matrix has
    info = h.solve()                                                         # after all that the handle solves ...
    assert len(info) == B and all(i.iter > 0 for i in info)
    sc = K.WorldScene(L, h, 8, 2, s["chain"], s["balls"], s["lines"], caps, s["con_lo"], s["con_hi"])
    assert sc.rc == 0 and sc.ptr                                             # ... and takes a scene, which works
    _rows_and_verdicts("K8", sc, pr)
    refused(INVALID, why="already has a scene")
    sc.close()
    sc = K.WorldScene(L, h, 8, 2, s["chain"], s["balls"], s["lines"], caps, s["con_lo"], s["con_hi"])         # a second scene after the first
    assert sc.rc == 0 and sc.ptr
    sc.close()
    sc = K.WorldScene(L, h, 8, 2, None, [], [], caps, None, None)            # chain == NULL: mi_gomp_scene_create's case
    assert sc.rc == 0 and sc.ptr
    sc.close()
    rc, ptr = K.create_world(L, h._h, 8, 2, None, s["balls"], s["lines"], caps)        # ... which refuses chain balls
    assert rc == INVALID and not ptr
    h.close()


def test_struct_size_and_symbol():
    assert C.sizeof(K.Capsule) == 64
    assert hasattr(M.lib(), "mi_gomp_scene_create_world")
