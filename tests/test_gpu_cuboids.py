"""GPU (-m gpu): cuboid obstacles (mi_gomp_cuboid, the loop over g.cuboids in gomp_relinearise_kernel) through
mi_gomp_scene_create_cuboids and every call that launches the kernel, against the mpmath reference of tests/cuboid_refs.py.

Scene X7 (the 7-joint chain of dh_refs, 40 waypoints, 7 balls = 280 (ball, waypoint) pairs: both sides of the 256-thread
stride; a line, a capsule, a box turned about three axes, a plate and a rounded box), scene X8 (8 joints, 2 waypoints, one
ball, one cuboid, no line, no capsule), scenes XT and XP (TABLE model, identity, every row exact in fp64, compared BIT FOR BIT:
the six faces from inside, the three-way and two-way ties, points on faces, c = -0.0, the activity flips at s = margin -+ 2^-20
for margin 1/8 and margin 0, the verdict flips at s = -1e-3 -+ 2^-20, axes that are a signed permutation, a point cuboid at
out = 0) and scene XM (cuboids behind a gripper ball's work-space rows, two lines and a capsule: the row order).  Rows within
32 x the fp64 error of the formulas themselves and never looser than 1e-13 (cuboid_refs.gpu_tolerance;
tests/test_cuboid_refs.py holds the figures), no row of the committed trajectories within 1e-9 of a threshold and no verdict
excluded; joint-space entries and unpopulated rows bit for bit.  The re-linearised QPs of XT are solved and compared with the
oracle on the rows read back.  Scene K7 of capsule_refs with its slanted capsule as the equivalent cuboid gives the capsule's
rows within the sum of the two tolerances.
Observed on an MI355X (device - reference; values absolute / bounds of their term scale): X7 2.6e-15 / 6.7e-15 (tolerance
9.8e-14 / 1.0e-13), X8 1.3e-15 / 6.1e-16 (3.9e-14 / 1.7e-14), XT 0 / 0, XM 8.9e-16 / 5.3e-16 (2.8e-14 / 1.6e-14), XP 0 / 0; K7 with
its slanted capsule as a cuboid against the capsule reference 1.7e-15 / 5.5e-15 (1.0e-13 / 2.0e-13); the re-linearised QPs of
XT: device and oracle both infeasible after 150 (QPs 0, 1, 2) and 125 (QP 6) iterations, optimal after 50 (QP 5); the planners
on the device against the host callbacks (tests/test_gomp_cuboid_cpp.py): max |dx| 5.8e-15 (point robot past a box corner) and
2.9e-13 (7-joint arm into a bin).  Run with -s to see the figures."""
import ctypes as C

import numpy as np
import pytest

import capsule_refs as K
import cuboid_refs as X
import gomp_refs as G
import osqp_solver_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu
B = 8
IDS_A, IDS_B = [5, 2, 7, 0, 3], [6, 1, 4]          # permuted strict subsets of the batch
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _make(name, **kw):
    s, pr = X._scene(name), X.scene_batch(name)
    solver = _solver(pr, **kw)
    sc = X.CuboidScene(M.lib(), solver, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["con_lo"], s["con_hi"])
    assert sc.rc == 0, (sc.rc, M.lib().mi_osqp_last_error())
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
    tv, tb = X.gpu_tolerance(name)
    assert not ref["near"].any()
    ev = float(np.max(np.abs(vals - ref["vals"])))
    worst["values"] = max(worst.get("values", 0.0), ev)
    assert ev <= tv, (ev, tv)
    for side, dev in (("l", l[r0:r1]), ("u", u[r0:r1])):
        sc = ref[side + "_scale"]
        inf = sc == 0
        assert _same_bits(dev[inf], ref[side][inf])                           # an absent side, a dummy row, an inactive row: -+1e30 exactly
        fin = sc > 0
        eb = float(np.max(np.abs(dev[fin] - ref[side][fin]) / sc[fin], initial=0.0))
        worst["bounds"] = max(worst.get("bounds", 0.0), eb)
        assert eb <= tb, (side, eb, tb)
    if name in X.EXACT:                                                       # the exact cases: bit for bit
        assert np.array_equal(vals, ref["vals"]) and np.array_equal(l[r0:r1], ref["l"]) and np.array_equal(u[r0:r1], ref["u"])


def _check_verdicts(ok, refs):
    for j, r in enumerate(refs):
        assert ok[j] in (0, 1)
        assert not r["verdict_excluded"]
        assert bool(ok[j]) == r["ok"], j


def _rows_and_verdicts(name, sc, pr):
    s, ref = X.scene(name), X.scene_reference(name)
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
    tv, tb = X.gpu_tolerance(name)
    print(f"\nscene {name}: worst device - reference: values {worst['values']:.3e} (tolerance {tv:.3e}),"
          f" bounds {worst['bounds']:.3e} of their term scale (tolerance {tb:.3e})")


@pytest.mark.parametrize("name", X.SCENES)
def test_rows_and_verdicts_of_permuted_id_lists(handles, name):
    solver, sc, pr = handles(name)
    _rows_and_verdicts(name, sc, pr)


def test_the_exact_cases_of_scenes_XT_and_XP_on_the_device(handles):
    """What tests/test_cuboid_refs.py pins in the reference, read from the device's rows."""
    solver, sc, pr = handles("XT")
    s = X.scene("XT")
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
    assert rc == 0 and ok.tolist() == [0, 0, 0, 1, 1, 0, 0, 1]               # 4 | 5: the verdict flips
    W, nx = s["W"], 2
    T, o = s["trajs"], X.XT_O
    rA, r0, r1, h = X.XT_RA, X.XT_RB, X.XT_RB1, X.XT_H

    def row(sc_, pr_, b, ball, w, cub, W_=W, nx_=nx):
        A, l, u = sc_.get_rows(b)
        k = (ball * W_ + w) * nx_ + cub
        return A[pr_["aidx"][k]].tolist(), l[pr_["row0"] + k], u[pr_["row0"] + k]

    for w in range(6):                                                       # inside the cube, nearest to each face in turn
        n = [0.0, 0.0, 0.0]
        n[w // 2] = 1.0 - 2 * (w % 2)
        assert row(sc, pr, 0, 0, w, 0) == (n, (rA + r0) + 1 / 16 + n[w // 2] * T[0][3 * w + w // 2], G.INF)
    assert row(sc, pr, 1, 0, 1, 0) == ([1.0, 0.0, 0.0], (rA + r0) + h + o[0], G.INF)              # three-way tie at the cube's centre: k* = 0, +
    assert row(sc, pr, 1, 0, 1, 1) == ([-1.0, 0.0, 0.0], r0 + 1 / 64 - o[0], G.INF)               # the slab at c_2 = 0: +u_2 = -x
    assert row(sc, pr, 1, 0, 3, 0) == ([0.0, -1.0, 0.0], (rA + r0) + 1 / 8 - T[1][3 * 3 + 1], G.INF)      # two-way tie: the lower axis, signed by c_1
    assert row(sc, pr, 1, 0, 3, 1) == ([-1.0, 0.0, 0.0], r0 + 1 / 64 - o[0], G.INF)               # c_2 = -0.0: still +u_2
    assert row(sc, pr, 1, 1, 5, 0) == ([0.0, 1.0, 0.0], (rA + r1) + 1 / 8 + T[1][3 * 5 + 1], G.INF)
    assert row(sc, pr, 2, 0, 2, 0) == ([1.0, 0.0, 0.0], (rA + r0) + T[2][3 * 2], G.INF)           # on a face: sd = 0
    assert row(sc, pr, 2, 0, 4, 0) == ([0.0, 0.0, -1.0], (rA + r0) - T[2][3 * 4 + 2], G.INF)
    assert row(sc, pr, 2, 0, 6, 1) == ([1.0, 0.0, 0.0], r0 + T[2][3 * 6], G.INF)
    x1, x4 = T[3][3 * 1], T[3][3 * 4]
    assert row(sc, pr, 3, 0, 1, 0) == ([1.0, 0.0, 0.0], X.E20 - X.XT_MA + x1, G.INF)              # s = margin - 2^-20: active
    assert row(sc, pr, 3, 0, 4, 0) == ([-1.0, 0.0, 0.0], -G.INF, G.INF)                           # s = margin + 2^-20: not
    assert row(sc, pr, 6, 0, 1, 1) == ([1.0, 0.0, 0.0], X.E20 + T[6][3 * 1], G.INF)               # margin 0: s = -2^-20 | +2^-20
    assert row(sc, pr, 6, 0, 3, 1) == ([-1.0, 0.0, 0.0], -G.INF, G.INF)
    assert row(sc, pr, 7, 0, 5, 1)[0] == [0.0, 1.0, 0.0] and row(sc, pr, 7, 0, 6, 1)[0] == [0.0, 0.0, -1.0]       # u_0 = +y, u_1 = +z: not transposed
    solver, sc, pr = handles("XP")
    s = X.scene("XP")
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
    assert rc == 0 and ok.tolist() == [0, 1, 1, 0, 1, 1, 1, 1]
    assert row(sc, pr, 0, 0, 1, 0, 4, 1) == ([0.0, 1.0, 0.0], X.XP_R + X.XP_RB + o[1], G.INF)     # the point cuboid at out = 0: +u_0 = +y
    assert row(sc, pr, 1, 0, 1, 0, 4, 1)[1] == X.E20 - X.XP_M + s["trajs"][1][3 * 1] and row(sc, pr, 1, 0, 2, 0, 4, 1)[1] == -G.INF


def _drain(s, max_advances=400):
    for _ in range(max_advances):
        if not s.running():
            return
        s.advance(1)
        s.poll(True)
    raise AssertionError("continuous solve did not finish")


@pytest.mark.parametrize("name", ["XT", "X7"])
def test_relinearise_some_and_the_solves_that_follow(handles, name):
    solver, sc, pr = handles(name, scaling=0)
    s, ref = X.scene(name), X.scene_reference(name)
    ids = [5, 2, 7, 0, 3, 1, 4, 6]
    x = s["trajs"][ids]                                                      # QP b gets trajectory b, in the order of the list
    rejected = [b for b in range(B) if not ref[b]["ok"]]
    assert rejected == ([0, 1, 2, 5, 6] if name == "XT" else [0, 2, 4, 5, 7])
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
    if name != "XT":
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
    assert solved == 1                                                       # QP 5; the others are pinned inside a cuboid: infeasible


def test_no_cuboids_is_the_world_entry_point_bit_for_bit():
    """n_cuboids = 0 through mi_gomp_scene_create_cuboids against mi_gomp_scene_create_world on scene K7 of capsule_refs."""
    L = X.declare(M.lib())
    s, pr = K.scene("K7"), K.scene_batch("K7")
    got = {}
    for which in ("world", "cuboids"):
        h = _solver(pr)
        if which == "world":
            sc = K.WorldScene(L, h, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["con_lo"], s["con_hi"])
        else:
            sc = X.CuboidScene(L, h, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], [], s["con_lo"], s["con_hi"])
        assert sc.rc == 0 and sc.ptr
        assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
        rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
        assert rc == 0
        got[which] = (ok.tolist(), [sc.get_rows(b) for b in range(B)])
        sc.close()
        h.close()
    assert got["world"][0] == got["cuboids"][0] == [int(e["ok"]) for e in K.scene_reference("K7")]
    for a, b in zip(got["world"][1], got["cuboids"][1]):
        assert all(_same_bits(x, y) for x, y in zip(a, b))


def test_a_cuboid_with_two_zero_half_extents_is_the_capsule_on_the_device():
    """Scene K7 with its slanted capsule replaced by the equivalent cuboid: the same number of rows in the same places (the
    capsule was the last, the cuboid follows the capsules).  Rows within the sum of the two scenes' tolerances wherever
    out > NEAR, verdicts equal."""
    s, pr = K.scene("K7"), K.scene_batch("K7")
    ref = K.scene_reference("K7")
    xref = X.scene_reference("K7X")
    solver, sc, prx = _make("K7X")
    assert prx["rows3d"] == pr["rows3d"] and np.array_equal(prx["aidx"], pr["aidx"])
    assert sc.set_rows(range(B), prx["Ax"], prx["l"], prx["u"]) == 0
    rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
    assert rc == 0
    assert ok.tolist() == [int(e["ok"]) for e in ref]
    tv = K.gpu_tolerance("K7")[0] + X.gpu_tolerance("K7X")[0]
    tb = K.gpu_tolerance("K7")[1] + X.gpu_tolerance("K7X")[1]
    r0, r1 = pr["row0"], pr["row0"] + pr["rows3d"]
    worst_v = worst_b = 0.0
    for b in range(B):
        A, l, u = sc.get_rows(b)
        use = ~(xref[b]["out"] <= X.NEAR)                                    # (nan for the rows that are not the cuboid's: kept)
        ev = float(np.max(np.abs(A[pr["aidx"]] - ref[b]["vals"])[use]))
        eb = 0.0
        for side, dev in (("l", l[r0:r1]), ("u", u[r0:r1])):
            scale = ref[b][side + "_scale"]
            inf = (scale == 0) & use
            assert _same_bits(dev[inf], ref[b][side][inf])
            fin = (scale > 0) & use
            eb = max(eb, float(np.max(np.abs(dev - ref[b][side])[fin] / scale[fin], initial=0.0)))
        worst_v, worst_b = max(worst_v, ev), max(worst_b, eb)
        assert ev <= tv and eb <= tb, (b, ev, tv, eb, tb)
    print(f"\nscene K7, slanted capsule as a cuboid: worst device - capsule reference: values {worst_v:.3e} (tolerance {tv:.3e}), bounds {worst_b:.3e} ({tb:.3e})")
    sc.close()
    solver.close()


def test_refusals_leave_the_handle_usable():
    L = X.declare(M.lib())
    s, pr = X.scene("X8"), X.scene_batch("X8")
    h = _solver(pr)
    cubs = s["cuboids"]

    def refused(code, cuboids=cubs, why=None, capsules=(), **kw):
        rc, ptr = X.create_cuboids(L, h._h, 8, 2, s["chain"], s["balls"], s["lines"], list(capsules), cuboids, s["con_lo"], s["con_hi"], **kw)
        assert rc == code and not ptr, (rc, ptr, L.mi_osqp_last_error())
        if why:
            assert why in L.mi_osqp_last_error().decode(), L.mi_osqp_last_error()

    refused(NULL, null_cuboids=True, why="no cuboids")
    refused(INVALID, n_cuboids=-1, why="negative")
    refused(INVALID, [dict(cubs[0], radius=np.nan)], why="cuboid 0 has a field that is not finite")
    refused(INVALID, [dict(cubs[0], half=[0.1, -0.1, 0.1])], why="negative")
    refused(INVALID, [cubs[0], dict(cubs[0], axes=[1.0, 1e-6, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])], why="cuboid 1: the axes are not orthonormal")
    refused(INVALID, cubs + cubs, why="does not hold")                       # a row per (ball, waypoint) more than the matrix has
    refused(INVALID, cubs, why="does not hold", capsules=K.K8_CAPSULES)      # caps + cuboids beyond the matrix's rows
    info = h.solve()                                                         # after all that the handle solves ...
    assert len(info) == B and all(i.iter > 0 for i in info)
    sc = X.CuboidScene(L, h, 8, 2, s["chain"], s["balls"], s["lines"], [], cubs, s["con_lo"], s["con_hi"])
    assert sc.rc == 0 and sc.ptr                                             # ... and takes a scene, which works
    _rows_and_verdicts("X8", sc, pr)
    refused(INVALID, why="already has a scene")
    sc.close()
    sc = X.CuboidScene(L, h, 8, 2, s["chain"], s["balls"], s["lines"], [], cubs, s["con_lo"], s["con_hi"])         # a second scene after the first
    assert sc.rc == 0 and sc.ptr
    sc.close()
    sc = X.CuboidScene(L, h, 8, 2, None, [], [], [], cubs, None, None)       # chain == NULL: mi_gomp_scene_create's case
    assert sc.rc == 0 and sc.ptr
    sc.close()
    h.close()


def test_struct_size_and_symbol():
    assert C.sizeof(X.Cuboid) == 136
    assert hasattr(M.lib(), "mi_gomp_scene_create_cuboids")
