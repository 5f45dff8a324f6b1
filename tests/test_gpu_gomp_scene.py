"""GPU (-m gpu): gomp_relinearise_kernel and the mi_gomp_* entry points against the plain reference of tests/gomp_refs.py.

The kernel's only other GPU test (`devasm` of tests/cpp/gomp_parity.cpp) compares it with the project's own host twin at
shapes of one pass, identity id lists and one ball order.  Here every scene has more (ball, waypoint) pairs than the
workgroup has threads (scene T also exactly as many, and two waypoints), the id lists are permuted strict subsets of the
batch with distinct trajectories, the balls mix gripper and non-gripper in every order with up to two lines, one of them
bypassed from below, the box has absent sides (given as +-1e30 and as NULL), and the trajectories are placed so that every
collision class and every rejection cause occurs - tests/test_gomp_refs.py counts them on the CPU.

Scene T (TABLE kinematics, every number a dyadic rational) is compared bit for bit; scenes U (UR5e) and Y (yaw + 2 links)
within 32 x the fp64 error of the reference's own formulas (gomp_refs.gpu_tolerance: about 1e-14 absolute for a matrix
value, about 1e-14 x the sum of the absolute values of its terms for a bound), leaving out the l and u of a row, and a
verdict, that hang on a decision within 1e-9 of its threshold in the reference (none in the committed trajectories).
Observed on an MI355X: scene U values 2.2e-16 / bounds 3.2e-16 of their term scale, scene Y 2.2e-16 / 2.1e-16, A x of
the re-linearised QPs within 2.6e-16 ||row||_1 ||x||_inf of the reference's.  Run with -s to see the figures."""
import ctypes as C

import numpy as np
import pytest

import gomp_refs as G
import osqp_solver_amd as M
from op_refs import Coo
from oracle import oracle as O

pytestmark = pytest.mark.gpu
B = 8
IDS_A, IDS_B = [5, 2, 7, 0, 3], [6, 1, 4]          # permuted strict subsets of the batch
CASES = [("T86", False), ("T64", False), ("T2", False), ("U", False), ("Y", False), ("Y", True)]
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


@pytest.fixture(scope="module")
def handles():
    """One handle and scene per (scene, over-allocated, settings), made on first use and kept for the module."""
    made = {}

    def get(name, over=False, **kw):
        key = (name, over, tuple(sorted(kw.items())))
        if key not in made:
            s, pr = G.scene(name), G.scene_batch(name, over)
            solver = _solver(pr, **kw)
            sc = G.GompScene(M.lib(), solver, s["D"], s["W"], s["balls"], s["lines"], s["con_lo"], s["con_hi"])
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
    3-D rows, against what set_rows wrote (`pr` rows of that QP, passed in got[3:])."""
    A, l, u, A0, l0, u0 = got
    r0, r1 = pr["row0"], pr["row0"] + pr["rows3d"]
    joint = np.ones(len(A), bool)
    joint[pr["aidx"].reshape(-1)] = False
    assert _same_bits(A[joint], A0[joint])                                    # joint-space entries
    assert _same_bits(l[:r0], l0[:r0]) and _same_bits(u[:r0], u0[:r0])
    assert _same_bits(l[r1:], l0[r1:]) and _same_bits(u[r1:], u0[r1:])        # unpopulated rows
    vals = A[pr["aidx"]]
    if name[0] == "T":
        assert _same_bits(vals, ref["vals"]) and _same_bits(l[r0:r1], ref["l"]) and _same_bits(u[r0:r1], ref["u"])
        return
    tv, tb = G.gpu_tolerance(name)
    ev = np.max(np.abs(vals - ref["vals"]))
    worst["values"] = max(worst.get("values", 0.0), float(ev))
    assert ev <= tv, (ev, tv)
    use = ~ref["near"]
    for side, dev in (("l", l[r0:r1]), ("u", u[r0:r1])):
        sc = ref[side + "_scale"]
        inf = use & (sc == 0)
        assert _same_bits(dev[inf], ref[side][inf])                           # an absent side, a dummy row: -+1e30 exactly
        fin = use & (sc > 0)
        eb = np.max(np.abs(dev[fin] - ref[side][fin]) / sc[fin], initial=0.0)
        worst["bounds"] = max(worst.get("bounds", 0.0), float(eb))
        assert eb <= tb, (side, eb, tb)


def _check_verdicts(ok, refs):
    for j, r in enumerate(refs):
        assert ok[j] in (0, 1)
        if not r["verdict_excluded"]:
            assert bool(ok[j]) == r["ok"], j


@pytest.mark.parametrize("name,over", CASES)
def test_rows_and_verdicts_of_permuted_id_lists(handles, name, over):
    solver, sc, pr = handles(name, over)
    s, ref = G.scene(name), G.scene_reference(name)
    worst = {}
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    before = [sc.get_rows(b) for b in range(B)]
    for b in range(B):
        assert all(_same_bits(x, y) for x, y in zip(before[b], (pr["Ax"][b], pr["l"][b], pr["u"][b])))
    rc, ok = sc.assemble_some(IDS_A, s["trajs"][:5])                         # trajectory j goes to QP IDS_A[j]
    assert rc == 0, M.lib().mi_osqp_last_error()                             # (the handle is LDS-resident: the continuous mode takes it)
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
    if worst:
        tv, tb = G.gpu_tolerance(name)
        print(f"\nscene {name}{' (over-allocated)' if over else ''}: worst device - reference: values {worst['values']:.3e} (tolerance {tv:.3e}),"
              f" bounds {worst['bounds']:.3e} of their term scale (tolerance {tb:.3e})")


def _drain(s, max_advances=400):
    for _ in range(max_advances):
        if not s.running():
            return
        s.advance(1)
        s.poll(True)
    raise AssertionError("continuous solve did not finish")


@pytest.mark.parametrize("name", ["T86", "U", "Y"])
def test_relinearise_some_rewrites_and_updates_the_rejected_qps_only(handles, name):
    import torch
    solver, sc, pr = handles(name, False, scaling=0)
    _, sc2, _ = handles(name, False)
    s, ref = G.scene(name), G.scene_reference(name)
    n, m = pr["n"], pr["m"]
    ids = IDS_A
    x = s["trajs"][ids]                                                      # QP b gets trajectory b, in the order of the list
    want = [ref[b]["ok"] for b in ids]
    assert any(want) and not all(want)                                       # accepted and rejected trajectories in one call
    for k in (sc, sc2):
        assert k.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    rng = np.random.default_rng(11)
    xv = rng.standard_normal((B, n))
    tx = torch.tensor(xv, device="cuda")
    Ax_old = torch.empty(B, m, dtype=torch.float64, device="cuda")
    Ax_new = torch.empty_like(Ax_old)
    solver.spmv_device(tx, None, None, None, Ax_old)
    rc, ok = sc.relinearise_some(ids, x)
    assert rc == 0, M.lib().mi_osqp_last_error()
    _check_verdicts(ok, [ref[b] for b in ids])
    rc, ok2 = sc2.assemble_some(ids, x)
    assert rc == 0 and np.array_equal(ok, ok2)
    solver.spmv_device(tx, None, None, None, Ax_new)
    Ax_old, Ax_new = Ax_old.cpu().numpy(), Ax_new.cpu().numpy()
    worst = 0.0
    for b in range(B):
        got = sc.get_rows(b)
        rejected = b in ids and not ok[ids.index(b)]
        if rejected:
            assert all(_same_bits(p, q) for p, q in zip(got, sc2.get_rows(b)))                     # the kept rows: those of assemble_some
            Aref = pr["A"].copy()
            Aref.data = G.reference_rows(pr, b, ref[b])[0]
            val, _, _ = Coo.from_scipy(Aref).matvec(xv[b])
            norm1 = np.asarray(abs(Aref).sum(axis=1)).reshape(-1)
            err = np.abs(Ax_new[b] - val.astype(np.float64))
            bound = 1e-13 * norm1 * np.max(np.abs(xv[b]))
            assert np.all(err <= bound), (b, float(np.max(err - bound)))
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))) * 1e-13)
            assert not _same_bits(Ax_new[b], Ax_old[b])
        else:
            assert all(_same_bits(p, q) for p, q in zip(got, (pr["Ax"][b], pr["l"][b], pr["u"][b])))  # accepted or not listed: as set_rows wrote
            assert _same_bits(Ax_new[b], Ax_old[b])                                                # and the solver keeps its matrix
    print(f"\nscene {name}: A x of the re-linearised QPs against the reference: worst {worst:.3e} of ||row||_1 ||x||_inf (bound 1e-13)")
    if name != "T86":
        return
    # one rejected QP solved from the rows the device wrote, against the oracle on the reference's rows
    b = G.SOLVED_QP
    assert b in ids and not ok[ids.index(b)]
    solver.warm_start_x_some([b], s["trajs"][b])
    solver.solve_begin_some([b])
    _drain(solver)
    info, xd = solver.info_some([b])[0], solver.primal_some([b])[0]
    Ax, l, u = G.reference_rows(pr, b, ref[b])
    A = pr["A"].copy()
    A.data = Ax
    o = O.OracleQPSolver(pr["P"], None, pr["A"], pr["l"][b], pr["u"][b], scaling=0)
    o.update(l, A, u)
    o.set_warm_start(s["trajs"][b])
    st, xo = o.solve()
    assert st == 1 and (info.status_val, info.iter) == (st, o.info().iter)
    assert np.max(np.abs(xd - xo)) <= 1e-6


def test_reinit_and_update_keep_the_raw_rows_in_the_scene(handles):
    solver, sc, pr = handles("T2", False)                                    # a scaled handle: the copy is the caller's raw data
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    rng = np.random.default_rng(3)
    kept = [sc.get_rows(b) for b in range(B)]
    for call, ids in ((solver.reinit_some, [6, 1, 4]), (solver.update_A_bounds_some, [3, 6])):
        Ax = pr["Ax"][ids] * (1.0 + 0.25 * rng.random((len(ids), pr["Ax"].shape[1])))
        l = np.where(pr["l"][ids] > -1e29, pr["l"][ids] - rng.random((len(ids), pr["m"])), pr["l"][ids])
        u = np.where(pr["u"][ids] < 1e29, pr["u"][ids] + rng.random((len(ids), pr["m"])), pr["u"][ids])
        call(ids, Ax, l, u)
        for b in range(B):
            got = sc.get_rows(b)
            if b in ids:
                j = ids.index(b)
                assert _same_bits(got[0], Ax[j]) and _same_bits(got[1], l[j]) and _same_bits(got[2], u[j])
                kept[b] = got
            else:
                assert all(_same_bits(p, q) for p, q in zip(got, kept[b]))


def test_refusals_are_host_side_and_leave_the_handle_usable():
    L = G.declare(M.lib())
    s = G.scene("T2")
    balls, lines = s["balls"], s["lines"]
    ur = [dict(model=G.FLANGE, gripper=True, radius=0.05, param=[0.0] * 12)]
    pr3 = G.scene_problem(3, 2, balls, 2, B, True, starts=s["trajs"][:, :3])           # over-allocated: room for a fourth ball's rows, no entries
    pr6 = G.scene_problem(6, 2, ur, 0, 2, False)
    h3, h6 = _solver(pr3), _solver(pr6)

    def refused(solver, D, W, bl, ln, lo=None, hi=None, codes=(INVALID,)):
        sc = G.GompScene(L, solver, D, W, bl, ln, lo, hi)
        assert sc.rc in codes and not sc.ptr, (sc.rc, sc.ptr)

    refused(h3, 3, 2, ur, lines)                                             # a UR5e ball with D = 3
    refused(h6, 6, 2, [balls[0]], [])                                        # a TABLE ball with D = 6
    refused(h3, 3, 3, balls, lines)                                          # n != 2 D W
    refused(h6, 3, 4, [balls[0]], [])                                        # (n = 2 D W, but the rows of D = 6, W = 2 are not those of D = 3, W = 4)
    refused(h3, 3, 2, balls + [balls[1]], lines)                             # the pattern lacks the 3-D rows of a fourth ball
    refused(h3, 3, 2, balls, [lines[0], dict(dir=[0.0, 0.0], point=[0.0, 0.0, 0.0], below=False)])   # a zero line direction
    for model in (0, 6):
        refused(h3, 3, 2, [dict(balls[0], model=model)] + balls[1:], lines)
    out = C.c_void_p()
    assert L.mi_gomp_scene_create(None, h3._h, 3, 2, len(balls), G.c_balls(balls), 2, G.c_lines(lines), None, None) == NULL
    assert L.mi_gomp_scene_create(C.byref(out), h3._h, 3, 2, len(balls), None, 2, G.c_lines(lines), None, None) == NULL and not out
    assert L.mi_gomp_scene_create(C.byref(out), None, 3, 2, len(balls), G.c_balls(balls), 2, G.c_lines(lines), None, None) == NULL and not out
    # after all that the handle takes a scene, and a second one is refused
    sc = G.GompScene(L, h3, 3, 2, balls, lines, s["con_lo"], s["con_hi"])
    assert sc.rc == 0 and sc.ptr
    refused(h3, 3, 2, balls, lines, s["con_lo"], s["con_hi"])
    assert sc.set_rows(range(B), pr3["Ax"], pr3["l"], pr3["u"]) == 0
    ref = G.scene_reference("T2")
    for bad in ([0, B], [-1], list(range(B)) + [0]):                         # an id out of range, more ids than QPs
        rc, ok = sc.relinearise_some(bad, s["trajs"][:1].repeat(len(bad), axis=0))
        assert rc == INVALID and np.all(ok == -1)
    rc, ok = sc.assemble_some([0, B], s["trajs"][:2])
    assert rc == INVALID
    h3.solve_begin_some([1])                                                 # QP 1 is running: not re-linearised
    rc, ok = sc.relinearise_some([2, 1], s["trajs"][[2, 1]])
    assert rc == INVALID and np.all(ok == -1)
    _drain(h3)
    before = [sc.get_rows(b) for b in range(B)]
    for b in range(B):
        assert all(_same_bits(p, q) for p, q in zip(before[b], (pr3["Ax"][b], pr3["l"][b], pr3["u"][b])))     # no refused call wrote a row
    rc, ok = sc.relinearise_some([3, 1], s["trajs"][[3, 1]])                 # and the handle and its scene still work
    assert rc == 0
    _check_verdicts(ok, [ref[3], ref[1]])
    assert not ref[3]["ok"] and ref[1]["ok"]
    sc.close()
    sc = G.GompScene(L, h3, 3, 2, balls, lines, None, None)                  # a freed scene makes room for the next; no box at all
    assert sc.rc == 0 and sc.ptr
    sc.close()
    h3.close()
    h6.close()
