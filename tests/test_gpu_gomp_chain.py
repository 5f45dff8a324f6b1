"""GPU (-m gpu): the DH-chain ball model (MI_GOMP_MODEL_DH_CHAIN, dh_point in gomp_relinearise_kernel) through
mi_gomp_scene_create_chain and every call that launches the kernel, against the mpmath reference of tests/dh_refs.py.

Scene C7 (7 joints, 40 waypoints, 7 balls = 280 (ball, waypoint) pairs: both sides of the 256-thread stride; its first ball sits
on a joint axis and has an all-zero Jacobian), scene C8 (8 joints, the largest `dims`, with 2 waypoints, the smallest), scene UC
(scene U of gomp_refs, its UR5e balls given as chain balls) and scene M3 (a chain ball beside a TABLE ball).  Rows within
32 x the fp64 error of the formulas themselves (dh_refs.gpu_tolerance, about 1e-14; tests/test_dh_refs.py holds the figures),
rows with a decision within 1e-9 of its threshold left out (none in the committed trajectories); joint-space entries and
unpopulated rows bit for bit.  The re-linearised QPs of C7 are solved and compared with the oracle on the rows read back.
Observed on an MI355X: C7 values 3.3e-16 / bounds 4.7e-16 of their term scale, C8 2.2e-16 / 2.4e-16, UC 2.2e-16 / 3.2e-16,
M3 2.2e-16 / 2.1e-16; the planner on the device against the host callbacks: max |dx| 2.4e-14.  Run with -s to see the figures."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dh_refs as DH
import gomp_refs as G
import osqp_solver_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 8
IDS_A, IDS_B = [5, 2, 7, 0, 3], [6, 1, 4]          # permuted strict subsets of the batch
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


@pytest.fixture(scope="module")
def handles():
    """One handle and chain scene per (scene, settings), made on first use and kept for the module."""
    made = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in made:
            s, pr = DH.scene(name), DH.scene_batch(name)
            solver = _solver(pr, **kw)
            sc = DH.ChainScene(M.lib(), solver, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["con_lo"], s["con_hi"])
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
    tv, tb = DH.gpu_tolerance(name)
    ev = float(np.max(np.abs(vals - ref["vals"])))
    worst["values"] = max(worst.get("values", 0.0), ev)
    assert ev <= tv, (ev, tv)
    use = ~ref["near"]
    for side, dev in (("l", l[r0:r1]), ("u", u[r0:r1])):
        sc = ref[side + "_scale"]
        inf = use & (sc == 0)
        assert _same_bits(dev[inf], ref[side][inf])                           # an absent side, a dummy row: -+1e30 exactly
        fin = use & (sc > 0)
        eb = float(np.max(np.abs(dev[fin] - ref[side][fin]) / sc[fin], initial=0.0))
        worst["bounds"] = max(worst.get("bounds", 0.0), eb)
        assert eb <= tb, (side, eb, tb)


def _check_verdicts(ok, refs):
    for j, r in enumerate(refs):
        assert ok[j] in (0, 1)
        if not r["verdict_excluded"]:
            assert bool(ok[j]) == r["ok"], j


def _rows_and_verdicts(name, sc, pr):
    s, ref = DH.scene(name), DH.scene_reference(name)
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
    tv, tb = DH.gpu_tolerance(name)
    print(f"\nscene {name}: worst device - reference: values {worst['values']:.3e} (tolerance {tv:.3e}),"
          f" bounds {worst['bounds']:.3e} of their term scale (tolerance {tb:.3e})")


@pytest.mark.parametrize("name", ["C7", "C8", "UC"])
def test_rows_and_verdicts_of_permuted_id_lists(handles, name):
    solver, sc, pr = handles(name)
    _rows_and_verdicts(name, sc, pr)
    if name == "C7":                                                         # the ball on the joint axis: zero rows, written as zeros
        A = sc.get_rows(IDS_A[0])[0]
        assert np.all(A[pr["aidx"][:DH.scene(name)["W"] * 2]] == 0.0)


def _drain(s, max_advances=400):
    for _ in range(max_advances):
        if not s.running():
            return
        s.advance(1)
        s.poll(True)
    raise AssertionError("continuous solve did not finish")


def test_relinearise_some_on_scene_C7_and_the_solves_that_follow(handles):
    name = "C7"
    solver, sc, pr = handles(name, scaling=0)
    s, ref = DH.scene(name), DH.scene_reference(name)
    ids = [5, 2, 7, 0, 3, 1, 4, 6]
    x = s["trajs"][ids]                                                      # QP b gets trajectory b, in the order of the list
    rejected = [b for b in range(B) if not ref[b]["ok"]]
    assert rejected == [0, 1, 2, 4, 7] and not any(ref[b]["verdict_excluded"] for b in range(B))
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
    assert solved == 2


def test_a_chain_ball_beside_a_table_ball(handles):
    L = DH.declare(M.lib())
    s7, table = DH.scene("C7"), G._ball(G.TABLE, 0, 1 / 8, G.T_TABLES[1])
    h7 = _solver(DH.scene_batch("C7"))                                       # D = 7: a TABLE ball has no place, whatever the chain
    mixed = s7["balls"][:5] + [table] + s7["balls"][6:]                      # (in the place of a ball of its kind: the same rows)
    rc, ptr = DH.create_chain(L, h7._h, 7, 40, s7["chain"], mixed, s7["lines"], s7["con_lo"], s7["con_hi"])
    assert rc == INVALID and not ptr
    rc, ptr = DH.create_chain(L, h7._h, 7, 40, s7["chain"], s7["balls"], s7["lines"], s7["con_lo"], s7["con_hi"])
    assert rc == 0 and ptr                                                   # the handle had nothing against a scene
    L.mi_gomp_scene_free(ptr)
    h7.close()
    solver, sc, pr = handles("M3")                                           # D = 3: accepted, rows of both correct
    _rows_and_verdicts("M3", sc, pr)


def test_refusals_leave_the_handle_usable(handles):
    L = DH.declare(M.lib())
    s = DH.scene("C8")
    pr = DH.scene_batch("C8")
    h = _solver(pr)
    balls, lines = s["balls"], s["lines"]

    def refused(code, ch, bl=balls, D=8, W=2):
        rc, ptr = DH.create_chain(L, h._h, D, W, ch, bl, lines, s["con_lo"], s["con_hi"])
        assert rc == code and not ptr, (rc, ptr, L.mi_osqp_last_error())

    refused(NULL, None)
    refused(INVALID, DH.C7)                                                  # n_joints = 7 on a handle of D = 8
    refused(INVALID, DH.c_chain(DH.C8, 9))
    bad = {k: list(v) for k, v in DH.C8.items()}
    bad["alpha"][3] = np.nan
    refused(INVALID, bad)
    refused(INVALID, DH.C8, [balls[0], dict(balls[1], param=[8.5] + balls[1]["param"][1:])])
    refused(INVALID, DH.C8, [balls[0], dict(balls[1], param=[9.0] + balls[1]["param"][1:])])
    refused(INVALID, DH.C8, [balls[0], dict(balls[1], param=[8.0, np.inf] + balls[1]["param"][2:])])
    refused(INVALID, DH.C8, W=3)                                             # n != 2 D W: the handle's own refusal, as before
    old = G.GompScene(L, h, 8, 2, balls, lines, s["con_lo"], s["con_hi"])   # model 6 through mi_gomp_scene_create: refused as ever
    assert old.rc == INVALID and not old.ptr
    sc = DH.ChainScene(L, h, 8, 2, DH.C8, balls, lines, s["con_lo"], s["con_hi"])
    assert sc.rc == 0 and sc.ptr                                             # after all that the handle takes a scene and it works
    _rows_and_verdicts("C8", sc, pr)
    refused(INVALID, DH.C8)                                                  # a second scene on the handle
    sc.close()
    sc = DH.ChainScene(L, h, 8, 2, None, [], lines, None, None)              # no chain, no chain ball: mi_gomp_scene_create's case
    assert sc.rc == 0 and sc.ptr
    sc.close()
    h.close()


# ------------------------------------------------------------------ the planner and the example

def _gxx(src, out, oracle):
    libdir, ordir = os.path.join(ROOT, "osqp-solver_amd"), os.path.join(ROOT, "oracle", "_build")
    cmd = ["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), src, "-o", str(out), "-L" + libdir, "-lmi_osqp", "-pthread", "-Wl,-rpath," + libdir]
    if oracle:
        cmd += ["-L" + ordir, "-loracle_osqp", "-fopenmp", "-Wl,-rpath," + ordir]
    subprocess.run(cmd, check=True)
    return str(out)


def test_continuous_planner_on_the_7_joint_chain(tmp_path):
    """ContinuousGOMPSolver<7> on chain c7 with C7's balls, line 0 and box: the SQP step on the device against the host
    callbacks - same exit codes and counters, trajectories within 1e-6, a repeated run bitwise equal, re-linearisations > 0."""
    M.lib(); O.lib()
    exe = _gxx(os.path.join(ROOT, "tests", "cpp", "gomp_chain.cpp"), tmp_path / "gomp_chain", True)
    r = subprocess.run([exe, "cont"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CONT OK" in r.stdout and "Memory access fault" not in r.stdout + r.stderr, r.stdout + r.stderr
    print("\n" + r.stdout)


def test_chain_gomp_example_plans_every_trajectory(tmp_path):
    M.lib()
    exe = _gxx(os.path.join(ROOT, "examples", "chain_gomp_example.cpp"), tmp_path / "chain_gomp_example", False)
    r = subprocess.run([exe, "8", "40", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "8 of 8 trajectories planned" in r.stdout and "Memory access fault" not in r.stdout + r.stderr, r.stdout + r.stderr
    assert "SQP step on the device" in r.stdout
