"""GPU (-m gpu): tilt limits (mi_gomp_tilt, the tilt items of gomp_relinearise_kernel) through mi_gomp_scene_create_tilts and
every call that launches the kernel, against the mpmath reference of tests/tilt_refs.py.

Scene T7 (the 7-joint chain of dh_refs, 40 waypoints, its 7 balls and 14 pairs, one tilt per frame 1 .. 7 = 280 tilt items: both
sides of the 256-thread stride and a last partial round, behind 560 pair rows; every frame value, so a wrong `on` select
shows), scene T8 (8 joints, 2 waypoints, one ball without rows, a tilt in frame 8 and one in frame 1: the smallest scene, the
last joint, a row with one column), scene TF (the flips: a 2-joint chain on which the tilt angle is |q_1|; activity at
max_angle - margin -+ 2^-20 for margin 1/8 and margin 0, the verdict at max_angle + 1e-3 -+ 2^-20), scenes TE and TEA (identity
rotations, dyadic or exactly dotted vectors, compared BIT FOR BIT: an active and an inactive row of one gradient, a frame-1
row, u = ref: a zero row, inactive; in TEA u = -ref besides: a zero row, active, 0 >= cos_lim + 1) and scene TM (two tilts behind
a gripper ball's work-space rows, two lines, a capsule, a cuboid and two pairs, once with the builder's over-allocated empty
rows behind them: the row order).  Rows within 32 x the fp64 error of the formulas themselves and never looser than 1e-13
(tilt_refs.gpu_tolerance; tests/test_tilt_refs.py holds the figures), no row of the committed trajectories within 1e-9 of a
threshold and no verdict excluded; joint-space entries, unlisted QPs and unpopulated rows bit for bit.  The re-linearised QPs of
TE and TEA are solved and compared with the oracle on the rows read back: those of TE are solved, those of TEA are primal
infeasible on both.
Observed on an MI355X (device - reference; values absolute / bounds of their term scale 1 + sum |g_j q_j|): T7 7.2e-16 / 2.2e-15
(tolerance 1.4e-14 / 3.2e-14), T8 2.2e-16 / 2.4e-16 (1.1e-14 / 6.5e-15), TF 1.1e-16 / 6.7e-17 (1.8e-15 / 2.3e-15), TE and TEA 0 / 0,
TM 8.9e-16 / 7.7e-16 (2.8e-14 / 1.7e-14), the same with over-allocated rows; the re-linearised QPs of TE: device and oracle both
solved after 50 iterations, those of TEA both primal infeasible after 50.  Run with -s to see the figures."""
import ctypes as C

import numpy as np
import pytest

import gomp_refs as G
import osqp_solver_amd as M
import pair_refs as P
import tilt_refs as T
from oracle import oracle as O

pytestmark = pytest.mark.gpu
B = 8
IDS_A, IDS_B = [5, 2, 7, 0, 3], [6, 1, 4]          # permuted strict subsets of the batch
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL
PRIMAL_INFEASIBLE = -3


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _scene(L, solver, s, tilts=None):
    return T.TiltScene(L, solver, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["pairs"],
                       s["tilts"] if tilts is None else tilts, s["con_lo"], s["con_hi"])


def _make(name, over=False, **kw):
    s, pr = T.scene(name), T.scene_batch(name, over)
    solver = _solver(pr, **kw)
    sc = _scene(M.lib(), solver, s)
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
    assert pr["rows3d"] == len(ref["l"])
    joint = np.ones(len(A), bool)
    joint[pr["aidx"].reshape(-1)] = False
    assert _same_bits(A[joint], A0[joint])                                    # joint-space entries
    assert _same_bits(l[:r0], l0[:r0]) and _same_bits(u[:r0], u0[:r0])
    assert _same_bits(l[r1:], l0[r1:]) and _same_bits(u[r1:], u0[r1:])        # unpopulated rows (behind the tilt rows)
    vals = A[pr["aidx"]]
    tv, tb = T.gpu_tolerance(name)
    assert not ref["near"].any()
    ev = float(np.max(np.abs(vals - ref["vals"])))
    worst["values"] = max(worst.get("values", 0.0), ev)
    print(f"  scene {name}: values {ev:.3e} (tolerance {tv:.3e})", end="")
    bounds = []
    for side, dev in (("l", l[r0:r1]), ("u", u[r0:r1])):
        sc = ref[side + "_scale"]
        inf = sc == 0
        assert _same_bits(dev[inf], ref[side][inf])                           # an absent side, a dummy row, an inactive row: -+1e30 exactly
        fin = sc > 0
        eb = float(np.max(np.abs(dev[fin] - ref[side][fin]) / sc[fin], initial=0.0))
        worst["bounds"] = max(worst.get("bounds", 0.0), eb)
        bounds.append((side, eb))
    print(f", bounds {max(e for _, e in bounds):.3e} of their term scale (tolerance {tb:.3e})")
    assert ev <= tv, (ev, tv)
    for side, eb in bounds:
        assert eb <= tb, (side, eb, tb)
    if name in T.EXACT:                                                       # the exact cases: bit for bit
        assert np.array_equal(vals, ref["vals"]) and np.array_equal(l[r0:r1], ref["l"]) and np.array_equal(u[r0:r1], ref["u"])


def _check_verdicts(ok, refs):
    for j, r in enumerate(refs):
        assert ok[j] in (0, 1)
        assert not r["verdict_excluded"]
        assert bool(ok[j]) == r["ok"], j


def _rows_and_verdicts(name, sc, pr):
    s, ref = T.scene(name), T.scene_reference(name)
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
    tv, tb = T.gpu_tolerance(name)
    print(f"\nscene {name}: worst device - reference: values {worst['values']:.3e} (tolerance {tv:.3e}),"
          f" bounds {worst['bounds']:.3e} of their term scale (tolerance {tb:.3e})")


@pytest.mark.parametrize("name,over", [("T7", False), ("T8", False), ("TF", False), ("TE", False), ("TEA", False), ("TM", False), ("TM", True)])
def test_rows_and_verdicts_of_permuted_id_lists(handles, name, over):
    solver, sc, pr = handles(name, over=over)
    if over:
        assert pr["m"] > pr["row0"] + pr["rows3d"]                            # empty rows behind the tilt rows
    _rows_and_verdicts(name, sc, pr)


def test_the_flips_of_scene_TF_on_the_device(handles):
    """What tests/test_tilt_refs.py pins in the reference, read from the device's rows: 2^-20 rad decide activity and verdict."""
    solver, sc, pr = handles("TF", over=False)
    s = T.scene("TF")
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
    assert rc == 0 and ok.tolist() == [1, 1, 0, 1, 0, 1, 0, 0]               # 3 | 4: the verdict flips
    W = s["W"]

    def active(b, tilt, w):
        _, l, u = sc.get_rows(b)
        k = pr["row0"] + pr["block_rows"] + tilt * W + w
        assert u[k] == G.INF
        return l[k] != -G.INF

    assert (active(0, 0, 1), active(0, 0, 2)) == (False, True) and (active(1, 0, 1), active(1, 0, 3)) == (False, True)      # margin 1/8
    assert (active(2, 1, 0), active(2, 1, 2)) == (False, True)                                                              # margin 0
    assert not any(active(b, 1, w) for b in (0, 1, 3, 4, 5) for w in range(W))


def test_the_exact_cases_of_scene_TEA_on_the_device(handles):
    solver, sc, pr = handles("TEA", over=False)
    s = T.scene("TEA")
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
    assert rc == 0 and ok.tolist() == [0] * B
    W, (q0, q1) = s["W"], T.TE_Q

    def row(b, tilt, w):
        A, l, u = sc.get_rows(b)
        k = pr["block_rows"] + tilt * W + w
        return A[pr["aidx"][k]].tolist(), l[pr["row0"] + k], u[pr["row0"] + k]

    for b in range(B):
        for w in range(W):
            assert row(b, 0, w) == ([0.8, 0.8, 0.0], (np.cos(0.875) - 0.6) + (0.8 * q0 + 0.8 * q1), G.INF)
            assert row(b, 1, w) == ([0.0, 0.0, 0.0], -G.INF, G.INF)                            # u = ref
            assert row(b, 2, w) == ([0.8, 0.8, 0.0], -G.INF, G.INF)                            # inactive, written all the same
            assert row(b, 3, w) == ([0.8, 0.0, 0.0], (np.cos(1.0) - 0.6) + 0.8 * q0, G.INF)    # frame 1
            assert row(b, 4, w) == ([0.0, 0.0, 0.0], np.cos(0.5) + 1.0, G.INF)                 # u = -ref: 0 >= cos_lim + 1


def _drain(s, max_advances=400):
    for _ in range(max_advances):
        if not s.running():
            return
        s.advance(1)
        s.poll(True)
    raise AssertionError("continuous solve did not finish")


@pytest.mark.parametrize("name", ["TE", "TEA", "T7"])
def test_relinearise_some_and_the_solves_that_follow(handles, name):
    solver, sc, pr = handles(name, over=False, scaling=0)
    s, ref = T.scene(name), T.scene_reference(name)
    ids = [5, 2, 7, 0, 3, 1, 4, 6]
    x = s["trajs"][ids]                                                      # QP b gets trajectory b, in the order of the list
    rejected = [b for b in range(B) if not ref[b]["ok"]]
    assert rejected == ([0, 1, 2, 3, 4, 6] if name == "T7" else list(range(B)))
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
    if name == "T7":
        return
    # ... and updated: solved from the device's rows, against the oracle fed with the rows read back
    for b in rejected:
        solver.warm_start_x_some([b], s["trajs"][b])
    solver.solve_begin_some(rejected)
    _drain(solver)
    infos, xs = solver.info_some(rejected), solver.primal_some(rejected)
    for k, b in enumerate(rejected):
        Ax, l, u = rows[b]
        A = pr["A"].copy()
        A.data = Ax
        o = O.OracleQPSolver(pr["P"], None, pr["A"], pr["l"][b], pr["u"][b], scaling=0)
        o.update(l, A, u)
        o.set_warm_start(s["trajs"][b])
        st, xo = o.solve()
        print(f"\nscene {name}, QP {b}: device status {infos[k].status_val} after {infos[k].iter} iterations, oracle {st} after {o.info().iter}")
        assert (infos[k].status_val, infos[k].iter) == (st, o.info().iter), b
        if name == "TEA":
            assert st == PRIMAL_INFEASIBLE                                   # the antiparallel tilt: 0 >= cos_lim + 1
        else:
            assert st == 1 and np.max(np.abs(xs[k] - xo)) <= 1e-6


def test_no_tilts_is_the_pair_entry_point_bit_for_bit():
    """n_tilts = 0 through mi_gomp_scene_create_tilts against mi_gomp_scene_create_pairs on scene P7 of pair_refs."""
    L = T.declare(M.lib())
    s, pr = P.scene("P7"), P.scene_batch("P7")
    got = {}
    for which in ("pairs", "tilts"):
        h = _solver(pr)
        if which == "pairs":
            sc = P.PairScene(L, h, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["pairs"], s["con_lo"], s["con_hi"])
        else:
            sc = _scene(L, h, s, tilts=[])
        assert sc.rc == 0 and sc.ptr
        assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
        rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
        assert rc == 0
        got[which] = (ok.tolist(), [sc.get_rows(b) for b in range(B)])
        sc.close()
        h.close()
    assert got["pairs"][0] == got["tilts"][0] == [int(e["ok"]) for e in P.scene_reference("P7")]
    for a, b in zip(got["pairs"][1], got["tilts"][1]):
        assert all(_same_bits(x, y) for x, y in zip(a, b))


def test_refusals_leave_the_handle_usable():
    L = T.declare(M.lib())
    s, pr = T.scene("T8"), T.scene_batch("T8")
    h = _solver(pr)
    tls = s["tilts"]
    ok = tls[0]

    def refused(code, tilts=tls, why=None, chain=s["chain"], **kw):
        rc, ptr = T.create_tilts(L, h._h, 8, 2, chain, s["balls"] if chain else [], [], [], [], [], tilts, None, None, **kw)
        assert rc == code and not ptr, (rc, ptr, L.mi_osqp_last_error())
        if why:
            assert why in L.mi_osqp_last_error().decode(), L.mi_osqp_last_error()

    refused(NULL, null_tilts=True, why="no tilts")
    refused(NULL, chain=None, why="tilt 0")
    refused(INVALID, n_tilts=-1, why="negative")
    refused(INVALID, [ok, dict(ok, frame=0)], why="tilt 1: frame")
    refused(INVALID, [dict(ok, frame=9)], why="tilt 0: frame")
    refused(INVALID, [ok, dict(ok, max_angle=np.nan)], why="tilt 1 has a field that is not finite")
    refused(INVALID, [dict(ok, axis=[0.0, np.inf, 0.0])], why="tilt 0 has a field that is not finite")
    refused(INVALID, [dict(ok, axis=[0.0, 0.0, 1.0 + 1e-8])], why="tilt 0: axis")
    refused(INVALID, [ok, dict(ok, ref=[0.0, 0.0, 0.0])], why="tilt 1: ref")
    for bad in (0.0, -0.5, np.pi, 4.0):
        refused(INVALID, [dict(ok, max_angle=bad)], why="tilt 0: max_angle")
    refused(INVALID, [dict(ok, margin=-1e-3)], why="tilt 0: the margin")
    refused(INVALID, tls + tls[:1], why="does not hold")                      # W rows more than the matrix has
    assert "tilt 2" in L.mi_osqp_last_error().decode()
    info = h.solve()                                                         # after all that the handle solves ...
    assert len(info) == B and all(i.iter > 0 for i in info)
    sc = _scene(L, h, s)
    assert sc.rc == 0 and sc.ptr                                             # ... and takes a scene, which works
    _rows_and_verdicts("T8", sc, pr)
    refused(INVALID, why="already has a scene")
    sc.close()
    sc = _scene(L, h, s)                                                     # a second scene after the first
    assert sc.rc == 0 and sc.ptr
    sc.close()
    h.close()


def test_struct_size_and_symbol():
    assert C.sizeof(T.Tilt) == 72
    assert hasattr(M.lib(), "mi_gomp_scene_create_tilts")
