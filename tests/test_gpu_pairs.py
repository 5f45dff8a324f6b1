"""GPU (-m gpu): self-collision pairs (mi_gomp_pair, the pair items of gomp_relinearise_kernel) through
mi_gomp_scene_create_pairs and every call that launches the kernel, against the mpmath reference of tests/pair_refs.py.

Scene P7 (the 7-joint chain of dh_refs, 40 waypoints, 7 balls = 280 ball items and the 14 pairs of dhSelfPairs = 560 pair items:
both sides of the 256-thread stride and a last partial round; a line and a capsule), scene P8 (8 joints, 2 waypoints, two balls,
one pair, nothing else: the smallest scene), scene PT (TABLE balls and fixed balls on the z axis, every row exact in fp64,
compared BIT FOR BIT: the activity flips at s = margin -+ 2^-20 for margin 1/8 and margin 0, the verdict flips at
s = -1e-3 -+ 2^-20, a pair listed as (a, b) and as (b, a), coincident centres with reach 0 and with reach > 0) and scene PM (two
pairs behind a gripper ball's work-space rows, two lines, a capsule and a cuboid, once with the builder's over-allocated empty
rows behind them: the row order).  Rows within 32 x the fp64 error of the formulas themselves and never looser than 1e-13
(pair_refs.gpu_tolerance; tests/test_pair_refs.py holds the figures), no row of the committed trajectories within 1e-9 of a
threshold and no verdict excluded; joint-space entries, unlisted QPs and unpopulated rows bit for bit.  The re-linearised QPs of
PT are solved and compared with the oracle on the rows read back.
Observed on an MI355X (device - reference; values absolute / bounds of their term scale): P7 7.2e-16 / 2.2e-15 (tolerance
1.2e-14 / 3.2e-14), P8 2.2e-16 / 1.4e-16 (8.9e-15 / 4.6e-15), PT 0 / 0, PM 8.9e-16 / 7.7e-16 (2.8e-14 / 1.7e-14), the same with
over-allocated rows; the re-linearised QPs of PT: device and oracle both infeasible after 75 (QP 3) and 125 (QP 5) iterations;
the planner on the device against the host callbacks on the folding problem (tests/test_gomp_pairs_cpp.py): max |dx| 3.9e-14,
minimum pair clearance +0.6 mm with pairs, -13 cm without.  Run with -s to see the figures."""
import ctypes as C

import numpy as np
import pytest

import cuboid_refs as X
import gomp_refs as G
import osqp_solver_amd as M
import pair_refs as P
from oracle import oracle as O

pytestmark = pytest.mark.gpu
B = 8
IDS_A, IDS_B = [5, 2, 7, 0, 3], [6, 1, 4]          # permuted strict subsets of the batch
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _make(name, over=False, **kw):
    s, pr = P.scene(name), P.scene_batch(name, over)
    solver = _solver(pr, **kw)
    sc = P.PairScene(M.lib(), solver, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["pairs"], s["con_lo"], s["con_hi"])
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
    assert _same_bits(l[r1:], l0[r1:]) and _same_bits(u[r1:], u0[r1:])        # unpopulated rows (behind the pair rows)
    vals = A[pr["aidx"]]
    tv, tb = P.gpu_tolerance(name)
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
    if name in P.EXACT:                                                       # the exact cases: bit for bit
        assert np.array_equal(vals, ref["vals"]) and np.array_equal(l[r0:r1], ref["l"]) and np.array_equal(u[r0:r1], ref["u"])


def _check_verdicts(ok, refs):
    for j, r in enumerate(refs):
        assert ok[j] in (0, 1)
        assert not r["verdict_excluded"]
        assert bool(ok[j]) == r["ok"], j


def _rows_and_verdicts(name, sc, pr):
    s, ref = P.scene(name), P.scene_reference(name)
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
    tv, tb = P.gpu_tolerance(name)
    print(f"\nscene {name}: worst device - reference: values {worst['values']:.3e} (tolerance {tv:.3e}),"
          f" bounds {worst['bounds']:.3e} of their term scale (tolerance {tb:.3e})")


@pytest.mark.parametrize("name,over", [("P7", False), ("P8", False), ("PT", False), ("PM", False), ("PM", True)])
def test_rows_and_verdicts_of_permuted_id_lists(handles, name, over):
    solver, sc, pr = handles(name, over=over)
    if over:
        assert pr["m"] > pr["row0"] + pr["rows3d"]                            # empty rows behind the pair rows
    _rows_and_verdicts(name, sc, pr)


def test_the_exact_cases_of_scene_PT_on_the_device(handles):
    """What tests/test_pair_refs.py pins in the reference, read from the device's rows."""
    solver, sc, pr = handles("PT", over=False)
    s = P.scene("PT")
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
    assert rc == 0 and ok.tolist() == [1, 1, 1, 0, 1, 0, 1, 1]               # 2 | 3: the verdict flips
    W, T = s["W"], s["trajs"]
    tz = [[float(v) for v in G.T_TABLES[k][6:9]] for k in range(3)]
    neg = lambda v: [-x for x in v]
    r03, r05, ma = P.PT_REACH0, P.PT_REACH2, P.PT_MA
    z = lambda b, w: T[b][3 * w + 2]

    def row(b, pair, w):
        A, l, u = sc.get_rows(b)
        k = pr["block_rows"] + pair * W + w
        return A[pr["aidx"][k]].tolist(), l[pr["row0"] + k], u[pr["row0"] + k]

    assert row(0, 0, 1) == (tz[0], (r03 - (r03 + ma - P.E20)) + z(0, 1), G.INF)              # s = margin - 2^-20: active
    assert row(0, 1, 1) == row(0, 0, 1)                                                       # (b, a): n and J_a - J_b both change sign
    assert row(0, 0, 3) == (neg(tz[0]), -G.INF, G.INF) == row(0, 1, 3)                        # s = margin + 2^-20: not, written all the same
    assert row(1, 2, 2) == (tz[0], (r05 - (r05 - P.E20)) + z(1, 2), G.INF)                    # margin 0: s = -2^-20 | +2^-20
    assert row(1, 2, 4) == (neg(tz[0]), -G.INF, G.INF)
    for b in range(B):                                                                        # two TABLE balls: coincident, reach 0, n = +z
        assert row(b, 3, 2) == ([u - v for u, v in zip(tz[1], tz[2])], (tz[1][2] - tz[2][2]) * z(b, 2), G.INF)
    assert row(4, 4, 1) == (tz[1], tz[1][2] * z(4, 1), G.INF)                                 # coincident with a fixed ball, reach 0: accepted
    assert row(4, 4, 4) == (neg(tz[1]), -G.INF, G.INF)
    assert row(5, 0, 3) == (tz[0], r03 + z(5, 3), G.INF)                                      # coincident, reach 3/16: rejected; n = +z for (a, b) ...
    assert row(5, 1, 3) == (neg(tz[0]), r03 - z(5, 3), G.INF)                                 # ... and for (b, a)
    assert row(6, 0, 1) == (neg(tz[0]), (r03 - 1 / 4) - z(6, 1), G.INF) and row(6, 0, 2) == (tz[0], (r03 - 1 / 4) + z(6, 2), G.INF)


def _drain(s, max_advances=400):
    for _ in range(max_advances):
        if not s.running():
            return
        s.advance(1)
        s.poll(True)
    raise AssertionError("continuous solve did not finish")


@pytest.mark.parametrize("name", ["PT", "P7"])
def test_relinearise_some_and_the_solves_that_follow(handles, name):
    solver, sc, pr = handles(name, over=False, scaling=0)
    s, ref = P.scene(name), P.scene_reference(name)
    ids = [5, 2, 7, 0, 3, 1, 4, 6]
    x = s["trajs"][ids]                                                      # QP b gets trajectory b, in the order of the list
    rejected = [b for b in range(B) if not ref[b]["ok"]]
    assert rejected == ([3, 5] if name == "PT" else [0, 1, 2, 3])
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
    if name != "PT":
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
        print(f"\nQP {b}: device status {infos[k].status_val} after {infos[k].iter} iterations, oracle {st} after {o.info().iter}")
        assert (infos[k].status_val, infos[k].iter) == (st, o.info().iter), b
        if st == 1:
            assert np.max(np.abs(xs[k] - xo)) <= 1e-6


def test_no_pairs_is_the_cuboid_entry_point_bit_for_bit():
    """n_pairs = 0 through mi_gomp_scene_create_pairs against mi_gomp_scene_create_cuboids on scene X7 of cuboid_refs."""
    L = P.declare(M.lib())
    s, pr = X.scene("X7"), X.scene_batch("X7")
    got = {}
    for which in ("cuboids", "pairs"):
        h = _solver(pr)
        if which == "cuboids":
            sc = X.CuboidScene(L, h, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["con_lo"], s["con_hi"])
        else:
            sc = P.PairScene(L, h, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["cuboids"], [], s["con_lo"], s["con_hi"])
        assert sc.rc == 0 and sc.ptr
        assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
        rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
        assert rc == 0
        got[which] = (ok.tolist(), [sc.get_rows(b) for b in range(B)])
        sc.close()
        h.close()
    assert got["cuboids"][0] == got["pairs"][0] == [int(e["ok"]) for e in X.scene_reference("X7")]
    for a, b in zip(got["cuboids"][1], got["pairs"][1]):
        assert all(_same_bits(x, y) for x, y in zip(a, b))


def test_refusals_leave_the_handle_usable():
    L = P.declare(M.lib())
    s, pr = P.scene("P8"), P.scene_batch("P8")
    h = _solver(pr)
    prs = s["pairs"]

    def refused(code, pairs=prs, why=None, balls=s["balls"], **kw):
        rc, ptr = P.create_pairs(L, h._h, 8, 2, s["chain"], balls, s["lines"], [], [], pairs, s["con_lo"], s["con_hi"], **kw)
        assert rc == code and not ptr, (rc, ptr, L.mi_osqp_last_error())
        if why:
            assert why in L.mi_osqp_last_error().decode(), L.mi_osqp_last_error()

    refused(NULL, null_pairs=True, why="no pairs")
    refused(INVALID, n_pairs=-1, why="negative")
    refused(INVALID, [P.pair(0, 1, np.nan)], why="pair 0: the margin")
    refused(INVALID, [prs[0], P.pair(0, 1, -0.1)], why="pair 1: the margin")
    refused(INVALID, [P.pair(0, 2, 0.0)], why="pair 0: a and b must be balls")
    refused(INVALID, [P.pair(-1, 0, 0.0)], why="pair 0: a and b must be balls")
    refused(INVALID, [P.pair(1, 1, 0.0)], why="itself")
    same = [dict(s["balls"][1], gripper=False), s["balls"][1]]                # two balls of frame 8: as many rows as the scene's own two balls
    refused(INVALID, [P.pair(0, 1, 0.0)], why="one frame", balls=same)
    refused(INVALID, prs + prs, why="does not hold")                          # W rows more than the matrix has
    info = h.solve()                                                         # after all that the handle solves ...
    assert len(info) == B and all(i.iter > 0 for i in info)
    sc = P.PairScene(L, h, 8, 2, s["chain"], s["balls"], s["lines"], [], [], prs, s["con_lo"], s["con_hi"])
    assert sc.rc == 0 and sc.ptr                                             # ... and takes a scene, which works
    _rows_and_verdicts("P8", sc, pr)
    refused(INVALID, why="already has a scene")
    sc.close()
    sc = P.PairScene(L, h, 8, 2, s["chain"], s["balls"], s["lines"], [], [], prs, s["con_lo"], s["con_hi"])          # a second scene after the first
    assert sc.rc == 0 and sc.ptr
    sc.close()
    h.close()


def test_struct_size_and_symbol():
    assert C.sizeof(P.Pair) == 16
    assert hasattr(M.lib(), "mi_gomp_scene_create_pairs")
