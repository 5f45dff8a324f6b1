"""GPU (-m gpu): distance grids (mi_gomp_grid, the grid loop of gomp_relinearise_kernel) through mi_gomp_scene_create_grids,
mi_gomp_scene_update_grid and every call that launches the kernel, against the mpmath reference of tests/grid_refs.py.

Scenes GT and GP (the TABLE model with the identity table, every number dyadic, compared BIT FOR BIT: a grid of 3 x 4 x 5 nodes
with three different extents and values without a symmetry; a node, a point on a cell face, the last node of every axis, 2^-20
outside on either side of every axis - zero rows and no verdict -, mid-cell points, a cell of eight equal values, the activity
flips at s = margin -+ 2^-20 for margin 1/8 and margin 0, the verdict flips at s = -1e-3 -+ 2^-20, a second grid with an offset),
scene G8 (8 joints, 2 waypoints, one ball, one grid of 2 x 2 x 2), scene G7 (the 7-joint chain of dh_refs, 40 waypoints, 7 balls =
280 items: both sides of the 256-thread stride; 9 x 8 x 7 nodes sampled from a box and a capsule, and 3 x 3 x 3 nodes that most
balls are outside of; a line, a capsule, a cuboid, two pairs and a tilt beside them: the shifted pair and tilt rows), scene GM
(a gripper ball's work-space rows, two lines, a capsule, a cuboid and a grid, once with the builder's over-allocated empty rows:
the row order), scene GN (trajectories of GT with a NaN, a +inf and a 1e300 joint value: those items read as outside) and scene
GX (cuboid_refs' XT re-sampled as a grid: the cuboid's rows exactly in the face regions).  Rows within 32 x the fp64 error of
the formulas themselves and never looser than 1e-13 (grid_refs.gpu_tolerance; tests/test_grid_refs.py holds the figures), no row
of the committed trajectories near a threshold and no verdict excluded; joint-space entries, unlisted QPs and unpopulated rows
bit for bit.  The re-linearised QP of GT is solved and compared with the oracle on the rows read back.
Observed on an MI355X (device - reference; values absolute / bounds of their term scale reach + |phi| + sum |g_j q_j|): GT, GP and
GX 0 / 0 (bit for bit), G8 2.9e-17 / 2.4e-16 (tolerance 1.1e-15 / 6.9e-15), G7 1.6e-15 / 4.1e-15 (5.8e-14 / 1.0e-13), GM 8.9e-16 /
5.3e-16 (2.8e-14 / 1.6e-14), the same with over-allocated rows; the re-linearised QP of GT: device and oracle both solved after 50
iterations.  Run with -s to see the figures."""
import ctypes as C

import numpy as np
import pytest

import cuboid_refs as X
import gomp_refs as G
import grid_refs as R
import osqp_solver_amd as M
import tilt_refs as T
from oracle import oracle as O

pytestmark = pytest.mark.gpu
B = 8
IDS_A, IDS_B = [5, 2, 7, 0, 3], [6, 1, 4]          # permuted strict subsets of the batch
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _scene(L, solver, s, grids=None):
    return R.GridScene(L, solver, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["pairs"], s["tilts"],
                       s["grids"] if grids is None else grids, s["con_lo"], s["con_hi"])


def _make(name, over=False, **kw):
    s, pr = R.scene(name), R.scene_batch(name, over)
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


def _check_rows(name, pr, got, ref, worst, tol=None, exact=None):
    """The rows (A, l, u) read back for a listed QP against the reference `ref` of its trajectory and, outside the populated
    3-D rows, against what set_rows wrote (got[3:])."""
    A, l, u, A0, l0, u0 = got
    r0, r1 = pr["row0"], pr["row0"] + pr["rows3d"]
    assert pr["rows3d"] == len(ref["l"])
    joint = np.ones(len(A), bool)
    joint[pr["aidx"].reshape(-1)] = False
    assert _same_bits(A[joint], A0[joint])                                    # joint-space entries
    assert _same_bits(l[:r0], l0[:r0]) and _same_bits(u[:r0], u0[:r0])
    assert _same_bits(l[r1:], l0[r1:]) and _same_bits(u[r1:], u0[r1:])        # unpopulated rows (behind the last row)
    vals = A[pr["aidx"]]
    tv, tb = R.gpu_tolerance(name) if tol is None else tol
    assert not ref["near"].any()
    ev = float(np.max(np.abs(vals - ref["vals"])))
    worst["values"] = max(worst.get("values", 0.0), ev)
    print(f"  scene {name}: values {ev:.3e} (tolerance {tv:.3e})", end="")
    bounds = []
    for side, dev in (("l", l[r0:r1]), ("u", u[r0:r1])):
        sc = ref[side + "_scale"]
        inf = sc == 0
        assert _same_bits(dev[inf], ref[side][inf])                           # an absent side, a dummy, inactive or outside row: -+1e30 exactly
        fin = sc > 0
        eb = float(np.max(np.abs(dev[fin] - ref[side][fin]) / sc[fin], initial=0.0))
        worst["bounds"] = max(worst.get("bounds", 0.0), eb)
        bounds.append((side, eb))
    print(f", bounds {max(e for _, e in bounds):.3e} of their term scale (tolerance {tb:.3e})")
    assert ev <= tv, (ev, tv)
    for side, eb in bounds:
        assert eb <= tb, (side, eb, tb)
    outside = np.array([c == "outside" for c in ref["cls"]])
    assert not vals[outside].any()                                            # the zeros are written
    if name in R.EXACT if exact is None else exact:                           # the exact cases: bit for bit
        assert np.array_equal(vals, ref["vals"]) and np.array_equal(l[r0:r1], ref["l"]) and np.array_equal(u[r0:r1], ref["u"])


def _check_verdicts(ok, refs):
    for j, r in enumerate(refs):
        assert ok[j] in (0, 1)
        assert not r["verdict_excluded"]
        assert bool(ok[j]) == r["ok"], j


def _rows_and_verdicts(name, sc, pr):
    s, ref = R.scene(name), R.scene_reference(name)
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
    tv, tb = R.gpu_tolerance(name)
    print(f"\nscene {name}: worst device - reference: values {worst['values']:.3e} (tolerance {tv:.3e}),"
          f" bounds {worst['bounds']:.3e} of their term scale (tolerance {tb:.3e})")


@pytest.mark.parametrize("name,over", [("GT", False), ("GP", False), ("G8", False), ("G7", False), ("GM", False), ("GM", True)])
def test_rows_and_verdicts_of_permuted_id_lists(handles, name, over):
    solver, sc, pr = handles(name, over=over)
    if over:
        assert pr["m"] > pr["row0"] + pr["rows3d"]                            # empty rows behind the last row
    _rows_and_verdicts(name, sc, pr)


def test_the_flips_of_scene_GT_on_the_device(handles):
    """What tests/test_grid_refs.py pins in the reference, read from the device's rows: 2^-20 decide activity and verdict."""
    solver, sc, pr = handles("GT", over=False)
    s = R.scene("GT")
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
    assert rc == 0 and ok.tolist() == [1, 1, 1, 1, 1, 1, 0, 1]               # 5 | 6: the verdict flips; 1: outside, no verdict

    def row(b, grid, w):
        A, l, u = sc.get_rows(b)
        k = w * 2 + grid
        assert u[pr["row0"] + k] == G.INF
        return A[pr["aidx"][k]].tolist(), l[pr["row0"] + k]

    assert row(4, 0, 1)[1] != -G.INF and row(4, 0, 2)[1] == -G.INF and row(4, 0, 1)[0][0] == row(4, 0, 2)[0][0] == 1.0       # margin 1/8; written all the same
    assert row(7, 1, 1)[1] != -G.INF and row(7, 1, 2)[1] == -G.INF and row(7, 1, 1)[0] == [1.0, 0.0, 0.0]       # grid B: offset 1/16, margin 0
    for w in range(s["W"]):
        assert row(1, 0, w) == ([0.0, 0.0, 0.0], -G.INF) and row(1, 1, w) == ([0.0, 0.0, 0.0], -G.INF)          # outside: zero rows
    for w in (1, 3, 5, 6):
        assert row(3, 0, w) == ([0.0, 0.0, 0.0], -G.INF)                                                        # the flat cell: G = 0


def _gn_trajectories():
    """Scene GN: trajectories 0, 2 and 3 of GT with one joint value of one waypoint replaced: a NaN, +inf, 1e300."""
    t = R.scene("GT")["trajs"][[0, 2, 3]].copy()
    t[0, 1 * 3 + 0] = np.nan                                                 # waypoint 1 (a node), x
    t[1, 2 * 3 + 1] = np.inf                                                 # waypoint 2 (mid-cell), y
    t[2, 5 * 3 + 2] = 1e300                                                  # waypoint 5 (the last node), z
    return t


def test_scene_GN_coordinates_that_are_not_finite_read_as_outside(handles):
    """The address-safety rule of gomp_grid_sample on valid input: an item whose centre is NaN, inf or huge is outside every
    grid - a zero row without bounds and no verdict - and the other rows are the reference's."""
    solver, sc, pr = handles("GT", over=False)
    s = R.scene("GT")
    trajs = _gn_trajectories()
    refs = [R.with_obstacles(s["D"], s["W"], None, s["balls"], [], [], [], [], [], s["grids"], None, None, t) for t in trajs]
    for r, w in zip(refs, (1, 2, 5)):
        assert r["cls"][2 * w] == r["cls"][2 * w + 1] == "outside" and r["ok"]
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    before = [sc.get_rows(b) for b in range(B)]
    for write in ("assemble", "relinearise"):
        rc, ok = (sc.assemble_some if write == "assemble" else sc.relinearise_some)([6, 0, 3], trajs)
        assert rc == 0, M.lib().mi_osqp_last_error()
        assert ok.tolist() == [1, 1, 1]
        if write == "assemble":
            for j, b in enumerate([6, 0, 3]):
                _check_rows("GT", pr, sc.get_rows(b) + before[b], refs[j], {})


@pytest.mark.parametrize("name", ["GT", "G7"])
def test_relinearise_some_and_the_solves_that_follow(handles, name):
    solver, sc, pr = handles(name, over=False, scaling=0)
    s, ref = R.scene(name), R.scene_reference(name)
    ids = [5, 2, 7, 0, 3, 1, 4, 6]
    x = s["trajs"][ids]                                                      # QP b gets trajectory b, in the order of the list
    rejected = [b for b in range(B) if not ref[b]["ok"]]
    assert rejected == ([6] if name == "GT" else list(range(B)))
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
    if name == "G7":
        return
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
        if st == 1:
            assert np.max(np.abs(xs[k] - xo)) <= 1e-6


def test_update_grid_gives_the_rows_of_a_fresh_scene_with_the_new_values():
    """A new camera frame: update_grid then assemble_some is bit-identical to a scene created with the new values, and is the
    reference of the new values (scene GT stays exact: the new values are the old ones + 1/32)."""
    L = R.declare(M.lib())
    s, pr = R.scene("GT"), R.scene_batch("GT")
    new_a = dict(s["grids"][0], values=[v + 1 / 32 for v in s["grids"][0]["values"]])
    grids = [new_a, s["grids"][1]]
    refs = [R.with_obstacles(s["D"], s["W"], None, s["balls"], [], [], [], [], [], grids, None, None, t) for t in s["trajs"]]
    lo = [R.with_obstacles(s["D"], s["W"], None, s["balls"], [], [], [], [], [], grids, None, None, t, K_=G.F64) for t in s["trajs"]]
    assert all(np.array_equal(a["vals"], b["vals"]) and np.array_equal(a["l"], b["l"]) for a, b in zip(refs, lo))      # still exact
    assert [r["ok"] for r in refs] == [True] * B and not R.scene_reference("GT")[6]["ok"]      # the new frame changes a verdict
    got = {}
    for which in ("updated", "fresh"):
        h = _solver(pr)
        sc = _scene(L, h, s, grids=None if which == "updated" else grids)
        assert sc.rc == 0 and sc.ptr
        assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
        if which == "updated":
            rc, ok = sc.assemble_some(list(range(B)), s["trajs"])             # the old values first
            assert rc == 0 and ok.tolist() == [int(r["ok"]) for r in R.scene_reference("GT")]
            kept = [sc.get_rows(b) for b in range(B)]
            bad = list(new_a["values"])
            bad[7] = np.nan
            assert sc.update_grid(0, bad) == INVALID and "grid 0" in L.mi_osqp_last_error().decode()       # refused: nothing changes
            assert sc.update_grid(2, new_a["values"]) == INVALID and sc.update_grid(-1, new_a["values"]) == INVALID
            rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
            assert rc == 0 and all(_same_bits(x, y) for b in range(B) for x, y in zip(sc.get_rows(b), kept[b]))
            assert sc.update_grid(0, new_a["values"]) == 0
            assert all(_same_bits(x, y) for b in range(B) for x, y in zip(sc.get_rows(b), kept[b]))     # kept rows are not touched
        rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
        assert rc == 0
        got[which] = (ok.tolist(), [sc.get_rows(b) for b in range(B)])
        if which == "fresh":
            for b in range(B):
                _check_rows("GT", pr, got[which][1][b] + (pr["Ax"][b], pr["l"][b], pr["u"][b]), refs[b], {})
        sc.close()
        h.close()
    assert got["updated"][0] == got["fresh"][0] == [int(r["ok"]) for r in refs]
    for a, b in zip(got["updated"][1], got["fresh"][1]):
        assert all(_same_bits(x, y) for x, y in zip(a, b))


def test_no_grids_is_the_tilt_entry_point_bit_for_bit():
    """n_grids = 0 through mi_gomp_scene_create_grids against mi_gomp_scene_create_tilts on scene TM of tilt_refs; update_grid
    refuses a scene without grids."""
    L = R.declare(M.lib())
    s, pr = T.scene("TM"), T.scene_batch("TM")
    got = {}
    for which in ("tilts", "grids"):
        h = _solver(pr)
        if which == "tilts":
            sc = T.TiltScene(L, h, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["pairs"], s["tilts"], s["con_lo"], s["con_hi"])
        else:
            sc = _scene(L, h, s, grids=[])
            assert L.mi_gomp_scene_update_grid(sc.ptr, 0, G._dp(np.zeros(8))) == INVALID and "no grids" in L.mi_osqp_last_error().decode()
        assert sc.rc == 0 and sc.ptr
        assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
        rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
        assert rc == 0
        got[which] = (ok.tolist(), [sc.get_rows(b) for b in range(B)])
        sc.close()
        h.close()
    assert got["tilts"][0] == got["grids"][0] == [int(e["ok"]) for e in T.scene_reference("TM")]
    for a, b in zip(got["tilts"][1], got["grids"][1]):
        assert all(_same_bits(x, y) for x, y in zip(a, b))


def test_a_resampled_box_gives_the_cuboids_rows_in_the_face_regions():
    """Scene GX (cuboid 0 of cuboid_refs' XT as a grid whose nodes fall on the cube's faces) on the device against the CUBOID's
    reference rows of scene XT, exactly, at the points of grid_refs.face_region_exact()."""
    s, pr = R.scene("GX"), R.scene_batch("GX")
    h = _solver(pr)
    sc = _scene(M.lib(), h, s)
    assert sc.rc == 0
    assert sc.set_rows(range(B), pr["Ax"], pr["l"], pr["u"]) == 0
    rc, ok = sc.assemble_some(list(range(B)), s["trajs"])
    assert rc == 0
    xt = X.scene_reference("XT")
    W, same = s["W"], 0
    for t in range(B):
        A, l, u = sc.get_rows(t)
        _check_rows("GX", pr, (A, l, u, pr["Ax"][t], pr["l"][t], pr["u"][t]), R.scene_reference("GX")[t], {}, exact=True)
        for bi in range(len(s["balls"])):
            for w in range(W):
                if not R.face_region_exact(s["trajs"][t][3 * w:3 * w + 3]):
                    continue
                kg, kx = bi * W + w, (bi * W + w) * 2
                assert A[pr["aidx"][kg]].tolist() == xt[t]["vals"][kx].tolist() and l[pr["row0"] + kg] == xt[t]["l"][kx], (t, bi, w)
                same += 1
    assert same >= 10
    sc.close()
    h.close()


def test_refusals_leave_the_handle_usable():
    L = R.declare(M.lib())
    s, pr = R.scene("G8"), R.scene_batch("G8")
    h = _solver(pr)
    ok = s["grids"][0]

    def refused(code, grids, why=None, **kw):
        rc, ptr = R.create_grids(L, h._h, 8, 2, s["chain"], s["balls"], [], [], [], [], [], grids, None, None, **kw)
        assert rc == code and not ptr, (rc, ptr, L.mi_osqp_last_error())
        if why:
            assert why in L.mi_osqp_last_error().decode(), L.mi_osqp_last_error()

    refused(NULL, [ok], null_grids=True, why="no grids")
    refused(NULL, [ok], null_values=(0,), why="grid 0")
    refused(INVALID, [ok], n_grids=-1, why="negative")
    refused(INVALID, [dict(ok, n=[2, 1, 2])], why="grid 0: n[1]")
    refused(INVALID, [dict(ok, cell=0.0)], why="grid 0: cell")
    refused(INVALID, [dict(ok, values=[0.0] * 7 + [np.inf])], why="(1, 1, 1)")
    refused(INVALID, [ok, ok], why="does not hold")                           # a row per (ball, waypoint) more than the matrix has
    assert "(grid 0)" in L.mi_osqp_last_error().decode()                      # the first row the matrix lacks: (waypoint 1, grid 0)
    info = h.solve()                                                         # after all that the handle solves ...
    assert len(info) == B and all(i.iter > 0 for i in info)
    sc = _scene(L, h, s)
    assert sc.rc == 0 and sc.ptr                                             # ... and takes a scene, which works
    _rows_and_verdicts("G8", sc, pr)
    refused(INVALID, [ok], why="already has a scene")
    sc.close()
    h.close()


def test_struct_size_and_symbols():
    assert C.sizeof(R.Grid) == 72
    assert hasattr(M.lib(), "mi_gomp_scene_create_grids") and hasattr(M.lib(), "mi_gomp_scene_update_grid")
