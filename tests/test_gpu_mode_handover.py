"""GPU (-m gpu): per-QP results across hand-overs between the blocking calls and the continuous mode (mi_osqp.h
"continuous batching"), with a PROPER SUBSET of the handle's QPs taking part in the continuous phase.

The contract is the header's: a QP's result does not depend on what the other QPs of its handle do, a blocking call ends the
continuous mode, and a QP that finishes no solve in a continuous phase keeps the results it had on entry - through the
whole-batch getters after the phase and through the *_some getters within it.  So one handle is walked through mode changes,
and every QP is compared BIT FOR BIT (x, y, and status_val, iter, rho_updates, rho, obj_val, pri_res, dua_res) with a handle
that performed that QP's own history through blocking calls only.  The blocking path is tied to the oracle as in
test_gpu_continuous.py: two QPs of each scenario, same status and iteration count, max|x - x_oracle| <= TOL_X = 1e-6.

Problems: random_box_qp(11, n=96, mg=64, nnz_per_row=6) (B = 11: a ragged last tile for tiles of 2 and of 4) as data 0; data 1
the perturbation of test_update_and_warm_start_some_equal_the_whole_batch_calls_bitwise (seed 7: A values * (1 + 0.2 N(0,1)),
l * 1.3, u * 0.8, warm start 0.1 N(0,1)); data 2 a second one (seed 13, l * 0.8, u * 1.3).  On the oracle all 11 QPs end
kOptimal on all three, and the solutions of a QP on two data sets lie 0.198 to 0.739 apart in max-norm: every scenario asserts
on its reference results that each row a hand-over error would swap differs by at least 0.1 (POWER) from what it would be
swapped for.  The subsets [0, 3, 4, 7, 10] and its complement each split two-QP tiles (one QP in, its partner out) and take /
leave the ragged last tile.

Pinned memory is recycled between handles, and a fresh block may be all zeros: before the handle under test makes its first
per-QP call, _dirty() solves another problem (q * -3: solutions 1.3 to 2.0 away) through the continuous entry points on a
handle of the same shape and closes it, so that its images are the blocks handed out next.

What these scenarios caught (solver.hip cont_enter, before it seeded the images and the per-QP reports on entry): A, C, D, E
returned the dirtying handle's rows for the untouched QPs (max|dx| 0.94 to 1.78; the adjoint's dP off by 1 to 16), B returned
the first phase's solutions instead of the blocking solve's (max|dx| 0.198 and 0.324 on QPs 1 and 0), D also read status 0
where a never-solved handle reads -10; F passed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_refs as AR                                                       # noqa: E402
import exit_cases as EC                                                         # noqa: E402
import osqp_solver_amd as M                                                     # noqa: E402
from oracle import oracle as O                                                  # noqa: E402
from osqp_solver_amd import problems as PR                                      # noqa: E402
from test_gpu_adjoint import KEYS, SETTINGS as ADJOINT_SETTINGS                 # noqa: E402
from test_gpu_certificates import _check_certs                                  # noqa: E402
from test_gpu_continuous import _drain, _same                                   # noqa: E402
from test_gpu_exit_codes import _check, _env, _make, _ref                       # noqa: E402
from test_gpu_parity import TOL_X                                               # noqa: E402

pytestmark = pytest.mark.gpu
B, N = 11, 96
POWER = 0.1
SUBSETS = {"ends": [0, 3, 4, 7, 10], "middle": [1, 2, 5, 6, 8, 9]}
FIELDS = ("status_val", "iter", "rho_updates", "rho", "obj_val", "pri_res", "dua_res")
ALL_FIELDS = tuple(k for k, _ in M.Info._fields_)
ADJ_KW = dict(ADJOINT_SETTINGS, polish=0)
_BLOCKING, _ORACLE = {}, {}


def _others(S):
    return [b for b in range(B) if b not in S]


@pytest.fixture(scope="module")
def data():
    """the three data sets; [k] = (A values, l, u, warm start) for k = 1, 2"""
    pr = PR.random_box_qp(B, n=N, mg=64, nnz_per_row=6)
    sets = [None]
    for seed, fl, fu in ((7, 1.3, 0.8), (13, 0.8, 1.3)):
        rng = np.random.default_rng(seed)
        Ax = pr["Ax"] * (1.0 + 0.2 * rng.standard_normal(pr["Ax"].shape))
        sets.append((Ax, pr["l"] * fl, pr["u"] * fu, 0.1 * rng.standard_normal((B, N))))
    for a in [pr["Ax"], pr["l"], pr["u"], pr["q"]] + [a for s in sets[1:] for a in s]:
        a.setflags(write=False)
    return dict(pr=pr, sets=sets)


def _getters(s):
    """the whole-batch getters, in the order primal, dual, info (the first one ends the continuous mode)"""
    x, y = s.primal(), s.dual()
    return s.info(), x, y


def _some(s, ids):
    return s.info_some(ids), s.primal_some(ids), s.dual_some(ids)


def _eq(p, q):
    return p == q or (p != p and q != q)


def _gap(a, b):
    """largest difference over the entries that are numbers in both (for the messages)"""
    d = np.abs(a - b)
    d = d[~np.isnan(d)]
    return float(d.max()) if d.size else float("nan")


def _rows_equal(tag, getter, rows, got, want, fields=FIELDS, got_rows=None):
    """QP by QP: got = (info, x, y) equals want bit for bit; got_rows: the position of each QP of `rows` in got"""
    for k, b in enumerate(rows):
        g = b if got_rows is None else got_rows[k]
        assert np.array_equal(got[1][g], want[1][b], equal_nan=True), \
            f"{tag}: x of QP {b} from {getter[0]} differs, max|dx| = {_gap(got[1][g], want[1][b]):.3e}"
        assert np.array_equal(got[2][g], want[2][b], equal_nan=True), \
            f"{tag}: y of QP {b} from {getter[1]} differs, max|dy| = {_gap(got[2][g], want[2][b]):.3e}"
        for f in fields:
            assert _eq(getattr(got[0][g], f), getattr(want[0][b], f)), \
                f"{tag}: {f} of QP {b} from {getter[2]} is {getattr(got[0][g], f)}, expected {getattr(want[0][b], f)}"
        _same(got[0][g], got[1][g], want[0][b], want[1][b])


WHOLE = ("primal()", "dual()", "info()")
SOME = ("primal_some()", "dual_some()", "info_some()")


def _differ(tag, xa, xb, rows):
    """the power condition: a mix-up of the two results would move every listed row by at least POWER"""
    for b in rows:
        d = float(np.max(np.abs(xa[b] - xb[b])))
        assert d >= POWER, f"{tag}: QP {b} differs by only {d:.3e}: the comparison could not tell the two results apart"


def _dirty(pr, **kw):
    """Solve another problem of the same shape through the continuous entry points and close the handle: its pinned images
    go back to the pool and are the blocks the next handle's continuous mode is given.  Returns the solutions left in them."""
    d = _make(dict(pr, q=-3.0 * pr["q"]), **kw)
    ids = list(range(pr["Ax"].shape[0]))
    d.solve_begin_some(ids)
    assert sorted(_drain(d)) == ids
    xd, yd = d.primal_some(ids), d.dual_some(ids)
    d.close()
    return xd, yd


def _update_all(s, st):
    s.update_A_bounds(st[0], st[1], st[2])
    s.warm_start_x(st[3])


def _update_some(s, S, st):
    """the continuous part of scenario A: new data and a warm start for the QPs of S, their solves begun and finished"""
    s.update_A_bounds_some(S, st[0][S], st[1][S], st[2][S])
    s.warm_start_x_some(S, st[3][S])
    s.solve_begin_some(S)
    assert sorted(_drain(s)) == sorted(S)


def _blocking(tile, data, key="default", **kw):
    """The blocking-only histories, computed once per tile form and never changed: [k] = (info, x, y) after the solve on
    data k, each reached from the one before by update_A_bounds + warm_start_x + solve; ["unsolved"]: the getters of the
    handle right after setup."""
    if (tile, key) not in _BLOCKING:
        r = _make(data["pr"], **kw)
        assert r.stats()["tile"] == tile
        rec = {"unsolved": _getters(r)}
        r.solve()
        rec[0] = _getters(r)
        if key == "adjoint":
            gx, gy = AR.gradient_seeds(B, N, data["pr"]["m"])
            rec["adjoint"] = r.adjoint(gx, gy)
        for k in (1, 2):
            _update_all(r, data["sets"][k])
            r.solve()
            rec[k] = _getters(r)
        r.close()
        for k in (0, 1, 2):
            assert [i.status_val for i in rec[k][0]] == [1] * B, (k, [i.status_val for i in rec[k][0]])
            rec[k][1].setflags(write=False); rec[k][2].setflags(write=False)
        _BLOCKING[(tile, key)] = rec
    return _BLOCKING[(tile, key)]


def _oracle_history(data, b, key="default", **kw):
    """QP b on the oracle through data 0, 1, 2: [(status, iter, x)]"""
    if (b, key) not in _ORACLE:
        pr = data["pr"]
        P, A = PR.qp_matrices(pr, b)
        o = O.OracleQPSolver(P, pr["q"][b], A, pr["l"][b], pr["u"][b], **kw)
        st, x = o.solve()
        hist = [(st, o.info().iter, x)]
        for k in (1, 2):
            Ax, l, u, xw = data["sets"][k]
            Ak = A.copy(); Ak.data[:] = Ax[b]
            o.update(l[b], Ak, u[b]); o.set_warm_start(xw[b])
            st, x = o.solve()
            hist.append((st, o.info().iter, x))
        _ORACLE[(b, key)] = hist
    return _ORACLE[(b, key)]


def _oracle_parity(tag, data, ref, qps, steps, key="default", **kw):
    """the blocking reference against the oracle: same status and iteration count, x to TOL_X"""
    for b in qps:
        hist = _oracle_history(data, b, key, **kw)
        for k in steps:
            st, it, xo = hist[k]
            info, x, _ = ref[k]
            err = float(np.max(np.abs(x[b] - xo)))
            print(f"  {tag}: QP {b} data {k}: status {info[b].status_val} / {st}, iter {info[b].iter} / {it}, max|x - x_oracle| = {err:.3e}")
            assert (info[b].status_val, info[b].iter) == (st, it), (tag, b, k, info[b].status_val, info[b].iter, st, it)
            assert err <= TOL_X, (tag, b, k, err)


TILES = pytest.mark.parametrize("tile", [1, 2, 4])
SUBS = pytest.mark.parametrize("sub", sorted(SUBSETS))


# ---- A: blocking solve, continuous subset, whole-batch getters --------------------------------------------------------------

@TILES
@SUBS
def test_a_blocking_then_continuous_subset(tile, sub, data, monkeypatch):
    _env(monkeypatch, tile)
    pr, S = data["pr"], SUBSETS[sub]
    rest = _others(S)
    ref = _blocking(tile, data)
    _oracle_parity(f"A tile{tile}", data, ref, (S[1], rest[1]), (0, 1))
    _differ("A, updated rows", ref[1][1], ref[0][1], S)
    xd, _ = _dirty(pr)
    _differ("A, kept rows against the recycled image", xd, ref[0][1], rest)
    s = _make(pr)
    assert s.stats()["tile"] == tile
    s.solve()
    _update_some(s, S, data["sets"][1])
    got = _getters(s)
    _rows_equal(f"A tile{tile}, re-solved in the continuous phase", WHOLE, S, got, ref[1])
    _rows_equal(f"A tile{tile}, untouched since the blocking solve", WHOLE, rest, got, ref[0])
    s.close()


# ---- B: continuous, blocking, continuous subset, whole-batch getters ---------------------------------------------------------

@TILES
@SUBS
def test_b_continuous_blocking_then_continuous_subset(tile, sub, data, monkeypatch):
    _env(monkeypatch, tile)
    pr, S = data["pr"], SUBSETS[sub]
    rest, ids = _others(S), list(range(B))
    ref = _blocking(tile, data)
    _oracle_parity(f"B tile{tile}", data, ref, (S[0], rest[0]), (0, 1, 2))
    _differ("B, updated rows", ref[2][1], ref[1][1], S)
    _differ("B, kept rows against the first phase", ref[1][1], ref[0][1], rest)
    _dirty(pr)
    s = _make(pr)
    assert s.stats()["tile"] == tile
    s.solve_begin_some(ids)                                    # first phase: everything, data 0
    assert sorted(_drain(s)) == ids
    _rows_equal(f"B tile{tile}, first phase", SOME, ids, _some(s, ids), ref[0])
    _update_all(s, data["sets"][1])                            # blocking: data 1
    s.solve()
    _rows_equal(f"B tile{tile}, blocking solve", WHOLE, ids, _getters(s), ref[1])
    _update_some(s, S, data["sets"][2])                        # second phase: data 2 for S only
    some = _some(s, ids)                                       # (just before the mode is left)
    _rows_equal(f"B tile{tile}, second phase, re-solved", SOME, S, some, ref[2])
    _rows_equal(f"B tile{tile}, second phase, untouched since the blocking solve", SOME, rest, some, ref[1])
    got = _getters(s)
    _rows_equal(f"B tile{tile}, re-solved in the second phase", WHOLE, S, got, ref[2])
    _rows_equal(f"B tile{tile}, untouched since the blocking solve", WHOLE, rest, got, ref[1])
    s.close()


# ---- C: *_some getters of QPs that have not finished a solve in this phase ----------------------------------------------------

@TILES
@SUBS
def test_c_some_getters_before_a_qp_finishes_in_the_phase(tile, sub, data, monkeypatch):
    """They return what the whole-batch getters returned on entry, in every field of mi_osqp_info; the certificates of such
    QPs read NaN (mi_osqp.h)."""
    _env(monkeypatch, tile)
    pr, S = data["pr"], SUBSETS[sub]
    rest = _others(S)
    ref = _blocking(tile, data)
    _oracle_parity(f"C tile{tile}", data, ref, (S[2], rest[2]), (0,))
    xd, _ = _dirty(pr)
    _differ("C, kept rows against the recycled image", xd, ref[0][1], rest)
    s = _make(pr)
    assert s.stats()["tile"] == tile
    s.solve()
    entry = _getters(s)
    _rows_equal(f"C tile{tile}, blocking solve", WHOLE, range(B), entry, ref[0])
    s.solve_begin_some(S)                                      # enters the mode; a plain warm re-solve of S
    for when in ("before any advance", "after the phase's solves"):
        _rows_equal(f"C tile{tile}, {when}", SOME, rest, _some(s, rest), entry, fields=ALL_FIELDS, got_rows=range(len(rest)))
        assert np.all(np.isnan(s.prim_inf_cert_some(rest))) and np.all(np.isnan(s.dual_inf_cert_some(rest))), when
        if s.running():
            assert sorted(_drain(s)) == S
    assert all(i.status_val == 1 for i in s.info_some(S))
    _rows_equal(f"C tile{tile}, after the phase", WHOLE, rest, _getters(s), entry, fields=ALL_FIELDS)
    s.close()


@TILES
def test_c_certificates_of_a_blocking_solve_survive_a_continuous_phase(tile, monkeypatch):
    """exit_cases.all_codes_batch: 13 QPs with every exit code.  Solved blocking, then two of the three feasible QPs solved
    again in the continuous mode: x, y, info and the certificates of every other QP are those of a handle that only solved
    blocking - the NaN rows of the infeasible QPs included -, within the phase (certificates: NaN) and after it."""
    _env(monkeypatch, tile)
    base = PR.random_box_qp(EC.BASE_B, **EC.BASE_SHAPE)
    pr, kw, expect = EC.all_codes_batch(base, "s10")
    nq = len(expect)
    S = [0, 7]
    assert [expect[b] for b in S] == [1, 1] and expect[4] == 2            # (feasible QPs; the third one stays out)
    rest = [b for b in range(nq) if b not in S]
    ref = _ref(("all", "s10"), pr, kw)
    twin = _make(pr, **kw)
    assert twin.stats()["tile"] == tile
    twin.solve()
    want = _getters(twin)
    pb, db = twin.prim_inf_cert(), twin.dual_inf_cert()
    twin.close()
    _check(want[0], want[1], want[2], ref, set())
    _check_certs(f"handover tile{tile}, blocking only", ("all", "s10"), pr, kw, ref, want[0], pb, db)
    nosol = [b for b in rest if expect[b] in (3, 4, -3, -4)]
    assert len(nosol) >= 6 and all(np.all(np.isnan(want[1][b])) and np.all(np.isnan(want[2][b])) for b in nosol)
    _dirty(pr, **kw)
    s = _make(pr, **kw)
    s.solve()
    s.solve_begin_some(S)
    for when in ("before any advance", "after the phase's solves"):
        _rows_equal(f"certificates tile{tile}, {when}", SOME, rest, _some(s, rest), want, fields=ALL_FIELDS, got_rows=range(len(rest)))
        assert np.all(np.isnan(s.prim_inf_cert_some(rest))) and np.all(np.isnan(s.dual_inf_cert_some(rest))), when
        if s.running():
            assert sorted(_drain(s)) == S
    pv, dv = s.prim_inf_cert(), s.dual_inf_cert()              # (ends the mode)
    assert np.array_equal(pv, pb, equal_nan=True), "prim_inf_cert() after the phase differs from the blocking-only handle's"
    assert np.array_equal(dv, db, equal_nan=True), "dual_inf_cert() after the phase differs from the blocking-only handle's"
    got = _getters(s)
    _rows_equal(f"certificates tile{tile}, after the phase", WHOLE, rest, got, want, fields=ALL_FIELDS)
    for b in nosol:
        assert np.all(np.isnan(got[1][b])) and np.all(np.isnan(got[2][b])), f"QP {b} (status {expect[b]}): primal() / dual() no longer NaN"
    assert [i.status_val for i in got[0]] == expect
    _check_certs(f"handover tile{tile}, after the phase", ("all", "s10"), pr, kw, ref, got[0], pv, dv)
    s.close()


# ---- D: never solved ---------------------------------------------------------------------------------------------------------

@TILES
@SUBS
def test_d_qps_never_solved(tile, sub, data, monkeypatch):
    """A fresh handle solves S only: the other QPs read as on a handle that was set up and never solved (zero x and y,
    status_val -10, the rho of setup) - compared with that handle's getters, not with constants."""
    _env(monkeypatch, tile)
    pr, S = data["pr"], SUBSETS[sub]
    rest = _others(S)
    ref = _blocking(tile, data)
    _oracle_parity(f"D tile{tile}", data, ref, (S[0], S[-1]), (0,))
    xd, _ = _dirty(pr)
    _differ("D, unsolved rows against the recycled image", xd, ref["unsolved"][1], rest)
    s = _make(pr)
    assert s.stats()["tile"] == tile
    s.solve_begin_some(S)
    _rows_equal(f"D tile{tile}, within the phase", SOME, rest, _some(s, rest), ref["unsolved"], fields=ALL_FIELDS, got_rows=range(len(rest)))
    assert sorted(_drain(s)) == S
    got = _getters(s)
    _rows_equal(f"D tile{tile}, solved in the phase", WHOLE, S, got, ref[0])
    _rows_equal(f"D tile{tile}, never solved", WHOLE, rest, got, ref["unsolved"], fields=ALL_FIELDS)
    s.close()


# ---- E: adjoint after a hand-over ----------------------------------------------------------------------------------------------

@TILES
@SUBS
def test_e_adjoint_differentiates_the_blocking_point(tile, sub, data, monkeypatch):
    """(the accuracy of the adjoint itself is test_gpu_adjoint.py's business: here its inputs must be the blocking solve's)"""
    _env(monkeypatch, tile)
    pr, S = data["pr"], SUBSETS[sub]
    rest = _others(S)
    ref = _blocking(tile, data, "adjoint", **ADJ_KW)
    _oracle_parity(f"E tile{tile}", data, ref, (S[1], rest[1]), (0,), "adjoint", eps_abs=ADJ_KW["eps_abs"], eps_rel=ADJ_KW["eps_rel"])
    twin = ref["adjoint"]
    assert all(twin["status"][b] == 1 and not np.any(np.isnan(twin[k][b])) for b in rest for k in KEYS)
    _differ("E, updated rows", ref[1][1], ref[0][1], S)
    xd, _ = _dirty(pr, **ADJ_KW)
    _differ("E, kept rows against the recycled image", xd, ref[0][1], rest)
    s = _make(pr, **ADJ_KW)
    assert s.stats()["tile"] == tile
    s.solve()
    _update_some(s, S, data["sets"][1])
    gx, gy = AR.gradient_seeds(B, N, pr["m"])
    out = s.adjoint(gx, gy)
    for b in rest:
        assert out["status"][b] == twin["status"][b], f"E tile{tile}: adjoint() status of QP {b} is {out['status'][b]}, the twin's {twin['status'][b]}"
        for k in KEYS:
            assert np.array_equal(out[k][b], twin[k][b], equal_nan=True), \
                f"E tile{tile}: {k} of QP {b} from adjoint() differs from the twin's, max = {_gap(out[k][b], twin[k][b]):.3e}"
    _rows_equal(f"E tile{tile}, untouched since the blocking solve", WHOLE, rest, _getters(s), ref[0])
    s.close()


# ---- F: solves in flight are forgotten ----------------------------------------------------------------------------------------

@TILES
def test_f_solves_in_flight_are_forgotten(tile, data, monkeypatch):
    _env(monkeypatch, tile)
    pr, ids = data["pr"], list(range(B))
    ref = _blocking(tile, data)
    _oracle_parity(f"F tile{tile}", data, ref, (2, 9), (0,))
    _dirty(pr)
    s = _make(pr)
    assert s.stats()["tile"] == tile
    s.solve_begin_some(ids)
    s.advance(1)                                               # (no poll: a launch is in flight, every solve unfinished)
    assert s.running() == B
    s.reset()
    assert s.running() == 0
    s.solve()
    assert s.running() == 0
    _rows_equal(f"F tile{tile}, blocking solve after reset()", WHOLE, ids, _getters(s), ref[0])
    s.close()
