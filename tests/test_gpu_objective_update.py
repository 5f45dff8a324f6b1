"""GPU (-m gpu): objective updates and dual warm starts (README "Objective updates"): osqp_update_lin_cost,
osqp_update_P, osqp_update_P_A and osqp_warm_start_y on every path (blocking, device input, continuous, shards, shim).

The oracle has no objective updates.  So every comparison with it uses a case where OSQP's semantics coincide with a
fresh setup (scaling off for q; a handle that has not solved yet for P), and the rest checks properties of the problem
itself (the reduced KKT system of the reported active set, oracle/kkt_check.py) or bitwise agreement between paths."""
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import osqp_solver_amd as M
from oracle import oracle as O
from oracle.kkt_check import kkt_residuals, sym_from_any
from osqp_solver_amd import problems as PR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_X = 1e-6
ST2EXIT = {1: 0, -3: 1, -4: 2, 2: 3, 3: 4, 4: 5, -2: 6, -7: 9, -10: 10}


def _make(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _oracle(pr, b, P=None, q=None, A=None, **kw):
    P0, A0 = PR.qp_matrices(pr, b)
    qb = q if q is not None else (None if pr["q"] is None else pr["q"][b])
    o = O.OracleQPSolver(P0 if P is None else P, qb, A0 if A is None else A, pr["l"][b], pr["u"][b], **kw)
    st, x = o.solve()
    return st, x, o.info()


def _compare(info, x, b, ref):
    """what test_gpu_parity._compare checks"""
    st, xo, io = ref
    assert info[b].status_val == st, (b, info[b].status_val, st)
    assert info[b].exit_code == ST2EXIT[st]
    assert info[b].iter == io.iter, (b, info[b].iter, io.iter)
    assert info[b].rho_updates == io.rho_updates
    if np.any(np.isnan(xo)):
        assert np.all(np.isnan(x[b]))
    else:
        assert np.max(np.abs(x[b] - xo)) <= TOL_X, (b, np.max(np.abs(x[b] - xo)))
        assert abs(info[b].pri_res - io.pri_res) <= 1e-6 * (1 + abs(io.pri_res))
        assert abs(info[b].obj_val - io.obj_val) <= 1e-6 * (1 + abs(io.obj_val))


def _with_P(pr, Px):
    """scipy upper-triangle P of every QP with the values Px[b]"""
    return [sp.csc_matrix((Px[b], pr["P"].indices, pr["P"].indptr), shape=pr["P"].shape) for b in range(len(Px))]


def _full_form(pr, Px):
    """P with both triangles: (pattern, values [B][nnz]) in CSC order"""
    idx = pr["P"].copy().astype(float)
    idx.data = np.arange(1, idx.nnz + 1, dtype=float)
    F = sym_from_any(idx)
    F.sort_indices()
    src = F.data.astype(np.int64) - 1
    pat = F.copy(); pat.data = np.ones(F.nnz)
    return pat, np.ascontiguousarray(Px[:, src])


def _state(s):
    info = s.info()
    return ([(i.status_val, i.iter, i.rho_updates, i.obj_val, i.pri_res, i.dua_res, i.rho) for i in info],
            s.primal().copy(), s.dual().copy())


def _same_state(a, b):
    assert a[0] == b[0]
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])


def _new_q(pr, seed):
    return np.random.default_rng(seed).standard_normal((pr["l"].shape[0], pr["n"]))


# ---------------------------------------------------------------- 1. update_q, scaling off
@pytest.mark.parametrize("case", ["box_tile1", "box_tile2", "gomp"])
def test_update_q_without_scaling_matches_an_oracle_setup_with_the_new_q(case, monkeypatch):
    if case == "gomp":
        pr = PR.gomp_batch(6, 3, 12)
    else:
        monkeypatch.setenv("MI_OSQP_TILE", case[-1])
        pr = PR.random_box_qp(6, n=64, mg=48, nnz_per_row=4)
    s = _make(pr, scaling=0)
    if case != "gomp":
        assert s.stats()["tile"] == int(case[-1])
    q1 = _new_q(pr, 31) * (0.1 if case == "gomp" else 1.0)
    s.update_q(q1)
    info = s.solve(); x = s.primal()
    for b in range(s.B):
        _compare(info, x, b, _oracle(pr, b, q=q1[b], scaling=0))


# ---------------------------------------------------------------- 2. update_P, scaling on, fresh handle
@pytest.mark.parametrize("B", [20, 6])          # device Ruiz (B >= 16) / host Ruiz (B < 16)
def test_update_P_on_a_fresh_handle_matches_an_oracle_setup_with_the_new_P(B):
    pr = PR.random_box_qp(B, n=64, mg=48, nnz_per_row=4)
    Px1 = PR.random_box_qp(B, n=64, mg=48, nnz_per_row=4, value_seed=7000)["Px"]
    s = _make(pr)
    s.update_P(Px1)
    info = s.solve(); x = s.primal()
    P1 = _with_P(pr, Px1)
    for b in range(B):
        _compare(info, x, b, _oracle(pr, b, P=P1[b]))


def test_update_P_device_and_host_equilibration_agree_bitwise(monkeypatch):
    pr = PR.random_box_qp(20, n=64, mg=48, nnz_per_row=4)
    other = PR.random_box_qp(20, n=64, mg=48, nnz_per_row=4, value_seed=7000)
    q1 = _new_q(pr, 5)
    res = []
    for host in (False, True):
        monkeypatch.delenv("MI_OSQP_DEVICE_RUIZ" if host else "MI_OSQP_HOST_RUIZ", raising=False)
        monkeypatch.setenv("MI_OSQP_HOST_RUIZ" if host else "MI_OSQP_DEVICE_RUIZ", "1")
        s = _make(pr)
        s.update_P(other["Px"])
        s.solve(); r1 = _state(s)
        s.update_q(q1)                                         # (host path: the mirrors' q follows)
        s.update_P_A(pr["Px"], other["Ax"])
        s.solve(); r2 = _state(s)
        s.update_bounds(pr["l"] * 0.5, pr["u"] * 0.5)
        s.solve(); r3 = _state(s)
        res.append((r1, r2, r3))
    for a, b in zip(*res):
        _same_state(a, b)


def test_update_P_full_and_upper_triangle_forms_agree_bitwise():
    for B in (20, 6):
        pr = PR.random_box_qp(B, n=64, mg=48, nnz_per_row=4)
        Px1 = PR.random_box_qp(B, n=64, mg=48, nnz_per_row=4, value_seed=7000)["Px"]
        pat, Pf = _full_form(pr, Px1)
        a = _make(pr); a.update_P(Px1); a.solve()
        b = _make(pr); b.update_P(Pf, P_pattern=pat); b.solve()
        _same_state(_state(a), _state(b))


def test_update_P_with_a_changed_pattern_is_refused_and_changes_nothing():
    for B in (20, 6):
        pr = PR.random_box_qp(B, n=64, mg=48, nnz_per_row=4)
        s = _make(pr)
        diag = sp.identity(pr["n"], format="csc")
        with pytest.raises(M.MiOsqpError) as e:
            s.update_P(np.ones((B, pr["n"])), P_pattern=diag)
        assert e.value.code == 3                               # MI_OSQP_ERR_PATTERN_CHANGED
        with pytest.raises(M.MiOsqpError) as e:
            s.update_P_A(np.ones((B, pr["n"])), pr["Ax"], P_pattern=diag)
        assert e.value.code == 3
        s.solve()
        ref = _make(pr); ref.solve()
        _same_state(_state(s), _state(ref))


# ---------------------------------------------------------------- 3. update_P_A
@pytest.mark.parametrize("B", [20, 6])
def test_update_P_A_matches_an_oracle_setup_and_refactors_once(B):
    pr = PR.random_box_qp(B, n=64, mg=48, nnz_per_row=4)
    other = PR.random_box_qp(B, n=64, mg=48, nnz_per_row=4, value_seed=7000)
    s = _make(pr)
    s.refactor_time()                                          # (resets the counters)
    s.update_P_A(other["Px"], other["Ax"])
    _, _, launches, qps = s.refactor_time()
    assert (launches, qps) == (1, B)
    info = s.solve(); x = s.primal()
    P1 = _with_P(pr, other["Px"])
    for b in range(B):
        _, A1 = PR.qp_matrices(other, b)
        _compare(info, x, b, _oracle(pr, b, P=P1[b], A=A1))


# ---------------------------------------------------------------- 4. update_q with scaling and polish, warm handle
def _reduced_solution(P, q, A, l, u, act):
    """[[P, A_act'], [A_act, 0]] [x; y_act] = [-q; b_act] (unscaled), y = 0 on the inactive rows."""
    rows = np.flatnonzero(act)
    Aa = A[rows]
    K = sp.bmat([[P, Aa.T], [Aa, None]], format="csc")
    rhs = np.concatenate([-q, np.where(act[rows] < 0, l[rows], u[rows])])
    sol = spla.spsolve(K, rhs)
    return sol[:P.shape[0]]


@pytest.mark.parametrize("B", [20, 6])
def test_update_q_on_a_warm_polished_handle_solves_the_new_problem(B):
    pr = PR.random_box_qp(B, n=64, mg=48, nnz_per_row=4)
    s = _make(pr, polish=1)
    s.solve(); x0 = s.primal().copy()
    q1 = _new_q(pr, 77)
    s.update_q(q1)
    info = s.solve(); x, y = s.primal(), s.dual()
    act = s.polish_active()
    accepted = [b for b in range(B) if info[b].status_polish == 1]
    assert len(accepted) >= B // 2
    for b in accepted:
        P, A = PR.qp_matrices(pr, b)
        Pf, A = sym_from_any(P), sp.csc_matrix(A)
        xr = _reduced_solution(Pf, q1[b], A, pr["l"][b], pr["u"][b], act[b])
        assert np.max(np.abs(x[b] - xr)) <= 1e-8 * max(1.0, np.max(np.abs(xr))), b
        r = kkt_residuals(P, q1[b], A, pr["l"][b], pr["u"][b], x[b], y[b])
        assert r["prim"] <= 1e-6 and r["stat"] <= 1e-6 and r["comp"] <= 1e-6, (b, r)
        assert np.max(np.abs(x[b] - x0[b])) > 1e-3


# ---------------------------------------------------------------- 5. update_q_device
@pytest.mark.parametrize("B", [20, 6])
def test_update_q_device_equals_update_q_bitwise(B):
    import torch
    pr = PR.random_box_qp(B, n=64, mg=48, nnz_per_row=4)
    q1 = _new_q(pr, 9)
    a = _make(pr); a.solve(); a.update_q(q1); a.solve()
    b = _make(pr); b.solve()
    dq = torch.tensor(q1, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    b.update_q_device(dq)
    b.solve()
    _same_state(_state(a), _state(b))
    # a later host-path bounds update sees the new q on both
    a.update_bounds(pr["l"] * 0.5, pr["u"] * 0.5); b.update_bounds(pr["l"] * 0.5, pr["u"] * 0.5)
    a.solve(); b.solve()
    _same_state(_state(a), _state(b))


# ---------------------------------------------------------------- 6. continuous mode
def _drain(s, max_advances=400):
    for _ in range(max_advances):
        if not s.running():
            return
        s.advance(1)
        s.poll(True)
    raise AssertionError("continuous solve did not finish")


def _same_qp(ia, xa, ib, xb):
    assert (ia.status_val, ia.iter, ia.rho_updates, ia.rho, ia.obj_val, ia.pri_res) == \
           (ib.status_val, ib.iter, ib.rho_updates, ib.rho, ib.obj_val, ib.pri_res)
    assert np.array_equal(xa, xb, equal_nan=True)


def test_update_q_some_equals_the_blocking_update_bitwise():
    pr = PR.random_box_qp(8, n=64, mg=48, nnz_per_row=4)
    q1 = _new_q(pr, 13)
    ids = np.array([1, 4, 6])
    blk = _make(pr); blk.update_q(q1); ib = blk.solve(); xb = blk.primal()
    c = _make(pr)
    c.update_q_some(ids, q1[ids])
    c.solve_begin_some(ids)
    _drain(c)
    ic, xc = c.info_some(ids), c.primal_some(ids)
    for j, b in enumerate(ids):
        _same_qp(ic[j], xc[j], ib[b], xb[b])


def test_reinit_some_after_update_q_some_equilibrates_from_the_new_q():
    pr = PR.random_box_qp(8, n=64, mg=48, nnz_per_row=4)
    q1 = _new_q(pr, 17)
    ids = np.array([0, 3, 5])
    c = _make(pr)
    c.update_q_some(ids, q1[ids])
    c.reinit_some(ids, pr["Ax"][ids], pr["l"][ids], pr["u"][ids])
    c.solve_begin_some(ids)
    _drain(c)
    ic, xc = c.info_some(ids), c.primal_some(ids)
    fresh = M.BatchSolver(pr["P"], pr["Px"], q1, pr["A"], pr["Ax"], pr["l"], pr["u"])
    inf, xf = fresh.solve(), fresh.primal()
    for j, b in enumerate(ids):
        _same_qp(ic[j], xc[j], inf[b], xf[b])


# ---------------------------------------------------------------- 7. dual warm start
def test_the_exact_kkt_point_is_a_fixed_point_of_the_admm():
    B = 6
    pr = PR.random_box_qp(B, n=64, mg=48, nnz_per_row=4)
    hi = _make(pr, polish=1, eps_abs=1e-8, eps_rel=1e-8)
    hi.solve(); xs, ys = hi.primal().copy(), hi.dual().copy()
    both = _make(pr); both.warm_start_x(xs); both.warm_start_y(ys)
    ib = both.solve(); xb = both.primal()
    ct = int(both.settings.check_termination)
    for b in range(B):
        assert ib[b].exit_code == 0 and ib[b].iter == ct, (b, ib[b].exit_code, ib[b].iter)
        assert np.max(np.abs(xb[b] - xs[b])) <= 1e-6
    only_x = _make(pr); only_x.warm_start_x(xs)
    ix = only_x.solve()
    assert sum(i.iter for i in ix) > sum(i.iter for i in ib)
    # the per-QP form gives the blocking form's results
    ids = np.array([0, 2, 5])
    c = _make(pr)
    c.warm_start_x_some(ids, xs[ids]); c.warm_start_y_some(ids, ys[ids])
    c.solve_begin_some(ids)
    _drain(c)
    ic, xc = c.info_some(ids), c.primal_some(ids)
    for j, b in enumerate(ids):
        _same_qp(ic[j], xc[j], ib[b], xb[b])


# ---------------------------------------------------------------- 8. non-convex P of one QP
@pytest.mark.parametrize("B", [20, 6])
def test_an_indefinite_P_fails_only_its_own_qp(B):
    pr = PR.random_box_qp(B, n=64, mg=48, nnz_per_row=4)
    Pgood = PR.random_box_qp(B, n=64, mg=48, nnz_per_row=4, value_seed=7000)["Px"]
    Pbad = Pgood.copy(); Pbad[1] = -Pbad[1]
    bad = _make(pr); bad.update_P(Pbad); ib = bad.solve(); xb, yb = bad.primal(), bad.dual()
    good = _make(pr); good.update_P(Pgood); ig = good.solve(); xg, yg = good.primal(), good.dual()
    assert ib[1].exit_code == 9                                 # kNonConvex
    for b in range(B):
        if b == 1:
            continue
        assert (ib[b].status_val, ib[b].iter, ib[b].rho_updates, ib[b].obj_val) == (ig[b].status_val, ig[b].iter, ig[b].rho_updates, ig[b].obj_val)
        np.testing.assert_array_equal(xb[b], xg[b]); np.testing.assert_array_equal(yb[b], yg[b])


# ---------------------------------------------------------------- 9. shards
def test_multi_batch_objective_updates_equal_a_single_handle_bitwise():
    B = 7
    pr = PR.random_box_qp(B, n=96, mg=64, nnz_per_row=6)
    other = PR.random_box_qp(B, n=96, mg=64, nnz_per_row=6, value_seed=7000)
    q1 = _new_q(pr, 23)
    one = _make(pr)
    multi = M.MultiBatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], devices=(0, 0))
    for step in ("q", "P", "PA", "y"):
        for h in (one, multi):
            if step == "q":
                h.update_q(q1)
            elif step == "P":
                h.update_P(other["Px"])
            elif step == "PA":
                h.update_P_A(pr["Px"], other["Ax"])
            else:
                h.warm_start_y(np.zeros((B, pr["m"])))
        i1, i2 = one.solve(), multi.solve()
        assert [(i.status_val, i.iter, i.rho_updates) for i in i1] == [(i.status_val, i.iter, i.rho_updates) for i in i2], step
        np.testing.assert_array_equal(one.primal(), multi.primal())
        np.testing.assert_array_equal(one.dual(), multi.dual())


# ---------------------------------------------------------------- 10. the osqp++ shim
def build_shim_objective(tmp_path):
    M.lib()
    exe = str(tmp_path / "shim_objective")
    cmd = ["g++", "-std=c++17", "-O1", "-DNDEBUG", "-I", os.path.join(ROOT, "tests", "cpp", "eigen_standin"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "osqp_shim_objective.cpp"),
           "-L", os.path.join(ROOT, "osqp-solver_amd"), "-lmi_osqp", "-Wl,-rpath," + os.path.join(ROOT, "osqp-solver_amd"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run_shim_objective(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]), res.stdout


def test_shim_objective_sequence_matches_the_python_binding(tmp_path):
    out, log = run_shim_objective(build_shim_objective(tmp_path))
    assert out["init_ok"] is True, log
    assert out["status"] == ["OK", "OK", "OK"], out
    assert out["wrong_pattern"] == "INVALID_ARGUMENT" and out["wrong_length"] == "INVALID_ARGUMENT"
    P = sp.csc_matrix(np.array([[4.0, 1.0], [1.0, 2.0]])); A = sp.csc_matrix(np.array([[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]]))
    P2 = sp.csc_matrix(np.array([[5.0, 1.5], [1.5, 3.0]]))
    l = np.array([1.0, 0.0, 0.0]); u = np.array([1.0, 0.7, 0.7])
    s = M.BatchSolver(P, P.data, np.array([1.0, 1.0]), A, A.data, l, u)
    c1 = s.solve()[0]; x1 = s.primal()[0].copy()
    s.update_q(np.array([-1.0, 2.0]))
    c2 = s.solve()[0]; x2, y2 = s.primal()[0].copy(), s.dual()[0].copy()
    s.update_P(P2.data)
    s.warm_start_x(x2); s.warm_start_y(y2)
    c3 = s.solve()[0]; x3, y3 = s.primal()[0].copy(), s.dual()[0].copy()
    assert out["codes"] == [M.EXIT_NAMES[c.exit_code] for c in (c1, c2, c3)]
    assert out["iters"] == [c1.iter, c2.iter, c3.iter]
    for k, v in (("x1", x1), ("x2", x2), ("y2", y2), ("x3", x3), ("y3", y3)):
        assert np.array_equal(np.array(out[k]), v), k          # same library, same kernels: bitwise
