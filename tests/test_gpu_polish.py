"""GPU (-m gpu): solution polishing (README "Polishing").

Checkers: the closed-form / 1e-9 solutions of tests/golden/qp_fixtures.json, oracle/kkt_check.py, the oracle run to high
accuracy, and the reduced KKT system of the reported active set solved by scipy in the unscaled data."""
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


def build_shim_polish(tmp_path):
    M.lib()
    exe = str(tmp_path / "shim_polish")
    cmd = ["g++", "-std=c++17", "-O1", "-DNDEBUG", "-I", os.path.join(ROOT, "tests", "cpp", "eigen_standin"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "osqp_shim_polish.cpp"),
           "-L", os.path.join(ROOT, "osqp-solver_amd"), "-lmi_osqp", "-Wl,-rpath," + os.path.join(ROOT, "osqp-solver_amd"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run_shim_polish(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]), res.stdout


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _qp(pr, b):
    P, A = PR.qp_matrices(pr, b)
    q = np.zeros(pr["n"] if "n" in pr else A.shape[1]) if pr["q"] is None else pr["q"][b]
    return sym_from_any(P), q, sp.csc_matrix(A), pr["l"][b], pr["u"][b]


def _reduced_solution(P, q, A, l, u, act):
    """[[P, A_act'], [A_act, 0]] [x; y_act] = [-q; b_act] (unscaled), y = 0 on the inactive rows."""
    rows = np.flatnonzero(act)
    Aa = A[rows]
    K = sp.bmat([[P, Aa.T], [Aa, None]], format="csc")
    rhs = np.concatenate([-q, np.where(act[rows] < 0, l[rows], u[rows])])
    s = spla.spsolve(K, rhs)
    y = np.zeros(A.shape[0])
    y[rows] = s[P.shape[0]:]
    return s[:P.shape[0]], y


def _check_reduced_system(pr, s, info, x, y):
    """Every accepted QP: x is the reduced system's solution of the reported active set, y agrees on the active rows
    whose multiplier has the sign of their side, and the reported residuals are those of the returned (x, y)."""
    act = s.polish_active()
    accepted = [b for b in range(s.B) if info[b].status_polish == 1]
    assert accepted
    for b in accepted:
        P, q, A, l, u = _qp(pr, b)
        xr, yr = _reduced_solution(P, q, A, l, u, act[b])
        sx = max(1.0, np.max(np.abs(xr)))
        assert np.max(np.abs(x[b] - xr)) <= 1e-8 * sx, (b, np.max(np.abs(x[b] - xr)))
        keep = ((act[b] < 0) & (yr < 0)) | ((act[b] > 0) & (yr > 0))
        sy = max(1.0, np.max(np.abs(yr)))
        assert np.max(np.abs(y[b][keep] - yr[keep]), initial=0.0) <= 1e-8 * sy, b
        # residuals / objective of the returned point (unscaled rules: scaled_termination = 0).  z: at the bound of the
        # multiplier's side, else A x clipped.  (An active row whose multiplier has the wrong sign leaves the projection with
        # y = 0 and z = A x + y_red in the scaled data: its contribution to pri_res is not recoverable from x and y alone.)
        Ax = A @ x[b]
        z = np.where(y[b] < 0, l, np.where(y[b] > 0, u, np.clip(Ax, l, u)))
        pri, dua = np.max(np.abs(Ax - z), initial=0.0), np.max(np.abs(P @ x[b] + q + A.T @ y[b]))
        obj = 0.5 * x[b] @ (P @ x[b]) + q @ x[b]
        tol_p = 1e-9 * max(1.0, np.max(np.abs(Ax)))
        if np.all(keep == (act[b] != 0)):
            assert abs(info[b].pri_res - pri) <= tol_p, (b, info[b].pri_res, pri)
        else:
            assert info[b].pri_res >= pri - tol_p, (b, info[b].pri_res, pri)
        assert abs(info[b].dua_res - dua) <= 1e-9 * max(1.0, np.max(np.abs(q))), (b, info[b].dua_res, dua)
        assert abs(info[b].obj_val - obj) <= 1e-9 * max(1.0, abs(obj)), (b, info[b].obj_val, obj)
    return accepted


def test_golden_fixtures_polished(qp_fixtures):
    # (none exempted: every kOptimal fixture has a strictly complementary solution)
    for name, d in qp_fixtures.items():
        s = M.QPSolver((d["l"], sp.csc_matrix(d["A"]), d["u"]), sp.csc_matrix(d["P"]), q=d["q"], polish=1)
        code, x = s.solve()
        info = s.info()
        assert M.EXIT_NAMES[code] == d["status"], name
        if d["x"] is None:
            assert info.status_polish == 0 and np.all(np.isnan(x)), name
            continue
        assert info.status_polish == 1, name
        y = s.dual()
        assert np.max(np.abs(x - d["x"])) <= 1e-7 * max(1.0, np.max(np.abs(d["x"]))), (name, np.max(np.abs(x - d["x"])))
        assert np.max(np.abs(y - d["y"])) <= 1e-7 * max(1.0, np.max(np.abs(d["y"]))), (name, np.max(np.abs(y - d["y"])))
        r = kkt_residuals(d["P"], d["q"], d["A"], d["l"], d["u"], x, y)
        assert max(r["prim"], r["stat"], r["comp"], r["dual_sign"]) <= 1e-8, (name, r)


def _batches():
    return {"config3": PR.random_box_qp(64), "gomp": PR.gomp_batch(16, 7, 20)}


@pytest.mark.parametrize("tile", [1, 2])
def test_reduced_system_and_high_accuracy_oracle(tile, monkeypatch):
    monkeypatch.setenv("MI_OSQP_TILE", str(tile))
    for name, pr in _batches().items():
        s = _solver(pr, polish=1)
        if name == "config3":
            assert s.stats()["dense_tail_rows"] > 0
        info = s.solve()
        x, y = s.primal(), s.dual()
        st = s.last_polish_stats()
        assert st["polished"] == sum(i.status_val == 1 for i in info) and st["accepted"] == sum(i.status_polish == 1 for i in info)
        assert all(i.status_polish == 0 for i in info if i.status_val != 1)
        _check_reduced_system(pr, s, info, x, y)
        if tile != 1:
            continue
        # polish at eps 1e-3 against the oracle at eps 1e-10.  The active set guessed at 1e-3 is wrong for a part of these
        # QPs ("Polishing"): most of those are rejected and keep their ADMM solution, a few are accepted
        # because their residuals still improve on the ADMM's (upstream's acceptance rule).  Measured: config 3, 16 of 64
        # farther than 1e-6, 2 of them accepted; GOMP, 6 of 16 farther, none accepted.
        far, far_accepted = 0, 0
        for b in range(s.B):
            P, A = PR.qp_matrices(pr, b)
            o = O.OracleQPSolver(P, None if pr["q"] is None else pr["q"][b], A, pr["l"][b], pr["u"][b],
                                 eps_abs=1e-10, eps_rel=1e-10, max_iter=200000)
            st_o, xo = o.solve()
            if st_o != 1 or np.max(np.abs(x[b] - xo)) > 1e-6 * max(1.0, np.max(np.abs(xo))):
                far += 1
                far_accepted += info[b].status_polish == 1
        print(f"{name}: {far} of {s.B} QPs farther than 1e-6 from the oracle at eps 1e-10 ({far_accepted} of them accepted)")
        assert far_accepted <= 0.05 * s.B, (name, far, far_accepted)


def test_polish_moves_nothing_else():
    import torch
    for pr in (PR.random_box_qp(24, n=96, mg=64, nnz_per_row=6), PR.gomp_batch(6, 3, 12)):
        s0, s1 = _solver(pr), _solver(pr, polish=1)
        i0, i1 = s0.solve(), s1.solve()
        assert [(a.iter, a.rho_updates, a.exit_code) for a in i0] == [(a.iter, a.rho_updates, a.exit_code) for a in i1]
        assert all(a.status_polish == 0 for a in i0) and s0.last_polish_stats()["polished"] == 0
        x0, y0, x1, y1 = s0.primal(), s0.dual(), s1.primal(), s1.dual()
        for b, a in enumerate(i1):
            if a.status_polish != 1:
                assert np.array_equal(x0[b], x1[b], equal_nan=True) and np.array_equal(y0[b], y1[b], equal_nan=True), b
        # the ADMM factor is untouched
        N = s0.n + s0.m
        rhs = torch.tensor(np.random.default_rng(5).standard_normal((s0.B, N)), device="cuda")
        o0, o1 = torch.empty_like(rhs), torch.empty_like(rhs)
        s0.kkt_solve_device(rhs, o0); s1.kkt_solve_device(rhs, o1)
        assert torch.equal(o0, o1)
        # the polished point is the next warm start: the next solve ends at its first termination check
        i2 = s1.solve()
        for b, a in enumerate(i1):
            if a.status_polish == 1:
                assert i2[b].iter == s1.settings.check_termination and i2[b].exit_code == 0, (b, i2[b].iter)


@pytest.mark.parametrize("groups", ["0", "16"])
def test_single_large_qp_dataflow_form(groups, monkeypatch):
    """The global-vector form (MI_OSQP_GROUPS workgroups share the QP; 0 = one workgroup).  A small random QP polishes
    (checked against scipy); the 30 x 30 grid QP at eps 1e-3 guesses a rank-deficient active set (784 rows, the
    unregularised reduced matrix is singular): polishing must fail there and leave the ADMM solution as it is."""
    monkeypatch.setenv("MI_OSQP_GLOBAL_XS", "1")
    monkeypatch.setenv("MI_OSQP_GROUPS", groups)
    pr = PR.random_box_qp(1, n=96, mg=64, nnz_per_row=6)
    s = _solver(pr, polish=1)
    info = s.solve()
    assert info[0].status_val == 1 and info[0].status_polish == 1
    if groups != "0":
        assert s.stats()["solve_groups"] == int(groups)
    _check_reduced_system(pr, s, info, s.primal(), s.dual())
    pr = PR.grid_qp(30)
    s0, s1 = _solver(pr), _solver(pr, polish=1)
    i0, i1 = s0.solve(), s1.solve()
    assert i1[0].status_val == 1 and i1[0].status_polish == -1 and i0[0].status_polish == 0
    assert np.array_equal(s0.primal(), s1.primal()) and np.array_equal(s0.dual(), s1.dual())
    assert (i1[0].pri_res, i1[0].dua_res, i1[0].obj_val) == (i0[0].pri_res, i0[0].dua_res, i0[0].obj_val)


def test_shards_device_io_and_continuous_mode():
    import torch
    pr = PR.random_box_qp(16, n=96, mg=64, nnz_per_row=6)
    one = _solver(pr, polish=1)
    i1 = one.solve()
    x1 = one.primal()
    assert sum(a.status_polish == 1 for a in i1) > 0
    mb = M.MultiBatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], devices=(0, 0), polish=1)
    im = mb.solve()
    assert [a.status_polish for a in im] == [a.status_polish for a in i1]
    assert np.allclose(mb.primal(), x1, rtol=0, atol=1e-12)
    mb.solve_async()
    im2 = mb.wait()
    assert all(a.status_polish in (1, -1) for a in im2 if a.status_val == 1)
    mb.close()
    dev = _solver(pr, polish=1)
    xd = torch.empty((dev.B, dev.n), dtype=torch.float64, device="cuda")
    dev.solve_device(xd)
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), dev.primal()) and np.array_equal(dev.primal(), x1)
    with pytest.raises(M.MiOsqpError) as e:
        dev.solve_begin_some([0, 1])
    assert e.value.code == 2


def test_shim_polish_on_the_gpu(tmp_path):
    out, log = run_shim_polish(build_shim_polish(tmp_path))
    assert out["init_ok"] is True and out["code"] == "kOptimal", log
    P = sp.csc_matrix(np.array([[4.0, 1.0], [1.0, 2.0]])); A = sp.csc_matrix(np.array([[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]]))
    s = M.QPSolver((np.array([1.0, 0.0, 0.0]), A, np.array([1.0, 0.7, 0.7])), P, polish=1)
    code, x = s.solve()
    assert s.info().status_polish == 1 and out["iter"] == s.info().iter
    assert np.array_equal(np.array(out["x"]), x)
