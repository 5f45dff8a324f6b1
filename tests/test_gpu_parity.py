"""GPU (-m gpu): parity of the HIP path, called through the C-ABI, against the
oracle on identical (P, q, A, l, u) and identical settings.

Tolerance (BASELINE.json north_star): primal solutions within 1e-6 (inf-norm) at
the same ADMM tolerance; we additionally require the same exit code and the same
iteration count, which holds because both sides run the same algorithm with the
same deterministic rho schedule (differences are fp64 round-off, ~1e-12)."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_solver_amd as M
from oracle import oracle as O
from oracle.kkt_check import kkt_residuals, sym_from_any
from osqp_solver_amd import problems as PR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_X = 1e-6
ST2EXIT = {1: 0, -3: 1, -4: 2, 2: 3, 3: 4, 4: 5, -2: 6, -7: 9, -10: 10}


def _oracle_batch(pr, idx, **settings):
    res = []
    for b in idx:
        P, A = PR.qp_matrices(pr, b)
        o = O.OracleQPSolver(P, None if pr["q"] is None else pr["q"][b], A, pr["l"][b], pr["u"][b], **settings)
        st, x = o.solve()
        res.append((st, x, o.info(), o))
    return res


def _compare(info, x, ref, idx):
    for k, b in enumerate(idx):
        st, xo, io, _ = ref[k]
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


@pytest.mark.parametrize("tile", [1, 2, 4])
@pytest.mark.parametrize("eps", [1e-3, 1e-8])
def test_config3_small_batch_matches_oracle(tile, eps, monkeypatch):
    monkeypatch.setenv("MI_OSQP_TILE", str(tile))
    B = 10                                        # not a multiple of 4: ragged last tile
    pr = PR.random_box_qp(B, n=96, mg=64, nnz_per_row=6)
    kw = dict(eps_abs=eps, eps_rel=eps)
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)
    assert s.stats()["tile"] == tile
    info = s.solve()
    _compare(info, s.primal(), _oracle_batch(pr, range(B), **kw), range(B))
    # duals too
    y = s.dual()
    for b, (_, _, _, o) in enumerate(_oracle_batch(pr, range(2), **kw)):
        assert np.max(np.abs(y[b] - o.y)) <= 1e-5


def test_config3_full_size_pattern_small_batch():
    pr = PR.random_box_qp(6)                       # n=512, m=1024 like the headline config
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    info = s.solve()
    _compare(info, s.primal(), _oracle_batch(pr, range(6)), range(6))


def test_golden_fixtures_through_c_abi(qp_fixtures):
    for name, d in qp_fixtures.items():
        s = M.QPSolver((d["l"], sp.csc_matrix(d["A"]), d["u"]), sp.csc_matrix(d["P"]), q=d["q"],
                       eps_abs=1e-9, eps_rel=1e-9, max_iter=200000)
        code, x = s.solve()
        assert M.EXIT_NAMES[code] == d["status"], name
        if d["x"] is not None:
            np.testing.assert_allclose(x, d["x"], atol=2e-6, err_msg=name)
            np.testing.assert_allclose(s.dual(), d["y"], atol=2e-5, err_msg=name)
        else:
            assert np.all(np.isnan(x)), name


def test_exit_codes_and_nan_solution(qp_fixtures):
    for name in ("primal_infeasible", "dual_infeasible"):
        d = qp_fixtures[name]
        s = M.QPSolver((d["l"], sp.csc_matrix(d["A"]), d["u"]), sp.csc_matrix(d["P"]), q=d["q"])
        o = O.OracleQPSolver(d["P"], d["q"], d["A"], d["l"], d["u"])
        st, _ = o.solve()
        code, x = s.solve()
        assert code == ST2EXIT[st] and M.EXIT_NAMES[code] == d["status"]
        assert s.info().iter == o.info().iter and np.all(np.isnan(x))
    d = qp_fixtures["generic_30x40"]
    kw = dict(eps_abs=1e-12, eps_rel=1e-12, max_iter=30)
    s = M.QPSolver((d["l"], sp.csc_matrix(d["A"]), d["u"]), sp.csc_matrix(d["P"]), q=d["q"], **kw)
    o = O.OracleQPSolver(d["P"], d["q"], d["A"], d["l"], d["u"], **kw)
    st, xo = o.solve()
    code, x = s.solve()
    assert code == ST2EXIT[st] and s.info().iter == 30 and np.max(np.abs(x - xo)) <= TOL_X


def test_gomp_config2_qpsolver_call_sequence():
    """BASELINE config 2 through the reference's call pattern
    ([REF] src/gomp-solver.h:61-88): ctor, setWarmStart, solve, update, solve."""
    D, W = 6, 50
    P, (l, A, u), warm = PR.gomp_qp(D, W, np.zeros(D), np.array([np.pi, 0, 0, 0, 0, 0]))
    s = M.QPSolver((l, A, u), P)
    o = O.OracleQPSolver(P, None, A, l, u)
    s.setWarmStart(warm); o.set_warm_start(warm)
    code, x = s.solve(); st, xo = o.solve()
    assert code == ST2EXIT[st] and s.info().iter == o.info().iter
    assert np.max(np.abs(x - xo)) <= TOL_X
    # SQP-style update: same pattern, perturbed values and tightened bounds, warm-started re-solve
    A2 = A.copy(); A2.data = A2.data * (1.0 + 0.01 * np.cos(np.arange(A2.nnz)))
    l2 = np.where(np.abs(l) < 1e29, l * 0.95, l); u2 = np.where(np.abs(u) < 1e29, u * 0.95, u)
    s.update((l2, A2, u2)); o.update(l2, A2, u2)
    code, x = s.solve(); st, xo = o.solve()
    assert code == ST2EXIT[st] and s.info().iter == o.info().iter
    assert np.max(np.abs(x - xo)) <= TOL_X
    with pytest.raises(ValueError):                # pattern change -> std::invalid_argument in the reference
        A3 = A.tolil(); A3[0, 5] = 1.0
        s.update((l, A3.tocsc(), u))
    with pytest.raises(ValueError):
        s.update((u + 1.0, A, l))


def test_gomp_batch_config4_shape_small():
    pr = PR.gomp_batch(5, 7, 20)
    s = M.BatchSolver(pr["P"], pr["Px"], None, pr["A"], pr["Ax"], pr["l"], pr["u"])
    s.warm_start_x(pr["warm"])
    info = s.solve()
    ref = []
    for b in range(5):
        P, A = PR.qp_matrices(pr, b)
        o = O.OracleQPSolver(P, None, A, pr["l"][b], pr["u"][b])
        o.set_warm_start(pr["warm"][b])
        st, x = o.solve()
        ref.append((st, x, o.info(), o))
    _compare(info, s.primal(), ref, range(5))


def test_warm_second_solve_and_reset_are_reproducible():
    pr = PR.random_box_qp(8, n=64, mg=48, nnz_per_row=4)
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    i1 = s.solve(); x1 = s.primal()
    i2 = s.solve(); x2 = s.primal()                # warm: continues from x, z, y, rho (osqp warm_start=1)
    ref = _oracle_batch(pr, range(8))
    for b, (_, _, _, o) in enumerate(ref):
        st, xo = o.solve()
        assert i2[b].iter == o.info().iter and np.max(np.abs(x2[b] - xo)) <= TOL_X
    s.reset()
    i3 = s.solve(); x3 = s.primal()
    assert [i.iter for i in i3] == [i.iter for i in i1]
    np.testing.assert_array_equal(x1, x3)           # deterministic reductions: bitwise repeatable


def test_ops_spmv_and_kkt_solve():
    import torch
    B = 9
    pr = PR.random_box_qp(B, n=96, mg=64, nnz_per_row=6)
    n, m = pr["n"], pr["m"]
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], scaling=0)
    rng = np.random.default_rng(2)
    x = rng.standard_normal((B, n)); y = rng.standard_normal((B, m))
    tx, ty = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
    Px = torch.empty(B, n, dtype=torch.float64, device="cuda"); Aty = torch.empty_like(Px)
    Ax = torch.empty(B, m, dtype=torch.float64, device="cuda")
    s.spmv_device(tx, ty, Px, Aty, Ax)
    for b in range(B):
        P, A = PR.qp_matrices(pr, b)
        Pf = sym_from_any(P)
        np.testing.assert_allclose(Px[b].cpu().numpy(), Pf @ x[b], rtol=0, atol=1e-12)
        np.testing.assert_allclose(Aty[b].cpu().numpy(), A.T @ y[b], rtol=0, atol=1e-12)
        np.testing.assert_allclose(Ax[b].cpu().numpy(), A @ x[b], rtol=0, atol=1e-12)
    # KKT solve with scaling on, against the oracle's independent factor
    s2 = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    rhs = rng.standard_normal((B, n + m))
    trhs = torch.tensor(rhs, device="cuda"); sol = torch.empty_like(trhs)
    s2.kkt_solve_device(trhs, sol)
    for b in range(B):
        P, A = PR.qp_matrices(pr, b)
        o = O.OracleQPSolver(P, pr["q"][b], A, pr["l"][b], pr["u"][b])
        ref = o.kkt_solve(rhs[b])
        assert np.max(np.abs(sol[b].cpu().numpy() - ref)) <= 1e-9 * np.max(np.abs(ref))


def test_device_resident_io_matches_host_io():
    import torch
    B = 12
    pr = PR.random_box_qp(B, n=64, mg=48, nnz_per_row=4)
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    l2, u2 = pr["l"] * 0.8, pr["u"] * 0.7
    s.update_bounds(l2, u2)
    ih = s.solve(); xh = s.primal()
    s2 = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    s2.update_bounds_device(torch.tensor(l2, device="cuda"), torch.tensor(u2, device="cuda"))
    xd = torch.empty(B, pr["n"], dtype=torch.float64, device="cuda")
    st = torch.empty(B, dtype=torch.int32, device="cuda"); it = torch.empty_like(st)
    s2.solve_device(xd, st, it)
    np.testing.assert_array_equal(xd.cpu().numpy(), xh)
    assert it.cpu().tolist() == [i.iter for i in ih] and st.cpu().tolist() == [i.status_val for i in ih]
    # and the oracle on the updated bounds
    prn = dict(pr, l=l2, u=u2)
    _compare(ih, xh, _oracle_batch(prn, range(4)), range(4))
    with pytest.raises(M.MiOsqpError):
        s2.update_bounds_device(torch.tensor(u2 + 1, device="cuda"), torch.tensor(l2, device="cuda"))


def test_update_of_values_and_bounds_in_one_call_equals_the_two_calls():
    """mi_osqp_batch_update_A_bounds (QPSolver::update, [REF] src/osqp-wrapper.h:33-43) = update_A then update_bounds with one
    refactorisation: bitwise the same iterates afterwards, also when the new bounds change row types (an equality, a free row)."""
    B = 6
    pr = PR.random_box_qp(B, n=64, mg=48, nnz_per_row=4)
    rng = np.random.default_rng(11)
    Ax2 = pr["Ax"] * (1.0 + 0.1 * rng.standard_normal(pr["Ax"].shape))
    l2, u2 = pr["l"] * 0.9, pr["u"] * 1.1
    l2[:, 3] = u2[:, 3] = 0.05                     # becomes an equality
    l2[:, 7] = -1e30; u2[:, 7] = 1e30              # becomes a free row
    sa = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    sb = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    sa.solve(); sb.solve()                         # (rho has adapted: the update path starts from a used handle)
    sa.update_A(Ax2); sa.update_bounds(l2, u2)
    sb.update_A_bounds(Ax2, l2, u2)
    ia, ib = sa.solve(), sb.solve()
    assert [i.iter for i in ia] == [i.iter for i in ib] and [i.exit_code for i in ia] == [i.exit_code for i in ib]
    np.testing.assert_array_equal(sa.primal(), sb.primal())
    np.testing.assert_array_equal(sa.dual(), sb.dual())
    xb = sb.primal().copy()
    with pytest.raises(M.MiOsqpError):
        sb.update_A_bounds(Ax2, u2 + 1.0, l2)      # l > u: refused, nothing changed
    sb.reset(); sa.reset()
    assert [i.iter for i in sa.solve()] == [i.iter for i in sb.solve()]
    # and the oracle taken through the same two updates
    for b in range(2):
        P, A = PR.qp_matrices(pr, b)
        o = O.OracleQPSolver(P, pr["q"][b], A, pr["l"][b], pr["u"][b]); o.solve()
        A2 = A.copy(); A2.data = Ax2[b].copy()
        o.update(l2[b], A2, u2[b])
        st, xo = o.solve()
        assert ib[b].iter == o.info().iter and np.max(np.abs(xb[b] - xo)) <= TOL_X


@pytest.mark.parametrize("tile", [1, 2])
def test_ruiz_on_the_device_equals_the_host_equilibration_bitwise(tile, monkeypatch):
    """Row E2 - at setup and after new A values - runs on the device (ruiz_kernel: maxima by atomics, separate multiplications,
    one sum in index order); MI_OSQP_HOST_RUIZ=1 keeps the host path (scale_qp) - same iterates bit for bit, with and without new
    bounds, scaling on and off, GOMP pattern (many all-zero rows with infinite bounds) and random pattern."""
    monkeypatch.setenv("MI_OSQP_TILE", str(tile))
    rng = np.random.default_rng(21)
    cases = [(PR.random_box_qp(5, n=64, mg=48, nnz_per_row=4), {}), (PR.random_box_qp(3, n=64, mg=48, nnz_per_row=4), dict(scaling=0)),
             (PR.gomp_batch(4, 3, 12), {})]
    for pr, kw in cases:
        Ax2 = pr["Ax"] * (1.0 + 0.2 * rng.standard_normal(pr["Ax"].shape))
        l2, u2 = pr["l"] - 0.05 * np.abs(pr["l"]), pr["u"] + 0.05 * np.abs(pr["u"])
        res = []
        for host in (False, True):
            monkeypatch.delenv("MI_OSQP_DEVICE_RUIZ" if host else "MI_OSQP_HOST_RUIZ", raising=False)
            monkeypatch.setenv("MI_OSQP_HOST_RUIZ" if host else "MI_OSQP_DEVICE_RUIZ", "1")      # (small batches default to the host)
            s = M.BatchSolver(pr["P"], pr["Px"], pr.get("q"), pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)
            i0 = s.solve(); x0 = s.primal().copy()                # (the setup itself equilibrates on the device / on the host)
            s.update_A_bounds(Ax2, l2, u2)
            i1 = s.solve(); x1, y1 = s.primal().copy(), s.dual().copy()
            s.update_A(pr["Ax"])                                   # values back, bounds kept
            i2 = s.solve(); x2 = s.primal().copy()
            s.update_bounds(pr["l"], pr["u"])                      # (host mirrors are fetched from the device if a row changes type)
            i3 = s.solve(); x3 = s.primal().copy()
            res.append(([i.iter for i in i1], x1, y1, [i.iter for i in i2], x2, [i.iter for i in i3], x3, [i.iter for i in i0], x0))
        dev, hst = res
        assert dev[0] == hst[0] and dev[3] == hst[3] and dev[5] == hst[5] and dev[7] == hst[7]
        for k in (1, 2, 4, 6, 8): np.testing.assert_array_equal(dev[k], hst[k])


def test_headline_config_properties_full_size():
    """BASELINE config 3 at full size (B=1024, n=512, m=1024): size-independent
    properties for every QP + oracle parity on a sample."""
    B = 1024
    pr = PR.random_box_qp(B)
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    info = s.solve()
    x, y = s.primal(), s.dual()
    assert all(i.status_val == 1 for i in info)
    for b in range(B):
        P, A = PR.qp_matrices(pr, b)
        Pf = sym_from_any(P)
        Ax = A @ x[b]
        viol = max(np.max(pr["l"][b] - Ax), np.max(Ax - pr["u"][b]), 0.0)
        # ||z - Ax|| >= bound violation, and termination enforced pri_res < eps_prim
        assert viol <= info[b].pri_res + 1e-12
        assert info[b].pri_res <= 1e-3 + 1e-3 * max(np.max(np.abs(Ax)), 1.0) * 2
        Pxv, Aty = Pf @ x[b], A.T @ y[b]
        dres = np.max(np.abs(Pxv + pr["q"][b] + Aty))
        assert abs(dres - info[b].dua_res) <= 1e-9 * (1 + dres)         # reported residual is the true one
        assert dres <= 1e-3 + 1e-3 * max(np.max(np.abs(Pxv)), np.max(np.abs(Aty)), np.max(np.abs(pr["q"][b])))
        assert info[b].iter % 25 == 0 and 25 <= info[b].iter <= 4000
    sample = [0, 1, 2, 3, 511, 1023]
    _compare(info, x, _oracle_batch(pr, sample), sample)
    st = s.stats()
    assert st["tile"] in (1, 2, 4) and st["n_tiles"] * st["tile"] == 1024


def test_cpp_facade_example_runs(tmp_path):
    exe = tmp_path / "solver_example"
    libdir = os.path.join(ROOT, "osqp-solver_amd")
    cmd = ["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "solver_example.cpp"),
           "-o", str(exe), "-L" + libdir, "-lmi_osqp", "-Wl,-rpath," + libdir]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "3, 3, 2, 3, 2, 2" and "STATUS: OK" in lines[1]
    assert lines[2] == "kOptimal" and "update refused" in lines[-1]
    x = [float(v) for v in lines[3].split()[2:4]]
    # q = 0: minimise 1/2 x'Px on x0+x1=1, 0<=x<=0.7 -> x = (0.3, 0.7) by the same active set
    P = np.array([[4.0, 1], [1, 2]]); A = np.array([[1.0, 1], [1, 0], [0, 1]])
    o = O.OracleQPSolver(P, None, A, [1, 0, 0], [1, 0.7, 0.7]); o.set_warm_start([0.5, 0.5])
    _, xo = o.solve()
    assert np.max(np.abs(np.array(x) - xo)) <= 2e-6


@pytest.mark.parametrize("tile", [1, 4])
def test_device_refactor_matches_host_factor(tile, monkeypatch):
    """Rows E5 / E13 on the device: the batched block LDL' (used at setup and for every rho / A update) is checked
    through the KKT-solve op against the oracle's independent factor, after setup and again after an explicit
    refactorisation (same KKT, same rho).  The host left-looking factor it replaced lives on as the reference of
    the CPU tests (tests/test_host_schedule.py)."""
    import torch
    monkeypatch.setenv("MI_OSQP_TILE", str(tile))
    for pr in (PR.random_box_qp(6, n=96, mg=64, nnz_per_row=6), PR.gomp_batch(3, 4, 12), PR.random_box_qp(2)):
        B, n, m = pr["Ax"].shape[0], pr["n"], pr["m"]
        s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
        rhs = np.random.default_rng(4).standard_normal((B, n + m))
        trhs = torch.tensor(rhs, device="cuda"); s0 = torch.empty_like(trhs); s1 = torch.empty_like(trhs)
        s.kkt_solve_device(trhs, s0)
        s.refactor_device()
        s.kkt_solve_device(trhs, s1)
        for b in range(B):
            P, A = PR.qp_matrices(pr, b)
            o = O.OracleQPSolver(P, None if pr["q"] is None else pr["q"][b], A, pr["l"][b], pr["u"][b])
            ref = o.kkt_solve(rhs[b])
            sc = np.max(np.abs(ref))
            assert np.max(np.abs(s0[b].cpu().numpy() - ref)) <= 1e-7 * sc
            assert np.max(np.abs(s1[b].cpu().numpy() - ref)) <= 1e-7 * sc
        # and a solve after the device refactor still matches the oracle
        info = s.solve()
        _compare(info, s.primal(), _oracle_batch(pr, range(B)), range(B))


def test_four_qps_per_tile_give_the_results_of_the_default_tiling(monkeypatch):
    """MI_OSQP_TILE=4 packs four QPs into every tile: the same iteration counts and the same solution up to round-off as
    the default tiling, and a tile-4 solver - its solve, a bounds update and the solve after it - is reproducible."""
    pr = PR.random_box_qp(24, n=96, mg=64, nnz_per_row=6)
    def run():
        s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
        i1 = s.solve(); x1 = s.primal().copy(); y1 = s.dual().copy()
        s.update_bounds(pr["l"] * 0.9, pr["u"] * 0.9)
        i2 = s.solve(); x2 = s.primal().copy()
        return [i.iter for i in i1], x1, y1, [i.iter for i in i2], x2, s.last_solve_stats()
    a = run()
    monkeypatch.setenv("MI_OSQP_TILE", "4")
    b = run()
    c = run()
    assert b[0] == c[0] and b[3] == c[3]
    for k in (1, 2, 4):
        assert np.max(np.abs(b[k] - c[k])) <= 1e-12
    assert a[0] == b[0] and np.max(np.abs(a[1] - b[1])) <= 1e-9      # default tiling vs tile 4: same algorithm, round-off only


def test_config4_full_size_gomp_batch():
    """BASELINE config 4: 256 GOMP 7-DOF trajectories, 100 waypoints (n=1400, m=4872,
    N=6272), warm-started like GOMPSolver::run; every QP optimal + sampled oracle parity."""
    B = 256
    pr = PR.gomp_batch(B, 7, 100)
    s = M.BatchSolver(pr["P"], pr["Px"], None, pr["A"], pr["Ax"], pr["l"], pr["u"])
    s.warm_start_x(pr["warm"])
    info = s.solve()
    x = s.primal()
    assert all(i.status_val == 1 for i in info)
    sample = [0, 1, 100, 255]
    ref = []
    for b in sample:
        P, A = PR.qp_matrices(pr, b)
        o = O.OracleQPSolver(P, None, A, pr["l"][b], pr["u"][b])
        o.set_warm_start(pr["warm"][b])
        st, xo = o.solve()
        ref.append((st, xo, o.info(), o))
    _compare(info, x, ref, sample)
    # start / goal pinned ([REF] src/gomp-solver.h:130-133): check on the returned trajectories
    D, W = 7, 100
    rng0 = np.random.default_rng(2000)
    start0, end0 = rng0.uniform(-np.pi, np.pi, D), rng0.uniform(-np.pi, np.pi, D)
    assert np.max(np.abs(x[0][:D] - start0)) < 5e-3 and np.max(np.abs(x[0][(W - 3) * D:(W - 2) * D] - end0)) < 5e-3


def test_config5_style_structured_sparse_qp():
    """BASELINE config 5 (single large sparse QP, deep level-set solve) at the largest size the
    LDS-resident design takes: 64x64 grid, n=4096, m=12160, N=16256 (the literal size runs in
    test_config5_literal_size_solves through the wide-index / global-vector variant)."""
    pr = PR.grid_qp(64)
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    st = s.stats()
    assert st["N"] == 16256 and st["tile"] == 1
    info = s.solve()
    _compare(info, s.primal(), _oracle_batch(pr, [0]), [0])
    r = kkt_residuals(*PR.qp_matrices(pr, 0)[:1], pr["q"][0], PR.qp_matrices(pr, 0)[1], pr["l"][0], pr["u"][0], s.primal()[0], s.dual()[0])
    assert r["prim"] < 5e-3 and r["stat"] < 5e-2


def test_wide_index_words_beyond_the_16_bit_range():
    """n + m = 89 700: the step streams carry 32-bit gather / row indices (Schedule::idxw64), the solve vector
    lives in global memory, one workgroup serves the QP.  Same checks as everywhere: oracle parity."""
    pr = PR.grid_qp(150)
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    st = s.stats()
    assert st["N"] == 89700 and st["tile"] == 1
    info = s.solve()
    # the KKT-solve op on the same handle (current factor, after the rho update of the solve) against the oracle's
    import torch
    ref = _oracle_batch(pr, [0])
    _compare(info, s.primal(), ref, [0])
    rhs = np.random.default_rng(1).standard_normal((1, st["N"]))
    d_rhs = torch.tensor(rhs, device="cuda"); d_sol = torch.empty_like(d_rhs)
    s.kkt_solve_device(d_rhs, d_sol)
    ko = ref[0][3].kkt_solve(rhs[0])
    assert np.max(np.abs(d_sol.cpu().numpy()[0] - ko)) <= 1e-9 * np.max(np.abs(ko))


@pytest.mark.parametrize("shape", ["0", "1:64", "3:192", "16:512", "256:128"])
def test_single_large_qp_group_shapes_agree(shape, monkeypatch):
    """One QP with a global solve vector runs the dataflow form of the sweeps (no barrier inside a sweep, consumers poll
    for the entries) on MI_OSQP_GROUPS workgroups of MI_OSQP_GROUP_THREADS threads; 0 = the barrier form in one workgroup.
    Whatever the shape: oracle parity (same iteration count, x to 1e-6) and the KKT-solve op against the oracle's."""
    import torch
    monkeypatch.setenv("MI_OSQP_GROUPS", shape.split(":")[0])
    if ":" in shape: monkeypatch.setenv("MI_OSQP_GROUP_THREADS", shape.split(":")[1])
    pr = PR.grid_qp(90)
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    st = s.stats()
    assert st["N"] == 8100 + 8100 + 2 * 90 * 89 and st["tile"] == 1
    info = s.solve()
    ref = _oracle_batch(pr, [0])
    _compare(info, s.primal(), ref, [0])
    x1 = s.primal().copy()
    rhs = np.random.default_rng(2).standard_normal((1, st["N"]))
    d_rhs = torch.tensor(rhs, device="cuda"); d_sol = torch.empty_like(d_rhs)
    for _ in range(3):                          # (the vector is re-armed by every call)
        s.kkt_solve_device(d_rhs, d_sol)
        ko = ref[0][3].kkt_solve(rhs[0])
        assert np.max(np.abs(d_sol.cpu().numpy()[0] - ko)) <= 1e-9 * np.max(np.abs(ko))
    # a second solve on the same handle (warm: continues from the first solution) and a fresh one after reset()
    info2 = s.solve()
    assert info2[0].exit_code == 0 and info2[0].iter <= info[0].iter
    s.reset()
    info3 = s.solve()
    assert info3[0].iter == info[0].iter and np.array_equal(s.primal(), x1)      # (no timing-dependent arithmetic: bitwise)


def test_dataflow_form_on_a_small_qp_with_mostly_idle_waves(monkeypatch):
    """A small QP forced into the global-vector mode: 256 waves for a 160-row factor, most streams empty."""
    monkeypatch.setenv("MI_OSQP_GLOBAL_XS", "1")
    pr = PR.random_box_qp(1, n=96, mg=64, nnz_per_row=6)
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    info = s.solve()
    _compare(info, s.primal(), _oracle_batch(pr, [0]), [0])


def test_single_large_qp_infeasible_and_rho_updates_on_the_grid(monkeypatch):
    """The exit paths of the grid-wide check_kernel (dataflow handles): a primal infeasible QP (certificate from the
    reductions over all workgroups) and a solve with several rho updates (factor_kernel on several workgroups inside the
    solve), both against the oracle: same exit code, same iteration count."""
    monkeypatch.setenv("MI_OSQP_GLOBAL_XS", "1")        # a 40 x 40 grid through the single-large-QP path
    pr = PR.grid_qp(40)
    n = pr["n"]
    l, u = pr["l"].copy(), pr["u"].copy()
    # x0 in [1, 2], x1 in [-2, -1], but x1 - x0 in [0.5, 1] (row n of A = first difference row): no such point
    l[0, 0], u[0, 0] = 1.0, 2.0
    l[0, 1], u[0, 1] = -2.0, -1.0
    l[0, n], u[0, n] = 0.5, 1.0
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], l, u)
    info = s.solve()
    P, A = PR.qp_matrices(pr, 0)
    o = O.OracleQPSolver(P, pr["q"][0], A, l[0], u[0])
    sto, _ = o.solve()
    assert ST2EXIT[sto] == info[0].exit_code == M.EXIT_NAMES.index("kPrimalInfeasible") and info[0].iter == o.info().iter
    assert np.all(np.isnan(s.primal()[0]))
    # tight tolerances on the feasible problem: hundreds of iterations, rho adapts more than once
    kw = dict(eps_abs=1e-7, eps_rel=1e-7)
    s2 = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)
    i2 = s2.solve()
    ref = _oracle_batch(pr, [0], **kw)
    _compare(i2, s2.primal(), ref, [0])
    assert i2[0].rho_updates >= 1 and i2[0].rho_updates == ref[0][2].rho_updates


def test_refactorisation_shared_by_workgroup_groups_is_bitwise_the_single_workgroup_one(monkeypatch):
    """Short work lists share each QP among several workgroups (factor_kernel, barriers of the group between the phases of
    a level): same tasks, same arithmetic - bitwise the results of MI_OSQP_FACTOR_GROUPS=1."""
    pr = PR.random_box_qp(1024)
    for k in ("Px", "Ax", "q", "l", "u"): pr[k] = pr[k][:5]
    def run():
        s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
        info = s.solve()
        return [i.iter for i in info], [i.rho_updates for i in info], s.primal().copy(), s.dual().copy()
    ita, rua, xa, ya = run()
    monkeypatch.setenv("MI_OSQP_FACTOR_GROUPS", "1")
    itb, rub, xb, yb = run()
    assert ita == itb and rua == rub and max(rua) >= 1
    np.testing.assert_array_equal(xa, xb); np.testing.assert_array_equal(ya, yb)


def test_config5_literal_size_solves():
    """BASELINE config 5 at its literal size: n = 99 856, m = 298 936 (316 x 316 grid), N = 398 792, nnz(L) = 3.3 M.
    The oracle needs minutes here, so the check is size-independent: OSQP's own termination inequalities and the
    KKT conditions of the returned point, recomputed in numpy."""
    pr = PR.grid_qp(316)
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    st = s.stats()
    assert st["n"] == 99856 and st["m"] == 298936 and st["tile"] == 1
    info = s.solve()[0]
    assert info.exit_code == 0 and info.iter % 25 == 0
    x, y = s.primal()[0], s.dual()[0]
    P, A = PR.qp_matrices(pr, 0)
    Pf = sym_from_any(P)
    Ax = A @ x
    z = np.clip(Ax, pr["l"][0], pr["u"][0])
    pri = np.max(np.abs(Ax - z))
    dua = np.max(np.abs(Pf @ x + pr["q"][0] + A.T @ y))
    eps_pri = 1e-3 + 1e-3 * max(np.max(np.abs(Ax)), np.max(np.abs(z)))
    eps_dua = 1e-3 + 1e-3 * max(np.max(np.abs(Pf @ x)), np.max(np.abs(A.T @ y)), np.max(np.abs(pr["q"][0])))
    assert pri <= 2 * eps_pri and dua <= 2 * eps_dua, (pri, eps_pri, dua, eps_dua)
    assert abs(info.pri_res - pri) <= 1e-6 + 1e-2 * pri or info.pri_res <= eps_pri
    r = kkt_residuals(P, pr["q"][0], A, pr["l"][0], pr["u"][0], x, y)
    assert r["prim"] < 5e-3 and r["stat"] < 5e-2 and r["dual_sign"] < 1e-9
    # oracle parity at the literal size: the oracle factors in the product's elimination order (its own exact minimum degree
    # would take minutes here; the ordering changes round-off only) - same exit code, iteration count, rho updates, x to 1e-6
    o = O.OracleQPSolver(P, pr["q"][0], A, pr["l"][0], pr["u"][0], kkt_perm=s.ordering())
    sto, xo = o.solve()
    assert ST2EXIT[sto] == info.exit_code and o.info().iter == info.iter and o.info().rho_updates == info.rho_updates
    assert np.max(np.abs(x - xo)) <= TOL_X


def test_global_solve_vector_mode_small(monkeypatch):
    """Same kernels with the solve vector in a per-tile global buffer (used when N*8 B exceeds LDS)."""
    monkeypatch.setenv("MI_OSQP_GLOBAL_XS", "1")
    pr = PR.random_box_qp(5, n=96, mg=64, nnz_per_row=6)
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    info = s.solve()
    _compare(info, s.primal(), _oracle_batch(pr, range(5)), range(5))
    pr = PR.gomp_batch(2, 4, 12)
    s = M.BatchSolver(pr["P"], pr["Px"], None, pr["A"], pr["Ax"], pr["l"], pr["u"])
    s.warm_start_x(pr["warm"])
    info = s.solve()
    ref = []
    for b in range(2):
        P, A = PR.qp_matrices(pr, b)
        o = O.OracleQPSolver(P, None, A, pr["l"][b], pr["u"][b]); o.set_warm_start(pr["warm"][b])
        st, x = o.solve(); ref.append((st, x, o.info(), o))
    _compare(info, s.primal(), ref, range(2))


def test_reference_example_horizon_802_waypoints():
    """The reference's own example size ([REF] examples/solver-example.cpp:12-16: D=6, W=802 ->
    n=9624, m=33660, N=43284) does not fit LDS: it runs in the global-solve-vector mode."""
    D, W = 6, 802
    P, (l, A, u), warm = PR.gomp_qp(D, W, np.zeros(D), np.array([np.pi, 0, 0, 0, 0, 0]))
    assert A.shape == (33660, 9624)
    s = M.QPSolver((l, A, u), P)
    st = s.stats()
    assert st["N"] == 43284
    o = O.OracleQPSolver(P, None, A, l, u)
    s.setWarmStart(warm); o.set_warm_start(warm)
    code, x = s.solve(); sto, xo = o.solve()
    assert code == ST2EXIT[sto] and s.info().iter == o.info().iter
    assert np.max(np.abs(x - xo)) <= TOL_X


@pytest.mark.parametrize("W", [330, 350, 372])
def test_solve_vector_that_fills_lds_to_the_budget(W):
    """GOMP horizons whose solve vector plus the second positions of the multi-row chunks want more than LDS holds: the extra
    rows are handed out until the budget is used up to the last byte - which must leave room for the kernels' own static LDS
    (a 160 KB request failed to launch: found with the reference's 802-waypoint example, whose fourth segment sits there)."""
    D = 6
    P, (l, A, u), warm = PR.gomp_qp(D, W, np.zeros(D), np.array([np.pi, 0, 0, 0, 0, 0]))
    s = M.QPSolver((l, A, u), P)
    o = O.OracleQPSolver(P, None, A, l, u)
    s.setWarmStart(warm); o.set_warm_start(warm)
    code, x = s.solve(); sto, xo = o.solve()
    assert code == ST2EXIT[sto] and s.info().iter == o.info().iter
    assert np.max(np.abs(x - xo)) <= TOL_X


def test_sixteen_waves_per_tile_variant(monkeypatch):
    """The 8-wave and 16-wave instantiations of the solve kernels (512 / 1 024 threads per tile; a batch with no more tiles
    than CUs gets 16 waves by default) walk schedules built for their wave count; results equal up to round-off, iteration
    counts exactly."""
    pr = PR.random_box_qp(10, n=96, mg=64, nnz_per_row=6)
    def run():
        s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
        info = s.solve()
        return s.stats()["threads_per_block"], [i.iter for i in info], s.primal().copy()
    tdef, _, _ = run()
    assert tdef == 1024                                      # 10 tiles on 256 CUs
    monkeypatch.setenv("MI_OSQP_THREADS", "512")
    t8, it8, x8 = run()
    monkeypatch.setenv("MI_OSQP_THREADS", "1024")
    t16, it16, x16 = run()
    assert (t8, t16) == (512, 1024)
    assert it8 == it16 and np.max(np.abs(x8 - x16)) <= 1e-9
    _compare_simple = _oracle_batch(pr, range(3))
    for b, (_, xo, _, _) in enumerate(_compare_simple):
        assert np.max(np.abs(x16[b] - xo)) <= TOL_X


def test_phase_trace_diagnostics_reproduce_the_op():
    """The traced twin of the kkt_solve op (mi_osqp_debug_trace_kkt_solve, scripts/trace_phases.py) computes the
    same solution bit for bit and returns one (before, after) clock stamp pair per phase barrier and wave."""
    import torch
    pr = PR.random_box_qp(8, n=96, mg=64, nnz_per_row=6)
    os.environ["MI_OSQP_TILE"] = "2"; os.environ["MI_OSQP_THREADS"] = "512"       # (the shape the traced twin exists for)
    try:
        s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    finally:
        del os.environ["MI_OSQP_TILE"]; del os.environ["MI_OSQP_THREADS"]
    B, N = 8, pr["n"] + pr["m"]
    rhs = torch.randn(B, N, dtype=torch.float64, device="cuda")
    sol_t = torch.empty_like(rhs); sol_o = torch.empty_like(rhs)
    tr, ftab, btab, (fp, bp, nw, words) = s.debug_trace_kkt_solve(rhs, sol_t)
    s.kkt_solve_device(rhs, sol_o)
    assert torch.equal(sol_t, sol_o)
    assert ftab.shape == (fp, 4 * nw + 1) and btab.shape == (bp, 4 * nw + 1) and tr.shape == (2, words)
    stamps = tr[0][8 + 4 * nw: 8 + 4 * nw + fp * nw * 2].reshape(fp, nw, 2).astype(np.int64)
    assert np.all((stamps[:, :, 1] - stamps[:, :, 0]) % (1 << 32) < (1 << 28))     # every barrier was passed by every wave
    assert np.all(stamps[:, :, 1] != 0)


def test_degenerate_shapes_no_constraints_and_one_variable():
    """Edge shapes of the boundary: m = 0 (unconstrained QP: the KKT system is just P + sigma I) and n = m = 1."""
    n = 5
    P = sp.csc_matrix(np.diag([1.0, 2, 3, 4, 5]) + 0.1 * np.ones((5, 5)))
    q = np.array([1.0, -2, 0.5, 0, 3])
    A = sp.csc_matrix((0, n))
    s = M.BatchSolver(P, np.tile(P.data, (2, 1)), np.tile(q, (2, 1)), A, np.zeros((2, 0)), np.zeros((2, 0)), np.zeros((2, 0)))
    info = s.solve()
    o = O.OracleQPSolver(P, q, A, np.zeros(0), np.zeros(0))
    st, xo = o.solve()
    for b in range(2):
        assert info[b].exit_code == ST2EXIT[st] and info[b].iter == o.info().iter
        assert np.max(np.abs(s.primal()[b] - xo)) <= TOL_X
    assert np.max(np.abs(xo + np.linalg.solve(P.toarray(), q))) < 1e-4          # and that is the unconstrained minimiser
    P1 = sp.csc_matrix([[2.0]]); A1 = sp.csc_matrix([[1.0]])
    s = M.BatchSolver(P1, np.array([[2.0]]), np.array([[1.0]]), A1, np.array([[1.0]]), np.array([[0.3]]), np.array([[1.0]]))
    info = s.solve()
    o = O.OracleQPSolver(P1, np.array([1.0]), A1, np.array([0.3]), np.array([1.0]))
    st, xo = o.solve()
    assert info[0].exit_code == ST2EXIT[st] and info[0].iter == o.info().iter and abs(s.primal()[0][0] - xo[0]) <= TOL_X


def test_max_iter_at_a_rho_update_iteration_then_resolve():
    """Found by scripts/stress_random.py: a QP that runs into max_iter (4000 = a multiple of the rho interval) adapts rho
    and refactors in its very last iteration (upstream's loop order), and the next Solve() of the warm-started solver
    continues from THAT factor.  The second solve must therefore follow the oracle's (here: again 4000 iterations),
    and the count of rho updates accumulates over a plain re-solve as upstream's info does."""
    pr = PR.random_box_qp(3, n=80, mg=63, nnz_per_row=1, pattern_seed=1021630442)
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    i1 = s.solve()
    i2 = s.solve()
    for b in range(3):
        P, A = PR.qp_matrices(pr, b)
        o = O.OracleQPSolver(P, pr["q"][b], A, pr["l"][b], pr["u"][b])
        st1, _ = o.solve(); io1 = o.info()
        it1, ru1 = io1.iter, io1.rho_updates
        st2, x2 = o.solve(); io2 = o.info()
        assert (i1[b].exit_code, i1[b].iter, i1[b].rho_updates) == (ST2EXIT[st1], it1, ru1)
        assert (i2[b].exit_code, i2[b].iter, i2[b].rho_updates) == (ST2EXIT[st2], io2.iter, io2.rho_updates)
        tol = 1e-3 if st2 == -2 else TOL_X
        assert np.max(np.abs(s.primal()[b] - x2)) <= tol
    assert any(i.exit_code == ST2EXIT[-2] for i in i1)          # the case really contains a max_iter QP


# ---- dense tail (inverted Schur complement of the trailing rows)

def test_dense_tail_on_and_off_agree_and_match_oracle(monkeypatch):
    pr = PR.random_box_qp(8)
    res = {}
    for mode in ("auto", "0"):
        if mode == "0":
            monkeypatch.setenv("MI_OSQP_DENSE_TAIL", "0")
        s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
        assert (s.stats()["dense_tail_rows"] > 0) == (mode == "auto")
        info = s.solve()
        x1 = s.primal().copy()
        s.update_bounds(pr["l"] * 0.7, pr["u"] * 0.7)          # re-solve from the refactored state (rho updates happened)
        info2 = s.solve()
        res[mode] = ([i.iter for i in info], x1, [i.iter for i in info2], s.primal().copy(), [i.rho_updates for i in info2])
        if mode == "auto":
            _compare(info, x1, _oracle_batch(pr, range(8)), range(8))
        s.close()
    assert res["auto"][0] == res["0"][0] and res["auto"][2] == res["0"][2] and res["auto"][4] == res["0"][4]
    assert np.max(np.abs(res["auto"][1] - res["0"][1])) <= 1e-9 and np.max(np.abs(res["auto"][3] - res["0"][3])) <= 1e-9


@pytest.mark.parametrize("k", [64, 192])
def test_forced_dense_tail_on_gomp_matches_oracle(k, monkeypatch):
    monkeypatch.setenv("MI_OSQP_DENSE_TAIL", str(k))
    P, (l, A, u), _ = PR.gomp_qp(6, 50, np.zeros(6), np.ones(6))
    s = M.QPSolver((l, A, u), P)
    assert s.stats()["dense_tail_rows"] == k
    code, x = s.solve()
    o = O.OracleQPSolver(P, None, A, l, u)
    st, xo = o.solve()
    assert code == 0 and st == 1 and s.info().iter == o.info().iter
    assert np.max(np.abs(x - xo)) <= TOL_X


# ---- relaxed supernodes (explicit zeros merge chains of near-identical columns; analyze() decides, MI_OSQP_RELAX forces)

@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 6, 50), (5, 3, 40)])
def test_relaxed_and_fundamental_supernodes_agree_and_match_oracle(shape, monkeypatch):
    """The factor with relaxed supernodes holds the same numbers plus exact zeros: solves, the refactorisation after an
    update of A and the bounds, and the rho updates of a long solve take the same iterations either way (x within 1e-9) and
    match the oracle; the relaxed form has fewer phases per sweep."""
    B, D, W = shape
    pr = PR.gomp_batch(B, D, W)
    res, phases = {}, {}
    rng = np.random.default_rng(4)
    Ax2 = pr["Ax"] * (1.0 + 0.05 * rng.standard_normal(pr["Ax"].shape))
    for relax in ("0", "16"):
        monkeypatch.setenv("MI_OSQP_RELAX", relax)
        s = M.BatchSolver(pr["P"], pr["Px"], None, pr["A"], pr["Ax"], pr["l"], pr["u"], eps_abs=1e-7, eps_rel=1e-7)
        st = s.stats()
        phases[relax] = st["fwd_levels"] + st["bwd_levels"]
        s.warm_start_x(pr["warm"])
        info = s.solve(); x1 = s.primal().copy()
        s.update_A_bounds(Ax2, pr["l"] * 0.9, pr["u"] * 0.9)
        info2 = s.solve()
        res[relax] = ([i.iter for i in info], x1, [i.iter for i in info2], s.primal().copy(), [i.rho_updates for i in info2], [i.exit_code for i in info2])
        if relax == "16":
            for b in range(B):
                P, A = PR.qp_matrices(pr, b)
                o = O.OracleQPSolver(P, None, A, pr["l"][b], pr["u"][b], eps_abs=1e-7, eps_rel=1e-7)
                o.set_warm_start(pr["warm"][b])
                sto, xo = o.solve()
                assert info[b].exit_code == 0 and sto == 1 and info[b].iter == o.info().iter
                assert np.max(np.abs(x1[b] - xo)) <= TOL_X
        s.close()
    assert phases["16"] < phases["0"]
    a, r = res["0"], res["16"]
    assert a[0] == r[0] and a[2] == r[2] and a[4] == r[4] and a[5] == r[5]
    assert np.max(np.abs(a[1] - r[1])) <= 1e-9 and np.max(np.abs(a[3] - r[3])) <= 1e-9


@pytest.mark.gpu
def test_update_from_device_resident_values_equals_the_host_pointer_update_bitwise():
    """mi_osqp_batch_update_A_bounds_device (new A values and bounds already in HBM) is QPSolver::update without the PCIe
    leg: same kernels on the same numbers -> the same bits as the host-pointer call; l > u is refused and leaves the handle as
    it was."""
    import torch
    pr = PR.gomp_batch(24, 6, 30)
    rng = np.random.default_rng(8)
    Ax2 = pr["Ax"] * (1.0 + 0.05 * rng.standard_normal(pr["Ax"].shape))
    l2, u2 = pr["l"] * 0.9, pr["u"] * 0.9
    out = []
    for dev in (False, True):
        s = M.BatchSolver(pr["P"], pr["Px"], None, pr["A"], pr["Ax"], pr["l"], pr["u"])
        s.warm_start_x(pr["warm"]); s.solve()
        if dev:
            tA, tl, tu = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (Ax2, l2, u2))
            bad_l = tl.clone(); bad_l[3, 5] = 1e3; bad_u = tu.clone(); bad_u[3, 5] = -1e3
            with pytest.raises(M.MiOsqpError):
                s.update_A_bounds_device(tA, bad_l, bad_u)
            s.update_A_bounds_device(tA, tl, tu, stream=torch.cuda.current_stream().cuda_stream)
        else:
            s.update_A_bounds(Ax2, l2, u2)
        info = s.solve()
        out.append(([i.iter for i in info], [i.exit_code for i in info], s.primal().copy(), s.dual().copy()))
        s.close()
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])


@pytest.mark.gpu
def test_launch_shape_follows_the_pattern_class():
    """solver.hip shape_and_analysis: a batch whose pattern gets a dense tail (bandwidth-bound iteration) runs at one QP per
    tile in 16-wave workgroups whatever its size; trajectory QPs (phase-bound, no dense tail) keep two per tile from 384 QPs
    on.  Both solve to the oracle's answer."""
    pr = PR.random_box_qp(400)
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"])
    st = s.stats()
    assert st["dense_tail_rows"] > 0 and st["tile"] == 1 and st["threads_per_block"] == 1024
    info = s.solve(); x = s.primal()
    _compare(info, x, _oracle_batch(pr, [0, 399]), [0, 399])
    s.close()
    pg = PR.gomp_batch(400, 3, 20)
    s = M.BatchSolver(pg["P"], pg["Px"], None, pg["A"], pg["Ax"], pg["l"], pg["u"])
    st = s.stats()
    assert st["dense_tail_rows"] == 0 and st["tile"] == 2
    s.warm_start_x(pg["warm"])
    info = s.solve(); x = s.primal()
    for b in (0, 399):
        P, A = PR.qp_matrices(pg, b)
        o = O.OracleQPSolver(P, None, A, pg["l"][b], pg["u"][b])
        o.set_warm_start(pg["warm"][b])
        sto, xo = o.solve()
        assert info[b].exit_code == 0 and sto == 1 and info[b].iter == o.info().iter and np.max(np.abs(x[b] - xo)) <= TOL_X
    s.close()
