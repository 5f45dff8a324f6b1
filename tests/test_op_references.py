"""CPU: the references of tests/op_refs.py are right, the oracle's equilibration is OSQP 0.6's scale_data, and the
backward-error bound of the GPU KKT-solve tests (tests/test_gpu_ops.py) is calibrated on the host replay of the device
schedules."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import op_refs as R
import osqp_solver_amd as M
from oracle import oracle as O
from osqp_solver_amd import problems as PR

# Largest normwise backward error of the host replay of the device schedules (mi_osqp_debug_host_kkt_solve) on the shapes
# of the GPU tests, every solve form, scaling on and off, as measured by test_kkt_backward_error_calibration below (2.44e-16, on grid40).  The
# GPU tests allow KKT_BWD_GPU = 16 x this: the device sums the same schedules with wave-wide reductions in another order.
KKT_BWD_CALIBRATED = 2.5e-16
KKT_BWD_GPU = 16 * KKT_BWD_CALIBRATED


# ------------------------------------------------------------------ spmv_ref
def _random_pattern(rng, nr, nc, max_row):
    rows, cols = [], []
    for r in range(nr):
        k = int(rng.integers(0, max_row + 1))
        c = rng.choice(nc, size=min(k, nc), replace=False)
        rows += [r] * len(c); cols += list(c)
    return np.array(rows, np.int64), np.array(cols, np.int64)


def _logu(rng, size):
    """magnitudes in [1e-3, 1e3], random signs: no term is negligible next to another"""
    return rng.choice([-1.0, 1.0], size) * 10.0 ** rng.uniform(-3, 3, size)


def _small_case(seed):
    rng = np.random.default_rng(seed)
    n, m = int(rng.integers(1, 9)), int(rng.integers(0, 9))
    pr, pc = _random_pattern(rng, n, n, 4)
    up = pr <= pc
    P = sp.csc_matrix((_logu(rng, int(up.sum())), (pr[up], pc[up])), shape=(n, n))
    ar, ac = _random_pattern(rng, m, n, 5)
    A = sp.csc_matrix((_logu(rng, len(ar)), (ar, ac)), shape=(m, n))
    return P, A, _logu(rng, n), _logu(rng, m)


def _F(v):
    """the exact value of a long double"""
    return Fraction(*np.longdouble(v).as_integer_ratio())


def _exact_rows(Md, v):
    """M v and sum |m_ij v_j| in rational arithmetic (dense M)"""
    V = [Fraction(float(t)) for t in v]
    val = [sum((Fraction(float(Md[i, j])) * V[j] for j in range(Md.shape[1])), Fraction(0)) for i in range(Md.shape[0])]
    mag = [sum((abs(Fraction(float(Md[i, j])) * V[j]) for j in range(Md.shape[1])), Fraction(0)) for i in range(Md.shape[0])]
    return val, mag


@pytest.mark.parametrize("seed", range(12))
def test_spmv_ref_equals_exact_rational_arithmetic(seed):
    P, A, x, y = _small_case(seed)
    ref = R.spmv_ref(P, A, x, y)
    Pd, Ad = P.toarray(), A.toarray()
    Pf = np.triu(Pd) + np.triu(Pd, 1).T
    exact = {"Px": _exact_rows(Pf, x), "Aty": _exact_rows(Ad.T, y), "Ax": _exact_rows(Ad, x)}
    for key, (ev, em) in exact.items():
        val, mag, _ = ref[key]
        for i in range(len(ev)):
            # long double: 64-bit products, sums of <= 9 terms -> far below the fp64 bound (2^-58 of the magnitude)
            assert abs(_F(val[i]) - ev[i]) <= Fraction(2) ** -58 * em[i], (key, i)
            assert abs(_F(mag[i]) - em[i]) <= Fraction(2) ** -58 * em[i], (key, i)
    # the symmetric product is the same from the upper triangle and from the full matrix
    full = R.spmv_ref(sp.csc_matrix(Pf), A, x, y)
    np.testing.assert_array_equal(full["Px"][0], ref["Px"][0])
    np.testing.assert_array_equal(full["Px"][2], ref["Px"][2])
    # None reads as zeros
    z = R.spmv_ref(P, A, None, None)
    assert all(np.all(z[k][0] == 0) for k in z)


def _fp64_rows(Mc, v):
    """rows of M v as an fp64 kernel forms them: one rounding per term, in stored order"""
    out = np.zeros(Mc.shape[0])
    for r in range(Mc.shape[0]):
        s = 0.0
        for k in range(Mc.indptr[r], Mc.indptr[r + 1]):
            s = s + Mc.data[k] * v[Mc.indices[k]]
        out[r] = s
    return out


@pytest.mark.parametrize("seed", range(6))
def test_spmv_bound_holds_for_fp64_sums_and_breaks_for_a_dropped_or_doubled_term(seed):
    rng = np.random.default_rng(100 + seed)
    ar, ac = _random_pattern(rng, 40, 30, 12)
    A = sp.csr_matrix((_logu(rng, len(ar)), (ar, ac)), shape=(40, 30))
    x = _logu(rng, 30)
    val, mag, length = R.Coo.from_scipy(A).matvec(x)
    tol = R.spmv_tol(mag, length, 0)
    fp = _fp64_rows(A, x)
    assert np.all(np.abs(fp - val.astype(np.float64)) <= tol)
    for r in range(A.shape[0]):
        for k in range(A.indptr[r], A.indptr[r + 1]):
            term = A.data[k] * x[A.indices[k]]
            assert abs(term) > 2 * tol[r]                          # (built so that every term matters)
            for wrong in (fp[r] - term, fp[r] + term):             # one term dropped / counted twice
                assert abs(wrong - float(val[r])) > tol[r], (r, k)
    assert np.all(R.spmv_tol(mag, length, 10) >= tol)


# ------------------------------------------------------------------ the oracle's equilibration = OSQP 0.6 scale_data
def _limit(v):
    v = np.where(v < R.OQ_MIN_SCALING, 1.0, v)
    return np.minimum(v, 1e4)


def _scale_data_restated(P, q, A, iters=10):
    """OSQP 0.6 scale_data (Ruiz equilibration, then cost scaling, `iters` times) in numpy; P upper triangle, dense."""
    Pu, A = np.triu(np.asarray(P, float)), np.asarray(A, float).copy()
    n, m = A.shape[1], A.shape[0]
    q = np.zeros(n) if q is None else np.asarray(q, float).copy()
    D, E, c = np.ones(n), np.ones(m), 1.0

    def colnorm_P(Pu):
        return np.max(np.abs(Pu + np.triu(Pu, 1).T), axis=0, initial=0.0)

    for _ in range(iters):
        dt = np.maximum(colnorm_P(Pu), np.max(np.abs(A), axis=0, initial=0.0))
        et = np.max(np.abs(A), axis=1, initial=0.0)
        dt, et = 1.0 / np.sqrt(_limit(dt)), 1.0 / np.sqrt(_limit(et))
        Pu = dt[:, None] * Pu * dt[None, :]
        A = et[:, None] * A * dt[None, :]
        q, D, E = q * dt, D * dt, E * et
        ct = 1.0 / _limit(max(np.mean(colnorm_P(Pu)), float(_limit(np.max(np.abs(q), initial=0.0)))))
        Pu, q, c = Pu * ct, q * ct, c * ct
    return D, E, c


def _check_oracle_scaling(P, q, A, l, u):
    o = O.OracleQPSolver(sp.csc_matrix(P), q, sp.csc_matrix(A), l, u)
    D, E, c = o.scaling()
    Dr, Er, cr = _scale_data_restated(P, q, A)
    np.testing.assert_allclose(D, Dr, rtol=1e-14, atol=0)
    np.testing.assert_allclose(E, Er, rtol=1e-14, atol=0)
    assert abs(c - cr) <= 1e-14 * cr
    D0, E0, c0 = O.OracleQPSolver(sp.csc_matrix(P), q, sp.csc_matrix(A), l, u, scaling=0).scaling()
    assert np.all(D0 == 1.0) and np.all(E0 == 1.0) and c0 == 1.0
    return D, E, c


def test_oracle_scaling_is_osqp_scale_data_on_the_golden_fixtures(qp_fixtures):
    for name, d in qp_fixtures.items():
        _check_oracle_scaling(d["P"], d["q"], d["A"], d["l"], d["u"])


@pytest.mark.parametrize("seed", range(4))
def test_oracle_scaling_is_osqp_scale_data_on_random_box_qps(seed):
    pr = PR.random_box_qp(1, n=24, mg=16, nnz_per_row=3, pattern_seed=50 + seed, value_seed=60 + seed)
    P, A = PR.qp_matrices(pr, 0)
    _check_oracle_scaling(P.toarray(), pr["q"][0], A.toarray(), pr["l"][0], pr["u"][0])


def test_oracle_scaling_at_the_limits():
    rng = np.random.default_rng(4)
    n, m = 6, 5
    P = np.diag(rng.uniform(0.5, 2.0, n)); P[0, 1] = 0.3
    A = rng.standard_normal((m, n))
    A[:, 2] = 0.0; P[2, :] = 0.0; P[:, 2] = 0.0     # an empty column: limit_scaling gives 1
    A[1, :] = 0.0                                   # an empty row
    A[:, 3] = 0.0; A[0, 3] = 1e-4; P[3, :] = 0.0; P[:, 3] = 0.0     # column norm exactly MIN_SCALING (kept)
    A[:, 4] = 0.0; A[2, 4] = 5e-5; P[4, :] = 0.0; P[:, 4] = 0.0     # below MIN_SCALING (-> 1)
    A[3, 5] = 1e4; A[4, 0] = 1e9                    # at and beyond MAX_SCALING (-> 1e4)
    q = rng.standard_normal(n) * 1e6                # |q| beyond MAX_SCALING: the cost factor saturates
    D, E, c = _check_oracle_scaling(P, q, A, -np.ones(m), np.ones(m))
    assert E[1] == 1.0


# ------------------------------------------------------------------ KKT backward error: calibration of the GPU bound
def calibration_cases():
    pr = PR.random_box_qp(1, n=96, mg=64, nnz_per_row=6)
    P, A = PR.qp_matrices(pr, 0)
    yield "box96", P, A, pr["l"][0], pr["u"][0]
    pr = PR.random_box_qp(1, n=64, mg=48, nnz_per_row=4)
    P, A = PR.qp_matrices(pr, 0)
    yield "box64", P, A, pr["l"][0], pr["u"][0]
    pr = PR.random_box_qp(1, n=48, mg=24, nnz_per_row=3)
    P, A = PR.qp_matrices(pr, 0)
    A = sp.vstack([A, sp.csr_matrix(np.full((1, 48), 0.25))]).tocsc()       # one dense row (48 entries)
    yield "dense_row", P, A, np.append(pr["l"][0], -1.0), np.append(pr["u"][0], 1.0)
    pr = PR.grid_qp(40)                                                       # the deep elimination tree of a 2-D mesh
    P, A = PR.qp_matrices(pr, 0)
    yield "grid40", P, A, pr["l"][0], pr["u"][0]


def kkt_of(P, A, l, u, D, E, c, sigma, rho):
    Ps, As, _, ls, us = R.scaled_qp(P, A, None, l, u, D, E, c)
    return R.kkt_matrix(Ps, As, sigma, R.rho_vec(ls, us, rho))


@pytest.mark.parametrize("env", [{}, {"MI_OSQP_DENSE_TAIL": "64"}, {"MI_OSQP_DENSE_TAIL": "0"}, {"MI_OSQP_RELAX": "16"}],
                         ids=["default", "tail64", "tail0", "relax16"])
@pytest.mark.parametrize("scaling", [10, 0])
@pytest.mark.parametrize("tri_waves", [0, 16])
def test_kkt_backward_error_calibration(env, scaling, tri_waves, monkeypatch):
    """The host replay of the device schedules (LDS tiles or the dataflow form, dense tail, relaxed supernodes) against kkt_matrix.  The test
    problems are well conditioned on purpose: the explicit inverse of the dense tail is not backward stable in general."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    worst = 0.0
    for name, P, A, l, u in calibration_cases():
        n, m = A.shape[1], A.shape[0]
        D, E, c = O.OracleQPSolver(P, None, A, l, u, scaling=scaling).scaling()
        K = kkt_of(P, A, l, u, D, E, c, 1e-6, 0.1)
        for seed in range(3):
            rhs = np.random.default_rng(seed).standard_normal(n + m)
            sol, _, _ = M.debug_host_kkt_solve(P, A, l, u, rhs, tri_waves=tri_waves, scaling=scaling)
            worst = max(worst, R.backward_error(K, sol, rhs))
    print(f"KKT backward error of the host replay: {worst:.3e}")
    assert worst <= KKT_BWD_CALIBRATED, worst
