"""CPU: the references of the adjoint derivative (tests/adjoint_refs.py) against central differences of the active-set
solution map in mpmath, against closed forms, and the float64 reference against its mpmath twin on the problems the GPU
tests use; the preconditions of those problems (README "Adjoint derivative")."""
import mpmath as mp
import numpy as np
import pytest
import scipy.sparse as sp

import adjoint_refs as AR
import osqp_solver_amd as M     # noqa: F401  (the tests need the feature: BatchSolver.adjoint)
from osqp_solver_amd import problems as PR


def test_the_feature_is_present():
    assert callable(getattr(M.BatchSolver, "adjoint", None)) and callable(getattr(M.BatchSolver, "adjoint_device", None))


# ------------------------------------------------------------------ central differences, mpmath
def _mp_map(Prc, Pv, Arc, Av, q, l, u, act, n, m, gx, gy):
    """L = g_x'x + g_y'y at the active-set solution of the given data (all mpf), by a direct mpmath LU"""
    ia = [i for i in range(m) if act[i]]
    pos = {i: k for k, i in enumerate(ia)}
    N = n + len(ia)
    K = mp.zeros(N, N)
    for (i, j), v in zip(zip(*Prc), Pv):
        K[i, j] += v
        if i != j:
            K[j, i] += v
    for (i, j), v in zip(zip(*Arc), Av):
        if i in pos:
            K[n + pos[i], j] += v; K[j, n + pos[i]] += v
    b = mp.matrix([-v for v in q] + [l[i] if act[i] < 0 else u[i] for i in ia])
    s = mp.lu_solve(K, b)
    return mp.fsum(gx[i] * s[i] for i in range(n)) + mp.fsum(gy[i] * s[n + pos[i]] for i in ia), s, ia


@pytest.mark.parametrize("shape", [dict(n=12, mg=8, nnz_per_row=3), dict(n=7, mg=5, nnz_per_row=2, half_bw=2)], ids=["12x20", "7x12"])
def test_formulas_agree_with_central_differences_of_the_solution_map(shape):
    pr = PR.random_box_qp(1, **shape)
    fx = AR.fixture(pr, 0)
    n, m, act = pr["n"], pr["m"], fx["act"]
    assert 0 < np.count_nonzero(act) < m
    if n == 12:
        assert (act < 0).any() and (act > 0).any()           # (the small shape has lower-active rows only)
    gx, gy = AR.gradient_seeds(1, n, m, seed=5)
    with mp.workdps(AR.DPS):
        f = lambda a: [mp.mpf(float(v)) for v in a]
        U = AR.triu_csc(fx["P"])
        Prc, Arc = AR.rows_cols(U), AR.rows_cols(fx["A"])
        data = dict(Pv=f(U.data), Av=f(sp.csc_matrix(fx["A"]).data), q=f(fx["q"]), l=f(fx["l"]), u=f(fx["u"]))
        g = (f(gx[0]), f(gy[0]))
        run = lambda d: _mp_map(Prc, d["Pv"], Arc, d["Av"], d["q"], d["l"], d["u"], act, n, m, *g)
        _, s, ia = run(data)
        x = [s[i] for i in range(n)]
        y = [mp.mpf(0)] * m
        for k, i in enumerate(ia):
            y[i] = s[n + k]
        ref = AR.adjoint_ref_mp(fx["P"], fx["A"], act, x, y, gx[0], gy[0])
        h = mp.mpf(10) ** -20
        offdiag = [k for k in range(len(Prc[0])) if Prc[0][k] != Prc[1][k]]
        diag = [k for k in range(len(Prc[0])) if Prc[0][k] == Prc[1][k]]
        rows_act = [k for k in range(len(Arc[0])) if act[Arc[0][k]]]
        rows_in = [k for k in range(len(Arc[0])) if not act[Arc[0][k]]]
        assert offdiag and diag and rows_act and rows_in
        chosen = dict(q=range(n), l=range(m), u=range(m), Av=rows_act[:5] + rows_in[:3], Pv=offdiag[:5] + diag[:3])
        name = dict(q="dq", l="dl", u="du", Av="dA", Pv="dP")
        worst = mp.mpf(0)
        for key, idx in chosen.items():
            for k in idx:
                vals = []
                for sgn in (1, -1):
                    d = dict(data); d[key] = list(data[key]); d[key][k] += sgn * h
                    vals.append(run(d)[0])
                cd = (vals[0] - vals[1]) / (2 * h)
                worst = max(worst, abs(cd - ref[name[key]][k]))
        assert worst < mp.mpf(10) ** -30, worst      # truncation h^2 = 1e-40 times third derivatives of order 1


# ------------------------------------------------------------------ closed forms
def _one(p, a):
    return sp.csc_matrix(np.array([[p]])), sp.csc_matrix(np.array([[a]]))


def test_closed_form_one_variable_inactive():
    p, q, g = 2.0, 0.6, 1.25
    P, A = _one(p, 1.0)
    act = np.array([0], dtype=np.int8)
    x, y = AR.active_set_solution(P, np.array([q]), A, np.array([-1.0]), np.array([1.0]), act)
    assert x[0] == -q / p and y[0] == 0.0
    r = AR.adjoint_ref(P, A, act, x, y, np.array([g]), np.array([7.0]))        # g_y of an inactive row is not read
    np.testing.assert_allclose(r["dq"], [-g / p], rtol=1e-15)
    np.testing.assert_allclose(r["dP"], [g * q / p ** 2], rtol=1e-15)
    assert r["dl"][0] == 0.0 and r["du"][0] == 0.0 and r["dA"][0] == 0.0


def test_closed_form_one_variable_active_at_u():
    p, q, g, ub = 2.0, -3.0, 1.25, 1.0                       # -q/p = 1.5 > u = 1
    P, A = _one(p, 1.0)
    act = np.array([1], dtype=np.int8)
    x, y = AR.active_set_solution(P, np.array([q]), A, np.array([-1.0]), np.array([ub]), act)
    assert x[0] == ub and y[0] == -(p * ub + q) and y[0] > 0
    r = AR.adjoint_ref(P, A, act, x, y, np.array([g]))
    assert r["dq"][0] == 0.0 and r["dl"][0] == 0.0 and r["dP"][0] == 0.0
    assert r["du"][0] == g                                   # dx/du = 1
    np.testing.assert_allclose(r["dA"], [-g * ub], rtol=1e-15)      # x = u / a: dx/da = -u at a = 1
    # and dL/dy: y = -(p u / a + q) / a, dy/du = -p, dy/dq = -1
    r = AR.adjoint_ref(P, A, act, x, y, np.array([0.0]), np.array([1.0]))
    np.testing.assert_allclose([r["du"][0], r["dq"][0], r["dP"][0]], [-p, -1.0, -ub], rtol=1e-15)


def test_closed_form_no_constraints():
    P = sp.csc_matrix(np.array([[2.0, 0.5], [0.5, 1.0]]))
    A = sp.csc_matrix((0, 2))
    q, g = np.array([1.0, -2.0]), np.array([0.3, 0.7])
    act = np.zeros(0, dtype=np.int8)
    x, y = AR.active_set_solution(P, q, A, np.zeros(0), np.zeros(0), act)
    r = AR.adjoint_ref(P, A, act, x, y, g)
    Pd = P.toarray()
    rx = np.linalg.solve(Pd, g)
    np.testing.assert_allclose(r["dq"], -rx, rtol=1e-14)
    # stored upper triangle, CSC order: (0,0), (0,1), (1,1)
    np.testing.assert_allclose(r["dP"], [-rx[0] * x[0], -(rx[0] * x[1] + rx[1] * x[0]), -rx[1] * x[1]], rtol=1e-14)
    assert len(r["dA"]) == 0 and len(r["dl"]) == 0 and len(r["du"]) == 0


@pytest.mark.parametrize("side", [-1, 1])
def test_closed_form_equality_row_gets_its_gradient_on_the_marked_side(side):
    P, A = _one(2.0, 1.0)
    act = np.array([side], dtype=np.int8)
    l = u = np.array([0.25])
    x, y = AR.active_set_solution(P, np.array([0.6]), A, l, u, act)
    assert abs(x[0] - 0.25) <= 1e-15
    r = AR.adjoint_ref(P, A, act, x, y, np.array([1.5]))
    marked, other = ("dl", "du") if side < 0 else ("du", "dl")
    assert abs(r[marked][0] - 1.5) <= 1e-15 and r[other][0] == 0.0


# ------------------------------------------------------------------ the GPU test problems
@pytest.fixture(scope="module")
def gpu_fixtures():
    pr = AR.gpu_problem()
    return pr, [AR.fixture(pr, b, key="gpu") for b in range(AR.GPU_B)]


def test_gpu_fixture_preconditions(gpu_fixtures):
    pr, fxs = gpu_fixtures
    for b, fx in enumerate(fxs):
        AR.assert_preconditions(fx)
        # the refinement argument of the GPU bound: every round multiplies the error by delta |K^-1| = 1e-6 |K^-1|, and one
        # solve plus three rounds must leave less than rounding (1e-12): |K^-1| <= 1e3 does (measured on these six: <= 20.3)
        assert fx["inv_norm"] <= 1e3, (b, fx["inv_norm"])
        # the oracle's solution lies within its tolerance of the active-set solution
        assert np.max(np.abs(fx["x"] - fx["x_oracle"])) <= 1e-8 and np.max(np.abs(fx["y"] - fx["y_oracle"])) <= 1e-8
        np.testing.assert_array_equal(AR.polish_rule(fx["A"], fx["x"], fx["y"], fx["l"], fx["u"]), fx["act"])


def test_float64_reference_against_mpmath_on_the_gpu_problems(gpu_fixtures):
    """The reference's own error, in the units of the GPU bound (max |difference| / term scale): it must be a small part
    of the 1e-9 the GPU tests allow."""
    pr, fxs = gpu_fixtures
    gx, gy = AR.gradient_seeds(AR.GPU_B, pr["n"], pr["m"])
    worst = 0.0
    for b, fx in enumerate(fxs):
        xm, ym = AR.active_set_solution_mp(fx["P"], fx["q"], fx["A"], fx["l"], fx["u"], fx["act"])
        exact = AR.to_float(AR.adjoint_ref_mp(fx["P"], fx["A"], fx["act"], xm, ym, gx[b], gy[b]))
        ref = AR.adjoint_ref(fx["P"], fx["A"], fx["act"], fx["x"], fx["y"], gx[b], gy[b])
        e, _ = AR.worst_ratio(ref, exact, fx["x"], fx["y"])
        worst = max(worst, e)
    print(f"float64 reference against mpmath, worst ratio {worst:.2e}")
    assert worst <= 1e-12, worst          # a thousandth of the GPU bound; cond(K) 2^-53 = 5e-15 is what a stable solve gives (measured 4e-15)
