"""CPU: the problem families of tests/exit_cases.py pinned on the oracle and by arguments of their own, so that the GPU
tests of the exit codes (tests/test_gpu_exit_codes.py) cannot pass vacuously.

* every (family, settings) pair the GPU tests use ends with exactly the intended oracle status on every QP, and every
  all-codes batch holds all of 1, 2, 3, 4, -2, -3, -4 (the one exception: the dual infeasible ray at the 150 x 150 grid,
  whose oracle setup takes a quarter of a minute - the GPU test asserts its oracle status itself; its construction is
  checked here);
* each construction without the oracle: pinf by interval arithmetic in long double, dinf by P d = 0, q'd < 0 and A d in
  the recession cone for d = -e_0 (tests/op_refs.py, Coo.matvec); the feasible members by the KKT residuals of the
  oracle's solution at a tight tolerance (oracle/kkt_check.py);
* thresholds: the inaccurate codes sit near a decision by nature, and an fp64 difference of 1e-12 between the oracle and
  a kernel could flip a case that sits ON one.  Of the two remedies the second was taken: no getter was added to the
  oracle; instead every case with an inaccurate code (and every kMaxIterations one) keeps its oracle status when
  max_iter moves by +-1 and the tolerances by +-1 % (exit_cases.perturbations: 16 neighbouring settings)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exit_cases as EC                                   # noqa: E402
import op_refs as R                                       # noqa: E402
from oracle import oracle as O                            # noqa: E402
from oracle.kkt_check import kkt_residuals                # noqa: E402
from osqp_solver_amd import problems as PR                # noqa: E402


@pytest.fixture(scope="module")
def base():
    pr = PR.random_box_qp(EC.BASE_B, **EC.BASE_SHAPE)
    EC.assert_identity_block(pr)
    return pr


@pytest.fixture(scope="module")
def grid():
    pr = PR.grid_qp(40)
    EC.assert_identity_block(pr)
    return pr


def oracle_status(pr, b, **kw):
    P, A = PR.qp_matrices(pr, b)
    o = O.OracleQPSolver(P, pr["q"][b], A, pr["l"][b], pr["u"][b], **kw)
    st, x = o.solve()
    return st, x, o


def assert_pinf(pr, b, row):
    """The range of row `row` over the box of its columns, in long double with the rounding slack of the sum, misses [l, u]."""
    cols, vals = EC._a_row(pr, b, row)
    assert np.all(cols < pr["n"]) and len(cols) > 0
    a = vals.astype(R.LD)
    lo, hi = pr["l"][b, cols].astype(R.LD), pr["u"][b, cols].astype(R.LD)       # identity rows: the box of x_k is [l_k, u_k]
    assert np.all(lo <= hi) and np.all(np.abs(lo) < 1e20) and np.all(np.abs(hi) < 1e20)
    rmin = np.sum(np.minimum(a * lo, a * hi)); rmax = np.sum(np.maximum(a * lo, a * hi))
    slack = (len(cols) + 1) * np.finfo(R.LD).eps * np.sum(np.maximum(np.abs(a * lo), np.abs(a * hi)))
    l, u = R.LD(pr["l"][b, row]), R.LD(pr["u"][b, row])
    assert l <= u
    assert rmax + slack < l or rmin - slack > u, (float(rmin), float(rmax), float(l), float(u))


def assert_dinf(pr, b):
    """d = -e_0: P d = 0 (exactly: the entries are zeros), q'd < 0, (A d)_i = 0 wherever row i has a finite bound; the
    zeros of P are still stored entries; x = 0 is feasible."""
    n = pr["n"]
    P, A = PR.qp_matrices(pr, b)
    assert P.nnz == pr["P"].nnz and np.array_equal(P.indices, pr["P"].indices)       # pattern kept, zeros explicit
    d = np.zeros(n); d[0] = -1.0
    Pd, _, _ = R.sym_full(R.Coo.from_scipy(P)).matvec(d)
    assert np.all(Pd == 0)
    assert float(np.dot(pr["q"][b].astype(R.LD), d.astype(R.LD))) < 0
    Ad, _, _ = R.Coo.from_scipy(A).matvec(d)
    up_fin, lo_fin = pr["u"][b] < EC.INF, pr["l"][b] > -EC.INF
    assert np.all(Ad[up_fin] <= 0) and np.all(Ad[lo_fin] >= 0)        # recession cone of {l <= Ax <= u}
    assert np.count_nonzero(Ad) > 0 and np.all(~up_fin[Ad != 0]) and np.all(~lo_fin[Ad != 0])
    assert np.all(pr["l"][b] <= 0) and np.all(pr["u"][b] >= 0)        # x = 0 is feasible
    # positive semidefinite: what is left of P next to the zero row / column is still strictly diagonally dominant or
    # a principal submatrix of the positive definite Laplacian + I
    Pf = np.array(R.sym_full(R.Coo.from_scipy(P)).matvec(np.ones(n))[0], float)      # (touches every entry: finite)
    assert np.all(np.isfinite(Pf))
    assert np.min(np.linalg.eigvalsh(_dense_sym(P))) > -1e-12


def _dense_sym(P):
    U = np.triu(P.toarray())
    return U + np.triu(U, 1).T


def check_members(pr, kinds):
    for b, k in enumerate(kinds):
        if k == "pinf":
            assert_pinf(pr, b, pr["n"])
        elif k == "dinf":
            assert_dinf(pr, b)


def test_constructions_hold_without_the_oracle(base, grid):
    for _, pr, kinds in EC.exact_batches(base):
        check_members(pr, kinds)
    for name in EC.ALL_CODES:
        pr, _, _ = EC.all_codes_batch(base, name)
        check_members(pr, [s[0] for s in EC.ALL_CODES[name][1]])
    for name, (kind, _, _, _) in EC.GRID_CASES.items():
        pr, _, _ = EC.grid_case(grid, name)
        check_members(pr, [kind])
    big = PR.grid_qp(150)
    EC.assert_identity_block(big)
    pr = EC.apply_kinds(big, ["dinf"], grid=True)                 # (assert_dinf without its eigenvalues of a 22 500^2 matrix)
    d = np.zeros(pr["n"]); d[0] = -1.0
    P, A = PR.qp_matrices(pr, 0)
    assert np.all(R.sym_full(R.Coo.from_scipy(P)).matvec(d)[0] == 0) and pr["q"][0, 0] > 0
    Ad = R.Coo.from_scipy(A).matvec(d)[0]
    assert np.all(np.abs(pr["l"][0][Ad != 0]) >= EC.INF) and np.all(np.abs(pr["u"][0][Ad != 0]) >= EC.INF)
    # a pinf construction that is NOT infeasible must be caught by the interval check (the check can fail)
    ok = EC.take(base, [0])
    with pytest.raises(AssertionError):
        assert_pinf(ok, 0, ok["n"])


@pytest.mark.parametrize("settings", sorted(EC.EXACT_SETTINGS))
def test_rotated_batches_give_the_exact_codes_on_the_oracle(base, settings):
    kw = EC.EXACT_SETTINGS[settings]
    its = set()
    for name, pr, kinds in EC.exact_batches(base):
        for b, k in enumerate(kinds):
            st, x, o = oracle_status(pr, b, **kw)
            assert st == EC.KIND_STATUS[k], (name, b, k, st)
            assert np.all(np.isnan(x)) == (k != "feas") and np.all(np.isnan(o.y)) == (k != "feas")
            if k != "feas":
                assert o.info().obj_val == (1e30 if k == "pinf" else -1e30)
            its.add((k, o.info().iter))
    assert len({i for k, i in its if k == "pinf"}) > 1          # the infeasible QPs of a batch do not leave together


def test_feasible_members_are_feasible(base):
    for b in range(EC.BASE_B):
        st, x, o = oracle_status(base, b, eps_abs=1e-9, eps_rel=1e-9, max_iter=20000)
        assert st == 1
        P, A = PR.qp_matrices(base, b)
        r = kkt_residuals(P, base["q"][b], A, base["l"][b], base["u"][b], x, o.y)
        assert r["prim"] <= 1e-7 and r["stat"] <= 1e-7 and r["comp"] <= 1e-6 and r["dual_sign"] == 0.0, r


@pytest.mark.parametrize("name", sorted(EC.ALL_CODES))
def test_all_codes_batches_hold_every_status_with_a_margin(base, name):
    pr, kw, expect = EC.all_codes_batch(base, name)
    assert set(expect) == set(EC.STATUSES) and len(expect) == 13
    for b, want in enumerate(expect):
        st, x, o = oracle_status(pr, b, **kw)
        assert st == want, (name, b, st, want)
        assert np.all(np.isnan(x)) == (want in (3, 4, -3, -4))
        if want in (2, 3, 4, -2):                                    # threshold cases: the status has a margin
            assert o.info().iter == kw["max_iter"]
            for k2 in EC.perturbations(kw):
                assert oracle_status(pr, b, **k2)[0] == want, (name, b, want, k2)
    # the single slots the B = 1 forms use are the same QPs with the same settings: nothing else to pin


@pytest.mark.parametrize("name", sorted(EC.GRID_CASES))
def test_grid_cases_on_the_oracle(grid, name):
    pr, kw, want = EC.grid_case(grid, name)
    st, x, o = oracle_status(pr, 0, **kw)
    assert st == want
    if want in (4, -2):
        for k2 in EC.perturbations(dict(dict(eps_dual_inf=1e-4), **kw)):
            assert oracle_status(pr, 0, **k2)[0] == want, k2
