"""CPU: the references of tests/factor_refs.py, before tests/test_gpu_factor_refs.py holds the device refactorisation to them.

The long-double reference against mpmath (REF_ERROR); the recorded errors of the three fp64 twins, measured again for every
case (FACTOR_TWIN_ERROR: the only source of FACTOR_BOUND); the convergence of the reference's refinement for every case, QP and
right-hand side, none excluded; the CPU oracle's kkt_solve - a correct fp64 implementation with its own factor - inside the
bound of every case; the distance of four deliberate defects of the inverted-tail twin from the reference, in bounds, and what
the backward error of one Gaussian right-hand side (KKT_BWD_GPU) sees of them; the construction of the lost-inertia cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import admm_refs as AF                                                          # noqa: E402
import factor_refs as F                                                         # noqa: E402
import op_refs as R                                                             # noqa: E402
from osqp_solver_amd import problems as PR                                      # noqa: E402
from test_op_references import KKT_BWD_GPU                                      # noqa: E402

CASES = F.case_list()
POWER = 100.0


# ------------------------------------------------------------------ the reference itself
def test_reference_against_mpmath():
    """n = 12, m = 20 (N = 32), every rho of RHOS, the Gaussian vector and 8 unit vectors: the refined long-double solve against
    the same refinement at 50 digits, in err_x and err_y.  At least 1000 x below every recorded twin error of those measures."""
    pr = PR.random_box_qp(1, n=12, mg=8, nnz_per_row=3)
    (D, E, c), perm = F.oracle_scaling_and_order(pr, 0)
    worst = 0.0
    for rho in F.RHOS:
        system = F.system_of(pr, 0, D, E, c, rho)
        n = system.n
        rhs, _ = F.rhs_set(perm, 0, 5)
        with AF.context("mp"):
            exact = AF.refined_solver(AF.arr(system.Kd, "mp"), "mp")
            for r in rhs:
                ref, mp = AF.arr(system.ref(r), "mp"), exact(AF.arr(r, "mp"))
                for lo, hi in ((0, n), (n, len(r))):
                    err = max(abs(a - b) for a, b in zip(ref[lo:hi], mp[lo:hi])) / max(abs(b) for b in mp[lo:hi])
                    worst = max(worst, float(err))
    print(f"reference against mpmath: {worst:.3e}")
    assert worst <= F.REF_ERROR <= 2 * worst
    for name, row in F.FACTOR_TWIN_ERROR.items():
        assert F.REF_ERROR <= min(row["err_x"], row["err_y"]) / 1000, name


def test_box_pattern_is_well_conditioned():
    """cond(K) <= 1e4 on the N = 640 batch at every rho the device is taken to (measured: 5.07e3 at rho = 1e-3, QP 0, the
    largest): the floor of the reference's refinement, cond(K) 2^-64, is below 1e-15 of its solutions there, and the fp64
    twins, at cond(K) 2^-53, are what the bound is made of"""
    for b in range(F.BOX_B):
        for rho in F.RHOS + (F.INERTIA_RHO[0],):
            cond = np.linalg.cond(F.oracle_system(F.data("box"), b, rho).K64())
            assert cond <= 1e4, (b, rho, cond)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_twin_errors_are_the_recorded_table(case):
    """and, of every QP and right-hand side of the case: the refinement converges (System.ref raises otherwise) to a
    backward error of 2^-58 or less; the two residual measures are the rows of op_refs.backward_error"""
    name, pattern, k, rho = case
    got = F.measure_twins(pattern, k, rho)
    print(f"twin errors {name}:", {m: f"{v:.3e}" for m, v in got.items()})
    for m in F.MEASURES:
        const = F.FACTOR_TWIN_ERROR[name][m]
        assert got[m] <= const <= 2 * got[m], (name, m, got[m], const)
        assert F.FACTOR_BOUND[name][m] == 32 * const
    for order, perm in F.orders(pattern, k).items():
        for pr, b in F.case_qps(pattern, k, rho, perm):
            system = F.oracle_system(pr, b, rho)
            rhs, labels = F.rhs_set(perm, k, F.seed_of(k, b))
            assert len(rhs) == 1 + (k // 16 if k else 8)
            for r, label in zip(rhs, labels):
                ref = system.ref(r)
                assert R.backward_error(system.K, ref, r) <= 2.0 ** -58, (name, order, b, label)
            sol = AF.ldl_solver(system.K64(), perm, 0)(rhs[0])
            ms = system.measures(sol, rhs[0])
            assert max(ms["bwd_x"], ms["bwd_y"]) == R.backward_error(system.K, sol, rhs[0])


def test_unit_vectors_sit_in_every_tile_column_of_the_tail():
    perm = F.oracle_scaling_and_order(F.data("box"), 0)[1]
    N = len(perm)
    where = np.empty(N, int)
    where[perm] = np.arange(N)
    for k in F.TAILS[1:]:
        rhs, _ = F.rhs_set(perm, k, 0)
        cols = sorted((where[np.flatnonzero(r)[0]] - (N - k)) // 16 for r in rhs[1:])
        assert cols == list(range(k // 16)) and all(np.count_nonzero(r) == 1 for r in rhs[1:]), k
    rhs, _ = F.rhs_set(perm, 0, 0)
    assert sorted(where[np.flatnonzero(r)[0]] for r in rhs[1:]) == list(range(N - 8, N))


def test_sweep_inverse_inverts():
    """a quasi-definite 128 x 128 matrix (both signs of pivots, as S has): the blocked sweep against numpy's inverse"""
    rng = np.random.default_rng(4)
    G = rng.standard_normal((128, 128))
    S = G @ G.T / 128 + np.eye(128)
    S[64:, 64:] = -(S[64:, 64:] + np.eye(64))
    inv = np.linalg.inv(S)
    got = F.sweep_inverse(S)
    assert np.array_equal(got, got.T) and np.max(np.abs(got - inv)) <= 1e-13 * np.max(np.abs(inv))


# ------------------------------------------------------------------ a correct fp64 implementation of another make
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_oracle_meets_the_bound(case):
    name, pattern, k, rho = case
    worst, where = 0.0, None
    for pr, b in F.case_qps(pattern, k, rho):
        (D, E, c), perm = F.oracle_scaling_and_order(pr, b)
        o = F.oracle_of(pr, b, rho)
        for got, want in zip(o.scaling(), (D, E, c)):
            np.testing.assert_array_equal(got, want)                           # (the scaling does not depend on rho)
        system = F.oracle_system(pr, b, rho)
        rhs, labels = F.rhs_set(perm, k, F.seed_of(k, b))
        for r, label in zip(rhs, labels):
            ratio, m = F.ratio(system.measures(o.kkt_solve(r), r), name)
            if ratio >= worst:
                worst, where = ratio, (b, label, m)
    print(f"oracle {name}: worst ratio {worst:.3f} at {where}")
    assert worst <= 1.0, (name, worst, where)


# ------------------------------------------------------------------ power
def power_setup(pattern, k, rho=F.RHO0):
    pr = F.data(pattern)
    (D, E, c), perm = F.oracle_scaling_and_order(pr, 0)
    system = F.oracle_system(pr, 0, rho)
    rhs, labels = F.rhs_set(perm, k, F.seed_of(k, 0))
    return pr, (D, E, c), perm, system, rhs, labels


def defective(pattern, k, defect, rho=F.RHO0):
    """(the sweep twin of QP 0 at rho and k tail rows with one defect, what it was applied to)"""
    pr, (D, E, c), perm, system, rhs, labels = power_setup(pattern, k, rho)
    if defect == "stale_rho":                                    # row 7 of A keeps the rho_vec entry of rho = 1
        stale = F.system_of(pr, 0, D, E, c, rho, stale=(7, 1.0))
        assert np.count_nonzero(stale.rho_vec != system.rho_vec) == 1
        return F.twins(stale, perm, k)["sweep"], 7
    tail = AF.ldl_solver(system.K64(), perm, k)
    if defect == "tile_diag":
        return F.sweep_solver(system.K64(), tail, "tile", (2, 2)), (2, 2)
    if defect == "tile_off":
        return F.sweep_solver(system.K64(), tail, "tile", (3, 2)), (3, 2)
    if defect == "drop":                                         # the source column with the largest update of S
        _, h, L, d = tail.factor
        c0 = int(np.argmax(np.abs(d[:h]) * np.max(np.abs(L[h:, :h]), axis=0) ** 2))
        return F.sweep_solver(system.K64(), tail, "drop", c0), c0
    assert defect == "unsym"
    return F.sweep_solver(system.K64(), tail, "unsym", 1), 1


def bounds_off(pattern, k, defect, rho=F.RHO0):
    """[(distance of the defective twin from the reference in bounds, its measure)] per right-hand side, the labels"""
    _, _, _, system, rhs, labels = power_setup(pattern, k, rho)
    solve, where = defective(pattern, k, defect, rho)
    name = F.case_name(pattern, k, rho)
    ratios = [F.ratio(system.measures(solve(r), r), name) for r in rhs]
    best = int(np.argmax([r for r, _ in ratios]))
    print(f"{defect} at {where}, {name}: {ratios[best][0]:.3g} bounds in {ratios[best][1]} at {labels[best]}; "
          f"Gaussian vector alone: {ratios[0][0]:.3g}")
    return ratios, best, solve


@pytest.mark.parametrize("k", [128, 320])
@pytest.mark.parametrize("defect", ["tile_diag", "tile_off", "drop", "unsym", "stale_rho"])
def test_deliberate_defects_are_far_away(defect, k):
    """one 16 x 16 tile of S^-1 scaled by 1 + 1e-10 (a diagonal one, and one beside the diagonal); the Schur update of one
    source column dropped; one diagonal 16-tile left unsymmetrised; the rho of one row stale: each at least 100 bounds off on
    at least one right-hand side (box pattern, QP 0, rho = 0.1)"""
    ratios, best, _ = bounds_off("box", k, defect)
    assert ratios[best][0] >= POWER, (defect, k, ratios[best])


@pytest.mark.parametrize("rho", sorted({F.RHO0, *F.GOMP_RHO_EACH}))
def test_the_backward_error_of_one_gaussian_vector_does_not_see_a_scaled_tile(rho):
    """What the criterion of test_gpu_ops.py (the backward error of one Gaussian right-hand side under KKT_BWD_GPU) cannot see.
    GOMP pattern, 320 tail rows, tile (2, 2) of S^-1 scaled by 1 + 1e-10: more than 100 bounds off on a unit vector of that
    tile column (measured 1.7e4 .. 2.7e4), while the Gaussian vector's backward error stays at 1e-17 - its free rows make
    |K|_inf 1e6 - and even the four measures of this module stay inside the bound on the Gaussian vector alone.  (On the box
    pattern, |K|_inf about 10, the same defect does show in the Gaussian vector's backward error: 1.5e-12.)"""
    ratios, best, solve = bounds_off("gomp", 320, "tile_diag", rho)
    _, _, _, system, rhs, _ = power_setup("gomp", 320, rho)
    bwd = R.backward_error(system.K, solve(rhs[0]), rhs[0])
    print(f"rho = {rho}: backward error {bwd:.3e} of the Gaussian vector, KKT_BWD_GPU {KKT_BWD_GPU:.3e}")
    assert ratios[best][0] >= POWER and best > 0
    assert bwd <= KKT_BWD_GPU and ratios[0][0] < 1.0


# ------------------------------------------------------------------ the lost-inertia cases
@pytest.mark.parametrize("order", ["oracle", "handle"])
@pytest.mark.parametrize("k", F.CLASS_TAILS)
def test_inertia_construction(k, order):
    """the lowered variables lie in the last k rows of the order; K keeps inertia (n, m) at rho = 10 - the twins' pivots say so
    too - and loses it at rho = 1e-3, where the oracle refuses the factor"""
    box = F.data("box")
    perm = F.orders("box", k)[order]
    bad, variables, amount = F.inertia_batch(perm, k)
    print(f"k = {k}: diagonal of P lowered by {amount} on variables {variables}")
    assert set(variables) <= set(perm[len(perm) - k:].tolist())
    assert np.array_equal(np.delete(bad["Px"], F.INERTIA_QP, 0), np.delete(box["Px"], F.INERTIA_QP, 0))
    (D, E, c), _ = F.oracle_scaling_and_order(bad, F.INERTIA_QP, F.INERTIA_RHO[0])
    n, m = box["n"], box["m"]
    for rho, keeps in zip(F.INERTIA_RHO, (True, False)):
        system = F.system_of(bad, F.INERTIA_QP, D, E, c, rho)
        assert (F.reduced_min_eig(system) > 0) == keeps
        eig = np.linalg.eigvalsh(system.K64())
        assert ((eig > 0).sum(), (eig < 0).sum()) == (n, m) or not keeps
        _, h, L, d = AF.ldl_solver(system.K64(), perm, 0).factor
        assert ((d > 0).sum() == n) == keeps and np.all(d[:h - k] != 0)
    lead = AF.ldl_solver(F.system_of(box, F.INERTIA_QP, D, E, c, F.INERTIA_RHO[1]).K64(), perm, 0).factor[3]
    assert np.array_equal(np.sign(d[:len(d) - k]), np.sign(lead[:len(d) - k]))      # the wrong pivots appear in the tail only
    with pytest.raises(ValueError):
        F.oracle_of(bad, F.INERTIA_QP, F.INERTIA_RHO[1])
