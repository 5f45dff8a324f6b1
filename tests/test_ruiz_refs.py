"""CPU: the equilibration reference of tests/ruiz_refs.py is right (mpmath, closed forms), its constants are the measured
ones, no case of the GPU tests sits at a discontinuity of the limit, the oracle lies within the bound in every case and path,
and the cases can see a wrong equilibration: every mutation of the fp64 twin lies >= 100 bounds away somewhere."""
import numpy as np
import pytest
import scipy.sparse as sp

import admm_refs as AF
import ruiz_refs as RR
from osqp_solver_amd import problems as PR

LD = RR.LD


def _pinned(measured, constant, what):
    """measured <= constant <= 2 x measured (0.0: exactly 0.0)"""
    if measured == 0.0:
        assert constant == 0.0, (what, constant)
    else:
        assert measured <= constant <= 2 * measured, (what, measured, constant)


# ------------------------------------------------------------------ the reference itself
def _small_cases():
    """n = 12, m = 20 with the limits: setup at every iteration count, and every kind of step"""
    base = RR.limit_values(PR.random_box_qp(RR.B, n=12, mg=8, nnz_per_row=3))
    sets = (base,) + tuple(RR.limit_values(PR.random_box_qp(RR.B, n=12, mg=8, nnz_per_row=3, value_seed=RR.OTHER_SEED + 1000 * k))
                           for k in (0, 1))
    for it in RR.ITERS:
        yield RR.Case(f"small_iters{it}", base, iters=it)
    for path in ("update_A_then_update_P", "update_P_A_then_update_A_bounds", "update_P_some_then_reinit_some",
                 "update_q_then_reinit_some"):
        yield RR.Case("small_" + path, base, path=path, sets=sets)


def test_reference_against_mpmath():
    worst = {k: 0.0 for k in RR.QUANTITIES}
    for case in _small_cases():
        assert (case.pr["n"], case.pr["m"]) == (12, 20)
        for b in range(case.B):
            ref, mp = case.model(b), case.model(b, "mp")
            assert [(w, i) for w, i, _ in ref.log] == [(w, i) for w, i, _ in mp.log]
            for k, e in RR.errors(ref.scaling(), mp, kind="mp").items():
                worst[k] = max(worst[k], e)
    print("long double against mpmath:", {k: f"{v:.3g}" for k, v in worst.items()})
    _pinned(max(worst.values()), RR.REF_ERROR, "REF_ERROR")
    smallest = min(v for row in RR.RUIZ_BOUND.values() for v in row.values() if v > 0)
    assert RR.REF_ERROR <= smallest / 100, (RR.REF_ERROR, smallest)         # the reference's own error: below 1 % of any bound


def test_closed_form_n1_m1():
    """P = [4], A = [1], q = [0.25]: D = 1/2 after the first iteration and for good; A_s = 1/2, then its square root each
    iteration, so E = 2 (1/2)^(1 / 2^(N - 1)); the cost factor is 1 throughout (P_s = 1, |q_s| = 1/8)."""
    import mpmath as mp
    pat = RR.Pattern(sp.csc_matrix(np.eye(1)), sp.csc_matrix(np.eye(1)))
    for N in RR.ITERS:
        r = RR.Ruiz(pat, N).setup([4.0], [1.0], [0.25])
        D, E, c = r.scaling()
        assert D[0] == 0.5 and c == 1.0
        with mp.workdps(RR.DPS):
            want = 2 * mp.mpf(0.5) ** (mp.mpf(1) / 2 ** (N - 1))
            assert abs(mp.mpf(float(E[0])) + mp.mpf(float(E[0] - LD(float(E[0])))) - want) <= 64 * mp.mpf(2) ** -64 * want, N


def test_closed_form_diagonal_P_identity_A():
    """P = diag(p), p_j >= 1, A = I, q = 0: D_j = p_j^(-1/2), E_j = p_j^(1/2 - 1/2^N), c = 1."""
    import mpmath as mp
    n = 7
    p = np.array([1.0, 1.5, 2.0, 9.0, 100.0, 4000.0, 1e4])
    pat = RR.Pattern(sp.csc_matrix(np.eye(n)), sp.csc_matrix(np.eye(n)))
    for N in RR.ITERS:
        r = RR.Ruiz(pat, N).setup(p, np.ones(n), np.zeros(n))
        D, E, c = r.scaling()
        assert c == 1.0
        with mp.workdps(RR.DPS):
            for j in range(n):
                pj = mp.mpf(float(p[j]))
                for got, want in ((D[j], pj ** mp.mpf(-0.5)), (E[j], pj ** (mp.mpf(0.5) - mp.mpf(1) / 2 ** N))):
                    got = mp.mpf(float(got)) + mp.mpf(float(got - LD(float(got))))
                    assert abs(got - want) <= 64 * mp.mpf(2) ** -64 * want, (N, j)


def test_the_restatement_agrees_with_the_dense_one_of_test_op_references():
    from test_op_references import _scale_data_restated
    c = RR.cases()["iters10_limits"]
    for b in range(c.B):
        P, A = PR.qp_matrices(c.pr, b)
        Dr, Er, cr = _scale_data_restated(P.toarray(), c.pr["q"][b], A.toarray())
        D, E, cc = c.model(b, "f64").scaling()
        np.testing.assert_allclose(D, Dr, rtol=1e-14, atol=0); np.testing.assert_allclose(E, Er, rtol=1e-14, atol=0)
        assert abs(cc - cr) <= 1e-14 * cr


# ------------------------------------------------------------------ the cases
def test_every_dispatch_class_and_limit_is_among_the_cases():
    cs = RR.cases()
    assert {c.form for c in cs.values()} == {"reg4", "reg8", "reg16", "reg32", "global"}
    assert RR.pa_len(cs["form_reg8_full"].pr) == 4096 and RR.pa_len(cs["form_reg16_by_one"].pr) == 4097
    assert RR.pa_len(cs["form_reg32_full"].pr) == 16384 and RR.pa_len(cs["form_global_by_one"].pr) == 16385
    g = cs["form_global"].pr
    assert RR.pa_len(g) > 16384 and g["n"] > 2048 and g["n"] % 2048
    for name in ("iters10_limits", "limits_global"):
        c = cs[name]
        D, E, cc = c.model(0).scaling()
        log = {(w, i): v for w, i, v in c.model(0).log}
        col, row = log[("col", 0)], log[("row", 0)]
        assert col[2] == 0 and row[2] == 0 and D[2] == 1 and E[2] == 1           # an empty column and an empty row
        assert col[5] == LD(1e-4) and col[8] == LD(5e-5) and row[5] == LD(1e-4)   # kept / becomes 1
        assert np.max(row) == LD(1e9) and np.any(row == LD(1e4))
        assert col[10] == LD(0.9)                                                # from the stored row 10 of triu(P)
        assert all(np.any((c.pr[k][0] == 0) & np.signbit(c.pr[k][0])) for k in ("Px", "Ax"))      # -0.0 among the values
        log4 = {(w, i): v for w, i, v in c.model(4).log}
        assert log4[("q", 0)][0] > 1e4 and log4[("c", 0)][0] == 1e4              # the cost factor saturates
        log1 = {(w, i): v for w, i, v in c.model(1).log}
        assert 1e-4 < log1[("q", 0)][0] < log1[("c", 0)][0] < 1                  # the mean decides c
        log2 = {(w, i): v for w, i, v in c.model(2).log}
        assert log2[("q", 0)][0] < 1e-4 and log2[("c", 0)][0] == 1 and c.model(2).scaling()[2] == 1


def test_no_case_is_near_a_threshold_of_the_limit():
    for name, case in RR.cases().items():
        for b in range(case.B):
            near = RR.near_values(case.model(b), case.model(b, "f64"))
            assert near == [], (name, b, near[:4])


def test_constants_are_the_measured_ones_and_the_oracle_is_within_the_bound():
    assert set(RR.RUIZ_TWIN_ERROR) == set(RR.cases())
    with RR.one_blas_thread():
        for name, case in RR.cases().items():
            measured = RR.measure_twins(case)
            print(name, {k: f"{v:.3g}" for k, v in measured.items()})
            for k in RR.QUANTITIES:
                _pinned(measured[k], RR.RUIZ_TWIN_ERROR[name][k], (name, k))
            for b in range(case.B):
                r, where = RR.ratio(RR.errors(case.oracle_scaling(b), case.model(b)), name)
                assert r <= 1.0, (name, b, r, where)
                assert r <= 1.0 / 32 + 1e-12


def test_update_q_leaves_the_scaling_alone_and_fresh_takes_the_q_in_force():
    c = RR.cases()["update_q_then_reinit_some_benign"]
    new_q = c.sets[1]["q"]
    for b in range(c.B):
        r = RR.Ruiz(c.pat, c.iters).setup(c.pr["Px"][b], c.pr["Ax"][b], c.pr["q"][b])
        before = [np.array(v, copy=True) for v in r.scaling()]
        r.update_q(new_q[b])
        for x, y in zip(before, r.scaling()):
            assert np.array_equal(x, y)
        r.fresh(c.sets[2]["Ax"][b])
        want = RR.Ruiz(c.pat, c.iters).setup(c.pr["Px"][b], c.sets[2]["Ax"][b], new_q[b])
        for x, y in zip(want.scaling(), r.scaling()):
            assert np.array_equal(x, y)


# ------------------------------------------------------------------ mutations
@pytest.mark.parametrize("mutation", RR.MUTATIONS)
def test_a_wrong_equilibration_is_at_least_100_bounds_away(mutation):
    worst, where = 0.0, None
    for name, case in RR.cases().items():
        if case.pr["n"] > 96:
            continue
        for b in range(case.B):
            r, k = RR.ratio(RR.errors(case.model(b, "f64", mutation).scaling(), case.model(b)), name)
            if r > worst:
                worst, where = r, (name, b, k)
    print(f"{mutation}: {worst:.3g} bounds at {where}")
    assert worst >= 100.0, (mutation, worst, where)


# ------------------------------------------------------------------ the ADMM checkpoint's sensitivity to the scaling
@pytest.mark.parametrize("path", RR.ADMM_SCENARIOS)
def test_admm_sensitivity_is_the_measured_one(path):
    measured = RR.measure_admm_sensitivity(path)
    print(path, {k: f"{v:.3g}" for k, v in measured.items()})
    for k in AF.KEYS:
        _pinned(measured[k], RR.ADMM_SENSITIVITY[path][k], (path, k))
    case = RR.admm_case(path)
    c = RR.cases()[path + "_benign"]
    for b in range(c.B):                                    # what the checkpoint presupposes (tests/test_gpu_admm_refs.py)
        ref = AF.reference(case, b, *RR.rounded(c.model(b)))[(0, RR.ADMM_K)]
        assert ref["term_margin"] > 1.0 and ref["rho_margin"] >= 1e-3 and ref["rho_updates"] == 0
