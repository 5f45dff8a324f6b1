"""CPU: the references of the polish step (tests/polish_refs.py): the float64 reference against its mpmath twin on the
problems the GPU tests use (the number behind POLISH_BOUND), what the GPU tests can tell apart at that bound (a
refinement round more or fewer, a flipped sign of either delta block), closed forms, the acceptance rule clause by clause,
the sign rule against the oracle, and the scenarios of tests/test_gpu_polish_refs.py with the oracle standing in for the
device's ADMM."""
import numpy as np
import pytest
import scipy.sparse as sp

import adjoint_refs as AR
import polish_refs as PF
from oracle import oracle as O

B = AR.GPU_B


@pytest.fixture(scope="module")
def fxs():
    pr = AR.gpu_problem()
    out = [AR.fixture(pr, b, key="gpu") for b in range(B)]
    for fx in out:
        AR.assert_preconditions(fx)
    return out


_ORACLE = {}


def oracle_run(fx, b, eps=None, **more):
    """(status, y, info, scaling) of the oracle on fixture b at eps (None: default tolerances); computed once"""
    key = (b, eps, tuple(sorted(more.items())))
    if key not in _ORACLE:
        kw = {} if eps is None else dict(eps_abs=eps, eps_rel=eps, max_iter=100000)
        o = O.OracleQPSolver(fx["P"], fx["q"], fx["A"], fx["l"], fx["u"], **{**kw, **more})
        st, _ = o.solve()
        i = o.info()
        _ORACLE[key] = dict(status=st, y=o.y.copy(), pri=i.pri_res, dua=i.dua_res, iter=i.iter, scaling=o.scaling())
    return _ORACLE[key]


_REF = {}


def ref(fxs, b, delta, k, signs=(1, -1)):
    key = (b, delta, k, signs)
    if key not in _REF:
        fx = fxs[b]
        D, E, c = oracle_run(fx, b)["scaling"]
        _REF[key] = PF.polish_ref(fx["P"], fx["q"], fx["A"], fx["l"], fx["u"], D, E, c, fx["act"], delta, k, signs=signs)
    return _REF[key]


def xscale(r):
    return r["scale"]["x"]


# ------------------------------------------------------------------ the twin error and the bound of the GPU tests
def test_twin_error_and_the_gpu_bound(fxs):
    worst, where = 0.0, None
    for b, fx in enumerate(fxs):
        D, E, c = oracle_run(fx, b)["scaling"]
        assert np.ptp(D) > 0 and np.ptp(E) > 0                    # (a real scaling)
        for delta in (1e-6, 1e-2):
            for k in (0, 3):
                twin = PF.polish_ref_mp(fx["P"], fx["q"], fx["A"], fx["l"], fx["u"], D, E, c, fx["act"], delta, k)
                e, key = PF.worst_ratio(ref(fxs, b, delta, k), twin)
                if e >= worst:
                    worst, where = e, (b, delta, k, key)
    print(f"polish twin error {worst:.3e} at {where}; POLISH_BOUND {PF.POLISH_BOUND:.1e}")
    assert worst <= PF.TWIN_ERROR, (worst, where)
    assert PF.POLISH_BOUND == max(32 * PF.TWIN_ERROR, 1e-13) and PF.POLISH_BOUND <= PF.MAX_BOUND


# ------------------------------------------------------------------ what the bound can tell apart
def test_a_round_more_or_fewer_is_a_thousand_bounds_away(fxs):
    """delta = 1e-2: x after k and after k + 1 rounds differ by >= 1000 POLISH_BOUND and by >= 2.5e-7 for k = 0 .. 3"""
    closest = np.inf
    for b in range(B):
        r = ref(fxs, b, 1e-2, 4)
        for k in range(4):
            d = np.max(np.abs(r["rounds"][k] - r["rounds"][k + 1])) / xscale(r)
            closest = min(closest, d)
            assert d >= 1000 * PF.POLISH_BOUND, (b, k, d)
    print(f"closest rounds at delta 1e-2: {closest:.2e}")
    assert closest >= 2.5e-7
    # delta = 1e-6 and 1e-4 without refinement against one round (what the delta cases of the GPU test would miss otherwise)
    for delta in (1e-6, 1e-4):
        for b in range(B):
            r = ref(fxs, b, delta, 1)
            d = np.max(np.abs(r["rounds"][0] - r["rounds"][1])) / xscale(r)
            assert d >= 1000 * PF.POLISH_BOUND, (delta, b, d)


@pytest.mark.parametrize("signs", [(-1, -1), (1, 1)], ids=["top_flipped", "bottom_flipped"])
def test_a_flipped_sign_of_a_delta_block_is_a_thousand_bounds_away(signs, fxs):
    """s_0 at delta 1e-6 and 1e-2, and every round the GPU test runs at delta 1e-2.  (After three rounds at delta 1e-6
    either sign converges to the same point: scenario S1 cannot see it, S2 and the delta cases can.)"""
    for b in range(B):
        for delta, ks in ((1e-6, (0,)), (1e-4, (0,)), (1e-2, (0, 1, 2, 3))):
            good, bad = ref(fxs, b, delta, 3), ref(fxs, b, delta, 3, signs)
            for k in ks:
                d = np.max(np.abs(good["rounds"][k] - bad["rounds"][k])) / xscale(good)
                assert d >= 1000 * PF.POLISH_BOUND, (b, delta, k, d)


def test_refinement_contracts_to_the_active_set_solution(fxs):
    """the error of round k against the exact active-set solution (mpmath, unscaled data) falls by >= 10 x per round until it
    reaches the twin error"""
    for b, fx in enumerate(fxs):
        x_mp, _ = AR.active_set_solution_mp(fx["P"], fx["q"], fx["A"], fx["l"], fx["u"], fx["act"])
        exact = np.array([float(v) for v in x_mp])
        sx = max(1.0, np.max(np.abs(exact)))
        for delta, rounds in ((1e-2, 10), (1e-6, 3)):
            r = ref(fxs, b, delta, rounds)
            err = [np.max(np.abs(x - exact)) / sx for x in r["rounds"]]
            assert 0.3 * delta <= err[0] <= 3 * delta, (b, delta, err[0])
            for k in range(rounds):
                assert err[k + 1] <= max(err[k] / 10, 4 * PF.TWIN_ERROR), (b, delta, k, err)
            assert err[-1] <= 4 * PF.TWIN_ERROR, (b, delta, err)


# ------------------------------------------------------------------ closed forms (no scaling: D = E = c = 1)
def _plain(Pd, q, Ad, l, u, act, delta, k, **kw):
    n, m = len(q), len(l)
    Ad = np.zeros((0, n)) if m == 0 else np.asarray(Ad, float)
    return PF.polish_ref(sp.csc_matrix(np.asarray(Pd, float)), np.asarray(q, float), sp.csc_matrix(Ad), np.asarray(l, float),
                         np.asarray(u, float), np.ones(n), np.ones(m), 1.0, np.asarray(act, np.int8), delta, k, scaling=0, **kw)


def test_closed_form_one_variable_one_row_active_at_u():
    p, q, a, u, d = 2.0, -3.0, 0.5, 0.4, 1e-2
    r = _plain([[p]], [q], [[a]], [-1.0], [u], [1], d, 0)
    det = (p + d) * d + a * a                                 # K_d = [[p + d, a], [a, -d]], b = [-q, u]
    x0, y0 = (a * u - d * q) / det, -((p + d) * u + a * q) / det
    assert abs(r["rounds"][0][0] - x0) <= 4e-16 * abs(x0)
    z = a * x0
    t = z + y0                                                # y0 > 0: the projection puts z on u and keeps t - u
    assert y0 > 0 and abs(r["y"][0] - (t - u)) <= 4e-16 * abs(t) and abs(r["pri"] - abs(z - u)) <= 4e-16
    assert abs(r["dua"] - abs(p * x0 + q + a * (t - u))) <= 1e-15 and abs(r["obj"] - (0.5 * p * x0 * x0 + q * x0)) <= 1e-15
    # refined: x = u / a, y = -(p x + q) / a, residuals of round-off
    r = _plain([[p]], [q], [[a]], [-1.0], [u], [1], d, 12)
    assert abs(r["x"][0] - u / a) <= 1e-15 and abs(r["y"][0] + (p * u / a + q) / a) <= 1e-14 and r["pri"] <= 1e-15 and r["dua"] <= 1e-14
    # the flipped signs give the other 2 x 2 formulas
    for s0, s1 in ((-1, -1), (1, 1)):                         # [[p + s0 d, a], [a, s1 d]]
        rs = _plain([[p]], [q], [[a]], [-1.0], [u], [1], d, 0, signs=(s0, s1))
        xs = (-s1 * d * q - a * u) / ((p + s0 * d) * s1 * d - a * a)
        assert abs(rs["rounds"][0][0] - xs) <= 1e-15 and abs(xs - x0) >= 1e-4


def test_closed_forms_no_rows_and_no_active_row():
    Pd = np.array([[2.0, 0.5], [0.5, 1.0]])
    q, d = np.array([1.0, -2.0]), 1e-2
    r = _plain(Pd, q, None, [], [], [], d, 0)
    want = -np.linalg.solve(Pd + d * np.eye(2), q)
    assert np.max(np.abs(r["x"] - want)) <= 1e-15 and r["pri"] == 0.0 and len(r["y"]) == 0
    assert abs(r["dua"] - np.max(np.abs(Pd @ r["x"] + q))) <= 1e-15 and r["dua"] >= 1e-3      # (P + dI) x = -q: dua = d |x|
    full = _plain(Pd, q, None, [], [], [], d, 12)
    assert np.max(np.abs(full["x"] + np.linalg.solve(Pd, q))) <= 1e-15 and full["dua"] <= 1e-15
    # rows, none active: the same x; y = 0 exactly; z = A x inside the bounds, so pri = 0 exactly
    Ad = np.array([[1.0, 1.0], [1.0, -1.0], [0.0, 0.0]])
    r2 = _plain(Pd, q, Ad, [-100.0] * 3, [100.0] * 3, [0, 0, 0], d, 0)
    assert np.array_equal(r2["x"], r["x"]) and np.all(r2["y"] == 0.0) and r2["pri"] == 0.0 and r2["dua"] == r["dua"]
    # a row that is not active and violated: the projection clips z, y takes what is left and pri = |A x - z| shows it
    r3 = _plain(Pd, q, Ad, [-100.0] * 3, [0.5, 100.0, 100.0], [0, 0, 0], d, 0)
    z = Ad @ r3["x"]
    assert z[0] > 0.5 and r3["y"][0] == z[0] - 0.5 and r3["pri"] == z[0] - 0.5 and r3["zs"][0] == 0.5


@pytest.mark.parametrize("q, side", [(0.6, -1), (-3.0, 1)], ids=["y_negative", "y_positive"])
def test_closed_form_equality_row(q, side):
    p, v = 2.0, 0.25                                          # l = u = v: x = v, y = -(p v + q), either side marked
    r = _plain([[p]], [q], [[1.0]], [v], [v], [side], 1e-6, 6)
    y = -(p * v + q)
    assert np.sign(y) == side
    assert abs(r["x"][0] - v) <= 1e-16 and abs(r["y"][0] - y) <= 1e-15 and r["pri"] <= 1e-16 and r["dua"] <= 1e-15
    other = _plain([[p]], [q], [[1.0]], [v], [v], [-side], 1e-6, 6)        # l = u: b is the same on the other side
    assert np.array_equal(other["x"], r["x"]) and np.array_equal(other["y"], r["y"])


def test_active_row_with_a_multiplier_of_the_wrong_sign():
    """row forced active at u = 1 while the free minimiser is 0.3: y_red = -(p + q) = -1.4 < 0 on an upper-active row.  The
    projection t = 1 - 1.4 = -0.4 lies inside [-1, 1]: z = t, y = 0, and pri = |A x - z| = 1.4, dua = |p x + q| = 1.4."""
    p, q = 2.0, -0.6
    r = _plain([[p]], [q], [[1.0]], [-1.0], [1.0], [1], 1e-6, 8)
    assert abs(r["x"][0] - 1.0) <= 1e-15 and r["y"][0] == 0.0
    assert abs(r["zs"][0] + 0.4) <= 1e-15 and abs(r["pri"] - 1.4) <= 1e-15 and abs(r["dua"] - 1.4) <= 1e-15
    assert PF.accept(r["pri"], r["dua"], 1e-4, 1e-4)[0] is False


def test_unscaling_rules():
    """scaled_termination = 0: |E^-1 pres|, |D^-1 dres| / c; scaled_termination = 1: the scaled norms; obj / c either way"""
    rng = np.random.default_rng(4)
    n, m = 3, 2
    Pd = np.diag([2.0, 1.0, 3.0]); Pd[0, 2] = Pd[2, 0] = 0.4
    Ad = rng.standard_normal((m, n)); q = rng.standard_normal(n)
    l, u = np.array([-1.0, -0.1]), np.array([0.05, 1.0])
    D, E, c = np.array([0.5, 2.0, 1.25]), np.array([4.0, 0.25]), 0.125
    act = np.array([1, 0], np.int8)
    args = (sp.csc_matrix(Pd), q, sp.csc_matrix(Ad), l, u, D, E, c, act, 1e-2, 0)
    un, sc = PF.polish_ref(*args), PF.polish_ref(*args, scaled_termination=1)
    assert np.array_equal(un["x"], sc["x"]) and np.array_equal(un["y"], sc["y"]) and un["obj"] == sc["obj"]
    x, y = un["x"], un["y"]                                   # caller space: the residuals of the unscaled problem
    z = np.clip(Ad @ x + y * 0, l, u)
    z[0] = u[0] if y[0] != 0 else z[0]
    assert abs(un["dua"] - np.max(np.abs(Pd @ x + q + Ad.T @ y))) <= 1e-14
    assert abs(un["pri"] - np.max(np.abs(Ad @ x - z))) <= 1e-14 and un["pri"] > 1e-6
    assert abs(un["obj"] - (0.5 * x @ Pd @ x + q @ x)) <= 1e-14
    xs, ys = x / D, c * y / E
    assert abs(sc["dua"] - np.max(np.abs(c * D * (Pd @ x + q + Ad.T @ y)))) <= 1e-14 and sc["dua"] != un["dua"]
    assert abs(sc["pri"] - np.max(np.abs(E * (Ad @ x - z)))) <= 1e-14 and sc["pri"] != un["pri"]
    assert np.allclose(xs, sc["xs"], rtol=1e-14, atol=0) and np.allclose(ys, sc["ys"], rtol=1e-13, atol=1e-18)


# ------------------------------------------------------------------ the acceptance rule
def test_acceptance_rule_clause_by_clause():
    T = PF.SMALL_RES
    # clause 1 alone: both residuals improve, neither ADMM residual is small
    assert PF.accept(1e-8, 1e-8, 1e-6, 1e-6)[::2] == (True, [1])
    assert PF.accept(1e-6, 1e-8, 1e-6, 1e-6)[0] is False and PF.accept(1e-8, 1e-6, 1e-6, 1e-6)[0] is False     # equality is not strict
    assert PF.accept(2e-6, 1e-8, 1e-6, 1e-6)[0] is False and PF.accept(1e-8, 2e-6, 1e-6, 1e-6)[0] is False
    # clause 2 alone: pri improves, dua does not, the ADMM's dua was below 1e-10
    assert PF.accept(1e-8, 5e-11, 1e-6, 4e-11)[::2] == (True, [2])
    assert PF.accept(1e-8, 5e-10, 1e-6, 4e-10)[0] is False                 # dua0 not small
    assert PF.accept(1e-8, 2e-10, 1e-6, T)[0] is False                     # dua0 exactly 1e-10: not below
    assert PF.accept(1e-6, 5e-11, 1e-6, 4e-11)[0] is False                 # pri equal
    # clause 3 alone: dua improves, pri does not, the ADMM's pri was below 1e-10
    assert PF.accept(5e-11, 1e-8, 4e-11, 1e-6)[::2] == (True, [3])
    assert PF.accept(5e-10, 1e-8, 4e-10, 1e-6)[0] is False
    assert PF.accept(2e-10, 1e-8, T, 1e-6)[0] is False                     # pri0 exactly 1e-10
    assert PF.accept(5e-11, 1e-6, 4e-11, 1e-6)[0] is False                 # dua equal
    assert PF.accept(0.9 * T, 1e-8, np.nextafter(T, 0), 1e-6)[::2] == (True, [1, 3])
    # margins: an acceptance by the comparison that holds it, a rejection by the cheapest clause to turn
    assert PF.accept(1e-8, 1e-9, 4e-8, 1e-6)[1] == pytest.approx(4.0)
    assert PF.accept(3e-6, 1e-8, 1e-6, 1e-6)[1] == pytest.approx(3.0)      # clause 1 needs pri only; 2 and 3 need far more
    assert PF.accept(1e-6, 1e-8, 1e-6, 1e-6)[1] == 1.0
    v, margin, holds = PF.accept(1e-8, 5e-11, 1e-6, 4e-11)
    assert margin == pytest.approx(2.5)                                    # clause 2: min(1e-6 / 1e-8, 1e-10 / 4e-11)
    assert PF.accept(0.0, 0.0, 1e-9, 1e-9)[:2] == (True, np.inf)


def test_sign_rule_counts_undecided_rows():
    act, und = PF.active_from_dual([0.0, 1e-16, -1e-16, 2e-3, -5.0, 5e-10, -2e-12, 1e-12], 1e-9)
    assert act.tolist() == [0, 0, 0, 1, -1, 0, 0, 0] and und == 2


@pytest.mark.parametrize("eps", [1e-3, 1e-5, 1e-7])
def test_sign_rule_against_the_oracle(eps, fxs):
    big_zero, small_mult = 0.0, np.inf
    for b, fx in enumerate(fxs):
        o = oracle_run(fx, b, eps)
        assert o["status"] == 1
        act, und = PF.active_from_dual(o["y"], PF.DUAL_FLOOR)
        assert und == 0 and np.array_equal(act, fx["act"]), (b, und)
        assert np.array_equal(act, AR.polish_rule(fx["A"], fx["x"], o["y"], fx["l"], fx["u"]))
        big_zero = max(big_zero, np.max(np.abs(o["y"][act == 0]), initial=0.0))
        small_mult = min(small_mult, np.min(np.abs(o["y"][act != 0])))
    print(f"eps {eps:g}: largest zero |y| {big_zero:.1e}, smallest multiplier {small_mult:.1e}")
    assert big_zero <= 1e-12 and small_mult >= 1e-4


# ------------------------------------------------------------------ the scenarios, the oracle standing in for the device's ADMM
def _scenario(name, fxs):
    sc = PF.SCENARIOS[name]
    delta = PF.DEFAULT_DELTA if sc["delta"] is None else sc["delta"]
    k = PF.DEFAULT_ROUNDS if sc["rounds"] is None else sc["rounds"]
    out = []
    for b, fx in enumerate(fxs):
        o = oracle_run(fx, b, sc["eps"])
        assert o["status"] == 1 and np.array_equal(PF.active_from_dual(o["y"])[0], fx["act"])
        r = ref(fxs, b, delta, k)
        out.append((r, o) + PF.accept(r["pri"], r["dua"], o["pri"], o["dua"]))
    print(name, [(v, f"{mg:.1e}", h) for _, _, v, mg, h in out])
    return out


def test_scenario_s1_all_accepted(fxs):
    assert all(v and mg >= 1e3 for _, _, v, mg, _ in _scenario("S1", fxs))


def test_scenario_s2_accepted_with_residuals_that_are_not_round_off(fxs):
    for r, o, v, mg, _ in _scenario("S2", fxs):
        assert v and mg >= 2
        assert 1e-7 <= r["pri"] <= 1e-5 and 1e-7 <= r["dua"] <= 1e-5
        assert r["pri"] >= 1e6 * PF.POLISH_BOUND * r["scale"]["pri"] and r["dua"] >= 1e6 * PF.POLISH_BOUND * r["scale"]["dua"]


def test_scenario_s6_accepted_with_residuals_that_are_not_round_off(fxs):
    for r, o, v, mg, _ in _scenario("S6", fxs):
        assert v and mg >= 2
        assert 1e-8 <= r["pri"] <= 1e-5 and 1e-8 <= r["dua"] <= 1e-5
        assert r["pri"] >= 1e5 * PF.POLISH_BOUND * r["scale"]["pri"] and r["dua"] >= 1e5 * PF.POLISH_BOUND * r["scale"]["dua"]


def test_scenario_s3_all_rejected_by_orders_of_magnitude(fxs):
    assert all(not v and mg >= 10 for _, _, v, mg, _ in _scenario("S3", fxs))
    assert min(mg for _, _, _, mg, _ in _scenario("S3", fxs)) >= 1e5


def test_scenario_s4_the_rule_at_small_admm_residuals(fxs):
    res = _scenario("S4", fxs)
    assert all(v and mg >= 2 for _, _, v, mg, _ in res)
    assert any(2 in h for *_, h in res) and any(3 in h for *_, h in res)          # a small dua0 and a small pri0 are among them
    assert [b for b, (_, o, *_) in enumerate(res) if o["pri"] < PF.SMALL_RES] == [0, 2, 3]
    assert [b for b, (_, o, *_) in enumerate(res) if o["dua"] < PF.SMALL_RES] == [5]


def test_scenario_s5_clauses_2_and_3_decide_alone(fxs):
    res = _scenario("S5", fxs)
    assert all(v and mg >= 2 for _, _, v, mg, _ in res)
    assert [h for *_, h in res] == [[3], [1], [3], [3], [1], [2]]


# ------------------------------------------------------------------ the other presuppositions of the GPU tests
def test_round_cases_one_accepted_case_per_round_count(fxs):
    """eps 1e-3.  The four ACCEPTED_ROUND_CASES - one per round count 0 .. 3 - are accepted for all six QPs with a margin of
    2 x, and in each the rounds k - 1, k + 1 and either flipped sign lie >= 1000 bounds away.  Of the remaining cases the rule
    rejects every QP at (1e-2, 0) and (1e-2, 1): nothing of them could be compared."""
    assert sorted(k for _, k in PF.ACCEPTED_ROUND_CASES) == [0, 1, 2, 3] and set(PF.ACCEPTED_ROUND_CASES) <= set(PF.ROUND_CASES)
    table = {}
    for delta, k in PF.ROUND_CASES:
        row = []
        for b, fx in enumerate(fxs):
            o = oracle_run(fx, b, PF.ROUND_EPS)
            assert o["status"] == 1 and np.array_equal(PF.active_from_dual(o["y"])[0], fx["act"])
            r = ref(fxs, b, delta, k + 1)
            at_k = ref(fxs, b, delta, k)
            assert np.array_equal(at_k["rounds"][k], r["rounds"][k])
            row.append(PF.accept(at_k["pri"], at_k["dua"], o["pri"], o["dua"]))
            if (delta, k) in PF.ACCEPTED_ROUND_CASES:
                others = [r["rounds"][k + 1]] + ([r["rounds"][k - 1]] if k else [])
                others += [ref(fxs, b, delta, k + 1, signs)["rounds"][k] for signs in ((-1, -1), (1, 1))]
                for other in others:
                    assert np.max(np.abs(r["rounds"][k] - other)) / xscale(r) >= 1000 * PF.POLISH_BOUND, (delta, k, b)
        table[(delta, k)] = row
        print(delta, k, [("A" if v else "R") + f"{mg:.3g}" for v, mg, _ in row])
    for case in PF.ACCEPTED_ROUND_CASES:
        assert all(v and mg >= 2 for v, mg, _ in table[case]), case
    for case in ((1e-2, 0), (1e-2, 1)):
        assert not any(v for v, _, _ in table[case]), case


@pytest.mark.parametrize("scen", ["S2", "S6"])
@pytest.mark.parametrize("kw", [dict(scaling=0), dict(scaled_termination=1)], ids=["scaling0", "scaled_termination"])
def test_scenarios_s2_and_s6_with_scaling_off_and_with_scaled_termination(kw, scen, fxs):
    sc = PF.SCENARIOS[scen]
    for b, fx in enumerate(fxs):
        o = oracle_run(fx, b, sc["eps"], **kw)
        assert o["status"] == 1 and np.array_equal(PF.active_from_dual(o["y"])[0], fx["act"])
        D, E, c = o["scaling"]
        if "scaling" in kw:
            assert np.all(D == 1.0) and np.all(E == 1.0) and c == 1.0
        r = PF.polish_ref(fx["P"], fx["q"], fx["A"], fx["l"], fx["u"], D, E, c, fx["act"], sc["delta"], sc["rounds"],
                          scaling=kw.get("scaling", 10), scaled_termination=kw.get("scaled_termination", 0))
        v, mg, _ = PF.accept(r["pri"], r["dua"], o["pri"], o["dua"])
        assert v and mg >= 2, (b, mg)


def test_partner_split_on_the_oracle(fxs):
    """PARTNER: with their rho and max_iter = 50 QPs 1 and 2 end at max_iter and the others optimal, with the fixture's active
    set by the sign rule and a default polish that the rule accepts"""
    P = PF.PARTNER
    for b, fx in enumerate(fxs):
        o = oracle_run(fx, b, P["eps"], max_iter=P["max_iter"], rho=P["rho"][b])
        assert o["status"] == P["status"][b], (b, o["status"])
        if o["status"] == 1:
            act, undecided = PF.active_from_dual(o["y"])
            assert undecided == 0 and np.array_equal(act, fx["act"])
            r = ref(fxs, b, PF.DEFAULT_DELTA, PF.DEFAULT_ROUNDS)
            v, mg, _ = PF.accept(r["pri"], r["dua"], o["pri"], o["dua"])
            assert v and mg >= 1e3
        else:
            assert o["iter"] == P["max_iter"]
    assert sorted(set(P["status"])) == [-2, 1]
