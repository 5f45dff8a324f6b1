"""CPU: the references of tests/admm_refs.py, before tests/test_gpu_admm_refs.py holds the device to them.

The long-double reference against its mpmath twin (REF_ERROR); the errors of the two fp64 twins against the reference, per
scenario and quantity (TWIN_ERROR: the only source of ITERATE_BOUND); the reference against the CPU oracle - a correct fp64
implementation with another elimination order - at every case and checkpoint, which pins the reference's order of events;
the distance of every deliberate defect and of a neighbouring iteration from the reference, in bounds; what the GPU tests
presuppose of every case; closed forms."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import admm_refs as AF                                                          # noqa: E402
import op_refs as R                                                             # noqa: E402
from osqp_solver_amd import problems as PR                                      # noqa: E402

SCENARIOS = ("box", "early_rho", "continuation", "warm", "settings", "gomp", "edge")
SEPARATION = 1000.0


def oracle_scaling(case, b):
    o = AF.oracle_of(case, b)
    return o.scaling()


def ref_of(case, b):
    return AF.reference(case, b, *oracle_scaling(case, b))


def separation(a, ref, scenario):
    """the largest distance of a result from the reference over the quantities, in bounds of that quantity (quantities that
    must match exactly do not count)"""
    errs = AF.errors(a, ref)
    return max(e / AF.ITERATE_BOUND[scenario][k] for k, e in errs.items() if AF.ITERATE_BOUND[scenario][k] > 0.0)


# ------------------------------------------------------------------ the reference itself
def small_case():
    pr = PR.random_box_qp(1, n=12, mg=8, nnz_per_row=3)
    return AF.Case("small", "box", pr, dict(AF.EPS, check_termination=5, adaptive_rho_interval=10), (1, 10, 11, 30))


def test_reference_against_its_mpmath_twin():
    """n = 12, m = 20, 30 iterations, rho estimated every 10 and updated at least once: the long-double reference against the
    same rules at 50 digits.  Measured: x, y, z, the residuals and obj below 3e-19, rho 2.0e-17, rho_estimate 2.2e-15 (the
    residuals it divides have cancelled to 1e-4 of their terms by then) - each at least 50 x below its twin error in every scenario (x, y: 4000 x)."""
    case = small_case()
    D, E, c = oracle_scaling(case, 0)
    ld, mp = case.run(0, D, E, c), case.run(0, D, E, c, kind="mp")
    assert ld[(0, 30)]["rho_updates"] >= 1 and mp[(0, 30)]["rho_updates"] == ld[(0, 30)]["rho_updates"]
    assert [e[0] for e in ld[(0, 30)]["rho_events"]] == [10, 20, 30]
    worst = {}
    for key in ld:
        for k, e in AF.errors(ld[key], mp[key], kind="mp", keys=AF.KEYS + ("z",)).items():
            worst[k] = max(worst.get(k, 0.0), e)
    print("reference against mpmath:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= AF.REF_ERROR <= 2 * max(worst.values())
    # far below every twin error: the reference's own error is no part of a bound
    for sc in SCENARIOS:
        for k, v in AF.TWIN_ERROR[sc].items():
            assert v == 0.0 or worst[k] <= v / 50, (sc, k, worst[k], v)


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_twin_errors_are_the_pinned_constants(scenario):
    got = AF.measure_twins(scenario)
    print(f"twin errors {scenario}:", {k: f"{v:.3e}" for k, v in got.items()})
    for k in AF.KEYS:
        const = AF.TWIN_ERROR[scenario][k]
        assert got[k] <= const <= 2 * got[k], (scenario, k, got[k], const)
        assert AF.ITERATE_BOUND[scenario][k] == 32 * const
    if scenario == "box":                                        # the state of a correct fp64 ADMM lies 1e-14 from the exact one
        assert got["x"] < 1e-13 and got["y"] < 1e-13


# ------------------------------------------------------------------ the reference against the oracle
def oracle_results(case, b):
    """{(solve, k): result of the oracle taken through the case's calls} - warm_start_y is no call of the oracle's"""
    out = {}
    for k in case.ks:
        o = AF.oracle_of(case, b, max_iter=k)
        if case.warm_x is not None:
            o.set_warm_start(case.warm_x[b])
        keys = [(0, k)]
        res = [o.solve()]
        infos = [o.info()]
        ys = [o.y.copy()]
        if case.k2 is not None:
            if case.bounds is not None:
                o.update_bounds_only(case.bounds[0][b], case.bounds[1][b])
            keys.append((1, case.k2))
            res.append(o.solve()); infos.append(o.info()); ys.append(o.y.copy())
        for key, (st, x), i, y in zip(keys, res, infos, ys):
            out[key] = dict(status=st, iter=i.iter, rho_updates=i.rho_updates, x=x, y=y, pri_res=i.pri_res, dua_res=i.dua_res,
                            obj_val=i.obj_val, rho=i.rho, rho_estimate=i.rho_estimate)
    return out


@pytest.mark.parametrize("name", list(AF.cases()))
def test_reference_against_the_oracle(name):
    case = AF.cases()[name]
    worst, where = 0.0, None
    for b in range(case.B):
        D, E, c = oracle_scaling(case, b)
        ref = AF.reference(case, b, D, E, c) if case.warm_y is None else case.run(b, D, E, c, warm_y=False)
        got = oracle_results(case, b)
        assert set(got) == set(ref)
        for key, r in ref.items():
            g = got[key]
            assert (g["status"], g["iter"], g["rho_updates"]) == (-2, key[1], r["rho_updates"]), (name, b, key, g["status"], g["iter"])
            ratio, k = AF.judge(g, r, case.scenario)
            if ratio >= worst:
                worst, where = ratio, (b, key, k)
    print(f"oracle against the reference, {name}: worst ratio {worst:.3f} at {where}")
    assert worst <= 1.0, (name, worst, where)


# ------------------------------------------------------------------ preconditions of the GPU tests
@pytest.mark.parametrize("name", list(AF.cases()))
def test_no_termination_and_no_rho_decision_near_its_threshold(name):
    case = AF.cases()[name]
    for b in range(case.B):
        for key, r in ref_of(case, b).items():
            assert r["term_margin"] > 1.0, (name, b, key, r["term_margin"])        # tolerances 1e-12: status -2 at every checkpoint
            assert r["rho_margin"] >= 1e-3, (name, b, key, r["rho_margin"])


def test_update_patterns():
    cs = AF.cases()
    for b in range(AF.BOX_B):
        r = ref_of(cs["box"], b)
        assert [r[(0, k)]["rho_updates"] for k in cs["box"].ks] == [0, 0, 0, 0, 0, 1]
        assert [(it, up) for it, _, up in r[(0, 125)]["rho_events"]] == [(100, True)] and 0.585 <= r[(0, 125)]["rho"] <= 1.225
        e = ref_of(cs["early_rho"], b)[(0, 35)]
        assert [it for it, _, _ in e["rho_events"]] == [10, 20, 30]
        if b == 0:                                               # never: its estimates stay under 5 x 0.1
            assert e["rho_updates"] == 0 and max(v for _, v, _ in e["rho_events"]) < 0.5 and abs(e["rho_estimate"] - 0.443) < 1e-3
        else:
            assert e["rho_updates"] == 1 and 0.555 <= e["rho"] <= 0.795     # (0.56 .. 0.79 to two digits)
        for name in ("cont", "cont_bounds"):
            assert [v["rho_updates"] for v in ref_of(cs[name], b).values()] == [0, 0]
    a = AF.Admm(**cs["cont_bounds"].qp(0), D=np.ones(96), E=np.ones(160), c=1.0, scaling=0)
    before = a.rv.copy()
    a.update_bounds(cs["cont_bounds"].bounds[0][0], cs["cont_bounds"].bounds[1][0])
    changed = np.flatnonzero(a.rv != before)
    assert changed.tolist() == [AF.EQ_ROW] and a.rv[AF.EQ_ROW] == 1e3 * a.rho      # one row becomes an equality


# ------------------------------------------------------------------ sensitivity
def variant_of(case, b, variant):
    return case.run(b, *oracle_scaling(case, b), variant=variant)


@pytest.mark.parametrize("name", list(AF.cases()))
def test_next_iteration_is_far_away(name):
    """every case of the GPU tests; a continuation against a second solve of one iteration more"""
    case = AF.cases()[name]
    for b in range(case.B):
        D, E, c = oracle_scaling(case, b)
        ref = AF.reference(case, b, D, E, c)
        if case.k2 is None:
            nxt = case.run(b, D, E, c, ks=[k + 1 for k in case.ks])
            pairs = [((0, k + 1), (0, k)) for k in case.ks]
        else:
            longer = AF.Case(name, case.scenario, case.pr, case.settings, case.ks, k2=case.k2 + 1, bounds=case.bounds)
            nxt = longer.run(b, D, E, c)
            pairs = [((1, case.k2 + 1), (1, case.k2))]
        for a, r in pairs:
            sep = separation(nxt[a], ref[r], case.scenario)
            assert sep >= SEPARATION, (name, b, r, sep)


@pytest.mark.parametrize("name", list(AF.cases()))
def test_second_order_allowance_of_obj_is_nothing_where_obj_has_a_scale(name):
    """judge() takes x_bound^2 obj_quad off an obj difference (admm_refs.errors).  Outside the GOMP pattern - whose obj after
    one iteration is round-off squared - that is below 1e-20 of obj's scale at every checkpoint, 1e-6 of obj's own bound."""
    case = AF.cases()[name]
    xb = AF.ITERATE_BOUND[case.scenario]["x"]
    for b in range(case.B):
        for key, r in ref_of(case, b).items():
            allowance = float(r["scale"]["obj_quad"] * xb * xb / r["scale"]["obj_val"])
            if case.scenario != "gomp":
                assert allowance <= 1e-20, (name, b, key, allowance)
            else:
                assert key[1] == 1 or allowance <= 1e-20, (name, b, key, allowance)


@pytest.mark.parametrize("variant,name,keys", [
    ("stale_rho_inv", "box", [(0, 125)]), ("stale_rho_inv", "early_rho", [(0, 35)]),
    ("no_sigma_x", "box", [(0, 2), (0, 26), (0, 125)]), ("no_sigma_x", "set_sigma1e-3", [(0, 30)]), ("no_sigma_x", "gomp", [(0, 25)]),
    ("warm_z_zero", "warm_s10", [(0, 1), (0, 25)]), ("warm_z_zero", "warm_s0", [(0, 1), (0, 25)]), ("warm_z_zero", "gomp", [(0, 1)]),
    ("dua_no_cinv", "box", [(0, 26), (0, 125)]), ("dua_no_cinv", "early_rho", [(0, 35)])])
def test_deliberate_defects_are_far_away(variant, name, keys):
    case = AF.cases()[name]
    for b in range(case.B):
        ref, bad = ref_of(case, b), variant_of(case, b, variant)
        for key in keys:
            if variant == "stale_rho_inv" and ref[key]["rho_updates"] == 0:
                assert name == "early_rho" and b == 0            # (QP 0 never updates: nothing to keep)
                continue
            sep = separation(bad[key], ref[key], case.scenario)
            assert sep >= SEPARATION, (variant, name, b, key, sep)


# ------------------------------------------------------------------ closed forms
def one_qp(P, q, A, l, u, **kw):
    n, m = len(q), len(l)
    return AF.Admm(sp.csc_matrix(np.atleast_2d(P)), np.asarray(q, float), sp.csc_matrix(np.reshape(A, (m, n))), np.asarray(l, float),
                   np.asarray(u, float), np.ones(n), np.ones(m), 1.0, scaling=0, **AF.EPS, **kw)


def test_one_iteration_by_hand():
    """n = m = 1, P = 2, q = -3, A = 1.5, box [-1, 1], cold start: K = [[2 + sigma, 1.5], [1.5, -1 / rho]], rhs = [3; 0]"""
    p, q, a, rho, sigma, alpha = R.LD(2), R.LD(-3), R.LD(1.5), R.LD(0.1), R.LD(1e-6), R.LD(1.6)
    det = -(p + sigma) / rho - a * a
    xt, nu = (-q * (-1 / rho)) / det, (-a * -q) / det
    zt = nu / rho
    x1, zr = alpha * xt, alpha * zt
    z1 = min(max(zr, R.LD(-1)), R.LD(1))
    y1 = rho * (zr - z1)
    r = one_qp(2.0, [-3.0], [1.5], [-1.0], [1.0]).solve(1)[1]
    tol = 8 * R.LD(2) ** -63
    assert abs(r["x"][0] - x1) <= tol * abs(x1) and abs(r["z"][0] - z1) <= tol and abs(r["y"][0] - y1) <= tol * abs(y1)
    assert z1 == 1 and y1 > 0                                    # the upper bound is active after one step
    assert abs(r["pri_res"] - abs(a * x1 - z1)) <= tol * (abs(a * x1) + 1)
    assert abs(r["dua_res"] - abs(q + p * x1 + a * y1)) <= tol * (abs(q) + abs(p * x1) + abs(a * y1))
    assert abs(r["obj_val"] - (p * x1 * x1 / 2 + q * x1)) <= tol * (abs(p * x1 * x1) + abs(q * x1))
    assert (r["iter"], r["rho_updates"], float(r["rho"])) == (1, 0, 0.1)


def test_no_rows():
    """m = 0: pri_res is 0.0 and x after one iteration is alpha (P + sigma I)^-1 (-q)"""
    rng = np.random.default_rng(3)
    M = rng.standard_normal((4, 4))
    P, q = M @ M.T + np.eye(4), rng.standard_normal(4)
    r = one_qp(np.triu(P), q, np.zeros((0, 4)), [], []).solve(1)[1]
    want = 1.6 * np.linalg.solve(P + 1e-6 * np.eye(4), -q)
    assert r["pri_res"] == 0.0 and r["y"].shape == (0,)
    assert np.max(np.abs(r["x"].astype(float) - want)) <= 1e-14 * np.max(np.abs(want))
    assert float(r["rho_estimate"]) == R.OQ_RHO_MIN             # (a primal residual of 0: the estimate sits on its lower clamp)


def test_equality_and_free_rows():
    """a row with l = u has rho_vec = 1e3 rho, a free row RHO_MIN - and its y stays 0.0"""
    a = one_qp(np.diag([1.0, 2.0]), [1.0, -1.0], [[1.0, 1.0], [1.0, -1.0], [0.5, 2.0]], [0.3, -2e30, -1.0], [0.3, 2e30, 1.0])
    assert [float(v) for v in a.rv] == [1e3 * 0.1, R.OQ_RHO_MIN, 0.1]
    r = a.solve(7)[7]
    assert r["y"][1] == 0.0 and r["y"][0] != 0.0
    a2 = one_qp(np.diag([1.0, 2.0]), [1.0, -1.0], [[1.0, 1.0], [1.0, -1.0], [0.5, 2.0]], [0.3, -2e30, -1.0], [0.3, 2e30, 1.0], rho=2.0)
    assert [float(v) for v in a2.rv] == [2e3, R.OQ_RHO_MIN, 2.0]
