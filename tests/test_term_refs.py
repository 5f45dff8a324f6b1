"""CPU: the reference of the termination decision (tests/term_refs.py), before tests/test_gpu_term_refs.py holds the device to it.

The long-double reference against its mpmath twin; the errors of the two fp64 twins, per case (the only source of every bound);
the near rule with cap zero; every population the cases are there for, asserted from the ledger; the table of deliberate defects;
the CPU oracle taken through the same calls on every case; closed forms; and, as the statement of the gap, the margins by which
the older exit cases (tests/exit_cases.py) leave four of the five infeasibility clauses undecided."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import admm_refs as AF                                                          # noqa: E402
import cert_refs as CR                                                          # noqa: E402
import exit_cases as EC                                                         # noqa: E402
import op_refs as R                                                             # noqa: E402
import term_refs as T                                                           # noqa: E402
from osqp_solver_amd import problems as PR                                      # noqa: E402

CASES = list(T.cases())
S10 = ("s10_a", "s10_b", "s10_c", "s10_d", "close_on", "close_off", "rho", "ct0")       # scaling = 10, unscaled termination


def refs_of(name):
    """[(QP, [reference result of every solve])] with the oracle's scaling"""
    case = T.cases()[name]
    return [(b, T.reference(case, b, *case.oracle(b).scaling())) for b in range(case.B)]


def everything(names=CASES):
    for g in names:
        for b, rs in refs_of(g):
            for k, r in enumerate(rs):
                yield g, b, k, r


# ------------------------------------------------------------------ the reference itself
def small_cases():
    base = PR.random_box_qp(1, n=12, mg=8, nnz_per_row=3)
    st = dict(check_termination=5, adaptive_rho_interval=10, max_iter=40)
    return [T.TCase("small_pinf", T.pinf_qp(base, 0), dict(st, eps_prim_inf=1e-2), ("solve", "solve")),
            T.TCase("small_dinf", T.dinf_qp(base, 0, push=0.1), dict(st, eps_dual_inf=1e-6)),
            T.TCase("small_feas", EC.take(base, [0]), dict(st, max_iter=23, eps_abs=1e-7, eps_rel=1e-7))]


def test_reference_against_its_mpmath_twin():
    """n = 12, m = 20: a primal infeasible QP solved twice, a dual infeasible one and one that ends in the closing check, in long
    double and at 50 digits - the same exits, and the ledger, the published numbers and the certificates REF_ERROR apart at most"""
    worst = dict(clause=0.0, cert=0.0, res=0.0)
    seen = set()
    for case in small_cases():
        D, E, c = case.oracle(0).scaling()
        ld, mp = case.run(0, D, E, c), case.run(0, D, E, c, kind="mp")
        for a, m in zip(ld, mp):
            assert (a["status"], a["iter"], a["rho_updates"]) == (m["status"], m["iter"], m["rho_updates"]), case.name
            seen.add(a["status"])
            assert len(a["ledger"]) == len(m["ledger"])
            for ea, em in zip(a["ledger"], m["ledger"]):
                for cl, v in em["ratio"].items():
                    worst["clause"] = max(worst["clause"], T.ratio_distance(ea["ratio"][cl], v))
            keys = ("pri_res", "dua_res") + (("obj_val", "x", "y") if m["cert"] is None else ())
            worst["res"] = max([worst["res"]] + list(AF.errors(a, m, kind="mp", keys=keys).values()))
            if m["cert"] is not None:
                with AF.context("mp"):
                    worst["cert"] = max(worst["cert"], float(max(abs(AF._to_mp(s) - t) for s, t in zip(a["cert"], m["cert"]))))
    print("reference against mpmath:", {k: f"{v:.2e}" for k, v in worst.items()}, sorted(seen))
    assert {-3, -4} <= seen and seen & {2, -2}
    for k, v in worst.items():
        assert v <= T.REF_ERROR[k] <= 2 * v, (k, v, T.REF_ERROR[k])
    # far below every bound: the reference's own error is no part of one
    assert all(T.REF_ERROR[k] <= T.FLOOR / 3 for k in worst)                   # (and a bound is at least 32 round-offs)


@pytest.mark.parametrize("name", CASES)
def test_twin_errors_are_the_pinned_constants(name):
    clause, res, cert = T.measure_twins(T.cases()[name])
    got = dict(res, clause=clause, cert=cert)
    print(f"twin errors {name}:", {k: f"{v:.3e}" for k, v in got.items()})
    for k, v in got.items():
        const = T.TWIN[name][k]
        assert v <= const <= 2 * v, (name, k, v, const)
    assert T.CLAUSE_NEAR[name] == 32 * T.TWIN[name]["clause"]
    for k in T.RES_KEYS + ("cert",):                             # a bound is 32 x the constant; the named floors, and only they
        const = T.TWIN[name][k]
        bound = T.CERT_BOUND[name] if k == "cert" else T.RES_BOUND[name][k]
        floored = 0.0 < 32 * const < 2.0 ** -53
        assert ((name, k) in T.FLOORED) == floored, (name, k, const)
        assert bound == (32 * 2.0 ** -53 if floored else 32 * const), (name, k, bound)


def test_the_floored_entries_are_the_named_ones():
    assert sorted(T.FLOORED) == sorted((g, k) for g, row in T.TWIN.items() for k, v in row.items() if k != "clause" and 0.0 < 32 * v < 2.0 ** -53)


# ------------------------------------------------------------------ what the GPU tests presuppose
@pytest.mark.parametrize("name", CASES)
def test_no_ratio_and_no_rho_decision_is_near_and_the_unit_entry_is_decided(name):
    for b, rs in refs_of(name):
        for k, r in enumerate(rs):
            near, where = T.nearest(r)
            assert near > T.CLAUSE_NEAR[name], (name, b, k, near, where)
            assert r["rho_margin"] >= 1e-3, (name, b, k, r["rho_margin"])
            if r["cert"] is not None:
                assert T.cert_gap(r["cert"]) > T.CERT_BOUND[name], (name, b, k)
                assert float(np.max(np.abs(r["cert"]))) == 1.0
                assert float(r["obj_val"]) == (1e30 if r["status"] in (-3, 3) else -1e30)
                assert np.all(np.isnan(r["x"])) and np.all(np.isnan(r["y"]))


# ------------------------------------------------------------------ the populations
def deciders(names):
    """{clause: [(case, QP)]}: first solves whose exit check is the first at which that one clause holds (term_refs.decided_by)"""
    out = {}
    for g, b, k, r in everything(names):
        d = T.decided_by(r)
        if k == 0 and d is not None and len(d) == 1:
            out.setdefault(d[0], []).append((g, b))
    return out


def test_every_clause_decides_an_exit_alone():
    want = {"pri", "dua", "support", "atdy", "qdx", "pdx", "cone_u", "cone_l"}
    got = deciders(S10)
    print("decided alone, scaling = 10:", {k: v[:3] for k, v in got.items()})
    assert want <= set(got), want - set(got)
    for g in ("s0", "st"):
        one = deciders((g,))
        print(f"decided alone, {g}:", {k: v[:3] for k, v in one.items()})
        assert {"pri", "atdy"} <= set(one) and set(one) & {"qdx", "pdx", "cone_u", "cone_l"}, (g, set(one))
    assert "support" in deciders(("s0",)) and "qdx" in deciders(("s0",)) and "cone_u" in deciders(("st",))


def _bounds(name):
    pr = T.cases()["s10_b"].pr
    b = T.BATCH.index(name)
    return pr["l"][b], pr["u"][b]


def test_one_sided_rows_are_active():
    # primal: the projection changes norm_dy and its argmax (the scaled row, l alone) and the sign of the support-function sum
    b = T.BATCH.index("pinf2_norm")
    l, u = _bounds("pinf2_norm")
    assert l[T.NORM_ROW] > -1e29 and u[T.NORM_ROW] == 1e30
    r = dict(refs_of("s10_b"))[b][0]
    p = r["ledger"][-1]["projection"]
    assert r["status"] == -3 and p["norm_raw_over_norm"] > 2 and p["argmax_raw"] == T.NORM_ROW != p["argmax"]
    assert p["sum_negative"] and not p["sum_raw_negative"]
    r = dict(refs_of("s10_a"))[T.BATCH.index("pinf2_sided")][0]
    p = r["ledger"][-1]["projection"]
    assert r["status"] == -3 and p["sum_negative"] and not p["sum_raw_negative"]
    # dual: the cone clause decides, and its largest term - at the exit and at the check before, where it fails - is the scaled
    # row's, finite on one side only
    for name, side, clause in (("dinf2_scaled_u", 0, "cone_u"), ("dinf2_scaled_l", 1, "cone_l")):
        l, u = _bounds(name)
        assert (l[T.SCALED_ROW] == -1e30 and u[T.SCALED_ROW] < 1e29) if side == 0 else (u[T.SCALED_ROW] == 1e30 and l[T.SCALED_ROW] > -1e29)
        r = dict(refs_of("s10_b"))[T.BATCH.index(name)][0]
        assert r["status"] == -4 and T.decided_by(r) == (clause,)
        assert [e["cone_rows"][side] for e in r["ledger"][-2:]] == [T.SCALED_ROW] * 2
        assert r["ledger"][-2]["ratio"][clause] > 1 > r["ledger"][-1]["ratio"][clause] > 0


def test_the_closing_check_has_all_four_outcomes():
    seen = {}
    for g, b, k, r in everything(("close_on", "close_off", "ct0")):
        led = r["ledger"]
        if led[-1]["f"] != 10:
            continue
        assert r["iter"] == T.GROUPS[g]["max_iter"] and led[-2]["iter"] == led[-1]["iter"] and led[-2]["f"] == 1
        failed = [c for c, v in led[-2]["ratio"].items() if v >= 1]
        still = [c for c, v in led[-1]["ratio"].items() if v >= 1]
        assert failed and r["status"] in (2, 3, 4, -2)
        seen.setdefault(r["status"], []).append((g, b, failed, still))
    print("closing checks:", {k: v[0] for k, v in seen.items()})
    assert set(seen) == {2, 3, 4, -2}
    # max_iter on a check iteration, the cone clause violated at 1 x and clean at 10 x: the one clause between 0 and 4
    r = dict(refs_of("close_on"))[T.BATCH.index("dinf2_scaled_u")][0]
    one, ten = r["ledger"][-2]["ratio"], r["ledger"][-1]["ratio"]
    assert r["status"] == 4 and r["iter"] == 10 and T.GROUPS["close_on"]["check_termination"] == 10
    assert one["cone_u"] > 1 > ten["cone_u"] and all(one[c] < 1 for c in ("guard_dx", "qdx", "pdx", "cone_l"))


def test_rho_adaptation_and_no_checks_and_second_solves():
    adapted = [(b, r["iter"], r["rho_updates"]) for _, b, _, r in everything(("rho",)) if r["status"] in (-3, -4) and r["rho_updates"] >= 1]
    assert len(adapted) >= 2 and any(r[2] >= 2 for r in adapted), adapted
    assert all(len(r["ledger"]) <= 2 and r["iter"] == 60 for _, _, _, r in everything(("ct0",)))
    assert {-3, 3, -4, 2} <= {r["status"] for _, _, _, r in everything(("ct0",))}
    again = 0
    for b, rs in refs_of(T.AGAIN):
        assert len(rs) == 3
        if rs[0]["status"] in (-3, -4):                      # an infeasible exit cold-starts the QP and rho is fixed: the same solve again
            assert (rs[1]["status"], rs[1]["iter"]) == (rs[0]["status"], rs[0]["iter"])
            assert np.array_equal(rs[1]["cert"], rs[0]["cert"])
            again += rs[2]["status"] == 1
    assert again >= 4


# ------------------------------------------------------------------ the deliberate defects
@pytest.mark.parametrize("mutation", T.MUTATIONS)
def test_every_deliberate_defect_shows(mutation):
    eff = T.mutation_effects(mutation)
    exits = [e for e in eff if e[3] == "exit"]
    certs = [e for e in eff if e[3] == "cert"]
    print(f"defect {mutation}: {len(exits)} exits changed (first {exits[:1]}), {len(certs)} certificates moved by up to "
          f"{max([e[4] for e in certs], default=0.0):.3g} bounds")
    assert exits or certs, mutation


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", CASES)
def test_reference_against_the_oracle(name):
    case = T.cases()[name]
    worst, where, cworst = 0.0, None, 0.0
    for b, rs in refs_of(name):
        o = case.oracle(b)
        k = 0
        for s in case.solves:
            if s != "solve":
                o.update_bounds_only(s[1][b], s[2][b])
                continue
            st, x = o.solve()
            i, r = o.info(), rs[k]
            assert (st, i.iter, i.rho_updates) == (r["status"], r["iter"], r["rho_updates"]), (name, b, k, st, i.iter, r["status"], r["iter"])
            got = dict(pri_res=i.pri_res, dua_res=i.dua_res, obj_val=i.obj_val, x=x, y=o.y.copy())
            if r["cert"] is not None:
                assert i.obj_val == float(r["obj_val"]) and np.all(np.isnan(x)) and np.all(np.isnan(o.y))
                if k == 0 and r["iter"] >= 2:
                    kw = dict(case.settings)
                    v = CR.reference(case.pr, b, kw, st, int(i.iter))
                    CR.check_shape(v, case.pr, b, st, exact=False, tol=1e-12)
                    got["cert"] = v
                    cworst = max(cworst, T.cert_error(v, r) / T.CERT_BOUND[name])
            ratio, key = T.judge(case, got, r)
            if ratio >= worst:
                worst, where = ratio, (b, k, key)
            k += 1
    print(f"oracle against the reference, {name}: worst ratio {worst:.3f} at {where}; certificates {cworst:.3f}")
    assert worst <= 1.0, (name, worst, where)


# ------------------------------------------------------------------ closed forms
def test_two_rows_on_one_variable():
    """a_1 x in [1, 2], a_2 x in [-2, -1], a > 0: the certificate is (-a_2, a_1) / max(a) up to the tolerance of A'v"""
    case = T.cases()["n1m2_s0"]
    for b, rs in refs_of("n1m2_s0"):
        r = rs[0]
        a = case.pr["Ax"][b]
        want = np.array([-a[1], a[0]]) / max(a)
        assert r["status"] == -3 and np.max(np.abs(r["cert"].astype(float) - want)) <= 2 * 1e-4 / min(a), (b, r["cert"], want)
        assert float(r["obj_val"]) == 1e30


@pytest.mark.parametrize("name", ["m0_s0", "m0_s10"])
def test_no_rows_and_a_zero_column_of_p(name):
    """m = 0, P_kk = 0, q_k != 0: the certificate is -sign(q_k) e_k; the other entries decay with |P dx| < eps |dx|"""
    case = T.cases()[name]
    for b, rs in refs_of(name):
        r = rs[0]
        v = r["cert"].astype(float)
        q = case.pr["q"][b]
        assert r["status"] == -4 and float(r["obj_val"]) == -1e30 and r["y"].shape == (0,)
        assert v[2] == -np.sign(q[2]) and np.max(np.abs(np.delete(v, 2))) < 1e-4 * 10
        assert r["ledger"][-1]["ratio"]["cone_u"] == -np.inf and r["ledger"][-1]["ratio"]["pri"] == 0.0


# ------------------------------------------------------------------ the gap this file closes
def test_the_older_exit_cases_leave_four_clauses_undecided():
    """QP 0 of exit_cases' base, scaling = 0, a fixed rho, eps_*_inf = 1e-4: the margins by which the infeasibility clauses hold
    where the older cases exit (measured: q'dx 1e4 / 1e6, P dx 690 / 1.1e4, the cone clause 810 / 1.6e4 at the first check for a
    push of 1 / 100; the support-function clause 1.1e4 .. 1.6e4 at every check from 25 to 200) - no factor c, D^-1 or E^-1 below
    about 700 changes a status or an iteration count there"""
    base = PR.random_box_qp(EC.BASE_B, **EC.BASE_SHAPE)
    ones = (np.ones(base["n"]), np.ones(base["m"]), 1.0)
    st = dict(scaling=0, adaptive_rho=0)
    for push, lo in ((1.0, (5e3, 300, 400)), (100.0, (5e5, 5e3, 8e3))):
        r = T.TCase("old", EC.apply_kinds(EC.take(base, [0]), ["dinf"], push=push), st).run(0, *ones)[0]
        q = r["ledger"][0]["ratio"]
        margins = (1 / q["qdx"], 1 / q["pdx"], 1 / max(q["cone_u"], q["cone_l"]))
        print(f"dinf, push {push}: exit at {r['iter']}, margins q'dx {margins[0]:.3g}, P dx {margins[1]:.3g}, cone {margins[2]:.3g}")
        assert (r["status"], r["iter"]) == (-4, 25) and all(m > l_ for m, l_ in zip(margins, lo)), margins
    r = T.TCase("old", EC.apply_kinds(EC.take(base, [0]), ["pinf"]), dict(st, max_iter=200, eps_prim_inf=1e-300)).run(0, *ones)[0]
    sup = [1e-300 / 1e-4 / e["ratio"]["support"] for e in r["ledger"] if e["f"] == 1]
    print(f"pinf: margins of the support-function clause at the checks 25 .. 200: {min(sup):.3g} .. {max(sup):.3g}")
    assert len(sup) == 8 and 5e3 < min(sup) and max(sup) < 5e4
