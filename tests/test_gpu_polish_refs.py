"""GPU (-m gpu): the polish step ("Solution polishing") on every launch form against the float64
reference of tests/polish_refs.py, whose own error tests/test_polish_refs.py pins (TWIN_ERROR; POLISH_BOUND = 32 x that with a
floor of 1e-13, in the term scales of polish_refs).

Every comparison uses the handle's own scaling() and the fixture's active set, which the device's polish_active() must
equal.  pri0 / dua0 of the acceptance rule come from a twin handle with polish = 0 whose ADMM is asserted to be the same
(iterations, rho updates, exit code).  A QP's verdict is DECIDED if the reference's verdict has a margin of 2 x (polish_refs.accept)
and does not change when the polished residuals move by the bound; then status_polish must equal it.  An accepted QP has
x, y, pri_res, dua_res and obj_val within the bound of the reference at the handle's (delta, rounds); a rejected one has all
five bit for bit the twin's.  A QP that is not decided must still be one or the other.

Scenarios (polish_refs.SCENARIOS): S1 eps 1e-7, delta 1e-6, 3 rounds; S2 eps 1e-3, delta 1e-6, 0 rounds (residuals of 1e-6:
the published scalars mean something); S3 eps 1e-9, delta 1e-4, 0 rounds (rejected by 5 orders); S4 eps 1e-9, default polish;
S5 eps 1e-9, delta 1e-3, 3 rounds (clauses 2 and 3 of the rule decide alone); S6 eps 1e-3, delta 1e-2, 3 rounds (residuals of
4e-8 .. 1e-6 as in S2, through three rounds).

The reference applies K_d^-1 exactly, so S2 and the cases with 0 or 1 rounds at delta <= 1e-4 hold the device to an accurate
single solve with the polish factor (kernels.hip reduced_solve_refine, `inner`).  The measured ratios are in
DESIGN.md section 6."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_refs as AR                                                       # noqa: E402
import exit_cases as EC                                                         # noqa: E402
import osqp_solver_amd as M                                                     # noqa: E402
import polish_refs as PF                                                        # noqa: E402
from osqp_solver_amd import problems as PR                                      # noqa: E402
from test_gpu_adjoint import FORMS as ADJOINT_FORMS                             # noqa: E402
from test_gpu_ops import _env, edge_qp, tiny_qp                                 # noqa: E402

pytestmark = pytest.mark.gpu
BOUND = PF.POLISH_BOUND
FORMS = list(ADJOINT_FORMS) + [("tile1_t512", 1, {"MI_OSQP_THREADS": "512"}, 6), ("tile2_t512", 2, {"MI_OSQP_THREADS": "512"}, 6),
                               ("tile4_B5", 4, {}, 5)]
FORM = {f[0]: f for f in FORMS}


@pytest.fixture(scope="module")
def refs():
    """the problems and their fixtures (asserted): computed once, never changed"""
    pr = AR.gpu_problem()
    fxs = [AR.fixture(pr, b, key="gpu") for b in range(AR.GPU_B)]
    for fx in fxs:
        AR.assert_preconditions(fx)
    return dict(pr=pr, fx=fxs)


def form_env(monkeypatch, form):
    name, BT, env, B = form
    monkeypatch.delenv("MI_OSQP_THREADS", raising=False)
    _env(monkeypatch, BT, env)
    return BT, env, B


def make(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def pair(pr, settings, prepare=None):
    """(handle, its twin with polish = 0), both solved; the twin's ADMM is the handle's"""
    s, twin = make(pr, **settings), make(pr, **{**settings, "polish": 0})
    for h in (s, twin):
        if prepare is not None:
            prepare(h)
    info, i0 = s.solve(), twin.solve()
    assert [(a.iter, a.rho_updates, a.exit_code) for a in info] == [(a.iter, a.rho_updates, a.exit_code) for a in i0]
    assert all(a.status_polish == 0 for a in i0)
    return s, twin, info, i0


def form_asserts(s, BT, env):
    st = s.stats()
    if BT:
        assert st["tile"] == BT
    if "MI_OSQP_THREADS" in env:
        assert st["threads_per_block"] == int(env["MI_OSQP_THREADS"])
    if env.get("MI_OSQP_GROUPS", "0") != "0":
        assert st["solve_groups"] == int(env["MI_OSQP_GROUPS"])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def state(s):
    return dict(x=s.primal(), y=s.dual(), info=[bytes(i) for i in s.info()])


_REF = {}


def reference(fx, act, D, E, c, st):
    key = (fx["P"].data.tobytes(), fx["A"].data.tobytes(), fx["q"].tobytes(), fx["l"].tobytes(), fx["u"].tobytes(), act.tobytes(),
           D.tobytes(), E.tobytes(), float(c), st.delta, st.polish_refine_iter, st.scaling, st.scaled_termination)
    if key not in _REF:
        _REF[key] = PF.polish_ref(fx["P"], fx["q"], fx["A"], fx["l"], fx["u"], D, E, c, act, st.delta, int(st.polish_refine_iter),
                                  int(st.scaling), int(st.scaled_termination))
    return _REF[key]


def judge(s, twin, info, i0, fxs, label, qps=None, acts=None):
    """every QP of qps against the reference (module docstring).  fxs[b]: the data (and, without acts, the active set) of
    QP b.  Returns dict(worst ratio, verdicts {b: True | False}, undecided [b])."""
    qps = range(s.B) if qps is None else qps
    D, E, c = s.scaling()
    st = s.settings()
    x, y, x0, y0 = s.primal(), s.dual(), twin.primal(), twin.dual()
    dev_act = s.polish_active()
    worst, where, verdicts, undecided = 0.0, None, {}, []
    for b in qps:
        fx = fxs[b]
        act = fx["act"] if acts is None else acts[b]
        assert info[b].status_val == 1, (label, b, info[b].status_val)
        np.testing.assert_array_equal(dev_act[b], act, err_msg=f"{label}: active set of QP {b}")
        r = reference(fx, act, D[b], E[b], c[b], st)
        p0, d0 = i0[b].pri_res, i0[b].dua_res
        v, margin, holds = PF.accept(r["pri"], r["dua"], p0, d0)
        tp, td = BOUND * r["scale"]["pri"], BOUND * r["scale"]["dua"]
        stable = all(PF.accept(max(r["pri"] + sp, 0.0), max(r["dua"] + sd, 0.0), p0, d0)[0] == v for sp in (-tp, tp) for sd in (-td, td))
        got = info[b].status_polish
        verdicts[b] = v
        if margin >= 2 and stable:
            assert got == (1 if v else -1), (label, b, got, v, margin, holds, r["pri"], r["dua"], p0, d0)
        else:
            undecided.append(b)
            print(f"polish {label}: QP {b} not decided (reference {v}, margin {margin:.3g}, stable {stable}, device {got})")
            assert got in (1, -1), (label, b, got)
        if got == 1:
            e, k = PF.worst_ratio(dict(x=x[b], y=y[b], pri=info[b].pri_res, dua=info[b].dua_res, obj=info[b].obj_val), r)
            if e >= worst:
                worst, where = e, (b, k)
        else:
            assert same_bits(x[b], x0[b]) and same_bits(y[b], y0[b]), (label, b)
            assert (info[b].pri_res, info[b].dua_res, info[b].obj_val) == (i0[b].pri_res, i0[b].dua_res, i0[b].obj_val), (label, b)
    print(f"polish {label}: worst ratio {worst:.3e} at {where} (bound {BOUND:.1e}); accepted "
          f"{[b for b in qps if info[b].status_polish == 1]}, undecided {undecided}")
    assert worst <= BOUND, (label, worst, where)
    return dict(worst=worst, verdicts=verdicts, undecided=undecided)


def next_solve(s, twin, info):
    """the polished point is the next warm start: an accepted QP ends at its first termination check; a QP that was not
    accepted runs the iterations of the twin"""
    i2, t2 = s.solve(), twin.solve()
    for b, a in enumerate(info):
        if a.status_polish == 1:
            assert i2[b].iter == s.settings.check_termination and i2[b].exit_code == 0, (b, i2[b].iter)
        else:
            assert (i2[b].iter, i2[b].exit_code) == (t2[b].iter, t2[b].exit_code), (b, i2[b].iter, t2[b].iter)


# ------------------------------------------------------------------ a. every launch form
@pytest.mark.parametrize("scen", ["S1", "S2", "S6"])
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_every_launch_form_against_the_reference(form, scen, refs, monkeypatch):
    BT, env, B = form_env(monkeypatch, form)
    pr = EC.take(refs["pr"], np.arange(B))
    settings = PF.scenario_settings(scen)
    s, twin, info, i0 = pair(pr, settings)
    form_asserts(s, BT, env)
    assert [i.status_val for i in info] == [1] * B and [i.status_polish for i in info] == [1] * B
    res = judge(s, twin, info, i0, refs["fx"], f"{form[0]} {scen}")
    assert res["undecided"] == [] and all(res["verdicts"].values())
    first = state(s)
    next_solve(s, twin, info)
    fresh = make(pr, **settings)                                # a repeated fresh handle: the same bits
    fresh.solve()
    again = state(fresh)
    assert same_bits(first["x"], again["x"]) and same_bits(first["y"], again["y"]) and first["info"] == again["info"]
    for h in (s, twin, fresh):
        h.close()


# ------------------------------------------------------------------ b. refinement rounds and delta
@pytest.mark.parametrize("case", PF.ROUND_CASES, ids=lambda c: f"delta{c[0]:g}_k{c[1]}")
@pytest.mark.parametrize("BT", [0, 4], ids=["default", "tile4"])
def test_refinement_rounds_and_delta(BT, case, refs, monkeypatch):
    """x of an accepted QP is the reference's round-k result; tests/test_polish_refs.py shows that k +- 1 or a flipped sign of
    either delta block lies >= 1000 bounds away in every ACCEPTED_ROUND_CASE.  At eps 1e-3 the rule accepts all six QPs in
    those four cases - which is asserted - and rejects most of them at delta 1e-2 with 0, 1 or 2 rounds and at delta 1e-4
    with none (their residuals, delta |x| and delta |y| after round 0, are above the ADMM's): there the verdict is checked,
    and the rejected QPs bit for bit."""
    _env(monkeypatch, BT, {})
    delta, k = case
    s, twin, info, i0 = pair(refs["pr"], dict(polish=1, eps_abs=PF.ROUND_EPS, eps_rel=PF.ROUND_EPS, delta=delta, polish_refine_iter=k))
    if BT:
        assert s.stats()["tile"] == BT
    got = s.settings()
    assert (got.delta, got.polish_refine_iter) == (delta, k)
    res = judge(s, twin, info, i0, refs["fx"], f"tile {BT} delta {delta:g} k {k}")
    if case in PF.ACCEPTED_ROUND_CASES:
        assert res["undecided"] == [] and all(res["verdicts"].values()) and [i.status_polish for i in info] == [1] * s.B
    else:
        assert len(res["undecided"]) < s.B                       # (something was decided)
    s.close(); twin.close()


# ------------------------------------------------------------------ c. rejections
@pytest.mark.parametrize("name", ["tile1", "tile2", "tile4", "gx_groups16"])
def test_rejected_polish_changes_nothing(name, refs, monkeypatch):
    BT, env, B = form_env(monkeypatch, FORM[name])
    pr = EC.take(refs["pr"], np.arange(B))
    s, twin, info, i0 = pair(pr, PF.scenario_settings("S3"))
    form_asserts(s, BT, env)
    assert [i.status_val for i in info] == [1] * B and [i.status_polish for i in info] == [-1] * B
    res = judge(s, twin, info, i0, refs["fx"], f"{name} S3")
    assert res["undecided"] == [] and not any(res["verdicts"].values())
    assert s.last_polish_stats()["polished"] == B and s.last_polish_stats()["accepted"] == 0
    a, b = state(s), state(twin)
    assert same_bits(a["x"], b["x"]) and same_bits(a["y"], b["y"])
    for ia, ib in zip(info, i0):
        assert (ia.pri_res, ia.dua_res, ia.obj_val, ia.iter, ia.rho) == (ib.pri_res, ib.dua_res, ib.obj_val, ib.iter, ib.rho)
    next_solve(s, twin, info)                                    # (the same iterations as the twin's next solve)
    s.close(); twin.close()


# ------------------------------------------------------------------ d. the rule
@pytest.mark.parametrize("scen", ["S4", "S5"])
@pytest.mark.parametrize("BT", [2, 4])
def test_acceptance_rule_at_small_admm_residuals(BT, scen, refs, monkeypatch):
    """S4: pri0 or dua0 below 1e-10 for some QPs (clauses 2 and 3 hold beside clause 1); S5: the polished residuals lie
    beside the ADMM's, so that clause 3 alone accepts QPs 0, 2, 3 and clause 2 alone QP 5 on the oracle stand-in.  The
    device's own ADMM residuals decide here; a QP whose verdict is not decided is printed, at most one of the six."""
    _env(monkeypatch, BT, {})
    s, twin, info, i0 = pair(refs["pr"], PF.scenario_settings(scen))
    assert s.stats()["tile"] == BT and [i.status_val for i in info] == [1] * s.B
    got = s.settings()
    if scen == "S4":
        assert (got.delta, got.polish_refine_iter) == (PF.DEFAULT_DELTA, PF.DEFAULT_ROUNDS)
    res = judge(s, twin, info, i0, refs["fx"], f"tile {BT} {scen}")
    assert len(res["undecided"]) <= 1
    small = [b for b in range(s.B) if i0[b].pri_res < PF.SMALL_RES or i0[b].dua_res < PF.SMALL_RES]
    print(f"polish tile {BT} {scen}: QPs with pri0 or dua0 below 1e-10: {small}; status_polish {[i.status_polish for i in info]}")
    assert small                                                 # clauses 2 and 3 are live
    if scen == "S4":                                             # (S5 leaves residuals of 1e-10 .. 1e-9 at eps 1e-9: its next solve iterates)
        next_solve(s, twin, info)
    s.close(); twin.close()


# ------------------------------------------------------------------ e. scaling
@pytest.mark.parametrize("scen", ["S2", "S6"])
@pytest.mark.parametrize("kw", [dict(scaling=0), dict(), dict(scaled_termination=1)], ids=["scaling0", "default", "scaled_termination"])
def test_scaling_off_on_and_scaled_termination(kw, scen, refs, monkeypatch):
    _env(monkeypatch, 0, {})
    s, twin, info, i0 = pair(refs["pr"], {**PF.scenario_settings(scen), **kw})
    assert [i.status_val for i in info] == [1] * s.B and [i.status_polish for i in info] == [1] * s.B
    D, E, c = s.scaling()
    if kw.get("scaling", 1) == 0:
        assert np.all(D == 1.0) and np.all(E == 1.0) and np.all(c == 1.0)
    res = judge(s, twin, info, i0, refs["fx"], scen + " " + ("+".join(f"{k}={v}" for k, v in kw.items()) or "default"))
    assert res["undecided"] == [] and all(res["verdicts"].values())
    if kw.get("scaled_termination"):
        # the published residuals are the scaled ones: they differ from the unscaled ones of the same point by far more than the bound
        st = s.settings()
        for b in range(s.B):
            fx = refs["fx"][b]
            un = PF.polish_ref(fx["P"], fx["q"], fx["A"], fx["l"], fx["u"], D[b], E[b], c[b], fx["act"], st.delta, int(st.polish_refine_iter))
            assert abs(info[b].pri_res - un["pri"]) >= 1e3 * BOUND * un["scale"]["pri"], b
            assert abs(info[b].dua_res - un["dua"]) >= 1e3 * BOUND * un["scale"]["dua"], b
    s.close(); twin.close()


# ------------------------------------------------------------------ f. a tile partner that is not polished
@pytest.mark.parametrize("BT", [2, 4])
def test_a_tile_partner_that_is_not_polished(BT, refs, monkeypatch):
    """One handle, max_iter = 50: update_rho_each gives QPs 1 and 2 a rho with which they run into max_iter while their tile
    partners end optimal and are polished (polish_refs.PARTNER; the split is confirmed on the oracle by
    tests/test_polish_refs.py)."""
    _env(monkeypatch, BT, {})
    P = PF.PARTNER
    settings = dict(polish=1, eps_abs=P["eps"], eps_rel=P["eps"], max_iter=P["max_iter"])
    s, twin, info, i0 = pair(refs["pr"], settings, prepare=lambda h: h.update_rho_each(P["rho"]))
    assert s.stats()["tile"] == BT
    assert [i.status_val for i in info] == P["status"], [i.status_val for i in info]
    rest = [b for b in range(s.B) if P["status"][b] != 1]
    done = [b for b in range(s.B) if P["status"][b] == 1]
    a, t = state(s), state(twin)
    for b in rest:                                               # not polished: everything of theirs is the twin's
        assert info[b].status_polish == 0 and not s.polish_active()[b].any()
        assert same_bits(a["x"][b], t["x"][b]) and same_bits(a["y"][b], t["y"][b]) and a["info"][b] == t["info"][b], b
    acts = {}
    for b in done:
        acts[b], undecided_rows = PF.active_from_dual(t["y"][b], PF.DUAL_FLOOR)
        assert undecided_rows == 0, b
        np.testing.assert_array_equal(acts[b], refs["fx"][b]["act"])
    res = judge(s, twin, info, i0, refs["fx"], f"tile {BT} partner", qps=done, acts=acts)
    assert res["undecided"] == [] and all(res["verdicts"].values()) and [info[b].status_polish for b in done] == [1] * len(done)
    assert s.last_polish_stats()["polished"] == len(done)
    # the ADMM iterates of the mixed tiles (polish_kernel writes x, z, y of marked QPs only): the polished QPs start the next
    # solve from the polished point and end at its first check, QPs 1 and 2 run the iterations of the twin's next solve
    next_solve(s, twin, info)
    a2, t2, i2 = state(s), state(twin), s.info()
    for b in rest:
        assert i2[b].status_polish == 0, (b, i2[b].status_val)   # (still not optimal: 50 more iterations at rho = 1e-3)
        assert same_bits(a2["x"][b], t2["x"][b]) and same_bits(a2["y"][b], t2["y"][b]) and a2["info"][b] == t2["info"][b], b
    s.close(); twin.close()


# ------------------------------------------------------------------ g. edge shapes through BatchSolver
def _edge_problem(name):
    if name == "n1_m2":
        return tiny_qp(5, 1, 2)
    if name == "n4_m0":
        return tiny_qp(5, 4, 0)
    pr = edge_qp()                  # variable 2 has no entry in P and none in A: q_2 = 0 keeps the QP bounded (x_2 = 0), and
    pr["q"][:, 2] = 0.0             # K_d holds that variable by delta alone
    return pr


@pytest.mark.parametrize("scaling", [0, 10])
@pytest.mark.parametrize("name", ["n1_m2", "n4_m0", "empty_row_and_columns"])
def test_edge_shapes(name, scaling, monkeypatch):
    """Active set from the twin's dual by the sign rule; a QP with an undecided row is excluded (at most one per shape)."""
    _env(monkeypatch, 0, {})
    pr = _edge_problem(name)
    B, n, m = pr["Px"].shape[0], pr["n"], pr["m"]
    s, twin, info, i0 = pair(pr, dict(polish=1, eps_abs=1e-7, eps_rel=1e-7, scaling=scaling))
    assert [i.status_val for i in info] == [1] * B
    y0 = twin.dual()
    fxs, acts, qps = {}, {}, []
    for b in range(B):
        P, A = PR.qp_matrices(pr, b)
        fxs[b] = dict(P=P, A=A, q=pr["q"][b], l=pr["l"][b], u=pr["u"][b])
        acts[b], undecided_rows = PF.active_from_dual(y0[b], PF.DUAL_FLOOR)
        if undecided_rows == 0:
            qps.append(b)
    assert len(qps) >= B - 1, qps
    res = judge(s, twin, info, i0, fxs, f"edge {name} scaling={scaling}", qps=qps, acts=acts)
    x, y = s.primal(), s.dual()
    accepted = [b for b in qps if info[b].status_polish == 1]
    assert len(res["undecided"]) <= 1, res["undecided"]
    assert all(res["verdicts"][b] for b in qps if b not in res["undecided"]), res["verdicts"]       # every decided QP is accepted
    assert len(accepted) >= len(qps) - 1, (name, [i.status_polish for i in info], res)
    for b in accepted:
        if m == 0:
            assert info[b].pri_res == 0.0
        if name == "empty_row_and_columns":
            assert acts[b][1] == 0 and y[b, 1] == 0.0 and x[b, 2] == 0.0
    if m == 0:                                                   # no row: clause 3 (pri0 = 0) accepts whatever improves dua
        assert all(i.pri_res == 0.0 for i in i0)
        st = s.settings()
        D, E, c = s.scaling()
        # x is the refined solve with P + delta I alone, restated densely.  judge() has held x to 1 x the bound of the reference
        # already; this second restatement rounds on its own, hence 2 x between it and the device.
        for b in accepted:
            Pd = AR.sym_dense(fxs[b]["P"])
            sc = D[b][:, None] * Pd * D[b][None, :] * c[b]
            K, rhs = sc + st.delta * np.eye(n), -c[b] * D[b] * fxs[b]["q"]
            v = np.linalg.solve(K, rhs)
            for _ in range(int(st.polish_refine_iter)):
                v = v + np.linalg.solve(K, rhs - sc @ v)
            assert np.max(np.abs(x[b] - D[b] * v)) <= 2 * BOUND * max(1.0, np.max(np.abs(x[b]))), b    
    s.close(); twin.close()
