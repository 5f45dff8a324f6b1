"""GPU (-m gpu): the ADMM iterates of the device (kernels.hip iterate_body E6-E10, check_body E11-E14 and the refactorisation a
rho update triggers) against the long-double reference of tests/admm_refs.py, on every launch form.

A solve with max_iter = k and tolerances it cannot meet (1e-12) ends with status -2 and publishes the state after exactly k
iterations: x, y and the closing check's pri_res, dua_res, obj_val, rho, rho_estimate and rho_updates.  Every case builds the
reference from the handle's own scaling() (computed once per case, QP and scaling; shared by the forms), asserts iter == k,
status -2 and the reference's count of rho updates, and requires the seven quantities within ITERATE_BOUND of their scenario -
32 x the error of the fp64 twins, per quantity (tests/test_admm_refs.py pins it) - in the term scales of admm_refs.  No QP is
skipped.  What the cases presuppose (no termination test met, no rho decision near its threshold) is asserted of every
reference used here and, with the oracle's scaling, on the CPU.  The measured ratios are in DESIGN.md section 6."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import admm_refs as AF                                                          # noqa: E402
from test_gpu_polish_refs import FORM, FORMS, form_asserts, form_env, make      # noqa: E402

pytestmark = pytest.mark.gpu
FEW = ["tile1", "tile2", "tile4", "tail64", "tail0"]


def published(s, info):
    x, y = s.primal(), s.dual()
    return [dict(x=x[j], y=y[j], pri_res=i.pri_res, dua_res=i.dua_res, obj_val=i.obj_val, rho=i.rho, rho_estimate=i.rho_estimate)
            for j, i in enumerate(info)]


def compare(s, info, case, key, label, qps=None):
    """every QP of the handle (qps: their indices in the case) against the reference at key = (solve, k); the worst ratio"""
    qps = list(range(s.B)) if qps is None else qps
    D, E, c = s.scaling()
    got = published(s, info)
    worst, where, ex, ey = 0.0, None, 0.0, 0.0
    for j, b in enumerate(qps):
        ref = AF.reference(case, b, D[j], E[j], c[j])[key]
        assert ref["term_margin"] > 1.0 and ref["rho_margin"] >= 1e-3, (label, b, ref["term_margin"], ref["rho_margin"])
        assert (info[j].status_val, info[j].iter, info[j].rho_updates) == (-2, key[1], ref["rho_updates"]), \
            (label, b, info[j].status_val, info[j].iter, info[j].rho_updates, ref["rho_updates"])
        r, k = AF.judge(got[j], ref, case.scenario)
        if r >= worst:
            worst, where = r, (b, k)
        errs = AF.errors(got[j], ref, keys=("x", "y"))
        ex, ey = max(ex, errs["x"]), max(ey, errs["y"])
    print(f"admm {label} {key}: worst ratio {worst:.3f} at {where}; errors of x {ex:.2e}, y {ey:.2e}")
    assert worst <= 1.0, (label, key, worst, where)
    return worst


def run(case, form, monkeypatch, ks=None):
    """one fresh handle per checkpoint, taken through the case's calls; the info of every solve"""
    BT, env, B = form_env(monkeypatch, form)
    infos = []
    B = min(B, case.B)
    pr = AF.take(case.pr, B)
    for k in case.ks if ks is None else ks:
        s = make(pr, **dict(case.settings, max_iter=k))
        form_asserts(s, BT, env)
        tail = s.stats()["dense_tail_rows"]
        if "MI_OSQP_DENSE_TAIL" in env:
            assert tail == int(env["MI_OSQP_DENSE_TAIL"]), tail
        if case.rho_each is not None:
            s.update_rho_each(np.asarray(case.rho_each[:B], dtype=np.float64))
        if case.warm_x is not None:
            s.warm_start_x(case.warm_x[:B])
        if case.warm_y is not None:
            s.warm_start_y(case.warm_y[:B])
        label = f"{case.name} {form[0]} (dense tail {tail})"
        infos += s.solve()
        compare(s, infos[-B:], case, (0, k), label)
        if case.k2 is not None:
            if case.bounds is not None:
                s.update_bounds(case.bounds[0][:B], case.bounds[1][:B])
            infos += s.solve()
            compare(s, infos[-B:], case, (1, case.k2), label)
        s.close()
    return infos


# ------------------------------------------------------------------ a. checkpoints on every form
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_checkpoints_on_every_form(form, monkeypatch):
    """k = 26: at the defaults the second launch is a single iteration.  k = 125: every QP takes a new rho at iteration 100 and
    runs 25 iterations on the device's new factor."""
    run(AF.cases()["box"], form, monkeypatch, ks=(26, 125))


@pytest.mark.parametrize("name", FEW)
def test_early_checkpoints(name, monkeypatch):
    run(AF.cases()["box"], FORM[name], monkeypatch, ks=(1, 2, 25, 30))


# ------------------------------------------------------------------ b. an early, uneven rho update
@pytest.mark.parametrize("name", ["tile1", "tile2", "tile4", "tail64"])
def test_early_uneven_rho_update(name, monkeypatch):
    """checks every 5, estimates every 10, 35 iterations: QPs 1-5 refactor once (at 20 or 30), QP 0 never does - in a tile of 2 or
    4 one QP takes a new factor while its partner keeps its own"""
    run(AF.cases()["early_rho"], FORM[name], monkeypatch)


# ------------------------------------------------------------------ c. continuation
@pytest.mark.parametrize("case", ["cont", "cont_bounds"])
@pytest.mark.parametrize("name", ["tile1", "tile2"])
def test_second_solve_continues_from_the_stored_state(name, case, monkeypatch):
    """30 iterations, then 30 more on the same handle: the only view of the stored z and of the resident state's write-back.
    cont_bounds: update_bounds in between turns one inequality row into l = u - its rho_vec entry and the factor change."""
    run(AF.cases()[case], FORM[name], monkeypatch)


# ------------------------------------------------------------------ d. warm starts
@pytest.mark.parametrize("case", ["warm_s10", "warm_s0"])
def test_warm_starts(case, monkeypatch):
    run(AF.cases()[case], FORM["tile2"], monkeypatch)


# ------------------------------------------------------------------ e. settings
SETTINGS = ["set_scaling0", "set_scaled_termination", "set_alpha1", "set_alpha1.8", "set_sigma1e-3", "set_rho_each"]


@pytest.mark.parametrize("case", SETTINGS)
@pytest.mark.parametrize("name", ["tile2", "tail64"])
def test_settings(name, case, monkeypatch):
    run(AF.cases()[case], FORM[name], monkeypatch)


def test_settings_on_the_grouped_global_form(monkeypatch):
    run(AF.cases()["set_scaled_termination"], FORM["gx_groups16"], monkeypatch)


# ------------------------------------------------------------------ f. the GOMP pattern
GOMP_FORMS = [("default", 0, {}, 4), ("tail64", 0, {"MI_OSQP_DENSE_TAIL": "64"}, 4), ("tail0", 0, {"MI_OSQP_DENSE_TAIL": "0"}, 4)]


@pytest.mark.parametrize("form", GOMP_FORMS, ids=lambda f: f[0])
def test_gomp_pattern(form, monkeypatch):
    """equality rows at 1e3 rho, free rows at RHO_MIN, infinite bounds and all-zero rows, from the pattern's own warm start"""
    run(AF.cases()["gomp"], form, monkeypatch)


# ------------------------------------------------------------------ g. edge shapes
@pytest.mark.parametrize("scaling", [0, 10])
@pytest.mark.parametrize("shape", ["n1_m2", "n4_m0", "empty"])
def test_edge_shapes(shape, scaling, monkeypatch):
    case = AF.cases()[f"edge_{shape}_s{scaling}"]
    form = ("default", 0, {}, case.B)
    infos = run(case, form, monkeypatch)
    if shape == "n4_m0":
        assert len(infos) == 2 * case.B and all(i.pri_res == 0.0 for i in infos)


@pytest.mark.parametrize("scaling", [0, 10])
@pytest.mark.parametrize("name,case", [("tile2_B3", "box_B3"), ("tile4_B5", "box_B5")])
def test_padding_class_of_a_ragged_tile(name, case, scaling, monkeypatch):
    run(AF.cases()[case + ("_s0" if scaling == 0 else "")], FORM[name], monkeypatch)


# ------------------------------------------------------------------ h. the continuous mode
def test_continuous_mode_one_segment_apart(monkeypatch):
    """a tile of 2: QP 1 begins one segment after QP 0, so check_body inlined into advance_kernel sees the two at different
    iteration counts; each runs its 30 iterations and is compared on its own"""
    case = AF.cases()["box"]
    BT, env, _ = form_env(monkeypatch, FORM["tile2"])
    s = make(AF.take(case.pr, 2), **dict(case.settings, max_iter=30))
    form_asserts(s, BT, env)
    s.solve_begin_some([0])
    s.advance(1)
    order = [list(s.poll(True))]                                # a segment is gcd(25, 100, max_iter = 30) = 5 iterations: QP 0 runs 1 .. 5
    s.solve_begin_some([1])
    for _ in range(6):                                          # QP 1 stays 5 iterations behind QP 0
        s.advance(1)
        order.append(list(s.poll(True)))
    assert order == [[], [], [], [], [], [0], [1]] and not s.running(), order       # (each ends in its own sixth segment)
    compare(s, s.info_some([0, 1]), case, (0, 30), "box continuous tile2")
    s.close()
