"""GPU (-m gpu): the termination decision of the device (kernels.hip check_body, blocks E12 and E14 - also where it is inlined
into advance_kernel) against the long-double reference of tests/term_refs.py, on every launch form.

Every case of term_refs.cases() is solved to its exit; the reference is built from the handle's own scaling() (once per case, QP
and scaling; shared by the forms).  Per QP: status, iter and rho_updates equal the reference's; pri_res and dua_res within
RES_BOUND of the case (32 x the error of the fp64 twins, tests/test_term_refs.py pins it, in admm_refs' term scales); obj_val
bitwise +-1e30 after an infeasible exit and within the bound otherwise; x and y all NaN exactly where the status carries no
solution and within the bound otherwise; the certificate within CERT_BOUND of the reference's, its unit entry exactly +-1 at
the reference's index with the reference's sign, the other certificate all NaN.  No QP is skipped.  The batch is rotated from
form to form, so that every QP sits at every class position of a tile of 4; B = 11 leaves the last tile ragged.  What the cases
presuppose (no clause ratio and no rho decision near its threshold, the unit entry decided) is asserted of every reference used.
The measured ratios are in DESIGN.md section 6."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exit_cases as EC                                                         # noqa: E402
import term_refs as T                                                           # noqa: E402
from test_gpu_continuous import _drain                                          # noqa: E402
from test_gpu_polish_refs import FORM, FORMS, form_asserts, form_env, make      # noqa: E402

pytestmark = pytest.mark.gpu
GROUPS = list(T.GROUPS)
SMALL = ("n1m2_s10", "n1m2_s0", "m0_s10", "m0_s0")
WORST = {}


def check(case, label, D, E, c, qps, info, x, y, pv, dv, k=0):
    """QP qps[j] of the case in slot j, against the k-th solve of its reference; the worst error / bound"""
    worst, where = 0.0, None
    for j, b in enumerate(qps):
        ref = T.reference(case, b, D[j], E[j], c[j])[k]
        near, at = T.nearest(ref)
        assert near > T.CLAUSE_NEAR[case.name] and ref["rho_margin"] >= 1e-3, (label, b, near, at)
        i = info[j]
        assert (i.status_val, i.iter, i.rho_updates) == (ref["status"], ref["iter"], ref["rho_updates"]), \
            (label, b, k, i.status_val, i.iter, i.rho_updates, ref["status"], ref["iter"], ref["rho_updates"])
        got = dict(pri_res=i.pri_res, dua_res=i.dua_res, obj_val=i.obj_val, x=x[j], y=y[j])
        if ref["cert"] is None:
            assert np.all(np.isnan(pv[j])) and np.all(np.isnan(dv[j])), (label, b)
            assert np.all(np.isfinite(x[j])) and np.all(np.isfinite(y[j])), (label, b)
        else:
            primal = ref["status"] in (-3, 3)
            v, other = (pv[j], dv[j]) if primal else (dv[j], pv[j])
            assert np.all(np.isnan(other)) and np.all(np.isnan(x[j])) and np.all(np.isnan(y[j])), (label, b)
            assert i.obj_val == (1e30 if primal else -1e30), (label, b, i.obj_val)
            rv = np.asarray(ref["cert"], np.float64)
            assert T.cert_gap(rv) > T.CERT_BOUND[case.name]
            at = int(np.argmax(np.abs(rv)))
            assert float(np.max(np.abs(v))) == 1.0 and v[at] == rv[at] and abs(rv[at]) == 1.0, (label, b, at, v[at])
            got["cert"] = v
        r, key = T.judge(case, got, ref)
        if r >= worst:
            worst, where = r, (b, key)
    print(f"term {label} solve {k}: worst ratio {worst:.3f} at {where}")
    assert worst <= 1.0, (label, k, worst, where)
    WORST[label.split()[1]] = max(WORST.get(label.split()[1], 0.0), worst)
    return worst


def blocking(case, form, monkeypatch, qps, extra_env=None):
    BT, env, _ = form_env(monkeypatch, form)
    for key, val in (extra_env or {}).items():
        monkeypatch.setenv(key, val)
    s = make(EC.take(case.pr, qps), **case.settings)
    form_asserts(s, BT, env)
    if extra_env:
        assert s.stats()["resident_state"] == 0
    D, E, c = s.scaling()
    label, k = f"{case.name} {form[0]}{'_streamed' if extra_env else ''}", 0
    for call in case.solves:
        if call == "solve":
            info = s.solve()
            check(case, label, D, E, c, qps, info, s.primal(), s.dual(), s.prim_inf_cert(), s.dual_inf_cert(), k)
            k += 1
        else:
            s.update_bounds(call[1][qps], call[2][qps])
    s.close()


def rotation(case, shift):
    return [(j + shift) % case.B for j in range(case.B)]


# ------------------------------------------------------------------ a. every group on every form
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_every_group_on_every_form(form, monkeypatch):
    shift = [f[0] for f in FORMS].index(form[0]) % 4
    if form[3] == 1:                                         # one QP shared by the grid
        for g in GROUPS:
            for b in range(T.cases()[g].B):
                blocking(T.cases()[g], form, monkeypatch, [b])
    else:
        for g in GROUPS:
            blocking(T.cases()[g], form, monkeypatch, rotation(T.cases()[g], shift))
    print(f"worst ratio on {form[0]}: {WORST.get(form[0], 0.0):.3f}")


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_class_position_of_a_tile_of_four(shift, monkeypatch):
    for g in ("s10_a", "close_on"):
        blocking(T.cases()[g], FORM["tile4"], monkeypatch, rotation(T.cases()[g], shift))


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("tile", ["tile1", "tile4_B5"])
def test_small_shapes(tile, name, monkeypatch):
    case = T.cases()[name]
    blocking(case, FORM[tile], monkeypatch, list(range(case.B)))


# ------------------------------------------------------------------ b. the streamed state
@pytest.mark.parametrize("tile", ["tile1", "tile4"])
def test_streamed_state(tile, monkeypatch):
    for g in GROUPS:
        blocking(T.cases()[g], FORM[tile], monkeypatch, rotation(T.cases()[g], 1), extra_env={"MI_OSQP_STREAM_STATE": "1"})


# ------------------------------------------------------------------ c. the continuous mode
@pytest.mark.parametrize("tile", ["tile1", "tile2", "tile4"])
def test_continuous_mode_with_staggered_begins(tile, monkeypatch):
    """check_body inlined into advance_kernel: half of the QPs begin one segment after the others, every QP is read with the
    *_some getters; the group that solves again does so here too"""
    form = FORM[tile]
    for g in GROUPS:
        case = T.cases()[g]
        qps = rotation(case, 2)
        BT, env, _ = form_env(monkeypatch, form)
        s = make(EC.take(case.pr, qps), **case.settings)
        form_asserts(s, BT, env)
        D, E, c = s.scaling()
        ids = list(range(case.B))
        s.solve_begin_some(ids[0::2])
        s.advance(1)
        done = list(s.poll(True))
        s.solve_begin_some(ids[1::2])
        done += _drain(s)
        assert sorted(done) == ids
        check(case, f"{g} {tile}_continuous", D, E, c, qps, s.info_some(ids), s.primal_some(ids), s.dual_some(ids),
              s.prim_inf_cert_some(ids), s.dual_inf_cert_some(ids))
        if len(case.solves) > 1:
            # the second solve, data unchanged, begun the other way round.  (The solve after update_bounds stays with the blocking
            # forms: the continuous mode has no bounds-only update, and update_A_bounds_some equilibrates again - the reference
            # is built on the scaling of setup.)
            assert case.solves[1] == "solve"
            s.solve_begin_some(ids[1::2])
            s.advance(1)
            done = list(s.poll(True))
            s.solve_begin_some(ids[0::2])
            done += _drain(s)
            assert sorted(done) == ids
            check(case, f"{g} {tile}_continuous", D, E, c, qps, s.info_some(ids), s.primal_some(ids), s.dual_some(ids),
                  s.prim_inf_cert_some(ids), s.dual_inf_cert_some(ids), 1)
        s.close()
