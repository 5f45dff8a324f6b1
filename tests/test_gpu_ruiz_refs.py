"""GPU (-m gpu): the equilibration of the device (kernels.hip ruiz_kernel, ruiz_reg_kernel<4|8|16|32>) and of the host
(host_core.cpp scale_qp / unscale_qp) against the long-double reference of tests/ruiz_refs.py: scaling() of every QP of every
handle within RUIZ_BOUND - 32 x the error of the fp64 twins, per case and per quantity (D, E, c), pinned by
tests/test_ruiz_refs.py - on every dispatch class of launch_ruiz, at the limits of ruiz_limit, at other iteration counts and
after every kind of update.  Each handle is built twice, with MI_OSQP_DEVICE_RUIZ=1 and with MI_OSQP_HOST_RUIZ=1; the two must
agree bit for bit (the per-QP calls equilibrate on the device either way).  The stored scaled P and A are checked through the
SpMV op against the REFERENCE's scaling rounded to fp64, the scaled q, l, u through one ADMM checkpoint under that scaling.  No
QP and no entry is skipped.  The measured ratios are in DESIGN.md section 6."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import admm_refs as AF                                                          # noqa: E402
import osqp_solver_amd as M                                                     # noqa: E402
import ruiz_refs as RR                                                          # noqa: E402
from test_gpu_admm_refs import published                                        # noqa: E402
from test_gpu_ops import _env, check_spmv, vectors                              # noqa: E402

pytestmark = pytest.mark.gpu
TILES = ((1, 2), (2, 3), (4, 5))                            # (QPs per tile, B): a padding slot at 2 and at 4
PATH_TILE = 2                                               # the paths: B = 5 in tiles of 2


def make(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def handle(monkeypatch, case, ruiz, BT, B, **kw):
    _env(monkeypatch, BT, {"MI_OSQP_HOST_RUIZ" if ruiz == "host" else "MI_OSQP_DEVICE_RUIZ": "1"})
    s = make(AF.take(case.pr, B), scaling=case.iters, **kw)
    st = s.stats()
    assert st["tile"] == BT or (st["n"] + st["m"] > 4096 and st["tile"] < BT), st["tile"]
    # the class of launch_ruiz this pattern selects (on the host path the same counts, for the per-QP calls)
    assert RR.ruiz_form(st["n"], st["m"], st["nnz_P_triu"], st["nnz_A"]) == case.form
    return s


def take_steps(s, case):
    """the calls of the case's path on the handle; after each per-QP call the unlisted QPs' scaling is bitwise unchanged"""
    import torch
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")
    ids = case.ids
    for call, k in case.steps:
        v = case.sets[k]
        before = s.scaling()
        if call == "update_A":
            s.update_A(v["Ax"])
        elif call == "update_A_bounds":
            s.update_A_bounds(v["Ax"], v["l"], v["u"])
        elif call == "update_P":
            s.update_P(v["Px"])
        elif call == "update_P_A":
            s.update_P_A(v["Px"], v["Ax"])
        elif call == "update_q":
            s.update_q(v["q"])
        elif call == "update_A_bounds_device":
            s.update_A_bounds_device(dev(v["Ax"]), dev(v["l"]), dev(v["u"]))
        elif call == "update_P_device":
            s.update_P_device(dev(v["Px"]))
        elif call == "update_P_A_bounds_device":
            s.update_P_A_bounds_device(dev(v["Px"]), dev(v["Ax"]), dev(v["l"]), dev(v["u"]))
        elif call == "update_A_bounds_some":
            s.update_A_bounds_some(ids, v["Ax"][ids], v["l"][ids], v["u"][ids])
        elif call == "update_P_some":
            s.update_P_some(ids, v["Px"][ids])
        elif call == "update_P_A_bounds_some":
            s.update_P_A_bounds_some(ids, v["Px"][ids], v["Ax"][ids], v["l"][ids], v["u"][ids])
        elif call == "reinit_some":
            s.reinit_some(ids, v["Ax"][ids], v["l"][ids], v["u"][ids])
        else:
            raise KeyError(call)
        after = s.scaling()
        rest = [b for b in range(s.B) if b not in ids] if call in RR.PER_QP else (range(s.B) if call == "update_q" else [])
        for b in rest:
            for x, y in zip(before, after):
                assert x[b].tobytes() == y[b].tobytes(), (case.name, call, b)


def compare(s, case, label):
    """scaling() of every QP of the handle against the reference; the worst ratio and the worst errors"""
    D, E, c = s.scaling()
    worst, where, errs = 0.0, None, {k: 0.0 for k in RR.QUANTITIES}
    for b in range(s.B):
        e = RR.errors((D[b], E[b], c[b]), case.model(b))
        r, k = RR.ratio(e, case.name)
        if r >= worst:
            worst, where = r, (b, k)
        errs = {k: max(errs[k], e[k]) for k in errs}
    print(f"ruiz {label}: worst ratio {worst:.3f} at {where}; errors of D {errs['D']:.2e}, E {errs['E']:.2e}, c {errs['c']:.2e}")
    assert worst <= 1.0, (label, worst, where)
    return worst


def spmv_under_the_reference_scaling(s, case):
    """the scaled P and A the handle stores, against the raw data in force scaled by the reference's D, E, c"""
    pr = AF.take(case.data_after(), s.B)
    ref = [RR.rounded(case.model(b)) for b in range(s.B)]
    scaled = (np.array([r[0] for r in ref]), np.array([r[1] for r in ref]).reshape(s.B, s.m), np.array([r[2] for r in ref]))
    x, y = vectors(s.B, s.n, s.m, seed=6)
    check_spmv(s, pr, x, y, scaled=scaled)


def both(monkeypatch, case, BT, B, label):
    """the case on a handle that equilibrates on the device and on one that does so on the host: bitwise equal, both
    within the bound"""
    got = {}
    for ruiz in ("device", "host"):
        s = handle(monkeypatch, case, ruiz, BT, B)
        take_steps(s, case)
        got[ruiz] = s.scaling()
        compare(s, case, f"{label} {ruiz}")
        spmv_under_the_reference_scaling(s, case)
        s.close()
    for x, y in zip(got["device"], got["host"]):
        assert x.tobytes() == y.tobytes(), label
    return got["device"]


# ------------------------------------------------------------------ a. every dispatch class of launch_ruiz, every tile shape
@pytest.mark.parametrize("BT,B", TILES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", [n for n in RR.cases() if n.startswith("form_")])
def test_every_dispatch_class(name, BT, B, monkeypatch):
    both(monkeypatch, RR.cases()[name], BT, B, f"{name} tile {BT} B {B}")


# ------------------------------------------------------------------ b. the limits of ruiz_limit
@pytest.mark.parametrize("name,BT", [("iters10_limits", 1), ("iters10_limits", 2), ("iters10_limits", 4), ("limits_global", 2),
                                     ("tiny_n1_m2", 2), ("tiny_n4_m0", 4)])
def test_limits_and_edge_shapes(name, BT, monkeypatch):
    case = RR.cases()[name]
    D, E, c = both(monkeypatch, case, BT, case.B, f"{name} tile {BT}")
    if "limits" in name:
        assert D[0, 2] == 1.0 and E[0, 2] == 1.0 and c[2] == 1.0 and c[3] == 1.0       # empty column, empty row, cost factor 1


# ------------------------------------------------------------------ c. iteration counts
@pytest.mark.parametrize("kind", ["benign", "limits"])
@pytest.mark.parametrize("iters", RR.ITERS)
def test_iteration_counts(iters, kind, monkeypatch):
    case = RR.cases()[f"iters{iters}_{kind}"]
    both(monkeypatch, case, PATH_TILE, case.B, f"{case.name}")


# ------------------------------------------------------------------ d. every path that equilibrates again
@pytest.mark.parametrize("kind", ["benign", "limits"])
@pytest.mark.parametrize("path", list(RR.PATHS))
def test_paths(path, kind, monkeypatch):
    case = RR.cases()[f"{path}_{kind}"]
    assert case.ids == list(RR.SOME) and sorted(case.ids) != case.ids and len(case.ids) < case.B
    both(monkeypatch, case, PATH_TILE, case.B, case.name)


# ------------------------------------------------------------------ e. the scaled q, l, u: one ADMM checkpoint under the reference's scaling
@pytest.mark.parametrize("ruiz", ["device", "host"])
@pytest.mark.parametrize("path", RR.ADMM_SCENARIOS)
def test_admm_checkpoint_under_the_reference_scaling(path, ruiz, monkeypatch):
    case, ac = RR.cases()[path + "_benign"], RR.admm_case(path)
    s = handle(monkeypatch, case, ruiz, PATH_TILE, case.B, **dict(ac.settings, max_iter=RR.ADMM_K))
    take_steps(s, case)
    info = s.solve()
    got = published(s, info)
    bound = RR.admm_bound(path)
    worst, where = 0.0, None
    for b in range(s.B):
        ref = AF.reference(ac, b, *RR.rounded(case.model(b)))[(0, RR.ADMM_K)]
        assert ref["term_margin"] > 1.0 and ref["rho_margin"] >= 1e-3
        assert (info[b].status_val, info[b].iter, info[b].rho_updates) == (-2, RR.ADMM_K, ref["rho_updates"]), (path, b)
        for k, e in AF.errors(got[b], ref, x_bound=bound["x"]).items():
            r = (0.0 if e == 0.0 else float("inf")) if bound[k] == 0.0 else e / bound[k]
            if r >= worst:
                worst, where = r, (b, k)
    print(f"ruiz admm after {path} {ruiz}: worst ratio {worst:.3f} at {where}")
    assert worst <= 1.0, (path, worst, where)
    s.close()
