"""GPU (-m gpu): the adjoint derivative (mi_osqp.h "adjoint derivative") on every launch form against
the float64 reference of tests/adjoint_refs.py, whose own error tests/test_adjoint_refs.py pins at 1e-12 of the same scale.

The error of a gradient is max |device - reference| divided by the scale of its terms: |r|_inf for dq, dl, du and
|r|_inf max(|x|_inf, |y|_inf) for dP, dA.  The bound is 1e-9 (adjoint_refs.GPU_BOUND): three refinement rounds at
delta = 1e-6 with |K^-1| <= 20 leave nothing above rounding, rounding is cond(K) 2^-53 N ~ 1e-12, and the remaining 1e3 covers
the conditioning of the equilibrated matrix and the 1e-12 .. 1e-10 by which the polished solution differs from the exact one.
Measured on an MI355X: at most 5.1e-15 on every form (the table of DESIGN.md section 8, "Adjoint derivative")."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_refs as AR                                                       # noqa: E402
import exit_cases as EC                                                         # noqa: E402
import osqp_solver_amd as M                                                     # noqa: E402
from osqp_solver_amd import problems as PR                                      # noqa: E402
from test_gpu_ops import _env, with_full_P                                      # noqa: E402

pytestmark = pytest.mark.gpu
SETTINGS = dict(polish=1, eps_abs=1e-7, eps_rel=1e-7)
KEYS = ("dq", "dP", "dA", "dl", "du")


@pytest.fixture(scope="module")
def refs():
    """the problems, their fixtures (asserted), the gradient seeds and the reference gradients: computed once, never changed"""
    pr = AR.gpu_problem()
    fxs = [AR.fixture(pr, b, key="gpu") for b in range(AR.GPU_B)]
    for fx in fxs:
        AR.assert_preconditions(fx)
    gx, gy = AR.gradient_seeds(AR.GPU_B, pr["n"], pr["m"])
    ref = [AR.adjoint_ref(fx["P"], fx["A"], fx["act"], fx["x"], fx["y"], gx[b], gy[b]) for b, fx in enumerate(fxs)]
    for a in (gx, gy):
        a.setflags(write=False)
    return dict(pr=pr, fx=fxs, gx=gx, gy=gy, ref=ref)


def make(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **{**SETTINGS, **kw})


def solve_checked(s, fxs):
    """the preconditions of every comparison: kOptimal, polished, and the reference's active set"""
    info = s.solve()
    assert [i.status_val for i in info] == [1] * s.B, [i.status_val for i in info]
    assert [i.status_polish for i in info] == [1] * s.B, [i.status_polish for i in info]
    act = s.polish_active()
    for b in range(s.B):
        np.testing.assert_array_equal(act[b], fxs[b]["act"], err_msg=f"QP {b}")
    return info


def within_bound(out, refs, qps, label):
    worst, where = 0.0, None
    for b in qps:
        fx = refs["fx"][b]
        e, k = AR.worst_ratio({k: out[k][b] for k in KEYS}, refs["ref"][b], fx["x"], fx["y"])
        if e >= worst:
            worst, where = e, (b, k)
    print(f"adjoint {label}: worst ratio {worst:.3e} at {where}")
    assert worst <= AR.GPU_BOUND, (label, worst, where)
    return worst


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ 1. closed forms through the C-ABI
def _single(p, q, l, u):
    return _single_qp(1, 1, [0, 1], [0], [p], [q], [0, 1], [0], [1.0], [l], [u])


def _single_qp(n, m, Pp, Pi, Pv, q, Ap, Ai, Av, l, u):
    L = M.lib()
    h = C.c_void_p()
    i64 = lambda v: (C.c_int64 * max(len(v), 1))(*v)
    f64 = lambda v: (C.c_double * max(len(v), 1))(*v)
    s = M.default_settings(**SETTINGS)
    rc = L.mi_osqp_setup(C.byref(h), n, m, i64(Pp), i64(Pi), f64(Pv), f64(q), i64(Ap), i64(Ai), f64(Av), f64(l), f64(u), C.byref(s))
    assert rc == 0, rc
    info = M.Info()
    assert L.mi_osqp_solve(h, C.byref(info)) == 0 and info.status_val == 1
    return L, h


def _adjoint_qp(L, h, g, sizes):
    """mi_osqp_adjoint with dy = NULL; sizes: entries of every output"""
    out = {k: (C.c_double * max(sizes[k], 1))(*([np.nan] * max(sizes[k], 1))) for k in KEYS}
    st = (C.c_int32 * 1)(7)
    rc = L.mi_osqp_adjoint(h, (C.c_double * len(g))(*g), None, out["dq"], out["dP"], out["dA"], out["dl"], out["du"], st)
    assert rc == 0 and st[0] == 1, (rc, st[0])
    return {k: np.array(out[k][:sizes[k]]) for k in KEYS}


def _single_adjoint(L, h, g, gy=None):
    out = {k: (C.c_double * 1)(np.nan) for k in KEYS}
    st = (C.c_int32 * 1)(7)
    rc = L.mi_osqp_adjoint(h, (C.c_double * 1)(g), None if gy is None else (C.c_double * 1)(gy), out["dq"], out["dP"], out["dA"], out["dl"],
                           out["du"], st)
    assert rc == 0 and st[0] == 1, (rc, st[0])
    return {k: v[0] for k, v in out.items()}


def test_closed_forms_through_the_c_abi():
    p, g = 2.0, 1.25
    # inactive: x = -q/p, dq = -g/p, dP = g q/p^2, dl = du = 0 (scale of the terms: |r| = g/p, |x| = q/p)
    q = 0.6
    L, h = _single(p, q, -1.0, 1.0)
    o = _single_adjoint(L, h, g, gy=3.0)
    L.mi_osqp_free(h)
    r = g / p
    assert abs(o["dq"] + g / p) <= AR.GPU_BOUND * r and abs(o["dP"] - g * q / p ** 2) <= AR.GPU_BOUND * r * q / p
    assert o["dl"] == 0.0 and o["du"] == 0.0 and abs(o["dA"]) <= AR.GPU_BOUND * r * q / p
    # active at u = 1 (-q/p = 1.5): dx/du = 1, dq = 0, y = -(p u + q) = 1, dA = -g u   (|r| = g, max(|x|, |y|) = 1)
    q = -3.0
    L, h = _single(p, q, -1.0, 1.0)
    y = (C.c_double * 1)()
    assert L.mi_osqp_get_dual(h, y) == 0 and abs(y[0] - 1.0) <= 1e-9
    o = _single_adjoint(L, h, g)
    L.mi_osqp_free(h)
    assert abs(o["du"] - g) <= AR.GPU_BOUND * g and abs(o["dq"]) <= AR.GPU_BOUND * g and o["dl"] == 0.0
    assert abs(o["dA"] + g) <= AR.GPU_BOUND * g and abs(o["dP"]) <= AR.GPU_BOUND * g


def test_closed_forms_no_constraints_and_equality_row_through_the_c_abi():
    # m = 0, P = [[2, .5], [.5, 1]] (upper triangle stored): x = -P^-1 q, r = P^-1 g, dq = -r,
    # dP = [-r0 x0, -(r0 x1 + r1 x0), -r1 x1]
    Pd = np.array([[2.0, 0.5], [0.5, 1.0]])
    q, g = np.array([1.0, -2.0]), np.array([0.3, 0.7])
    L, h = _single_qp(2, 0, [0, 1, 3], [0, 0, 1], [2.0, 0.5, 1.0], q, [0, 0, 0], [], [], [], [])
    o = _adjoint_qp(L, h, g, dict(dq=2, dP=3, dA=0, dl=0, du=0))
    L.mi_osqp_free(h)
    det = Pd[0, 0] * Pd[1, 1] - Pd[0, 1] ** 2
    inv = np.array([[Pd[1, 1], -Pd[0, 1]], [-Pd[0, 1], Pd[0, 0]]]) / det
    x, r = -inv @ q, inv @ g
    rn, xn = np.max(np.abs(r)), np.max(np.abs(x))
    assert np.max(np.abs(o["dq"] + r)) <= AR.GPU_BOUND * rn
    want = np.array([-r[0] * x[0], -(r[0] * x[1] + r[1] * x[0]), -r[1] * x[1]])
    assert np.max(np.abs(o["dP"] - want)) <= AR.GPU_BOUND * rn * xn
    # a row with l = u = 1/4 (p = 2, q = 0.6): x = 1/4, y = -(p/4 + q) = -1.1 < 0, so the rule marks the lower side:
    # dl = g, du = 0, dq = 0, dP = 0, dA = -g x   (|r| = g, max(|x|, |y|) = 1.1)
    g1 = 1.5
    L, h = _single(2.0, 0.6, 0.25, 0.25)
    o = _adjoint_qp(L, h, [g1], dict(dq=1, dP=1, dA=1, dl=1, du=1))
    L.mi_osqp_free(h)
    assert abs(o["dl"][0] - g1) <= AR.GPU_BOUND * g1 and o["du"][0] == 0.0 and abs(o["dq"][0]) <= AR.GPU_BOUND * g1
    assert abs(o["dA"][0] + g1 * 0.25) <= AR.GPU_BOUND * g1 * 1.1 and abs(o["dP"][0]) <= AR.GPU_BOUND * g1 * 1.1


# ------------------------------------------------------------------ 2. every launch form
FORMS = [("tile1", 1, {}, 6), ("tile2", 2, {}, 6), ("tile4", 4, {}, 6), ("tile2_B3", 2, {}, 3),
         ("tail64", 0, {"MI_OSQP_DENSE_TAIL": "64"}, 6), ("tail0", 0, {"MI_OSQP_DENSE_TAIL": "0"}, 6),
         ("gx_tile2", 2, {"MI_OSQP_GLOBAL_XS": "1"}, 5), ("gx_tile4", 4, {"MI_OSQP_GLOBAL_XS": "1"}, 6),
         ("gx_groups0", 0, {"MI_OSQP_GLOBAL_XS": "1", "MI_OSQP_GROUPS": "0"}, 1),
         ("gx_groups16", 0, {"MI_OSQP_GLOBAL_XS": "1", "MI_OSQP_GROUPS": "16"}, 1)]


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_every_launch_form_against_the_reference(form, refs, monkeypatch):
    name, BT, env, B = form
    _env(monkeypatch, BT, env)
    s = make(EC.take(refs["pr"], np.arange(B)))
    if BT:
        assert s.stats()["tile"] == BT
    solve_checked(s, refs["fx"])
    out = s.adjoint(refs["gx"][:B], refs["gy"][:B])
    assert out["status"].tolist() == [1] * B
    within_bound(out, refs, range(B), name)
    again = s.adjoint(refs["gx"][:B], refs["gy"][:B])
    for k in KEYS:
        assert same_bits(out[k], again[k]), k                   # deterministic
    s.close()


# ------------------------------------------------------------------ 3. scaling
@pytest.mark.parametrize("kw", [dict(scaling=0), dict(), dict(scaled_termination=1)], ids=["scaling0", "default", "scaled_termination"])
def test_scaling_off_on_and_scaled_termination(kw, refs, monkeypatch):
    _env(monkeypatch, 0, {})
    B = 5
    s = make(EC.take(refs["pr"], np.arange(B)), **kw)
    solve_checked(s, refs["fx"])
    out = s.adjoint(refs["gx"][:B], refs["gy"][:B])
    assert out["status"].tolist() == [1] * B
    within_bound(out, refs, range(B), "+".join(f"{k}={v}" for k, v in kw.items()) or "default")
    s.close()


# ------------------------------------------------------------------ 4. P with both triangles
def test_full_P_gives_the_same_dP_in_the_upper_layout(refs, monkeypatch):
    _env(monkeypatch, 0, {})
    B = 3
    pr = EC.take(refs["pr"], np.arange(B))
    full = with_full_P(pr)
    assert full["P"].nnz == 2 * pr["P"].nnz - pr["n"]
    outs = []
    for p in (pr, full):
        s = make(p)
        solve_checked(s, refs["fx"])
        outs.append(s.adjoint(refs["gx"][:B], refs["gy"][:B]))
        s.close()
    assert outs[1]["dP"].shape == (B, pr["P"].nnz)
    within_bound(outs[1], refs, range(B), "full P")
    for k in KEYS:
        assert same_bits(outs[0][k], outs[1][k]), k             # (setup extracts the upper triangle: the same handle data)


# ------------------------------------------------------------------ 5. + 6. a mixed batch; the call moves nothing else
def _mixed(refs):
    pr = EC.take(refs["pr"], np.arange(4))
    EC.assert_identity_block(pr)
    EC.make_pinf(pr, 1)
    return pr


def test_mixed_batch_status_and_nan_rows(refs, monkeypatch):
    _env(monkeypatch, 2, {})
    s = make(_mixed(refs))
    info = s.solve()
    assert [i.status_val for i in info] in ([1, -3, 1, 1], [1, 3, 1, 1]) and [i.status_polish for i in info] == [1, 0, 1, 1]
    act = s.polish_active()
    for b in (0, 2, 3):
        np.testing.assert_array_equal(act[b], refs["fx"][b]["act"])
    out = s.adjoint(refs["gx"][:4], refs["gy"][:4])
    assert out["status"].tolist() == [1, 0, 1, 1]
    for k in KEYS:
        assert np.all(np.isnan(out[k][1])), k
    within_bound(out, refs, (0, 2, 3), "mixed batch")
    s.close()


def _state(s):
    return dict(x=s.primal(), y=s.dual(), info=b"".join(bytes(i) for i in s.info()), pc=s.prim_inf_cert(), dc=s.dual_inf_cert(),
                sc=np.concatenate([a.ravel() for a in s.scaling()]))


def test_the_call_changes_nothing_else(refs, monkeypatch):
    _env(monkeypatch, 2, {})
    pr = _mixed(refs)
    s, twin = make(pr), make(pr)
    s.solve(); twin.solve()
    before = _state(s)
    assert np.isfinite(before["pc"][1]).all()                    # a real certificate is among what must not move
    out = s.adjoint(refs["gx"][:4], refs["gy"][:4])
    assert out["status"].tolist() == [1, 0, 1, 1]
    after, other = _state(s), _state(twin)
    for k in before:
        if k == "info":
            assert before[k] == after[k] == other[k]
        else:
            assert same_bits(before[k], after[k]) and same_bits(before[k], other[k]), k
    # the next (warm-started) solve, after new data: the same iterations and bits as on the handle that never called it
    q2 = pr["q"] * 1.05 + 0.01
    for h in (s, twin):
        h.update_q(q2)
    ia, ib = s.solve(), twin.solve()
    assert [i.iter for i in ia] == [i.iter for i in ib] and [i.rho_updates for i in ia] == [i.rho_updates for i in ib]
    a, b = _state(s), _state(twin)
    for k in a:
        assert (a[k] == b[k]) if k == "info" else same_bits(a[k], b[k]), k
    s.close(); twin.close()


def test_before_any_solve_and_after_continuous_solves_only(refs, monkeypatch):
    """No solve finished: status 0, NaN.  A handle solved (and polished) through the continuous entry points only: the call
    leaves the mode and differentiates those solves."""
    from test_gpu_continuous import _drain
    _env(monkeypatch, 2, {})
    B = 3
    s = make(EC.take(refs["pr"], np.arange(B)), polish=0)
    out = s.adjoint(refs["gx"][:B], refs["gy"][:B])
    assert out["status"].tolist() == [0] * B and all(np.all(np.isnan(out[k])) for k in KEYS)
    s.solve_begin_some(np.arange(B))
    assert sorted(_drain(s)) == list(range(B))
    s.polish_some(np.arange(B))
    s.advance(1)
    assert sorted(s.poll(True)) == list(range(B))
    out = s.adjoint(refs["gx"][:B], refs["gy"][:B])
    info = s.info()
    assert [i.status_val for i in info] == [1] * B and [i.status_polish for i in info] == [1] * B
    np.testing.assert_array_equal(s.polish_active(), np.array([fx["act"] for fx in refs["fx"][:B]]))
    assert out["status"].tolist() == [1] * B
    within_bound(out, refs, range(B), "continuous solves only")
    s.close()


# ------------------------------------------------------------------ 7. null handling
def _device_call(s, gx, gy, want=KEYS, stream=None, sentinel=-7.25):
    """adjoint_device into buffers of B + 1 rows: the row behind the batch must keep its sentinel"""
    import torch
    st = s.stats()
    width = dict(dq=s.n, dP=st["nnz_P_triu"], dA=st["nnz_A"], dl=s.m, du=s.m)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        tx = torch.tensor(gx, device="cuda")
        ty = None if gy is None else torch.tensor(gy, device="cuda")
        bufs = {k: torch.full((s.B + 1, width[k]), sentinel, dtype=torch.float64, device="cuda") for k in want}
        status = torch.full((s.B + 1,), 7, dtype=torch.int32, device="cuda")
        s.adjoint_device(tx, ty, status=status, stream=None if stream is None else stream.cuda_stream, **bufs)
        torch.cuda.synchronize()
    for k in want:
        assert bool((bufs[k][s.B] == sentinel).all()), k          # nothing written past QP B - 1
    assert int(status[s.B]) == 7
    out = {k: bufs[k][:s.B].cpu().numpy() for k in want}
    out["status"] = status[:s.B].cpu().numpy()
    return out


def test_null_dy_is_zero_and_null_outputs_are_skipped(refs, monkeypatch):
    _env(monkeypatch, 2, {})
    B = 3
    s = make(EC.take(refs["pr"], np.arange(B)))
    solve_checked(s, refs["fx"])
    gx = refs["gx"][:B]
    a, z = s.adjoint(gx, None), s.adjoint(gx, np.zeros((B, s.m)))
    for k in KEYS:
        assert same_bits(a[k], z[k]), k
    assert not same_bits(a["dq"], s.adjoint(gx, refs["gy"][:B])["dq"])       # (dy is read when it is given)
    full = _device_call(s, gx, refs["gy"][:B])
    for skip in KEYS:
        part = _device_call(s, gx, refs["gy"][:B], want=tuple(k for k in KEYS if k != skip))
        for k in part:
            assert same_bits(part[k], full[k]), (skip, k)
    only_status = _device_call(s, gx, None, want=())
    assert only_status["status"].tolist() == [1] * B
    s.close()


# ------------------------------------------------------------------ 8. the device form on a stream; the layer
def test_device_form_on_a_stream_and_the_layer(refs, monkeypatch):
    import torch
    from osqp_solver_amd.qp_layer import qp_layer
    _env(monkeypatch, 2, {})
    B = 4
    pr = EC.take(refs["pr"], np.arange(B))
    s = make(pr)
    solve_checked(s, refs["fx"])
    host = s.adjoint(refs["gx"][:B], refs["gy"][:B])
    dev = _device_call(s, refs["gx"][:B], refs["gy"][:B], stream=torch.cuda.Stream())
    for k in KEYS + ("status",):
        assert same_bits(host[k], dev[k]), k
    t = lambda a, g: torch.tensor(a, device="cuda", requires_grad=g)
    q, Ax, l, u = t(pr["q"], True), t(pr["Ax"], False), t(pr["l"], True), t(pr["u"], False)
    x = qp_layer(s, q, Ax, l, u)
    assert same_bits(x.detach().cpu().numpy(), s.primal())
    w = torch.tensor(refs["gx"][:B], device="cuda")
    asked = []
    inner = s.adjoint_device
    monkeypatch.setattr(s, "adjoint_device", lambda *a, **kw: (asked.append(kw), inner(*a, **kw))[1])
    (x * w).sum().backward()
    monkeypatch.setattr(s, "adjoint_device", inner)
    assert len(asked) == 1 and asked[0]["dq"] is not None and asked[0]["dl"] is not None
    assert asked[0]["dA"] is None and asked[0]["du"] is None and "dP" not in asked[0]      # only what needs_input_grad asks for
    want = s.adjoint(refs["gx"][:B])                              # the same handle state the backward saw
    assert same_bits(q.grad.cpu().numpy(), want["dq"]) and same_bits(l.grad.cpu().numpy(), want["dl"])
    assert Ax.grad is None and u.grad is None
    ref0 = [AR.adjoint_ref(fx["P"], fx["A"], fx["act"], fx["x"], fx["y"], refs["gx"][b]) for b, fx in enumerate(refs["fx"][:B])]
    within_bound(want, dict(refs, ref=ref0), range(B), "layer (dy = 0)")
    x = qp_layer(s, q.detach(), Ax, l.detach(), u)                # nothing needs a gradient: no graph, no backward
    assert not x.requires_grad
    # a backward after another forward on the same solver would differentiate the wrong solve: refused
    q2 = q.detach().clone().requires_grad_(True)
    x1 = qp_layer(s, q2, Ax, l.detach(), u)
    qp_layer(s, q2, Ax, l.detach(), u)
    with pytest.raises(RuntimeError, match="another forward"):
        x1.sum().backward()
    s.close()


# ------------------------------------------------------------------ 9. edge shapes, n <= 6
def _edge(name, B=3):
    rng = np.random.default_rng(21)
    if name == "m0":
        n, m = 4, 0
        Pd = np.diag([1.5, 2.0, 1.0, 2.5]); Pd[0, 1] = 0.3; Pd[2, 3] = -0.2
        Ad = np.zeros((0, n)); l = u = np.zeros(0)
    elif name == "no_active_row":
        n, m = 5, 4
        Pd = np.diag(rng.uniform(1, 2, n)); Pd[1, 3] = 0.25
        Ad = rng.standard_normal((m, n)); l, u = -100.0 * np.ones(m), 100.0 * np.ones(m)
    elif name == "equality_row":
        n, m = 5, 4
        Pd = np.diag(rng.uniform(1, 2, n)); Pd[0, 4] = -0.2
        Ad = rng.standard_normal((m, n)); l, u = -100.0 * np.ones(m), 100.0 * np.ones(m)
        l[2] = u[2] = 0.75
    else:       # an empty P column, an empty A row and a shared column (the pattern of test_gpu_ops.edge_qp): variable 2 has no
        n, m = 6, 5      # entry in P and is held by its box row, which its linear cost keeps active
        Pd = np.diag(rng.uniform(1, 2, n)); Pd[0, 1] = 0.2; Pd[2, 2] = 0.0
        Ad = rng.standard_normal((m, n)); Ad[:, 2] = 0.0; Ad[1, :] = 0.0; Ad[3, :] = 0.0; Ad[3, 2] = 1.0
        l, u = -np.ones(m), np.ones(m)
    Pp = sp.csc_matrix(np.triu(Pd) != 0, dtype=float); Ap = sp.csc_matrix(Ad != 0, dtype=float)
    Pp.sort_indices(); Ap.sort_indices()
    Px = np.array([Pd.T[np.triu(Pd).T != 0] * (1 + 0.1 * b) for b in range(B)])
    Ax = np.array([Ad.T[Ad.T != 0] * (1 - 0.1 * b) for b in range(B)]).reshape(B, Ap.nnz)
    q = rng.standard_normal((B, n))
    if name == "empty_P_column":
        q[:, 2] = 1.0 + 0.5 * np.arange(B)
    return dict(n=n, m=m, P=Pp, A=Ap, Px=Px, Ax=Ax, q=q, l=np.tile(l, (B, 1)), u=np.tile(u, (B, 1)))


@pytest.mark.parametrize("scaling", [0, 10])
@pytest.mark.parametrize("name", ["m0", "no_active_row", "equality_row", "empty_P_column"])
def test_edge_shapes(name, scaling, monkeypatch):
    """The active set the device used is proved optimal here (primal feasible, multipliers of the right sign, both with a margin
    of 1e-3: the KKT conditions of a convex QP), then the gradients are compared under the bound."""
    _env(monkeypatch, 0, {})
    pr = _edge(name)
    B, n, m = pr["Px"].shape[0], pr["n"], pr["m"]
    s = make(pr, scaling=scaling)
    info = s.solve()
    assert [i.status_val for i in info] == [1] * B and [i.status_polish for i in info] == [1] * B
    acts = s.polish_active()
    gx, gy = AR.gradient_seeds(B, n, m, seed=3)
    out = s.adjoint(gx, gy)
    assert out["status"].tolist() == [1] * B
    worst = 0.0
    for b in range(B):
        P, A = PR.qp_matrices(pr, b)
        act, l, u = acts[b], pr["l"][b], pr["u"][b]
        x, y = AR.active_set_solution(P, pr["q"][b], A, l, u, act)
        z = A @ x
        eq = l == u
        assert np.all(z >= l - 1e-12) and np.all(z <= u + 1e-12)
        assert np.all(np.minimum(z - l, u - z)[act == 0] >= AR.MIN_GAP)
        assert np.all(y[(act < 0) & ~eq] <= -AR.MIN_GAP) and np.all(y[(act > 0) & ~eq] >= AR.MIN_GAP)
        if name == "no_active_row":
            assert not act.any()
        if name == "equality_row":
            assert act[2] != 0
        if name == "empty_P_column":
            assert act[3] == -1 and P[:, 2].nnz == 0
        K, _ = AR.reduced_kkt(P, A, act)
        assert np.linalg.cond(K) <= AR.MAX_COND
        ref = AR.adjoint_ref(P, A, act, x, y, gx[b], gy[b])
        e, k = AR.worst_ratio({k: out[k][b] for k in KEYS}, ref, x, y)
        worst = max(worst, e)
        if name == "equality_row":
            marked, other = ("dl", "du") if act[2] < 0 else ("du", "dl")
            assert out[other][b, 2] == 0.0 and out[marked][b, 2] != 0.0
    print(f"adjoint edge {name} scaling={scaling}: worst ratio {worst:.3e}")
    assert worst <= AR.GPU_BOUND, (name, worst)
    s.close()
