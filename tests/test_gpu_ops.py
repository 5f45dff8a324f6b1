"""GPU (-m gpu): the SpMV op on every launch form and the KKT-solve op by its backward error, both against the plain
references of tests/op_refs.py, with scaling off and on, and after every kind of data change.

The SpMV forms (mi_osqp_batch_spmv / launch_spmv_fused), chosen at setup:
  fused_qp     spmv_fused_qp_kernel, one QP per workgroup: fused tables, ELL form, n_tiles % 8 == 0
  fused_ell    spmv_fused_kernel<BT>, ELL branch: fused tables, ELL form, n_tiles % 8 != 0
  fused_csr    spmv_fused_kernel<BT>, CSR loop: fused tables, a row > 24 entries or > 2048 rows
  stream_lds   spmv_kernel, output in LDS: no fused tables, (Next + 2n + m) BT doubles fit the op's LDS
  stream_out1  spmv_kernel, output in the tile's global scratch: the same doubles do not fit, or a global solve vector"""
import numpy as np
import pytest
import scipy.sparse as sp

import op_refs as R
import osqp_solver_amd as M
from oracle import oracle as O
from osqp_solver_amd import problems as PR
from test_op_references import KKT_BWD_GPU

pytestmark = pytest.mark.gpu
SCALING_ITERS = 10


def expected_spmv_form(stats, P, A):
    """The choice rules of solver.hip (tables of the fused SpMV op, mi_osqp_batch_spmv, launch_spmv_fused) restated."""
    n, m, BT = stats["n"], stats["m"], stats["tile"]
    nw = stats["threads_per_block"] // 64
    fixed = nw * 14 * BT + 14 * BT                               # lds_bytes(): the reduction scratch
    global_xs = stats["lds_bytes"] == fixed * 8                  # (lds_bytes(0, ...): the solve vector is in global memory)
    pa_len = stats["nnz_P_triu"] + stats["nnz_A"]
    if not global_xs and pa_len < 65536 and n + m < 65536 and (pa_len + 2 + n + m) * BT * 8 <= 150 * 1024:
        Pf = R.sym_full(P)
        A = R.Coo.from_scipy(A)
        longest = max(Pf.row_lengths().max(initial=0), A.T().row_lengths().max(initial=0), A.row_lengths().max(initial=0))
        if 2 * n + m <= 2048 and longest <= 24:
            return "fused_qp" if stats["n_tiles"] % 8 == 0 else "fused_ell"
        return "fused_csr"
    Next = (stats["lds_bytes"] // 8 - fixed) // BT - 2 * stats["dense_tail_rows"]
    if not global_xs and (Next + 2 * n + m) * BT * 8 <= 160 * 1024 - 1024:
        return "stream_lds"
    return "stream_out1"


# ------------------------------------------------------------------ problems
def box(B, n=96, mg=64, k=6, **kw):
    return PR.random_box_qp(B, n=n, mg=mg, nnz_per_row=k, **kw)


def with_dense_row(pr, k=40, seed=3):
    """one more A row with k entries (the CSR loop of the fused kernel)"""
    rng = np.random.default_rng(seed)
    cols = rng.choice(pr["n"], size=k, replace=False)
    row = sp.csr_matrix((np.ones(k), (np.zeros(k, int), cols)), shape=(1, pr["n"]))
    A_pat = sp.vstack([pr["A"], row]).tocsc(); A_pat.sort_indices()
    Ax = []
    for b in range(pr["Ax"].shape[0]):
        A = PR.qp_matrices(pr, b)[1]
        rb = row.copy(); rb.data = rng.uniform(0.5, 1.5, k)
        Ab = sp.vstack([A, rb]).tocsc(); Ab.sort_indices()
        assert np.array_equal(Ab.indices, A_pat.indices)
        Ax.append(Ab.data)
    B = len(Ax)
    return dict(pr, A=A_pat, Ax=np.array(Ax), m=pr["m"] + 1,
                l=np.hstack([pr["l"], -np.ones((B, 1))]), u=np.hstack([pr["u"], np.ones((B, 1))]))


def with_full_P(pr):
    """P passed with both triangles"""
    Pf = sp.csc_matrix(R_sym(pr["P"])); Pf.sort_indices()
    Px = []
    for b in range(pr["Px"].shape[0]):
        Pb = sp.csc_matrix(R_sym(PR.qp_matrices(pr, b)[0])); Pb.sort_indices()
        Px.append(Pb.data)
    return dict(pr, P=Pf, Px=np.array(Px))


def R_sym(P):
    P = sp.csc_matrix(P)
    return sp.triu(P) + sp.triu(P, 1).T


def edge_qp(B=3, n=6, m=5, seed=9):
    """an empty P column, an empty A row and an empty A column"""
    rng = np.random.default_rng(seed)
    Pd = np.diag(rng.uniform(1, 2, n)); Pd[0, 1] = 0.2; Pd[2, 2] = 0.0
    Ad = rng.standard_normal((m, n)); Ad[:, 2] = 0.0; Ad[1, :] = 0.0; Ad[:, 4] = 0.0; Ad[0, 4] = 1.0
    Pp = sp.csc_matrix(np.triu(Pd) != 0, dtype=float); Ap = sp.csc_matrix(Ad != 0, dtype=float)
    Pp.sort_indices(); Ap.sort_indices()
    Px = np.array([Pd.T[np.triu(Pd).T != 0] * (1 + 0.1 * b) for b in range(B)])
    Ax = np.array([Ad.T[Ad.T != 0] * (1 - 0.1 * b) for b in range(B)])
    return dict(n=n, m=m, P=Pp, A=Ap, Px=Px, Ax=Ax, q=rng.standard_normal((B, n)),
                l=-np.ones((B, m)), u=np.ones((B, m)))


def tiny_qp(B, n, m):
    """n = 1 or m = 0"""
    rng = np.random.default_rng(n * 10 + m)
    P = sp.csc_matrix(np.eye(n)); A = sp.csc_matrix(np.ones((m, n)))
    return dict(n=n, m=m, P=P, A=A, Px=rng.uniform(1, 2, (B, n)), Ax=rng.uniform(0.5, 1.5, (B, m * n)),
                q=rng.standard_normal((B, n)), l=-np.ones((B, m)), u=np.ones((B, m)))


def make(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


# ------------------------------------------------------------------ SpMV checks
def run_spmv(s, x, y, outputs=("Px", "Aty", "Ax"), sentinel=None):
    import torch
    B, n, m = s.B, s.n, s.m
    tx = None if x is None else torch.tensor(x, device="cuda")
    ty = None if y is None else torch.tensor(y, device="cuda")
    bufs = {}
    for key, w in (("Px", n), ("Aty", n), ("Ax", m)):
        if key in outputs:
            bufs[key] = torch.full((B + 1, max(w, 1)), np.nan if sentinel is None else sentinel, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                                       # (the fills run on torch's stream, the op on the handle's own)
    s.spmv_device(tx, ty, *(bufs[k][:B] if k in bufs else None for k in ("Px", "Aty", "Ax")))
    out = {k: v.cpu().numpy() for k, v in bufs.items()}
    if sentinel is not None:
        for k, v in out.items():
            assert np.all(v[B] == sentinel), k                    # nothing written past QP B - 1
    return {k: v[:B, :(n if k != "Ax" else m)] for k, v in out.items()}


def check_spmv(s, pr, x, y, outputs=("Px", "Aty", "Ax"), scaled=None, sentinel=None):
    """every output row inside the bound of op_refs.spmv_ref (scaled: the handle's scaling() in force)"""
    out = run_spmv(s, x, y, outputs, sentinel)
    D, E, c = s.scaling() if scaled is None else scaled
    iters = int(s.settings.scaling)
    for b in range(s.B):
        P, A = PR.qp_matrices(pr, b)
        Ps, As, _, _, _ = R.scaled_qp(P, A, None, np.zeros(s.m), np.zeros(s.m), D[b], E[b], c[b])
        ref = R.spmv_ref(Ps, As, None if x is None else x[b], None if y is None else y[b])
        for k in outputs:
            val, mag, ln = ref[k]
            err = np.abs(out[k][b] - val.astype(np.float64))
            tol = R.spmv_tol(mag, ln, iters)
            assert np.all(err <= tol), (k, b, int(np.argmax(err - tol)), float(np.max(err - tol)))
    return out


def vectors(B, n, m, seed=2):
    rng = np.random.default_rng(seed)
    return R_logu(rng, (B, n)), R_logu(rng, (B, m))


def R_logu(rng, shape):
    return rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-2, 2, shape)


# (form, BT, B, problem, env)
SPMV_CASES = [
    ("fused_qp", 1, 8, "box", {}), ("fused_qp", 2, 16, "box", {}), ("fused_qp", 2, 15, "box", {}),
    ("fused_qp", 4, 32, "box", {}), ("fused_qp", 4, 31, "box", {}),
    ("fused_ell", 1, 9, "box", {}), ("fused_ell", 2, 10, "box", {}), ("fused_ell", 4, 13, "box", {}),
    ("fused_csr", 1, 9, "dense_row", {}), ("fused_csr", 2, 9, "dense_row", {}), ("fused_csr", 4, 9, "dense_row", {}),
    ("stream_out1", 1, 5, "box", {"MI_OSQP_GLOBAL_XS": "1"}), ("stream_out1", 2, 5, "box", {"MI_OSQP_GLOBAL_XS": "1"}),
    ("stream_out1", 4, 5, "box", {"MI_OSQP_GLOBAL_XS": "1"}),
    ("stream_lds", 2, 4, "box512k12", {}), ("stream_lds", 4, 8, "box320", {}),
    ("stream_out1", 4, 4, "box1000", {}),
]


def spmv_problem(name, B):
    if name == "box":
        return box(B)
    if name == "dense_row":
        return with_dense_row(box(B))
    if name == "box512k12":
        return box(B, n=512, mg=512, k=12)
    if name == "box320":
        return box(B, n=320, mg=320, k=8)
    if name == "box1000":
        return box(B, n=1000, mg=500, k=8)
    raise KeyError(name)


def _env(monkeypatch, BT, env):
    for k in ("MI_OSQP_TILE", "MI_OSQP_GLOBAL_XS", "MI_OSQP_GROUPS", "MI_OSQP_DENSE_TAIL", "MI_OSQP_RELAX",
              "MI_OSQP_HOST_RUIZ", "MI_OSQP_DEVICE_RUIZ"):
        monkeypatch.delenv(k, raising=False)
    if BT:
        monkeypatch.setenv("MI_OSQP_TILE", str(BT))
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("case", SPMV_CASES, ids=lambda c: f"{c[0]}-BT{c[1]}-B{c[2]}-{c[3]}")
def test_spmv_form_matrix(case, monkeypatch):
    form, BT, B, name, env = case
    _env(monkeypatch, BT, env)
    pr = spmv_problem(name, B)
    x, y = vectors(B, pr["n"], pr["m"])
    for scaling in (0, SCALING_ITERS):
        s = make(pr, scaling=scaling)
        st = s.stats()
        assert st["tile"] == BT
        assert expected_spmv_form(st, pr["P"], pr["A"]) == form
        D, E, c = s.scaling()
        if scaling == 0:
            assert np.all(D == 1) and np.all(E == 1) and np.all(c == 1)
        out = check_spmv(s, pr, x, y, sentinel=-7.25)
        again = run_spmv(s, x, y)
        for k in out:
            np.testing.assert_array_equal(out[k], again[k])       # deterministic: bitwise repeatable
        # only some outputs, and x / y read as zeros when absent
        check_spmv(s, pr, x, y, outputs=("Ax",), scaled=(D, E, c))
        check_spmv(s, pr, None, y, outputs=("Px", "Aty"), scaled=(D, E, c))
        check_spmv(s, pr, x, None, scaled=(D, E, c))
        s.close()


def test_wide_grid_spmv_and_scaling(monkeypatch):
    """n + m = 89 700: 32-bit index words, global solve vector (spmv_kernel<..., GX, WIDE>).  Equilibrated on the device,
    which at this size is ruiz_kernel (the register form ruiz_reg_kernel takes n + m <= 16384), at setup and after new A
    values."""
    monkeypatch.setenv("MI_OSQP_DEVICE_RUIZ", "1")
    pr = PR.grid_qp(150)
    x, y = vectors(1, pr["n"], pr["m"])
    for scaling in (0, SCALING_ITERS):
        s = make(pr, scaling=scaling)
        assert expected_spmv_form(s.stats(), pr["P"], pr["A"]) == "stream_out1"
        check_spmv(s, pr, x, y)
        Ax = pr["Ax"] * (1.0 + 0.25 * np.cos(np.arange(pr["Ax"].shape[1])))
        s.update_A(Ax)
        check_spmv(s, dict(pr, Ax=Ax), x, y)
        s.close()


@pytest.mark.parametrize("variant", ["full_P", "edges", "n1", "m0"])
@pytest.mark.parametrize("env", [{}, {"MI_OSQP_GLOBAL_XS": "1"}], ids=["fused", "stream"])
def test_spmv_edge_shapes(variant, env, monkeypatch):
    _env(monkeypatch, 0, env)
    pr = {"full_P": lambda: with_full_P(box(9)), "edges": lambda: edge_qp(), "n1": lambda: tiny_qp(5, 1, 2),
          "m0": lambda: tiny_qp(5, 4, 0)}[variant]()
    x, y = vectors(pr["Px"].shape[0], pr["n"], pr["m"], seed=5)
    for scaling in (0, SCALING_ITERS):
        s = make(pr, scaling=scaling)
        form = expected_spmv_form(s.stats(), pr["P"], pr["A"])
        assert form.startswith("fused") == (not env), form
        check_spmv(s, pr, x, y, sentinel=3.5)
        s.close()


def test_all_forms_agree_within_the_bound(monkeypatch):
    B = 16
    pr = box(B)
    x, y = vectors(B, pr["n"], pr["m"], seed=8)
    outs = {}
    for BT, env in ((2, {}), (4, {}), (1, {}), (2, {"MI_OSQP_GLOBAL_XS": "1"})):
        _env(monkeypatch, BT, env)
        s = make(pr)
        form = expected_spmv_form(s.stats(), pr["P"], pr["A"])
        outs[(form, BT)] = (run_spmv(s, x, y), s.scaling())
        s.close()
    assert {f for f, _ in outs} >= {"fused_qp", "fused_ell", "stream_out1"}
    (o0, (D, E, c)), rest = list(outs.values())[0], list(outs.values())[1:]
    for o1, (D1, E1, c1) in rest:
        np.testing.assert_array_equal(D, D1); np.testing.assert_array_equal(E, E1); np.testing.assert_array_equal(c, c1)
        for b in range(B):
            P, A = PR.qp_matrices(pr, b)
            Ps, As, _, _, _ = R.scaled_qp(P, A, None, np.zeros(pr["m"]), np.zeros(pr["m"]), D[b], E[b], c[b])
            ref = R.spmv_ref(Ps, As, x[b], y[b])
            for k in ("Px", "Aty", "Ax"):
                _, mag, ln = ref[k]
                assert np.all(np.abs(o0[k][b] - o1[k][b]) <= 2 * R.spmv_tol(mag, ln, SCALING_ITERS)), k


@pytest.mark.parametrize("case", [c for c in SPMV_CASES if c[0].startswith("fused") and c[3] in ("box", "dense_row")],
                         ids=lambda c: f"{c[0]}-BT{c[1]}-B{c[2]}-{c[3]}")
def test_spmv_nonfinite_entry_stays_in_its_rows(case, monkeypatch):
    """x[0] = inf in QP 0: rows whose stored pattern holds column 0 are not finite, every other row of every QP stays
    finite and equal to the result with x[0] = 0 (a padding entry of the ELL tables must not read x[0]: 0 * inf = NaN).
    The fused forms only: the stream forms walk the check schedule of the solve, whose idle lanes gather vector entry 0."""
    form, BT, B, name, env = case
    _env(monkeypatch, BT, env)
    pr = spmv_problem(name, B)
    x, y = vectors(B, pr["n"], pr["m"], seed=4)
    s = make(pr, scaling=0)
    xi = x.copy(); xi[0, 0] = np.inf
    out = run_spmv(s, xi, y)
    P, A = PR.qp_matrices(pr, 0)
    Pf = R.sym_full(P)
    A = R.Coo.from_scipy(A)
    hits = {"Px": set(Pf.rows[Pf.cols == 0]), "Aty": set(), "Ax": set(A.rows[A.cols == 0])}
    xr = x.copy(); xr[0, 0] = 0.0
    ref0 = run_spmv(s, xr, y)
    for k in ("Px", "Aty", "Ax"):
        for r in range(out[k].shape[1]):
            if r in hits[k]:
                assert not np.isfinite(out[k][0, r]), (k, r)
            else:
                assert out[k][0, r] == ref0[k][0, r], (k, r)
        np.testing.assert_array_equal(out[k][1:], ref0[k][1:])


# ------------------------------------------------------------------ KKT solve: backward error
def kkt_check(s, pr, rho=None, qps=None, seed=3):
    """backward error of the KKT-solve op against K assembled from the raw data and the handle's scaling()"""
    import torch
    B, n, m = s.B, s.n, s.m
    D, E, c = s.scaling()
    if rho is None:
        rho = [s.settings.rho] * B
    rhs = np.random.default_rng(seed).standard_normal((B, n + m))
    trhs = torch.tensor(rhs, device="cuda"); sol = torch.full_like(trhs, np.nan)
    torch.cuda.synchronize()                                       # (the fill runs on torch's stream, the op on the handle's own)
    s.kkt_solve_device(trhs, sol)
    sol = sol.cpu().numpy()
    worst = 0.0
    for b in (range(B) if qps is None else qps):
        P, A = PR.qp_matrices(pr, b)
        Ps, As, _, ls, us = R.scaled_qp(P, A, None, pr["l"][b], pr["u"][b], D[b], E[b], c[b])
        K = R.kkt_matrix(Ps, As, s.settings.sigma, R.rho_vec(ls, us, rho[b]))
        worst = max(worst, R.backward_error(K, sol[b], rhs[b]))
    assert worst <= KKT_BWD_GPU, worst
    return worst


KKT_FORMS = [("tile1", 1, {}), ("tile2", 2, {}), ("tile4", 4, {}), ("tail64", 0, {"MI_OSQP_DENSE_TAIL": "64"}),
             ("tail0", 0, {"MI_OSQP_DENSE_TAIL": "0"}), ("gx_groups0", 0, {"MI_OSQP_GLOBAL_XS": "1", "MI_OSQP_GROUPS": "0"}),
             ("gx_groups16", 0, {"MI_OSQP_GLOBAL_XS": "1", "MI_OSQP_GROUPS": "16"}), ("relax16", 0, {"MI_OSQP_RELAX": "16"})]


@pytest.mark.parametrize("form", KKT_FORMS, ids=lambda f: f[0])
def test_kkt_solve_backward_error(form, monkeypatch):
    name, BT, env = form
    _env(monkeypatch, BT, env)
    B = 1 if name.startswith("gx") else 6
    pr = box(B)
    s = make(pr, eps_abs=1e-8, eps_rel=1e-8)
    kkt_check(s, pr)                                              # fresh handle: settings.rho
    pr2 = dict(pr, l=pr["l"] * 0.05, u=pr["u"] * 0.05)            # tight boxes: rho adapts
    s.update_bounds(pr2["l"], pr2["u"])
    info = s.solve()
    assert any(i.rho_updates > 0 for i in info)
    kkt_check(s, pr2, rho=[i.rho for i in info])
    s.refactor_device()
    kkt_check(s, pr2, rho=[i.rho for i in info])
    # and the oracle's equilibration of the same data
    for b in range(min(B, 2)):
        P, A = PR.qp_matrices(pr, b)
        Do, Eo, co = O.OracleQPSolver(P, pr["q"][b], A, pr["l"][b], pr["u"][b]).scaling()
        D, E, c = s.scaling()
        np.testing.assert_allclose(D[b], Do, rtol=1e-13, atol=0); np.testing.assert_allclose(E[b], Eo, rtol=1e-13, atol=0)
        assert abs(c[b] - co) <= 1e-13 * co


def test_kkt_solve_backward_error_wide_grid():
    pr = PR.grid_qp(150)
    s = make(pr)
    kkt_check(s, pr)


# ------------------------------------------------------------------ after data changes
class _Shard(M.BatchSolver):
    """a shard's handle of a MultiBatchSolver, seen as a BatchSolver (owned by the multi handle)"""

    def __init__(self, handle, n, m, B, settings):
        self._h, self.n, self.m, self.B, self.settings = handle, n, m, B, settings

    def __del__(self):
        pass

    close = __del__


def shard_views(multi):
    import ctypes as C
    views = []
    for k, (_, b0, b1) in enumerate(multi.shards()):
        h = C.c_void_p()
        d, b, e = C.c_int64(), C.c_int64(), C.c_int64()
        M.lib().mi_osqp_multi_batch_shard(multi._h, k, C.byref(d), C.byref(b), C.byref(e), C.byref(h))
        views.append((_Shard(h, multi.n, multi.m, int(b1 - b0), multi.settings), int(b0), int(b1)))
    return views


def _sub(pr, b0, b1):
    return dict(pr, Px=pr["Px"][b0:b1], Ax=pr["Ax"][b0:b1], q=pr["q"][b0:b1], l=pr["l"][b0:b1], u=pr["u"][b0:b1])


UPDATES = ["update_A", "update_A_bounds", "update_P", "update_P_full", "update_P_A", "update_q", "update_A_bounds_device",
           "some", "multi"]


@pytest.mark.parametrize("update", UPDATES)
@pytest.mark.parametrize("ruiz", ["host", "device"])
@pytest.mark.parametrize("handle", ["fused", "stream"])
def test_ops_after_data_changes(handle, ruiz, update, monkeypatch):
    import torch
    # the stream handle: no fused tables at tile 4 (the continuous calls need an LDS-resident solve vector)
    _env(monkeypatch, 4 if handle == "stream" else 0, {})
    monkeypatch.setenv("MI_OSQP_HOST_RUIZ" if ruiz == "host" else "MI_OSQP_DEVICE_RUIZ", "1")
    B = 6
    dims = dict(n=320, mg=320, k=8) if handle == "stream" else {}
    pr = box(B, **dims)
    other = box(B, value_seed=7000, **dims)
    rng = np.random.default_rng(12)
    new = dict(pr)
    if update == "multi":
        multi = M.MultiBatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], devices=(0, 0))
        multi.update_P_A(other["Px"], other["Ax"])
        new = dict(pr, Px=other["Px"], Ax=other["Ax"])
        handles = [(v, _sub(new, b0, b1)) for v, b0, b1 in shard_views(multi)]
        assert len(handles) == 2
    else:
        s = make(pr)
        form = expected_spmv_form(s.stats(), pr["P"], pr["A"])
        assert form.startswith("fused") == (handle == "fused"), form
        before = s.scaling()
        if update == "update_A":
            s.update_A(other["Ax"]); new["Ax"] = other["Ax"]
        elif update == "update_A_bounds":
            new.update(Ax=other["Ax"], l=pr["l"] * 0.9, u=pr["u"] * 1.1)
            s.update_A_bounds(new["Ax"], new["l"], new["u"])
        elif update == "update_P":
            s.update_P(other["Px"]); new["Px"] = other["Px"]
        elif update == "update_P_full":
            full = with_full_P(other)
            s.update_P(full["Px"], P_pattern=full["P"]); new["Px"] = other["Px"]
        elif update == "update_P_A":
            s.update_P_A(other["Px"], other["Ax"]); new.update(Px=other["Px"], Ax=other["Ax"])
        elif update == "update_q":
            s.update_q(other["q"]); new["q"] = other["q"]
        elif update == "update_A_bounds_device":
            new.update(Ax=other["Ax"], l=pr["l"] * 0.8, u=pr["u"] * 0.9)
            s.update_A_bounds_device(*(torch.tensor(new[k], device="cuda") for k in ("Ax", "l", "u")))
        elif update == "some":
            ids = [1, 4]
            Ax = pr["Ax"].copy(); Ax[ids] = other["Ax"][ids]
            l, u = pr["l"].copy(), pr["u"].copy(); l[ids] *= 0.7; u[ids] *= 0.6
            s.update_A_bounds_some(ids, Ax[ids], l[ids], u[ids])
            s.reinit_some([4], Ax[[4]], l[[4]], u[[4]])
            new.update(Ax=Ax, l=l, u=u)
        handles = [(s, new)]
    for h, prn in handles:
        D, E, c = h.scaling()
        if update == "update_q":
            for a, b in zip((D, E, c), before):
                np.testing.assert_array_equal(a, b)
        else:
            for b in ((0, 1, 4) if update == "some" else range(min(h.B, 2))):       # ("some": QP 0 and both listed QPs)
                P, A = PR.qp_matrices(prn, b)
                Do, Eo, co = O.OracleQPSolver(P, prn["q"][b], A, prn["l"][b], prn["u"][b]).scaling()
                np.testing.assert_allclose(D[b], Do, rtol=1e-13, atol=0)
                np.testing.assert_allclose(E[b], Eo, rtol=1e-13, atol=0)
                assert abs(c[b] - co) <= 1e-13 * co
        x, y = vectors(h.B, prn["n"], prn["m"], seed=6)
        check_spmv(h, prn, x, y, scaled=(D, E, c))
        kkt_check(h, prn)
