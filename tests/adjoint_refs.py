"""References for the adjoint derivative (mi_osqp.h "adjoint derivative"), written from the mathematics
alone: dense numpy in float64 and an mpmath twin at 50 digits.  No solver code is involved.

For a QP min 1/2 x'Px + q'x, l <= Ax <= u with active set act (-1 lower, +1 upper, 0 inactive), A_a the active rows and
b_a = l_i or u_i on them, the active-set solution solves K [x; y_a] = [-q; b_a], K = [[P, A_a'], [A_a, 0]].  Given
g_x = dL/dx and g_y = dL/dy, with K [r_x; r_a] = [g_x; g_y,a] and r_y = r_a scattered to the active rows:
  dq = -r_x,  dl_i = r_y,i (act_i = -1),  du_i = r_y,i (act_i = +1),  dA_k = -(y_i r_x,j + r_y,i x_j) at (i, j),
  dP_k = -(r_x,i x_i) on the diagonal, -(r_x,i x_j + r_x,j x_i) off it, per stored entry of the upper triangle."""
import numpy as np
import scipy.sparse as sp

DPS = 50


def triu_csc(P):
    """upper triangle of P (given with either or both triangles), CSC with sorted indices: the layout of dP"""
    U = sp.triu(sp.csc_matrix(P)).tocsc()
    U.sort_indices()
    return U


def sym_dense(P):
    U = triu_csc(P).toarray()
    return U + np.triu(U, 1).T


def rows_cols(M):
    M = sp.csc_matrix(M)
    return M.indices.astype(int), np.repeat(np.arange(M.shape[1]), np.diff(M.indptr)).astype(int)


def polish_rule(A, x, y, l, u):
    """the active set OSQP's polish derives from a solution: lower-active z - l < -y, upper-active u - z < y"""
    z = A @ x
    act = np.zeros(len(l), dtype=np.int8)
    act[z - l < -y] = -1
    act[(u - z < y) & (act == 0)] = 1
    return act


def reduced_kkt(P, A, act):
    """(K dense, indices of the active rows)"""
    Pd, Ad = sym_dense(P), sp.csc_matrix(A).toarray()
    ia = np.flatnonzero(act)
    Aa = Ad[ia]
    n = Pd.shape[0]
    K = np.zeros((n + len(ia), n + len(ia)))
    K[:n, :n] = Pd; K[:n, n:] = Aa.T; K[n:, :n] = Aa
    return K, ia


def active_set_solution(P, q, A, l, u, act):
    """(x, y) of the equality-constrained QP the active set defines, float64"""
    K, ia = reduced_kkt(P, A, act)
    n = len(q)
    b = np.where(act[ia] < 0, l[ia], u[ia])
    s = np.linalg.solve(K, np.concatenate([-q, b]))
    y = np.zeros(len(l)); y[ia] = s[n:]
    return s[:n], y


def _gradients(xp, n, m, ia, act, r, x, y, Prc, Arc, zero):
    """the formulas of the module docstring on any number type (r: the solution of K r = g)"""
    rx = [r[i] for i in range(n)]
    ry = [zero] * m
    for k, i in enumerate(ia):
        ry[i] = r[n + k]
    dq = [-v for v in rx]
    dl = [ry[i] if act[i] < 0 else zero for i in range(m)]
    du = [ry[i] if act[i] > 0 else zero for i in range(m)]
    dP = [-(rx[i] * x[i]) if i == j else -(rx[i] * x[j] + rx[j] * x[i]) for i, j in zip(*Prc)]
    dA = [-(y[i] * rx[j] + ry[i] * x[j]) for i, j in zip(*Arc)]
    return dict(dq=xp(dq), dP=xp(dP), dA=xp(dA), dl=xp(dl), du=xp(du), rx=xp(rx), ry=xp(ry))


def adjoint_ref(P, A, act, x, y, gx, gy=None):
    """float64 reference: dict(dq, dP, dA, dl, du, rx, ry)"""
    n, m = len(x), len(act)
    K, ia = reduced_kkt(P, A, act)
    gy = np.zeros(m) if gy is None else gy
    r = np.linalg.solve(K, np.concatenate([gx, gy[ia]])) if len(K) else np.zeros(0)
    return _gradients(lambda v: np.array(v, dtype=float), n, m, ia, act, r, x, y, rows_cols(triu_csc(P)), rows_cols(A), 0.0)


def term_scales(ref, x, y):
    """the scale of every gradient's terms: |r|_inf for dq, dl, du; |r|_inf max(|x|_inf, |y|_inf) for dP, dA"""
    rn = max(np.max(np.abs(ref["rx"]), initial=0.0), np.max(np.abs(ref["ry"]), initial=0.0))
    xy = max(np.max(np.abs(x), initial=0.0), np.max(np.abs(y), initial=0.0))
    return dict(dq=rn, dl=rn, du=rn, dP=rn * xy, dA=rn * xy)


def worst_ratio(got, ref, x, y, keys=("dq", "dP", "dA", "dl", "du")):
    """max over the gradients of max|got - ref| / term scale (and the key it belongs to)"""
    sc = term_scales(ref, x, y)
    worst, where = 0.0, None
    for k in keys:
        if len(ref[k]) == 0:
            continue
        assert np.all(np.isfinite(got[k])), k
        e = float(np.max(np.abs(np.asarray(got[k], float) - np.asarray(ref[k], float)))) / sc[k]
        if e >= worst:
            worst, where = e, k
    return worst, where


# ------------------------------------------------------------------ mpmath twin
def mp_solve(K, b):
    """K s = b at DPS digits: a float64 LU as the preconditioner of a refinement whose residuals are taken in mpmath; the
    last residual is asserted below 1e-45 of |b|.  (A 200 x 200 mpmath LU would take minutes; this takes a second.)"""
    import mpmath as mp
    import scipy.linalg as sla
    N = len(b)
    if N == 0:
        return []
    Kf = np.array([[float(v) for v in row] for row in K])
    lu = sla.lu_factor(Kf)
    nz = [[(j, K[i][j]) for j in range(N) if K[i][j] != 0] for i in range(N)]
    s = [mp.mpf(0)] * N
    bn = max(abs(v) for v in b) or mp.mpf(1)
    for _ in range(12):
        res = [b[i] - mp.fsum(v * s[j] for j, v in nz[i]) for i in range(N)]
        rn = max(abs(v) for v in res)
        if rn <= bn * mp.mpf(10) ** (-(DPS - 3)):
            break
        scale = rn                                            # (keeps the float64 correction in range)
        d = sla.lu_solve(lu, np.array([float(v / scale) for v in res]))
        s = [s[i] + mp.mpf(float(d[i])) * scale for i in range(N)]
    assert rn <= bn * mp.mpf(10) ** (-45), rn
    return s


def _mp_kkt(P, A, act):
    import mpmath as mp
    K, ia = reduced_kkt(P, A, act)
    return [[mp.mpf(float(v)) for v in row] for row in K], ia


def active_set_solution_mp(P, q, A, l, u, act):
    import mpmath as mp
    with mp.workdps(DPS):
        K, ia = _mp_kkt(P, A, act)
        n = len(q)
        b = [-mp.mpf(float(v)) for v in q] + [mp.mpf(float(l[i] if act[i] < 0 else u[i])) for i in ia]
        s = mp_solve(K, b)
        y = [mp.mpf(0)] * len(l)
        for k, i in enumerate(ia):
            y[i] = s[n + k]
        return s[:n], y


def adjoint_ref_mp(P, A, act, x, y, gx, gy=None):
    """the twin of adjoint_ref at DPS digits; x, y: mpmath numbers (or floats); returns lists of mpf"""
    import mpmath as mp
    with mp.workdps(DPS):
        n, m = len(x), len(act)
        K, ia = _mp_kkt(P, A, act)
        g = [mp.mpf(float(v)) for v in gx] + [mp.mpf(float(gy[i])) if gy is not None else mp.mpf(0) for i in ia]
        r = mp_solve(K, g)
        x = [mp.mpf(v) for v in x]; y = [mp.mpf(v) for v in y]
        return _gradients(list, n, m, ia, act, r, x, y, rows_cols(triu_csc(P)), rows_cols(A), mp.mpf(0))


def to_float(d):
    return {k: np.array([float(v) for v in vs]) for k, vs in d.items()}


# ------------------------------------------------------------------ the GPU test problems
GPU_SHAPE = dict(n=96, mg=64, nnz_per_row=6)
GPU_B = 6
ORACLE_EPS = 1e-10
MIN_GAP = 1e-3          # smallest slack of an inactive row and smallest |y| of an active one the fixtures must keep
MAX_COND = 1e3
GPU_BOUND = 1e-9


def gpu_problem(B=GPU_B):
    from osqp_solver_amd import problems as PR
    return PR.random_box_qp(B, **GPU_SHAPE)


def gradient_seeds(B, n, m, seed=11):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, n)), rng.standard_normal((B, m))


_CACHE = {}


def fixture(pr, b, key=None):
    """QP b of the batch dict pr: active set from the oracle at eps 1e-10, the active-set solution, K's conditioning and the
    gaps.  Computed once per (key, b) and shared between the tests; the preconditions are asserted by the caller."""
    from oracle import oracle as O
    from osqp_solver_amd import problems as PR
    if key is not None and (key, b) in _CACHE:
        return _CACHE[(key, b)]
    P, A = PR.qp_matrices(pr, b)
    q = pr["q"][b] if pr["q"] is not None else np.zeros(pr["n"])
    l, u = pr["l"][b], pr["u"][b]
    o = O.OracleQPSolver(P, q, A, l, u, eps_abs=ORACLE_EPS, eps_rel=ORACLE_EPS, max_iter=100000)
    st, xo = o.solve()
    assert st == 1, st
    act = polish_rule(A, xo, o.y, l, u)
    x, y = active_set_solution(P, q, A, l, u, act)
    z = A @ x
    ia = act != 0
    slack = np.minimum(z - l, u - z)[~ia]
    K, _ = reduced_kkt(P, A, act)
    fx = dict(P=P, A=A, q=q, l=l, u=u, act=act, x=x, y=y, x_oracle=xo, y_oracle=o.y.copy(),
              min_slack=float(slack.min(initial=np.inf)), min_mult=float(np.abs(y[ia]).min(initial=np.inf)),
              signs_ok=bool(np.all(y[act < 0] < 0) and np.all(y[act > 0] > 0)),
              cond=float(np.linalg.cond(K)) if len(K) else 1.0,
              inv_norm=float(np.linalg.norm(np.linalg.inv(K), 2)) if len(K) else 0.0)
    if key is not None:
        _CACHE[(key, b)] = fx
    return fx


def assert_preconditions(fx):
    assert fx["signs_ok"]
    assert fx["min_slack"] >= MIN_GAP, fx["min_slack"]
    assert fx["min_mult"] >= MIN_GAP, fx["min_mult"]
    assert fx["cond"] <= MAX_COND, fx["cond"]
