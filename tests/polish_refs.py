"""References for solution polishing ("Solution polishing", steps 2-4), written from the mathematics
alone in the scaled data: np.float64 and an mpmath twin at 50 digits.  No solver code is involved.

With D, E, c the handle's scaling, the scaled problem is Ps = c D P D, As = E A D, qs = c D q, ls = E l, us = E u
(op_refs.scaled_qp).  For an active set act (-1 lower, +1 upper, 0 inactive), A~ = As with its inactive rows zeroed:
  K_d = [[Ps + d I, A~'], [A~, -d I]],   K = [[Ps, A~'], [A~, 0]],   b = [-qs; ls_j (lower) | us_j (upper) | 0]
  s_0 = K_d^-1 b,   s_{k+1} = s_k + K_d^-1 (b - K s_k)   for refine_iter rounds, every K_d^-1 applied exactly
  x = s_x,  z = As x,  y = s_y on the active rows, 0 elsewhere;   t = z + y,  z = clip(t, ls, us),  y = t - z
  pri = |As x - z|_inf,  dua = |Ps x + qs + As'y|_inf,  obj = 1/2 x'Ps x + qs'x          (the scaled residuals of OSQP)
and, with scaling on and scaled_termination off, the unscaled ones OSQP reports: pri = |E^-1 (As x - z)|_inf,
dua = |D^-1 (Ps x + qs + As'y)|_inf / c; obj / c whenever scaling is on.  m = 0: pri = 0.  The caller sees x = D s_x and
y = E y / c.  The polished point is accepted if
  (pri < pri0 and dua < dua0) or (pri < pri0 and dua0 < 1e-10) or (dua < dua0 and pri0 < 1e-10)
with pri0, dua0 the residuals of the ADMM's last termination check.

Errors are measured in term scales: x and y in units of max(1, |.|_inf) of the caller-space vector, a residual in units
of the largest magnitude sum of its terms (|Ps||x| + |qs| + |As'||y| and |As||x| + |z|, each row unscaled the way its
residual is), obj in 1/2 |x|'|Ps||x| + |qs|'|x|.

TWIN_ERROR is the largest such error of the float64 reference against its mpmath twin on the six QPs the GPU tests use
(tests/test_polish_refs.py measures and pins it); POLISH_BOUND = 32 x that, the margin dh_refs uses for a device that sums
in another order, with a floor of 1e-13."""
import numpy as np

import adjoint_refs as AR
import op_refs as R

DPS = AR.DPS
TWIN_ERROR = 2e-15          # measured 1.64e-15 (x of QP 4 at delta = 1e-6, round 0); y 1.57e-15, pri 4.8e-16, dua 4.5e-16, obj 3.0e-16
POLISH_BOUND = max(32 * TWIN_ERROR, 1e-13)
MAX_BOUND = 1e-10           # POLISH_BOUND may not exceed this: test_polish_refs asserts rounds at delta = 1e-2 >= 2.5e-7 apart
SMALL_RES = 1e-10           # the threshold of clauses 2 and 3 of the acceptance rule
DUAL_FLOOR = 1e-9           # |y| below this reads as 0 in active_from_dual

# The scenarios of the GPU tests (settings beside polish = 1); tests/test_polish_refs.py asserts on the CPU oracle what the
# GPU tests presuppose of each.
#   S1  accepted, residuals of round-off                      S2, S6  accepted, residuals of 4e-8 .. 4e-6 (not round-off)
#   S3  rejected with every deciding margin >= 1e5            S4      accepted; pri0 or dua0 below 1e-10 for QPs 0, 2, 3, 5
#   S5  accepted by clause 3 alone (QPs 0, 2, 3) and by clause 2 alone (QP 5): the polished residuals lie beside the ADMM's
# (In S4 clause 1 holds wherever clause 2 or 3 does: a default polish leaves residuals of 1e-16, below any ADMM residual.)
SCENARIOS = dict(S1=dict(eps=1e-7, delta=1e-6, rounds=3), S2=dict(eps=1e-3, delta=1e-6, rounds=0),
                 S3=dict(eps=1e-9, delta=1e-4, rounds=0), S4=dict(eps=1e-9, delta=None, rounds=None),
                 S5=dict(eps=1e-9, delta=1e-3, rounds=3), S6=dict(eps=1e-3, delta=1e-2, rounds=3))
DEFAULT_DELTA, DEFAULT_ROUNDS = 1e-6, 3

# Refinement rounds and delta at eps 1e-3, (delta, rounds).  ACCEPTED_ROUND_CASES holds one case per round count 0 .. 3 that the
# rule accepts for all six QPs, each >= 1000 POLISH_BOUND away from rounds k - 1, k + 1 and from either flipped sign
# (tests/test_polish_refs.py asserts both).  In the other cases the rule rejects some or all QPs - after round 0 the residuals
# are delta |y| and delta |x|, above the ADMM's at delta 1e-2 - and a rejected polish publishes nothing: there the GPU test
# checks verdicts, rejected QPs bit for bit and accepted ones against their round.
ROUND_EPS = 1e-3
ROUND_CASES = [(1e-2, 0), (1e-2, 1), (1e-2, 2), (1e-2, 3), (1e-6, 0), (1e-4, 0), (1e-4, 1), (1e-3, 2)]
ACCEPTED_ROUND_CASES = [(1e-6, 0), (1e-4, 1), (1e-3, 2), (1e-2, 3)]

# A tile partner that is not polished: one handle at eps 1e-3 and max_iter 50 whose QPs get these rho values (update_rho_each);
# with rho = 1 a QP is optimal after 25 or 50 iterations, with rho = 1e-3 it runs into max_iter (status -2).
PARTNER = dict(eps=1e-3, max_iter=50, rho=[1.0, 1e-3, 1e-3, 1.0, 1.0, 1.0], status=[1, -2, -2, 1, 1, 1])


def scenario_settings(name):
    """the solver settings of a scenario (S4: the handle's default delta and polish_refine_iter)"""
    sc = SCENARIOS[name]
    kw = dict(polish=1, eps_abs=sc["eps"], eps_rel=sc["eps"])
    if sc["delta"] is not None:
        kw.update(delta=sc["delta"], polish_refine_iter=sc["rounds"])
    return kw


# ------------------------------------------------------------------ the scaled problem in one number type
def _num_float(v):
    return float(v)                                        # (rounds the long double of op_refs to fp64)


def _num_mp(v):
    import mpmath as mp
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - R.LD(hi)))        # the long double, exactly


class Scaled:
    """the scaled problem as sparse triplets and vectors of one number type (num: long double -> that type)"""

    def __init__(self, P, q, A, l, u, D, E, c, num):
        import scipy.sparse as sp
        A = sp.csc_matrix(A)
        self.m, self.n = A.shape
        q = np.zeros(self.n) if q is None else q
        Ps, As, qs, ls, us = R.scaled_qp(P, A, q, l, u, D, E, c)
        self.P = [(int(i), int(j), num(v)) for i, j, v in zip(Ps.rows, Ps.cols, Ps.vals)]
        self.A = [(int(i), int(j), num(v)) for i, j, v in zip(As.rows, As.cols, As.vals)]
        self.q, self.l, self.u = [num(v) for v in qs], [num(v) for v in ls], [num(v) for v in us]
        self.D, self.E, self.c = [num(R.LD(v)) for v in D], [num(R.LD(v)) for v in E], num(R.LD(c))
        self.zero = num(R.LD(0))


def _matvec(ent, v, rows, zero, transpose=False, mag=False):
    out = [zero] * rows
    for i, j, a in ent:
        if transpose:
            i, j = j, i
        out[i] += abs(a * v[j]) if mag else a * v[j]
    return out


def _solver_float(Kd):
    import scipy.linalg as sla
    lu = sla.lu_factor(np.array(Kd, dtype=np.float64))
    return lambda r: [float(v) for v in sla.lu_solve(lu, np.array(r, dtype=np.float64))]


def _solver_mp(Kd):
    return lambda r: AR.mp_solve(Kd, r)


def refine_rounds(pb, act, delta, rounds, make_solver, signs=(1, -1)):
    """[s_0, .., s_rounds], s_k = [x; y] in the scaled data, natural order (y over all m rows, 0 on the inactive ones).
    signs: the signs of the delta blocks of K_d (the rule's are +, -; the others are what a test flips)."""
    n, m, zero = pb.n, pb.m, pb.zero
    N = n + m
    K = list(pb.P) + [e for i, j, a in pb.A if act[i] for e in ((n + i, j, a), (j, n + i, a))]
    Kd = [[zero] * N for _ in range(N)]
    for i, j, a in K:
        Kd[i][j] += a
    d = zero + delta
    for i in range(N):
        Kd[i][i] += d * signs[0] if i < n else d * signs[1]
    b = [-v for v in pb.q] + [pb.l[i] if act[i] < 0 else pb.u[i] if act[i] > 0 else zero for i in range(m)]
    solve = make_solver(Kd)
    s = solve(b)
    out = [s]
    for _ in range(rounds):
        Ks = _matvec(K, s, N, zero)
        corr = solve([b[i] - Ks[i] for i in range(N)])
        s = [s[i] + corr[i] for i in range(N)]
        out.append(s)
    return out


def finish(pb, act, s, scaling=1, scaled_termination=0):
    """the ending of a polish at the refinement iterate s: projection, residuals, objective, caller-space solution and the
    term scales of every quantity"""
    n, m, zero = pb.n, pb.m, pb.zero
    x = list(s[:n])
    z = _matvec(pb.A, x, m, zero)
    t = [z[i] + (s[n + i] if act[i] else zero) for i in range(m)]
    zc = [min(max(t[i], pb.l[i]), pb.u[i]) for i in range(m)]
    y = [t[i] - zc[i] for i in range(m)]
    Px, Aty = _matvec(pb.P, x, n, zero), _matvec(pb.A, y, n, zero, transpose=True)
    dres = [Px[i] + pb.q[i] + Aty[i] for i in range(n)]
    pres = [z[i] - zc[i] for i in range(m)]
    dmag = [a + abs(qv) + b for a, qv, b in zip(_matvec(pb.P, x, n, zero, mag=True), pb.q,
                                                _matvec(pb.A, y, n, zero, transpose=True, mag=True))]
    pmag = [a + abs(b) for a, b in zip(_matvec(pb.A, x, m, zero, mag=True), zc)]
    unscale = bool(scaling) and not scaled_termination
    wd = [1 / (pb.c * dv) for dv in pb.D] if unscale else [zero + 1] * n
    wp = [1 / ev for ev in pb.E] if unscale else [zero + 1] * m
    cinv = 1 / pb.c if scaling else zero + 1
    big = lambda vals, w: max([abs(v) * wi for v, wi in zip(vals, w)], default=zero)
    xc, yc = [pb.D[i] * x[i] for i in range(n)], [pb.E[i] * y[i] / pb.c for i in range(m)]
    one = zero + 1
    return dict(
        x=xc, y=yc, xs=x, ys=y, zs=zc,
        pri=big(pres, wp), dua=big(dres, wd),
        obj=cinv * sum((Px[i] / 2 + pb.q[i]) * x[i] for i in range(n)),
        scale=dict(x=max([one] + [abs(v) for v in xc]), y=max([one] + [abs(v) for v in yc]),
                   pri=big(pmag, wp), dua=big(dmag, wd),
                   obj=cinv * sum((abs(Px_i) / 2 + abs(qv)) * abs(xv) for Px_i, qv, xv in
                                  zip(_matvec(pb.P, [abs(v) for v in x], n, zero, mag=True), pb.q, x))))


def polish_ref(P, q, A, l, u, D, E, c, act, delta=1e-6, refine_iter=3, scaling=1, scaled_termination=0, signs=(1, -1)):
    """float64 reference: dict(x, y (caller space, arrays), pri, dua, obj, scale, rounds = [caller-space x of s_0 .. s_k])"""
    pb = Scaled(P, q, A, l, u, D, E, c, _num_float)
    ss = refine_rounds(pb, act, delta, refine_iter, _solver_float, signs)
    out = finish(pb, act, ss[-1], scaling, scaled_termination)
    for k in ("x", "y", "xs", "ys", "zs"):
        out[k] = np.array(out[k], dtype=np.float64)
    out["rounds"] = [np.array(pb.D) * np.array(s[:pb.n]) for s in ss]
    return out


def polish_ref_mp(P, q, A, l, u, D, E, c, act, delta=1e-6, refine_iter=3, scaling=1, scaled_termination=0, signs=(1, -1)):
    """the twin at DPS digits: the same dict with mpf entries (lists of mpf for the vectors)"""
    import mpmath as mp
    with mp.workdps(DPS):
        pb = Scaled(P, q, A, l, u, D, E, c, _num_mp)
        ss = refine_rounds(pb, act, mp.mpf(float(delta)), refine_iter, _solver_mp, signs)
        out = finish(pb, act, ss[-1], scaling, scaled_termination)
        out["rounds"] = [[pb.D[i] * s[i] for i in range(pb.n)] for s in ss]
        return out


def worst_ratio(got, ref, keys=("x", "y", "pri", "dua", "obj")):
    """max over the quantities of |got - ref| / term scale (ref: a reference dict, float64 or mpf), and its key"""
    import mpmath as mp
    worst, where = 0.0, None
    with mp.workdps(DPS):
        for k in keys:
            if k in ("x", "y"):
                g = [v for v in np.asarray(got[k], dtype=np.float64)]
                assert len(g) == len(ref[k]) and np.all(np.isfinite(g)), k
                diff = max([abs(mp.mpf(float(a)) - b) for a, b in zip(g, ref[k])], default=0)
            else:
                assert np.isfinite(float(got[k])), k
                diff = abs(mp.mpf(float(got[k])) - ref[k])
            e = 0.0 if diff == 0 else float(diff / ref["scale"][k])
            if e >= worst:
                worst, where = e, k
    return worst, where


# ------------------------------------------------------------------ the acceptance rule and the sign rule
def accept(pri, dua, pri0, dua0):
    """(verdict, margin, clauses that hold): the three-clause rule.  A comparison a < b has the margin max(a, b) / min(a, b)
    (1 at equality, which is not strict and so false).  An acceptance stands while one holding clause keeps both its
    comparisons: margin = the largest, over the holding clauses, of the smaller margin of its two comparisons.  A rejection
    stands until one clause has all its false comparisons turned: margin = the smallest, over the clauses, of the largest
    margin among its false comparisons."""
    def cmp(a, b):
        lo, hi = min(a, b), max(a, b)
        return bool(a < b), (1.0 if a == b else np.inf if lo == 0 else float(hi / lo))
    c = dict(p=cmp(pri, pri0), d=cmp(dua, dua0), p0=cmp(pri0, SMALL_RES), d0=cmp(dua0, SMALL_RES))
    clauses = (("p", "d"), ("p", "d0"), ("d", "p0"))
    holds = [all(c[k][0] for k in cl) for cl in clauses]
    if any(holds):
        margin = max(min(c[k][1] for k in cl) for cl, h in zip(clauses, holds) if h)
    else:
        margin = min(max(c[k][1] for k in cl if not c[k][0]) for cl in clauses)
    return any(holds), margin, [i + 1 for i, h in enumerate(holds) if h]


def active_from_dual(y, floor=DUAL_FLOOR):
    """The active set of a converged (z, y): z - l < -y / u - z < y with z in [l, u] and y = 0 up to round-off off the
    bounds is the sign of y wherever |y| is not round-off.  Returns (int8 active set with |y| < floor read as 0, the number
    of rows with floor 1e-3 < |y| < floor: those are undecided)."""
    y = np.asarray(y, dtype=np.float64)
    act = np.where(np.abs(y) < floor, 0, np.sign(y)).astype(np.int8)
    return act, int(np.count_nonzero((np.abs(y) > floor * 1e-3) & (np.abs(y) < floor)))
