"""References for the ADMM iterates, written from the mathematics and the OSQP 0.6 rules alone (a
helper module of the tests, not a conftest).  No solver code is involved.

With D, E, c a handle's scaling the state (x, z, y) lives in the scaled problem Ps = c D P D, As = E A D, qs = c D q,
ls = E l, us = E u (op_refs.scaled_qp).  rho_vec is op_refs.rho_vec's classification of the scaled bounds (free rows
RHO_MIN, equalities 1e3 rho, the others rho), rho_inv = 1 / rho_vec, K = [[Ps + sigma I, As'], [As, -diag(rho_inv)]].
One iteration (E6-E10):
  rhs = [sigma x - qs ; z - rho_inv y],  K [xt ; nu] = rhs,  zt = z - rho_inv y + rho_inv nu
  x+ = alpha xt + (1 - alpha) x,  zr = alpha zt + (1 - alpha) z,  z+ = clip(zr + rho_inv y, ls, us),  y+ = y + rho_vec (zr - z+)
  delta_x = x+ - x,  delta_y = rho_vec (zr - z+)
The check (E11-E13) of an iterate: r_p = As x - z, r_d = qs + Ps x + As'y;
  scaled:    pri = |r_p|_inf, dua = |r_d|_inf, pri_nrm = max(|z|, |As x|), dua_nrm = max(|qs|, |As'y|, |Ps x|)
  unscaled (scaling and not scaled_termination): pri = |E^-1 r_p|, dua = |D^-1 r_d| / c, the norms likewise
  obj = (1/2 x'Ps x + qs'x) / c (whenever scaling is on);  m = 0: pri = 0
  rho estimate = clamp(rho sqrt((pri_s / (pri_nrm_s + 1e-10)) / (dua_s / (dua_nrm_s + 1e-10))), 1e-6, 1e6) from the SCALED norms
  update rule: estimate > rho tol or estimate < rho / tol -> rho = estimate, a new rho_vec and a new K
Order of events at iteration i (upstream's osqp_solve): the iteration; if i is a check iteration the termination tests; if
i is a rho iteration and the status is still undecided the estimate and perhaps the update - also at max_iter on a rho
iteration that is not a check iteration; at i = max_iter the check of the last iterate, the 10 x tests, status -2; the
closing rho_estimate uses the rho then in force.  Published: x = D x_s, y = E y_s / c.  warm_start_x: x_s = D^-1 x0,
z = As x_s; warm_start_y: y_s = c E^-1 y0.  A second solve: the iteration count from 0, the state and rho kept;
update_bounds re-derives rho_vec (and K) from the rho in force and clears the count of rho updates.

Three number types run this one code path (kind):
  "ld"  np.longdouble, K dense, every solve refined against K in long double with an fp64 LU as the preconditioner until the
        correction is below 2^-60 of the solution (or stops shrinking: cond(K) 2^-64 is its floor) - THE REFERENCE
  "mp"  mpmath at 50 digits, the same refinement to 1e-47 - pins the reference (REF_ERROR)
  "f64" np.float64 with an unpivoted LDL' by substitution in a given elimination order and no refinement, as on the device;
        tail = t sends the last t rows of that order through an explicitly inverted Schur complement - the two TWINS that
        stand for "a correct fp64 implementation" and are the only source of the tolerance

Errors are in term scales, as in polish_refs: x, y (and the scaled z) in max(1, |.|_inf), a residual in the largest magnitude sum
of its terms (|As||x| + |z|, |Ps||x| + |qs| + |As'||y|, each row unscaled the way the residual is), obj in
(1/2 |x|'|Ps||x| + |qs|'|x|) / c - but no less than 2^-53 of that sum at |x_i| = max(1, |x|_inf), see _check - rho and
rho_estimate relative.

TWIN_ERROR[scenario][quantity]: the worst error of the fp64 twins against the reference over that scenario's cases, QPs and
checkpoints (tests/test_admm_refs.py measures and pins it: measured <= constant <= 2 x measured); ITERATE_BOUND = 32 x that, the margin
of polish_refs for a device that sums the same schedules with wave-wide reductions in another order, contracts to FMAs and
eliminates in its own order."""
import contextlib

import numpy as np

import op_refs as R

DPS = 50
# The guard of the rho estimate's two denominators, as the specification of this reference states the rule.  It is a recollection
# of OSQP 0.6 and is not pinned against upstream's source (whose demo log shows rho to three digits: either guard passes).
DIV_TOL = 1e-10
INF_DIV_TOL = 1e-30                                    # OSQP_DIVISION_TOL: the smallest |delta_y|, |delta_x| an infeasibility test divides by
RHO_FIXED, RHO_MULTIPLE = 100, 4                       # the "auto" adaptive_rho_interval: 4 x check_termination (100 without checks)
DEFAULTS = dict(rho=0.1, sigma=1e-6, scaling=10, adaptive_rho=1, adaptive_rho_interval=0, adaptive_rho_tolerance=5.0,
                max_iter=4000, eps_abs=1e-3, eps_rel=1e-3, eps_prim_inf=1e-4, eps_dual_inf=1e-4, alpha=1.6,
                scaled_termination=0, check_termination=25)
KEYS = ("x", "y", "pri_res", "dua_res", "obj_val", "rho", "rho_estimate")
VARIANTS = ("stale_rho_inv", "no_sigma_x", "warm_z_zero", "dua_no_cinv")

# Worst error of the fp64 twins against the long-double reference, per scenario AND per quantity (the measured value
# beside each; tests/test_admm_refs.py measures all of them again and asserts measured <= constant <= 2 x measured).  A bound
# per quantity is never wider than one per scenario - the scenario's figure is the largest of its row - and keeps x and y sharp
# where rho_estimate is not: the estimate divides two residuals that cancel to 1e-6 .. 1e-11 of their terms, and its relative
# error is theirs (GOMP at k = 50: residuals within 3 x of the 1e-12 tolerances).  0.0: the twins match the reference exactly
# (rho without an update, y and pri_res without rows), and so must the device.  Columns of the measured values: x, y, pri_res,
# dua_res, obj_val, rho, rho_estimate.
TWIN_ERROR = {
    # measured 2.88e-15, 9.28e-15, 1.02e-15, 3.63e-16, 2.37e-16, 1.91e-11, 5.41e-10
    'box': dict(x=3.6e-15, y=1.2e-14, pri_res=1.3e-15, dua_res=4.6e-16, obj_val=3.0e-16, rho=2.4e-11, rho_estimate=6.8e-10),
    # measured 2.18e-15, 1.49e-14, 6.6e-16, 9.72e-16, 2.05e-16, 1.43e-13, 5.46e-13
    'early_rho': dict(x=2.8e-15, y=1.9e-14, pri_res=8.3e-16, dua_res=1.3e-15, obj_val=2.6e-16, rho=1.8e-13, rho_estimate=6.9e-13),
    # measured 1.22e-14, 3.73e-13, 6.22e-16, 2.25e-16, 1.82e-16, 0, 2.7e-12
    'continuation': dict(x=1.6e-14, y=4.7e-13, pri_res=7.8e-16, dua_res=2.9e-16, obj_val=2.3e-16, rho=0.0, rho_estimate=3.4e-12),
    # measured 1.12e-15, 1.19e-15, 5.52e-16, 4.34e-16, 1.61e-16, 0, 1.32e-13
    'warm': dict(x=1.5e-15, y=1.5e-15, pri_res=6.9e-16, dua_res=5.5e-16, obj_val=2.1e-16, rho=0.0, rho_estimate=1.7e-13),
    # measured 5.95e-15, 2.88e-14, 5.77e-16, 1.58e-14, 8.37e-16, 0, 4.72e-13
    'settings': dict(x=7.5e-15, y=3.7e-14, pri_res=7.3e-16, dua_res=2.0e-14, obj_val=1.1e-15, rho=0.0, rho_estimate=6.0e-13),
    # measured 1.06e-14, 6.67e-14, 5.58e-16, 4.89e-16, 7.88e-16, 0, 1.49e-10
    'gomp': dict(x=1.4e-14, y=8.4e-14, pri_res=7.0e-16, dua_res=6.2e-16, obj_val=9.9e-16, rho=0.0, rho_estimate=1.9e-10),
    # measured 7.98e-16, 9.72e-16, 5.01e-16, 2.7e-16, 4.11e-16, 0, 3.98e-11
    'edge': dict(x=1.0e-15, y=1.3e-15, pri_res=6.3e-16, dua_res=3.4e-16, obj_val=5.2e-16, rho=0.0, rho_estimate=5.0e-11),
}
ITERATE_BOUND = {sc: {k: 32 * v for k, v in row.items()} for sc, row in TWIN_ERROR.items()}
REF_ERROR = 2.8e-15        # measured 2.23e-15 (rho_estimate; rho 2.0e-17, x, y, z, the residuals and obj below 3e-19) on the small QP
# The dense tail of the tail twin, where K has more rows than that.  It counts in every scenario: the default forms carry a
# dense tail on these shapes (128 rows at a tile of 1, 64 at tiles of 2 and 4; tests/test_gpu_admm_refs.py prints it).
TAIL = 64


# ------------------------------------------------------------------ number types
def _to_mp(v):
    import mpmath as mp
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(R.LD(v) - R.LD(hi)))          # the long double, exactly


def arr(v, kind):
    """a long-double (or float) scalar / array in the number type of kind"""
    v = np.asarray(v, R.LD)
    if kind == "ld":
        return v.copy()
    if kind == "f64":
        return v.astype(np.float64)
    out = np.empty(v.shape, dtype=object)
    for idx in np.ndindex(v.shape):
        out[idx] = _to_mp(v[idx])
    return out


def context(kind):
    if kind == "mp":
        import mpmath as mp
        return mp.workdps(DPS)
    return contextlib.nullcontext()


def _ninf(v, zero):
    return np.max(np.abs(v)) if v.size else zero


def _dense(M):
    out = np.zeros(M.shape, R.LD)
    np.add.at(out, (M.rows, M.cols), M.vals)
    return out


# ------------------------------------------------------------------ the two ways to solve with K
def refined_solver(K, kind):
    """s = K^-1 r in the number type of K: an fp64 LU as preconditioner, residuals in that type"""
    import scipy.linalg as sla
    lu = sla.lu_factor(K.astype(np.float64))
    zero = arr(0, kind)[()]
    tol = arr(R.LD(2) ** -60, kind)[()] if kind == "ld" else arr(R.LD(10) ** -47, kind)[()]

    def solve(r):
        s, res, last = r * zero, r, None
        for _ in range(60):
            rn = _ninf(res, zero)
            if rn == 0:
                return s
            d = arr(sla.lu_solve(lu, (res / rn).astype(np.float64)), kind) * rn
            dn = _ninf(d, zero)
            if kind == "ld" and last is not None and dn >= last / 2:      # (the floor of a long-double residual: cond(K) 2^-64)
                return s
            s = s + d
            if dn <= tol * _ninf(s, zero):
                return s
            res, last = r - K @ s, dn
        raise AssertionError("the refinement did not converge")
    return solve


def ldl_solver(K, perm, tail=0):
    """fp64: unpivoted LDL' of K[perm][:, perm] by substitution, no refinement.  tail = t: only the first N - t rows are
    eliminated; the Schur complement S of the last t is formed from that factor, inverted explicitly and applied as a matrix."""
    import scipy.linalg as sla
    N = K.shape[0]
    perm = np.arange(N) if perm is None else np.asarray(perm)
    Kp = K[np.ix_(perm, perm)]
    h = N - min(int(tail), N)
    L, d = np.eye(N), np.zeros(N)
    for j in range(h):
        v = L[j, :j] * d[:j]
        d[j] = Kp[j, j] - L[j, :j] @ v
        L[j + 1:, j] = (Kp[j + 1:, j] - L[j + 1:, :j] @ v) / d[j]
    L11, L21 = L[:h, :h], L[h:, :h]
    Sinv = None
    if h < N:
        Sinv = np.linalg.inv(Kp[h:, h:] - (L21 * d[:h]) @ L21.T)
        Sinv = 0.5 * (Sinv + Sinv.T)

    def solve(r):
        b = r[perm]
        y1 = sla.solve_triangular(L11, b[:h], lower=True, unit_diagonal=True) if h else b[:0]
        x2 = Sinv @ (b[h:] - L21 @ y1) if h < N else b[:0]
        t = y1 / d[:h] - (L21.T @ x2 if h < N else 0.0)
        x1 = sla.solve_triangular(L11.T, t, lower=False, unit_diagonal=True) if h else t
        out = np.empty(N)
        out[perm] = np.concatenate([x1, x2])
        return out
    solve.factor = (perm, h, L, d)                          # (factor_refs builds its third twin on this leading factor)
    return solve


# ------------------------------------------------------------------ the ADMM
class Admm:
    """One QP's ADMM in one number type (module docstring).  variant (tests): one deliberate defect of VARIANTS."""

    def __init__(self, P, q, A, l, u, D, E, c, kind="ld", perm=None, tail=0, variant=None, **settings):
        import scipy.sparse as sp
        assert R.WIDE, "the reference needs an 80-bit long double"
        assert variant is None or variant in VARIANTS
        unknown = set(settings) - set(DEFAULTS)
        assert not unknown, unknown
        self.st = st = dict(DEFAULTS, **settings)
        if st["adaptive_rho"] and not st["adaptive_rho_interval"]:
            st["adaptive_rho_interval"] = RHO_MULTIPLE * st["check_termination"] if st["check_termination"] else RHO_FIXED
        self.kind, self.perm, self.tail, self.variant = kind, perm, tail, variant
        self.P, self.A = P, sp.csc_matrix(A)
        self.m, self.n = self.A.shape
        self.q = np.zeros(self.n) if q is None else np.asarray(q, np.float64)
        self.Dl, self.El, self.cl = np.asarray(D, R.LD), np.asarray(E, R.LD), R.LD(c)
        with context(kind):
            self.zero, self.one = self.num(0)[()], self.num(1)[()]
            self.D, self.E, self.c = self.num(self.Dl), self.num(self.El), self.num(self.cl)[()]
            self.sigma, self.alpha = self.num(st["sigma"])[()], self.num(st["alpha"])[()]
            self.rho = self.num(min(max(st["rho"], R.OQ_RHO_MIN), R.OQ_RHO_MAX))[()]
            self._data(l, u)
            self.x, self.z, self.y = self.num(np.zeros(self.n)), self.num(np.zeros(self.m)), self.num(np.zeros(self.m))
            self.dx, self.dy = self.x, self.y
            self._refactor()
        self.rho_updates, self.rho_est = 0, self.rho
        self.stale = 0

    def num(self, v):
        return arr(v, self.kind)

    def _data(self, l, u):
        Ps, As, qs, ls, us = R.scaled_qp(self.P, self.A, self.q, l, u, self.Dl, self.El, self.cl)
        self.Ps, self.As, self.qs = self.num(_dense(Ps)), self.num(_dense(As)), self.num(qs)
        self.ls, self.us = self.num(ls), self.num(us)
        self.rows = R.rho_vec(ls, us, 1.0)                   # the class of every row: RHO_MIN free, 1e3 equality, 1 inequality
        self.lfin = np.asarray(ls, np.float64) > -R.OQ_INFTY * R.OQ_MIN_SCALING
        self.ufin = np.asarray(us, np.float64) < R.OQ_INFTY * R.OQ_MIN_SCALING

    def _refactor(self):
        n, m = self.n, self.m
        free, eq = self.rows == R.OQ_RHO_MIN, self.rows == R.OQ_RHO_EQ_OVER_INEQ
        self.rv = np.where(free, self.num(R.OQ_RHO_MIN)[()], np.where(eq, self.num(R.OQ_RHO_EQ_OVER_INEQ)[()] * self.rho, self.rho))
        self.rv = self.rv.astype(self.x.dtype) if self.kind != "mp" else self.rv.astype(object)
        self.ri = (self.rv * 0 + self.one) / self.rv if m else self.rv
        self.ri_step = self.ri
        K = np.empty((n + m, n + m), dtype=self.Ps.dtype)
        K[:n, :n] = self.Ps + np.eye(n, dtype=int) * self.sigma
        K[:n, n:], K[n:, :n] = self.As.T, self.As
        K[n:, n:] = np.diag(-self.ri) if m else self.As[:, :0]
        if self.kind != "f64":
            K = K + self.zero                                  # (object arrays: every entry an mpf)
        self.K = K
        self.solver = ldl_solver(K, self.perm, self.tail) if self.kind == "f64" else refined_solver(K, self.kind)

    # ---- the entry points a test drives
    def warm_start_x(self, x0):
        with context(self.kind):
            self.x = self.num(np.asarray(x0, np.float64)) / self.D
            self.z = self.As @ self.x if self.variant != "warm_z_zero" else self.z * self.zero

    def warm_start_y(self, y0):
        with context(self.kind):
            self.y = self.num(np.asarray(y0, np.float64)) * self.c / self.E

    def update_bounds(self, l, u):
        with context(self.kind):
            self._data(l, u)
            self._refactor()
        self.rho_updates = 0

    def _iterate(self):
        n, a, ri = self.n, self.alpha, self.ri_step
        x, z, y = self.x, self.z, self.y
        top = x * self.sigma - self.qs if self.variant != "no_sigma_x" else -self.qs
        sol = self.solver(np.concatenate([top, z - ri * y]))
        xt, nu = sol[:n], sol[n:]
        zt = z - ri * y + ri * nu
        xn = xt * a + x * (self.one - a)
        zr = zt * a + z * (self.one - a)
        zn = np.minimum(np.maximum(zr + ri * y, self.ls), self.us)
        self.dy = self.rv * (zr - zn)
        self.dx = xn - x
        self.x, self.z, self.y = xn, zn, y + self.dy

    def _check(self):
        """everything E11-E13 derive from the iterate, in the number type"""
        st, zero, one = self.st, self.zero, self.one
        x, z, y = self.x, self.z, self.y
        Px, Aty, Ax = self.Ps @ x, self.As.T @ y, self.As @ x
        rd, rp = self.qs + Px + Aty, Ax - z
        unscale = bool(st["scaling"]) and not st["scaled_termination"]
        cinv = one / self.c if st["scaling"] else one
        wd = (self.D * 0 + cinv) / self.D if unscale else self.D * 0 + one
        wp = (self.E * 0 + one) / self.E if unscale else self.E * 0 + one
        if unscale and self.variant == "dua_no_cinv":
            wd = (self.D * 0 + one) / self.D
        nrm = lambda v, w: _ninf(v * w, zero)
        k = dict(pri_s=_ninf(rp, zero), dua_s=_ninf(rd, zero), pn_s=max(_ninf(z, zero), _ninf(Ax, zero)),
                 dn_s=max(_ninf(self.qs, zero), _ninf(Aty, zero), _ninf(Px, zero)),
                 pri=nrm(rp, wp) if self.m else zero, dua=nrm(rd, wd), pn=max(nrm(z, wp), nrm(Ax, wp)),
                 dn=max(nrm(self.qs, wd), nrm(Aty, wd), nrm(Px, wd)),
                 obj=cinv * (x @ Px / 2 + self.qs @ x))
        ax, ay = np.abs(x), np.abs(y)
        aP, aA = np.abs(self.Ps), np.abs(self.As)
        # (obj: an x at round-off level - the GOMP velocities after one iteration from a warm start without any are 0 exactly -
        #  gives an obj of round-off squared; its scale does not fall below one fp64 round-off of obj's scale at |x_i| = max(1, |x|_inf))
        unit = ax * 0 + max(one, _ninf(x, zero))
        floor = cinv * (unit @ (aP @ unit) / 2 + np.abs(self.qs) @ unit) * self.num(R.U)[()]
        dq = (self.D * 0 + max(one, _ninf(self.D * x, zero))) / self.D      # one unit of x's error measure in every entry, scaled space
        k["scale"] = dict(pri_res=nrm(aA @ ax + np.abs(z), wp), dua_res=nrm(aP @ ax + np.abs(self.qs) + aA.T @ ay, wd),
                          obj_val=max(cinv * (ax @ (aP @ ax) / 2 + np.abs(self.qs) @ ax), floor),
                          obj_quad=cinv * dq @ (aP @ dq) / 2)
        return k

    def _estimate(self, k):
        pr, du = k["pri_s"] / (k["pn_s"] + self.num(DIV_TOL)[()]), k["dua_s"] / (k["dn_s"] + self.num(DIV_TOL)[()])
        if self.kind == "mp":
            import mpmath as mp
            e = self.rho * mp.sqrt(pr / du)
        else:
            e = self.rho * np.sqrt(pr / du)
        return min(max(e, self.num(R.OQ_RHO_MIN)[()]), self.num(R.OQ_RHO_MAX)[()])

    def _missed(self, k, f):
        """the factor by which every termination test at f x the tolerances is missed (>= 1: not met), in float"""
        st, fl = self.st, float
        eps_abs, eps_rel, eps_p, eps_d = f * st["eps_abs"], f * st["eps_rel"], f * st["eps_prim_inf"], f * st["eps_dual_inf"]
        opt = fl(k["dua"]) / (eps_abs + eps_rel * fl(k["dn"]))
        if self.m:
            opt = max(opt, fl(k["pri"]) / (eps_abs + eps_rel * fl(k["pn"])))
        unscale = bool(st["scaling"]) and not st["scaled_termination"]
        D, E, c = self.D.astype(np.float64), self.E.astype(np.float64), fl(self.c)
        f64 = lambda v: np.asarray(v.astype(np.float64))
        As, Ps, ls, us = f64(self.As), f64(self.Ps), f64(self.ls), f64(self.us)
        dy, dx = f64(self.dy).copy(), f64(self.dx)
        dy = np.where(~self.ufin, np.where(~self.lfin, 0.0, np.minimum(dy, 0.0)), np.where(~self.lfin, np.maximum(dy, 0.0), dy))
        inf = float("inf")
        pinf = dinf = inf
        ndy = np.max(np.abs(E * dy if unscale else dy), initial=0.0)
        if ndy > INF_DIV_TOL:
            lhs = np.sum(us * np.maximum(dy, 0.0) + ls * np.minimum(dy, 0.0))
            atdy = np.max(np.abs((As.T @ dy) / (D if unscale else 1.0)), initial=0.0)
            pinf = max(inf if lhs >= 0 else eps_p * ndy / -lhs, atdy / (eps_p * ndy))
        ndx = np.max(np.abs(D * dx if unscale else dx), initial=0.0)
        cs = c if unscale else 1.0
        if ndx > INF_DIV_TOL:
            qdx = f64(self.qs) @ dx
            pdx = np.max(np.abs((Ps @ dx) / (D if unscale else 1.0)), initial=0.0)
            adx = (As @ dx) / (E if unscale else 1.0)
            out = max(np.max(np.where(self.ufin, adx, -inf), initial=-inf), np.max(np.where(self.lfin, -adx, -inf), initial=-inf))
            dinf = max(inf if qdx >= 0 else cs * eps_d * ndx / -qdx, pdx / (cs * eps_d * ndx), out / (eps_d * ndx))
        return min(opt, pinf, dinf)

    def _publish(self, k, it, margin):
        one = self.one
        x = self.D * self.x
        y = self.E * self.y / self.c if self.st["scaling"] else self.y * one
        return dict(iter=it, x=x, y=y, z=self.z, pri_res=k["pri"], dua_res=k["dua"], obj_val=k["obj"], rho=self.rho,
                    rho_estimate=self._estimate(k), rho_updates=self.rho_updates, term_margin=margin, rho_margin=self.rho_margin,
                    rho_events=list(self.rho_events),
                    scale=dict(k["scale"], x=max(one, _ninf(x, self.zero)), y=max(one, _ninf(y, self.zero)),
                               z=max(one, _ninf(self.z, self.zero))))

    def solve(self, max_iter=None, checkpoints=None):
        """max_iter iterations from the state in force; {k: what a solve with max_iter = k publishes} for every checkpoint
        (default: max_iter alone).  term_margin: the smallest factor by which a termination test was missed at a check up to
        k or in the closing of k (exact and 10 x); rho_margin: the smallest relative distance of a rho decision from its
        threshold so far; rho_events: [(iteration, estimate, updated)]."""
        st = self.st
        last = int(st["max_iter"] if max_iter is None else max_iter)
        checkpoints = (last,) if checkpoints is None else tuple(checkpoints)
        assert max(checkpoints) <= last
        ct, ri = st["check_termination"], st["adaptive_rho_interval"] if st["adaptive_rho"] else 0
        tol = self.num(st["adaptive_rho_tolerance"])[()]
        out, running = {}, float("inf")
        self.rho_margin, self.rho_events = float("inf"), []
        with context(self.kind):
            for it in range(1, last + 1):
                self._iterate()
                if self.stale:
                    self.stale -= 1
                    if not self.stale:
                        self.ri_step = self.ri
                is_check, is_rho = bool(ct) and it % ct == 0, bool(ri) and it % ri == 0
                if not (is_check or is_rho or it in checkpoints):
                    continue
                k = self._check()
                here = self._missed(k, 1.0) if (is_check or it in checkpoints) else float("inf")
                if is_check:
                    running = min(running, here)
                if is_rho:
                    rn = self._estimate(k)
                    self.rho_est = rn
                    lo, hi = self.rho / tol, self.rho * tol
                    self.rho_margin = min(self.rho_margin, float(abs(rn - lo) / lo), float(abs(rn - hi) / hi))
                    update = bool(rn > hi or rn < lo)
                    self.rho_events.append((it, float(rn), update))
                    if update:
                        old = self.ri
                        self.rho = rn
                        self.rho_updates += 1
                        self._refactor()
                        if self.variant == "stale_rho_inv":
                            self.ri_step, self.stale = old, (ct or ri)
                if it in checkpoints:
                    out[it] = self._publish(k, it, min(running, here, self._missed(k, 10.0)))
        return out


# ------------------------------------------------------------------ the error measure
def _in(kind, v):
    """a float, long double or mpf (array) in the number type of a reference"""
    if kind == "mp":
        import mpmath as mp
        conv = lambda t: t if isinstance(t, mp.mpf) else _to_mp(t)
        if np.ndim(v) == 0:
            return conv(v[()] if isinstance(v, np.ndarray) else v)
        return np.array([conv(t) for t in v] + [None], dtype=object)[:-1]
    return np.asarray(v, R.LD)


def errors(got, ref, kind="ld", keys=KEYS, x_bound=0.0):
    """{key: |got - ref| / term scale} for a result got (floats: the device, the oracle, a twin; or a long-double reference
    against its mpmath twin with kind = "mp").  x_bound: the bound x itself is held to.  obj is a function of x, and its term
    scale covers what is linear in an error of x; an x that lies d = x_bound max(1, |x|_inf) off in every entry also moves obj
    by up to 1/2 d'|P|d, which no factor on the twins' error covers where the linear terms vanish (the velocities of the GOMP
    pattern after one iteration are 0 exactly, q is 0: obj is the square of the round-off in x).  That much is taken off the
    difference first: 1e-24 of obj's scale on the box QPs."""
    out = {}
    with context(kind):
        for key in keys:
            g, r = _in(kind, got[key]), ref[key]
            if key in ("x", "y", "z"):
                assert np.shape(g) == np.shape(r), key
                diff = max([abs(a - b) for a, b in zip(g, r)], default=0)
                out[key] = float(diff / ref["scale"][key])
            elif key in ("rho", "rho_estimate"):
                out[key] = float(abs(g - r) / abs(r))
            else:
                diff = abs(g - r)
                if key == "obj_val" and x_bound:
                    diff = max(diff - ref["scale"]["obj_quad"] * x_bound * x_bound, diff * 0)
                out[key] = 0.0 if diff == 0 else float(diff / ref["scale"][key])
            assert np.isfinite(out[key]), (key, got[key])
    return out


# ------------------------------------------------------------------ the cases of the tests
BOX_SHAPE = dict(n=96, mg=64, nnz_per_row=6)
BOX_B = 6
EPS = dict(eps_abs=1e-12, eps_rel=1e-12)
RHO_EACH = (0.01, 1.0, 10.0, 0.1, 0.1, 100.0)
EQ_ROW = 100                                               # the inequality row (a row of G) that update_bounds turns into l = u
EQ_VALUE = 0.05
# gomp_batch's default seed 2000 would bring in a QP that is within 34 x of the 1e-12 tolerances after 50 iterations: its consecutive
# iterates lie 714 bounds apart there and its rho_estimate is noise (twin error 1.1e-5).  Seeds 2001 .. 2004 keep all four QPs.
GOMP_SEED = 2001


class Case:
    """One run of a batch: settings (without max_iter), the calls before the first solve (warm_x / warm_y: [B, n] / [B, m],
    rho_each: [B]), the checkpoints ks of that solve - one fresh handle each - and, for a continuation, a second solve of
    k2 iterations on the handle of ks[0], after update_bounds(*bounds) if given."""

    def __init__(self, name, scenario, pr, settings, ks, warm_x=None, warm_y=None, rho_each=None, k2=None, bounds=None):
        self.name, self.scenario, self.pr, self.settings, self.ks = name, scenario, pr, dict(settings), tuple(ks)
        self.warm_x, self.warm_y, self.rho_each, self.k2, self.bounds = warm_x, warm_y, rho_each, k2, bounds
        self.B = pr["Ax"].shape[0]
        assert k2 is None or len(self.ks) == 1

    def qp(self, b):
        from osqp_solver_amd import problems as PR
        P, A = PR.qp_matrices(self.pr, b)
        return dict(P=P, A=A, q=None if self.pr["q"] is None else self.pr["q"][b], l=self.pr["l"][b], u=self.pr["u"][b])

    def settings_of(self, b):
        return dict(self.settings, rho=self.rho_each[b]) if self.rho_each is not None else dict(self.settings)

    def run(self, b, D, E, c, kind="ld", perm=None, tail=0, variant=None, ks=None, warm_y=True):
        """{(solve index, k): published result} of QP b in the number type of kind"""
        d = self.qp(b)
        a = Admm(d["P"], d["q"], d["A"], d["l"], d["u"], D, E, c, kind=kind, perm=perm, tail=tail, variant=variant, **self.settings_of(b))
        if self.warm_x is not None:
            a.warm_start_x(self.warm_x[b])
        if self.warm_y is not None and warm_y:
            a.warm_start_y(self.warm_y[b])
        ks = self.ks if ks is None else tuple(ks)
        out = {(0, k): v for k, v in a.solve(max(ks), ks).items()}
        if self.k2 is not None:
            if self.bounds is not None:
                a.update_bounds(self.bounds[0][b], self.bounds[1][b])
            out[(1, self.k2)] = a.solve(self.k2)[self.k2]
        return out


def take(pr, B):
    out = dict(pr)
    for k in ("Px", "Ax", "q", "l", "u", "warm"):
        if out.get(k) is not None:
            out[k] = out[k][:B]
    return out


def n1_m2(B=5, seed=0):
    """n = 1, m = 2 in the layout of test_gpu_ops.tiny_qp with q three times as large: the optimum lies on a bound, and no
    QP is within 1e7 of a termination test after 25 iterations (half of tiny_qp's own QPs are optimal to 1e-12 by then)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    return dict(n=1, m=2, P=sp.csc_matrix(np.eye(1)), A=sp.csc_matrix(np.ones((2, 1))), Px=rng.uniform(1, 2, (B, 1)),
                Ax=rng.uniform(0.5, 1.5, (B, 2)), q=3.0 * rng.standard_normal((B, 1)), l=-np.ones((B, 2)), u=np.ones((B, 2)))


_CASES = {}


def cases():
    """{name: Case}: every run the GPU tests make (built once)"""
    if _CASES:
        return _CASES
    from osqp_solver_amd import problems as PR
    from test_gpu_ops import edge_qp, tiny_qp
    box = PR.random_box_qp(BOX_B, **BOX_SHAPE)
    n, m = box["n"], box["m"]
    rng = np.random.default_rng(77)
    wx, wy = 0.5 * rng.standard_normal((BOX_B, n)), 0.5 * rng.standard_normal((BOX_B, m))
    l2, u2 = box["l"].copy(), box["u"].copy()
    l2[:, EQ_ROW] = u2[:, EQ_ROW] = EQ_VALUE
    gomp = PR.gomp_batch(4, 3, 12, seed=GOMP_SEED)
    edge = edge_qp()                                       # variable 2 has no entry in P and none in A: q_2 = 0 keeps the QP bounded
    edge["q"][:, 2] = 0.0
    add = lambda *a, **kw: _CASES.__setitem__(a[0], Case(*a, **kw))
    add("box", "box", box, EPS, (1, 2, 25, 26, 30, 125))
    add("box_B3", "box", take(box, 3), EPS, (1, 25))
    add("box_B5", "box", take(box, 5), EPS, (1, 25))
    add("box_B3_s0", "box", take(box, 3), dict(EPS, scaling=0), (1, 25))
    add("box_B5_s0", "box", take(box, 5), dict(EPS, scaling=0), (1, 25))
    add("early_rho", "early_rho", box, dict(EPS, check_termination=5, adaptive_rho_interval=10), (35,))
    add("cont", "continuation", box, EPS, (30,), k2=30)
    add("cont_bounds", "continuation", box, EPS, (30,), k2=30, bounds=(l2, u2))
    add("warm_s10", "warm", box, EPS, (1, 25), warm_x=wx, warm_y=wy)
    add("warm_s0", "warm", box, dict(EPS, scaling=0), (1, 25), warm_x=wx, warm_y=wy)
    for name, kw in (("scaling0", dict(scaling=0)), ("scaled_termination", dict(scaled_termination=1)), ("alpha1", dict(alpha=1.0)),
                     ("alpha1.8", dict(alpha=1.8)), ("sigma1e-3", dict(sigma=1e-3))):
        add("set_" + name, "settings", box, dict(EPS, **kw), (30,))
    add("set_rho_each", "settings", box, EPS, (30,), rho_each=RHO_EACH)
    add("gomp", "gomp", gomp, EPS, (1, 25, 50), warm_x=gomp["warm"])
    for s in (0, 10):
        add(f"edge_n1_m2_s{s}", "edge", n1_m2(), dict(EPS, scaling=s), (1, 25))
        add(f"edge_n4_m0_s{s}", "edge", tiny_qp(5, 4, 0), dict(EPS, scaling=s), (1, 25))
        add(f"edge_empty_s{s}", "edge", edge, dict(EPS, scaling=s), (1, 25))
    return _CASES


_REF = {}


def reference(case, b, D, E, c):
    """the long-double results of QP b of a case with the scaling (D, E, c), computed once per scaling"""
    key = (case.name, b, case.pr["l"][b].tobytes(), case.pr["u"][b].tobytes(), np.asarray(D).tobytes(), np.asarray(E).tobytes(), float(c))
    if key not in _REF:
        _REF[key] = case.run(b, D, E, c)
    return _REF[key]


def judge(got, ref, scenario):
    """(worst error / bound over the quantities, its key) of a result against a reference of that scenario"""
    return ratio(errors(got, ref, x_bound=ITERATE_BOUND[scenario]["x"]), scenario)


def ratio(errs, scenario):
    """(worst error / bound over the quantities, its key); a bound of 0.0 admits no error at all"""
    out, where = 0.0, None
    for k, e in errs.items():
        bound = ITERATE_BOUND[scenario][k]
        r = (0.0 if e == 0.0 else float("inf")) if bound == 0.0 else e / bound
        if r >= out:
            out, where = r, k
    return out, where


def oracle_of(case, b, **kw):
    """the CPU oracle of QP b with the case's settings: the source of a scaling and of a sparse elimination order without a GPU"""
    from oracle import oracle as O
    d = case.qp(b)
    return O.OracleQPSolver(d["P"], d["q"], d["A"], d["l"], d["u"], **dict(case.settings_of(b), **kw))


def measure_twins(scenario):
    """{quantity: worst error of the two fp64 twins against the reference} over the scenario's cases, QPs and checkpoints,
    with the oracle's scaling and the oracle's elimination order"""
    out = {k: 0.0 for k in KEYS}
    for case in cases().values():
        if case.scenario != scenario:
            continue
        for b in range(case.B):
            o = oracle_of(case, b)
            D, E, c = o.scaling()
            perm = o.factor()[0]
            ref = reference(case, b, D, E, c)
            tails = (0, TAIL) if len(perm) > TAIL else (0,)
            for t in tails:
                twin = case.run(b, D, E, c, kind="f64", perm=perm, tail=t)
                for key, r in ref.items():
                    assert twin[key]["rho_updates"] == r["rho_updates"], (case.name, b, key)
                    for k, e in errors(twin[key], r).items():
                        out[k] = max(out[k], e)
    return out
