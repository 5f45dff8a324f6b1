"""References for the equilibration (kernels.hip ruiz_kernel / ruiz_reg_kernel<4|8|16|32>, host_core.cpp
scale_qp / unscale_qp), written from the comment above ruiz_kernel and from test_op_references._scale_data_restated (a helper
module of the tests, not a conftest).  No solver code is involved.

OSQP 0.6 scale_data on the stored patterns of triu(P) and A.  D = 1, E = 1, c = 1; then `iters` times:
  dn_j = max(column j of the symmetric P, column j of A) in absolute value, en_i = the same of row i of A
  dn = 1 / sqrt(limit(dn)), en = 1 / sqrt(limit(en)),  limit(v) = 1 if v < 1e-4, 1e4 if v > 1e4, else v
  P_ij *= dn_i, then *= dn_j;  A_ij *= en_i, then *= dn_j;  q *= dn;  D *= dn;  E *= en
  ct = 1 / limit(max(mean column norm of the new P, limit(|q|_inf)));  P *= ct;  q *= ct;  c *= ct
The mean is added up in index order and divided by n.  An update unscales what it keeps with the scaling in force
(P_ij *= 1/c, *= 1/D_i, *= 1/D_j; q_j *= (1/c) (1/D_j); A_ij *= 1/E_i, *= 1/D_j), replaces the rest by the new raw values and
equilibrates again from D = E = c = 1.  The `fresh` form (reinit_some) starts from the raw P of setup - or of the last P
update - and the raw q in force instead of unscaling.  update_q stores c (D q) and leaves D, E, c alone.

One code path (class Ruiz) in three number types (kind):
  "ld"  np.longdouble - THE REFERENCE
  "mp"  mpmath at 50 digits - pins the reference (REF_ERROR) on a small case that includes the limits
  "f64" np.float64, the operations above in the stated order - the first TWIN; the second is the CPU oracle
        (oracle/osqp_oracle.c scale_data / unscale_data) through the calls it has: setup at any iteration count and the A
        update, with a fresh setup on the raw data in force wherever the path changes P or q (it has no such call; the
        unscaling it then skips is exact to 1e-19 in the reference, so it stands for a correct fp64 implementation as well).
Errors are relative, per entry of D, per entry of E, and of c, each apart.  RUIZ_TWIN_ERROR[case][quantity] is the worst error
of the two twins over the case's QPs (tests/test_ruiz_refs.py measures and pins it with one BLAS thread: measured <= constant
<= 2 x measured); RUIZ_BOUND = 32 x that, the margin of admm_refs and factor_refs.  REF_ERROR: the reference against mpmath.

limit() is discontinuous at 1e-4 and 1e4.  Every value a run passes to it is recorded (column norms, row norms, |q|_inf and
the max that decides c, of every iteration); a case is NEAR when such a value lies within a relative 1e-9 of a threshold
without being bit for bit that threshold in the reference and in the fp64 twin alike.  The limit cases put 1e-4 and 1e4 there
as data of the first iteration, where a norm is an exact maximum.  No case of cases() may be near (tests/test_ruiz_refs.py)."""
import contextlib

import numpy as np

LD = np.longdouble
DPS = 50
MIN_SCALING, MAX_SCALING = 1e-4, 1e4
NEAR = 1e-9
QUANTITIES = ("D", "E", "c")
MUTATIONS = ("le_at_min", "no_q_limit", "mean_nonempty", "no_lower_triangle", "c_not_reset", "unscale_skips_a_product")
REF_ERROR = 1.2e-18        # measured 9.58e-19 (D 9.58e-19, E 7.27e-19, c 5.6e-19): the reference against mpmath, n = 12, m = 20, limits included
# Worst relative error of the two fp64 twins against the long-double reference, per case and quantity (D, E, c; the measured
# values beside each).  0.0: the twins match the reference exactly, and so must the device.
RUIZ_TWIN_ERROR = {
    # measured 4.25e-16, 7.28e-16, 6.29e-16
    'form_reg4': dict(D=5.4e-16, E=9.2e-16, c=7.9e-16),
    # measured 5.59e-16, 8.45e-16, 1.93e-16
    'form_reg8': dict(D=7e-16, E=1.06e-15, c=2.5e-16),
    # measured 5.59e-16, 8.45e-16, 1.87e-16
    'form_reg8_full': dict(D=7e-16, E=1.06e-15, c=2.4e-16),
    # measured 5.59e-16, 8.45e-16, 1.93e-16
    'form_reg16_by_one': dict(D=7e-16, E=1.06e-15, c=2.5e-16),
    # measured 4.76e-16, 7.74e-16, 1.7e-16
    'form_reg16': dict(D=6e-16, E=9.7e-16, c=2.2e-16),
    # measured 6.76e-16, 7.47e-16, 1.8e-16
    'form_reg32': dict(D=8.5e-16, E=9.4e-16, c=2.3e-16),
    # measured 5.5e-16, 7.81e-16, 4.09e-16
    'form_reg32_full': dict(D=6.9e-16, E=9.8e-16, c=5.2e-16),
    # measured 5.5e-16, 7.81e-16, 4.09e-16
    'form_global_by_one': dict(D=6.9e-16, E=9.8e-16, c=5.2e-16),
    # measured 6.96e-16, 8.4e-16, 1.91e-16
    'form_global': dict(D=8.8e-16, E=1.06e-15, c=2.4e-16),
    # measured 6.58e-16, 9.67e-16, 4.55e-16
    'limits_global': dict(D=8.3e-16, E=1.21e-15, c=5.7e-16),
    # measured 1.46e-16, 2.66e-16, 2.22e-16
    'tiny_n1_m2': dict(D=1.9e-16, E=3.4e-16, c=2.8e-16),
    # measured 3.54e-16, 0, 8.45e-16
    'tiny_n4_m0': dict(D=4.5e-16, E=0.0, c=1.06e-15),
    # measured 1.49e-16, 1.61e-16, 2.56e-16
    'iters1_benign': dict(D=1.9e-16, E=2.1e-16, c=3.2e-16),
    # measured 1.53e-16, 1.61e-16, 1.21e-16
    'iters1_limits': dict(D=2e-16, E=2.1e-16, c=1.6e-16),
    # measured 3.64e-16, 3.34e-16, 3.58e-16
    'iters3_benign': dict(D=4.6e-16, E=4.2e-16, c=4.5e-16),
    # measured 3.54e-16, 3.34e-16, 3e-16
    'iters3_limits': dict(D=4.5e-16, E=4.2e-16, c=3.8e-16),
    # measured 4.25e-16, 7.28e-16, 6.29e-16
    'iters10_benign': dict(D=5.4e-16, E=9.2e-16, c=7.9e-16),
    # measured 5.01e-16, 7.62e-16, 2.87e-16
    'iters10_limits': dict(D=6.3e-16, E=9.6e-16, c=3.6e-16),
    # measured 6.55e-16, 1.17e-15, 1.89e-16
    'iters25_benign': dict(D=8.2e-16, E=1.5e-15, c=2.4e-16),
    # measured 8.47e-16, 9.16e-16, 5.45e-16
    'iters25_limits': dict(D=1.06e-15, E=1.15e-15, c=6.9e-16),
    # measured 4.72e-16, 6.41e-16, 3.97e-16
    'update_A_benign': dict(D=5.9e-16, E=8.1e-16, c=5e-16),
    # measured 4.72e-16, 6.41e-16, 3.97e-16
    'update_A_bounds_benign': dict(D=5.9e-16, E=8.1e-16, c=5e-16),
    # measured 6.77e-16, 1.06e-15, 3.85e-16
    'update_P_benign': dict(D=8.5e-16, E=1.4e-15, c=4.9e-16),
    # measured 4.84e-16, 6.41e-16, 2.98e-16
    'update_P_A_benign': dict(D=6.1e-16, E=8.1e-16, c=3.8e-16),
    # measured 4.72e-16, 6.41e-16, 3.97e-16
    'update_A_bounds_device_benign': dict(D=5.9e-16, E=8.1e-16, c=5e-16),
    # measured 6.77e-16, 1.06e-15, 3.85e-16
    'update_P_device_benign': dict(D=8.5e-16, E=1.4e-15, c=4.9e-16),
    # measured 4.84e-16, 6.41e-16, 2.98e-16
    'update_P_A_bounds_device_benign': dict(D=6.1e-16, E=8.1e-16, c=3.8e-16),
    # measured 4.04e-16, 7.28e-16, 6.29e-16
    'update_A_bounds_some_benign': dict(D=5.1e-16, E=9.2e-16, c=7.9e-16),
    # measured 6.77e-16, 1.06e-15, 6.29e-16
    'update_P_some_benign': dict(D=8.5e-16, E=1.4e-15, c=7.9e-16),
    # measured 3.61e-16, 7.28e-16, 6.29e-16
    'update_P_A_bounds_some_benign': dict(D=4.6e-16, E=9.2e-16, c=7.9e-16),
    # measured 4.07e-16, 7.28e-16, 6.29e-16
    'reinit_some_benign': dict(D=5.1e-16, E=9.2e-16, c=7.9e-16),
    # measured 8.21e-16, 9.13e-16, 2.97e-16
    'update_A_then_update_P_benign': dict(D=1.03e-15, E=1.15e-15, c=3.8e-16),
    # measured 4.58e-16, 8.3e-16, 3.72e-16
    'update_P_A_then_update_A_bounds_benign': dict(D=5.8e-16, E=1.04e-15, c=4.7e-16),
    # measured 3.82e-16, 7.28e-16, 6.29e-16
    'update_P_some_then_reinit_some_benign': dict(D=4.8e-16, E=9.2e-16, c=7.9e-16),
    # measured 3.55e-16, 7.28e-16, 6.29e-16
    'update_q_then_reinit_some_benign': dict(D=4.5e-16, E=9.2e-16, c=7.9e-16),
    # measured 4.49e-16, 9.84e-16, 3.85e-16
    'update_P_then_reinit_some_benign': dict(D=5.7e-16, E=1.23e-15, c=4.9e-16),
    # measured 7.29e-16, 6.52e-16, 3.77e-16
    'update_A_limits': dict(D=9.2e-16, E=8.2e-16, c=4.8e-16),
    # measured 7.29e-16, 6.52e-16, 3.77e-16
    'update_A_bounds_limits': dict(D=9.2e-16, E=8.2e-16, c=4.8e-16),
    # measured 6.77e-16, 1.17e-15, 3.23e-16
    'update_P_limits': dict(D=8.5e-16, E=1.5e-15, c=4.1e-16),
    # measured 6.16e-16, 7.73e-16, 5.69e-16
    'update_P_A_limits': dict(D=7.8e-16, E=9.7e-16, c=7.2e-16),
    # measured 7.29e-16, 6.52e-16, 3.77e-16
    'update_A_bounds_device_limits': dict(D=9.2e-16, E=8.2e-16, c=4.8e-16),
    # measured 6.77e-16, 1.17e-15, 3.23e-16
    'update_P_device_limits': dict(D=8.5e-16, E=1.5e-15, c=4.1e-16),
    # measured 6.16e-16, 7.73e-16, 5.69e-16
    'update_P_A_bounds_device_limits': dict(D=7.8e-16, E=9.7e-16, c=7.2e-16),
    # measured 7.29e-16, 7.28e-16, 3.77e-16
    'update_A_bounds_some_limits': dict(D=9.2e-16, E=9.2e-16, c=4.8e-16),
    # measured 6.77e-16, 1.17e-15, 3.23e-16
    'update_P_some_limits': dict(D=8.5e-16, E=1.5e-15, c=4.1e-16),
    # measured 4.49e-16, 7.73e-16, 5.69e-16
    'update_P_A_bounds_some_limits': dict(D=5.7e-16, E=9.7e-16, c=7.2e-16),
    # measured 5.84e-16, 7.28e-16, 3.2e-17
    'reinit_some_limits': dict(D=7.3e-16, E=9.2e-16, c=4.1e-17),
    # measured 9.13e-16, 1.06e-15, 2.97e-16
    'update_A_then_update_P_limits': dict(D=1.15e-15, E=1.4e-15, c=3.8e-16),
    # measured 5.73e-16, 7.47e-16, 8.13e-16
    'update_P_A_then_update_A_bounds_limits': dict(D=7.2e-16, E=9.4e-16, c=1.02e-15),
    # measured 4.23e-16, 7.28e-16, 1.9e-16
    'update_P_some_then_reinit_some_limits': dict(D=5.3e-16, E=9.2e-16, c=2.4e-16),
    # measured 4.37e-16, 7.28e-16, 5.47e-17
    'update_q_then_reinit_some_limits': dict(D=5.5e-16, E=9.2e-16, c=6.9e-17),
    # measured 4.29e-16, 1e-15, 1.9e-16
    'update_P_then_reinit_some_limits': dict(D=5.4e-16, E=1.3e-15, c=2.4e-16),
}
# The ADMM checkpoint at k = 2 with the reference's scaling against the same checkpoint with a twin's scaling, in the term
# scales of admm_refs, per scenario of ADMM_SCENARIOS and quantity (tests/test_ruiz_refs.py measures and pins it).
# Columns of the measured values: x, y, pri_res, dua_res, obj_val, rho, rho_estimate.
ADMM_SENSITIVITY = {
    # measured 2.83e-16, 4.67e-16, 2.06e-16, 2.56e-17, 4.74e-17, 0, 1.27e-16
    'update_A': dict(x=3.6e-16, y=5.9e-16, pri_res=2.6e-16, dua_res=3.3e-17, obj_val=6e-17, rho=0.0, rho_estimate=1.6e-16),
    # measured 4.13e-16, 5.71e-16, 4.64e-17, 2.27e-17, 6.79e-17, 0, 5.27e-16
    'update_P': dict(x=5.2e-16, y=7.2e-16, pri_res=5.8e-17, dua_res=2.9e-17, obj_val=8.5e-17, rho=0.0, rho_estimate=6.6e-16),
    # measured 3.11e-16, 6.54e-16, 1.74e-16, 3.23e-17, 2.98e-17, 0, 2.9e-16
    'update_P_A_bounds_some': dict(x=3.9e-16, y=8.2e-16, pri_res=2.2e-16, dua_res=4.1e-17, obj_val=3.8e-17, rho=0.0, rho_estimate=3.7e-16),
}


RUIZ_BOUND = {name: {k: 32 * v for k, v in row.items()} for name, row in RUIZ_TWIN_ERROR.items()}


# ------------------------------------------------------------------ number types
def context(kind):
    if kind == "mp":
        import mpmath as mp
        return mp.workdps(DPS)
    return contextlib.nullcontext()


def num(v, kind):
    """float64 data in the number type of kind (exactly)"""
    v = np.asarray(v, np.float64)
    if kind == "f64":
        return v.copy()
    if kind == "ld":
        return v.astype(LD)
    import mpmath as mp
    out = np.empty(v.shape, dtype=object)
    for idx in np.ndindex(v.shape):
        out[idx] = mp.mpf(float(v[idx]))
    return out


class Pattern:
    """rows and columns of the stored entries of triu(P) and of A, in CSC order"""

    def __init__(self, P, A):
        import scipy.sparse as sp
        P, A = sp.csc_matrix(P), sp.csc_matrix(A)
        assert P.has_sorted_indices and A.has_sorted_indices
        self.n, self.m = A.shape[1], A.shape[0]
        self.Pi, self.Pj = P.indices.astype(np.int64), np.repeat(np.arange(self.n), np.diff(P.indptr))
        assert np.all(self.Pi <= self.Pj), "the upper triangle of P"
        self.Ai, self.Aj = A.indices.astype(np.int64), np.repeat(np.arange(self.n), np.diff(A.indptr))


class Ruiz:
    """The equilibration state of one QP in the number type of kind; mutation: one of MUTATIONS (a wrong implementation)."""

    def __init__(self, pat, iters, kind="ld", mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.pat, self.iters, self.kind, self.mutation = pat, int(iters), kind, mutation
        self.log = []                       # (what, iteration, the values passed to limit()) of every equilibration so far

    # ---- arithmetic that differs between the number types
    def _ones(self, k):
        return num(np.ones(k), self.kind)

    def _sqrt(self, v):
        if self.kind == "mp":
            import mpmath as mp
            return np.array([mp.sqrt(t) for t in v] + [None], dtype=object)[:-1]
        return np.sqrt(v)

    def _limit(self, v):
        if self.kind != "mp":
            low = v <= MIN_SCALING if self.mutation == "le_at_min" else v < MIN_SCALING
            v = np.where(low, v.dtype.type(1), v)
            return np.where(v > MAX_SCALING, v.dtype.type(MAX_SCALING), v)
        out = v.copy()
        for k in range(len(out)):
            t = out[k]
            low = t <= MIN_SCALING if self.mutation == "le_at_min" else t < MIN_SCALING
            t = t * 0 + 1 if low else t
            out[k] = t * 0 + MAX_SCALING if t > MAX_SCALING else t
        return out

    def _amax(self, dst, idx, vals):
        if self.kind == "mp":
            for k, t in zip(idx, vals):
                if t > dst[k]:
                    dst[k] = t
        else:
            np.maximum.at(dst, idx, vals)

    def _seqsum(self, v):
        """added up in index order (np.sum and np.mean add pairwise)"""
        s = v[0] * 0
        if self.kind == "mp":
            for t in v:
                s = s + t
            return s
        return np.cumsum(v)[-1] if len(v) else s

    # ---- the algorithm
    def _p_norms(self):
        pat = self.pat
        dn = self._ones(pat.n) * 0
        a = np.abs(self.Pv)
        self._amax(dn, pat.Pj, a)
        if self.mutation != "no_lower_triangle":
            self._amax(dn, pat.Pi, a)
        return dn

    def _scale(self):
        pat, n, m = self.pat, self.pat.n, self.pat.m
        self.D, self.E = self._ones(n), self._ones(m)
        if self.mutation != "c_not_reset" or not hasattr(self, "c"):
            self.c = self._ones(1)[0]
        for it in range(self.iters):
            dn, en = self._p_norms(), self._ones(m) * 0
            a = np.abs(self.Av)
            self._amax(dn, pat.Aj, a)
            self._amax(en, pat.Ai, a)
            self.log.append(("col", it, dn.copy())); self.log.append(("row", it, en.copy()))
            dn, en = 1 / self._sqrt(self._limit(dn)), 1 / self._sqrt(self._limit(en))
            self.Pv = self.Pv * dn[pat.Pi]; self.Pv = self.Pv * dn[pat.Pj]
            self.Av = self.Av * en[pat.Ai]; self.Av = self.Av * dn[pat.Aj]
            self.q = self.q * dn; self.D = self.D * dn; self.E = self.E * en
            dn = self._p_norms()
            cols = n
            if self.mutation == "mean_nonempty":
                cols = max(1, int(sum(1 for t in dn if t > 0)))
            mean = self._seqsum(dn) / cols
            nq = self._ones(1) * 0
            self._amax(nq, np.zeros(n, np.int64), np.abs(self.q))
            self.log.append(("q", it, nq.copy()))
            q1 = nq if self.mutation == "no_q_limit" else self._limit(nq)
            mx = q1.copy()
            self._amax(mx, np.zeros(1, np.int64), mean + 0 * q1)
            self.log.append(("c", it, mx.copy()))
            ct = (1 / self._limit(mx))[0]
            self.Pv = self.Pv * ct; self.q = self.q * ct; self.c = self.c * ct
        self.Dinv, self.Einv, self.cinv = 1 / self.D, 1 / self.E, 1 / self.c

    # ---- the calls
    def setup(self, Px, Ax, q):
        with context(self.kind):
            self.rawP, self.rawq = num(Px, self.kind), num(q, self.kind)
            self.Pv, self.Av, self.q = self.rawP.copy(), num(Ax, self.kind), self.rawq.copy()
            self._scale()
        return self

    def update(self, Px=None, Ax=None):
        """new raw values of triu(P) and / or of A (None: kept, unscaled with the scaling in force); q is always kept"""
        pat = self.pat
        with context(self.kind):
            if Px is not None:
                self.rawP = num(Px, self.kind)
                self.Pv = self.rawP.copy()
            else:
                v = self.Pv * self.cinv
                if self.mutation != "unscale_skips_a_product":
                    v = v * self.Dinv[pat.Pi]
                self.Pv = v * self.Dinv[pat.Pj]
            self.q = self.q * (self.cinv * self.Dinv)
            if Ax is not None:
                self.Av = num(Ax, self.kind)
            else:
                v = self.Av * self.Einv[pat.Ai]
                self.Av = v * self.Dinv[pat.Aj]
            self._scale()
        return self

    def fresh(self, Ax):
        """reinit_some: the raw P of setup (or of the last P update), the raw q in force, new A values"""
        with context(self.kind):
            self.Pv, self.q, self.Av = self.rawP.copy(), self.rawq.copy(), num(Ax, self.kind)
            self._scale()
        return self

    def update_q(self, q):
        with context(self.kind):
            self.rawq = num(q, self.kind)
            v = self.rawq * self.D
            self.q = v * self.c
        return self

    def scaling(self):
        return self.D.copy(), self.E.copy(), self.c


def rounded(r):
    """(D, E, c) of a reference, rounded to fp64"""
    D, E, c = r.scaling()
    return np.asarray(D, LD).astype(np.float64), np.asarray(E, LD).astype(np.float64), float(c)


# ------------------------------------------------------------------ the measures
def errors(got, ref, kind="ld"):
    """{D, E, c: worst relative error per entry} of a scaling got (floats, or long doubles with kind = "mp") against ref"""
    out = {}
    with context(kind):
        for key, g, r in zip(QUANTITIES, got, ref.scaling()):
            if key == "c":
                g, r = [g], [r]
            assert len(g) == len(r), key
            if kind == "mp":
                import mpmath as mp
                g = [mp.mpf(float(t)) + mp.mpf(float(LD(t) - LD(float(t)))) for t in g]
            else:
                g = np.asarray(g, LD)
            out[key] = float(max([abs(a - b) / abs(b) for a, b in zip(g, r)], default=0.0))
            assert np.isfinite(out[key]), key
    return out


def ratio(errs, name):
    """(worst error / bound over D, E, c; its key); a bound of 0.0 admits no error at all"""
    out, where = 0.0, None
    for k, e in errs.items():
        b = RUIZ_BOUND[name][k]
        r = (0.0 if e == 0.0 else float("inf")) if b == 0.0 else e / b
        if r >= out:
            out, where = r, k
    return out, where


def near_values(ref, twin):
    """[(what, iteration, index, value)]: the recorded values that make a case near (module docstring)"""
    assert len(ref.log) == len(twin.log)
    out = []
    for (what, it, a), (what2, it2, b) in zip(ref.log, twin.log):
        assert (what, it, len(a)) == (what2, it2, len(b))
        a, b = np.asarray(a, LD), np.asarray(b, np.float64)
        for thr in (MIN_SCALING, MAX_SCALING):
            exact = (a == LD(thr)) & (b == thr)
            close = (np.abs(a / LD(thr) - 1) <= NEAR) | (np.abs(b / thr - 1) <= NEAR)
            for k in np.nonzero(close & ~exact)[0]:
                out.append((what, it, int(k), float(b[k])))
    return out


# ------------------------------------------------------------------ the problems
def ruiz_form(n, m, nnzP, nnzA):
    """launch_ruiz's dispatch rule restated"""
    pa_len = nnzP + nnzA
    if n + m <= 16384 and pa_len <= 32 * 512:
        for vpt in (4, 8, 16):
            if pa_len <= vpt * 512:
                return f"reg{vpt}"
        return "reg32"
    return "global"


def form_of(pr):
    return ruiz_form(pr["n"], pr["m"], pr["P"].nnz, pr["A"].nnz)


def pa_len(pr):
    return pr["P"].nnz + pr["A"].nnz


def padded(pr, total, seed=3):
    """dense A rows (bounds -1, 1) appended until the pattern has exactly `total` entries"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    B, n = pr["Ax"].shape[0], pr["n"]
    while pa_len(pr) < total:
        k = min(n, total - pa_len(pr))
        cols = np.sort(rng.choice(n, size=k, replace=False))
        row = sp.csr_matrix((np.ones(k), (np.zeros(k, int), cols)), shape=(1, n))
        A_pat = sp.vstack([pr["A"], row]).tocsc(); A_pat.sort_indices()
        Ax = []
        for b in range(B):
            A = pr["A"].copy(); A.data = pr["Ax"][b].copy()
            rb = row.copy(); rb.data = rng.uniform(0.5, 1.5, k)
            Ab = sp.vstack([A, rb]).tocsc(); Ab.sort_indices()
            assert np.array_equal(Ab.indices, A_pat.indices) and Ab.nnz == A_pat.nnz
            Ax.append(Ab.data)
        pr = dict(pr, A=A_pat, Ax=np.array(Ax), m=pr["m"] + 1, l=np.hstack([pr["l"], -np.ones((B, 1))]),
                  u=np.hstack([pr["u"], np.ones((B, 1))]))
    assert pa_len(pr) == total
    return pr


def _entries(pr):
    P, A = pr["P"], pr["A"]
    return (P.indices, np.repeat(np.arange(pr["n"]), np.diff(P.indptr)), A.indices, np.repeat(np.arange(pr["n"]), np.diff(A.indptr)))


def _clear_column(pr, b, j, diag, a_max):
    """column j of QP b: P_jj = diag, every other stored entry of row / column j of P 0.0 (the rest of P is a principal
    submatrix: still PSD); the stored entries of column j of A: the first a_max, the others half of it (stored zeros stay)"""
    Pi, Pj, Ai, Aj = _entries(pr)
    pr["Px"][b, (Pi == j) | (Pj == j)] = 0.0
    pr["Px"][b, (Pi == j) & (Pj == j)] = diag
    ks = np.nonzero(Aj == j)[0]
    pr["Ax"][b, ks] = 0.5 * a_max
    pr["Ax"][b, ks[0]] = a_max


def limit_values(pr):
    """The limits of limit() as data of a random_box_qp batch (same patterns, stored zeros kept), QP by QP:
      0  column 2 all 0.0 (its identity row of A with it: an all-zero row); column 5: norm exactly 1e-4; column 8: 5e-5;
         columns 10, 11: P_10,10 = 0.01, P_11,11 = 100, P_10,11 = 0.9 and A's column 10 at 0.01, so that column 10 of the
         symmetric P takes its norm from the stored row 10 (the "lower triangle"); entries of G: exactly 1e4 and 1e9; -0.0
      1  q x 1e-3 and column 2 all 0.0: 1e-4 < |q|_inf < the mean column norm of P, taken over all n columns, the empty one
         included - the mean decides c
      2  P and q x 1e-7 (max(mean, |q|) < 1e-4: the cost factor is 1)
      3  q x 1e-7 alone (|q|_inf below 1e-4 is limited to 1 and decides c = 1; unlimited, the mean would)
      4  all of 0 and q x 1e6 (the cost factor saturates at 1e-4)
    QPs beyond 4 stay as they are."""
    pr = dict(pr, Px=pr["Px"].copy(), Ax=pr["Ax"].copy(), q=pr["q"].copy())
    B, n = pr["Ax"].shape[0], pr["n"]
    Pi, Pj, Ai, Aj = _entries(pr)
    SPECIAL = (2, 5, 8, 10, 11)
    assert n >= 12
    for b in range(B):
        if b in (0, 4):
            _clear_column(pr, b, 2, 0.0, 0.0)
            _clear_column(pr, b, 5, 1e-4, 1e-4)
            _clear_column(pr, b, 8, 5e-5, 5e-5)
            _clear_column(pr, b, 10, 0.01, 0.01)
            _clear_column(pr, b, 11, 100.0, 1.0)
            pr["Px"][b, (Pi == 10) & (Pj == 11)] = 0.9
            g = np.nonzero((Ai >= n) & ~np.isin(Aj, SPECIAL))[0]
            pr["Ax"][b, g[0]] = 1e4
            pr["Ax"][b, g[len(g) // 2]] = -1e9
            pr["Ax"][b, g[1]] = -0.0
            off = np.nonzero((Pi != Pj) & ~np.isin(Pi, SPECIAL) & ~np.isin(Pj, SPECIAL))[0]
            pr["Px"][b, off[3]] = -0.0
        if b == 4:
            pr["q"][b] *= 1e6
        if b == 1:
            pr["q"][b] *= 1e-3
            _clear_column(pr, b, 2, 0.0, 0.0)
        if b == 2:
            pr["Px"][b] *= 1e-7; pr["q"][b] *= 1e-7
        if b == 3:
            pr["q"][b] *= 1e-7
    return pr


# ------------------------------------------------------------------ the cases
B = 5
SMALL = dict(n=96, mg=64, nnz_per_row=6)                   # 950 entries: ruiz_reg_kernel<4>
# (name, shape of random_box_qp, entries to pad to or None, the form that must run)
FORM_PATTERNS = (
    ("reg4", SMALL, None, "reg4"),
    ("reg8", dict(n=320, mg=320, nnz_per_row=6), None, "reg8"),                 # 3 830
    ("reg8_full", dict(n=320, mg=320, nnz_per_row=6), 8 * 512, "reg8"),         # the last thread's last slot is occupied
    ("reg16_by_one", dict(n=320, mg=320, nnz_per_row=6), 8 * 512 + 1, "reg16"),
    ("reg16", dict(n=320, mg=320, nnz_per_row=8), None, "reg16"),               # 4 470
    ("reg32", dict(n=1000, mg=500, nnz_per_row=8), None, "reg32"),              # 9 990
    ("reg32_full", dict(n=1000, mg=1000, nnz_per_row=10), 32 * 512, "reg32"),
    ("global_by_one", dict(n=1000, mg=1000, nnz_per_row=10), 32 * 512 + 1, "global"),
    ("global", dict(n=2100, mg=500, nnz_per_row=8), None, "global"),            # 16 590, n = 2048 + 52: a second, partial chunk
)
ITERS = (1, 3, 10, 25)
SOME = (3, 1)                                              # the listed QPs of the per-QP calls: permuted, a strict subset
OTHER_SEED = 7000
# name -> steps (call, index of the value set the changed part comes from)
PATHS = {
    "update_A": (("update_A", 1),),
    "update_A_bounds": (("update_A_bounds", 1),),
    "update_P": (("update_P", 1),),
    "update_P_A": (("update_P_A", 1),),
    "update_A_bounds_device": (("update_A_bounds_device", 1),),
    "update_P_device": (("update_P_device", 1),),
    "update_P_A_bounds_device": (("update_P_A_bounds_device", 1),),
    "update_A_bounds_some": (("update_A_bounds_some", 1),),
    "update_P_some": (("update_P_some", 1),),
    "update_P_A_bounds_some": (("update_P_A_bounds_some", 1),),
    "reinit_some": (("reinit_some", 1),),
    "update_A_then_update_P": (("update_A", 1), ("update_P", 2)),
    "update_P_A_then_update_A_bounds": (("update_P_A", 1), ("update_A_bounds", 2)),
    "update_P_some_then_reinit_some": (("update_P_some", 1), ("reinit_some", 2)),
    "update_q_then_reinit_some": (("update_q", 1), ("reinit_some", 2)),
    "update_P_then_reinit_some": (("update_P", 1), ("reinit_some", 2)),
}
PER_QP = ("update_A_bounds_some", "update_P_some", "update_P_A_bounds_some", "reinit_some")
CHANGES = {                                                # what a call replaces
    "update_A": ("Ax",), "update_A_bounds": ("Ax", "l", "u"), "update_P": ("Px",), "update_P_A": ("Px", "Ax"),
    "update_A_bounds_device": ("Ax", "l", "u"), "update_P_device": ("Px",), "update_P_A_bounds_device": ("Px", "Ax", "l", "u"),
    "update_A_bounds_some": ("Ax", "l", "u"), "update_P_some": ("Px",), "update_P_A_bounds_some": ("Px", "Ax", "l", "u"),
    "reinit_some": ("Ax", "l", "u"), "update_q": ("q",),
}
ADMM_SCENARIOS = ("update_A", "update_P", "update_P_A_bounds_some")     # benign pattern: one ADMM checkpoint at k = 2 each
ADMM_K = 2


class Case:
    """One handle's life: setup on pr with `iters` equilibration iterations, then the steps of a path.  sets[k]: the value set
    (a batch dict on pr's patterns) step k takes its changed part from.  ids: the QPs the per-QP calls list."""

    def __init__(self, name, pr, iters=10, path=None, sets=(), form=None):
        self.name, self.pr, self.iters, self.path, self.sets = name, pr, iters, path, tuple(sets)
        self.steps = PATHS[path] if path else ()
        self.B = pr["Ax"].shape[0]
        self.ids = [b for b in SOME if b < self.B] if self.B > 2 else [self.B - 1]
        self.form = form_of(pr) if form is None else form
        self.pat = Pattern(pr["P"], pr["A"])
        self._models = {}

    def data_after(self, upto=None):
        """the raw data in force after the first `upto` steps (default: all)"""
        cur = {k: self.pr[k].copy() for k in ("Px", "Ax", "q", "l", "u")}
        for call, k in self.steps[:upto]:
            rows = self.ids if call in PER_QP else list(range(self.B))
            for key in CHANGES[call]:
                cur[key][rows] = self.sets[k][key][rows]
        return dict(self.pr, **cur)

    def model(self, b, kind="ld", mutation=None):
        """the Ruiz state of QP b after the whole path"""
        ids = self.ids
        key = (b, kind, mutation, tuple(ids))
        if key in self._models:
            return self._models[key]
        pr = self.pr
        r = Ruiz(self.pat, self.iters, kind, mutation).setup(pr["Px"][b], pr["Ax"][b], pr["q"][b])
        for call, k in self.steps:
            if call in PER_QP and b not in ids:
                continue
            new = self.sets[k]
            if call == "update_q":
                r.update_q(new["q"][b])
            elif call == "reinit_some":
                r.fresh(new["Ax"][b])
            else:
                ch = CHANGES[call]
                r.update(Px=new["Px"][b] if "Px" in ch else None, Ax=new["Ax"][b] if "Ax" in ch else None)
        if mutation is None:
            self._models[key] = r
        return r

    def oracle_scaling(self, b):
        """the second twin (module docstring)"""
        from oracle import oracle as O
        import scipy.sparse as sp

        def mats(d):
            P = self.pr["P"].copy(); P.data = d["Px"][b].copy()
            A = self.pr["A"].copy(); A.data = d["Ax"][b].copy()
            return sp.csc_matrix(P), sp.csc_matrix(A)

        kw = dict(scaling=self.iters)
        d = self.pr
        P, A = mats(d)
        o = O.OracleQPSolver(P, d["q"][b], A, d["l"][b], d["u"][b], **kw)
        new_q = False                                      # (update_q: no equilibration; the oracle keeps the old q until its next setup)
        for s, (call, k) in enumerate(self.steps):
            if call in PER_QP and b not in self.ids:
                continue
            if call == "update_q":
                new_q = True
                continue
            d = self.data_after(s + 1)
            P, A = mats(d)
            if call != "reinit_some" and "Px" not in CHANGES[call] and not new_q:
                o.update(d["l"][b], A, d["u"][b])
            else:
                o, new_q = O.OracleQPSolver(P, d["q"][b], A, d["l"][b], d["u"][b], **kw), False
        return o.scaling()


_CASES = {}


def cases():
    """{name: Case}: every handle the GPU tests make (built once)"""
    if _CASES:
        return _CASES
    from osqp_solver_amd import problems as PR
    from test_gpu_ops import tiny_qp

    def add(name, *a, **kw):
        _CASES[name] = Case(name, *a, **kw)

    for name, shape, total, form in FORM_PATTERNS:
        pr = PR.random_box_qp(B, **shape)
        if total:
            pr = padded(pr, total)
        add("form_" + name, pr, form=form)
    benign = PR.random_box_qp(B, **SMALL)
    limits = limit_values(benign)
    glob = PR.random_box_qp(B, **FORM_PATTERNS[-1][1])
    add("limits_global", limit_values(glob), form="global")
    add("tiny_n1_m2", tiny_qp(B, 1, 2)); add("tiny_n4_m0", tiny_qp(B, 4, 0))
    for it in ITERS:
        add(f"iters{it}_benign", benign, iters=it); add(f"iters{it}_limits", limits, iters=it)
    for kind, base, edit in (("benign", benign, lambda p: p), ("limits", limits, limit_values)):
        sets = (base,) + tuple(edit(PR.random_box_qp(B, value_seed=OTHER_SEED + 1000 * k, **SMALL)) for k in (0, 1))
        for path in PATHS:
            add(f"{path}_{kind}", base, path=path, sets=sets)
    for c in _CASES.values():
        assert form_of(c.pr) == c.form, (c.name, form_of(c.pr), pa_len(c.pr))
    return _CASES


def one_blas_thread():
    from factor_refs import one_blas_thread as f
    return f()


def measure_twins(case):
    """{D, E, c: worst error of the two fp64 twins against the reference} over the case's QPs"""
    out = {k: 0.0 for k in QUANTITIES}
    for b in range(case.B):
        ref = case.model(b)
        for got in (case.model(b, "f64").scaling(), case.oracle_scaling(b)):
            for k, e in errors(got, ref).items():
                out[k] = max(out[k], e)
    return out


# ------------------------------------------------------------------ the ADMM checkpoint under the reference's scaling
_ADMM = {}


def admm_case(path):
    """the benign pattern after `path` as a case of admm_refs (scenario "box"), one checkpoint at k = ADMM_K"""
    import admm_refs as AF
    if path not in _ADMM:
        c = cases()[path + "_benign"]
        _ADMM[path] = AF.Case("ruiz_" + path, "box", c.data_after(), AF.EPS, (ADMM_K,))
    return _ADMM[path]


def admm_bound(path):
    import admm_refs as AF
    return {k: AF.ITERATE_BOUND["box"][k] + ADMM_SENSITIVITY[path][k] for k in AF.KEYS}


def measure_admm_sensitivity(path):
    """{quantity: distance between the checkpoint with the reference's scaling and with a twin's}, over the QPs and both twins"""
    import admm_refs as AF
    c, ac = cases()[path + "_benign"], admm_case(path)
    out = {k: 0.0 for k in AF.KEYS}
    for b in range(c.B):
        ref = AF.reference(ac, b, *rounded(c.model(b)))[(0, ADMM_K)]
        for D, E, cc in (c.model(b, "f64").scaling(), c.oracle_scaling(b)):
            other = ac.run(b, D, E, float(cc))[(0, ADMM_K)]
            got = {k: np.asarray(other[k], LD).astype(np.float64) if np.ndim(other[k]) else float(other[k]) for k in AF.KEYS}
            for k, e in AF.errors(got, ref).items():
                out[k] = max(out[k], e)
    return out
