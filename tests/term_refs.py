"""Reference for the termination decision (DESIGN.md section 8 "Infeasibility certificates"), written
from the specification alone on top of admm_refs.Admm (a helper module of the tests, not a conftest).  No solver code is involved.

Term runs admm_refs' iteration and check to the exit the specification prescribes.  At a check iteration, and at max_iter,
with f = 1 (and f = 10 in the closing check of an undecided solve) on all four tolerances, unscale = scaling and not
scaled_termination, W_D = D, W_E = E, cs = c if unscale else W_D = W_E = I, cs = 1:
  pri   pri_res < f eps_abs + f eps_rel pri_nrm (m = 0: holds)          dua   dua_res < f eps_abs + f eps_rel dua_nrm
  primal infeasibility, tested only where pri fails: v = delta_y projected by bound type (0 on a free row, min(., 0) where
        only u is infinite, max(., 0) where only l is; infinite: beyond 1e30 x 1e-4 in the scaled bounds), norm_dy = |W_E v|_inf
    guard_dy  norm_dy > 1e-30      support  us'v+ + ls'v- < -f eps_prim_inf norm_dy      atdy  |W_D^-1 As'v|_inf < f eps_prim_inf norm_dy
  dual infeasibility, tested only where dua fails: norm_dx = |W_D delta_x|_inf
    guard_dx  norm_dx > 1e-30      qdx  qs'delta_x < -cs f eps_dual_inf norm_dx          pdx   |W_D^-1 Ps delta_x|_inf < cs f eps_dual_inf norm_dx
    cone_u    (W_E^-1 As delta_x)_i <= f eps_dual_inf norm_dx on every row with a finite u;  cone_l  >= -f eps ... with a finite l
  pri and dua -> 1 (2 at f = 10); else primal infeasible -> -3 (3); else dual infeasible -> -4 (4); undecided at max_iter -> -2
Order of events at iteration i: the iteration; on a check iteration or at max_iter the decision at f = 1; on a rho iteration,
if that left the solve undecided (or at max_iter off a check iteration), admm_refs' rho estimate and update; at max_iter, if
undecided, the decision at f = 10.  Published: admm_refs' pri_res, dua_res, rho, rho_updates; obj_val = 1e30 exactly for -3 / 3,
-1e30 for -4 / 4; x, y all NaN for those four; the certificate W_E v / norm_dy or W_D delta_x / norm_dx - the vector the accepted
test saw, in the space it ran in, so that its largest entry is exactly +-1.  After an infeasible exit x = y = z = 0, rho stays.

The LEDGER of a solve holds one entry per decision taken: dict(iter, f, ratio = {clause: r}), every clause written so that it
holds iff r < 1 (support: f eps norm_dy / -lhs, inf where lhs >= 0; the guards: 1e-30 / norm; cone_u / cone_l: the largest row term
over f eps norm_dx, -inf without such a row) - all clauses, also those the decision did not reach.

Number types as in admm_refs: "ld" is the reference, "mp" pins it (REF_ERROR), the two "f64" twins are the only source of every
tolerance.  The distance of two values of a ratio is |r - r'| where the reference's |r| <= 1 and |1 / r - 1 / r'| beyond: at a
threshold both are the relative error, and a clause missed by 1e8 whose numerator is a cancelled sum does not count for more
than it can decide.  CLAUSE_TWIN_ERROR[case]: the twins' worst such distance over the ledger; a ratio is NEAR within CLAUSE_NEAR =
32 x that of 1, and no case has one (cap zero).  RES_TWIN_ERROR / CERT_TWIN_ERROR[case]: the twins' worst error of pri_res, dua_res,
obj_val, x, y (admm_refs' term scales) and of a certificate entry (absolute: unit vectors); bounds 32 x those (FLOORED: four named entries).
tests/test_term_refs.py measures all of them again and pins measured <= constant <= 2 x measured."""
import numpy as np

import admm_refs as AF
import op_refs as R

INF_ROW = R.OQ_INFTY * R.OQ_MIN_SCALING
CLAUSES = ("pri", "dua", "guard_dy", "support", "atdy", "guard_dx", "qdx", "pdx", "cone_u", "cone_l")
PINF_CLAUSES, DINF_CLAUSES = ("support", "atdy"), ("qdx", "pdx", "cone")
MUTATIONS = ("no_c_qdx", "no_c_pdx", "no_dinv_atdy", "no_dinv_pdx", "no_einv_cone", "no_de_norms", "ndy_before_projection",
             "projection_swapped", "cone_upper_only", "inf_at_1e30", "ten_on_residuals_only", "cert_scaled_space",
             "cert_unprojected_norm")
MARGIN = 32
RES_KEYS = ("pri_res", "dua_res", "obj_val", "x", "y")
# Worst error of the fp64 twins against the long-double reference per case (the measured values beside each; module docstring).
# A bound is MARGIN x the constant and nothing else, with the exceptions named in FLOORED: entries whose constant lies below
# 2^-53 / MARGIN, so that MARGIN x it is less than ONE fp64 round-off of the quantity's scale.  There the twins meet the reference
# by cancellation, not by accuracy (m = 0 with scaling: dua_res = |c D q| / (c D) in one entry, the factors cancel in the twins'
# order of operations; the certificates after 5 or 10 iterations: every entry but the unit one is below 1e-6, its error below
# 1e-22), and an fp64 evaluation in another order cannot be held to less than its own last bit: those entries get MARGIN
# round-offs.  A constant of 0.0 admits no error at all.  tests/test_term_refs.py asserts that FLOORED is exactly that set.
FLOOR = R.U
FLOORED = (("close_on", "cert"), ("m0_s10", "cert"), ("m0_s10", "dua_res"), ("m0_s0", "cert"))
TWIN = {
    # measured clause 1.93e-12, cert 3.84e-14, pri_res 7.12e-16, dua_res 3.24e-16, obj_val 2.3e-16, x 1.67e-15, y 6.7e-16
    's10_a': dict(clause=2.4e-12, cert=4.8e-14, pri_res=8.9e-16, dua_res=4e-16, obj_val=2.9e-16, x=2.1e-15, y=8.4e-16),
    # measured clause 3.27e-12, cert 1.19e-14, pri_res 7.71e-16, dua_res 6.17e-17, obj_val 1.95e-16, x 1.03e-15, y 5.26e-16
    's10_b': dict(clause=4.1e-12, cert=1.5e-14, pri_res=9.6e-16, dua_res=7.7e-17, obj_val=2.4e-16, x=1.3e-15, y=6.6e-16),
    # measured clause 3.88e-13, cert 2.24e-14, pri_res 2.89e-15, dua_res 3.63e-17, obj_val 2.3e-16, x 1.12e-15, y 3.7e-16
    's10_c': dict(clause=4.9e-13, cert=2.8e-14, pri_res=3.6e-15, dua_res=4.5e-17, obj_val=2.9e-16, x=1.4e-15, y=4.6e-16),
    # measured clause 1.9e-10, cert 1.27e-14, pri_res 1.71e-15, dua_res 1.17e-14, obj_val 1.14e-16, x 2.65e-14, y 1.89e-14
    's10_d': dict(clause=2.4e-10, cert=1.6e-14, pri_res=2.1e-15, dua_res=1.5e-14, obj_val=1.4e-16, x=3.3e-14, y=2.4e-14),
    # measured clause 4.14e-12, cert 7.92e-14, pri_res 2.45e-16, dua_res 4.54e-16, obj_val 2.61e-16, x 2.03e-15, y 6.83e-16
    's0': dict(clause=5.2e-12, cert=9.9e-14, pri_res=3.1e-16, dua_res=5.7e-16, obj_val=3.3e-16, x=2.5e-15, y=8.5e-16),
    # measured clause 1.62e-12, cert 1.04e-14, pri_res 7.67e-16, dua_res 6.24e-17, obj_val 1.95e-16, x 1.17e-15, y 5.05e-16
    'st': dict(clause=2e-12, cert=1.3e-14, pri_res=9.6e-16, dua_res=7.8e-17, obj_val=2.4e-16, x=1.5e-15, y=6.3e-16),
    # measured clause 1.22e-13, cert 2.24e-18, pri_res 7.12e-16, dua_res 2.43e-16, obj_val 2.34e-16, x 2.8e-15, y 5.49e-16
    'close_on': dict(clause=1.5e-13, cert=2.8e-18, pri_res=8.9e-16, dua_res=3e-16, obj_val=2.9e-16, x=3.5e-15, y=6.9e-16),
    # measured clause 1.3e-13, cert 1.36e-14, pri_res 8.2e-16, dua_res 8.31e-17, obj_val 1.51e-16, x 2.47e-15, y 6.74e-16
    'close_off': dict(clause=1.6e-13, cert=1.7e-14, pri_res=1e-15, dua_res=1e-16, obj_val=1.9e-16, x=3.1e-15, y=8.4e-16),
    # measured clause 1.41e-10, cert 3.76e-13, pri_res 1.63e-14, dua_res 2.88e-16, obj_val 1.88e-16, x 1.39e-15, y 2.62e-15
    'rho': dict(clause=1.8e-10, cert=4.7e-13, pri_res=2e-14, dua_res=3.6e-16, obj_val=2.4e-16, x=1.7e-15, y=3.3e-15),
    # measured clause 3.88e-13, cert 4.04e-14, pri_res 2.89e-15, dua_res 5.19e-17, obj_val 8.5e-17, x 8.13e-16, y 3.94e-16
    'ct0': dict(clause=4.9e-13, cert=5e-14, pri_res=3.6e-15, dua_res=6.5e-17, obj_val=1.1e-16, x=1e-15, y=4.9e-16),
    # measured clause 1.21e-10, cert 8.54e-15, pri_res 2.53e-15, dua_res 2e-16, obj_val 0, x 0, y 0
    'n1m2_s10': dict(clause=1.5e-10, cert=1.1e-14, pri_res=3.2e-15, dua_res=2.5e-16, obj_val=0.0, x=0.0, y=0.0),
    # measured clause 5.2e-18, cert 3.47e-22, pri_res 0, dua_res 9.38e-21, obj_val 0, x 0, y 0
    'm0_s10': dict(clause=6.5e-18, cert=4.3e-22, pri_res=0.0, dua_res=1.2e-20, obj_val=0.0, x=0.0, y=0.0),
    # measured clause 1.01e-10, cert 8.25e-15, pri_res 1.83e-15, dua_res 1.49e-16, obj_val 0, x 0, y 0
    'n1m2_s0': dict(clause=1.3e-10, cert=1e-14, pri_res=2.3e-15, dua_res=1.9e-16, obj_val=0.0, x=0.0, y=0.0),
    # measured clause 3.9e-18, cert 2.24e-22, pri_res 0, dua_res 0, obj_val 0, x 0, y 0
    'm0_s0': dict(clause=4.9e-18, cert=2.8e-22, pri_res=0.0, dua_res=0.0, obj_val=0.0, x=0.0, y=0.0),
}
CLAUSE_TWIN_ERROR = {k: v["clause"] for k, v in TWIN.items()}
CLAUSE_NEAR = {k: MARGIN * v for k, v in CLAUSE_TWIN_ERROR.items()}


def _bound(case, q):
    v = TWIN[case][q]
    return MARGIN * (FLOOR if (case, q) in FLOORED else v)


CERT_BOUND = {k: _bound(k, "cert") for k in TWIN}
RES_BOUND = {k: {q: _bound(k, q) for q in RES_KEYS} for k in TWIN}
# the long-double reference against mpmath on the n = 12, m = 20 shape (tests/test_term_refs.py: measured <= constant <= 2 x measured)
REF_ERROR = dict(clause=3.5e-17, cert=2.1e-19, res=4.7e-19)        # measured 2.78e-17, 1.65e-19, 3.77e-19


class Term(AF.Admm):
    """admm_refs.Admm run to its exit.  mutation (tests): one deliberate defect of MUTATIONS."""

    def __init__(self, *a, mutation=None, **kw):
        assert mutation is None or mutation in MUTATIONS
        self.mutation = mutation
        super().__init__(*a, **kw)

    def _data(self, l, u):
        super()._data(l, u)
        thr = R.OQ_INFTY if self.mutation == "inf_at_1e30" else INF_ROW            # (the check's own reading of the bounds)
        self.lfin_t = np.array([float(v) for v in self.ls], np.float64) > -thr
        self.ufin_t = np.array([float(v) for v in self.us], np.float64) < thr

    def _decide(self, k, f):
        """(status or 0, {clause: ratio}, (projected delta_y in the test's space, norm_dy, delta_x likewise, norm_dx))"""
        st, zero, one, mut = self.st, self.zero, self.one, self.mutation
        num = lambda v: self.num(v)[()]
        fi = 1.0 if (mut == "ten_on_residuals_only") else f
        eps_abs, eps_rel = num(f * st["eps_abs"]), num(f * st["eps_rel"])
        eps_p, eps_d = num(fi * st["eps_prim_inf"]), num(fi * st["eps_dual_inf"])
        unscale = bool(st["scaling"]) and not st["scaled_termination"]
        inf, fl = float("inf"), float
        r = {}
        eps_prim, eps_dual = eps_abs + eps_rel * k["pn"], eps_abs + eps_rel * k["dn"]
        prim_ok = (not self.m) or bool(k["pri"] < eps_prim)
        dual_ok = bool(k["dua"] < eps_dual)
        r["pri"], r["dua"] = (fl(k["pri"] / eps_prim) if self.m else 0.0), fl(k["dua"] / eps_dual)
        # ---- primal infeasibility
        lo_inf, up_inf = ~self.lfin_t, ~self.ufin_t
        dn, dp = np.minimum(self.dy, zero), np.maximum(self.dy, zero)
        if mut == "projection_swapped":
            dn, dp = dp, dn
        v = np.where(up_inf, np.where(lo_inf, self.dy * zero, dn), np.where(lo_inf, dp, self.dy))
        wE = self.E if (unscale and mut != "no_de_norms") else self.E * 0 + one
        wD = self.D if (unscale and mut != "no_de_norms") else self.D * 0 + one
        ndy = AF._ninf(wE * (self.dy if mut == "ndy_before_projection" else v), zero)
        lhs = np.sum(self.us * np.maximum(v, zero) + self.ls * np.minimum(v, zero)) if self.m else zero
        atdy = self.As.T @ v
        if unscale and mut != "no_dinv_atdy":
            atdy = atdy / self.D
        atdy = AF._ninf(atdy, zero)
        g_dy = bool(ndy > num(AF.INF_DIV_TOL))
        # (what the projection did, for the tests' populations: |W_E delta_y| / norm_dy, the two argmax rows, the two signs of the sum)
        raw = wE * self.dy
        lhs_raw = np.sum(self.us * np.maximum(self.dy, zero) + self.ls * np.minimum(self.dy, zero)) if self.m else zero
        am = lambda t: int(np.argmax(np.abs(np.array([fl(s_) for s_ in t])))) if self.m else -1
        self.projection = dict(norm_raw_over_norm=fl(AF._ninf(raw, zero) / ndy) if ndy > 0 else inf, argmax_raw=am(raw), argmax=am(wE * v),
                               sum_raw_negative=bool(lhs_raw < 0), sum_negative=bool(lhs < 0))
        r["guard_dy"] = fl(num(AF.INF_DIV_TOL) / ndy) if ndy > 0 else inf
        r["support"] = fl(eps_p * ndy / -lhs) if (g_dy and lhs < 0) else inf
        r["atdy"] = fl(atdy / (eps_p * ndy)) if g_dy else inf
        prim_inf = (not prim_ok) and g_dy and bool(lhs < -eps_p * ndy) and bool(atdy < eps_p * ndy)
        # ---- dual infeasibility
        dx = self.dx
        ndx = AF._ninf(wD * dx, zero)
        cs = self.c if unscale else one
        cq, cp = (one if mut == "no_c_qdx" else cs), (one if mut == "no_c_pdx" else cs)
        qdx = self.qs @ dx
        pdx = self.Ps @ dx
        if unscale and mut != "no_dinv_pdx":
            pdx = pdx / self.D
        pdx = AF._ninf(pdx, zero)
        adx = self.As @ dx
        if unscale and mut != "no_einv_cone":
            adx = adx / self.E
        g_dx = bool(ndx > num(AF.INF_DIV_TOL))
        r["guard_dx"] = fl(num(AF.INF_DIV_TOL) / ndx) if ndx > 0 else inf
        r["qdx"] = fl(cq * eps_d * ndx / -qdx) if (g_dx and qdx < 0) else inf
        r["pdx"] = fl(pdx / (cp * eps_d * ndx)) if g_dx else inf
        up_rows = self.ufin_t
        lo_rows = self.lfin_t if mut != "cone_upper_only" else np.zeros(self.m, bool)
        cu = max([t for t in adx[up_rows]], default=None)
        cl = max([-t for t in adx[lo_rows]], default=None)
        self.cone_rows = (int(np.flatnonzero(up_rows)[np.argmax(adx[up_rows].astype(np.float64))]) if cu is not None else -1,
                          int(np.flatnonzero(lo_rows)[np.argmax(-adx[lo_rows].astype(np.float64))]) if cl is not None else -1)
        r["cone_u"] = -inf if cu is None else (fl(cu / (eps_d * ndx)) if g_dx else inf)
        r["cone_l"] = -inf if cl is None else (fl(cl / (eps_d * ndx)) if g_dx else inf)
        cone = (cu is None or bool(cu <= eps_d * ndx)) and (cl is None or bool(cl <= eps_d * ndx))
        dual_inf = (not dual_ok) and g_dx and bool(qdx < -cq * eps_d * ndx) and bool(pdx < cp * eps_d * ndx) and cone
        status = (2 if f != 1.0 else 1) if (prim_ok and dual_ok) else (3 if f != 1.0 else -3) if prim_inf else \
                 (4 if f != 1.0 else -4) if dual_inf else 0
        return status, r, (v, ndy, dx, ndx)

    def _certificate(self, status, seen):
        st, zero, one, mut = self.st, self.zero, self.one, self.mutation
        unscale = bool(st["scaling"]) and not st["scaled_termination"]
        v, ndy, dx, ndx = seen
        if status in (-3, 3):
            if mut == "cert_scaled_space":
                return v / AF._ninf(v, zero)
            if mut == "cert_unprojected_norm":
                ndy = AF._ninf((self.E if unscale else self.E * 0 + one) * self.dy, zero)
            return (self.E * v if unscale else v) / ndy
        if mut == "cert_scaled_space":
            return dx / AF._ninf(dx, zero)
        return (self.D * dx if unscale else dx) / ndx

    def solve(self):
        """one solve from the state in force to its exit: dict(status, iter, rho_updates, rho, pri_res, dua_res, obj_val, x, y,
        cert (None with a solution), ledger, rho_margin, scale)"""
        st = self.st
        last = int(st["max_iter"])
        ct, ri = st["check_termination"], st["adaptive_rho_interval"] if st["adaptive_rho"] else 0
        tol = self.num(st["adaptive_rho_tolerance"])[()]
        ledger, self.rho_margin, self.rho_events = [], float("inf"), []
        with AF.context(self.kind):
            for it in range(1, last + 1):
                self._iterate()
                is_check, is_rho, is_last = bool(ct) and it % ct == 0, bool(ri) and it % ri == 0, it == last
                if not (is_check or is_rho or is_last):
                    continue
                k = self._check()
                status, seen = 0, None
                if is_check or is_last:
                    status, ratio, seen = self._decide(k, 1.0)
                    ledger.append(dict(iter=it, f=1, ratio=ratio, cone_rows=self.cone_rows, projection=self.projection))
                if is_rho and (status == 0 or (is_last and not is_check)):
                    rn = self._estimate(k)
                    lo, hi = self.rho / tol, self.rho * tol
                    self.rho_margin = min(self.rho_margin, float(abs(rn - lo) / lo), float(abs(rn - hi) / hi))
                    update = bool(rn > hi or rn < lo)
                    self.rho_events.append((it, float(rn), update))
                    if update:
                        self.rho = rn
                        self.rho_updates += 1
                        self._refactor()
                if is_last and status == 0:
                    status, ratio, seen = self._decide(k, 10.0)
                    ledger.append(dict(iter=it, f=10, ratio=ratio, cone_rows=self.cone_rows, projection=self.projection))
                    status = status or -2
                if status:
                    return self._finish(k, it, status, seen, ledger)
        raise AssertionError("no exit")

    def _finish(self, k, it, status, seen, ledger):
        one, zero = self.one, self.zero
        x = self.D * self.x
        y = self.E * self.y / self.c if self.st["scaling"] else self.y * one
        out = dict(status=status, iter=it, rho_updates=self.rho_updates, rho=self.rho, pri_res=k["pri"], dua_res=k["dua"],
                   obj_val=k["obj"], x=x, y=y, cert=None, ledger=ledger, rho_margin=self.rho_margin, rho_events=list(self.rho_events),
                   scale=dict(k["scale"], x=max(one, AF._ninf(x, zero)), y=max(one, AF._ninf(y, zero))))
        if status in (-3, 3, -4, 4):
            out["obj_val"] = self.num(R.OQ_INFTY if status in (-3, 3) else -R.OQ_INFTY)[()]
            out["x"], out["y"] = np.full(self.n, np.nan), np.full(self.m, np.nan)
            out["cert"] = self._certificate(status, seen)
            self.x, self.z, self.y = self.x * zero, self.z * zero, self.y * zero
        return out


# ------------------------------------------------------------------ reading a ledger
def held(entry, clause):
    r = entry["ratio"]
    if clause == "cone":
        return r["cone_u"] < 1 and r["cone_l"] < 1
    return r[clause] < 1


def inf_clauses(kind):
    return ("guard_dy",) + PINF_CLAUSES if kind == "pinf" else ("guard_dx",) + DINF_CLAUSES


def decided_by(res):
    """the clauses of the accepted test that the exit check is the first to hold, every other clause of that test having held
    at the decision before (same f); None where there is no decision before"""
    led = res["ledger"]
    if len(led) < 2 or led[-1]["f"] != led[-2]["f"]:
        return None
    st = res["status"]
    group = ("pri", "dua") if st in (1, 2) else inf_clauses("pinf") if st in (-3, 3) else inf_clauses("dinf") if st in (-4, 4) else ()
    group = tuple(c for g in group for c in (("cone_u", "cone_l") if g == "cone" else (g,)))
    return tuple(c for c in group if held(led[-1], c) and not held(led[-2], c))


def ratio_distance(r, ref):
    """module docstring: the distance of two values of a ratio"""
    if not np.isfinite(ref) or not np.isfinite(r):
        return 0.0 if r == ref else float("inf")
    if abs(ref) <= 1:
        return abs(r - ref)
    return abs(1.0 / r - 1.0 / ref) if r != 0 else float("inf")


def nearest(res):
    """(smallest |r - 1| over the ledger, where)"""
    best, where = float("inf"), None
    for e in res["ledger"]:
        for c, r in e["ratio"].items():
            if np.isfinite(r) and abs(r - 1) < best:
                best, where = abs(r - 1), (e["iter"], e["f"], c)
    return best, where


def cert_gap(v):
    """|largest| - |second largest| of a certificate"""
    a = np.sort(np.abs(np.asarray(v, np.float64)))
    return float(a[-1] - a[-2]) if a.size > 1 else float("inf")


# ------------------------------------------------------------------ the cases
BASE_B = 12
BASE_SHAPE = dict(n=96, mg=64, nnz_per_row=6)


class TCase:
    """One batch under one set of settings.  solves: the calls of a handle, each "solve" or ("bounds", l [B, m], u [B, m])."""

    def __init__(self, name, pr, settings, solves=("solve",)):
        self.name, self.pr, self.settings, self.solves = name, pr, dict(settings), tuple(solves)
        self.B = pr["Ax"].shape[0]

    qp = AF.Case.qp

    def run(self, b, D, E, c, kind="ld", perm=None, tail=0, mutation=None):
        """[result of every solve] of QP b"""
        d = self.qp(b)
        a = Term(d["P"], d["q"], d["A"], d["l"], d["u"], D, E, c, kind=kind, perm=perm, tail=tail, mutation=mutation, **self.settings)
        out = []
        for s in self.solves:
            if s == "solve":
                out.append(a.solve())
            else:
                a.update_bounds(s[1][b], s[2][b])
        return out

    def oracle(self, b, **kw):
        from oracle import oracle as O
        d = self.qp(b)
        return O.OracleQPSolver(d["P"], d["q"], d["A"], d["l"], d["u"], **dict(self.settings, **kw))


def _base():
    from osqp_solver_amd import problems as PR
    return PR.random_box_qp(BASE_B, **BASE_SHAPE)


def scale_row(pr, r_, s):
    """row r_ of A of QP 0 and its two finite bounds times s, in place: the same feasible set (s < 0 swaps the bounds)"""
    pr["Ax"][0, pr["A"].indices == r_] *= s
    lo, up = pr["l"][0, r_], pr["u"][0, r_]
    assert abs(lo) < 1e29 and abs(up) < 1e29
    pr["l"][0, r_], pr["u"][0, r_] = (s * lo, s * up) if s > 0 else (s * up, s * lo)


def pinf_qp(base, b, gap=1.0, row=None, row_scale=(), one_sided=()):
    """QP b of base, primal infeasible with a gap parameter: row `row` (default n) asks for a'x in [cap + gap, cap + 2 gap], cap
    the most the boxes admit (exit_cases.make_pinf is gap = 1).  one_sided: [(row, "l" | "u")] boxed rows that keep that bound only."""
    import exit_cases as EC
    out = EC.take(base, [b])
    EC.make_pinf(out, 0, row)
    n = out["n"]
    row = n if row is None else row
    cap = out["l"][0, row] - 1.0
    out["l"][0, row], out["u"][0, row] = cap + gap, cap + 2 * gap
    for r_, f in row_scale:
        scale_row(out, r_, f)
    for r_, side in one_sided:
        if side == "l":
            out["u"][0, r_] = 1e30
        else:
            out["l"][0, r_] = -1e30
    return out


def dinf_qp(base, b, push=1.0, one_sided=(), row_scale=(), col_scale=()):
    """QP b of base, dual infeasible along -e_0 (exit_cases.make_dinf).  row_scale: [(row, factor)] on A, l, u - the same
    feasible set (a negative factor swaps the bounds: the mirrored row); col_scale: [(column, factor)] on P and q, a factor s scaling P_jj by s^2 - the substitution x_j = s x_j'
    restricted to the objective's curvature and slope of a column other than 0 (P stays positive semidefinite, P e_0 = 0)."""
    import exit_cases as EC
    out = EC.take(base, [b])
    EC.make_dinf(out, 0, push)
    A, P = out["A"], out["P"]
    for r_, s in row_scale:
        scale_row(out, r_, s)
    cols = np.repeat(np.arange(P.shape[1]), np.diff(P.indptr))
    for j, s in col_scale:
        assert j != 0
        out["Px"][0, cols == j] *= s
        out["Px"][0, P.indices == j] *= s
        out["q"][0, j] *= s
    for r_, side in one_sided:
        if side == "l":
            out["u"][0, r_] = 1e30
        else:
            out["l"][0, r_] = -1e30
    return out


def stack(prs):
    out = dict(prs[0])
    for k in ("Px", "Ax", "q", "l", "u"):
        out[k] = np.concatenate([p[k] for p in prs])
    return out


def _sided_rows(pr, keep, count, seed):
    """count rows of QP 0 with two finite bounds, outside `keep`, alternately left with l alone and with u alone"""
    rng = np.random.default_rng(seed)
    rows = [r for r in range(pr["m"]) if r not in keep and pr["u"][0, r] < 1e29 and pr["l"][0, r] > -1e29]
    return [(int(r), "l" if i % 2 else "u") for i, r in enumerate(rng.choice(rows, size=count, replace=False))]


# the QPs of the main batch (n = 96, m = 160): name -> (kind, base QP); B = 11 leaves a ragged last tile for tiles of 2 and of 4
BATCH = ("pinf0", "pinf2_norm", "feas0", "pinf2_sided", "dinf2_scaled_u", "feas1", "pinf1", "dinf0_weak", "pinf0_gap", "dinf1_sided", "dinf2_scaled_l")
KIND = {n_: n_[:4] for n_ in BATCH}
BASE_OF = dict(pinf0=0, pinf2_norm=2, feas0=0, pinf2_sided=2, dinf2_scaled_u=2, feas1=1, pinf1=1, dinf0_weak=0, pinf0_gap=0, dinf1_sided=1, dinf2_scaled_l=2)
NORM_ROW = 136
SCALED_ROW = 130                                           # the row of A (and its bounds) that the two dinf2_scaled QPs scale by 100


def batch_qp(base, name):
    import exit_cases as EC
    n = base["n"]
    if name in ("feas0", "feas1"):
        return EC.take(base, [BASE_OF[name]])
    if name in ("pinf0", "pinf1"):
        return pinf_qp(base, BASE_OF[name])
    if name == "pinf0_gap":
        return pinf_qp(base, 0, gap=0.05)
    if name == "pinf2_sided":                               # the core - the row and the boxes of its columns - keeps both bounds
        pr = pinf_qp(base, 2)
        cols, _ = EC._a_row(pr, 0, n)
        return pinf_qp(base, 2, one_sided=_sided_rows(pr, [n] + [int(c) for c in cols], 60, 1))
    if name == "pinf2_norm":                                # row 136 times 0.01, l alone: its delta_y, 100 x as large, is positive
        return pinf_qp(base, 2, row_scale=[(NORM_ROW, 0.01)], one_sided=[(NORM_ROW, "l")])  # for the checks 12 .. 28 and projected away
    if name == "dinf0_weak":
        return dinf_qp(base, 0, push=0.01)
    if name == "dinf1_sided":                               # (rows that hold column 0 are free already)
        pr = dinf_qp(base, 1, push=0.01)
        return dinf_qp(base, 1, push=0.01, one_sided=_sided_rows(pr, [], 80, 2))
    if name in ("dinf2_scaled_u", "dinf2_scaled_l"):         # the scaled row keeps u alone; its mirror image keeps l alone
        return dinf_qp(base, 2, push=0.1, row_scale=[(SCALED_ROW, 100.0 if name[-1] == "u" else -100.0)], col_scale=[(5, 30.0)],
                       one_sided=[(SCALED_ROW, name[-1])])
    raise KeyError(name)


FIXED = dict(adaptive_rho=0)
# settings of the groups: every group runs the whole batch.  The tolerances come from the reference's own clause values at
# consecutive checks (the geometric mean of the two values a clause takes before and at its exit; tests/test_term_refs.py asserts
# what each group is for from the ledger)
GROUPS = {
    "s10_a": dict(FIXED, check_termination=5, eps_prim_inf=0.35, eps_dual_inf=2e-5, max_iter=400),
    "s10_b": dict(FIXED, check_termination=10, eps_prim_inf=0.179, eps_dual_inf=6.89e-5, eps_abs=2e-4, eps_rel=2e-4),
    "s10_c": dict(FIXED, check_termination=10, eps_prim_inf=0.0751, eps_dual_inf=0.00908),
    "s10_d": dict(FIXED, check_termination=10, eps_prim_inf=0.0751, eps_dual_inf=6.89e-5, rho=10.0, max_iter=400),
    "s0": dict(FIXED, scaling=0, check_termination=10, eps_prim_inf=0.332, eps_dual_inf=0.00907),
    "st": dict(FIXED, scaled_termination=1, check_termination=10, eps_prim_inf=0.182, eps_dual_inf=1.36e-5, eps_abs=2e-4, eps_rel=2e-4),
    "close_on": dict(FIXED, check_termination=10, max_iter=10, eps_prim_inf=0.179, eps_dual_inf=6.89e-5, eps_abs=2e-4, eps_rel=2e-4),
    "close_off": dict(FIXED, check_termination=10, max_iter=17, eps_prim_inf=0.179, eps_dual_inf=6.89e-5, eps_abs=2e-4, eps_rel=2e-4),
    "rho": dict(check_termination=10, adaptive_rho_interval=20, eps_prim_inf=1e-3, eps_dual_inf=1e-8),
    "ct0": dict(FIXED, check_termination=0, max_iter=60, eps_prim_inf=0.02, eps_dual_inf=1e-5),
}
AGAIN = "s10_a"                                            # the group that solves again: unchanged, then with feasible bounds

_CASES = {}


def n1m2_pinf(B=5):
    """n = 1, m = 2 (admm_refs.n1_m2's layout): a_1 x in [1, 2] and a_2 x in [-2, -1] with a_1, a_2 > 0 - no x does both"""
    pr = AF.n1_m2(B)
    pr["l"], pr["u"] = np.tile([1.0, -2.0], (B, 1)), np.tile([2.0, -1.0], (B, 1))
    return pr


def m0_dinf(B=5, k=2):
    """n = 4, m = 0, P diagonal with P_kk = 0 (an explicit zero) and q_k != 0: unbounded along -sign(q_k) e_k"""
    import scipy.sparse as sp
    rng = np.random.default_rng(40)                        # (the values of test_gpu_ops.tiny_qp(B, 4, 0))
    pr = dict(n=4, m=0, P=sp.csc_matrix(np.eye(4)), A=sp.csc_matrix(np.ones((0, 4))), Px=rng.uniform(1, 2, (B, 4)),
              Ax=rng.uniform(0.5, 1.5, (B, 0)), q=rng.standard_normal((B, 4)), l=-np.ones((B, 0)), u=np.ones((B, 0)))
    pr["Px"][:, k] = 0.0
    pr["q"][:, k] = np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * (0.5 + np.arange(B))
    return pr


def cases():
    """{name: TCase}: every run of the GPU tests (built once)"""
    if _CASES:
        return _CASES
    base = _base()
    prs = [batch_qp(base, n_) for n_ in BATCH]
    main = stack(prs)
    feasible = (np.stack([base["l"][BASE_OF[n_]] for n_ in BATCH]), np.stack([base["u"][BASE_OF[n_]] for n_ in BATCH]))
    for g, st in GROUPS.items():
        solves = ("solve", "solve", ("bounds",) + feasible, "solve") if g == AGAIN else ("solve",)
        _CASES[g] = TCase(g, main, st, solves)
    for s in (10, 0):
        _CASES[f"n1m2_s{s}"] = TCase(f"n1m2_s{s}", n1m2_pinf(), dict(FIXED, scaling=s, check_termination=5))
        _CASES[f"m0_s{s}"] = TCase(f"m0_s{s}", m0_dinf(), dict(FIXED, scaling=s, check_termination=5))
    return _CASES


_REF = {}


def reference(case, b, D, E, c):
    """the long-double results of QP b of a case with the scaling (D, E, c), computed once per scaling"""
    key = (case.name, b, np.asarray(D).tobytes(), np.asarray(E).tobytes(), float(c))
    if key not in _REF:
        _REF[key] = case.run(b, D, E, c)
    return _REF[key]


def res_errors(got, ref):
    """{quantity: error in admm_refs' term scales} of what a solve published against the reference (x, y, obj_val only with a solution)"""
    keys = ("pri_res", "dua_res") + (("obj_val", "x", "y") if ref["cert"] is None else ())
    return AF.errors(got, ref, keys=keys)


def cert_error(v, ref):
    return float(np.max(np.abs(np.asarray(v, R.LD) - ref["cert"]))) if ref["cert"].size else 0.0


def measure_twins(case):
    """(worst ratio distance, {quantity: worst error}, worst certificate error) of the two fp64 twins against the reference over
    the case's QPs and solves, with the oracle's scaling and elimination order; status, iter and rho_updates must agree"""
    clause, res, cert = 0.0, {k: 0.0 for k in RES_KEYS}, 0.0
    for b in range(case.B):
        o = case.oracle(b)
        D, E, c = o.scaling()
        perm = o.factor()[0]
        ref = reference(case, b, D, E, c)
        for t in ((0, AF.TAIL) if len(perm) > AF.TAIL else (0,)):
            twin = case.run(b, D, E, c, kind="f64", perm=perm, tail=t)
            for tw, r in zip(twin, ref):
                assert (tw["status"], tw["iter"], tw["rho_updates"]) == (r["status"], r["iter"], r["rho_updates"]), (case.name, b, t)
                for et, er in zip(tw["ledger"], r["ledger"]):
                    for cl, v in er["ratio"].items():
                        clause = max(clause, ratio_distance(et["ratio"][cl], v))
                for k, e in res_errors(tw, r).items():
                    res[k] = max(res[k], e)
                if r["cert"] is not None:
                    cert = max(cert, cert_error(tw["cert"], r))
    return clause, res, cert


def judge(case, got, ref):
    """(worst error / bound, its key) of what a solve published - dict(pri_res, dua_res, obj_val, x, y, cert) - against the reference"""
    worst, where = 0.0, None
    errs = res_errors(got, ref)
    if ref["cert"] is not None and "cert" in got:              # (the oracle has a certificate for its first solves only)
        errs["cert"] = cert_error(got["cert"], ref)
    for k, e in errs.items():
        b = CERT_BOUND[case.name] if k == "cert" else RES_BOUND[case.name][k]
        r = (0.0 if e == 0.0 else float("inf")) if b == 0.0 else e / b
        if r >= worst:
            worst, where = r, k
    return worst, where


MUTATION_GROUPS = ("s10_a", "s10_b", "s10_c", "s0", "close_on", "ct0")


def mutation_effects(mutation, groups=MUTATION_GROUPS):
    """[(case, QP, solve, "exit" | "cert", size)]: where the plain fp64 twin with the defect leaves the reference's (status, iter)
    or moves a certificate by size >= 100 certificate bounds, with the oracle's scaling and elimination order"""
    out = []
    for g in groups:
        case = cases()[g]
        for b in range(case.B):
            o = case.oracle(b)
            D, E, c = o.scaling()
            ref = reference(case, b, D, E, c)
            bad = case.run(b, D, E, c, kind="f64", perm=o.factor()[0], mutation=mutation)
            for k, (m_, r) in enumerate(zip(bad, ref)):
                if (m_["status"], m_["iter"]) != (r["status"], r["iter"]):
                    out.append((g, b, k, "exit", (r["status"], r["iter"], m_["status"], m_["iter"])))
                    break                                                   # (later solves start from another state)
                if r["cert"] is not None:
                    size = cert_error(m_["cert"], r) / CERT_BOUND[g]
                    if size >= 100:
                        out.append((g, b, k, "cert", size))
    return out
