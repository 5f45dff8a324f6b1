"""Plain high-precision references of the path's ops (a helper module of the tests, not a conftest).

Everything here is numpy on the host: the scaled problem of OSQP's Ruiz equilibration, the three products of the SpMV op
with their error bound, the rho vector of OSQP 0.6 and the KKT matrix with a normwise backward error.  The products and
sums run in np.longdouble (x86-64: 64-bit mantissa, 11 more bits than fp64), so that the reference is exact to far below
the rounding of the fp64 kernels it judges.  Where long double is not wider than fp64 the products are split exactly
(TwoProduct) and every row is summed with math.fsum (correctly rounded) instead."""
import math

import numpy as np

U = 2.0 ** -53                                          # unit round-off of fp64
WIDE = np.finfo(np.longdouble).nmant >= 63
LD = np.longdouble if WIDE else np.float64

# OSQP 0.6 constants, as in oracle/osqp_oracle.c
OQ_INFTY = 1e30
OQ_RHO_MIN, OQ_RHO_MAX = 1e-6, 1e6
OQ_RHO_EQ_OVER_INEQ = 1e3
OQ_RHO_TOL = 1e-4
OQ_MIN_SCALING = 1e-4


class Coo:
    """A sparse matrix as (rows, cols, vals) triplets with vals in long double.  Explicit zeros stay entries: they belong
    to the stored pattern, and the pattern decides the row lengths of the bound."""

    def __init__(self, rows, cols, vals, shape):
        self.rows, self.cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        self.vals = np.asarray(vals, LD)
        self.shape = shape

    @staticmethod
    def from_scipy(M):
        M = M.tocoo()
        return Coo(M.row, M.col, M.data.astype(LD), M.shape)

    def T(self):
        return Coo(self.cols, self.rows, self.vals, (self.shape[1], self.shape[0]))

    def row_lengths(self):
        return np.bincount(self.rows, minlength=self.shape[0])

    def norm_inf(self):
        s = np.zeros(self.shape[0], LD)
        np.add.at(s, self.rows, np.abs(self.vals))
        return s.max(initial=LD(0))

    def matvec(self, v):
        """(M v, per-row sum |m_k v_k|, row lengths) in long double."""
        v = np.zeros(self.shape[1], LD) if v is None else np.asarray(v, LD)
        if WIDE:
            prod = self.vals * v[self.cols]
            out, mag = np.zeros(self.shape[0], LD), np.zeros(self.shape[0], LD)
            np.add.at(out, self.rows, prod)
            np.add.at(mag, self.rows, np.abs(prod))
            return out, mag, self.row_lengths()
        return _matvec_fsum(self, v)


def _split(a):
    c = 134217729.0 * a                                  # Veltkamp splitting, 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_product(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _matvec_fsum(M, v):
    p, e = _two_product(M.vals.astype(np.float64), v[M.cols].astype(np.float64))
    terms = [[] for _ in range(M.shape[0])]
    for r, a, b in zip(M.rows, p, e):
        terms[r] += [a, b]
    out = np.array([math.fsum(t) for t in terms])
    mag = np.array([math.fsum(abs(x) for x in t) for t in terms])
    return out, mag, M.row_lengths()


def sym_full(P):
    """The symmetric matrix of a P that holds the upper triangle or both (the lower one is ignored, as OSQP does)."""
    P = P if isinstance(P, Coo) else Coo.from_scipy(P)
    up = P.rows <= P.cols
    r, c, v = P.rows[up], P.cols[up], P.vals[up]
    off = r < c
    return Coo(np.concatenate([r, c[off]]), np.concatenate([c, r[off]]), np.concatenate([v, v[off]]), P.shape)


def scaled_qp(P, A, q, l, u, D, E, c):
    """The problem the kernels work on: (c D P D, E A D, c D q, E l, E u) in long double, P as its full symmetric matrix.
    l and u are clipped to +-OSQP_INFTY first, as osqp_setup does."""
    Pf, A = sym_full(P), Coo.from_scipy(A)
    D, E, c = np.asarray(D, LD), np.asarray(E, LD), LD(c)
    Ps = Coo(Pf.rows, Pf.cols, c * D[Pf.rows] * Pf.vals * D[Pf.cols], Pf.shape)
    As = Coo(A.rows, A.cols, E[A.rows] * A.vals * D[A.cols], A.shape)
    qs = None if q is None else c * D * np.asarray(q, LD)
    ls = E * np.maximum(np.asarray(l, np.float64), -OQ_INFTY).astype(LD)
    us = E * np.minimum(np.asarray(u, np.float64), OQ_INFTY).astype(LD)
    return Ps, As, qs, ls, us


def spmv_ref(P, A, x, y):
    """P x, A'y and A x in long double, P symmetric (given as its upper triangle or in full), each with its per-row
    magnitude sum |a_k v_k| and its row length.  x or y None reads as zeros.  Returns {"Px" | "Aty" | "Ax": (value, mag, len)}.

    Bound of an fp64 kernel row (spmv_tol): a row of `len` stored entries is a chain of `len` fma's, each rounding once,
    so its recursive-summation error is at most len * u * sum|a_k v_k| (to first order; u = 2^-53).  With scaling on, the
    stored value a_k itself is off from the exact c D_i a D_j (or E_i a D_j) that the reference forms from the D, E, c the
    handle reports: the Ruiz kernels rescale every stored value in place once per factor and iteration - P by D_i, D_j and
    c (3 roundings), A by E_i and D_j (2) - while D, E and c are themselves running products rounded once per iteration
    after the first; together at most 6 * iters roundings per value (P; A: 4 * iters - 2), i.e. 6 * iters * u relative.
    The +4 covers the second-order terms, the exactness of the long-double reference and the final store."""
    Pf = sym_full(P)
    A = A if isinstance(A, Coo) else Coo.from_scipy(A)
    return {"Px": Pf.matvec(x), "Aty": A.T().matvec(y), "Ax": A.matvec(x)}


def spmv_tol(mag, length, scaling_iters):
    """Per-row bound on |kernel - reference| (derivation: spmv_ref)."""
    return (np.asarray(length, np.float64) + 6.0 * scaling_iters + 4.0) * U * np.asarray(mag, np.float64)


def rho_vec(l_s, u_s, rho):
    """OSQP 0.6 set_rho_vec on the SCALED bounds: free rows get RHO_MIN, equalities (u - l < RHO_TOL) RHO_EQ_OVER_INEQ * rho,
    the others rho (itself clipped to [RHO_MIN, RHO_MAX])."""
    rho = min(max(float(rho), OQ_RHO_MIN), OQ_RHO_MAX)
    l_s, u_s = np.asarray(l_s, np.float64), np.asarray(u_s, np.float64)
    free = (l_s < -OQ_INFTY * OQ_MIN_SCALING) & (u_s > OQ_INFTY * OQ_MIN_SCALING)
    eq = ~free & (u_s - l_s < OQ_RHO_TOL)
    return np.where(free, OQ_RHO_MIN, np.where(eq, OQ_RHO_EQ_OVER_INEQ * rho, rho))


def kkt_matrix(Ps, As, sigma, rho):
    """K = [[Ps + sigma I, As'], [As, -diag(1 / rho)]] (Ps full symmetric), long double."""
    n, m = As.shape[1], As.shape[0]
    i_n, i_m = np.arange(n), np.arange(m)
    rows = np.concatenate([Ps.rows, i_n, As.cols, n + As.rows, n + i_m])
    cols = np.concatenate([Ps.cols, i_n, n + As.rows, As.cols, n + i_m])
    vals = np.concatenate([Ps.vals, np.full(n, sigma, LD), As.vals, As.vals, -LD(1) / np.asarray(rho, LD)])
    return Coo(rows, cols, vals, (n + m, n + m))


def backward_error(K, sol, rhs):
    """||rhs - K sol||_inf / (||K||_inf ||sol||_inf + ||rhs||_inf), in long double: the smallest relative change of K and
    rhs for which sol is an exact solution (Rigal-Gaches, normwise)."""
    rhs = np.asarray(rhs, LD)
    Ks, _, _ = K.matvec(np.asarray(sol, LD))
    r = np.max(np.abs(rhs - Ks), initial=LD(0))
    den = K.norm_inf() * np.max(np.abs(np.asarray(sol, LD)), initial=LD(0)) + np.max(np.abs(rhs), initial=LD(0))
    return float(r / den)
