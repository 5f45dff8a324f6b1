"""References for the device refactorisation (factor_kernel, tail_assemble_kernel, tail_kernel), seen through one observable:
the KKT solve K sol = rhs of a handle (a helper module of the tests, not a conftest; no GPU import).

K = [[Ps + sigma I, As'], [As, -diag(1 / rho_vec)]] is built from the raw data, a scaling (D, E, c) and the rho of the QP
(op_refs.scaled_qp, rho_vec, kkt_matrix).  THE REFERENCE is admm_refs.refined_solver(K, "ld"): long double, refined to 2^-60;
REF_ERROR pins it against the same refinement in mpmath on a small QP.

Right-hand sides of a case with a dense tail of k rows (rhs_set): one Gaussian vector per QP and one unit vector per 16-row
tile column of the tail, k / 16 of them (32 at k = 512), each on a natural index that the elimination order puts into that
tile column of the last k rows.  A right-hand side supported on a tail row returns a column of S^-1, so every 64 x 64 product
task and every 16 x 16 tile of S^-1 is the dominant term of at least one output.  k = 0: the Gaussian vector and 8 unit
vectors on the last eliminated rows.

Measures, separately over the x part (the first n entries) and the y part of the solution:
  err_x, err_y   max|sol - ref| / max|ref| over that part (a part whose reference is 0 exactly: / max|ref| over both)
  bwd_x, bwd_y   max|rhs - K sol| over the rows of that part / (|K|_inf |sol|_inf + |rhs|_inf), in long double: the rows of
                 op_refs.backward_error (whose value is the larger of the two; tests/test_factor_refs.py asserts that)

Three fp64 TWINS stand for "a correct fp64 implementation" and are the only source of the tolerance:
  ldl     admm_refs.ldl_solver(K, perm, 0)
  tail    admm_refs.ldl_solver(K, perm, k): S inverted by numpy.linalg.inv
  sweep   the leading factor of `tail`; S assembled as the KKT block minus sum_c L[:, c] d_c L[:, c]' and inverted by the
          unpivoted symmetric sweep on 64 x 64 pivot blocks that the comment above tail_kernel describes (sweep_inverse) -
          written from that description, not from the kernel
perm is the oracle's order on the CPU and the handle's ordering() on the GPU.  The two orders put other rows into the tail, and
the round-off of an explicit S^-1 depends on which (box pattern, 256 tail rows, rho = 1e-3: bwd_y of the twins is 8e-19 in the
oracle's order and 5e-16 in the handle's, where the host replay of the device schedule and the device itself are too).  So the
twins are measured in both: the handle's orders are recorded in tests/golden/factor_handle_orders.json, and
tests/test_gpu_factor_refs.py asserts them of every handle it judges.

FACTOR_TWIN_ERROR[case][measure]: the worst twin error over the case's QPs, the two orders and their right-hand sides
(measure_twins; with the oracle's scaling).  A case is one pattern, one tail size and ONE rho: the twins lose a factor of 30 between
rho = 0.1 and rho = 50 at k = 512 (S is worse conditioned at large rho), so a figure over all rho would hide errors at the
small ones.  FACTOR_BOUND = 32 x that - the margin of admm_refs.ITERATE_BOUND and of KKT_BWD_GPU, for the same reason: the
device sums in another order and on the matrix cores.  One figure per case and measure, never widened by hand."""
import numpy as np

import admm_refs as AF
import op_refs as R

MEASURES = ("err_x", "err_y", "bwd_x", "bwd_y")
SIGMA = 1e-6
RHO0 = 0.1                                                 # the default rho: what a handle holds after setup
RHOS = (1e-3, 0.1, 1.0, 50.0)                              # update_rho_each of the N = 640 batch, QP b gets RHOS[b]
RHO_SOME = ((1, 50.0), (2, 1e-3))                          # then update_rho_some: two QPs with unlisted neighbours
BOX = dict(n=256, mg=128, nnz_per_row=6)                   # N = 640: holds every tail up to 512 rows
BOX_B = 4
TAILS = (0, 64, 128, 192, 256, 320, 384, 448, 512)
CLASS_TAILS = (128, 320, 512)                              # one per size class: staged once; in halves; tail_kernel<4, 4>
OTHER_SEED = 7000                                          # the values update_P_A_bounds_device brings in
INERTIA_QP = 2
INERTIA_RHO = (10.0, 1e-3)                                 # K keeps inertia (n, m) at the first and loses it at the second
INERTIA_LOWERED = 4                                        # variables of the tail whose diagonal entry of P is lowered
SMALL = dict(n=96, mg=64, nnz_per_row=6)                   # N = 256: the packed work lists
SMALL_TAILS = (0, 64)
# The QPs of the packed case the twins are measured on: the sample tests/test_gpu_factor_refs.py checks at 256 CUs
# (B = 1025: first tile, a middle tile, the last full tile, the lone last QP), each at every rho of the cycle.
PACKED_QPS = (0, 1, 2, 3, 512, 513, 514, 515, 1020, 1021, 1022, 1023, 1024)
# The smallest horizon of the 6-joint GOMP pattern whose analysis accepts forced tails of 192 and 320 rows (found with
# debug_host_kkt_solve: W = 8, N = 408; 3 joints accept 320 from W = 14 on, N = 366, and 192 at every W >= 8).
GOMP = dict(dims=6, waypoints=8)
GOMP_B = 3
GOMP_TAILS = (192, 320)
GOMP_RHO_EACH = (1e-3, 1.0, 50.0)
REF_ERROR = 2.3e-19        # measured 1.79e-19: err_x, err_y of the reference against mpmath, n = 12, m = 20, every rho of RHOS

# Worst error of the fp64 twins against the long-double reference per case (pattern, tail rows, rho) and measure, the measured
# value above each row in the order err_x, err_y, bwd_x, bwd_y (tests/test_factor_refs.py measures every row again and asserts
# measured <= constant <= 2 x measured).  The GOMP pattern has free rows (1 / rho_vec = 1e6) and equality rows: cond(K) is
# about 1e10 there, and the x part of a correct fp64 solve is no better than 1e-10 .. 1e-6; its y part and both residuals
# stay as sharp as on the box pattern.
FACTOR_TWIN_ERROR = {
    # measured 1.23e-15, 7.06e-16, 3.19e-19, 3.4e-19
    'box_k0_rho0.001': dict(err_x=1.7e-15, err_y=9.9e-16, bwd_x=4.5e-19, bwd_y=4.8e-19),
    # measured 1.01e-15, 8.92e-16, 4.37e-17, 1.85e-17
    'box_k0_rho0.1': dict(err_x=1.4e-15, err_y=1.2e-15, bwd_x=6.1e-17, bwd_y=2.6e-17),
    # measured 9.14e-16, 8.82e-16, 1.81e-16, 2.81e-17
    'box_k0_rho1': dict(err_x=1.3e-15, err_y=1.2e-15, bwd_x=2.5e-16, bwd_y=3.9e-17),
    # measured 1.04e-15, 1.38e-15, 4.21e-16, 1.07e-18
    'box_k0_rho50': dict(err_x=1.5e-15, err_y=1.9e-15, bwd_x=5.9e-16, bwd_y=1.5e-18),
    # measured 6.41e-16, 6.73e-16, 3.36e-19, 3.76e-19
    'box_k64_rho0.001': dict(err_x=9.0e-16, err_y=9.4e-16, bwd_x=4.7e-19, bwd_y=5.3e-19),
    # measured 8.31e-16, 9.64e-16, 3.93e-17, 2.61e-17
    'box_k64_rho0.1': dict(err_x=1.2e-15, err_y=1.4e-15, bwd_x=5.5e-17, bwd_y=3.7e-17),
    # measured 9.12e-16, 8.84e-16, 2.35e-16, 3.45e-17
    'box_k64_rho1': dict(err_x=1.3e-15, err_y=1.2e-15, bwd_x=3.3e-16, bwd_y=4.8e-17),
    # measured 1.26e-15, 1.52e-15, 3.54e-16, 1.29e-18
    'box_k64_rho50': dict(err_x=1.8e-15, err_y=2.1e-15, bwd_x=5.0e-16, bwd_y=1.8e-18),
    # measured 1.07e-15, 1.23e-15, 4.75e-19, 3.59e-19
    'box_k128_rho0.001': dict(err_x=1.5e-15, err_y=1.7e-15, bwd_x=6.6e-19, bwd_y=5.0e-19),
    # measured 1.18e-15, 1.1e-15, 4.83e-17, 2.41e-17
    'box_k128_rho0.1': dict(err_x=1.6e-15, err_y=1.5e-15, bwd_x=6.8e-17, bwd_y=3.4e-17),
    # measured 1.13e-15, 1.14e-15, 3.59e-16, 4.22e-17
    'box_k128_rho1': dict(err_x=1.6e-15, err_y=1.6e-15, bwd_x=5.0e-16, bwd_y=5.9e-17),
    # measured 1.23e-15, 1.38e-15, 3.93e-16, 1.33e-18
    'box_k128_rho50': dict(err_x=1.7e-15, err_y=1.9e-15, bwd_x=5.5e-16, bwd_y=1.9e-18),
    # measured 1.04e-15, 1.31e-15, 4.59e-19, 6.88e-19
    'box_k192_rho0.001': dict(err_x=1.5e-15, err_y=1.8e-15, bwd_x=6.4e-19, bwd_y=9.6e-19),
    # measured 9.3e-16, 9.49e-16, 4.68e-17, 6.12e-17
    'box_k192_rho0.1': dict(err_x=1.3e-15, err_y=1.3e-15, bwd_x=6.6e-17, bwd_y=8.6e-17),
    # measured 1.17e-15, 1.16e-15, 3.9e-16, 8.32e-17
    'box_k192_rho1': dict(err_x=1.6e-15, err_y=1.6e-15, bwd_x=5.5e-16, bwd_y=1.2e-16),
    # measured 4.92e-15, 6.16e-15, 2.39e-15, 3.12e-17
    'box_k192_rho50': dict(err_x=6.9e-15, err_y=8.6e-15, bwd_x=3.3e-15, bwd_y=4.4e-17),
    # measured 1.17e-15, 1.58e-14, 5.67e-19, 2.71e-16
    'box_k256_rho0.001': dict(err_x=1.6e-15, err_y=2.2e-14, bwd_x=7.9e-19, bwd_y=3.8e-16),
    # measured 9.66e-16, 8.92e-16, 4.53e-17, 7.9e-17
    'box_k256_rho0.1': dict(err_x=1.4e-15, err_y=1.2e-15, bwd_x=6.3e-17, bwd_y=1.1e-16),
    # measured 1.58e-15, 1.7e-15, 4.53e-16, 2.37e-16
    'box_k256_rho1': dict(err_x=2.2e-15, err_y=2.4e-15, bwd_x=6.3e-16, bwd_y=3.3e-16),
    # measured 1.44e-14, 3.02e-14, 6.6e-15, 1.03e-16
    'box_k256_rho50': dict(err_x=2.0e-14, err_y=4.2e-14, bwd_x=9.2e-15, bwd_y=1.4e-16),
    # measured 1.46e-15, 8.21e-15, 4.18e-19, 1.48e-16
    'box_k320_rho0.001': dict(err_x=2.0e-15, err_y=1.1e-14, bwd_x=5.9e-19, bwd_y=2.1e-16),
    # measured 1.41e-15, 1.21e-15, 4.82e-17, 1.37e-16
    'box_k320_rho0.1': dict(err_x=2.0e-15, err_y=1.7e-15, bwd_x=6.7e-17, bwd_y=1.9e-16),
    # measured 1.84e-15, 1.5e-15, 3.62e-16, 2.19e-16
    'box_k320_rho1': dict(err_x=2.6e-15, err_y=2.1e-15, bwd_x=5.1e-16, bwd_y=3.1e-16),
    # measured 2.35e-14, 3.54e-14, 1.27e-14, 2.7e-16
    'box_k320_rho50': dict(err_x=3.3e-14, err_y=5.0e-14, bwd_x=1.8e-14, bwd_y=3.8e-16),
    # measured 3.51e-14, 3.04e-14, 1.26e-17, 2.25e-16
    'box_k384_rho0.001': dict(err_x=4.9e-14, err_y=4.3e-14, bwd_x=1.8e-17, bwd_y=3.2e-16),
    # measured 1.28e-15, 1.03e-15, 5.05e-17, 1.8e-16
    'box_k384_rho0.1': dict(err_x=1.8e-15, err_y=1.4e-15, bwd_x=7.1e-17, bwd_y=2.5e-16),
    # measured 1.98e-15, 1.33e-15, 3.8e-16, 2.24e-16
    'box_k384_rho1': dict(err_x=2.8e-15, err_y=1.9e-15, bwd_x=5.3e-16, bwd_y=3.1e-16),
    # measured 5.45e-14, 8.03e-14, 1.22e-14, 2.61e-16
    'box_k384_rho50': dict(err_x=7.6e-14, err_y=1.1e-13, bwd_x=1.7e-14, bwd_y=3.7e-16),
    # measured 1.45e-15, 2.63e-15, 5.13e-19, 1.08e-16
    'box_k448_rho0.001': dict(err_x=2.0e-15, err_y=3.7e-15, bwd_x=7.2e-19, bwd_y=1.5e-16),
    # measured 1.27e-15, 1.14e-15, 4.88e-17, 1.07e-16
    'box_k448_rho0.1': dict(err_x=1.8e-15, err_y=1.6e-15, bwd_x=6.8e-17, bwd_y=1.5e-16),
    # measured 2.58e-15, 1.94e-15, 5.73e-16, 3.02e-16
    'box_k448_rho1': dict(err_x=3.6e-15, err_y=2.7e-15, bwd_x=8.0e-16, bwd_y=4.2e-16),
    # measured 7.35e-14, 8.03e-14, 1.3e-14, 1.63e-16
    'box_k448_rho50': dict(err_x=1.0e-13, err_y=1.1e-13, bwd_x=1.8e-14, bwd_y=2.3e-16),
    # measured 1.3e-15, 1.3e-14, 5.67e-19, 2.71e-16
    'box_k512_rho0.001': dict(err_x=1.8e-15, err_y=1.8e-14, bwd_x=7.9e-19, bwd_y=3.8e-16),
    # measured 1.63e-15, 1.08e-15, 6.23e-17, 1.01e-16
    'box_k512_rho0.1': dict(err_x=2.3e-15, err_y=1.5e-15, bwd_x=8.7e-17, bwd_y=1.4e-16),
    # measured 1.96e-15, 3.57e-15, 4.71e-16, 5.33e-16
    'box_k512_rho1': dict(err_x=2.7e-15, err_y=5.0e-15, bwd_x=6.6e-16, bwd_y=7.5e-16),
    # measured 8.78e-14, 1.03e-13, 2.44e-14, 3.13e-16
    'box_k512_rho50': dict(err_x=1.2e-13, err_y=1.4e-13, bwd_x=3.4e-14, bwd_y=4.4e-16),
    # measured 1.41e-15, 1.77e-15, 5.35e-16, 6.8e-18
    'box_k128_rho10': dict(err_x=2.0e-15, err_y=2.5e-15, bwd_x=7.5e-16, bwd_y=9.5e-18),
    # measured 4.77e-15, 5.69e-15, 1.91e-15, 2.1e-16
    'box_k320_rho10': dict(err_x=6.7e-15, err_y=8.0e-15, bwd_x=2.7e-15, bwd_y=2.9e-16),
    # measured 2.83e-14, 3.81e-14, 5.38e-15, 2.81e-16
    'box_k512_rho10': dict(err_x=4.0e-14, err_y=5.3e-14, bwd_x=7.5e-15, bwd_y=3.9e-16),
    # measured 4.34e-11, 1.94e-14, 8.62e-21, 4.34e-17
    'gomp_k192_rho0.001': dict(err_x=6.1e-11, err_y=2.7e-14, bwd_x=1.2e-20, bwd_y=6.1e-17),
    # measured 2.54e-09, 4.93e-12, 6.51e-18, 1.88e-16
    'gomp_k192_rho0.1': dict(err_x=3.6e-09, err_y=6.9e-12, bwd_x=9.1e-18, bwd_y=2.6e-16),
    # measured 1.66e-10, 1.04e-13, 9.98e-20, 7.56e-17
    'gomp_k192_rho1': dict(err_x=2.3e-10, err_y=1.5e-13, bwd_x=1.4e-19, bwd_y=1.1e-16),
    # measured 2.05e-10, 1.09e-13, 1.35e-19, 1.9e-18
    'gomp_k192_rho50': dict(err_x=2.9e-10, err_y=1.5e-13, bwd_x=1.9e-19, bwd_y=2.7e-18),
    # measured 4.06e-11, 1.75e-14, 2.48e-20, 4.06e-17
    'gomp_k320_rho0.001': dict(err_x=5.7e-11, err_y=2.5e-14, bwd_x=3.5e-20, bwd_y=5.7e-17),
    # measured 1.64e-09, 3.68e-14, 3.14e-20, 6.41e-17
    'gomp_k320_rho0.1': dict(err_x=2.3e-09, err_y=5.2e-14, bwd_x=4.4e-20, bwd_y=9.0e-17),
    # measured 1.2e-08, 4.85e-14, 4.87e-20, 4.68e-17
    'gomp_k320_rho1': dict(err_x=1.7e-08, err_y=6.8e-14, bwd_x=6.8e-20, bwd_y=6.6e-17),
    # measured 6.14e-07, 1.2e-13, 1.2e-19, 4.78e-17
    'gomp_k320_rho50': dict(err_x=8.6e-07, err_y=1.7e-13, bwd_x=1.7e-19, bwd_y=6.7e-17),
    # measured 7.5e-16, 9.84e-16, 3.21e-19, 3.69e-19
    'small_k0_rho0.001': dict(err_x=1.0e-15, err_y=1.4e-15, bwd_x=4.5e-19, bwd_y=5.2e-19),
    # measured 5.94e-16, 5.67e-16, 2.64e-17, 2.9e-17
    'small_k0_rho0.1': dict(err_x=8.3e-16, err_y=7.9e-16, bwd_x=3.7e-17, bwd_y=4.1e-17),
    # measured 1.09e-15, 1.15e-15, 2.74e-16, 3.49e-17
    'small_k0_rho1': dict(err_x=1.5e-15, err_y=1.6e-15, bwd_x=3.8e-16, bwd_y=4.9e-17),
    # measured 7.44e-16, 8.87e-16, 3.01e-16, 1.09e-18
    'small_k0_rho50': dict(err_x=1.0e-15, err_y=1.2e-15, bwd_x=4.2e-16, bwd_y=1.5e-18),
    # measured 8.9e-16, 1.07e-15, 4.41e-19, 4.39e-19
    'small_k64_rho0.001': dict(err_x=1.2e-15, err_y=1.5e-15, bwd_x=6.2e-19, bwd_y=6.2e-19),
    # measured 1.3e-15, 1.18e-15, 5.78e-17, 2.59e-17
    'small_k64_rho0.1': dict(err_x=1.8e-15, err_y=1.7e-15, bwd_x=8.1e-17, bwd_y=3.6e-17),
    # measured 1.23e-15, 1.11e-15, 3.28e-16, 4.02e-17
    'small_k64_rho1': dict(err_x=1.7e-15, err_y=1.6e-15, bwd_x=4.6e-16, bwd_y=5.6e-17),
    # measured 1.65e-15, 1.74e-15, 3.84e-16, 8.59e-19
    'small_k64_rho50': dict(err_x=2.3e-15, err_y=2.4e-15, bwd_x=5.4e-16, bwd_y=1.2e-18),
}

FACTOR_BOUND = {name: {k: 32 * v for k, v in row.items()} for name, row in FACTOR_TWIN_ERROR.items()}


# ------------------------------------------------------------------ the system of one QP at one rho
class System:
    """K of one QP (raw data, scaling, rho) with its reference solves; stale = (row, rho): that row of rho_vec is the one
    of another rho (a deliberate defect - such a System is only ever the source of a twin)"""

    def __init__(self, P, A, l, u, D, E, c, rho, sigma=SIGMA, stale=None):
        Ps, As, _, ls, us = R.scaled_qp(P, A, None, l, u, D, E, c)
        self.n, self.m = As.shape[1], As.shape[0]
        self.rho_vec = R.rho_vec(ls, us, rho)
        if stale is not None:
            self.rho_vec[stale[0]] = R.rho_vec(ls, us, stale[1])[stale[0]]
        self.Ps, self.As = Ps, As
        self.K = R.kkt_matrix(Ps, As, sigma, self.rho_vec)
        self.norm = self.K.norm_inf()
        self._Kd, self._solve, self._refs = None, None, {}

    @property
    def Kd(self):
        if self._Kd is None:
            self._Kd = AF._dense(self.K)
        return self._Kd

    def K64(self):
        return self.Kd.astype(np.float64)

    def residuals(self, sol, rhs):
        """bwd_x and bwd_y alone: they need K and no reference solve"""
        n = self.n
        sol, rhs = np.asarray(sol, R.LD), np.asarray(rhs, R.LD)
        res = np.abs(rhs - self.K.matvec(sol)[0])
        den = self.norm * np.max(np.abs(sol)) + np.max(np.abs(rhs))
        return dict(bwd_x=float(np.max(res[:n], initial=R.LD(0)) / den), bwd_y=float(np.max(res[n:], initial=R.LD(0)) / den))

    def ref(self, rhs):
        """K^-1 rhs in long double (raises when the refinement does not converge); computed once per right-hand side"""
        key = np.asarray(rhs, np.float64).tobytes()
        if key not in self._refs:
            if self._solve is None:
                self._solve = AF.refined_solver(self.Kd, "ld")
            self._refs[key] = self._solve(np.asarray(rhs, R.LD))
        return self._refs[key]

    def measures(self, sol, rhs):
        n = self.n
        sol, ref = np.asarray(sol, R.LD), self.ref(rhs)
        d = np.abs(sol - ref)
        part = lambda v, lo, hi: np.max(v[lo:hi], initial=R.LD(0))
        N = n + self.m
        whole = part(np.abs(ref), 0, N)                      # (a part that is 0 exactly - a unit vector on an empty row of A - is
        sx, sy = part(np.abs(ref), 0, n), part(np.abs(ref), n, N)       #  measured in the scale of the whole solution)
        out = dict(self.residuals(sol, rhs), err_x=part(d, 0, n) / (sx if sx > 0 else whole),
                   err_y=part(d, n, N) / (sy if sy > 0 else whole) if self.m else R.LD(0))
        return {k: float(out[k]) for k in MEASURES}


def rhs_set(perm, k, seed):
    """([1 + max(k / 16, 8), N] right-hand sides, their labels) - module docstring"""
    perm = np.asarray(perm)
    N = len(perm)
    assert k % 16 == 0 and k <= min(N, 512)
    at = [perm[N - k + 16 * t + (5 * t + 3) % 16] for t in range(k // 16)] if k else list(perm[N - 8:])
    out = np.zeros((1 + len(at), N))
    out[0] = np.random.default_rng(seed).standard_normal(N)
    for j, i in enumerate(at):
        out[1 + j, i] = 1.0
    return out, ["gauss"] + [f"e{int(i)}" for i in at]


# ------------------------------------------------------------------ the third twin
def sweep_inverse(S, block=64, unsym=None):
    """S^-1 by the symmetric sweep operator on pivot blocks, unpivoted, in fp64.  Per pivot block p:
        Pn = -inv(A_pp);  Gn = A_:p Pn;  A_ij += Gn_i A_pj (i, j outside p);  A_:p = -Gn;  A_pp = Pn
    and after the last block A = -inv(S).  Pn itself comes from the same operator on single pivots inside the block.  The
    lower triangle is the result (its mirror image the upper one).  unsym = T (a defect): the diagonal 16-tile T is not
    symmetrised - the strict upper triangle of that tile misses the update of the last pass."""
    A = np.array(S, dtype=np.float64)
    k = len(A)
    assert k % block == 0
    for p0 in range(0, k, block):
        p = np.arange(p0, p0 + block)
        o = np.concatenate([np.arange(0, p0), np.arange(p0 + block, k)])
        Pn = A[np.ix_(p, p)].copy()
        for j in range(block):
            g = Pn[:, j] * (-1.0 / Pn[j, j])
            pn = -1.0 / Pn[j, j]
            Pn += np.outer(g, Pn[j, :])
            Pn[:, j], Pn[j, :] = -g, -g
            Pn[j, j] = pn
        Gn = A[np.ix_(o, p)] @ Pn
        keep = None
        if unsym is not None and p0 + block == k:
            t = np.arange(16 * unsym, 16 * unsym + 16)
            assert t[-1] < p0
            keep = A[np.ix_(t, t)].copy()
        A[np.ix_(o, o)] += Gn @ A[np.ix_(p, o)]
        if keep is not None:
            up = np.triu_indices(16, 1)
            A[t[up[0]], t[up[1]]] = keep[up]
        A[np.ix_(o, p)], A[np.ix_(p, o)] = -Gn, -Gn.T
        A[np.ix_(p, p)] = Pn
    if unsym is not None:                                    # (the defective tile is delivered as it stands)
        t = np.arange(16 * unsym, 16 * unsym + 16)
        tile = -A[np.ix_(t, t)]
    out = -(np.tril(A) + np.tril(A, -1).T)
    if unsym is not None:
        out[np.ix_(t, t)] = tile
    return out


def sweep_solver(K, tail_twin, defect=None, where=None):
    """fp64: the solve of admm_refs.ldl_solver(K, perm, k) - tail_twin, whose leading factor this one shares - with S^-1 from
    sweep_inverse.  defect (tests): "tile": the 16 x 16 tile where = (I, J) of S^-1 scaled by 1 + 1e-10; "drop": the Schur
    update of source column where = c left out of S; "unsym": the diagonal 16-tile `where` unsymmetrised."""
    import scipy.linalg as sla
    perm, h, L, d = tail_twin.factor
    N = K.shape[0]
    assert h < N and defect in (None, "tile", "drop", "unsym")
    Kp = K[np.ix_(perm, perm)]
    L11, L21 = L[:h, :h], L[h:, :h]
    W = L21 * d[:h]
    if defect == "drop":
        W[:, where] = 0.0
    Sinv = sweep_inverse(Kp[h:, h:] - W @ L21.T, unsym=where if defect == "unsym" else None)
    if defect == "tile":
        I, J = where
        Sinv[16 * I:16 * I + 16, 16 * J:16 * J + 16] *= 1.0 + 1e-10
        if I != J:
            Sinv[16 * J:16 * J + 16, 16 * I:16 * I + 16] *= 1.0 + 1e-10

    def solve(r):
        b = r[perm]
        y1 = sla.solve_triangular(L11, b[:h], lower=True, unit_diagonal=True) if h else b[:0]
        x2 = Sinv @ (b[h:] - L21 @ y1)
        t = y1 / d[:h] - L21.T @ x2
        x1 = sla.solve_triangular(L11.T, t, lower=False, unit_diagonal=True) if h else t
        out = np.empty(N)
        out[perm] = np.concatenate([x1, x2])
        return out
    solve.factor = tail_twin.factor
    return solve


def twins(system, perm, k):
    """{name: solve} of the fp64 twins of a system with a tail of k rows (k = 0: the plain LDL' alone)"""
    K = system.K64()
    out = {"ldl": AF.ldl_solver(K, perm, 0)}
    if k:
        out["tail"] = AF.ldl_solver(K, perm, k)
        out["sweep"] = sweep_solver(K, out["tail"])
    return out


# ------------------------------------------------------------------ the data of the cases
_DATA = {}


def data(name):
    """the batches of the cases, built once: box, other (the values an update brings in), small<B>, gomp"""
    if name not in _DATA:
        from osqp_solver_amd import problems as PR
        if name == "box":
            _DATA[name] = PR.random_box_qp(BOX_B, **BOX)
        elif name == "other":
            _DATA[name] = PR.random_box_qp(BOX_B, value_seed=OTHER_SEED, **BOX)
        elif name.startswith("small"):
            _DATA[name] = PR.random_box_qp(int(name[5:]), **SMALL)
        elif name == "gomp":
            _DATA[name] = PR.gomp_batch(GOMP_B, GOMP["dims"], GOMP["waypoints"])
        else:
            raise KeyError(name)
    return _DATA[name]


def qp(pr, b):
    from osqp_solver_amd import problems as PR
    P, A = PR.qp_matrices(pr, b)
    return dict(P=P, A=A, q=None if pr["q"] is None else pr["q"][b], l=pr["l"][b], u=pr["u"][b])


def system_of(pr, b, D, E, c, rho, **kw):
    d = qp(pr, b)
    return System(d["P"], d["A"], d["l"], d["u"], D, E, c, rho, **kw)


def reduced_min_eig(system):
    """the smallest eigenvalue of Ps + sigma I + As' diag(rho_vec) As: K has inertia (n, m) exactly when it is positive"""
    n = system.n
    K = system.K64()
    As = K[n:, :n]
    return float(np.linalg.eigvalsh(K[:n, :n] + As.T @ (system.rho_vec[:, None] * As))[0])


def lowered(pr, b, variables, amount):
    """pr with the diagonal of QP b's P lowered by `amount` on `variables`"""
    Pp = pr["P"]
    cols = np.repeat(np.arange(Pp.shape[1]), np.diff(Pp.indptr))
    hit = (Pp.indices == cols) & np.isin(cols, variables)
    assert hit.sum() == len(variables)
    Px = pr["Px"].copy()
    Px[b, hit] -= amount
    return dict(pr, Px=Px)


_INERTIA = {}


def inertia_batch(perm, k):
    key = (np.asarray(perm, np.int64).tobytes(), k)
    if key not in _INERTIA:
        _INERTIA[key] = _inertia_batch(perm, k)
    return _INERTIA[key]


def _inertia_batch(perm, k):
    """(the N = 640 batch in which QP INERTIA_QP has the diagonal of P lowered on INERTIA_LOWERED variables of the last k rows
    of the order perm, those variables, the amount).  The amount is the smallest of 1.5, 2, 3, 4, 6 for which - with the
    oracle's scaling of that QP, set up at INERTIA_RHO[0] - K keeps inertia (n, m) at INERTIA_RHO[0] and loses it at
    INERTIA_RHO[1], each with a margin of 1e-2 in the smallest eigenvalue of the reduced matrix (a handle's scaling agrees
    with the oracle's to 1e-13; tests/test_gpu_factor_refs.py verifies both signs again with the handle's own)."""
    pr = data("box")
    n = pr["n"]
    variables = [int(i) for i in perm[len(perm) - k:] if i < n][:INERTIA_LOWERED]
    assert len(variables) == INERTIA_LOWERED, variables
    for amount in (1.5, 2.0, 3.0, 4.0, 6.0):
        bad = lowered(pr, INERTIA_QP, variables, amount)
        try:
            (D, E, c), _ = oracle_scaling_and_order(bad, INERTIA_QP, INERTIA_RHO[0])
        except ValueError:                                   # (the oracle refuses a K without its inertia at setup)
            continue
        keeps = reduced_min_eig(system_of(bad, INERTIA_QP, D, E, c, INERTIA_RHO[0]))
        loses = reduced_min_eig(system_of(bad, INERTIA_QP, D, E, c, INERTIA_RHO[1]))
        if keeps >= 1e-2 and loses <= -1e-2:
            return bad, variables, amount
    raise AssertionError("no amount keeps the inertia at the first rho and loses it at the second")


# ------------------------------------------------------------------ the cases and the twins' errors
def case_name(pattern, k, rho):
    return f"{pattern}_k{k}_rho{rho:g}"


def case_list():
    """[(name, pattern, k, rho)] of every case that has a bound"""
    out = [(case_name("box", k, rho), "box", k, rho) for k in TAILS for rho in RHOS]
    out += [(case_name("box", k, INERTIA_RHO[0]), "box", k, INERTIA_RHO[0]) for k in CLASS_TAILS]
    out += [(case_name("gomp", k, rho), "gomp", k, rho) for k in GOMP_TAILS for rho in sorted({RHO0, *GOMP_RHO_EACH})]
    out += [(case_name("small", k, rho), "small", k, rho) for k in SMALL_TAILS for rho in RHOS]
    return out


def oracle_of(pr, b, rho=RHO0):
    from oracle import oracle as O
    d = qp(pr, b)
    return O.OracleQPSolver(d["P"], d["q"], d["A"], d["l"], d["u"], rho=rho)


_ORACLE = {}
_HANDLE_ORDERS = {}


def handle_order(pattern, k):
    """the recorded BatchSolver.ordering() of a pattern at a forced tail of k rows (tests/golden/factor_handle_orders.json)"""
    if not _HANDLE_ORDERS:
        import json
        import os
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factor_handle_orders.json")) as f:
            _HANDLE_ORDERS.update({key: np.asarray(v, np.int64) for key, v in json.load(f).items() if key != "about"})
    return _HANDLE_ORDERS[f"gomp_k{k}" if pattern == "gomp" else pattern]


def orders(pattern, k):
    """{"oracle" | "handle": elimination order} of a case"""
    pr = data({"box": "box", "gomp": "gomp", "small": f"small{max(PACKED_QPS) + 1}"}[pattern])
    return dict(oracle=oracle_scaling_and_order(pr, 0)[1], handle=handle_order(pattern, k))


def oracle_scaling_and_order(pr, b, rho=RHO0):
    """((D, E, c), elimination order) of the oracle set up at rho (neither depends on it), once per QP"""
    key = (id(pr["Px"]), b)
    if key not in _ORACLE:
        o = oracle_of(pr, b, rho)
        _ORACLE[key] = (pr["Px"], o.scaling(), np.asarray(o.factor()[0]))          # (pr["Px"] kept alive: its id is the key)
    return _ORACLE[key][1:]


def case_qps(pattern, k, rho, perm=None):
    """[(batch, QP)] the twins of a case are measured on: the QPs that tests/test_gpu_factor_refs.py takes to that rho (perm:
    the order that places the lowered variables of the lost-inertia batch; default: the oracle's)"""
    if pattern == "small":
        return [(data(f"small{max(PACKED_QPS) + 1}"), b) for b in PACKED_QPS]
    if pattern == "gomp":
        return [(data("gomp"), b) for b in range(GOMP_B)]
    box = data("box")
    if rho == INERTIA_RHO[0]:
        bad, _, _ = inertia_batch(oracle_scaling_and_order(box, 0)[1] if perm is None else perm, k)
        return [(bad if b == INERTIA_QP else box, b) for b in range(BOX_B)]
    out = [(box, b) for b in range(BOX_B)]
    if rho == RHO0 and k in CLASS_TAILS:
        out += [(data("other"), b) for b in range(BOX_B)]
    return out


def seed_of(k, b):
    return 1000 * k + b


_SYSTEMS = {}


def oracle_system(pr, b, rho):
    """the System of QP b at rho with the oracle's scaling, built once (its reference solves are shared by the tests)"""
    key = (id(pr["Px"]), b, rho)
    if key not in _SYSTEMS:
        (D, E, c), _ = oracle_scaling_and_order(pr, b)
        _SYSTEMS[key] = (pr["Px"], system_of(pr, b, D, E, c, rho))
    return _SYSTEMS[key][1]


def worst_of(system, solve, rhs, into=None):
    """{measure: worst over the right-hand sides} of a solver against the system's reference; merged into `into`"""
    out = dict.fromkeys(MEASURES, 0.0) if into is None else into
    for r in rhs:
        for key, v in system.measures(solve(r), r).items():
            assert np.isfinite(v), key
            out[key] = max(out[key], v)
    return out


def one_blas_thread():
    """The twins' round-off depends on how the BLAS splits a product over its threads (measured: up to 50 % in a worst error
    at N = 640).  The table is measured with one thread, so that it is the same on a machine with another core count."""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        import contextlib
        return contextlib.nullcontext()
    return threadpool_limits(limits=1)


def measure_twins(pattern, k, rho):
    """{measure: the worst error of the twins against the reference} of a case, with the oracle's scaling, in the oracle's
    order and in the handle's"""
    out = dict.fromkeys(MEASURES, 0.0)
    with one_blas_thread():
        for perm in orders(pattern, k).values():
            for pr, b in case_qps(pattern, k, rho, perm):
                system = oracle_system(pr, b, rho)
                rhs, _ = rhs_set(perm, k, seed_of(k, b))
                for solve in twins(system, perm, k).values():
                    worst_of(system, solve, rhs, out)
    return out


def ratio(measured, name):
    """(worst measure / its bound, which) of measured errors (all four, or the residuals alone) against the bound of a case"""
    out, where = 0.0, None
    for key in measured:
        r = measured[key] / FACTOR_BOUND[name][key]
        if not r < out:                                      # (a NaN counts as the worst)
            out, where = r, key
    return out, where
