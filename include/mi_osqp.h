/*
 * mi_osqp.h -- C-ABI of the MI355X-native OSQP ADMM core.
 *
 * This is the drop-in boundary for the solver path of ZPP-Robotics/OSQP-Solver:
 * every entry point names the reference interface it replaces ([REF] = path
 * under /root/reference, file:line).  The reference reaches its solver only
 * through class QPSolver ([REF] src/osqp-wrapper.h:12-60), whose four methods
 * wrap google/osqp-cpp calls; a maintainer binds this library there (see
 * INTEGRATION.md for the exact stub).
 *
 * Conventions
 *   - plain C, no torch / Eigen types; all arrays caller-owned and copied at
 *     the call (matches the reference: its OsqpInstance dies at the end of the
 *     constructor, [REF] src/osqp-wrapper.h:18-31);
 *   - sparse matrices are CSC with 64-bit indices = Eigen::SparseMatrix<double,
 *     ColMajor, long long> ([REF] src/utils.h:12);
 *   - +-1e30 means "unbounded" ([REF] src/constraints/constraints.h:11);
 *   - every function returns an mi_osqp_error (0 = ok) unless stated; nothing
 *     aborts and nothing falls back to a CPU solve: without a usable gfx950
 *     device setup fails with MI_OSQP_ERR_DEVICE.
 */
#ifndef MI_OSQP_H
#define MI_OSQP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  MI_OSQP_OK = 0,
  MI_OSQP_ERR_INVALID_DATA = 1,      /* dims, l>u, bad CSC      -> osqp-cpp InvalidArgument */
  MI_OSQP_ERR_INVALID_SETTINGS = 2,
  MI_OSQP_ERR_PATTERN_CHANGED = 3,   /* UpdateConstraintMatrix with a new pattern */
  MI_OSQP_ERR_NONCONVEX = 4,         /* KKT inertia wrong / zero pivot */
  MI_OSQP_ERR_DEVICE = 5,            /* HIP error or no gfx950 device */
  MI_OSQP_ERR_NULL = 6,
  MI_OSQP_ERR_ALLOC = 7
} mi_osqp_error;

/* exit codes = osqp::OsqpExitCode as consumed by the reference
 * ([REF] src/utils.h:11; src/gomp-solver.h:40,46-49,68,72,79;
 *  examples/solver-example.cpp:71,94).  Values follow the osqp-cpp enum order. */
typedef enum {
  MI_OSQP_EXIT_OPTIMAL = 0,
  MI_OSQP_EXIT_PRIMAL_INFEASIBLE = 1,
  MI_OSQP_EXIT_DUAL_INFEASIBLE = 2,
  MI_OSQP_EXIT_OPTIMAL_INACCURATE = 3,
  MI_OSQP_EXIT_PRIMAL_INFEASIBLE_INACCURATE = 4,
  MI_OSQP_EXIT_DUAL_INFEASIBLE_INACCURATE = 5,
  MI_OSQP_EXIT_MAX_ITERATIONS = 6,
  MI_OSQP_EXIT_INTERRUPTED = 7,
  MI_OSQP_EXIT_TIME_LIMIT_REACHED = 8,
  MI_OSQP_EXIT_NON_CONVEX = 9,
  MI_OSQP_EXIT_UNKNOWN = 10
} mi_osqp_exit_code;

/* OsqpSettings subset that influences the iterates.  The reference sets only
 * `verbose` ([REF] src/osqp-wrapper.h:26-27), so defaults = osqp 0.6.x defaults. */
typedef struct {
  double  rho;                    /* 0.1  */
  double  sigma;                  /* 1e-6 */
  int64_t scaling;                /* 10   */
  int64_t adaptive_rho;           /* 1    */
  int64_t adaptive_rho_interval;  /* 0 = auto -> 4*check_termination (deterministic) */
  double  adaptive_rho_tolerance; /* 5    */
  int64_t max_iter;               /* 4000 */
  double  eps_abs;                /* 1e-3 */
  double  eps_rel;                /* 1e-3 */
  double  eps_prim_inf;           /* 1e-4 */
  double  eps_dual_inf;           /* 1e-4 */
  double  alpha;                  /* 1.6  */
  int64_t scaled_termination;     /* 0    */
  int64_t check_termination;      /* 25   */
  int64_t warm_start;             /* 1    */
  int64_t verbose;                /* 0 here; the reference passes 1 (log only) */
  /* solution polishing (OSQP polish.c, README "Polishing"): after every blocking solve, each QP that ended kOptimal solves
   * the reduced KKT system of the active set guessed from its final iterate and keeps the result when its residuals are
   * smaller.  The continuous mode polishes on demand instead (mi_osqp_batch_polish_some, with polish_refine_iter and delta
   * of the handle): mi_osqp_batch_solve_begin_some refuses a handle with polish = 1. */
  int64_t polish;                 /* 0    */
  int64_t polish_refine_iter;     /* 3    (>= 0) */
  double  delta;                  /* 1e-6 (> 0): regularisation of the reduced KKT matrix */
} mi_osqp_settings;

typedef struct {
  int64_t iter;
  int64_t status_val;   /* raw osqp status (1 solved, -2 max iter, ...) */
  int64_t exit_code;    /* mi_osqp_exit_code */
  double  obj_val;
  double  pri_res;
  double  dua_res;
  int64_t rho_updates;
  double  rho_estimate;
  double  rho;
  int64_t status_polish;  /* 1 polished solution accepted, -1 polishing failed / not better, 0 not polished (polish off, or
                           * the QP did not end kOptimal) */
} mi_osqp_info;

/* analysis / schedule statistics (DESIGN.md quotes these) */
typedef struct {
  int64_t n, m, N, batch, tile, n_tiles;
  int64_t nnz_P_triu, nnz_A, nnz_KKT, nnz_L;
  int64_t n_supernodes, n_blocks;
  int64_t fwd_levels, bwd_levels, fwd_slots, bwd_slots, chk_slots;
  int64_t lds_bytes, threads_per_block;
  int64_t dense_tail_rows, dense_tail_slots;   /* trailing rows served by the inverted Schur complement (0 = none), its stream slots */
  double  setup_seconds_host, setup_seconds_factor, setup_seconds_upload;
  int64_t nnz_L_before_tail;   /* entries of L in the columns before the dense tail (= nnz_L without one): what the two sweeps stream */
  int64_t solve_groups, solve_group_threads;   /* large single QP: workgroups x threads that share its sweeps (0 = one workgroup); never more than the device keeps resident */
  int64_t resident_state, lds_bytes_iterate;   /* 1: the iterate keeps the ADMM state and D^-1 of a tile in LDS across a segment; dynamic LDS of its launches (= lds_bytes when 0) */
  int64_t pipelined_refactors;   /* rho-update points since setup whose refactorisation ran in chunks, overlapped with the iterate segment behind it */
  int64_t resident_factor_steps, lds_bytes_factor;   /* resident head of S^-1: 512 B steps of the dense-tail stream every wave of a tile keeps in registers and LDS across a segment (0 = streamed); LDS of its part, which the iterate launches take on top of lds_bytes_iterate */
  int64_t dense_tail_tasks, dense_tail_waves_used, dense_tail_wave_tasks_max;   /* deal of the dense-tail product: 64 x 64 block tasks, waves of a tile that own at least one, most tasks of one wave */
  int64_t refactor_lanes;   /* the most chunk lanes a pipelined rho-update point has run on since setup: streams that each run factor -> tail -> iterate of their chunks (1 = one refactorisation stream and one iterate stream; 0 = none pipelined yet) */
  int64_t iterate_launches_deep_ring, iterate_launches_long_head;   /* iterate launches since setup by the form of the resident head they ran (MI_OSQP_RF_FORM, MI_OSQP_RF_LONG_MIN): 16 steps resident and a product ring of 16, or resident_factor_steps (32) and a ring of 8; both 0 on a handle without a head */
  int64_t runahead_regions, runahead_tiles, runahead_left, runahead_missed;   /* run-ahead since setup (switches, read at setup: MI_OSQP_RUNAHEAD = 0 / 1 off / on, MI_OSQP_RUNAHEAD_TILES = tiles of a group, default half the CUs, MI_OSQP_RUNAHEAD_MIN = active tiles below which no group is sent, default the CU count, MI_OSQP_RUNAHEAD_END = most segments of a chain, default up to the rho-update point after next): pipelined rho-update points that sent the active tiles furthest from convergence ahead as a chain of launches beside the region, without a host turn; tiles sent; members still active when their chain ended (they went on alone afterwards); QPs outside the groups still active after the segment that follows the region (late QPs the group did not hold) */
  int64_t region_priority, region_lane_checks, region_chunks;   /* the last pipelined rho-update point (0 before the first; switches read at setup): the stream priorities it ran with, MI_OSQP_REGION_PRIORITY - 0 every stream alike, 1 the chunk lanes at the least priority of the device, 2 the run-ahead chain on a stream of its own at the greatest, -1 asked for 1 or 2 where that priority is the one every stream has, so nothing changed; 1 when every lane failed and checked its own chunks and only the flag copy followed the join (MI_OSQP_LANE_CHECKS, one-QP tiles); its refactorisation chunks (default size: mi_osqp_debug_region_chunks) */
  int64_t resident_index_words;   /* 1: every thread of the resident iterate keeps its entries of the permutation tables (pinv, xloc) in registers across a launch, so the passes between the sweeps load nothing; 0: they are loaded in every iteration (no resident state, more entries per thread than the registers set aside hold - mi_osqp_debug_index_words_fit - or MI_OSQP_INDEX_LOADS=1, read at setup) */
} mi_osqp_stats;

typedef struct mi_osqp_solver mi_osqp_solver; /* one QP  */
typedef struct mi_osqp_batch  mi_osqp_batch;  /* B QPs, ONE shared sparsity pattern */

void        mi_osqp_default_settings(mi_osqp_settings *s);
const char *mi_osqp_exit_code_name(int64_t exit_code);  /* replaces osqp::ToString(OsqpExitCode) */
const char *mi_osqp_error_name(int64_t err);
const char *mi_osqp_version(void);
const char *mi_osqp_last_error(void);   /* text of the last MI_OSQP_ERR_DEVICE / _ALLOC on this thread */

/* ------------------------------------------------------------------ single QP
 * Replaces QPSolver::QPSolver(const QPConstraints&, const QPMatrixSparse&)
 * = OsqpSolver::Init ([REF] src/osqp-wrapper.h:16-31).  P may hold both
 * triangles (the reference's triDiagonalMatrix does, [REF] src/utils.h:53-61);
 * the upper one is used.  q may be NULL (= 0, [REF] src/osqp-wrapper.h:22). */
int mi_osqp_setup(mi_osqp_solver **out, int64_t n, int64_t m,
                  const int64_t *P_colptr, const int64_t *P_rowidx, const double *P_val,
                  const double *q,
                  const int64_t *A_colptr, const int64_t *A_rowidx, const double *A_val,
                  const double *l, const double *u, const mi_osqp_settings *settings);
/* QPSolver::update, first half = OsqpSolver::UpdateConstraintMatrix
 * ([REF] src/osqp-wrapper.h:36): same pattern required. */
int mi_osqp_update_A(mi_osqp_solver *h, const int64_t *A_colptr, const int64_t *A_rowidx,
                     const double *A_val);
/* QPSolver::update, second half = OsqpSolver::SetBounds ([REF] src/osqp-wrapper.h:40). */
int mi_osqp_update_bounds(mi_osqp_solver *h, const double *l, const double *u);
/* QPSolver::update as ONE call ([REF] src/osqp-wrapper.h:33-43: UpdateConstraintMatrix, then SetBounds): the state it
 * leaves is that of mi_osqp_update_A followed by mi_osqp_update_bounds, with one numeric refactorisation instead of two
 * when the new bounds change a row's type (equality / inequality / free).  Nothing is changed when l > u somewhere or the
 * pattern differs. */
int mi_osqp_update_A_bounds(mi_osqp_solver *h, const int64_t *A_colptr, const int64_t *A_rowidx, const double *A_val,
                            const double *l, const double *u);
/* QPSolver::setWarmStart = SetPrimalWarmStart ([REF] src/osqp-wrapper.h:45-49). */
int mi_osqp_warm_start_x(mi_osqp_solver *h, const double *x);
/* Objective updates (README "Objective updates"; OSQP 0.6.x semantics, no value validation, like OSQP):
 * osqp_update_lin_cost = osqp-cpp SetObjectiveVector: q_s = c * (D .* q) with the D and c in force; no refactorisation,
 * iterates and rho kept, the count of rho updates restarts. */
int mi_osqp_update_q(mi_osqp_solver *h, const double *q);
/* osqp_update_P = osqp-cpp UpdateObjectiveMatrix: P in the form mi_osqp_setup accepts (both triangles or the upper one);
 * its upper triangle must have the pattern of setup's (else MI_OSQP_ERR_PATTERN_CHANGED, nothing changed).  P, A and q are
 * unscaled, triu(P) replaced, the problem equilibrated again (new D, E, c; bounds rescaled) and refactored with the current
 * rho vectors. */
int mi_osqp_update_P(mi_osqp_solver *h, const int64_t *P_colptr, const int64_t *P_rowidx, const double *P_val);
/* osqp_update_P_A = osqp-cpp UpdateObjectiveAndConstraintMatrices: both, with one equilibration and one refactorisation. */
int mi_osqp_update_P_A(mi_osqp_solver *h, const int64_t *P_colptr, const int64_t *P_rowidx, const double *P_val,
                       const int64_t *A_colptr, const int64_t *A_rowidx, const double *A_val);
/* osqp_warm_start_y = osqp-cpp SetDualWarmStart: y_s = c * (Einv .* y), warm_start = 1; x and z untouched.  osqp-cpp
 * SetWarmStart(x, y) = mi_osqp_warm_start_x followed by mi_osqp_warm_start_y. */
int mi_osqp_warm_start_y(mi_osqp_solver *h, const double *y);
/* QPSolver::solve = Solve ([REF] src/osqp-wrapper.h:52); returns error code,
 * exit code and residuals in *info (may be NULL). */
int mi_osqp_solve(mi_osqp_solver *h, mi_osqp_info *info);
/* primal_solution() ([REF] src/osqp-wrapper.h:53) / dual_solution(); NaN-filled
 * when the exit code carries no solution. */
int mi_osqp_get_primal(mi_osqp_solver *h, double *x_out);
int mi_osqp_get_dual(mi_osqp_solver *h, double *y_out);
/* Infeasibility certificates: what osqp_solve leaves in OSQPSolution::y / ::x of an infeasible problem (OSQP 0.6.2
 * store_solution: prim_inf_cert = delta_y, dual_inf_cert = delta_x) and osqp-cpp returns from
 * primal_infeasibility_certificate() / dual_infeasibility_certificate().
 *   primal (status_val -3 or 3; m entries): delta_y of the exit iteration after the projection of the infeasibility test -
 *     0 on rows without bounds, min(., 0) where only u is infinite, max(., 0) where only l is infinite -,
 *   dual (status_val -4 or 4; n entries): delta_x of the exit iteration,
 * multiplied by E / D when scaling != 0 and scaled_termination = 0 (else left in the scaled space, as upstream leaves it),
 * then divided by its infinity norm: the largest entry is exactly +-1.  With any other status (kNonConvex included), before
 * the first finished solve, and for the certificate of the other kind every entry reads NaN.  A certificate belongs to the
 * last finished solve of its QP, like mi_osqp_info: updates and warm starts in between leave it, the next finished solve
 * replaces it - with NaN when that solve ends with a solution.  x, y and info of an infeasible QP are what they were: NaN,
 * NaN, obj_val = +-1e30.  m = 0: mi_osqp_get_prim_inf_cert writes nothing. */
int mi_osqp_get_prim_inf_cert(mi_osqp_solver *h, double *dy_out /*[m]*/);
int mi_osqp_get_dual_inf_cert(mi_osqp_solver *h, double *dx_out /*[n]*/);
/* Adjoint derivative of the solution (OSQP 1.0 osqp_adjoint_derivative_compute / _get_mat / _get_vec; see
 * mi_osqp_batch_adjoint_device below for the mathematics, the layouts and the status): one QP, a large one in the dataflow
 * form included.  dx, dq [n]; dy, dl, du [m]; dP [nnz of triu(P)]; dA [nnzA]; status [1].  dy and every output may be NULL. */
int mi_osqp_adjoint(mi_osqp_solver *h, const double *dx, const double *dy, double *dq, double *dP, double *dA, double *dl, double *du,
                    int32_t *status);
int mi_osqp_get_stats(mi_osqp_solver *h, mi_osqp_stats *st);
/* Settings after setup (see "settings updates" below); a large single QP - one workgroup or the dataflow grid - included. */
int mi_osqp_get_settings(mi_osqp_solver *h, mi_osqp_settings *out);
int mi_osqp_update_settings(mi_osqp_solver *h, const mi_osqp_settings *s);
void mi_osqp_free(mi_osqp_solver *h);

/* --------------------------------------------------------------------- batch
 * B independent QPs sharing ONE sparsity pattern (the GOMP situation: the
 * reference keeps A's pattern constant on purpose, [REF]
 * src/constraints/constraint-builder.h:112-116).  Values/bounds are QP-major:
 * P_val[B][nnzP], q[B][n] (or NULL), A_val[B][nnzA], l/u[B][m].
 * device < 0 selects the current HIP device. */
int mi_osqp_batch_setup(mi_osqp_batch **out, int64_t B, int64_t n, int64_t m,
                        const int64_t *P_colptr, const int64_t *P_rowidx, const double *P_val,
                        const double *q,
                        const int64_t *A_colptr, const int64_t *A_rowidx, const double *A_val,
                        const double *l, const double *u, const mi_osqp_settings *settings,
                        int64_t device);
int mi_osqp_batch_update_A(mi_osqp_batch *h, const int64_t *A_colptr, const int64_t *A_rowidx,
                           const double *A_val);
int mi_osqp_batch_update_bounds(mi_osqp_batch *h, const double *l, const double *u);
int mi_osqp_batch_update_A_bounds(mi_osqp_batch *h, const int64_t *A_colptr, const int64_t *A_rowidx, const double *A_val,
                                  const double *l, const double *u);      /* see mi_osqp_update_A_bounds */
int mi_osqp_batch_warm_start_x(mi_osqp_batch *h, const double *x);
/* Objective updates of every QP (see mi_osqp_update_q / _update_P / _update_P_A / _warm_start_y): q[B][n]; P values
 * [B][nnz of the P array as passed], in the caller's CSC order as at setup; y[B][m].  After them the raw P and q the handle
 * keeps (mi_osqp_batch_reinit_some) are the ones in force.  A QP whose new KKT matrix is not quasi-definite ends its next
 * solve as kNonConvex; the other QPs are not affected. */
int mi_osqp_batch_update_q(mi_osqp_batch *h, const double *q);                                     /* osqp_update_lin_cost */
int mi_osqp_batch_update_P(mi_osqp_batch *h, const int64_t *P_colptr, const int64_t *P_rowidx, const double *P_val);   /* osqp_update_P */
int mi_osqp_batch_update_P_A(mi_osqp_batch *h, const int64_t *P_colptr, const int64_t *P_rowidx, const double *P_val,
                             const int64_t *A_colptr, const int64_t *A_rowidx, const double *A_val);  /* osqp_update_P_A */
int mi_osqp_batch_warm_start_y(mi_osqp_batch *h, const double *y);                                 /* osqp_warm_start_y */
/* The pattern of triu(P) as the analysis keeps it (CSC, n + 1 column pointers, *nnz_out = nnzPu row indices): the order of
 * the adjoint's dP and of every P array of the _device and _some forms below, whichever form P had at setup.  Either array may
 * be NULL; *nnz_out is always written.  No device is touched; the continuous mode stays. */
int mi_osqp_batch_get_P_upper_pattern(mi_osqp_batch *h, int64_t *colptr, int64_t *rowidx, int64_t *nnz_out);   /* [n+1], [nnzPu] */
/* Blocking solve of all B QPs (the ADMM iterate runs on the GPU). */
int mi_osqp_batch_solve(mi_osqp_batch *h);
int mi_osqp_batch_get_primal(mi_osqp_batch *h, double *x_out /*[B][n]*/);
int mi_osqp_batch_get_dual(mi_osqp_batch *h, double *y_out /*[B][m]*/);
int mi_osqp_batch_get_info(mi_osqp_batch *h, mi_osqp_info *info /*[B]*/);
/* Infeasibility certificates of every QP (see mi_osqp_get_prim_inf_cert): the rows of QPs without a certificate of that kind
 * are NaN.  Like mi_osqp_batch_get_primal they end the continuous mode, and they work after mi_osqp_batch_solve_device. */
int mi_osqp_batch_get_prim_inf_cert(mi_osqp_batch *h, double *dy_out /*[B][m]*/);
int mi_osqp_batch_get_dual_inf_cert(mi_osqp_batch *h, double *dx_out /*[B][n]*/);
int mi_osqp_batch_get_stats(mi_osqp_batch *h, mi_osqp_stats *st);
/* the elimination order the analysis chose for the KKT matrix [[P + sigma I, A'], [A, -1/rho]]: kkt_perm[k] = natural index
 * (0 .. n-1 variables, n .. n+m-1 constraint rows) eliminated k-th; n + m entries.  (Lets a CPU checker factor the same
 * large KKT matrix without a minimum-degree ordering of its own.) */
int mi_osqp_batch_get_ordering(mi_osqp_batch *h, int64_t *kkt_perm);
void mi_osqp_batch_free(mi_osqp_batch *h);
/* Compute the pattern analysis (ordering, symbolic factor, schedules) that a later mi_osqp_batch_setup / mi_osqp_setup of B
 * QPs with this sparsity pattern on this device will need, into the process-wide analysis cache.  Thread-safe; blocking (call
 * it from a spare host thread); a setup that arrives meanwhile waits for it.  The reference builds a fresh QPSolver per horizon
 * ([REF] src/gomp-solver.h:61-65): a planner that knows its horizons up front takes the analyses off its critical path. */
int mi_osqp_prefetch_analysis(int64_t B, int64_t n, int64_t m, const int64_t *Pp, const int64_t *Pi,
                              const int64_t *Ap, const int64_t *Ai, int64_t device);
/* Freed handles leave their device buffers (at most 8 GiB), pinned host buffers (at most 1 GiB) and stream / event sets in
 * process-wide caches for the next setup - the GOMP drivers build one solver per horizon segment; this returns them to
 * the HIP runtime. */
void mi_osqp_release_device_cache(void);

/* Device-resident I/O (HBM pointers on the solver's device; `stream` is a
 * hipStream_t passed as void*, NULL = default stream).
 * d_l/d_u: [B][m] doubles, unscaled; the E-scaling and the constraint-type
 * check run on the device (no refactor happens unless a type changes, in which
 * case the call returns through the host path transparently). */
int mi_osqp_batch_update_bounds_device(mi_osqp_batch *h, const double *d_l, const double *d_u, void *stream);
/* QPSolver::update ([REF] src/osqp-wrapper.h:33-43) with the new A values ([B][nnzA], CSC order of setup's pattern) and bounds
 * ([B][m]) in HBM; `stream`: the stream that wrote them (NULL: none pending) */
int mi_osqp_batch_update_A_bounds_device(mi_osqp_batch *h, const double *d_Av, const double *d_l, const double *d_u, void *stream);
/* osqp_update_lin_cost with q ([B][n], unscaled) in HBM: nothing crosses PCIe; `stream`: the stream that wrote it */
int mi_osqp_batch_update_q_device(mi_osqp_batch *h, const double *d_q, void *stream);
/* osqp_update_P with the new values in HBM: d_Pv [B][nnzPu] holds triu(P) in the order of
 * mi_osqp_batch_get_P_upper_pattern - the layout of the adjoint's dP, so a gradient step on dP can be handed straight back.
 * Semantics of mi_osqp_batch_update_P (unscale q, A and the bounds with the scaling in force, replace triu(P), equilibrate,
 * refactor every QP with its current rho vectors, snapshot, restart the count of rho updates; the raw P the handle keeps
 * follows); P does not cross PCIe.  `stream`: the stream that wrote the values (NULL: none pending).
 * _update_P_A_bounds_device: new A values ([B][nnzA]) and bounds ([B][m]) with it - one equilibration, one refactorisation and
 * one snapshot for everything given.  d_Pv == NULL is mi_osqp_batch_update_A_bounds_device; d_Av, d_l and d_u all NULL is
 * mi_osqp_batch_update_P_device; any other NULL is MI_OSQP_ERR_NULL.  l > u anywhere: MI_OSQP_ERR_INVALID_DATA, nothing
 * changes.  Handles that equilibrate on host threads (fewer than 16 QPs, or large ones) fetch the values and take the host
 * path: same results, the data crosses PCIe twice. */
int mi_osqp_batch_update_P_device(mi_osqp_batch *h, const double *d_Pv, void *stream);
int mi_osqp_batch_update_P_A_bounds_device(mi_osqp_batch *h, const double *d_Pv, const double *d_Av, const double *d_l, const double *d_u,
                                           void *stream);
/* Solve and leave x[B][n] (and optionally status[B]/iters[B], int32) in HBM. */
int mi_osqp_batch_solve_device(mi_osqp_batch *h, double *d_x_out, int32_t *d_status, int32_t *d_iters, void *stream);
/* Back to the state right after setup (or after the last update that refactored): cold-start every QP, restore rho,
 * the rho vectors and the factor of that moment, forget the count of rho updates.  q is not part of that state: the q in
 * force (the last mi_osqp_batch_update_q, if any) is kept.  A planner that builds the same
 * solver again and again (one per horizon segment and run, [REF] src/gomp-solver.h:61) may keep the handle instead:
 * reset + update_bounds + warm_start gives bitwise the results of a fresh setup with the same P and A.  The bench uses it
 * so that repeated steps do identical work. */
int mi_osqp_batch_reset(mi_osqp_batch *h);
/* Totals of the last solve: ADMM iterations summed over QPs, iterate launches (= segments),
 * seconds in iterate_kernel (HIP events), in device refactorisations and in the
 * compaction swaps (wall, including their synchronisation). */
int mi_osqp_batch_last_solve_stats(mi_osqp_batch *h, int64_t *total_iters, int64_t *kernel_launches,
                                   double *device_seconds, double *refactor_seconds, int64_t *refactor_count,
                                   double *compact_seconds);
/* Polishing of the last solve: QPs polished (those that ended kOptimal), QPs whose polished solution was accepted, and the
 * seconds the polish took on the device (HIP events: active set, polish factor, polish kernel).  Zeros without polish.
 * In the continuous mode: the counts of the last poll() that reported polished QPs; seconds = 0 (not measured there: nothing
 * waits for the polish). */
int mi_osqp_batch_last_polish_stats(mi_osqp_batch *h, int64_t *polished, int64_t *accepted, double *seconds);
/* (tests) the active set of the last polish, act[B][m]: -1 lower-active, +1 upper-active, 0 inactive (all 0 for QPs that
 * were not polished, and before the first polish).  After mi_osqp_batch_polish_some: per QP, the active set of its last
 * polish; in the continuous mode the call waits for the work enqueued on the handle (polishes included) and does not end
 * the mode. */
int mi_osqp_batch_get_polish_active(mi_osqp_batch *h, int8_t *act);

/* -------------------------------------------------------- adjoint derivative
 * OSQP 1.0 osqp_adjoint_derivative_compute + osqp_adjoint_derivative_get_mat + osqp_adjoint_derivative_get_vec in one call
 * (README "Adjoint derivative").  Given dx = dL/dx [B][n] and dy = dL/dy [B][m] (NULL = zero; read on
 * active rows only, y is 0 on the others) of a loss L(x, y) at the solutions of the last solve, the call returns the gradient
 * of L with respect to the problem data, per QP:
 *   dq [B][n], dl [B][m], du [B][m],
 *   dA [B][nnzA]  in the CSC order of A,
 *   dP [B][nnzP]  on the pattern and CSC order of the UPPER triangle of P (the upper form mi_osqp_batch_update_P takes),
 *                 whichever form P had at setup: the derivative with respect to the stored value, which stands for (i, j)
 *                 and (j, i).
 * It is the derivative of the active-set solution map: the active set is taken from the current iterate by the polish rule,
 * K = [[P, A_a'], [A_a, 0]] is factored by the polish machinery (settings delta, polish_refine_iter) and K r = [dx; dy_a] is
 * solved; dq = -r_x, dl_i / du_i = r_y,i on the side the row is active at (an equality row: the side the rule marked),
 * dA_k = -(y_i r_x,j + r_y,i x_j), dP_k = -(r_x,i x_j + r_x,j x_i) (diagonal: -(r_x,i x_i)).  Where strict complementarity
 * fails (a weakly active row) the true map is not differentiable and the call returns the derivative for the marked set.
 * The result is exact for the exact solution of the active set: solve with polish = 1 or tight tolerances for accurate
 * gradients.  Call it after a solve and before the next update or warm start: it differentiates the data in force.
 * status [B] (may be NULL): 1 computed; 0 the QP's last solve did not end kOptimal, or none has finished; -1 its reduced
 * factor failed the inertia test.  The outputs of a QP whose status is not 1 read NaN.  Any output may be NULL: it is not
 * computed.  dx is required (MI_OSQP_ERR_NULL); an output that aliases dx or dy is MI_OSQP_ERR_INVALID_DATA; a refused call
 * has enqueued nothing.  The call changes nothing else - x, y, the iterates, rho, the ADMM factor, the infos (status_polish
 * included) and the certificates stay bit for bit, and the next solve is the one that would have run without it - except that
 * mi_osqp_batch_get_polish_active afterwards returns the active set the adjoint used.  Like the other whole-batch calls it
 * ends the continuous mode.  _device: every pointer is device memory, the work is ordered on `stream` (NULL: the handle's)
 * and finished when the call returns. */
int mi_osqp_batch_adjoint_device(mi_osqp_batch *h, const double *d_dx, const double *d_dy, double *d_dq, double *d_dP, double *d_dA,
                                 double *d_dl, double *d_du, int32_t *d_status, void *stream);
int mi_osqp_batch_adjoint(mi_osqp_batch *h, const double *dx, const double *dy, double *dq, double *dP, double *dA, double *dl,
                          double *du, int32_t *status);

/* ---------------------------------------------------------- settings updates
 * OSQP 0.6.x osqp_update_* (README "Settings updates").  update_settings takes a whole struct - get, change fields, update:
 *   changeable  rho, max_iter, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf, alpha, scaled_termination, check_termination,
 *               warm_start, polish, polish_refine_iter, delta, verbose (the fields with an osqp_update_*);
 *   fixed       sigma, scaling, adaptive_rho, adaptive_rho_interval, adaptive_rho_tolerance must be those in force
 *               (adaptive_rho_interval = 0 is also accepted where setup derived the interval from 0).
 * A struct that differs in a fixed field, or whose values setup would refuse, gives MI_OSQP_ERR_INVALID_SETTINGS: nothing is
 * changed, no device is touched, the reason is in mi_osqp_last_error().  mi_osqp_settings_update_check is that decision as a
 * host function of two structs (it cannot know where an interval came from and accepts 0 against any interval in force).
 * get_settings returns the settings in force: the resolved adaptive_rho_interval, the clamped rho of the last scalar update -
 * not the rho a QP has adapted to, which mi_osqp_info.rho reports.
 *
 * Fields other than rho take effect at the next solve; nothing on the device changes: iterates, every QP's rho, the factor
 * and the count of rho updates are kept.  A changed check_termination does not move adaptive_rho_interval (derived at setup).
 * A rho that differs from the settings' rho is osqp_update_rho: settings.rho = min(max(rho, 1e-6), 1e6), every QP's rho
 * becomes that value and every QP is refactored on the device with the rho vector derived from it (equality rows 1e3 * rho,
 * free rows at the minimum); iterates and the count of rho updates are kept, the state mi_osqp_batch_reset returns to is
 * retaken, mi_osqp_batch_reinit_some starts from the new settings.rho.  A QP whose new KKT matrix loses its inertia ends its
 * next solve as kNonConvex; the others are not affected.
 * update_rho_each / update_rho_some: the same with one value per QP (clamped likewise); settings.rho is not touched.  A value
 * that is not > 0 (NaN included) gives MI_OSQP_ERR_INVALID_SETTINGS and nothing changes.
 *
 * Continuous mode: update_rho_some is one of its per-QP calls (idle QPs, ids in range and not repeated, else
 * MI_OSQP_ERR_INVALID_DATA; all or nothing; enqueued in stream order, nothing waits).  update_settings is refused with
 * MI_OSQP_ERR_INVALID_DATA while mi_osqp_batch_running() > 0 and otherwise accepted without leaving the mode (a new rho is
 * applied like update_rho_some over all QPs; polish = 1 is stored, and solve_begin_some goes on refusing such a handle).
 * update_rho_each and the multi-batch forms end the continuous mode like every blocking call. */
int mi_osqp_settings_update_check(const mi_osqp_settings *in_force, const mi_osqp_settings *wanted);   /* host only */
int mi_osqp_batch_get_settings(mi_osqp_batch *h, mi_osqp_settings *out);
int mi_osqp_batch_update_settings(mi_osqp_batch *h, const mi_osqp_settings *s);
int mi_osqp_batch_update_rho_each(mi_osqp_batch *h, const double *rho /*[B]*/);
int mi_osqp_batch_update_rho_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *rho /*[n_ids]*/);

/* ------------------------------------------------------ continuous batching
 * The reference's SQP loop is per trajectory: solve -> check -> re-linearise -> update -> solve again
 * ([REF] src/gomp-solver.h:70-88), with a fresh QPSolver per horizon segment ([REF] src/gomp-solver.h:61-65).  The QPs of a
 * batch therefore do not finish together, and a planner must not wait for the slowest of them.  These entry points address
 * single QPs of a batch handle (`ids`: n_ids QP numbers in [0, B); per-QP arguments are QP-major in the order of `ids`) and
 * advance whatever is iterating without blocking:
 *
 *     reinit_some / update_A_bounds_some / warm_start_x_some   new data for QPs that are not iterating
 *     update_q_some / warm_start_y_some
 *     update_P_some / update_P_A_bounds_some
 *     solve_begin_some                                         Solve() entry of those QPs (own iteration count from 0)
 *     advance(n_segments)                                      enqueue ONE launch in which every iterating QP runs up to
 *                                                              n_segments segments of L iterations + check, L =
 *                                                              gcd(check_termination, adaptive_rho_interval, max_iter) = 25 by
 *                                                              default - with the checks / rho updates a blocking solve of
 *                                                              its own would see at those iterations.  With n_segments > 1 the
 *                                                              launch ends at the first segment boundary after ANY QP of the
 *                                                              handle has finished (so that the caller can react to it), and
 *                                                              a QP whose rho changes pauses until the refactorisation that
 *                                                              follows the launch in stream order
 *     poll(wait, ...)                                          which QPs finished in the oldest advance not polled yet
 *     get_primal_some / get_dual_some / get_info_some          results of finished QPs (host memory, no device access)
 *     get_prim_inf_cert_some / get_dual_inf_cert_some          their infeasibility certificates (likewise)
 *     polish_some                                              polish finished kOptimal QPs on demand; reported once more
 *     update_rho_some                                          a new rho for QPs that are not iterating ("settings updates")
 *
 * Every QP takes exactly the iterations of a mi_osqp_batch_solve of its own: same exit code, iteration count, rho updates
 * and solution, bit for bit.  Nothing here waits for the device except poll() (and a full staging ring); at most two
 * advances may be waiting for their poll().  A blocking mi_osqp_batch_* call ends the continuous mode of the handle (solves
 * in flight are forgotten).  Not available for handles whose solve vector does not fit LDS (large single QPs).
 *
 * Results across the two modes.  The first per-QP call after setup or after a blocking call begins a continuous phase; the
 * next blocking call ends it.  A QP that finishes no solve in a phase keeps the results it had on entry - those of its last
 * finished solve, blocking or of an earlier phase, or the state after setup (zero x and y, status_val -10) if it was never
 * solved -, whatever the other QPs of the handle, its tile partner included, are given and solve meanwhile:
 *   - get_primal_some / get_dual_some / get_info_some return for it, from the first call of the phase on, what
 *     mi_osqp_batch_get_primal / _get_dual / _get_info returned on entry, in every field of mi_osqp_info (rho_updates reads 0
 *     where a whole-batch data update since the QP's last solve has restarted the count), until poll() reports a solve of it;
 *   - after the phase the whole-batch getters return the same for it, next to the new results of the QPs that did finish,
 *     and mi_osqp_batch_adjoint differentiates its solution of before the phase;
 *   - its certificates read NaN through get_*_inf_cert_some (below) and are served again by the whole-batch getters after
 *     the phase.
 *
 * reinit_some = QPSolver::QPSolver for those QPs ([REF] src/osqp-wrapper.h:16-31) with the P and q in force (those given
 * at setup, or by the last mi_osqp_batch_update_P / _update_P_A / _update_P_device / update_P_some / _update_q / update_q_some of the QP) and new A values / bounds: equilibration from the raw data, rho = settings.rho, zero iterates, no rho updates - the state
 * mi_osqp_batch_setup leaves for that QP, bit for bit, without analysis or allocation.
 * update_A_bounds_some = QPSolver::update ([REF] src/osqp-wrapper.h:33-43) for those QPs. */
int mi_osqp_batch_reinit_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids,
                              const double *A_val /*[n_ids][nnzA]*/, const double *l /*[n_ids][m]*/, const double *u);
int mi_osqp_batch_update_A_bounds_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids,
                                       const double *A_val, const double *l, const double *u);
/* osqp_update_P for those QPs, and with QPSolver::update in one equilibration and refactorisation: P_val [n_ids][nnzPu] holds
 * triu(P) in the order of mi_osqp_batch_get_P_upper_pattern (host memory, like every per-QP argument).  The listed QPs get
 * what mi_osqp_batch_update_P (then _update_A_bounds) gives them, bit for bit; the other QPs - iterating or not, the other QP
 * of a two-QP tile included - are not touched.  The QP's count of rho updates restarts, a failed factor is forgotten (an
 * indefinite P ends the QP's next solve as kNonConvex, a later good P clears that), the QP is no longer polishable, its
 * share of the reset state is retaken, and a later reinit_some of the slot starts from the new P.  ids must be idle, in range
 * and not repeated (MI_OSQP_ERR_INVALID_DATA, as is l > u); a refused call has enqueued and changed nothing. */
int mi_osqp_batch_update_P_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *P_val /*[n_ids][nnzPu]*/);
int mi_osqp_batch_update_P_A_bounds_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *P_val,
                                         const double *A_val, const double *l, const double *u);
int mi_osqp_batch_warm_start_x_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *x /*[n_ids][n]*/);
/* osqp_update_lin_cost / osqp_warm_start_y for those QPs (see mi_osqp_update_q / mi_osqp_warm_start_y) */
int mi_osqp_batch_update_q_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *q /*[n_ids][n]*/);
int mi_osqp_batch_warm_start_y_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *y /*[n_ids][m]*/);
int mi_osqp_batch_solve_begin_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids);   /* polish = 1: MI_OSQP_ERR_INVALID_SETTINGS */
int mi_osqp_batch_advance(mi_osqp_batch *h, int64_t n_segments);
/* wait != 0: block until the oldest unpolled advance has run; wait == 0: *n_finished = -1 when it has not.  ids_out receives
 * the QPs that finished in it (capacity >= B is always enough; too small: error, *n_finished = the number, nothing consumed). */
int mi_osqp_batch_poll(mi_osqp_batch *h, int64_t wait, int64_t *n_finished, int64_t *ids_out, int64_t capacity);
int mi_osqp_batch_get_primal_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, double *x_out /*[n_ids][n]*/);
int mi_osqp_batch_get_dual_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, double *y_out /*[n_ids][m]*/);
int mi_osqp_batch_get_info_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, mi_osqp_info *info /*[n_ids]*/);
/* Infeasibility certificates (see mi_osqp_get_prim_inf_cert) of the listed QPs, by the status poll() last reported for each:
 * NaN rows for QPs that have not finished a solve in this continuous phase or finished it otherwise.  Same id checks as
 * get_primal_some, no device access; bit for bit what the whole-batch getters return for the same solves.  A QP reads NaN
 * again from solve_begin_some (the solve in flight writes the row when it finishes) and from reinit_some (a new QP in the
 * slot) on, before any poll(); the other per-QP updates and warm starts leave its certificate. */
int mi_osqp_batch_get_prim_inf_cert_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, double *dy_out /*[n_ids][m]*/);
int mi_osqp_batch_get_dual_inf_cert_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, double *dx_out /*[n_ids][n]*/);
int64_t mi_osqp_batch_running(mi_osqp_batch *h);      /* QPs whose solve (or polish) has been begun and not been reported by poll() */
/* Polish the listed QPs now (OSQP polish.c; settings polish_refine_iter and delta of the handle), without waiting for the
 * device and without disturbing the QPs that are iterating - in an SQP loop only the last, accepted QP of a trajectory is
 * worth the refactorisation that a polish costs.  The handle must be in the continuous mode (else MI_OSQP_ERR_INVALID_DATA).
 * A QP is polishable from the poll() that reports it with status_val = 1 until a call changes its data or iterate or begins
 * a solve of it (reinit_some, update_A_bounds_some, update_q_some, warm_start_x_some, warm_start_y_some, solve_begin_some,
 * update_rho_some - and update_settings with a new rho, for every QP -,
 * mi_gomp_relinearise_some for the QPs it updates) or polishes it: once per solve.  All or nothing: an id out of range,
 * listed twice, still running or not polishable gives MI_OSQP_ERR_INVALID_DATA (text in mi_osqp_last_error()) and nothing
 * is enqueued or changed.  n_ids = 0: nothing happens.  (MI_OSQP_ERR_DEVICE / _ALLOC are not refusals: part of the chain
 * may have been enqueued.)
 *
 * The call enqueues, in stream order behind everything enqueued so far: the active sets of the listed QPs, their polish
 * factors, the polish, the publication of the results.  (The first polish of a handle also allocates the polish buffers.)
 * The listed QPs count as running again (mi_osqp_batch_running; no per-QP call accepts them) and are reported a SECOND time by
 * the poll() of the first advance enqueued AFTER this call - that advance need not have anything to iterate; the poll() of an
 * advance enqueued before it does not report them: the publication moves the QP's epoch, like the begin of a solve.  Then
 * get_primal_some / get_dual_some / get_info_some return the polished x, y, obj_val, pri_res, dua_res and status_polish = 1 -
 * or, with status_polish = -1 (the polished point was not better, or its KKT matrix not quasi-definite), those of the ADMM
 * solve, unchanged bit for bit.  An accepted point is the QP's iterate, i.e. its next warm start.  Every result - x, y, the
 * three scalars, status_polish, the active set - is bit for bit that of a blocking mi_osqp_batch_solve with polish = 1 on the
 * same data.  Several calls may be enqueued before a poll.  A blocking call that ends the continuous mode finds every enqueued
 * polish executed: the whole-batch getters return the polished solutions and status_polish. */
int mi_osqp_batch_polish_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids);
/* (tests) times the staging ring of the per-QP calls has wrapped since setup (a wrap waits for the handle's stream) */
int64_t mi_osqp_batch_ring_wraps(mi_osqp_batch *h);

/* ------------------------------------------- GOMP re-linearisation on the device
 * The step before and the step after the solver path in the reference's SQP loop - the re-linearised 3-D / obstacle rows
 * of the constraint matrix (ConstraintBuilder::withObstacles, [REF] src/constraints/constraint-builder.h:90-136) and the
 * feasibility check that ends the loop (GOMPSolver::isSolutionOK, [REF] src/gomp-solver.h:141-199) - for collision balls
 * whose kinematics are built-in models or a DH chain (the reference binds arbitrary host callbacks, [REF] src/utils.h:21-22,33-42; those
 * stay on the host path of include/mi_osqp/gomp.hpp).  A scene belongs to one batch handle whose QPs have the reference's
 * GOMP row layout ([REF] constraint-builder.h:34-44) for `dims` joints and `waypoints` waypoints; it keeps the raw
 * constraint data of every QP on the device, so an SQP step moves one trajectory to the device and one flag back. */
typedef enum {
  MI_GOMP_MODEL_UR5E_FLANGE = 1,   /* UR5e (published DH parameters, include/mi_osqp/ur5e_kinematics.hpp): tool flange */
  MI_GOMP_MODEL_UR5E_WRIST3 = 2,   /*   wrist-3 joint (forward_kinematics_6_back)                                      */
  MI_GOMP_MODEL_UR5E_ELBOW = 3,    /*   elbow joint                                                                    */
  MI_GOMP_MODEL_YAW_2LINK = 4,     /* 3 joints: yaw, shoulder, elbow; param = {link 1, link 2, base height}            */
  MI_GOMP_MODEL_TABLE = 5,         /* 3 joints: p = (q0, q1, q2), constant 3 x 3 Jacobian in param (known-answer tests) */
  MI_GOMP_MODEL_DH_CHAIN = 6       /* any serial arm: the scene's mi_gomp_chain; param = {frame k, centre c in frame k}  */
} mi_gomp_model;
typedef struct { int32_t model; int32_t is_gripper; double radius; double param[12]; } mi_gomp_ball;   /* = RobotBall */
typedef struct { double dir[2]; double point[3]; int32_t below; int32_t reserved; } mi_gomp_line;       /* = HorizontalLine */
typedef struct mi_gomp_scene mi_gomp_scene;
/* con_lo / con_hi: the work-space box of the gripper balls (con_3d), +-1e30 or NULL = none */
int mi_gomp_scene_create(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints,
                         int64_t n_balls, const mi_gomp_ball *balls, int64_t n_lines, const mi_gomp_line *lines,
                         const double *con_lo, const double *con_hi);
/* A serial chain of revolute joints by its standard DH table, T_i = Rz(q_i + theta0_i) Tz(d_i) Tx(a_i) Rx(alpha_i) for
 * i = 0 .. n_joints-1 (the convention of include/mi_osqp/ur5e_kinematics.hpp; host twin: include/mi_osqp/dh_kinematics.hpp).
 * Frame k (1 <= k <= n_joints) is the frame after k joints, with origin o_k and rotation R_k.  A ball of
 * MI_GOMP_MODEL_DH_CHAIN is fixed in one of them: param[0] = k, param[1..3] = its centre c in frame k; its position is
 * p = o_k + R_k c and column j of its Jacobian z_j x (p - o_j) for j < k (z_j, o_j: axis and origin of joint j), 0 for j >= k. */
typedef struct { int32_t n_joints; int32_t reserved; double a[8], d[8], alpha[8], theta0[8]; } mi_gomp_chain;
/* mi_gomp_scene_create with one chain for the scene's MI_GOMP_MODEL_DH_CHAIN balls (n_joints = dims); balls of the other
 * models of that `dims` may stand beside them.  chain == NULL: exactly mi_gomp_scene_create, which refuses model 6.
 * Refused on the host, before any device call, with *out = NULL, the handle usable and the reason in mi_osqp_last_error():
 * a chain ball without a chain (MI_OSQP_ERR_NULL); n_joints != dims or outside 1..8, a non-finite chain or ball
 * parameter, param[0] not an integer in 1..n_joints (MI_OSQP_ERR_INVALID_DATA). */
int mi_gomp_scene_create_chain(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints,
                               const mi_gomp_chain *chain, int64_t n_balls, const mi_gomp_ball *balls,
                               int64_t n_lines, const mi_gomp_line *lines, const double *con_lo, const double *con_hi);
/* A capsule obstacle: the segment a .. b swept by a sphere of radius `radius`; a == b is a sphere (host twin:
 * CapsuleObstacle in include/mi_osqp/gomp.hpp).  For a ball with centre p = fk(q_w), radius r and position Jacobian J:
 * c = the point of the segment closest to p (c = a + t (b - a), t = min(1, max(0, (p - a).(b - a) / |b - a|^2)); c = a for
 * a == b), dist = |p - c|, clearance s = dist - (radius + r), normal nrm = (p - c) / dist, or (0, 0, 1) when dist <= 1e-12.
 * The row of (ball, waypoint, capsule) holds nrm' J in the columns of q_w, whether it is active or not.  It is active when
 * s < margin: l = (radius + r) - dist + (nrm' J) q_w, u = +1e30 - the linearisation of s(q) >= 0 around q_w, the ball's radius
 * included; otherwise l = -1e30, u = +1e30.  A trajectory is accepted only if s >= -1e-3 for every ball, waypoint and
 * capsule.  `margin` is the caller's tool against passing through an obstacle between two waypoints. */
typedef struct { double a[3], b[3]; double radius; double margin; } mi_gomp_capsule;
/* mi_gomp_scene_create_chain with capsules besides the lines.  Inside the block of a (ball, waypoint) pair the rows are: the
 * three box rows of a gripper ball, the lines, then the capsules in the order given, so the constraint matrix must hold
 * waypoints * sum over the balls of ((gripper ? 3 : 0) + n_lines + n_capsules) rows from the first 3-D row on.
 * chain == NULL: as mi_gomp_scene_create; n_capsules == 0: exactly mi_gomp_scene_create_chain.  Refused on the host, before any
 * device call, with *out = NULL, the handle usable and the reason in mi_osqp_last_error(): n_capsules > 0 without capsules
 * (MI_OSQP_ERR_NULL); n_capsules < 0, a capsule field that is not finite, a negative radius or margin, a constraint matrix
 * that does not hold the rows (MI_OSQP_ERR_INVALID_DATA). */
int mi_gomp_scene_create_world(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints,
                               const mi_gomp_chain *chain, int64_t n_balls, const mi_gomp_ball *balls,
                               int64_t n_lines, const mi_gomp_line *lines, int64_t n_capsules, const mi_gomp_capsule *capsules,
                               const double *con_lo, const double *con_hi);
/* A cuboid obstacle: an oriented box with centre `centre`, orthonormal axes u_0, u_1, u_2 (the rows of `axes`, u_k =
 * axes[3 k .. 3 k + 2] in world coordinates; a left-handed frame describes the same set and is accepted) and half extents
 * half[k] >= 0 along them (0: a plate, a bar, a point), swept by a sphere of radius `radius` (0: the sharp box); host twin:
 * CuboidObstacle in include/mi_osqp/gomp.hpp.  (Not the "three box rows of a gripper ball": those are the work-space limits
 * con_lo / con_hi.)  For a ball with centre p = fk(q_w), radius r and position Jacobian J, in this order of operations:
 *   d_k = p_k - centre_k;  y_k = u_k0 d_0 + u_k1 d_1 + u_k2 d_2  (p in the cuboid's frame);
 *   c_k = min(half_k, max(-half_k, y_k))  (the closest point of the box);  v_k = y_k - c_k;  out = sqrt(v_0^2 + v_1^2 + v_2^2);
 *   out > 1e-12 (outside: face, edge or corner region):  sd = out,  nl_k = v_k / out;
 *   otherwise (inside or on the surface: leave through the nearest face):  slack_k = half_k - |c_k|,  k* = the smallest k
 *     with slack_k = min(slack),  sd = -slack_k*,  nl = e_k* times (c_k* < 0 ? -1 : +1)  (so -0.0 and 0 give +1);
 *   n_i = nl_0 u_0i + nl_1 u_1i + nl_2 u_2i  (back to the world);  reach = radius + r;  clearance s = sd - reach.
 * The row of (ball, waypoint, cuboid) holds g_j = n_x J[x][j] + n_y J[y][j] + n_z J[z][j] in the columns of q_w, whether it
 * is active or not.  It is active when s < margin: l = (reach - sd) + sum_j g_j q_w[j], u = +1e30; otherwise l = -1e30,
 * u = +1e30.  A trajectory is accepted only if s >= -1e-3 for every ball, waypoint and cuboid.  `margin` has the capsule's
 * meaning; as there, no neighbouring waypoint is looked at. */
typedef struct { double centre[3]; double axes[9]; double half[3]; double radius; double margin; } mi_gomp_cuboid;   /* 136 bytes */
/* mi_gomp_scene_create_world with cuboids besides the lines and capsules.  Inside the block of a (ball, waypoint) pair the
 * rows are: the three work-space rows of a gripper ball, the lines, the capsules, then the cuboids in the order given, so the
 * constraint matrix must hold waypoints * sum over the balls of ((gripper ? 3 : 0) + n_lines + n_capsules + n_cuboids) rows
 * from the first 3-D row on.  n_cuboids == 0: exactly mi_gomp_scene_create_world.  Refused on the host, before any device
 * call, with *out = NULL, the handle usable and the reason in mi_osqp_last_error() naming the cuboid's index: n_cuboids > 0
 * without cuboids (MI_OSQP_ERR_NULL); n_cuboids < 0, a cuboid field that is not finite, a negative half extent, radius or
 * margin, axes with |u_i . u_j - delta_ij| > 1e-9 for some i, j, a constraint matrix that does not hold the rows
 * (MI_OSQP_ERR_INVALID_DATA). */
int mi_gomp_scene_create_cuboids(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints,
                                 const mi_gomp_chain *chain, int64_t n_balls, const mi_gomp_ball *balls,
                                 int64_t n_lines, const mi_gomp_line *lines, int64_t n_capsules, const mi_gomp_capsule *capsules,
                                 int64_t n_cuboids, const mi_gomp_cuboid *cuboids, const double *con_lo, const double *con_hi);
/* A self-collision pair: balls a and b of the scene (indices into `balls`) must stay apart; host twin: BallPair in
 * include/mi_osqp/gomp.hpp.  At waypoint w, with p_a, p_b the two centres, J_a, J_b the 3 x D position Jacobians and r_a, r_b
 * the radii, in this order of operations:
 *   v = p_a - p_b;  dist = sqrt(v_x^2 + v_y^2 + v_z^2);
 *   dist > 1e-12:  n = v / dist;  otherwise n = (0, 0, 1);
 *   reach = r_a + r_b;  clearance s = dist - reach;
 *   g_j = (n_x Ja[x][j] + n_y Ja[y][j] + n_z Ja[z][j]) - (n_x Jb[x][j] + n_y Jb[y][j] + n_z Jb[z][j]).
 * The row of (pair, waypoint) holds g_j in the columns of q_w, whether it is active or not.  It is active when s < margin:
 * l = (reach - dist) + sum_j g_j q_w[j], u = +1e30; otherwise l = -1e30, u = +1e30.  A trajectory is accepted only if
 * s >= -1e-3 at every (pair, waypoint).  Both radii are part of the bound, as for capsules; nothing is added on top. */
typedef struct { int32_t a, b; double margin; } mi_gomp_pair;   /* 16 bytes */
/* mi_gomp_scene_create_cuboids with ball pairs besides.  The pair rows follow the block of the last ball and waypoint,
 * pair-major: the row of (pair k, waypoint w) is the first 3-D row + the rows of all ball blocks + k waypoints + w, so the
 * constraint matrix must hold waypoints * n_pairs rows more.  n_pairs == 0: exactly mi_gomp_scene_create_cuboids.  Refused on
 * the host, before any device call, with *out = NULL, the handle usable and the reason in mi_osqp_last_error() naming the
 * pair's index: n_pairs > 0 without pairs (MI_OSQP_ERR_NULL); n_pairs < 0, a margin that is not finite or negative, a or b
 * outside 0 .. n_balls - 1, a == b, two MI_GOMP_MODEL_DH_CHAIN balls of one frame (their distance is constant and the row all
 * zeros), a constraint matrix that does not hold the rows (MI_OSQP_ERR_INVALID_DATA). */
int mi_gomp_scene_create_pairs(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints,
                               const mi_gomp_chain *chain, int64_t n_balls, const mi_gomp_ball *balls,
                               int64_t n_lines, const mi_gomp_line *lines, int64_t n_capsules, const mi_gomp_capsule *capsules,
                               int64_t n_cuboids, const mi_gomp_cuboid *cuboids, int64_t n_pairs, const mi_gomp_pair *pairs,
                               const double *con_lo, const double *con_hi);
/* A tilt limit: the unit vector `axis`, fixed in frame `frame` of the scene's mi_gomp_chain (1 <= frame <= n_joints), must stay
 * within max_angle radians of the unit world vector `ref` ("keep the tool upright"); host twin: TiltLimit in
 * include/mi_osqp/gomp.hpp.  At waypoint w, q = q_w, with R_k the rotation of frame k (R_0 = I) and z_j the third column of
 * R_j, the axis of joint j, in this order of operations:
 *   u_r = R_k[r][0] axis_0 + R_k[r][1] axis_1 + R_k[r][2] axis_2            (the axis in the world)
 *   c   = u_x ref_x + u_y ref_y + u_z ref_z                                  (cosine of the tilt)
 *   h_j = z_j x u;   g_j = h_jx ref_x + h_jy ref_y + h_jz ref_z   for j < k;   g_j = 0 for j >= k
 * (a joint j < k rotates everything behind it about z_j, so du/dq_j = z_j x u: g is the exact gradient of c).  Three
 * thresholds are taken once on the host, in fp64, when the scene is created:
 *   cos_lim = cos(max_angle);  cos_act = cos(max(0, max_angle - margin));  cos_ok = cos(min(pi, max_angle + 1e-3)).
 * The row of (tilt, waypoint) holds g_j in the columns of q_w, whether it is active or not.  It is active when c < cos_act,
 * that is within `margin` radians of the cone: l = (cos_lim - c) + sum_j g_j q_w[j], u = +1e30, the linearisation of
 * c(q) >= cos_lim around q_w; otherwise l = -1e30, u = +1e30.  A trajectory is accepted only if c >= cos_ok at every (tilt,
 * waypoint): 1 mrad, the angular counterpart of the 1 mm of the other primitives.  The cosine form is smooth where the axis
 * meets ref; an angle has no gradient there.  When u is parallel or antiparallel to ref the row is all zeros: parallel it is
 * inactive; antiparallel it is active with l = cos_lim + 1 > 0, and that QP is primal infeasible. */
typedef struct { int32_t frame; int32_t reserved; double axis[3]; double ref[3]; double max_angle; double margin; } mi_gomp_tilt;   /* 72 bytes */
/* mi_gomp_scene_create_pairs with tilt limits besides.  The tilt rows follow the pair rows, tilt-major: the row of (tilt k,
 * waypoint w) is the first 3-D row + the rows of all ball blocks + waypoints * n_pairs + k waypoints + w, so the constraint
 * matrix must hold waypoints * n_tilts rows more.  n_tilts == 0: exactly mi_gomp_scene_create_pairs.  Refused on the host,
 * before any device call, with *out = NULL, the handle usable and the reason in mi_osqp_last_error() naming the tilt's
 * index: n_tilts > 0 without tilts, tilts without a chain (MI_OSQP_ERR_NULL); n_tilts < 0, a frame outside 1 .. n_joints, a
 * field that is not finite, | |axis| - 1 | > 1e-9 and the same for ref, max_angle not in (0, pi), margin < 0, a constraint
 * matrix that does not hold the rows (MI_OSQP_ERR_INVALID_DATA). */
int mi_gomp_scene_create_tilts(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints,
                               const mi_gomp_chain *chain, int64_t n_balls, const mi_gomp_ball *balls,
                               int64_t n_lines, const mi_gomp_line *lines, int64_t n_capsules, const mi_gomp_capsule *capsules,
                               int64_t n_cuboids, const mi_gomp_cuboid *cuboids, int64_t n_pairs, const mi_gomp_pair *pairs,
                               int64_t n_tilts, const mi_gomp_tilt *tilts, const double *con_lo, const double *con_hi);
/* A distance grid: a sensed world.  A box of n[0] x n[1] x n[2] nodes (each n[k] >= 2) of spacing cell > 0 on all axes,
 * axis-aligned in the world, node (0,0,0) at `origin`; each node holds a finite distance to the nearest surface, positive in
 * free space, negative inside material, possibly truncated; the x index is fastest: V[(iz * n[1] + iy) * n[0] + ix].  Host
 * twin: DistanceGrid in include/mi_osqp/gomp.hpp.  inv_cell = 1 / cell is taken once on the host, in fp64, when the scene is
 * created.  For a ball with centre p = fk(q_w), radius r and 3 x D position Jacobian J, in this order of operations:
 *   f_k = (p_k - origin_k) * inv_cell                                   k = 0, 1, 2
 *   inside  <=>  for every k:  f_k >= 0  and  f_k <= n_k - 1             (written so that a NaN is outside)
 *   outside:  the grid says nothing: g = 0 (the zeros are written), l = -1e30, u = +1e30, the verdict is not touched
 *   inside:   i_k = min(n_k - 2, (int) floor(f_k));   t_k = f_k - i_k     (0 <= t_k <= 1; a point on a cell face belongs to the
 *                                                                          upper cell, the last node to the last cell with t = 1)
 *     v_abc = V at node (i_0 + a, i_1 + b, i_2 + c),  a, b, c in {0, 1}
 *     e_bc  = v_1bc - v_0bc;          x_bc = v_0bc + t_0 * e_bc          (along x: 4 differences, 4 values)
 *     ey_c  = x_1c - x_0c;            y_c  = x_0c + t_1 * ey_c           (along y, of the values)
 *     ex_c  = e_0c + t_1 * (e_1c - e_0c)                                 (along y, of the x differences)
 *     phi   = y_0 + t_2 * (y_1 - y_0)
 *     G_x   = (ex_0 + t_2 * (ex_1 - ex_0)) * inv_cell
 *     G_y   = (ey_0 + t_2 * (ey_1 - ey_0)) * inv_cell
 *     G_z   = (y_1 - y_0) * inv_cell
 *     reach = offset + r;   s = phi - reach
 *     g_j   = G_x J[x][j] + G_y J[y][j] + G_z J[z][j]                    written whether the row is active or not
 *     s < margin:  l = (reach - phi) + sum_j g_j q_w[j],  u = +1e30       otherwise l = -1e30, u = +1e30
 *     accepted only if s >= -1e-3
 * G is the exact gradient of the trilinear interpolant inside the cell and is deliberately not normalised: the row is the exact
 * linearisation of phi(p(q)) - reach >= 0.  Where G = 0 (a flat, truncated region) the row is all zeros; such a row that is
 * active with s < 0 makes its QP primal infeasible: start outside the material, and truncate no lower than the margin.
 * offset >= 0 inflates the obstacles; margin >= 0 has the capsule's meaning. */
typedef struct { double origin[3]; double cell; int32_t n[3]; int32_t reserved; double offset; double margin;
                 const double *values; } mi_gomp_grid;   /* 72 bytes; values: host memory, copied at creation */
/* mi_gomp_scene_create_tilts with distance grids besides.  Inside the block of a (ball, waypoint) pair the grids' rows follow
 * the cuboids', in the order given: a ball's block is (gripper ? 3 : 0) + n_lines + n_capsules + n_cuboids + n_grids rows per
 * waypoint; the pair rows and then the tilt rows follow the last block.  n_grids == 0: exactly mi_gomp_scene_create_tilts.
 * Refused on the host, before any device call, with *out = NULL, the handle usable and the reason in mi_osqp_last_error()
 * naming the grid's index: n_grids > 0 without grids, a grid without values (MI_OSQP_ERR_NULL); n_grids < 0, an n[k] outside
 * 2 .. 1024 or more than 2^24 values, a cell, offset or margin that is not finite, cell <= 0, a negative offset or margin, an
 * origin that is not finite, a value that is not finite (the message names the first such node), a constraint matrix that
 * does not hold the rows (MI_OSQP_ERR_INVALID_DATA). */
int mi_gomp_scene_create_grids(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints, const mi_gomp_chain *chain,
        int64_t n_balls, const mi_gomp_ball *balls, int64_t n_lines, const mi_gomp_line *lines,
        int64_t n_capsules, const mi_gomp_capsule *capsules, int64_t n_cuboids, const mi_gomp_cuboid *cuboids,
        int64_t n_pairs, const mi_gomp_pair *pairs, int64_t n_tilts, const mi_gomp_tilt *tilts,
        int64_t n_grids, const mi_gomp_grid *grids, const double *con_lo, const double *con_hi);
/* New values of the same shape for grid k of the scene (a new camera frame without a new scene), copied on the handle's
 * stream.  Kept rows are not touched: the next mi_gomp_assemble_some / mi_gomp_relinearise_some sees the new values.  Refused,
 * with nothing changed: no scene or no values (MI_OSQP_ERR_NULL); a scene without grids, k outside 0 .. n_grids - 1, a value
 * that is not finite (MI_OSQP_ERR_INVALID_DATA). */
int mi_gomp_scene_update_grid(mi_gomp_scene *sc, int64_t k, const double *values);
/* A grasp goal: where a trajectory has to arrive, in task space (host twin: GraspGoal in include/mi_osqp/gomp.hpp).  The
 * structure, shared by every QP of the scene: the centre of ball `ball` at waypoint `waypoint`, and with frame >= 1 the unit
 * vector `axis` fixed in frame `frame` of the scene's mi_gomp_chain (frame 0: a position-only goal, `axis` is not read).  What
 * is asked differs from QP to QP (mi_gomp_goal_value): the target `point`, half widths tol[3] >= 0 (>= 1e30: that axis is
 * free; 0: an equality), and for frame >= 1 the unit world vector `ref` and max_angle in (0, pi).  A goal owns four rows, their
 * entries in the columns of q_w, w its waypoint.  With p the ball's centre at q_w, J its Jacobian and
 * Jq_ax = sum_j J[ax][j] q_w[j], j ascending, in this order of operations:
 *   rows 0 .. 2 (ax = x, y, z) hold J[ax][j];  a free axis: l = -1e30, u = +1e30;  otherwise
 *     l = ((point_ax - tol_ax) - p_ax) + Jq_ax,   u = ((point_ax + tol_ax) - p_ax) + Jq_ax
 *   (the ball's radius does not enter: a goal is about the centre).  Always active: there is no margin.  A trajectory is
 *   accepted only if fabs(p_ax - point_ax) <= tol_ax + 1e-3 on every axis that is not free (a NaN fails).
 *   row 3, frame 0: zeros (written), l = -1e30, u = +1e30, no say in the verdict.
 *   row 3, frame >= 1: c and g_j exactly those of mi_gomp_tilt; the row holds g_j, l = (cos_lim - c) + sum_j g_j q_w[j],
 *     u = +1e30, always active; accepted only if c >= cos_ok, with cos_lim = cos(max_angle) and
 *     cos_ok = cos(min(pi, max_angle + 1e-3)) taken once on the host, in fp64, when the values are set.
 * Where the axis is exactly opposite to ref the row is all zeros with l = cos_lim + 1 > 0 and that QP is primal infeasible, as
 * for tilt limits: seed on the right side - linearise first around joints whose axis is not opposite to ref. */
typedef struct { int32_t ball; int32_t waypoint; int32_t frame; int32_t reserved; double axis[3]; } mi_gomp_goal;   /* 40 bytes */
typedef struct { double point[3]; double tol[3]; double ref[3]; double max_angle; } mi_gomp_goal_value;             /* 80 bytes */
/* mi_gomp_scene_create_grids with 0 .. 4 grasp goals besides.  The goal rows follow the tilt rows, goal-major: row r of goal k
 * is the first 3-D row + the rows of all ball blocks + waypoints * (n_pairs + n_tilts) + 4 k + r, so the constraint matrix must
 * hold 4 n_goals rows more, each with entries in the columns of its goal's waypoint.  n_goals == 0: exactly
 * mi_gomp_scene_create_grids.  Refused on the host, before any device call, with *out = NULL, the handle usable and the reason
 * in mi_osqp_last_error() naming the goal's index: n_goals > 0 without goals, a frame >= 1 without a chain (MI_OSQP_ERR_NULL);
 * n_goals outside 0 .. 4, a ball outside 0 .. n_balls - 1, a waypoint outside 0 .. waypoints - 1, a frame outside
 * 0 .. n_joints, an axis that is not finite or (frame >= 1) not a unit vector to 1e-9, a constraint matrix that does not hold
 * the rows (MI_OSQP_ERR_INVALID_DATA). */
int mi_gomp_scene_create_goals(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints, const mi_gomp_chain *chain,
        int64_t n_balls, const mi_gomp_ball *balls, int64_t n_lines, const mi_gomp_line *lines,
        int64_t n_capsules, const mi_gomp_capsule *capsules, int64_t n_cuboids, const mi_gomp_cuboid *cuboids,
        int64_t n_pairs, const mi_gomp_pair *pairs, int64_t n_tilts, const mi_gomp_tilt *tilts,
        int64_t n_grids, const mi_gomp_grid *grids, int64_t n_goals, const mi_gomp_goal *goals,
        const double *con_lo, const double *con_hi);
/* What the listed QPs ask of the scene's goals: values[j * n_goals + k] for goal k of QP ids[j], copied on the handle's stream
 * (also for idle QPs of a handle in the continuous mode).  Kept rows are not touched: the next mi_gomp_assemble_some /
 * mi_gomp_relinearise_some of such a QP reads the new values, and both refuse a QP of a goal scene whose values were never set
 * (MI_OSQP_ERR_INVALID_DATA).  Refused, with nothing changed: no scene, ids or values (MI_OSQP_ERR_NULL); a scene without
 * goals, an id outside 0 .. B - 1, a value that is not finite, a negative tol, and for a goal with frame >= 1 a ref that is not
 * a unit vector to 1e-9 or a max_angle outside (0, pi) (MI_OSQP_ERR_INVALID_DATA). */
int mi_gomp_scene_set_goal_values(mi_gomp_scene *sc, int64_t n_ids, const int64_t *ids, const mi_gomp_goal_value *values);
void mi_gomp_scene_free(mi_gomp_scene *sc);          /* before mi_osqp_batch_free of its handle; one scene per handle */
/* While a scene exists, mi_osqp_batch_reinit_some / _update_A_bounds_some of its handle also keep the QPs' raw constraint
 * data (as ConstraintBuilder::build() produced it) in the scene, so nothing extra is needed when a trajectory enters the
 * handle.  set_rows writes that copy directly ([n_ids][nnzA], [n_ids][m]); get_rows reads it back (tests). */
int mi_gomp_scene_set_rows(mi_gomp_scene *sc, int64_t n_ids, const int64_t *ids, const double *A_val, const double *l, const double *u);
int mi_gomp_scene_get_rows(mi_gomp_scene *sc, int64_t id, double *A_val, double *l, double *u);       /* (tests) */
/* withObstacles(con_3d, x) on the kept rows of the listed QPs (x: [n_ids][n] trajectories, host); ok_out[j] = isSolutionOK(x_j) */
int mi_gomp_assemble_some(mi_gomp_scene *sc, int64_t n_ids, const int64_t *ids, const double *x, int32_t *ok_out);
/* one SQP step of the listed, finished QPs ([REF] src/gomp-solver.h:79-87): ok_out[j] = isSolutionOK(x_j); the QPs whose
 * trajectory is not acceptable are re-linearised around it and updated (QPSolver::update from the device-resident rows)
 * and are ready for mi_osqp_batch_solve_begin_some */
int mi_gomp_relinearise_some(mi_gomp_scene *sc, int64_t n_ids, const int64_t *ids, const double *x, int32_t *ok_out);

/* ---------------------------------------------------------- multi-GPU batch
 * The batch is the shard axis across the GPUs of a node (the runs of a planner are independent,
 * [REF] src/gomp-solver.h:38-55): the B QPs are cut into n_devices contiguous blocks (the first B % n_devices one QP
 * longer), block k lives on HIP device devices[k] (devices == NULL: 0 .. n_devices-1; a device may be listed more than
 * once - two shards then share it), every call fans out over one long-lived worker thread + stream per shard and joins.  There is
 * no data-path collective; results come back QP-major in the order of the whole batch.  Arguments as for
 * mi_osqp_batch_*; the return value is the first shard error (0 = ok). */
typedef struct mi_osqp_multi mi_osqp_multi;
int mi_osqp_multi_batch_setup(mi_osqp_multi **out, int64_t n_devices, const int64_t *devices,
                              int64_t B, int64_t n, int64_t m,
                              const int64_t *P_colptr, const int64_t *P_rowidx, const double *P_val,
                              const double *q,
                              const int64_t *A_colptr, const int64_t *A_rowidx, const double *A_val,
                              const double *l, const double *u, const mi_osqp_settings *settings);
int mi_osqp_multi_batch_update_A(mi_osqp_multi *h, const int64_t *A_colptr, const int64_t *A_rowidx, const double *A_val);
int mi_osqp_multi_batch_update_bounds(mi_osqp_multi *h, const double *l, const double *u);
int mi_osqp_multi_batch_update_A_bounds(mi_osqp_multi *h, const int64_t *A_colptr, const int64_t *A_rowidx, const double *A_val,
                                        const double *l, const double *u);
int mi_osqp_multi_batch_warm_start_x(mi_osqp_multi *h, const double *x);
int mi_osqp_multi_batch_update_q(mi_osqp_multi *h, const double *q);                               /* osqp_update_lin_cost */
int mi_osqp_multi_batch_update_P(mi_osqp_multi *h, const int64_t *P_colptr, const int64_t *P_rowidx, const double *P_val);  /* osqp_update_P */
int mi_osqp_multi_batch_update_P_A(mi_osqp_multi *h, const int64_t *P_colptr, const int64_t *P_rowidx, const double *P_val,
                                   const int64_t *A_colptr, const int64_t *A_rowidx, const double *A_val);    /* osqp_update_P_A */
int mi_osqp_multi_batch_warm_start_y(mi_osqp_multi *h, const double *y);                           /* osqp_warm_start_y */
/* settings updates, fanned out per shard (all shards hold the same settings; a refusal changes no shard) */
int mi_osqp_multi_batch_get_settings(mi_osqp_multi *h, mi_osqp_settings *out);
int mi_osqp_multi_batch_update_settings(mi_osqp_multi *h, const mi_osqp_settings *s);
int mi_osqp_multi_batch_update_rho_each(mi_osqp_multi *h, const double *rho /*[B]*/);
int mi_osqp_multi_batch_solve(mi_osqp_multi *h);
/* The same without waiting (every shard has one long-lived worker thread; all calls of this section run on them): solve_async
 * returns once the shards have their job, wait() joins them and returns the first shard error.  Any other multi-batch call
 * joins a pending solve first. */
int mi_osqp_multi_batch_solve_async(mi_osqp_multi *h);
int mi_osqp_multi_batch_wait(mi_osqp_multi *h);
int mi_osqp_multi_batch_get_primal(mi_osqp_multi *h, double *x_out /*[B][n]*/);
int mi_osqp_multi_batch_get_dual(mi_osqp_multi *h, double *y_out /*[B][m]*/);
int mi_osqp_multi_batch_get_info(mi_osqp_multi *h, mi_osqp_info *info /*[B]*/);
int mi_osqp_multi_batch_get_prim_inf_cert(mi_osqp_multi *h, double *dy_out /*[B][m]*/);      /* see mi_osqp_batch_get_prim_inf_cert */
int mi_osqp_multi_batch_get_dual_inf_cert(mi_osqp_multi *h, double *dx_out /*[B][n]*/);
/* shard k: its device, its QP range [begin, end) and its single-device handle (owned by the multi handle) */
int64_t mi_osqp_multi_batch_shards(mi_osqp_multi *h);
int mi_osqp_multi_batch_shard(mi_osqp_multi *h, int64_t k, int64_t *device, int64_t *begin, int64_t *end, mi_osqp_batch **handle);
void mi_osqp_multi_batch_free(mi_osqp_multi *h);

/* ------------------------------------------------- the path's kernels as ops
 * (parity tests and roofline measurements call these; all pointers HBM)
 * KKT-structured SpMV on the scaled data: from x[B][n], y[B][m] compute
 * Px[B][n], Aty[B][n], Ax[B][m]  (rows E11/E14 of SURVEY 8(a)). */
int mi_osqp_batch_spmv(mi_osqp_batch *h, const double *d_x, const double *d_y,
                       double *d_Px, double *d_Aty, double *d_Ax, void *stream);
/* One KKT solve per QP with the current factor: sol = K^-1 rhs, [B][n+m]
 * (row E7: permute, level-scheduled L solve, D^-1, L' solve, un-permute). */
int mi_osqp_batch_kkt_solve(mi_osqp_batch *h, const double *d_rhs, double *d_sol, void *stream);
/* Row E13 as an op: rebuild every QP's KKT factor ON THE DEVICE from the current
 * scaled data and rho vector (batched block LDL'), scatter it into the solve
 * schedules.  solve() calls the same kernel for the QPs whose rho changed. */
int mi_osqp_batch_refactor_device(mi_osqp_batch *h);
/* average duration (ms) of the last `iterate` launches measured with HIP events
 * on the launch stream, and their count (bench.py's roofline leg). */
int mi_osqp_batch_kernel_time(mi_osqp_batch *h, double *avg_ms, int64_t *launches);
/* the same for the refactorisation kernels (row E13) since the last call: summed durations (ms, HIP events on the
 * launch stream) of factor_kernel and of dense_inverse_kernel, their launches and the QPs they refactored. */
int mi_osqp_batch_refactor_time(mi_osqp_batch *h, double *factor_ms, double *tail_ms, int64_t *launches, int64_t *qps);
/* the largest of those refactorisations (most QPs; a solve also holds small ones for stragglers): its QPs and the
 * durations of factor_kernel and of the dense-tail kernels (tail_assemble_kernel + tail_kernel). Reset by refactor_time. */
int mi_osqp_batch_refactor_peak(mi_osqp_batch *h, int64_t *qps, double *factor_ms, double *tail_ms);

/* The Ruiz scaling in force (all ones with scaling = 0), read from the device copies the kernels use: the scaled problem is
 * c D P D, c D q, E A D, E l, E u.  Ends the continuous mode like mi_osqp_batch_get_primal. */
int mi_osqp_batch_get_scaling(mi_osqp_batch *h, double *D /*[B][n]*/, double *E /*[B][m]*/, double *c /*[B]*/);

/* --------------------------------------------------- host-only diagnostics
 * No GPU needed: analyse a pattern + one value set and replay the DEVICE
 * schedules on the host (a sequential interpreter of the same task tables) so
 * that the schedule builder is testable in CPU-only CI.  Not a solve path. */
int mi_osqp_debug_host_kkt_solve(int64_t n, int64_t m,
                                 const int64_t *P_colptr, const int64_t *P_rowidx, const double *P_val,
                                 const int64_t *A_colptr, const int64_t *A_rowidx, const double *A_val,
                                 const double *l, const double *u, const mi_osqp_settings *settings,
                                 int64_t tile, const double *rhs /*[n+m], scaled space*/,
                                 double *sol_schedule /*[n+m]*/, double *sol_direct /*[n+m]*/,
                                 mi_osqp_stats *st);

/* Host interpreter of the DEVICE block refactorisation (row E13) against the
 * host left-looking factor: max relative differences of L and D^-1, and
 * counts[4] = {blocks, triples, storage doubles per QP, levels}. */
int mi_osqp_debug_host_block_factor(int64_t n, int64_t m,
                                    const int64_t *P_colptr, const int64_t *P_rowidx, const double *P_val,
                                    const int64_t *A_colptr, const int64_t *A_rowidx, const double *A_val,
                                    const double *l, const double *u, const mi_osqp_settings *settings,
                                    double *max_rel_diff_L, double *max_rel_diff_Dinv, int64_t *counts);

/* Host only: the chunks of a pipelined refactorisation (solver.hip "pipelined refactorisation").  flagged / active: the
 * slots (tile * `tile` + b, ascending) that get a new factor / iterate on; chunk_qps flagged slots per chunk, at most
 * max_chunks refactorisation chunks.  Out: *n_chunks (chunk 0 = tiles without a flagged slot), work_begin[n_chunks + 1]
 * (chunk c refactors flagged[work_begin[c] .. work_begin[c + 1])), tiles[<= n_active] (the active tiles chunk after
 * chunk) and tile_begin[n_chunks + 1]; work_begin / tile_begin hold max_chunks + 2 entries. */
int mi_osqp_debug_refactor_chunks(int64_t n_flagged, const int64_t *flagged, int64_t n_active, const int64_t *active, int64_t tile,
                                  int64_t chunk_qps, int64_t max_chunks, int64_t *n_chunks, int64_t *work_begin, int64_t *tiles,
                                  int64_t *tile_begin);

/* Host only: the default chunk size of a pipelined region (neither MI_OSQP_REFACTOR_CHUNKS nor MI_OSQP_REFACTOR_CHUNK_QPS set;
 * host_core.hpp region_chunk_qps).  nq = flagged slots of the region's work list, gw = flagged slots of the run-ahead chain
 * that refactors beside it (0 without run-ahead), n_cus = CUs.  Out: *chunk_qps = ceil(nq / n_even) with rounds =
 * ceil((nq + gw) / n_cus) and n_even = rounds (gw = 0) or 2 rounds - 1 (gw > 0) even chunks, at most 8 and at most nq of
 * them, and *n_chunks = the refactorisation chunks that gives, ceil(nq / chunk_qps) (0 for nq = 0). */
int mi_osqp_debug_region_chunks(int64_t nq, int64_t gw, int64_t n_cus, int64_t *chunk_qps, int64_t *n_chunks);

/* Host only: the chunk lanes of those chunks (MI_OSQP_REFACTOR_LANES; solver.hip "pipelined refactorisation").  kbt = slots
 * per workgroup of the refactorisation kernels, lanes = 1 .. 3, chunk0_first = chunk 0 in front of the last lane instead of
 * behind the shortest one, scratch_slots = slots the refactorisation scratch holds (too few: one lane).  Out: *n_lanes,
 * lane_of[n_chunks], order[n_chunks] (the chunks lane after lane in launch order) with order_begin[n_lanes + 1],
 * scratch_begin[n_chunks] (first scratch slot of every chunk) and *n_waits pairs: the iterate of chunk wait_chunk[i] waits
 * for the tail of chunk wait_for[i] on another lane.  Per-chunk arrays hold max_chunks + 2 entries, order_begin 4, the
 * wait arrays (max_chunks + 1)^2. */
int mi_osqp_debug_refactor_lanes(int64_t n_flagged, const int64_t *flagged, int64_t n_active, const int64_t *active, int64_t tile,
                                 int64_t chunk_qps, int64_t max_chunks, int64_t kbt, int64_t lanes, int64_t chunk0_first,
                                 int64_t scratch_slots, int64_t *n_lanes, int64_t *lane_of, int64_t *order, int64_t *order_begin,
                                 int64_t *scratch_begin, int64_t *n_waits, int64_t *wait_chunk, int64_t *wait_for);

/* Host only: the run-ahead group of a rho-update point (MI_OSQP_RUNAHEAD; host_core.hpp runahead_group).  tiles[n_active] = the
 * active tiles (no tile twice), pri_res / dua_res = their residuals (>= 0 or NaN) of the check that has just run, size = tiles
 * of the group, min_active = no group when fewer tiles are active.  Out: *n_group and group[<= min(size, n_active)], in
 * descending score pri / median(pri) + dua / median(dua), ties by ascending tile. */
int mi_osqp_debug_runahead_group(int64_t n_active, const int64_t *tiles, const double *pri_res, const double *dua_res, int64_t size,
                                 int64_t min_active, int64_t *n_group, int64_t *group);

/* Host only: the form of the resident head of S^-1 one iterate launch takes (host_core.hpp iterate_form).  tiles = tiles the
 * launch iterates, has_head = the handle keeps a head, forced_form = MI_OSQP_RF_FORM (0 none, 1 deep ring, 2 long head),
 * long_min = MI_OSQP_RF_LONG_MIN (-1 = the default, 0).  Out: *form = 0 streamed, 1 deep ring, 2 long head. */
int mi_osqp_debug_iterate_form(int64_t tiles, int64_t has_head, int64_t forced_form, int64_t long_min, int64_t *form);

/* Host only: whether the resident iterate of a handle keeps its index words in registers (host_core.hpp index_words_fit;
 * mi_osqp_stats::resident_index_words without MI_OSQP_INDEX_LOADS).  resident_state / lds_vector = the handle keeps the ADMM
 * state in LDS / its solve vector in LDS, tile = QPs per tile, threads = threads per tile, n / m = variables / constraints.
 * Out: *fit = 1 when (n + m) * tile <= *xloc_trips * threads and n * tile, m * tile <= *pinv_trips * threads, and the two
 * caps (trips of a thread through xloc / through either kind of pinv row). */
int mi_osqp_debug_index_words_fit(int64_t resident_state, int64_t lds_vector, int64_t tile, int64_t threads, int64_t n, int64_t m,
                                  int64_t *fit, int64_t *xloc_trips, int64_t *pinv_trips);

/* Device diagnostics (tile 2, LDS mode only): one KKT solve of the whole batch with
 * per-phase / per-wave shader-clock stamps of two tiles (first, middle).
 * which = 0: run the traced solve; trace receives 2 * dims[3] words (see kkt_trace_kernel).
 * which = 1 / 2: copy the forward / backward phase table (dims[0|1] rows of 4*dims[2]+1 words) instead.
 * dims[4] = {forward phases, backward phases, waves per tile, trace words per tile}. */
int mi_osqp_debug_trace_kkt_solve(mi_osqp_batch *h, int32_t which, const double *d_rhs, double *d_sol,
                                  uint32_t *out, int64_t out_capacity_words, int64_t *dims);

#ifdef __cplusplus
}
#endif
#endif /* MI_OSQP_H */
