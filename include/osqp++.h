// osqp++.h -- the subset of google/osqp-cpp's header that ZPP-Robotics/OSQP-Solver compiles against, implemented on the
// C-ABI of the MI355X-native core (mi_osqp.h) instead of the osqp C library.
//
// Put this directory in front of the include path and link libmi_osqp.so: the reference's headers then compile
// UNCHANGED -- [REF] src/utils.h:7,11 (`#include <osqp++.h>`, `using ExitCode = osqp::OsqpExitCode`),
// src/constraints/constraint-builder.h:10, src/osqp-wrapper.h:6,18-28,36,40,46,52-53, examples/solver-example.cpp:71,94
// (`ToString(exit_code)`).  Like upstream's header this one pulls in Eigen (the reference relies on that for
// Eigen::SparseMatrix / VectorXd / Triplet, [REF] src/utils.h:12-20) and a Status type under namespace absl.
//
// What is provided, and which reference line uses it:
//   osqp::OsqpInstance  {objective_matrix, objective_vector, constraint_matrix, lower_bounds, upper_bounds}   [REF] osqp-wrapper.h:18-24
//   osqp::OsqpSettings  (every field of osqp-cpp's struct; the reference sets only `verbose`)                 [REF] osqp-wrapper.h:26-27
//   osqp::OsqpSolver::Init / UpdateConstraintMatrix / SetBounds / SetPrimalWarmStart / Solve / primal_solution [REF] :28,36,40,46,52,53
//   absl::Status::ok / ToString                                                                               [REF] :30,34-48
//   osqp::OsqpExitCode, osqp::ToString                                                                        [REF] utils.h:11; gomp-solver.h:40,46-49,68,72,79
// plus dual_solution / iterations / objective_value / IsInitialized, and the objective updates and warm starts the reference
// does not call: SetObjectiveVector, UpdateObjectiveMatrix, UpdateObjectiveAndConstraintMatrices, SetDualWarmStart and
// SetWarmStart(x, y) (C-ABI mi_osqp_update_q / _update_P / _update_P_A / _warm_start_y; README "Objective updates").
// Statuses as upstream: kFailedPrecondition before a successful Init, kInvalidArgument for a wrong length or shape or a
// changed sparsity pattern (the core extracts the upper triangle of an objective matrix given with both).
//
// The fourteen settings updates of osqp-cpp - UpdateRho, UpdateMaxIter, UpdateEpsAbs, UpdateEpsRel, UpdateEpsPrimInf,
// UpdateEpsDualInf, UpdateAlpha, UpdateDelta, UpdatePolish, UpdatePolishRefineIter, UpdateWarmStart, UpdateScaledTermination,
// UpdateCheckTermination, UpdateTimeLimit - go through mi_osqp_get_settings / mi_osqp_update_settings (README "Settings
// updates"): kFailedPrecondition before a successful Init, kInvalidArgument for a value the core refuses (nothing changes).
// UpdateRho refactors the KKT matrix on the device; the others take effect at the next Solve.  UpdateTimeLimit validates
// (>= 0) and stores the value, which is then ignored like the time_limit given to Init.
//
// primal_infeasibility_certificate() / dual_infeasibility_certificate() return, after a Solve() that ended kPrimalInfeasible(Inaccurate)
// / kDualInfeasible(Inaccurate), the certificate with unit infinity norm (mi_osqp_get_prim_inf_cert / _dual_inf_cert; README
// "Infeasibility certificates"); after any other Solve() - and before the first - every entry is NaN.
//
// polish, polish_refine_iter and delta map onto the core's solution polishing (mi_osqp_settings, README "Polishing").
// Settings that the MI355X core does not implement are validated like upstream and otherwise ignored: time_limit,
// adaptive_rho_fraction (the wall-clock rule; the deterministic interval 4 * check_termination stands in for "auto",
// DESIGN.md section 2).
#ifndef MI_OSQP_OSQPPP_SHIM_H_
#define MI_OSQP_OSQPPP_SHIM_H_

#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#if !__has_include(<Eigen/Sparse>)
#error "osqp++.h (mi_osqp shim): Eigen is required, exactly as for google/osqp-cpp's own header - add Eigen to the include path"
#endif
#include <Eigen/Core>
#include <Eigen/Sparse>

#include "mi_osqp.h"

// ---- absl::Status: the real one when abseil is on the include path, else the few members the reference touches
#if __has_include("absl/status/status.h")
#include "absl/status/status.h"
#define MI_OSQP_SHIM_STATUS(code, msg) ::absl::Status(::absl::StatusCode::code, msg)
#define MI_OSQP_SHIM_OK() ::absl::OkStatus()
#else
namespace absl {
enum class StatusCode : int { kOk = 0, kUnknown = 2, kInvalidArgument = 3, kFailedPrecondition = 9, kUnimplemented = 12 };
class Status {
 public:
  Status() = default;
  Status(StatusCode code, std::string msg) : code_(code), msg_(std::move(msg)) {}
  bool ok() const { return code_ == StatusCode::kOk; }
  StatusCode code() const { return code_; }
  const std::string &message() const { return msg_; }
  std::string ToString() const {
    if (ok()) return "OK";
    const char *n = code_ == StatusCode::kInvalidArgument ? "INVALID_ARGUMENT"
                  : code_ == StatusCode::kFailedPrecondition ? "FAILED_PRECONDITION"
                  : code_ == StatusCode::kUnimplemented ? "UNIMPLEMENTED" : "UNKNOWN";
    return std::string(n) + ": " + msg_;
  }
 private:
  StatusCode code_ = StatusCode::kOk;
  std::string msg_;
};
inline Status OkStatus() { return Status(); }
}  // namespace absl
#define MI_OSQP_SHIM_STATUS(code, msg) ::absl::Status(::absl::StatusCode::code, msg)
#define MI_OSQP_SHIM_OK() ::absl::Status()
#endif

namespace osqp {

using c_int = long long;            // OSQP built with DLONG, which is what Eigen::SparseMatrix<.., long long> of the reference needs

struct OsqpInstance {
  c_int num_variables() const { return static_cast<c_int>(objective_vector.size()); }
  c_int num_constraints() const { return static_cast<c_int>(lower_bounds.size()); }
  Eigen::SparseMatrix<double, Eigen::ColMajor, c_int> objective_matrix;     // upper triangle is used (both may be given)
  Eigen::VectorXd objective_vector;
  Eigen::SparseMatrix<double, Eigen::ColMajor, c_int> constraint_matrix;
  Eigen::VectorXd lower_bounds;
  Eigen::VectorXd upper_bounds;
};

struct OsqpSettings {               // defaults = osqp 0.6.x (osqp_set_default_settings)
  double rho = 0.1;
  double sigma = 1e-6;
  c_int scaling = 10;
  bool adaptive_rho = true;
  c_int adaptive_rho_interval = 0;
  double adaptive_rho_tolerance = 5.0;
  double adaptive_rho_fraction = 0.4;
  c_int max_iter = 4000;
  double eps_abs = 1e-3;
  double eps_rel = 1e-3;
  double eps_prim_inf = 1e-4;
  double eps_dual_inf = 1e-4;
  double alpha = 1.6;
  double delta = 1e-6;
  bool polish = false;
  c_int polish_refine_iter = 3;
  bool verbose = true;
  bool scaled_termination = false;
  c_int check_termination = 25;
  bool warm_start = true;
  double time_limit = 0.0;
};

enum class OsqpExitCode {
  kOptimal, kPrimalInfeasible, kDualInfeasible, kOptimalInaccurate, kPrimalInfeasibleInaccurate,
  kDualInfeasibleInaccurate, kMaxIterations, kInterrupted, kTimeLimitReached, kNonConvex, kUnknown,
};
inline std::string ToString(OsqpExitCode exitcode) { return mi_osqp_exit_code_name(static_cast<int64_t>(exitcode)); }

class OsqpSolver {
 public:
  OsqpSolver() = default;
  OsqpSolver(OsqpSolver &&o) noexcept { *this = std::move(o); }
  OsqpSolver &operator=(OsqpSolver &&o) noexcept {
    if (this != &o) { reset(); h_ = o.h_; n_ = o.n_; m_ = o.m_; x_ = std::move(o.x_); y_ = std::move(o.y_); pcert_ = std::move(o.pcert_); dcert_ = std::move(o.dcert_); info_ = o.info_; time_limit_ = o.time_limit_; o.h_ = nullptr; }
    return *this;
  }
  OsqpSolver(const OsqpSolver &) = delete;
  OsqpSolver &operator=(const OsqpSolver &) = delete;
  ~OsqpSolver() { reset(); }

  // osqp_setup: validates, copies the data (the caller's instance may die right after, [REF] osqp-wrapper.h:18-31),
  // equilibrates, orders and factors the KKT matrix, uploads everything to the GPU.
  absl::Status Init(const OsqpInstance &instance, const OsqpSettings &settings) {
    reset();
    const c_int n = instance.num_variables(), m = instance.num_constraints();
    if (n <= 0) return MI_OSQP_SHIM_STATUS(kInvalidArgument, "The number of variables must be positive");
    if (instance.objective_matrix.rows() != n || instance.objective_matrix.cols() != n ||
        instance.constraint_matrix.rows() != m || instance.constraint_matrix.cols() != n || instance.upper_bounds.size() != m)
      return MI_OSQP_SHIM_STATUS(kInvalidArgument, "The dimensions of the objective / constraint data do not agree");
    Eigen::SparseMatrix<double, Eigen::ColMajor, c_int> P = instance.objective_matrix, A = instance.constraint_matrix;
    P.makeCompressed(); A.makeCompressed();
    mi_osqp_settings s;
    mi_osqp_default_settings(&s);
    s.rho = settings.rho; s.sigma = settings.sigma; s.scaling = settings.scaling; s.adaptive_rho = settings.adaptive_rho;
    s.adaptive_rho_interval = settings.adaptive_rho_interval; s.adaptive_rho_tolerance = settings.adaptive_rho_tolerance;
    s.max_iter = settings.max_iter; s.eps_abs = settings.eps_abs; s.eps_rel = settings.eps_rel;
    s.eps_prim_inf = settings.eps_prim_inf; s.eps_dual_inf = settings.eps_dual_inf; s.alpha = settings.alpha;
    s.scaled_termination = settings.scaled_termination; s.check_termination = settings.check_termination;
    s.warm_start = settings.warm_start; s.verbose = settings.verbose;
    s.polish = settings.polish ? 1 : 0; s.polish_refine_iter = settings.polish_refine_iter; s.delta = settings.delta;
    static_assert(sizeof(c_int) == sizeof(int64_t), "CSC index width");
    const int rc = mi_osqp_setup(&h_, n, m, reinterpret_cast<const int64_t *>(P.outerIndexPtr()),
                                 reinterpret_cast<const int64_t *>(P.innerIndexPtr()), P.valuePtr(), instance.objective_vector.data(),
                                 reinterpret_cast<const int64_t *>(A.outerIndexPtr()), reinterpret_cast<const int64_t *>(A.innerIndexPtr()),
                                 A.valuePtr(), instance.lower_bounds.data(), instance.upper_bounds.data(), &s);
    if (rc != MI_OSQP_OK) { h_ = nullptr; return from_error(rc, "osqp_setup"); }
    n_ = n; m_ = m;
    x_.assign(static_cast<size_t>(n), 0.0); y_.assign(static_cast<size_t>(m), 0.0);
    pcert_.assign(static_cast<size_t>(m), kNaN); dcert_.assign(static_cast<size_t>(n), kNaN);
    return MI_OSQP_SHIM_OK();
  }
  bool IsInitialized() const { return h_ != nullptr; }

  // osqp_solve + the copy-out of the solution; never throws ([REF] osqp-wrapper.h:51-54)
  OsqpExitCode Solve() {
    if (!h_) return OsqpExitCode::kUnknown;
    pcert_.assign(static_cast<size_t>(m_), kNaN); dcert_.assign(static_cast<size_t>(n_), kNaN);      // (also where the solve fails)
    last_error_ = mi_osqp_solve(h_, &info_);
    if (last_error_ != MI_OSQP_OK) {
      // osqp-cpp turns a failing osqp_solve into kUnknown, which the reference's driver reads as "not converged, go on"
      // ([REF] src/gomp-solver.h:44-51): a device fault must not pass as that silently
      std::fprintf(stderr, "OsqpSolver::Solve: %s (%s)\n", mi_osqp_error_name(last_error_), mi_osqp_last_error());
      return last_error_ == MI_OSQP_ERR_NONCONVEX ? OsqpExitCode::kNonConvex : OsqpExitCode::kUnknown;
    }
    mi_osqp_get_primal(h_, x_.data());
    if (m_) mi_osqp_get_dual(h_, y_.data());
    // (the certificates are read only when there is one: an exit with a solution costs no further copy)
    const OsqpExitCode code = static_cast<OsqpExitCode>(info_.exit_code);
    if (code == OsqpExitCode::kPrimalInfeasible || code == OsqpExitCode::kPrimalInfeasibleInaccurate) mi_osqp_get_prim_inf_cert(h_, pcert_.data());
    if (code == OsqpExitCode::kDualInfeasible || code == OsqpExitCode::kDualInfeasibleInaccurate) mi_osqp_get_dual_inf_cert(h_, dcert_.data());
    return code;
  }
  int last_error() const { return last_error_; }        // mi_osqp_error of the last Solve() (not part of osqp-cpp)
  c_int iterations() const { return info_.iter; }
  double objective_value() const { return info_.obj_val; }
  Eigen::Map<const Eigen::VectorXd> primal_solution() const { return Eigen::Map<const Eigen::VectorXd>(x_.data(), n_); }
  Eigen::Map<const Eigen::VectorXd> dual_solution() const { return Eigen::Map<const Eigen::VectorXd>(y_.data(), m_); }
  // delta_y / delta_x of the last Solve() with unit infinity norm, NaN where that Solve() proved no infeasibility of the kind
  Eigen::Map<const Eigen::VectorXd> primal_infeasibility_certificate() const { return Eigen::Map<const Eigen::VectorXd>(pcert_.data(), m_); }
  Eigen::Map<const Eigen::VectorXd> dual_infeasibility_certificate() const { return Eigen::Map<const Eigen::VectorXd>(dcert_.data(), n_); }

  absl::Status SetPrimalWarmStart(const Eigen::Ref<const Eigen::VectorXd> &primal_vector) {
    if (!h_) return not_initialized();
    if (primal_vector.size() != n_) return MI_OSQP_SHIM_STATUS(kInvalidArgument, "The warm start has the wrong length");
    const Eigen::VectorXd x = primal_vector;                    // (a Ref may be strided)
    return from_error(mi_osqp_warm_start_x(h_, x.data()), "osqp_warm_start_x");
  }
  absl::Status SetBounds(const Eigen::Ref<const Eigen::VectorXd> &lower_bounds, const Eigen::Ref<const Eigen::VectorXd> &upper_bounds) {
    if (!h_) return not_initialized();
    if (lower_bounds.size() != m_ || upper_bounds.size() != m_) return MI_OSQP_SHIM_STATUS(kInvalidArgument, "The bounds have the wrong length");
    const Eigen::VectorXd l = lower_bounds, u = upper_bounds;
    return from_error(mi_osqp_update_bounds(h_, l.data(), u.data()), "osqp_update_bounds");
  }
  absl::Status UpdateConstraintMatrix(const Eigen::SparseMatrix<double, Eigen::ColMajor, c_int> &constraint_matrix) {
    if (!h_) return not_initialized();
    if (constraint_matrix.rows() != m_ || constraint_matrix.cols() != n_)
      return MI_OSQP_SHIM_STATUS(kInvalidArgument, "The constraint matrix has the wrong shape");
    Eigen::SparseMatrix<double, Eigen::ColMajor, c_int> A = constraint_matrix;
    A.makeCompressed();
    return from_error(mi_osqp_update_A(h_, reinterpret_cast<const int64_t *>(A.outerIndexPtr()),
                                       reinterpret_cast<const int64_t *>(A.innerIndexPtr()), A.valuePtr()), "osqp_update_A");
  }
  // objective updates and dual warm starts (the reference uses none of them)
  absl::Status SetDualWarmStart(const Eigen::Ref<const Eigen::VectorXd> &dual_vector) {
    if (!h_) return not_initialized();
    if (dual_vector.size() != m_) return MI_OSQP_SHIM_STATUS(kInvalidArgument, "The dual warm start has the wrong length");
    const Eigen::VectorXd y = dual_vector;
    return from_error(mi_osqp_warm_start_y(h_, y.data()), "osqp_warm_start_y");
  }
  absl::Status SetWarmStart(const Eigen::Ref<const Eigen::VectorXd> &primal_vector, const Eigen::Ref<const Eigen::VectorXd> &dual_vector) {
    if (!h_) return not_initialized();
    if (primal_vector.size() != n_ || dual_vector.size() != m_) return MI_OSQP_SHIM_STATUS(kInvalidArgument, "The warm start has the wrong length");
    const absl::Status sx = SetPrimalWarmStart(primal_vector);
    if (!sx.ok()) return sx;
    return SetDualWarmStart(dual_vector);
  }
  absl::Status SetObjectiveVector(const Eigen::Ref<const Eigen::VectorXd> &objective_vector) {
    if (!h_) return not_initialized();
    if (objective_vector.size() != n_) return MI_OSQP_SHIM_STATUS(kInvalidArgument, "The objective vector has the wrong length");
    const Eigen::VectorXd q = objective_vector;
    return from_error(mi_osqp_update_q(h_, q.data()), "osqp_update_lin_cost");
  }
  absl::Status UpdateObjectiveMatrix(const Eigen::SparseMatrix<double, Eigen::ColMajor, c_int> &objective_matrix) {
    if (!h_) return not_initialized();
    if (objective_matrix.rows() != n_ || objective_matrix.cols() != n_)
      return MI_OSQP_SHIM_STATUS(kInvalidArgument, "The objective matrix has the wrong shape");
    Eigen::SparseMatrix<double, Eigen::ColMajor, c_int> P = objective_matrix;
    P.makeCompressed();
    return from_error(mi_osqp_update_P(h_, reinterpret_cast<const int64_t *>(P.outerIndexPtr()),
                                       reinterpret_cast<const int64_t *>(P.innerIndexPtr()), P.valuePtr()), "osqp_update_P");
  }
  absl::Status UpdateObjectiveAndConstraintMatrices(const Eigen::SparseMatrix<double, Eigen::ColMajor, c_int> &objective_matrix,
                                                    const Eigen::SparseMatrix<double, Eigen::ColMajor, c_int> &constraint_matrix) {
    if (!h_) return not_initialized();
    if (objective_matrix.rows() != n_ || objective_matrix.cols() != n_)
      return MI_OSQP_SHIM_STATUS(kInvalidArgument, "The objective matrix has the wrong shape");
    if (constraint_matrix.rows() != m_ || constraint_matrix.cols() != n_)
      return MI_OSQP_SHIM_STATUS(kInvalidArgument, "The constraint matrix has the wrong shape");
    Eigen::SparseMatrix<double, Eigen::ColMajor, c_int> P = objective_matrix, A = constraint_matrix;
    P.makeCompressed(); A.makeCompressed();
    return from_error(mi_osqp_update_P_A(h_, reinterpret_cast<const int64_t *>(P.outerIndexPtr()),
                                         reinterpret_cast<const int64_t *>(P.innerIndexPtr()), P.valuePtr(),
                                         reinterpret_cast<const int64_t *>(A.outerIndexPtr()),
                                         reinterpret_cast<const int64_t *>(A.innerIndexPtr()), A.valuePtr()), "osqp_update_P_A");
  }
  // settings updates (osqp_update_*): get the settings in force, change one field, update
  absl::Status UpdateRho(double rho_new) { return update_setting("osqp_update_rho", [&](mi_osqp_settings &s) { s.rho = rho_new; }); }
  absl::Status UpdateMaxIter(int max_iter_new) { return update_setting("osqp_update_max_iter", [&](mi_osqp_settings &s) { s.max_iter = max_iter_new; }); }
  absl::Status UpdateEpsAbs(double eps_abs_new) { return update_setting("osqp_update_eps_abs", [&](mi_osqp_settings &s) { s.eps_abs = eps_abs_new; }); }
  absl::Status UpdateEpsRel(double eps_rel_new) { return update_setting("osqp_update_eps_rel", [&](mi_osqp_settings &s) { s.eps_rel = eps_rel_new; }); }
  absl::Status UpdateEpsPrimInf(double eps_prim_inf_new) { return update_setting("osqp_update_eps_prim_inf", [&](mi_osqp_settings &s) { s.eps_prim_inf = eps_prim_inf_new; }); }
  absl::Status UpdateEpsDualInf(double eps_dual_inf_new) { return update_setting("osqp_update_eps_dual_inf", [&](mi_osqp_settings &s) { s.eps_dual_inf = eps_dual_inf_new; }); }
  absl::Status UpdateAlpha(double alpha_new) { return update_setting("osqp_update_alpha", [&](mi_osqp_settings &s) { s.alpha = alpha_new; }); }
  absl::Status UpdateDelta(double delta_new) { return update_setting("osqp_update_delta", [&](mi_osqp_settings &s) { s.delta = delta_new; }); }
  absl::Status UpdatePolish(bool polish_new) { return update_setting("osqp_update_polish", [&](mi_osqp_settings &s) { s.polish = polish_new ? 1 : 0; }); }
  absl::Status UpdatePolishRefineIter(int polish_refine_iter_new) { return update_setting("osqp_update_polish_refine_iter", [&](mi_osqp_settings &s) { s.polish_refine_iter = polish_refine_iter_new; }); }
  absl::Status UpdateWarmStart(bool warm_start_new) { return update_setting("osqp_update_warm_start", [&](mi_osqp_settings &s) { s.warm_start = warm_start_new ? 1 : 0; }); }
  absl::Status UpdateScaledTermination(bool scaled_termination_new) { return update_setting("osqp_update_scaled_termination", [&](mi_osqp_settings &s) { s.scaled_termination = scaled_termination_new ? 1 : 0; }); }
  absl::Status UpdateCheckTermination(c_int check_termination_new) { return update_setting("osqp_update_check_termination", [&](mi_osqp_settings &s) { s.check_termination = check_termination_new; }); }
  absl::Status UpdateTimeLimit(double time_limit_new) {
    if (!h_) return not_initialized();
    if (!(time_limit_new >= 0.0)) return MI_OSQP_SHIM_STATUS(kInvalidArgument, "osqp_update_time_limit: time_limit must be nonnegative");
    time_limit_ = time_limit_new;           // (stored, not enforced: the core has no wall-clock rule)
    return MI_OSQP_SHIM_OK();
  }

 private:
  template <class F>
  absl::Status update_setting(const char *where, F &&change) {
    if (!h_) return not_initialized();
    mi_osqp_settings s;
    const int rc = mi_osqp_get_settings(h_, &s);
    if (rc != MI_OSQP_OK) return from_error(rc, where);
    change(s);
    return from_error(mi_osqp_update_settings(h_, &s), where);
  }
  void reset() { if (h_) mi_osqp_free(h_); h_ = nullptr; n_ = m_ = 0; }
  static absl::Status not_initialized() { return MI_OSQP_SHIM_STATUS(kFailedPrecondition, "OsqpSolver is not initialized."); }
  static absl::Status from_error(int rc, const char *where) {
    if (rc == MI_OSQP_OK) return MI_OSQP_SHIM_OK();
    std::string msg = std::string(where) + ": " + mi_osqp_error_name(rc);
    const char *extra = mi_osqp_last_error();
    if (extra && *extra && (rc == MI_OSQP_ERR_DEVICE || rc == MI_OSQP_ERR_ALLOC)) msg += std::string(" (") + extra + ")";
    if (rc == MI_OSQP_ERR_INVALID_DATA || rc == MI_OSQP_ERR_INVALID_SETTINGS || rc == MI_OSQP_ERR_PATTERN_CHANGED || rc == MI_OSQP_ERR_NONCONVEX)
      return MI_OSQP_SHIM_STATUS(kInvalidArgument, msg);      // what osqp-cpp reports for rejected data / a changed sparsity pattern
    return MI_OSQP_SHIM_STATUS(kUnknown, msg);
  }
  mi_osqp_solver *h_ = nullptr;
  c_int n_ = 0, m_ = 0;
  static constexpr double kNaN = __builtin_nan("");
  std::vector<double> x_, y_, pcert_, dcert_;
  mi_osqp_info info_{};
  int last_error_ = 0;
  double time_limit_ = 0.0;
};

}  // namespace osqp

#endif  // MI_OSQP_OSQPPP_SHIM_H_
