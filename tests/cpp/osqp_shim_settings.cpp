// include/osqp++.h settings updates: the fourteen Update* methods of osqp-cpp.
// First all of them on an uninitialised solver (osqp-cpp answers FAILED_PRECONDITION), then, where Init succeeds:
// Init, Solve, UpdateEpsAbs(1e-6), UpdateEpsRel(1e-6), UpdateMaxIter(3000), UpdateRho(0.7), Solve, and values the core refuses
// (INVALID_ARGUMENT, nothing changed: one more Solve from the same warm start must then take 0 < iterations).  Output: one
// line of JSON that tests/test_settings_update_abi.py and tests/test_gpu_settings_update.py read.
#include <cmath>
#include <cstdio>
#include <iostream>
#include <string>

#include <osqp++.h>

using Sparse = Eigen::SparseMatrix<double, Eigen::ColMajor, long long>;

static Sparse from_dense(int rows, int cols, const double *a) {
  std::vector<Eigen::Triplet<double, long long>> t;
  for (int c = 0; c < cols; c++) for (int r = 0; r < rows; r++) if (a[r * cols + c] != 0.0) t.emplace_back(r, c, a[r * cols + c]);
  Sparse M(rows, cols);
  M.setFromTriplets(t.begin(), t.end());
  return M;
}

static std::string vec(const Eigen::VectorXd &x) {
  std::string s = "[";
  char buf[40];
  for (Eigen::Index i = 0; i < x.size(); i++) { std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", x[i]); s += buf; }
  return s + "]";
}

static std::string head(const absl::Status &s) { const std::string t = s.ToString(); return t.substr(0, t.find(':')); }

static std::string all_updates(osqp::OsqpSolver &s) {
  const absl::Status st[14] = {s.UpdateRho(0.2), s.UpdateMaxIter(100), s.UpdateEpsAbs(1e-4), s.UpdateEpsRel(1e-4), s.UpdateEpsPrimInf(1e-5),
                               s.UpdateEpsDualInf(1e-5), s.UpdateAlpha(1.5), s.UpdateDelta(1e-7), s.UpdatePolish(false),
                               s.UpdatePolishRefineIter(2), s.UpdateWarmStart(true), s.UpdateScaledTermination(false),
                               s.UpdateCheckTermination(25), s.UpdateTimeLimit(1.0)};
  std::string json = "[";
  for (int k = 0; k < 14; k++) json += std::string(k ? ", " : "") + "\"" + head(st[k]) + "\"";
  return json + "]";
}

int main() {
  const double Pd[4] = {4, 1, 1, 2}, Ad[6] = {1, 1, 1, 0, 0, 1};
  const Sparse P = from_dense(2, 2, Pd), A = from_dense(3, 2, Ad);
  Eigen::VectorXd l(3), u(3), q0(2);
  l[0] = 1; l[1] = 0; l[2] = 0; u[0] = 1; u[1] = 0.7; u[2] = 0.7;
  q0[0] = 1; q0[1] = 1;

  // ---- before Init
  osqp::OsqpSolver fresh;
  const std::string pre_json = all_updates(fresh);

  // ---- the sequence
  osqp::OsqpInstance instance;
  instance.objective_matrix = P; instance.constraint_matrix = A; instance.objective_vector = q0;
  instance.lower_bounds = l; instance.upper_bounds = u;
  osqp::OsqpSettings settings;
  settings.verbose = false;
  osqp::OsqpSolver solver;
  const absl::Status init = solver.Init(instance, settings);
  std::cout << "Init: " << init.ToString() << std::endl;
  std::string body;
  if (init.ok()) {
    const osqp::OsqpExitCode c1 = solver.Solve();
    const long long it1 = solver.iterations();
    const Eigen::VectorXd x1 = solver.primal_solution();
    const absl::Status s_up[4] = {solver.UpdateEpsAbs(1e-6), solver.UpdateEpsRel(1e-6), solver.UpdateMaxIter(3000), solver.UpdateRho(0.7)};
    const osqp::OsqpExitCode c2 = solver.Solve();
    const long long it2 = solver.iterations();
    const Eigen::VectorXd x2 = solver.primal_solution(), y2 = solver.dual_solution();
    const absl::Status s_bad[6] = {solver.UpdateRho(0.0), solver.UpdateRho(std::nan("")), solver.UpdateAlpha(2.0), solver.UpdateMaxIter(0),
                                   solver.UpdateDelta(0.0), solver.UpdateTimeLimit(-1.0)};
    const osqp::OsqpExitCode c3 = solver.Solve();
    const long long it3 = solver.iterations();
    char buf[512];
    std::snprintf(buf, sizeof buf, ", \"codes\": [\"%s\", \"%s\", \"%s\"], \"iters\": [%lld, %lld, %lld], ", osqp::ToString(c1).c_str(),
                  osqp::ToString(c2).c_str(), osqp::ToString(c3).c_str(), it1, it2, it3);
    body = buf;
    body += "\"x1\": " + vec(x1) + ", \"x2\": " + vec(x2) + ", \"y2\": " + vec(y2);
    body += ", \"status\": [";
    for (int k = 0; k < 4; k++) body += std::string(k ? ", " : "") + "\"" + s_up[k].ToString() + "\"";
    body += "], \"refused\": [";
    for (int k = 0; k < 6; k++) body += std::string(k ? ", " : "") + "\"" + head(s_bad[k]) + "\"";
    body += "], \"after_init\": " + all_updates(solver);
  }
  std::printf("{\"before_init\": %s, \"init_ok\": %s%s}\n", pre_json.c_str(), init.ok() ? "true" : "false", body.c_str());
  return 0;
}
