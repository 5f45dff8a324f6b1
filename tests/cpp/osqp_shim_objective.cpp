// include/osqp++.h objective updates and warm starts: SetObjectiveVector, UpdateObjectiveMatrix,
// UpdateObjectiveAndConstraintMatrices, SetDualWarmStart and SetWarmStart(x, y).
// First the five calls on an uninitialised solver (osqp-cpp answers FAILED_PRECONDITION), then, where Init succeeds:
// Init, Solve, SetObjectiveVector, Solve, UpdateObjectiveMatrix, SetWarmStart(x, y), Solve, and an objective matrix with a
// different pattern (INVALID_ARGUMENT).  Output: one line of JSON that tests/test_objective_update_abi.py and
// tests/test_gpu_objective_update.py read.
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

int main() {
  const double Pd[4] = {4, 1, 1, 2}, P2d[4] = {5, 1.5, 1.5, 3}, Pdiag[4] = {4, 0, 0, 2}, Ad[6] = {1, 1, 1, 0, 0, 1};
  const Sparse P = from_dense(2, 2, Pd), P2 = from_dense(2, 2, P2d), Pwrong = from_dense(2, 2, Pdiag), A = from_dense(3, 2, Ad);
  Eigen::VectorXd l(3), u(3), q0(2), q1(2), x0(2), y0(3);
  l[0] = 1; l[1] = 0; l[2] = 0; u[0] = 1; u[1] = 0.7; u[2] = 0.7;
  q0[0] = 1; q0[1] = 1; q1[0] = -1; q1[1] = 2;
  x0.setZero(2); y0.setZero(3);

  // ---- before Init
  osqp::OsqpSolver fresh;
  const std::string pre[5] = {fresh.SetObjectiveVector(q1).ToString(), fresh.UpdateObjectiveMatrix(P2).ToString(),
                              fresh.UpdateObjectiveAndConstraintMatrices(P2, A).ToString(), fresh.SetDualWarmStart(y0).ToString(),
                              fresh.SetWarmStart(x0, y0).ToString()};
  std::string pre_json = "[";
  for (int k = 0; k < 5; k++) pre_json += std::string(k ? ", " : "") + "\"" + pre[k].substr(0, pre[k].find(':')) + "\"";
  pre_json += "]";

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
    const absl::Status s_q = solver.SetObjectiveVector(q1);
    const osqp::OsqpExitCode c2 = solver.Solve();
    const long long it2 = solver.iterations();
    const Eigen::VectorXd x2 = solver.primal_solution(), y2 = solver.dual_solution();
    const absl::Status s_p = solver.UpdateObjectiveMatrix(P2);
    const absl::Status s_w = solver.SetWarmStart(x2, y2);
    const osqp::OsqpExitCode c3 = solver.Solve();
    const long long it3 = solver.iterations();
    const Eigen::VectorXd x3 = solver.primal_solution(), y3 = solver.dual_solution();
    const absl::Status s_bad = solver.UpdateObjectiveMatrix(Pwrong);
    const absl::Status s_len = solver.SetObjectiveVector(l);
    char buf[512];
    std::snprintf(buf, sizeof buf, ", \"codes\": [\"%s\", \"%s\", \"%s\"], \"iters\": [%lld, %lld, %lld], ", osqp::ToString(c1).c_str(),
                  osqp::ToString(c2).c_str(), osqp::ToString(c3).c_str(), it1, it2, it3);
    body = buf;
    body += "\"x1\": " + vec(x1) + ", \"x2\": " + vec(x2) + ", \"y2\": " + vec(y2) + ", \"x3\": " + vec(x3) + ", \"y3\": " + vec(y3);
    body += ", \"status\": [\"" + s_q.ToString() + "\", \"" + s_p.ToString() + "\", \"" + s_w.ToString() + "\"]";
    body += ", \"wrong_pattern\": \"" + s_bad.ToString().substr(0, s_bad.ToString().find(':')) + "\"";
    body += ", \"wrong_length\": \"" + s_len.ToString().substr(0, s_len.ToString().find(':')) + "\"";
  }
  std::printf("{\"before_init\": %s, \"init_ok\": %s%s}\n", pre_json.c_str(), init.ok() ? "true" : "false", body.c_str());
  return 0;
}
