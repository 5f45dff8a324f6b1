// include/osqp++.h infeasibility certificates: primal_infeasibility_certificate() / dual_infeasibility_certificate().
// Two QPs through the shim, where Init succeeds:
//   primal infeasible, two variables: x0 + x1 in [3, 4] with x0, x1 in [0, 1] (the sum reaches 2 at most);
//   dual infeasible, one variable:    minimise x subject to x <= 0 (P = 0 as an explicit entry, q = 1).
// For each: the exit code, both certificates before the first Solve() and after it.  Output: one line of JSON that
// tests/test_osqp_shim_certificates.py reads.
#include <cstdio>
#include <iostream>
#include <string>

#include <osqp++.h>

using Sparse = Eigen::SparseMatrix<double, Eigen::ColMajor, long long>;

static Sparse from_entries(int rows, int cols, const std::vector<Eigen::Triplet<double, long long>> &t) {
  Sparse M(rows, cols);
  M.setFromTriplets(t.begin(), t.end());
  return M;
}

// NaN is no JSON: null
static std::string vec(const Eigen::VectorXd &x) {
  std::string s = "[";
  char buf[40];
  for (Eigen::Index i = 0; i < x.size(); i++) {
    if (x[i] != x[i]) std::snprintf(buf, sizeof buf, "%snull", i ? ", " : "");
    else std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", x[i]);
    s += buf;
  }
  return s + "]";
}

static std::string run(const char *name, const osqp::OsqpInstance &instance, bool &ok) {
  osqp::OsqpSettings settings;
  settings.verbose = false;
  osqp::OsqpSolver solver;
  const absl::Status init = solver.Init(instance, settings);
  std::cout << name << " Init: " << init.ToString() << std::endl;
  ok = ok && init.ok();
  if (!init.ok()) return std::string("\"") + name + "\": null";
  const Eigen::VectorXd p0 = solver.primal_infeasibility_certificate(), d0 = solver.dual_infeasibility_certificate();
  const osqp::OsqpExitCode code = solver.Solve();
  const Eigen::VectorXd p1 = solver.primal_infeasibility_certificate(), d1 = solver.dual_infeasibility_certificate();
  const Eigen::VectorXd x = solver.primal_solution();
  return std::string("\"") + name + "\": {\"code\": \"" + osqp::ToString(code) + "\", \"iter\": " + std::to_string(solver.iterations()) +
         ", \"prim_before\": " + vec(p0) + ", \"dual_before\": " + vec(d0) + ", \"prim\": " + vec(p1) + ", \"dual\": " + vec(d1) +
         ", \"x\": " + vec(x) + "}";
}

int main() {
  osqp::OsqpSolver fresh;
  const long long empty = (long long)fresh.primal_infeasibility_certificate().size() + (long long)fresh.dual_infeasibility_certificate().size();

  osqp::OsqpInstance pinf;
  pinf.objective_matrix = from_entries(2, 2, {{0, 0, 1.0}, {1, 1, 1.0}});
  pinf.constraint_matrix = from_entries(3, 2, {{0, 0, 1.0}, {1, 0, 1.0}, {0, 1, 1.0}, {2, 1, 1.0}});
  pinf.objective_vector = Eigen::VectorXd(2); pinf.objective_vector[0] = 0; pinf.objective_vector[1] = 0;
  pinf.lower_bounds = Eigen::VectorXd(3); pinf.upper_bounds = Eigen::VectorXd(3);
  pinf.lower_bounds[0] = 3; pinf.upper_bounds[0] = 4;
  pinf.lower_bounds[1] = 0; pinf.upper_bounds[1] = 1;
  pinf.lower_bounds[2] = 0; pinf.upper_bounds[2] = 1;

  osqp::OsqpInstance dinf;
  dinf.objective_matrix = from_entries(1, 1, {{0, 0, 0.0}});
  dinf.constraint_matrix = from_entries(1, 1, {{0, 0, 1.0}});
  dinf.objective_vector = Eigen::VectorXd(1); dinf.objective_vector[0] = 1;
  dinf.lower_bounds = Eigen::VectorXd(1); dinf.upper_bounds = Eigen::VectorXd(1);
  dinf.lower_bounds[0] = -1e30; dinf.upper_bounds[0] = 0;

  bool ok = true;
  const std::string a = run("pinf", pinf, ok), b = run("dinf", dinf, ok);
  std::printf("{\"uninitialised_entries\": %lld, \"init_ok\": %s, %s, %s}\n", empty, ok ? "true" : "false", a.c_str(), b.c_str());
  return 0;
}
