// include/osqp++.h with solution polishing: osqp::OsqpSolver::Init takes polish / polish_refine_iter / delta (osqp-cpp's
// settings fields) and maps them onto the core's polishing.  Output: one line of JSON (Init status, exit code name,
// iterations, solution) that tests/test_polish_settings.py and tests/test_gpu_polish.py compare with the ctypes binding.
// Without a gfx950 GPU, Init reports the device error (not kUnimplemented) and Solve() returns kUnknown.
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

int main() {
  // upstream's documentation demo (q = 0): active set {row 0 equality, row 2 upper}
  const double Pd[4] = {4, 1, 1, 2}, Ad[6] = {1, 1, 1, 0, 0, 1};
  Eigen::VectorXd l(3), u(3);
  l[0] = 1; l[1] = 0; l[2] = 0; u[0] = 1; u[1] = 0.7; u[2] = 0.7;
  osqp::OsqpInstance instance;
  instance.objective_matrix = from_dense(2, 2, Pd); instance.constraint_matrix = from_dense(3, 2, Ad);
  instance.objective_vector.setZero(2);
  instance.lower_bounds = l; instance.upper_bounds = u;
  osqp::OsqpSettings settings;
  settings.verbose = false;
  settings.polish = true;
  settings.polish_refine_iter = 3;
  settings.delta = 1e-6;
  osqp::OsqpSolver solver;
  const absl::Status status = solver.Init(instance, settings);
  std::cout << "Init: " << status.ToString() << std::endl;
  const osqp::OsqpExitCode code = solver.Solve();
  const Eigen::VectorXd x = solver.primal_solution();
  auto num = [&](int i) { return x.size() > i ? x[i] : 0.0; };
  std::printf("{\"init_ok\": %s, \"code\": \"%s\", \"iter\": %lld, \"x\": [%.17g, %.17g]}\n", status.ok() ? "true" : "false",
              osqp::ToString(code).c_str(), (long long)solver.iterations(), num(0), num(1));
  return 0;
}
