// The P updates of the C++ facades (include/mi_osqp/qp_solver.hpp): ContinuousQPSolver::updateP runs one per-QP P update, and
// one with new constraints, on a two-slot solver and prints the solutions for tests/test_gpu_p_update_cpp.py to compare with
// the Python binding's, bit for bit (%.17g round-trips a double).  BatchQPSolver's device forms are compiled and its pattern
// getter is run; the device forms need device memory, which this host-only program does not have.
#include <cstdio>
#include <string>
#include <vector>

#include "mi_osqp/qp_solver.hpp"

using namespace miosqp_ref;

// never called: the device forms compile with the documented shapes
void device_forms(BatchQPSolver &s, const double *d_P, const double *d_A, const double *d_l, const double *d_u, void *stream) {
  s.updatePDevice(d_P);
  s.updatePDevice(d_P, stream);
  s.updateDevice(d_P, d_A, d_l, d_u);
  s.updateDevice(d_P, d_A, d_l, d_u, stream);
}

static void print_vec(const char *name, const QPVector &v, bool last = false) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); i++) std::printf("%s%.17g", i ? ", " : "", v[i]);
  std::printf("]%s", last ? "" : ", ");
}

static void drain(ContinuousQPSolver &s) {
  for (int k = 0; k < 400 && s.running() > 0; k++) { s.advance(1); s.poll(); }
}

int main() {
  // triu(P) of a 3 x 3 matrix with off-diagonal entries; A = [1 1 1; I], one equality row and a box
  QPMatrixSparse P{3, 3, {0, 1, 3, 5}, {0, 0, 1, 1, 2}, {4.0, 1.0, 3.0, 0.5, 2.0}};
  QPMatrixSparse A{4, 3, {0, 2, 4, 6}, {0, 1, 0, 2, 0, 3}, {1.0, 1.0, 1.0, 1.0, 1.0, 1.0}};
  QPConstraints c0{{1.0, 0.0, 0.0, 0.0}, A, {1.0, 0.7, 0.7, 0.7}};
  ContinuousQPSolver s(2, c0, P);
  if (s.setup_status() != MI_OSQP_OK) { std::printf("{\"setup\": %d}\n", s.setup_status()); return 1; }
  const QPVector P1{2.0, -0.5, 5.0, 1.5, 3.0};
  s.updateP({1}, {&P1});
  s.begin({0, 1});
  drain(s);
  const auto r0 = s.result(0);
  const long long it0 = s.last_info().iter;
  const auto r1 = s.result(1);
  const long long it1 = s.last_info().iter;
  // slot 0: new P together with new A values and bounds
  QPMatrixSparse A2 = A;
  A2.values = {1.0, 1.0, 2.0, 1.0, 0.5, 1.0};
  QPConstraints c1{{1.0, 0.0, 0.0, 0.0}, A2, {1.0, 0.6, 0.8, 0.9}};
  const QPVector P2{3.0, 0.25, 2.0, -0.75, 4.0};
  s.updateP({0}, {&P2}, {&c1});
  s.begin({0});
  drain(s);
  const auto r2 = s.result(0);
  const long long it2 = s.last_info().iter;
  // refusals throw and change nothing
  int thrown = 0;
  try { s.updateP({1, 1}, {&P1, &P1}); } catch (const std::invalid_argument &) { thrown++; }
  try { s.updateP({2}, {&P1}); } catch (const std::invalid_argument &) { thrown++; }
  const QPVector shortP{1.0, 2.0};
  try { s.updateP({1}, {&shortP}); } catch (const std::invalid_argument &) { thrown++; }
  try { s.updateP({0, 1}, {&P1}); } catch (const std::invalid_argument &) { thrown++; }
  // the pattern getter of the blocking facade: a P given with both triangles comes back as its upper one
  QPMatrixSparse Pfull{3, 3, {0, 2, 5, 7}, {0, 1, 0, 1, 2, 1, 2}, {4.0, 1.0, 1.0, 3.0, 0.5, 0.5, 2.0}};
  BatchQPSolver b({c0, c0}, Pfull);
  const auto pat = b.upperPatternP();
  const bool pattern_ok = pat.first == P.outer && pat.second == P.inner;
  std::printf("{\"codes\": [%d, %d, %d], \"iters\": [%lld, %lld, %lld], \"thrown\": %d, \"pattern_ok\": %s, ",
              (int)r0.first, (int)r1.first, (int)r2.first, it0, it1, it2, thrown, pattern_ok ? "true" : "false");
  print_vec("x0", r0.second); print_vec("x1", r1.second); print_vec("x2", r2.second, true);
  std::printf("}\n");
  return 0;
}
