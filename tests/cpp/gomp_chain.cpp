// tests/cpp/gomp_chain.cpp -- TEST PROGRAM (links the oracle; never part of the product): the DH-chain ball model
// (include/mi_osqp/dh_kinematics.hpp, MI_GOMP_MODEL_DH_CHAIN) on the host and through the planners.
//
//   ./gomp_chain host FILE   CPU: FILE holds a chain, balls (frame, centre) and joint positions as hexadecimal floats (written
//                            by tests/test_dh_refs.py); prints mi_osqp::dh::point of every ball at every position in %a, one
//                            line "P b p[3] J[3 n]" each.  With a 6-joint chain and balls at the origins of frames 2, 5 and 6
//                            it adds the same from ur5e_kinematics.hpp's own functions as lines "U ...".
//   ./gomp_chain oracle      CPU: the 7-joint planning problems of `cont` through the sequential GOMPSolver on the oracle
//                            backend (the dhBall callbacks alone).
//   ./gomp_chain cont        GPU: ContinuousGOMPSolver<7> with the SQP step on the device (dh_chain set) against the same
//                            planner on the host callbacks: exit codes, counters, trajectories within 1e-6; a repeated
//                            device run bitwise equal.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>

#include "mi_osqp/dh_kinematics.hpp"
#include "mi_osqp/gomp.hpp"
#include "mi_osqp/ur5e_kinematics.hpp"
extern "C" {
#include "../../oracle/osqp_oracle.h"
}

using namespace miosqp_ref;

// QPSolver twin on the CPU oracle (as in gomp_parity.cpp)
class OracleQPSolver {
 public:
  OracleQPSolver(const QPConstraints &c, const QPMatrixSparse &P, bool = false) {
    const auto &[l, A, u] = c;
    oq_settings s; oq_default_settings(&s);
    oq_int err = 0;
    w_ = oq_setup(A.cols, A.rows, P.outer.data(), P.inner.data(), P.values.data(), nullptr, A.outer.data(), A.inner.data(),
                  A.values.data(), l.data(), u.data(), &s, &err);
    if (!w_) throw std::runtime_error("oracle setup failed");
    n_ = A.cols;
  }
  ~OracleQPSolver() { oq_cleanup(w_); }
  OracleQPSolver(const OracleQPSolver &) = delete;
  void update(const QPConstraints &c) {
    const auto &[l, A, u] = c;
    if (oq_update_A(w_, A.outer.data(), A.inner.data(), A.values.data())) throw std::invalid_argument("pattern");
    if (oq_update_bounds(w_, l.data(), u.data())) throw std::invalid_argument("bounds");
  }
  void setWarmStart(const QPVector &x) { oq_warm_start_x(w_, x.data()); }
  std::pair<OsqpExitCode, QPVector> solve() {
    const oq_int st = oq_solve(w_);
    QPVector x(n_);
    oq_get_solution(w_, x.data(), nullptr);
    OsqpExitCode c = OsqpExitCode::kUnknown;
    switch (st) {
      case 1: c = OsqpExitCode::kOptimal; break;
      case 2: c = OsqpExitCode::kOptimalInaccurate; break;
      case -3: c = OsqpExitCode::kPrimalInfeasible; break;
      case 3: c = OsqpExitCode::kPrimalInfeasibleInaccurate; break;
      case -4: c = OsqpExitCode::kDualInfeasible; break;
      case 4: c = OsqpExitCode::kDualInfeasibleInaccurate; break;
      case -2: c = OsqpExitCode::kMaxIterations; break;
      case -7: c = OsqpExitCode::kNonConvex; break;
      default: break;
    }
    return {c, x};
  }
 private:
  oq_work *w_ = nullptr;
  long long n_ = 0;
};

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); fails++; } } while (0)

static int run_host(const char *path) {
  std::ifstream in(path);
  if (!in) { std::printf("cannot read %s\n", path); return 2; }
  auto num = [&in]() { std::string t; in >> t; return std::strtod(t.c_str(), nullptr); };
  mi_gomp_chain ch{};
  ch.n_joints = (int)num();
  const int n = ch.n_joints;
  if (n < 1 || n > 8) return 2;
  for (int i = 0; i < n; ++i) ch.a[i] = num();
  for (int i = 0; i < n; ++i) ch.d[i] = num();
  for (int i = 0; i < n; ++i) ch.alpha[i] = num();
  for (int i = 0; i < n; ++i) ch.theta0[i] = num();
  const int nb = (int)num();
  std::vector<int> frame((size_t)nb);
  std::vector<std::array<double, 3>> centre((size_t)nb);
  bool ur5e_points = n == 6;
  for (int b = 0; b < nb; ++b) {
    frame[b] = (int)num();
    for (int k = 0; k < 3; ++k) centre[b][k] = num();
    ur5e_points = ur5e_points && (frame[b] == 2 || frame[b] == 5 || frame[b] == 6) && centre[b][0] == 0 && centre[b][1] == 0 && centre[b][2] == 0;
  }
  const int nq = (int)num();
  auto print = [n](const char *tag, int b, const double *p, const double *J) {
    std::printf("%s %d", tag, b);
    for (int k = 0; k < 3; ++k) std::printf(" %a", p[k]);
    for (int k = 0; k < 3 * n; ++k) std::printf(" %a", J[k]);
    std::printf("\n");
  };
  for (int w = 0; w < nq; ++w) {
    double q[8], p[3], J[24];
    for (int j = 0; j < n; ++j) q[j] = num();
    if (!in) { std::printf("short file\n"); return 2; }
    for (int b = 0; b < nb; ++b) {
      mi_osqp::dh::point(ch, q, frame[b], centre[b].data(), p, J);
      print("P", b, p, J);
      // the RobotBall made from the same data gives the same numbers through its callbacks
      RobotBall ball = dhBall(ch, frame[b], centre[b], 0.1, false);
      auto [x, y, z] = ball.fk(q);
      double J2[24];
      ball.jacobian(J2, q);
      CHECK(x == p[0] && y == p[1] && z == p[2] && !std::memcmp(J, J2, sizeof(double) * 3 * (size_t)n));
      CHECK(ball.builtin_model == MI_GOMP_MODEL_DH_CHAIN && ball.builtin_param[0] == frame[b] && ball.builtin_param[3] == centre[b][2]);
      if (ur5e_points) {
        const ur5e::Chain c = ur5e::chain(q);
        ur5e::point_jacobian(J2, q, frame[b]);
        print("U", b, c.o[frame[b]], J2);
      }
    }
  }
  std::printf(fails ? "HOST FAILED (%d)\n" : "HOST OK\n", fails);
  return fails ? 1 : 0;
}

// ---- the planning problems: the 7-joint chain c7 of tests/dh_refs.py with its seven link balls, the bar y = 0, z = 0.2 to pass
// above and the box z >= 0.15, x <= 0.75 of its gripper ball
constexpr size_t D7 = 7;
static mi_gomp_chain chain7() {
  const double H = 1.5707963267948966;
  mi_gomp_chain ch{};
  ch.n_joints = 7;
  const double a[7] = {0, 0, 0.0825, -0.0825, 0, 0.088, 0}, d[7] = {0.333, 0, 0.316, 0, 0.384, 0, 0.107};
  const double alpha[7] = {-H, H, H, -H, H, H, 0.3}, theta0[7] = {0, 0, 0, 0.25, 0, 0, -0.7};
  for (int i = 0; i < 7; ++i) { ch.a[i] = a[i]; ch.d[i] = d[i]; ch.alpha[i] = alpha[i]; ch.theta0[i] = theta0[i]; }
  return ch;
}
struct Problems {
  mi_gomp_chain chain = chain7();
  std::vector<RobotBall> balls;
  std::vector<HorizontalLine> lines{HorizontalLine({1, 0}, {0.0, 0.0, 0.2}, false)};
  Constraint<D7> pos, vel, acc;
  Constraint<3> c3d = constraints::inRange<3>(Vec<3>{-INF, -INF, 0.15}, Vec<3>{0.75, INF, INF});
  std::vector<Ctrl<D7>> starts, ends;
  Problems() {
    const double pi = 3.14159265358979323846;
    balls = {dhBall(chain, 2, {0, 0, 0}, 0.09), dhBall(chain, 3, {0, 0.05, -0.1}, 0.08), dhBall(chain, 4, {0.02, 0, 0.03}, 0.07),
             dhBall(chain, 5, {0, 0.04, -0.15}, 0.07), dhBall(chain, 6, {0.03, 0, 0}, 0.06), dhBall(chain, 7, {0, 0, -0.05}, 0.05),
             dhBall(chain, 7, {0.02, -0.01, 0.06}, 0.04, true)};
    pos = constraints::inRange<D7>(constraints::of<D7>(-2 * pi), constraints::of<D7>(2 * pi));
    vel = constraints::inRange<D7>(constraints::of<D7>(-pi), constraints::of<D7>(pi));
    acc = constraints::inRange<D7>(constraints::of<D7>(-pi * 800 / 180), constraints::of<D7>(pi * 800 / 180));
    const double base[7] = {0, 0.4, 0, -1.6, 0, 1.9, 0.6};
    for (int b = 0; b < 8; ++b) {
      Ctrl<D7> s{}, e{};
      for (int j = 0; j < 7; ++j) { s[j] = base[j] + 0.02 * ((b + j) % 3 - 1); e[j] = base[j] - 0.02 * ((b + 2 * j) % 3 - 1); }
      s[0] = -1.0 + 0.05 * b; e[0] = 0.9 - 0.04 * b;
      s[1] += 0.08 * (b % 4); e[1] += 0.06 * (b % 3);         // the lower poses sweep the forearm through the bar
      if (b == 7) { s[0] = 0.5; e[0] = 0.9; }                  // never comes near the bar
      starts.push_back(s); ends.push_back(e);
    }
  }
};

static int run_oracle() {
  Problems pr;
  int updates = 0;
  for (size_t b = 0; b < pr.starts.size(); ++b) {
    GOMPSolver<D7, OracleQPSolver> o(40, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, pr.lines, pr.balls, nullptr, false);
    auto [code, x] = o.run(pr.starts[b], pr.ends[b]);
    std::printf("traj %zu %s segments %d solves %d updates %d\n", b, ToString(code).c_str(), o.segments_run, o.qp_solves, o.qp_updates);
    CHECK(code == ExitCode::kOptimal);
    updates += o.qp_updates;
  }
  CHECK(updates > 0);
  std::printf(fails ? "ORACLE FAILED (%d)\n" : "ORACLE OK\n", fails);
  return fails ? 1 : 0;
}

static int run_cont() {
  Problems pr;
  ContinuousGOMPSolver<D7> host(40, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, pr.lines, pr.balls), dev(40, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, pr.lines, pr.balls),
      nochain(40, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, pr.lines, pr.balls);
  dev.device_assembly = true;
  dev.dh_chain = pr.chain;
  nochain.device_assembly = true;                        // chain balls without the chain: the host callbacks, bit for bit the host run
  auto rh = host.run(pr.starts, pr.ends);
  auto rd = dev.run(pr.starts, pr.ends);
  const std::vector<int> solves1 = dev.qp_solves, updates1 = dev.qp_updates;
  auto rd2 = dev.run(pr.starts, pr.ends);
  auto rn = nochain.run(pr.starts, pr.ends);
  CHECK(dev.qp_solves == solves1 && dev.qp_updates == updates1);
  double worst = 0.0;
  int updates = 0;
  for (size_t b = 0; b < pr.starts.size(); ++b) {
    std::printf("traj %zu host: %s segments %d solves %d updates %d | device: %s %d %d %d\n", b, ToString(rh[b].first).c_str(), host.segments_run[b],
                host.qp_solves[b], host.qp_updates[b], ToString(rd[b].first).c_str(), dev.segments_run[b], dev.qp_solves[b], dev.qp_updates[b]);
    CHECK(rh[b].first == rd[b].first);
    CHECK(host.segments_run[b] == dev.segments_run[b] && host.qp_solves[b] == dev.qp_solves[b] && host.qp_updates[b] == dev.qp_updates[b]);
    CHECK(rd2[b].first == rd[b].first && rd2[b].second == rd[b].second);                     // repeated run: bitwise
    CHECK(rn[b].first == rh[b].first && rn[b].second == rh[b].second);
    CHECK(rh[b].second.size() == rd[b].second.size());
    for (size_t k = 0; k < rh[b].second.size() && k < rd[b].second.size(); ++k) worst = std::fmax(worst, std::fabs(rh[b].second[k] - rd[b].second[k]));
    updates += dev.qp_updates[b];
  }
  std::printf("continuous planner, 7-joint chain, device assembly vs host assembly: %zu trajectories, %d re-linearisations on the device, max |dx| %.3e\n",
              pr.starts.size(), updates, worst);
  CHECK(updates > 0);
  CHECK(worst <= 1e-6);
  std::printf(fails ? "CONT FAILED (%d)\n" : "CONT OK\n", fails);
  return fails ? 1 : 0;
}

int main(int argc, char **argv) {
  setenv("GPU_MAX_HW_QUEUES", "10", 0);                 // one hardware queue per horizon stage, as the planner examples set it
  if (argc > 2 && !std::strcmp(argv[1], "host")) return run_host(argv[2]);
  if (argc > 1 && !std::strcmp(argv[1], "oracle")) return run_oracle();
  if (argc > 1 && !std::strcmp(argv[1], "cont")) return run_cont();
  std::printf("usage: gomp_chain host FILE | oracle | cont\n");
  return 2;
}
