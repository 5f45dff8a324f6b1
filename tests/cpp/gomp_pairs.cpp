// tests/cpp/gomp_pairs.cpp -- TEST PROGRAM (links the oracle; never part of the product): self-collision pairs (BallPair in
// include/mi_osqp/gomp.hpp, mi_gomp_pair) on the host and through the planners.
//
//   ./gomp_pairs rows FILE     CPU: FILE holds a scene of TABLE and yaw + 2-link balls (D = 3), lines, capsules, cuboids, pairs, the
//                              work-space limits and trajectories as hexadecimal floats (written by tests/test_gomp_pairs_cpp.py);
//                              prints the populated 3-D rows of ConstraintBuilder<3>::withObstacles as lines "R t row v0 v1 v2 l u"
//                              in %a and the verdict of GOMPSolver::isSolutionOK as "V t ok"; checks the allocation (every row
//                              behind the pair rows empty) and that a builder with an empty pair list gives the rows of the
//                              five-argument builder bit for bit.
//   ./gomp_pairs selfpairs     CPU: dhSelfPairs on the seven balls of the 7-joint chain: exactly the 14 pairs with a frame gap >= 2.
//   ./gomp_pairs fold_oracle   CPU: the folding problem (the straight joint-space line folds the forearm through the shoulder)
//                              through the sequential GOMPSolver on the oracle backend, without and with pairs.
//   ./gomp_pairs cont          GPU: ContinuousGOMPSolver with the SQP step on the device (pairs in the scene) against the same
//                              planner on the host callbacks on the folding problem: 2 trajectories of 20 waypoints; exit codes,
//                              counters, trajectories within 1e-6; the scenes re-made without pairs; the lock-step driver.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>

#include "mi_osqp/dh_kinematics.hpp"
#include "mi_osqp/gomp.hpp"
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

// a TABLE ball: p = (q0, q1, q2), constant Jacobian
static RobotBall tableBall(const std::array<double, 9> &T, double radius, bool gripper) {
  RobotBall b([](double *q) { return std::make_tuple(q[0], q[1], q[2]); }, [T](double *J, double *) { for (int k = 0; k < 9; ++k) J[k] = T[k]; }, radius, gripper);
  b.withBuiltin(MI_GOMP_MODEL_TABLE, {T[0], T[1], T[2], T[3], T[4], T[5], T[6], T[7], T[8]});
  return b;
}
// a yaw + 2-link ball (MI_GOMP_MODEL_YAW_2LINK): yaw q0, shoulder q1, elbow q2; links L1, L2, base height Z0
static RobotBall yawBall(double L1, double L2, double Z0, double radius, bool gripper) {
  RobotBall b([=](double *q) {
                const double r = L1 * std::cos(q[1]) + L2 * std::cos(q[1] + q[2]);
                return std::make_tuple(r * std::cos(q[0]), r * std::sin(q[0]), Z0 + L1 * std::sin(q[1]) + L2 * std::sin(q[1] + q[2]));
              },
              [=](double *J, double *q) {
                const double c0 = std::cos(q[0]), s0 = std::sin(q[0]);
                const double r = L1 * std::cos(q[1]) + L2 * std::cos(q[1] + q[2]);
                const double dr1 = -L1 * std::sin(q[1]) - L2 * std::sin(q[1] + q[2]), dr2 = -L2 * std::sin(q[1] + q[2]);
                J[0] = -r * s0; J[1] = c0 * dr1; J[2] = c0 * dr2;
                J[3] = r * c0;  J[4] = s0 * dr1; J[5] = s0 * dr2;
                J[6] = 0.0;     J[7] = L1 * std::cos(q[1]) + L2 * std::cos(q[1] + q[2]); J[8] = L2 * std::cos(q[1] + q[2]);
              },
              radius, gripper);
  b.withBuiltin(MI_GOMP_MODEL_YAW_2LINK, {L1, L2, Z0});
  return b;
}

static int run_rows(const char *path) {
  std::ifstream in(path);
  if (!in) { std::printf("cannot read %s\n", path); return 2; }
  auto num = [&in]() { std::string t; in >> t; return std::strtod(t.c_str(), nullptr); };
  std::vector<RobotBall> balls;
  std::vector<HorizontalLine> lines;
  std::vector<CapsuleObstacle> caps;
  std::vector<CuboidObstacle> cubs;
  std::vector<BallPair> pairs;
  const int nb = (int)num();
  for (int b = 0; b < nb; ++b) {
    const int model = (int)num();
    const bool gripper = num() != 0;
    const double radius = num();
    std::array<double, 9> T;
    for (double &v : T) v = num();
    balls.push_back(model == MI_GOMP_MODEL_TABLE ? tableBall(T, radius, gripper) : yawBall(T[0], T[1], T[2], radius, gripper));
  }
  const int nl = (int)num();
  for (int k = 0; k < nl; ++k) {
    const double dx = num(), dy = num(), x = num(), y = num(), z = num();
    const bool below = num() != 0;
    lines.emplace_back(std::array<double, 2>{dx, dy}, Point{x, y, z}, below);
  }
  const int nc = (int)num();
  for (int k = 0; k < nc; ++k) {
    Point a, b;
    for (double &v : a) v = num();
    for (double &v : b) v = num();
    const double R = num(), margin = num();
    caps.emplace_back(a, b, R, margin);
  }
  const int nx = (int)num();
  for (int k = 0; k < nx; ++k) {
    Point o, h;
    CuboidObstacle::Axes ax;
    for (double &v : o) v = num();
    for (double &v : ax) v = num();
    for (double &v : h) v = num();
    const double R = num(), margin = num();
    cubs.push_back(CuboidObstacle::oriented(o, ax, h, R, margin));
  }
  const int np = (int)num();
  for (int k = 0; k < np; ++k) {
    const size_t a = (size_t)num(), b = (size_t)num();
    const double margin = num();
    pairs.push_back(BallPair{a, b, margin});
  }
  Vec<3> lo, hi;
  for (double &v : lo) v = num();
  for (double &v : hi) v = num();
  const Constraint<3> c3d = constraints::inRange<3>(lo, hi);
  const size_t W = (size_t)num();
  const int nt = (int)num();
  if (!in || W < 4) { std::printf("short file\n"); return 2; }
  const Constraint<3> any = constraints::any<3>();
  const size_t row0 = (W - 1) * 3 + 3 * (W + W - 1 + W - 2);
  size_t rows3d = W * pairs.size();
  for (const RobotBall &b : balls) rows3d += W * ((b.is_gripper ? 3 : 0) + lines.size() + caps.size() + cubs.size());
  for (int t = 0; t < nt; ++t) {
    QPVector x(2 * 3 * W);
    for (double &v : x) v = num();
    if (!in) { std::printf("short file\n"); return 2; }
    ConstraintBuilder<3> b{W, balls, lines, caps, cubs, pairs};
    const auto [l, A, u] = b.withObstacles(c3d, x).build();
    // the allocation grows by W |pairs| rows: every row of the five-argument builder keeps its index
    CHECK(l.size() == (W - 1) * 3 + 3 * (W + W - 1 + W - 2 + W * (3 + (lines.size() + caps.size() + cubs.size()) * balls.size())) + W * pairs.size());
    // row-major view of the populated rows: D entries each, in the columns of their waypoint
    std::vector<std::array<double, 3>> vals(rows3d, {0, 0, 0});
    std::vector<int> seen(rows3d, 0);
    for (long long c = 0; c < A.cols; ++c)
      for (long long k = A.outer[c]; k < A.outer[c + 1]; ++k) {
        const size_t r = (size_t)A.inner[k];
        if (r < row0) continue;
        CHECK(r < row0 + rows3d && c < (long long)(3 * W));
        if (r < row0 + rows3d) { vals[r - row0][(size_t)c % 3] = A.values[k]; seen[r - row0]++; }
      }
    for (size_t r = 0; r < rows3d; ++r) {
      CHECK(seen[r] == 3);
      std::printf("R %d %zu %a %a %a %a %a\n", t, r, vals[r][0], vals[r][1], vals[r][2], l[row0 + r], u[row0 + r]);
    }
    for (size_t r = row0 + rows3d; r < l.size(); ++r) CHECK(l[r] == -INF && u[r] == INF);       // the empty rows come after the pair rows
    GOMPSolver<3, OracleQPSolver> g(W, 0.1, any, any, any, c3d, lines, balls);
    g.capsules = caps;
    g.cuboids = cubs;
    g.pairs = pairs;
    std::printf("V %d %d\n", t, g.acceptable(x) ? 1 : 0);
    // no pairs: the six-argument builder with an empty list is the five-argument one, bit for bit
    ConstraintBuilder<3> b5{W, balls, lines, caps, cubs}, b6{W, balls, lines, caps, cubs, {}};
    const auto [l5, A5, u5] = b5.withObstacles(c3d, x).build();
    const auto [l6, A6, u6] = b6.withObstacles(c3d, x).build();
    CHECK(l5.size() == l6.size() && !std::memcmp(l5.data(), l6.data(), l5.size() * sizeof(double)) && !std::memcmp(u5.data(), u6.data(), u5.size() * sizeof(double)));
    CHECK(A5.outer == A6.outer && A5.inner == A6.inner && A5.values.size() == A6.values.size() &&
          !std::memcmp(A5.values.data(), A6.values.data(), A5.values.size() * sizeof(double)));
    // ... and the rows before the pair rows are those of the five-argument builder, bit for bit
    CHECK(l.size() >= l5.size() && !std::memcmp(l.data(), l5.data(), (row0 + rows3d - W * pairs.size()) * sizeof(double)));
    const auto [lp5, Ap5, up5] = ConstraintBuilder<3>{W, balls, lines, caps, cubs}.withObstaclePattern().build();
    const auto [lp6, Ap6, up6] = ConstraintBuilder<3>{W, balls, lines, caps, cubs, pairs}.withObstaclePattern().build();
    CHECK(Ap5.outer == A5.outer && Ap5.inner == A5.inner && Ap6.outer == A.outer && Ap6.inner == A.inner);      // the pattern ahead of time
    CHECK(lp6.size() == l.size());
  }
  std::printf(fails ? "ROWS FAILED (%d)\n" : "ROWS OK\n", fails);
  return fails ? 1 : 0;
}

// ---- the 7-joint chain c7 of tests/dh_refs.py with its seven link balls
constexpr size_t D7 = 7;
struct FoldProblems {
  mi_gomp_chain chain{};
  std::vector<RobotBall> balls;
  std::vector<BallPair> pairs;
  Constraint<D7> pos, vel, acc;
  Constraint<3> c3d = constraints::any<3>();
  std::vector<Ctrl<D7>> starts, ends;
  explicit FoldProblems(int n) {
    const double H = 1.5707963267948966, pi = 3.14159265358979323846;
    chain.n_joints = 7;
    const double a[7] = {0, 0, 0.0825, -0.0825, 0, 0.088, 0}, d[7] = {0.333, 0, 0.316, 0, 0.384, 0, 0.107};
    const double alpha[7] = {-H, H, H, -H, H, H, 0.3}, theta0[7] = {0, 0, 0, 0.25, 0, 0, -0.7};
    for (int i = 0; i < 7; ++i) { chain.a[i] = a[i]; chain.d[i] = d[i]; chain.alpha[i] = alpha[i]; chain.theta0[i] = theta0[i]; }
    balls = {dhBall(chain, 2, {0, 0, 0}, 0.09), dhBall(chain, 3, {0, 0.05, -0.1}, 0.08), dhBall(chain, 4, {0.02, 0, 0.03}, 0.07),
             dhBall(chain, 5, {0, 0.04, -0.15}, 0.07), dhBall(chain, 6, {0.03, 0, 0}, 0.06), dhBall(chain, 7, {0, 0, -0.05}, 0.05),
             dhBall(chain, 7, {0.02, -0.01, 0.06}, 0.04, true)};
    pairs = dhSelfPairs(balls, 2, 0.03);
    pos = constraints::inRange<D7>(constraints::of<D7>(-2 * pi), constraints::of<D7>(2 * pi));
    vel = constraints::inRange<D7>(constraints::of<D7>(-pi), constraints::of<D7>(pi));
    acc = constraints::inRange<D7>(constraints::of<D7>(-pi * 800 / 180), constraints::of<D7>(pi * 800 / 180));
    // both postures are clear of every pair by 0.058 or more; half way along the straight line between them the wrist balls
    // are 0.13 inside the shoulder ball
    const double A[7] = {-1.096, -0.205, -0.756, 1.077, 0.129, -2.249, -2.505}, B[7] = {-0.746, -0.553, -0.574, 2.791, 0.213, -2.254, -2.375};
    for (int b = 0; b < n; ++b) {
      Ctrl<D7> s{}, e{};
      for (int j = 0; j < 7; ++j) { s[j] = A[j] + 0.01 * b * ((j % 3) - 1); e[j] = B[j] - 0.01 * b * ((j % 2) ? 1 : -1); }
      starts.push_back(s); ends.push_back(e);
    }
  }
};

template <size_t D>
static double minPairClearance(const std::vector<BallPair> &pairs, const std::vector<RobotBall> &balls, const QPVector &x) {
  double worst = INF;
  std::vector<double> xyz(3 * balls.size());
  for (size_t w = 0; w < x.size() / 2 / D; ++w) {
    std::vector<double> q(x.begin() + (long)(w * D), x.begin() + (long)((w + 1) * D));
    for (size_t i = 0; i < balls.size(); ++i) std::tie(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]) = balls[i].fk(q.data());
    for (const BallPair &p : pairs) worst = std::fmin(worst, pairClearance(p, xyz, balls));
  }
  return worst;
}

static int run_selfpairs() {
  FoldProblems pr(1);
  const std::vector<BallPair> want{{0, 2, 0.03}, {0, 3, 0.03}, {0, 4, 0.03}, {0, 5, 0.03}, {0, 6, 0.03}, {1, 3, 0.03}, {1, 4, 0.03}, {1, 5, 0.03}, {1, 6, 0.03},
                                   {2, 4, 0.03}, {2, 5, 0.03}, {2, 6, 0.03}, {3, 5, 0.03}, {3, 6, 0.03}};
  CHECK(pr.pairs.size() == 14 && pr.pairs == want);
  CHECK(dhSelfPairs(pr.balls).size() == 14 && dhSelfPairs(pr.balls)[0] == (BallPair{0, 2, 0.0}));
  CHECK(dhSelfPairs(pr.balls, 1).size() == 20 && dhSelfPairs(pr.balls, 0).size() == 20);      // never two balls of one frame
  CHECK(dhSelfPairs(pr.balls, 5, 0.1).size() == 2 && dhSelfPairs(pr.balls, 6).empty());
  std::vector<RobotBall> mixed = pr.balls;
  mixed.push_back(tableBall({1, 0, 0, 0, 1, 0, 0, 0, 1}, 0.1, false));
  CHECK(dhSelfPairs(mixed, 2, 0.03) == want);                                                   // balls of other models are left out
  CHECK(!(BallPair{0, 2, 0.03} == BallPair{2, 0, 0.03}) && !(BallPair{0, 2, 0.03} == BallPair{0, 2, 0.04}));
  // pairsClear / pairClearance on centres given directly: balls 0 and 2 (radii 0.09 + 0.07) 0.2 apart along x
  std::vector<double> xyz(3 * pr.balls.size(), 0.0);
  for (size_t i = 0; i < pr.balls.size(); ++i) xyz[3 * i + 1] = 10.0 * (double)i;
  xyz[0] = 0.0; xyz[1] = 0.0; xyz[6] = 0.2; xyz[7] = 0.0;
  CHECK(std::fabs(pairClearance({0, 2, 0.0}, xyz, pr.balls) - 0.04) < 1e-15 && pairsClear(pr.pairs, xyz, pr.balls));
  xyz[6] = 0.15;
  CHECK(!pairsClear(pr.pairs, xyz, pr.balls) && pairsClear({}, xyz, pr.balls));
  std::printf(fails ? "SELFPAIRS FAILED (%d)\n" : "SELFPAIRS OK\n", fails);
  return fails ? 1 : 0;
}

static int run_fold_oracle(int W) {
  FoldProblems pr(2);
  for (size_t b = 0; b < pr.starts.size(); ++b) {
    QPVector line = linspace<D7>(pr.starts[b], pr.ends[b], (size_t)W);
    line.resize(2 * (size_t)W * D7, 0.0);
    const double c_line = minPairClearance<D7>(pr.pairs, pr.balls, line);
    CHECK(c_line < -0.05);
    double clear[2];
    for (int with = 0; with < 2; ++with) {
      GOMPSolver<D7, OracleQPSolver> o((size_t)W, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls, nullptr, false);
      if (with) o.pairs = pr.pairs;
      auto [code, x] = o.run(pr.starts[b], pr.ends[b]);
      clear[with] = minPairClearance<D7>(pr.pairs, pr.balls, x);
      std::printf("fold traj %zu %s pairs: %s segments %d solves %d updates %d, %zu waypoints, minimum pair clearance %.6f (straight line %.6f)\n", b,
                  with ? "with" : "without", ToString(code).c_str(), o.segments_run, o.qp_solves, o.qp_updates, x.size() / 2 / D7, clear[with], c_line);
      CHECK(code == ExitCode::kOptimal);
      if (with) { CHECK(o.qp_updates >= 1); CHECK(o.acceptable(x)); }
    }
    CHECK(clear[0] < -0.01);                                   // without pairs the plan penetrates
    CHECK(clear[1] >= -1e-3);                                  // with them it is clear
  }
  std::printf(fails ? "FOLD ORACLE FAILED (%d)\n" : "FOLD ORACLE OK\n", fails);
  return fails ? 1 : 0;
}

static int run_cont() {
  FoldProblems pr(2);
  ContinuousGOMPSolver<D7> host(20, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls), dev(20, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls);
  host.pairs = dev.pairs = pr.pairs;
  dev.device_assembly = true;
  dev.dh_chain = pr.chain;
  auto rh = host.run(pr.starts, pr.ends);
  auto rd = dev.run(pr.starts, pr.ends);
  double worst = 0.0, clear = INF;
  int updates = 0, planned = 0;
  for (size_t b = 0; b < pr.starts.size(); ++b) {
    std::printf("fold traj %zu host: %s segments %d solves %d updates %d | device: %s %d %d %d\n", b, ToString(rh[b].first).c_str(), host.segments_run[b],
                host.qp_solves[b], host.qp_updates[b], ToString(rd[b].first).c_str(), dev.segments_run[b], dev.qp_solves[b], dev.qp_updates[b]);
    CHECK(rh[b].first == rd[b].first);
    CHECK(host.segments_run[b] == dev.segments_run[b] && host.qp_solves[b] == dev.qp_solves[b] && host.qp_updates[b] == dev.qp_updates[b]);
    CHECK(rh[b].second.size() == rd[b].second.size());
    for (size_t k = 0; k < rh[b].second.size() && k < rd[b].second.size(); ++k) worst = std::fmax(worst, std::fabs(rh[b].second[k] - rd[b].second[k]));
    updates += dev.qp_updates[b];
    if (rd[b].first == ExitCode::kOptimal) { ++planned; clear = std::fmin(clear, minPairClearance<D7>(pr.pairs, pr.balls, rd[b].second)); }
  }
  std::printf("fold: continuous planner with pairs, device assembly vs host assembly: %zu trajectories (%d planned), %d re-linearisations on the device, "
              "max |dx| %.3e, minimum pair clearance %.6f\n", pr.starts.size(), planned, updates, worst, clear);
  CHECK(updates > 0);
  CHECK(planned == 2 && clear >= -1e-3);
  CHECK(worst <= 1e-6);
  // the kept scenes are made again when the pairs change: the same planner without pairs penetrates
  dev.pairs.clear();
  auto rn = dev.run(pr.starts, pr.ends);
  for (size_t b = 0; b < pr.starts.size(); ++b) CHECK(rn[b].first == ExitCode::kOptimal && minPairClearance<D7>(pr.pairs, pr.balls, rn[b].second) < -0.01);
  // the lock-step driver takes the same decisions per trajectory
  BatchGOMPSolver<D7> batch(20, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls);
  batch.pairs = pr.pairs;
  auto rb = batch.run(pr.starts, pr.ends);
  for (size_t b = 0; b < pr.starts.size(); ++b) {
    double dx = 0.0;
    CHECK(rb[b].first == rh[b].first && rb[b].second.size() == rh[b].second.size());
    for (size_t k = 0; k < rb[b].second.size() && k < rh[b].second.size(); ++k) dx = std::fmax(dx, std::fabs(rb[b].second[k] - rh[b].second[k]));
    std::printf("fold traj %zu lock-step driver: %s, max |dx| against the continuous one %.3e, minimum pair clearance %.6f\n", b, ToString(rb[b].first).c_str(), dx,
                minPairClearance<D7>(pr.pairs, pr.balls, rb[b].second));
    CHECK(dx <= 1e-5 && minPairClearance<D7>(pr.pairs, pr.balls, rb[b].second) >= -1e-3);      // (1e-5: as gomp_parity compares two drivers)
  }
  std::printf(fails ? "CONT FAILED (%d)\n" : "CONT OK\n", fails);
  return fails ? 1 : 0;
}

int main(int argc, char **argv) {
  setenv("GPU_MAX_HW_QUEUES", "10", 0);                 // one hardware queue per horizon stage, as the planner examples set it
  if (argc > 2 && !std::strcmp(argv[1], "rows")) return run_rows(argv[2]);
  if (argc > 1 && !std::strcmp(argv[1], "selfpairs")) return run_selfpairs();
  if (argc > 1 && !std::strcmp(argv[1], "fold_oracle")) return run_fold_oracle(argc > 2 ? std::atoi(argv[2]) : 20);
  if (argc > 1 && !std::strcmp(argv[1], "cont")) return run_cont();
  std::printf("usage: gomp_pairs rows FILE | selfpairs | fold_oracle [W] | cont\n");
  return 2;
}
