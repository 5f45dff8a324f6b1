// tests/cpp/gomp_tilt.cpp -- TEST PROGRAM (links the oracle; never part of the product): tilt limits (TiltLimit in
// include/mi_osqp/gomp.hpp, mi_gomp_tilt) on the host and through the planners.
//
//   ./gomp_tilt rows FILE      CPU: FILE holds a scene of D = 2 or 3 joints: a DH chain, TABLE, yaw + 2-link and chain balls, lines,
//                              capsules, cuboids, pairs, tilts, the work-space limits and trajectories as hexadecimal floats (written
//                              by tests/test_gomp_tilt_cpp.py); prints the populated 3-D rows of ConstraintBuilder<D>::withObstacles
//                              as lines "R t row v0 .. l u" in %a and the verdict of GOMPSolver::isSolutionOK as "V t ok"; checks the
//                              allocation (every row behind the tilt rows empty) and that a builder with an empty tilt list gives
//                              the rows of the six-argument builder bit for bit.
//   ./gomp_tilt checks         CPU: dh::axis against central differences, tiltsOK / tiltsOKAlong at the 1 mrad, the thresholds.
//   ./gomp_tilt tilt_oracle    CPU: the upright problem (the straight joint-space line tips the tool far over) through the
//                              sequential GOMPSolver on the oracle backend, without and with the limit.
//   ./gomp_tilt cont           GPU: ContinuousGOMPSolver with the SQP step on the device (tilts in the scene) against the same
//                              planner on the host callbacks on the upright problem: 2 trajectories of 20 waypoints; exit codes,
//                              counters, largest tilt; the scenes re-made without tilts.
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

template <size_t D>
static int run_rows(std::ifstream &in) {
  auto num = [&in]() { std::string t; in >> t; return std::strtod(t.c_str(), nullptr); };
  mi_gomp_chain chain{};
  chain.n_joints = (int)num();
  for (int i = 0; i < chain.n_joints; ++i) { chain.a[i] = num(); chain.d[i] = num(); chain.alpha[i] = num(); chain.theta0[i] = num(); }
  std::vector<RobotBall> balls;
  std::vector<HorizontalLine> lines;
  std::vector<CapsuleObstacle> caps;
  std::vector<CuboidObstacle> cubs;
  std::vector<BallPair> pairs;
  std::vector<TiltLimit> tilts;
  const int nb = (int)num();
  for (int b = 0; b < nb; ++b) {
    const int model = (int)num();
    const bool gripper = num() != 0;
    const double radius = num();
    std::array<double, 9> T;
    for (double &v : T) v = num();
    if (model == MI_GOMP_MODEL_DH_CHAIN) balls.push_back(dhBall(chain, (int)T[0], {T[1], T[2], T[3]}, radius, gripper));
    else if constexpr (D == 3) balls.push_back(model == MI_GOMP_MODEL_TABLE ? tableBall(T, radius, gripper) : yawBall(T[0], T[1], T[2], radius, gripper));
    else { std::printf("model %d needs D = 3\n", model); return 2; }
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
  const int ntl = (int)num();
  for (int k = 0; k < ntl; ++k) {
    const int frame = (int)num();
    std::array<double, 3> ax, ref;
    for (double &v : ax) v = num();
    for (double &v : ref) v = num();
    const double max_angle = num(), margin = num();
    tilts.push_back(dhTilt(chain, frame, ax, ref, max_angle, margin));
  }
  Vec<3> lo, hi;
  for (double &v : lo) v = num();
  for (double &v : hi) v = num();
  const Constraint<3> c3d = constraints::inRange<3>(lo, hi);
  const size_t W = (size_t)num();
  const int nt = (int)num();
  if (!in || W < 4) { std::printf("short file\n"); return 2; }
  const Constraint<D> any = constraints::any<D>();
  const size_t row0 = (W - 1) * D + D * (W + W - 1 + W - 2);
  size_t rows3d = W * (pairs.size() + tilts.size());
  for (const RobotBall &b : balls) rows3d += W * ((b.is_gripper ? 3 : 0) + lines.size() + caps.size() + cubs.size());
  for (int t = 0; t < nt; ++t) {
    QPVector x(2 * D * W);
    for (double &v : x) v = num();
    if (!in) { std::printf("short file\n"); return 2; }
    ConstraintBuilder<D> b{W, balls, lines, caps, cubs, pairs, tilts};
    const auto [l, A, u] = b.withObstacles(c3d, x).build();
    // the allocation grows by W |tilts| rows: every row of the six-argument builder keeps its index
    CHECK(l.size() == (W - 1) * D + D * (W + W - 1 + W - 2 + W * (3 + (lines.size() + caps.size() + cubs.size()) * balls.size())) + W * (pairs.size() + tilts.size()));
    // row-major view of the populated rows: D entries each, in the columns of their waypoint
    std::vector<std::array<double, D>> vals(rows3d);
    for (auto &v : vals) v.fill(0.0);
    std::vector<int> seen(rows3d, 0);
    for (long long c = 0; c < A.cols; ++c)
      for (long long k = A.outer[c]; k < A.outer[c + 1]; ++k) {
        const size_t r = (size_t)A.inner[k];
        if (r < row0) continue;
        CHECK(r < row0 + rows3d && c < (long long)(D * W));
        if (r < row0 + rows3d) { vals[r - row0][(size_t)c % D] = A.values[k]; seen[r - row0]++; }
      }
    for (size_t r = 0; r < rows3d; ++r) {
      CHECK(seen[r] == (int)D);
      std::printf("R %d %zu", t, r);
      for (size_t j = 0; j < D; ++j) std::printf(" %a", vals[r][j]);
      std::printf(" %a %a\n", l[row0 + r], u[row0 + r]);
    }
    for (size_t r = row0 + rows3d; r < l.size(); ++r) CHECK(l[r] == -INF && u[r] == INF);       // the empty rows come after the tilt rows
    GOMPSolver<D, OracleQPSolver> g(W, 0.1, any, any, any, c3d, lines, balls);
    g.capsules = caps;
    g.cuboids = cubs;
    g.pairs = pairs;
    g.tilts = tilts;
    std::printf("V %d %d\n", t, g.acceptable(x) ? 1 : 0);
    CHECK(tiltsOKAlong<D>(tilts, x) || !g.acceptable(x));
    // no tilts: the seven-argument builder with an empty list is the six-argument one, bit for bit
    ConstraintBuilder<D> b6{W, balls, lines, caps, cubs, pairs}, b7{W, balls, lines, caps, cubs, pairs, {}};
    const auto [l6, A6, u6] = b6.withObstacles(c3d, x).build();
    const auto [l7, A7, u7] = b7.withObstacles(c3d, x).build();
    CHECK(l6.size() == l7.size() && !std::memcmp(l6.data(), l7.data(), l6.size() * sizeof(double)) && !std::memcmp(u6.data(), u7.data(), u6.size() * sizeof(double)));
    CHECK(A6.outer == A7.outer && A6.inner == A7.inner && A6.values.size() == A7.values.size() &&
          !std::memcmp(A6.values.data(), A7.values.data(), A6.values.size() * sizeof(double)));
    // ... and the rows before the tilt rows are those of the six-argument builder, bit for bit
    CHECK(l.size() >= l6.size() && !std::memcmp(l.data(), l6.data(), (row0 + rows3d - W * tilts.size()) * sizeof(double)));
    const auto [lp6, Ap6, up6] = ConstraintBuilder<D>{W, balls, lines, caps, cubs, pairs}.withObstaclePattern().build();
    const auto [lp7, Ap7, up7] = ConstraintBuilder<D>{W, balls, lines, caps, cubs, pairs, tilts}.withObstaclePattern().build();
    CHECK(Ap6.outer == A6.outer && Ap6.inner == A6.inner && Ap7.outer == A.outer && Ap7.inner == A.inner);      // the pattern ahead of time
    CHECK(lp7.size() == l.size());
  }
  std::printf(fails ? "ROWS FAILED (%d)\n" : "ROWS OK\n", fails);
  return fails ? 1 : 0;
}

// ---- the 7-joint chain c7 of tests/dh_refs.py with its seven link balls; the tool axis is the z axis of the last frame
constexpr size_t D7 = 7;
constexpr double kDeg = 3.14159265358979323846 / 180.0;
struct UprightProblems {
  mi_gomp_chain chain{};
  std::vector<RobotBall> balls;
  std::vector<TiltLimit> tilts;
  Constraint<D7> pos, vel, acc;
  Constraint<3> c3d = constraints::any<3>();
  std::vector<Ctrl<D7>> starts, ends;
  explicit UprightProblems(int n) {
    const double H = 1.5707963267948966, pi = 3.14159265358979323846;
    chain.n_joints = 7;
    const double a[7] = {0, 0, 0.0825, -0.0825, 0, 0.088, 0}, d[7] = {0.333, 0, 0.316, 0, 0.384, 0, 0.107};
    const double alpha[7] = {-H, H, H, -H, H, H, 0.3}, theta0[7] = {0, 0, 0, 0.25, 0, 0, -0.7};
    for (int i = 0; i < 7; ++i) { chain.a[i] = a[i]; chain.d[i] = d[i]; chain.alpha[i] = alpha[i]; chain.theta0[i] = theta0[i]; }
    balls = {dhBall(chain, 2, {0, 0, 0}, 0.09), dhBall(chain, 3, {0, 0.05, -0.1}, 0.08), dhBall(chain, 4, {0.02, 0, 0.03}, 0.07),
             dhBall(chain, 5, {0, 0.04, -0.15}, 0.07), dhBall(chain, 6, {0.03, 0, 0}, 0.06), dhBall(chain, 7, {0, 0, -0.05}, 0.05),
             dhBall(chain, 7, {0.02, -0.01, 0.06}, 0.04, true)};
    // the tool points down: its axis within 15 degrees of -z, the row active from 5 degrees inside the cone
    tilts = {dhTilt(chain, 7, {0, 0, 1}, {0, 0, -1}, 15 * kDeg, 5 * kDeg)};
    pos = constraints::inRange<D7>(constraints::of<D7>(-2 * pi), constraints::of<D7>(2 * pi));
    vel = constraints::inRange<D7>(constraints::of<D7>(-pi), constraints::of<D7>(pi));
    acc = constraints::inRange<D7>(constraints::of<D7>(-pi * 800 / 180), constraints::of<D7>(pi * 800 / 180));
    // the tool is within 0.2 degrees of vertical at both postures; along the straight line between them it tips far over
    const double A[7] = {-0.273, 0.728, -0.584, -1.6, 0.101, 1.877, 1.025}, B[7] = {-1.283, 1.929, -2.018, -2.923, 1.301, 1.35, -0.775};
    for (int b = 0; b < n; ++b) {
      Ctrl<D7> s{}, e{};
      for (int j = 0; j < 7; ++j) { s[j] = A[j] + 0.004 * b * ((j % 3) - 1); e[j] = B[j] - 0.004 * b * ((j % 2) ? 1 : -1); }
      starts.push_back(s); ends.push_back(e);
    }
  }
};

// the largest tilt angle along a trajectory, radians
template <size_t D>
static double maxTilt(const TiltLimit &t, const QPVector &x) {
  double worst = 0.0;
  for (size_t w = 0; w < x.size() / 2 / D; ++w) worst = std::fmax(worst, std::acos(std::fmax(-1.0, std::fmin(1.0, tiltCosine<D>(t, x.data() + w * D)))));
  return worst;
}

static int run_checks() {
  UprightProblems pr(1);
  const TiltLimit &t = pr.tilts[0];
  CHECK(t.builtin_frame == 7 && t.cosLimit() == std::cos(15 * kDeg) && t.cosActive() == std::cos(15 * kDeg - 5 * kDeg) && t.cosOK() == std::cos(15 * kDeg + 1e-3));
  TiltLimit wide = dhTilt(pr.chain, 3, {1, 0, 0}, {0, 1, 0}, 3.1411, 4.0);
  CHECK(wide.cosActive() == 1.0 && wide.cosOK() == std::cos(3.14159265358979323846));            // the clamps at 0 and pi
  CHECK(t == pr.tilts[0] && !(t == wide));
  // dh::axis: the derivative against central differences; nothing from the frame on
  const double q[7] = {0.3, -0.8, 1.1, -1.7, 0.4, 2.0, -0.6}, a[3] = {0.6, 0.0, 0.8};
  double worst = 0.0;
  for (int frame = 1; frame <= 7; ++frame) {
    double u[3], dU[21];
    mi_osqp::dh::axis(pr.chain, q, frame, a, u, dU);
    CHECK(std::fabs(u[0] * u[0] + u[1] * u[1] + u[2] * u[2] - 1.0) < 1e-14);
    for (int j = 0; j < 7; ++j) {
      double qp[7], qm[7], up[3], um[3];
      for (int k = 0; k < 7; ++k) { qp[k] = q[k] + (k == j ? 1e-6 : 0.0); qm[k] = q[k] - (k == j ? 1e-6 : 0.0); }
      mi_osqp::dh::axis(pr.chain, qp, frame, a, up, nullptr);
      mi_osqp::dh::axis(pr.chain, qm, frame, a, um, nullptr);
      for (int r = 0; r < 3; ++r) {
        worst = std::fmax(worst, std::fabs((up[r] - um[r]) / 2e-6 - dU[r * 7 + j]));
        if (j >= frame) CHECK(dU[r * 7 + j] == 0.0);
      }
    }
  }
  std::printf("dh::axis against central differences: %.3e\n", worst);
  CHECK(worst < 1e-9);
  // tiltsOK: a 2-joint chain on which the tilt angle is |q_1|; accepted up to max_angle + 1 mrad
  mi_gomp_chain c2{};
  c2.n_joints = 2; c2.alpha[0] = 1.5707963267948966;
  const std::vector<TiltLimit> two{dhTilt(c2, 2, {0, 1, 0}, {0, 0, 1}, 0.5, 0.125)};
  const double in[2] = {0.3, 0.5 + 1e-3 - 1e-6}, out[2] = {0.3, -(0.5 + 1e-3 + 1e-6)};
  CHECK(tiltsOK<2>(two, in) && !tiltsOK<2>(two, out) && tiltsOK<2>({}, out));
  QPVector x(2 * 2 * 4, 0.0);
  CHECK(tiltsOKAlong<2>(two, x));
  x[2 * 2 + 1] = 0.6;
  CHECK(!tiltsOKAlong<2>(two, x) && tiltsOKAlong<2>({}, x));
  double g[2];
  CHECK(std::fabs(tiltCosine<2>(two[0], in, g) - std::cos(in[1])) < 1e-15 && std::fabs(g[1] + std::sin(in[1])) < 1e-15 && std::fabs(g[0]) < 1e-15);
  std::printf(fails ? "CHECKS FAILED (%d)\n" : "CHECKS OK\n", fails);
  return fails ? 1 : 0;
}

static int run_tilt_oracle(int W) {
  UprightProblems pr(2);
  const TiltLimit &t = pr.tilts[0];
  for (size_t b = 0; b < pr.starts.size(); ++b) {
    QPVector line = linspace<D7>(pr.starts[b], pr.ends[b], (size_t)W);
    line.resize(2 * (size_t)W * D7, 0.0);
    const double t_line = maxTilt<D7>(t, line);
    CHECK(t_line > 2 * t.max_angle);
    double tip[2];
    for (int with = 0; with < 2; ++with) {
      GOMPSolver<D7, OracleQPSolver> o((size_t)W, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls, nullptr, false);
      if (with) o.tilts = pr.tilts;
      auto [code, x] = o.run(pr.starts[b], pr.ends[b]);
      tip[with] = maxTilt<D7>(t, x);
      std::printf("upright traj %zu %s tilt limit: %s segments %d solves %d updates %d, %zu waypoints, largest tilt %.3f deg (straight line %.3f deg)\n", b,
                  with ? "with" : "without", ToString(code).c_str(), o.segments_run, o.qp_solves, o.qp_updates, x.size() / 2 / D7, tip[with] / kDeg, t_line / kDeg);
      CHECK(code == ExitCode::kOptimal);
      if (with) { CHECK(o.qp_updates >= 1); CHECK(o.acceptable(x)); }
    }
    CHECK(tip[0] > t.max_angle + 1e-3);                        // without the limit the plan tips the tool over
    CHECK(tip[1] <= t.max_angle + 1e-3);                       // with it the tool stays upright
  }
  std::printf(fails ? "TILT ORACLE FAILED (%d)\n" : "TILT ORACLE OK\n", fails);
  return fails ? 1 : 0;
}

static int run_cont() {
  UprightProblems pr(2);
  const TiltLimit &t = pr.tilts[0];
  ContinuousGOMPSolver<D7> host(20, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls), dev(20, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls);
  host.tilts = dev.tilts = pr.tilts;
  dev.device_assembly = true;
  dev.dh_chain = pr.chain;
  auto rh = host.run(pr.starts, pr.ends);
  auto rd = dev.run(pr.starts, pr.ends);
  double worst = 0.0, tip = 0.0;
  int updates = 0, planned = 0;
  for (size_t b = 0; b < pr.starts.size(); ++b) {
    std::printf("upright traj %zu host: %s segments %d solves %d updates %d | device: %s %d %d %d\n", b, ToString(rh[b].first).c_str(), host.segments_run[b],
                host.qp_solves[b], host.qp_updates[b], ToString(rd[b].first).c_str(), dev.segments_run[b], dev.qp_solves[b], dev.qp_updates[b]);
    CHECK(rh[b].first == rd[b].first);
    CHECK(host.segments_run[b] == dev.segments_run[b] && host.qp_solves[b] == dev.qp_solves[b] && host.qp_updates[b] == dev.qp_updates[b]);
    CHECK(rh[b].second.size() == rd[b].second.size());
    for (size_t k = 0; k < rh[b].second.size() && k < rd[b].second.size(); ++k) worst = std::fmax(worst, std::fabs(rh[b].second[k] - rd[b].second[k]));
    updates += dev.qp_updates[b];
    if (rd[b].first == ExitCode::kOptimal) { ++planned; tip = std::fmax(tip, maxTilt<D7>(t, rd[b].second)); }
  }
  std::printf("upright: continuous planner with a tilt limit, device assembly vs host assembly: %zu trajectories (%d planned), %d re-linearisations on the device, "
              "max |dx| %.3e, largest tilt %.3f deg (limit %.3f deg)\n", pr.starts.size(), planned, updates, worst, tip / kDeg, t.max_angle / kDeg);
  CHECK(updates > 0);
  CHECK(planned == 2 && tip <= t.max_angle + 1e-3);
  CHECK(worst <= 1e-6);
  // the kept scenes are made again when the limits change: the same planner without them tips the tool over
  dev.tilts.clear();
  auto rn = dev.run(pr.starts, pr.ends);
  for (size_t b = 0; b < pr.starts.size(); ++b) {
    const double tn = rn[b].first == ExitCode::kOptimal ? maxTilt<D7>(t, rn[b].second) : 0.0;
    std::printf("upright traj %zu without the limit: %s, largest tilt %.3f deg\n", b, ToString(rn[b].first).c_str(), tn / kDeg);
    CHECK(rn[b].first == ExitCode::kOptimal && tn > t.max_angle + 1e-3);
  }
  std::printf(fails ? "CONT FAILED (%d)\n" : "CONT OK\n", fails);
  return fails ? 1 : 0;
}

int main(int argc, char **argv) {
  setenv("GPU_MAX_HW_QUEUES", "10", 0);                 // one hardware queue per horizon stage, as the planner examples set it
  if (argc > 2 && !std::strcmp(argv[1], "rows")) {
    std::ifstream in(argv[2]);
    if (!in) { std::printf("cannot read %s\n", argv[2]); return 2; }
    std::string t;
    in >> t;
    const int D = std::atoi(t.c_str());
    return D == 2 ? run_rows<2>(in) : D == 3 ? run_rows<3>(in) : 2;
  }
  if (argc > 1 && !std::strcmp(argv[1], "checks")) return run_checks();
  if (argc > 1 && !std::strcmp(argv[1], "tilt_oracle")) return run_tilt_oracle(argc > 2 ? std::atoi(argv[2]) : 20);
  if (argc > 1 && !std::strcmp(argv[1], "cont")) return run_cont();
  std::printf("usage: gomp_tilt rows FILE | checks | tilt_oracle [W] | cont\n");
  return 2;
}
