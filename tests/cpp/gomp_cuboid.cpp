// tests/cpp/gomp_cuboid.cpp -- TEST PROGRAM (links the oracle; never part of the product): cuboid obstacles (CuboidObstacle in
// include/mi_osqp/gomp.hpp, mi_gomp_cuboid) on the host and through the planners.
//
//   ./gomp_cuboid rows FILE    CPU: FILE holds a scene of TABLE balls (D = 3), lines, capsules, cuboids, the work-space limits and
//                              trajectories as hexadecimal floats (written by tests/test_gomp_cuboid_cpp.py); prints the
//                              populated 3-D rows of ConstraintBuilder<3>::withObstacles as lines "R t row v0 v1 v2 l u" in %a
//                              and the verdict of GOMPSolver::isSolutionOK as "V t ok"; checks that a builder with an empty
//                              cuboid list gives the rows of the four-argument builder bit for bit.
//   ./gomp_cuboid oracle       CPU: a point robot passes a box corner, sequential GOMPSolver on the oracle backend; the host
//                              twin's signedDistance / normal on the corner cases of the formulas.
//   ./gomp_cuboid bin_oracle   CPU: the 7-joint bin scene of `cont` through the sequential driver on the oracle backend.
//   ./gomp_cuboid cont         GPU: ContinuousGOMPSolver with the SQP step on the device (cuboids in the scene) against the
//                              same planner on the host callbacks: a 3-joint scene with 4 trajectories of 20 waypoints and the
//                              7-joint bin scene with 2 trajectories of 20 waypoints; exit codes, counters, trajectories within 1e-6.
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

static int run_rows(const char *path) {
  std::ifstream in(path);
  if (!in) { std::printf("cannot read %s\n", path); return 2; }
  auto num = [&in]() { std::string t; in >> t; return std::strtod(t.c_str(), nullptr); };
  std::vector<RobotBall> balls;
  std::vector<HorizontalLine> lines;
  std::vector<CapsuleObstacle> caps;
  std::vector<CuboidObstacle> cubs;
  const int nb = (int)num();
  for (int b = 0; b < nb; ++b) {
    const bool gripper = num() != 0;
    const double radius = num();
    std::array<double, 9> T;
    for (double &v : T) v = num();
    balls.push_back(tableBall(T, radius, gripper));
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
  Vec<3> lo, hi;
  for (double &v : lo) v = num();
  for (double &v : hi) v = num();
  const Constraint<3> c3d = constraints::inRange<3>(lo, hi);
  const size_t W = (size_t)num();
  const int nt = (int)num();
  if (!in || W < 4) { std::printf("short file\n"); return 2; }
  const Constraint<3> any = constraints::any<3>();
  const size_t row0 = (W - 1) * 3 + 3 * (W + W - 1 + W - 2);
  size_t rows3d = 0;
  for (const RobotBall &b : balls) rows3d += W * ((b.is_gripper ? 3 : 0) + lines.size() + caps.size() + cubs.size());
  for (int t = 0; t < nt; ++t) {
    QPVector x(2 * 3 * W);
    for (double &v : x) v = num();
    if (!in) { std::printf("short file\n"); return 2; }
    ConstraintBuilder<3> b{W, balls, lines, caps, cubs};
    const auto [l, A, u] = b.withObstacles(c3d, x).build();
    CHECK(l.size() == (W - 1) * 3 + 3 * (W + W - 1 + W - 2 + W * (3 + (lines.size() + caps.size() + cubs.size()) * balls.size())));
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
    for (size_t r = row0 + rows3d; r < l.size(); ++r) CHECK(l[r] == -INF && u[r] == INF);
    GOMPSolver<3, OracleQPSolver> g(W, 0.1, any, any, any, c3d, lines, balls);
    g.capsules = caps;
    g.cuboids = cubs;
    std::printf("V %d %d\n", t, g.acceptable(x) ? 1 : 0);
    // no cuboids: the five-argument builder with an empty list is the four-argument one, bit for bit
    ConstraintBuilder<3> b4{W, balls, lines, caps}, b5{W, balls, lines, caps, {}};
    const auto [l4, A4, u4] = b4.withObstacles(c3d, x).build();
    const auto [l5, A5, u5] = b5.withObstacles(c3d, x).build();
    CHECK(l4.size() == l5.size() && !std::memcmp(l4.data(), l5.data(), l4.size() * sizeof(double)) && !std::memcmp(u4.data(), u5.data(), u4.size() * sizeof(double)));
    CHECK(A4.outer == A5.outer && A4.inner == A5.inner && A4.values.size() == A5.values.size() &&
          !std::memcmp(A4.values.data(), A5.values.data(), A4.values.size() * sizeof(double)));
    const auto [lp4, Ap4, up4] = ConstraintBuilder<3>{W, balls, lines, caps}.withObstaclePattern().build();
    const auto [lp5, Ap5, up5] = ConstraintBuilder<3>{W, balls, lines, caps, cubs}.withObstaclePattern().build();
    CHECK(Ap4.outer == A4.outer && Ap4.inner == A4.inner && Ap5.outer == A.outer && Ap5.inner == A.inner);      // the pattern ahead of time
  }
  std::printf(fails ? "ROWS FAILED (%d)\n" : "ROWS OK\n", fails);
  return fails ? 1 : 0;
}

// ---- a point robot (TABLE model, identity) of radius 0.05 passes the corner of a box turned about z
constexpr size_t D3 = 3;
static CuboidObstacle::Axes turnedAboutZ(double a) { return {std::cos(a), std::sin(a), 0.0, -std::sin(a), std::cos(a), 0.0, 0.0, 0.0, 1.0}; }
struct PointProblems {
  std::vector<RobotBall> balls{tableBall({1, 0, 0, 0, 1, 0, 0, 0, 1}, 0.05, false)};
  std::vector<CuboidObstacle> cubs{CuboidObstacle::oriented({0.0, -0.15, 0.0}, turnedAboutZ(0.4), {0.15, 0.15, 0.4}, 0.0, 0.02)};
  Constraint<D3> pos = constraints::inRange<D3>(constraints::of<D3>(-2.0), constraints::of<D3>(2.0));
  Constraint<D3> vel = constraints::inRange<D3>(constraints::of<D3>(-1.0), constraints::of<D3>(1.0));
  Constraint<D3> acc = constraints::inRange<D3>(constraints::of<D3>(-4.0), constraints::of<D3>(4.0));
  Constraint<3> c3d = constraints::any<3>();
  std::vector<Ctrl<D3>> starts, ends;
  PointProblems() {
    for (int b = 0; b < 4; ++b) {
      starts.push_back({-0.6, 0.03 + 0.02 * b, -0.02 * b});
      ends.push_back({0.6, 0.02 * (b % 3), 0.04 - 0.01 * b});
    }
  }
};

static double minClearance(const std::vector<CuboidObstacle> &cubs, const std::vector<RobotBall> &balls, const QPVector &x, size_t D) {
  double worst = INF;
  const size_t W = x.size() / 2 / D;
  for (const RobotBall &ball : balls)
    for (size_t w = 0; w < W; ++w) {
      std::vector<double> q(x.begin() + (long)(w * D), x.begin() + (long)((w + 1) * D));
      auto [px, py, pz] = ball.fk(q.data());
      for (const CuboidObstacle &c : cubs) worst = std::fmin(worst, c.clearance({px, py, pz}, ball));
    }
  return worst;
}

static void host_twin_cases() {
  const CuboidObstacle cube({1.0, 0.5, 0.25}, {0.25, 0.25, 0.25}, 0.125, 0.125);
  CHECK(cube.signedDistance({1.0, 0.5, 0.25}) == -0.25 && cube.normal({1.0, 0.5, 0.25}) == (Point{1.0, 0.0, 0.0}));          // three-way tie: k* = 0, +
  CHECK(cube.signedDistance({1.0, 0.375, 0.125}) == -0.125 && cube.normal({1.0, 0.375, 0.125}) == (Point{0.0, -1.0, 0.0}));  // two-way tie: the lower axis
  CHECK(cube.signedDistance({1.25, 0.5, 0.25}) == 0.0 && cube.normal({1.25, 0.5, 0.25}) == (Point{1.0, 0.0, 0.0}));          // on a face
  CHECK(cube.signedDistance({1.0, 0.5, -0.5}) == 0.5 && cube.normal({1.0, 0.5, -0.5}) == (Point{0.0, 0.0, -1.0}));           // outside, face region
  const RobotBall ball = tableBall({1, 0, 0, 0, 1, 0, 0, 0, 1}, 0.0625, false);
  CHECK(cube.clearance({1.0, 0.5, -0.5}, ball) == 0.5 - 0.1875);
  const CuboidObstacle slab = CuboidObstacle::oriented({1.0, 0.5, 0.25}, {0, 1, 0, 0, 0, 1, -1, 0, 0}, {1.0, 1.0, 0.015625}, 0.0, 0.0);
  CHECK(slab.normal({1.0, 0.375, 0.125}) == (Point{-1.0, 0.0, 0.0}) && slab.signedDistance({1.0, 0.375, 0.125}) == -0.015625);   // c_2 = -0.0: the + side of u_2 = -x
  CHECK(slab.normal({1.015625, 0.5, 0.25}) == (Point{1.0, 0.0, 0.0}) && slab.normal({1.0, 2.0, 0.25}) == (Point{0.0, 1.0, 0.0}));
  const CuboidObstacle point = CuboidObstacle::oriented({1.0, 0.5, 0.25}, {0, 1, 0, 0, 0, -1, 1, 0, 0}, {0.0, 0.0, 0.0}, 0.125, 0.125);
  CHECK(point.signedDistance({1.0, 0.5, 0.25}) == 0.0 && point.normal({1.0, 0.5, 0.25}) == (Point{0.0, 1.0, 0.0}));          // out = 0: +u_0
  CHECK(point == point && !(point == slab) && !(cube == CuboidObstacle({1.0, 0.5, 0.25}, {0.25, 0.25, 0.25}, 0.125, 0.25)));
  CHECK(cuboidsClear({cube, slab}, {1.0, 0.5, 2.0}, ball) && !cuboidsClear({cube, slab}, {1.0, 0.5, 0.25}, ball));
}

static int run_oracle() {
  host_twin_cases();
  PointProblems pr;
  GOMPSolver<D3, OracleQPSolver> o(40, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls, nullptr, false);
  o.cuboids = pr.cubs;
  auto [code, x] = o.run(pr.starts[0], pr.ends[0]);
  const double clear = minClearance(pr.cubs, pr.balls, x, D3);
  std::printf("point robot past a box corner: %s segments %d solves %d updates %d, %zu waypoints, minimum clearance %.6f\n", ToString(code).c_str(), o.segments_run,
              o.qp_solves, o.qp_updates, x.size() / 2 / D3, clear);
  CHECK(code == ExitCode::kOptimal);
  CHECK(o.qp_updates >= 1);
  CHECK(clear >= -1e-3);
  // the straight line it started from goes through the box
  QPVector line = linspace<D3>(pr.starts[0], pr.ends[0], 40);
  line.resize(2 * 40 * D3, 0.0);
  CHECK(minClearance(pr.cubs, pr.balls, line, D3) < -0.05);
  std::printf(fails ? "ORACLE FAILED (%d)\n" : "ORACLE OK\n", fails);
  return fails ? 1 : 0;
}

template <size_t D>
static void compare(const char *what, ContinuousGOMPSolver<D> &host, ContinuousGOMPSolver<D> &dev, const std::vector<Ctrl<D>> &starts, const std::vector<Ctrl<D>> &ends,
                    const std::vector<RobotBall> &balls) {
  auto rh = host.run(starts, ends);
  auto rd = dev.run(starts, ends);
  double worst = 0.0, clear = INF;
  int updates = 0, planned = 0;
  for (size_t b = 0; b < starts.size(); ++b) {
    std::printf("%s traj %zu host: %s segments %d solves %d updates %d | device: %s %d %d %d\n", what, b, ToString(rh[b].first).c_str(), host.segments_run[b],
                host.qp_solves[b], host.qp_updates[b], ToString(rd[b].first).c_str(), dev.segments_run[b], dev.qp_solves[b], dev.qp_updates[b]);
    CHECK(rh[b].first == rd[b].first);
    CHECK(host.segments_run[b] == dev.segments_run[b] && host.qp_solves[b] == dev.qp_solves[b] && host.qp_updates[b] == dev.qp_updates[b]);
    CHECK(rh[b].second.size() == rd[b].second.size());
    for (size_t k = 0; k < rh[b].second.size() && k < rd[b].second.size(); ++k) worst = std::fmax(worst, std::fabs(rh[b].second[k] - rd[b].second[k]));
    updates += dev.qp_updates[b];
    if (rd[b].first == ExitCode::kOptimal) { ++planned; clear = std::fmin(clear, minClearance(dev.cuboids, balls, rd[b].second, D)); }
  }
  std::printf("%s: continuous planner with cuboids, device assembly vs host assembly: %zu trajectories (%d planned), %d re-linearisations on the device, "
              "max |dx| %.3e, minimum clearance %.6f\n", what, starts.size(), planned, updates, worst, clear);
  CHECK(updates > 0);
  CHECK(planned > 0 && clear >= -1e-3);
  CHECK(worst <= 1e-6);
}

// the 7-joint chain c7 of tests/dh_refs.py with its link balls reaches over the rim into a bin: four walls and a floor
constexpr size_t D7 = 7;
struct BinProblems {
  mi_gomp_chain chain{};
  std::vector<RobotBall> balls;
  std::vector<CuboidObstacle> cubs;
  Constraint<D7> pos, vel, acc;
  Constraint<3> c3d = constraints::inRange<3>(Vec<3>{-INF, -INF, 0.1}, Vec<3>{0.8, INF, INF});
  std::vector<Ctrl<D7>> starts, ends;
  explicit BinProblems(int n) {
    const double H = 1.5707963267948966, pi = 3.14159265358979323846;
    chain.n_joints = 7;
    const double a[7] = {0, 0, 0.0825, -0.0825, 0, 0.088, 0}, d[7] = {0.333, 0, 0.316, 0, 0.384, 0, 0.107};
    const double alpha[7] = {-H, H, H, -H, H, H, 0.3}, theta0[7] = {0, 0, 0, 0.25, 0, 0, -0.7};
    for (int i = 0; i < 7; ++i) { chain.a[i] = a[i]; chain.d[i] = d[i]; chain.alpha[i] = alpha[i]; chain.theta0[i] = theta0[i]; }
    balls = {dhBall(chain, 3, {0, 0.05, -0.1}, 0.08), dhBall(chain, 4, {0.02, 0, 0.03}, 0.07), dhBall(chain, 5, {0, 0.04, -0.15}, 0.07),
             dhBall(chain, 6, {0.03, 0, 0}, 0.06), dhBall(chain, 7, {0.02, -0.01, 0.06}, 0.04, true)};
    // the bin: inner 0.30 x 0.30 around (0.62, 0.37), floor top at z = 0.08, rim at z = 0.24, walls 0.02 thick
    const double cx = 0.62, cy = 0.37, in = 0.15, t = 0.01, z0 = 0.08, z1 = 0.24, m = 0.03;
    cubs = {CuboidObstacle({cx, cy, z0 - t}, {in + 2 * t, in + 2 * t, t}, 0.0, m),
            CuboidObstacle({cx - in - t, cy, (z0 + z1) / 2}, {t, in + 2 * t, (z1 - z0) / 2}, 0.0, m), CuboidObstacle({cx + in + t, cy, (z0 + z1) / 2}, {t, in + 2 * t, (z1 - z0) / 2}, 0.0, m),
            CuboidObstacle({cx, cy - in - t, (z0 + z1) / 2}, {in, t, (z1 - z0) / 2}, 0.0, m), CuboidObstacle({cx, cy + in + t, (z0 + z1) / 2}, {in, t, (z1 - z0) / 2}, 0.0, m)};
    pos = constraints::inRange<D7>(constraints::of<D7>(-2 * pi), constraints::of<D7>(2 * pi));
    vel = constraints::inRange<D7>(constraints::of<D7>(-pi), constraints::of<D7>(pi));
    acc = constraints::inRange<D7>(constraints::of<D7>(-pi * 800 / 180), constraints::of<D7>(pi * 800 / 180));
    const double base[7] = {0, 0.4, 0, -1.6, 0, 1.9, 0.6};
    for (int b = 0; b < n; ++b) {
      Ctrl<D7> s{}, e{};
      for (int j = 0; j < 7; ++j) { s[j] = base[j] + 0.02 * ((b + j) % 3 - 1); e[j] = base[j] - 0.02 * ((b + 2 * j) % 3 - 1); }
      s[0] = -0.5 + 0.1 * b; e[0] = 0.5 + 0.03 * b;              // from beside the bin ...
      e[1] = 0.8 - 0.03 * b;                                    // ... down into it
      starts.push_back(s); ends.push_back(e);
    }
  }
};

static int run_cont() {
  {
    PointProblems pr;
    ContinuousGOMPSolver<D3> host(20, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls), dev(20, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls);
    host.cuboids = dev.cuboids = pr.cubs;
    dev.device_assembly = true;
    compare<D3>("point", host, dev, pr.starts, pr.ends, pr.balls);
  }
  if (!fails) {
    BinProblems pr(2);
    ContinuousGOMPSolver<D7> host(20, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls), dev(20, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls);
    host.cuboids = dev.cuboids = pr.cubs;
    dev.device_assembly = true;
    dev.dh_chain = pr.chain;
    compare<D7>("bin", host, dev, pr.starts, pr.ends, pr.balls);
  }
  std::printf(fails ? "CONT FAILED (%d)\n" : "CONT OK\n", fails);
  return fails ? 1 : 0;
}

// the scenes of `cont` through the sequential driver on the oracle backend (CPU): what `cont` plans is plannable
static int run_bin_oracle() {
  int updates = 0, planned = 0;
  {
    PointProblems pr;
    for (size_t b = 0; b < pr.starts.size(); ++b) {
      GOMPSolver<D3, OracleQPSolver> o(20, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls, nullptr, false);
      o.cuboids = pr.cubs;
      auto [code, x] = o.run(pr.starts[b], pr.ends[b]);
      const double clear = minClearance(pr.cubs, pr.balls, x, D3);
      std::printf("point traj %zu %s segments %d solves %d updates %d minimum clearance %.6f\n", b, ToString(code).c_str(), o.segments_run, o.qp_solves, o.qp_updates, clear);
      CHECK(code == ExitCode::kOptimal && clear >= -1e-3 && o.qp_updates >= 1);
    }
  }
  BinProblems pr(2);
  for (size_t b = 0; b < pr.starts.size(); ++b) {
    GOMPSolver<D7, OracleQPSolver> o(20, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls, nullptr, false);
    o.cuboids = pr.cubs;
    auto [code, x] = o.run(pr.starts[b], pr.ends[b]);
    const double clear = minClearance(pr.cubs, pr.balls, x, D7);
    std::printf("bin traj %zu %s segments %d solves %d updates %d minimum clearance %.6f\n", b, ToString(code).c_str(), o.segments_run, o.qp_solves, o.qp_updates, clear);
    if (code == ExitCode::kOptimal) { ++planned; CHECK(clear >= -1e-3); }
    updates += o.qp_updates;
  }
  CHECK(planned == 2 && updates > 0);
  std::printf(fails ? "BIN ORACLE FAILED (%d)\n" : "BIN ORACLE OK\n", fails);
  return fails ? 1 : 0;
}

int main(int argc, char **argv) {
  setenv("GPU_MAX_HW_QUEUES", "10", 0);                 // one hardware queue per horizon stage, as the planner examples set it
  if (argc > 2 && !std::strcmp(argv[1], "rows")) return run_rows(argv[2]);
  if (argc > 1 && !std::strcmp(argv[1], "oracle")) return run_oracle();
  if (argc > 1 && !std::strcmp(argv[1], "bin_oracle")) return run_bin_oracle();
  if (argc > 1 && !std::strcmp(argv[1], "cont")) return run_cont();
  std::printf("usage: gomp_cuboid rows FILE | oracle | bin_oracle | cont\n");
  return 2;
}
