// tests/cpp/gomp_grid.cpp -- TEST PROGRAM (links the oracle; never part of the product): distance grids (DistanceGrid in
// include/mi_osqp/gomp.hpp, mi_gomp_grid) on the host and through the planners.
//
//   ./gomp_grid rows FILE    CPU: FILE holds a scene of TABLE balls (D = 3), lines, capsules, cuboids, grids, the work-space
//                            limits, trajectories, sample points and a fromObstacles case as hexadecimal floats (written by
//                            tests/test_gomp_grid_cpp.py); prints the populated 3-D rows of ConstraintBuilder<3>::withObstacles
//                            as lines "R t row v0 v1 v2 l u" in %a, the verdict of GOMPSolver::isSolutionOK as "V t ok", the
//                            samples of grid 0 as "S i inside phi gx gy gz" and the nodes of fromObstacles as "F k v"; checks
//                            that a builder with an empty grid list gives the rows of the seven-argument builder bit for bit.
//   ./gomp_grid oracle       CPU: a point robot passes the corner of a box that exists only as a grid (fromObstacles),
//                            sequential GOMPSolver on the oracle backend; the host twin on the corner cases of the formulas.
//   ./gomp_grid cont         GPU: the same problem, 4 trajectories of 20 waypoints, through ContinuousGOMPSolver with the SQP
//                            step on the device (grids in the scene) against the same planner on the host callbacks and
//                            through BatchGOMPSolver: exit codes, counters, trajectories within 1e-6; then updateGrid.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>

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
  std::vector<DistanceGrid> grids;
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
  const int ng = (int)num();
  for (int k = 0; k < ng; ++k) {
    Point o;
    for (double &v : o) v = num();
    const double cell = num();
    std::array<int, 3> n;
    for (int &v : n) v = (int)num();
    const double offset = num(), margin = num();
    std::vector<double> vals((size_t)n[0] * n[1] * n[2]);
    for (double &v : vals) v = num();
    grids.emplace_back(o, cell, n, std::move(vals), offset, margin);
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
  for (const RobotBall &b : balls) rows3d += W * ((b.is_gripper ? 3 : 0) + lines.size() + caps.size() + cubs.size() + grids.size());
  for (int t = 0; t < nt; ++t) {
    QPVector x(2 * 3 * W);
    for (double &v : x) v = num();
    if (!in) { std::printf("short file\n"); return 2; }
    ConstraintBuilder<3> b{W, balls, lines, caps, cubs, {}, {}, grids};
    const auto [l, A, u] = b.withObstacles(c3d, x).build();
    CHECK(l.size() == (W - 1) * 3 + 3 * (W + W - 1 + W - 2 + W * (3 + (lines.size() + caps.size() + cubs.size() + grids.size()) * balls.size())));
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
    g.grids = grids;
    std::printf("V %d %d\n", t, g.acceptable(x) ? 1 : 0);
    // no grids: the eight-argument builder with an empty list is the seven-argument one, bit for bit
    ConstraintBuilder<3> b7{W, balls, lines, caps, cubs, {}, {}}, b8{W, balls, lines, caps, cubs, {}, {}, {}};
    const auto [l7, A7, u7] = b7.withObstacles(c3d, x).build();
    const auto [l8, A8, u8] = b8.withObstacles(c3d, x).build();
    CHECK(l7.size() == l8.size() && !std::memcmp(l7.data(), l8.data(), l7.size() * sizeof(double)) && !std::memcmp(u7.data(), u8.data(), u7.size() * sizeof(double)));
    CHECK(A7.outer == A8.outer && A7.inner == A8.inner && A7.values.size() == A8.values.size() &&
          !std::memcmp(A7.values.data(), A8.values.data(), A7.values.size() * sizeof(double)));
    const auto [lp, Ap, up] = ConstraintBuilder<3>{W, balls, lines, caps, cubs, {}, {}, grids}.withObstaclePattern().build();
    CHECK(Ap.outer == A.outer && Ap.inner == A.inner);                      // the pattern ahead of time
  }
  const int ns = (int)num();
  for (int i = 0; i < ns; ++i) {
    Point p;
    for (double &v : p) v = num();
    const DistanceGrid::Sample s = grids[0].sample(p);
    std::printf("S %d %d %a %a %a %a\n", i, s.inside ? 1 : 0, s.phi, s.grad[0], s.grad[1], s.grad[2]);
  }
  if ((int)num() == 1) {                                                    // fromObstacles over a box and a capsule
    Point o, bc, bh, ca, cb;
    for (double &v : o) v = num();
    const double cell = num();
    std::array<int, 3> n;
    for (int &v : n) v = (int)num();
    for (double &v : bc) v = num();
    for (double &v : bh) v = num();
    for (double &v : ca) v = num();
    for (double &v : cb) v = num();
    const double cr = num();
    if (!in) { std::printf("short file\n"); return 2; }
    const DistanceGrid g = DistanceGrid::fromObstacles(o, cell, n, {CapsuleObstacle(ca, cb, cr)}, {CuboidObstacle(bc, bh)}, 0.01, 0.05);
    CHECK(g.offset == 0.01 && g.margin == 0.05 && g.values->size() == (size_t)n[0] * n[1] * n[2]);
    for (size_t k = 0; k < g.values->size(); ++k) std::printf("F %zu %a\n", k, (*g.values)[k]);
  }
  std::printf(fails ? "ROWS FAILED (%d)\n" : "ROWS OK\n", fails);
  return fails ? 1 : 0;
}

// ---- a point robot (TABLE model, identity) of radius 0.05 passes the corner of a box that exists only as a grid
constexpr size_t D3 = 3;
struct PointProblems {
  std::vector<RobotBall> balls{tableBall({1, 0, 0, 0, 1, 0, 0, 0, 1}, 0.05, false)};
  CuboidObstacle box = CuboidObstacle::oriented({0.0, -0.15, 0.0}, {std::cos(0.4), std::sin(0.4), 0.0, -std::sin(0.4), std::cos(0.4), 0.0, 0.0, 0.0, 1.0}, {0.15, 0.15, 0.4});   // turned about z
  // 41 x 33 x 5 nodes of 0.025 around the box: x -0.5 .. 0.5, y -0.4 .. 0.4, z -0.05 .. 0.05 (the plane the robot moves in)
  std::vector<DistanceGrid> grids{DistanceGrid::fromObstacles({-0.5, -0.4, -0.05}, 0.025, {41, 33, 5}, {}, {box}, 0.0, 0.02)};
  Constraint<D3> pos = constraints::inRange<D3>(constraints::of<D3>(-2.0), constraints::of<D3>(2.0));
  Constraint<D3> vel = constraints::inRange<D3>(constraints::of<D3>(-1.0), constraints::of<D3>(1.0));
  Constraint<D3> acc = constraints::inRange<D3>(constraints::of<D3>(-4.0), constraints::of<D3>(4.0));
  Constraint<3> c3d = constraints::any<3>();
  std::vector<Ctrl<D3>> starts, ends;
  PointProblems() {
    for (int b = 0; b < 4; ++b) {
      starts.push_back({-0.6, 0.03 + 0.02 * b, -0.004 * b});
      ends.push_back({0.6, 0.02 * (b % 3), 0.008 - 0.002 * b});
    }
  }
};

// the true clearance from the box the grid was sampled from
static double minClearance(const CuboidObstacle &box, const std::vector<RobotBall> &balls, const QPVector &x, size_t D) {
  double worst = INF;
  const size_t W = x.size() / 2 / D;
  for (const RobotBall &ball : balls)
    for (size_t w = 0; w < W; ++w) {
      std::vector<double> q(x.begin() + (long)(w * D), x.begin() + (long)((w + 1) * D));
      auto [px, py, pz] = ball.fk(q.data());
      worst = std::fmin(worst, box.clearance({px, py, pz}, ball));
    }
  return worst;
}

static void host_twin_cases() {
  // two nodes per axis, phi = x + 2 y + 4 z in cell units
  const DistanceGrid g({1.0, 2.0, 3.0}, 0.5, {2, 2, 2}, std::vector<double>{0, 1, 2, 3, 4, 5, 6, 7}, 0.25, 0.125);
  const RobotBall ball = tableBall({1, 0, 0, 0, 1, 0, 0, 0, 1}, 0.0625, false);
  DistanceGrid::Sample s = g.sample({1.0, 2.0, 3.0});
  CHECK(s.inside && s.phi == 0.0 && s.grad == (Point{2.0, 4.0, 8.0}));
  s = g.sample({1.5, 2.5, 3.5});                                           // the last node: the last cell with t = 1
  CHECK(s.inside && s.phi == 7.0 && s.grad == (Point{2.0, 4.0, 8.0}));
  s = g.sample({1.25, 2.125, 3.375});
  CHECK(s.inside && s.phi == 0.5 + 2 * 0.25 + 4 * 0.75);
  CHECK(!g.sample({1.5 + 1e-9, 2.0, 3.0}).inside && !g.sample({1.0, 2.0 - 1e-9, 3.0}).inside && !g.sample({1.0, 2.0, std::nan("")}).inside);
  CHECK(!g.sample({INFINITY, 2.0, 3.0}).inside && !g.sample({1.0, -INFINITY, 3.0}).inside && !g.sample({1.0, 2.0, 1e300}).inside);
  CHECK(g.clearance({1.5, 2.5, 3.5}, ball) == 7.0 - 0.3125 && g.clearance({9.0, 2.0, 3.0}, ball) == INF);
  CHECK(gridsClear({g}, {1.5, 2.5, 3.5}, ball) && !gridsClear({g}, {1.0, 2.0, 3.0}, ball) && gridsClear({g}, {0.0, 0.0, 0.0}, ball));
  DistanceGrid h = g;                                                      // a copy shares the values
  CHECK(h == g && h.values == g.values && !(g == DistanceGrid({1.0, 2.0, 3.0}, 0.5, {2, 2, 2}, std::vector<double>{0, 1, 2, 3, 4, 5, 6, 8}, 0.25, 0.125)));
}

static int run_oracle() {
  host_twin_cases();
  PointProblems pr;
  GOMPSolver<D3, OracleQPSolver> o(40, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls, nullptr, false);
  o.grids = pr.grids;
  auto [code, x] = o.run(pr.starts[0], pr.ends[0]);
  const double clear = minClearance(pr.box, pr.balls, x, D3);
  std::printf("point robot past a gridded box corner: %s segments %d solves %d updates %d, %zu waypoints, minimum clearance from the box %.6f\n",
              ToString(code).c_str(), o.segments_run, o.qp_solves, o.qp_updates, x.size() / 2 / D3, clear);
  CHECK(code == ExitCode::kOptimal);
  CHECK(o.qp_updates >= 1);
  CHECK(clear >= -1e-3 - 0.005);                                           // the interpolant rounds the corner off by less than a fifth of a cell
  CHECK(o.acceptable(x));
  QPVector line = linspace<D3>(pr.starts[0], pr.ends[0], 40);              // the straight line it started from goes through the box
  line.resize(2 * 40 * D3, 0.0);
  CHECK(minClearance(pr.box, pr.balls, line, D3) < -0.01 && !o.acceptable(line));
  std::printf(fails ? "ORACLE FAILED (%d)\n" : "ORACLE OK\n", fails);
  return fails ? 1 : 0;
}

static int run_cont() {
  PointProblems pr;
  ContinuousGOMPSolver<D3> host(20, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls), dev(20, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls);
  BatchGOMPSolver<D3> batch(20, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls);
  host.grids = dev.grids = batch.grids = pr.grids;
  dev.device_assembly = true;
  auto rh = host.run(pr.starts, pr.ends);
  auto rd = dev.run(pr.starts, pr.ends);
  auto rb = batch.run(pr.starts, pr.ends);
  double worst = 0.0, worst_batch = 0.0, clear = INF;
  int updates = 0, planned = 0;
  for (size_t b = 0; b < pr.starts.size(); ++b) {
    std::printf("traj %zu host: %s segments %d solves %d updates %d | device: %s %d %d %d | batch: %s\n", b, ToString(rh[b].first).c_str(), host.segments_run[b],
                host.qp_solves[b], host.qp_updates[b], ToString(rd[b].first).c_str(), dev.segments_run[b], dev.qp_solves[b], dev.qp_updates[b], ToString(rb[b].first).c_str());
    CHECK(rh[b].first == rd[b].first && rh[b].first == rb[b].first);
    CHECK(host.segments_run[b] == dev.segments_run[b] && host.qp_solves[b] == dev.qp_solves[b] && host.qp_updates[b] == dev.qp_updates[b]);
    CHECK(rh[b].second.size() == rd[b].second.size() && rh[b].second.size() == rb[b].second.size());
    for (size_t k = 0; k < rh[b].second.size() && k < rd[b].second.size(); ++k) worst = std::fmax(worst, std::fabs(rh[b].second[k] - rd[b].second[k]));
    for (size_t k = 0; k < rh[b].second.size() && k < rb[b].second.size(); ++k) worst_batch = std::fmax(worst_batch, std::fabs(rh[b].second[k] - rb[b].second[k]));
    updates += dev.qp_updates[b];
    if (rd[b].first == ExitCode::kOptimal) { ++planned; clear = std::fmin(clear, minClearance(pr.box, pr.balls, rd[b].second, D3)); }
  }
  std::printf("continuous planner with a grid, device assembly vs host assembly: %zu trajectories (%d planned), %d re-linearisations on the device, "
              "max |dx| %.3e (batch planner vs host: %.3e), minimum clearance from the box %.6f\n", pr.starts.size(), planned, updates, worst, worst_batch, clear);
  CHECK(updates > 0);
  CHECK(planned > 0 && clear >= -1e-3 - 0.005);
  CHECK(worst <= 1e-6 && worst_batch <= 1e-6);
  // a new camera frame: the box has gone; the kept device scenes take the new values and every straight line is accepted at once
  std::vector<double> far(pr.grids[0].values->size(), 1.0);
  CHECK(dev.updateGrid(0, far) && host.updateGrid(0, far));
  CHECK(!dev.updateGrid(1, far) && !dev.updateGrid(0, std::vector<double>(7, 1.0)));
  auto rh2 = host.run(pr.starts, pr.ends);
  auto rd2 = dev.run(pr.starts, pr.ends);
  double worst2 = 0.0;
  for (size_t b = 0; b < pr.starts.size(); ++b) {
    CHECK(rh2[b].first == ExitCode::kOptimal && rd2[b].first == ExitCode::kOptimal && dev.qp_updates[b] == 0 && host.qp_updates[b] == 0);
    for (size_t k = 0; k < rh2[b].second.size() && k < rd2[b].second.size(); ++k) worst2 = std::fmax(worst2, std::fabs(rh2[b].second[k] - rd2[b].second[k]));
  }
  std::printf("after updateGrid (an empty world): no re-linearisation, %d solver reuses, max |dx| %.3e\n", (int)dev.solver_reuses, worst2);
  CHECK(worst2 <= 1e-6 && dev.solver_reuses > 0);
  std::printf(fails ? "CONT FAILED (%d)\n" : "CONT OK\n", fails);
  return fails ? 1 : 0;
}

int main(int argc, char **argv) {
  setenv("GPU_MAX_HW_QUEUES", "10", 0);                 // one hardware queue per horizon stage, as the planner examples set it
  if (argc > 2 && !std::strcmp(argv[1], "rows")) return run_rows(argv[2]);
  if (argc > 1 && !std::strcmp(argv[1], "oracle")) return run_oracle();
  if (argc > 1 && !std::strcmp(argv[1], "cont")) return run_cont();
  std::printf("usage: gomp_grid rows FILE | oracle | cont\n");
  return 2;
}
