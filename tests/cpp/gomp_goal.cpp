// tests/cpp/gomp_goal.cpp -- TEST PROGRAM (links the oracle; never part of the product): grasp goals (GraspGoal / GoalTarget in
// include/mi_osqp/gomp.hpp, mi_gomp_goal) on the host and through the planners.
//
//   ./gomp_goal rows FILE      CPU: FILE holds a scene of 3 joints: a DH chain, TABLE, yaw + 2-link and chain balls, lines, capsules,
//                              cuboids, pairs, tilts, grids, goals, the work-space limits and per trajectory what it asks of every goal,
//                              as hexadecimal floats (written by tests/test_gomp_goal_cpp.py); prints the goal rows of
//                              ConstraintBuilder<3>::withObstacles as lines "R t row v0 .. l u" in %a, the rows before them as "N t count"
//                              and the verdicts as "V t goals scene"; checks the allocation, that a builder with an empty goal list gives
//                              the rows of the eight-argument builder bit for bit, and setGoalTarget on a copied template.
//   ./gomp_goal checks         CPU: goalOK at the 1 mm and the 1 mrad, a NaN, a free axis; dhGoal; goalWarmStart.
//   ./gomp_goal plan           CPU: the reach problem (7 joints, the tool axis down into a tolerance box) through the three planners on
//                              oracle backends: same exit codes and counters, trajectories bit for bit; the accepted end point inside
//                              tol + 1 mm and max_angle + 1 mrad; the cost against the fixed-end plan; a plan without a goal bit for
//                              bit what the parent commit planned (FILE of `plain`); the first QP of the goal run against the first QP
//                              of the fixed-end run.
//   ./gomp_goal plain          CPU: prints the fixed-end plan of the reach problem in %a (what tests/golden/goal_kats.json keeps).
//   ./gomp_goal cont           GPU: ContinuousGOMPSolver with the SQP step on the device (the goal in the scene, the targets set per
//                              arrival) against the same planner on the host callbacks on the reach problem.
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

static double g_eps = 1e-3;        // the oracle's eps_abs = eps_rel (its default; `plan` tightens it for the first-QP comparison)
static double g_last_obj = 0.0;

// QPSolver twin on the CPU oracle (as in gomp_parity.cpp)
class OracleQPSolver {
 public:
  OracleQPSolver(const QPConstraints &c, const QPMatrixSparse &P, bool = false) {
    const auto &[l, A, u] = c;
    oq_settings s; oq_default_settings(&s);
    s.eps_abs = s.eps_rel = g_eps;
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
    oq_info info;
    oq_get_info(w_, &info);
    g_last_obj = info.obj_val;
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

// BatchQPSolver twin: one oracle per QP, solved one after the other
class OracleBatchSolver {
 public:
  OracleBatchSolver(const std::vector<QPConstraints> &cons, const QPMatrixSparse &P, bool = false) {
    for (const QPConstraints &c : cons) qp_.push_back(std::make_unique<OracleQPSolver>(c, P));
  }
  bool reinit(const std::vector<QPConstraints> &, const QPMatrixSparse &) { return false; }      // always rebuilt
  void setWarmStart(const std::vector<QPVector> &x) { for (size_t k = 0; k < qp_.size(); ++k) qp_[k]->setWarmStart(x[k]); }
  void update(const std::vector<QPConstraints> &cons) { for (size_t k = 0; k < qp_.size(); ++k) qp_[k]->update(cons[k]); }
  std::vector<std::pair<OsqpExitCode, QPVector>> solve() {
    std::vector<std::pair<OsqpExitCode, QPVector>> r;
    for (auto &q : qp_) r.push_back(q->solve());
    return r;
  }
 private:
  std::vector<std::unique_ptr<OracleQPSolver>> qp_;
};

// ContinuousQPSolver twin: B slots; begin() queues, advance() solves what is queued, poll() hands it out
class OracleContSolver {
 public:
  OracleContSolver(long long B, const QPConstraints &c, const QPMatrixSparse &P, bool = false) : P_(P), rows_(std::get<0>(c).size()), qp_((size_t)B), res_((size_t)B) {}
  bool compatible(long long B, const QPConstraints &c, const QPMatrixSparse &) const { return (size_t)B == qp_.size() && std::get<0>(c).size() == rows_; }
  void reinit(const std::vector<long long> &ids, const std::vector<const QPConstraints *> &cs) {
    for (size_t k = 0; k < ids.size(); ++k) qp_[(size_t)ids[k]] = std::make_unique<OracleQPSolver>(*cs[k], P_);
  }
  void update(const std::vector<long long> &ids, const std::vector<const QPConstraints *> &cs) {
    for (size_t k = 0; k < ids.size(); ++k) qp_[(size_t)ids[k]]->update(*cs[k]);
  }
  void setWarmStart(const std::vector<long long> &ids, const std::vector<const QPVector *> &xs) {
    for (size_t k = 0; k < ids.size(); ++k) qp_[(size_t)ids[k]]->setWarmStart(*xs[k]);
  }
  void begin(const std::vector<long long> &ids) { queued_.insert(queued_.end(), ids.begin(), ids.end()); }
  size_t running() const { return queued_.size(); }
  bool advance(int) {
    for (long long id : queued_) { res_[(size_t)id] = qp_[(size_t)id]->solve(); done_.push_back(id); }
    queued_.clear();
    return true;
  }
  std::vector<long long> poll() { std::vector<long long> d; d.swap(done_); return d; }
  std::pair<OsqpExitCode, QPVector> result(long long id) const { return res_[(size_t)id]; }
  mi_osqp_batch *handle() { return nullptr; }
 private:
  QPMatrixSparse P_;
  size_t rows_;
  std::vector<std::unique_ptr<OracleQPSolver>> qp_;
  std::vector<std::pair<OsqpExitCode, QPVector>> res_;
  std::vector<long long> queued_, done_;
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

static bool sameBits(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * sizeof(double));
}

static int run_rows(const char *path) {
  constexpr size_t D = 3;
  std::ifstream in(path);
  if (!in) { std::printf("cannot read %s\n", path); return 2; }
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
  std::vector<DistanceGrid> grids;
  std::vector<GraspGoal> goals;
  const int nb = (int)num();
  for (int b = 0; b < nb; ++b) {
    const int model = (int)num();
    const bool gripper = num() != 0;
    const double radius = num();
    std::array<double, 9> T;
    for (double &v : T) v = num();
    if (model == MI_GOMP_MODEL_DH_CHAIN) balls.push_back(dhBall(chain, (int)T[0], {T[1], T[2], T[3]}, radius, gripper));
    else balls.push_back(model == MI_GOMP_MODEL_TABLE ? tableBall(T, radius, gripper) : yawBall(T[0], T[1], T[2], radius, gripper));
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
  const int ngl = (int)num();
  for (int k = 0; k < ngl; ++k) {
    const size_t ball = (size_t)num(), waypoint = (size_t)num();
    const int frame = (int)num();
    std::array<double, 3> ax;
    for (double &v : ax) v = num();
    GraspGoal g = dhGoal(chain, ball, frame, ax);
    g.waypoint = waypoint;
    CHECK((frame >= 1) == (bool)g.axis && g.builtin_frame == frame);
    goals.push_back(g);
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
  size_t before = W * (pairs.size() + tilts.size());
  for (const RobotBall &b : balls) before += W * ((b.is_gripper ? 3 : 0) + lines.size() + caps.size() + cubs.size() + grids.size());
  const size_t rows3d = before + 4 * goals.size();
  const ConstraintBuilder<D> tmpl = ConstraintBuilder<D>{W, balls, lines, caps, cubs, pairs, tilts, grids, goals}.withObstaclePattern().normalised();
  for (int t = 0; t < nt; ++t) {
    std::vector<GoalTarget> targets(goals.size());
    for (GoalTarget &g : targets) {
      for (double &v : g.point) v = num();
      for (double &v : g.tol) v = num();
      for (double &v : g.ref) v = num();
      g.max_angle = num();
    }
    QPVector x(2 * D * W);
    for (double &v : x) v = num();
    if (!in) { std::printf("short file\n"); return 2; }
    std::vector<GraspGoal> mine = goals;
    for (size_t k = 0; k < mine.size(); ++k) mine[k].target = targets[k];
    ConstraintBuilder<D> b{W, balls, lines, caps, cubs, pairs, tilts, grids, mine};
    const auto [l, A, u] = b.withObstacles(c3d, x).build();
    // the allocation grows by 4 |goals| rows: every row of the eight-argument builder keeps its index
    CHECK(l.size() == (W - 1) * D + D * (W + W - 1 + W - 2 + W * (3 + (lines.size() + caps.size() + cubs.size() + grids.size()) * balls.size())) +
                          W * (pairs.size() + tilts.size()) + 4 * goals.size());
    std::vector<std::array<double, D>> vals(rows3d);
    for (auto &v : vals) v.fill(0.0);
    std::vector<int> seen(rows3d, 0);
    for (long long c = 0; c < A.cols; ++c)
      for (long long k = A.outer[c]; k < A.outer[c + 1]; ++k) {
        const size_t r = (size_t)A.inner[k];
        if (r < row0) continue;
        CHECK(r < row0 + rows3d && c < (long long)(D * W));
        if (r >= row0 + before && r < row0 + rows3d) CHECK((size_t)c / D == goals[(r - row0 - before) / 4].waypoint);   // in the columns of the goal's waypoint
        if (r < row0 + rows3d) { vals[r - row0][(size_t)c % D] = A.values[k]; seen[r - row0]++; }
      }
    std::printf("N %d %zu\n", t, before);
    for (size_t r = before; r < rows3d; ++r) {
      CHECK(seen[r] == (int)D);
      std::printf("R %d %zu", t, r - before);
      for (size_t j = 0; j < D; ++j) std::printf(" %a", vals[r][j]);
      std::printf(" %a %a\n", l[row0 + r], u[row0 + r]);
    }
    for (size_t r = row0 + rows3d; r < l.size(); ++r) CHECK(l[r] == -INF && u[r] == INF);       // the empty rows come after the goal rows
    GOMPSolver<D, OracleQPSolver> g(W, 0.1, any, any, any, c3d, lines, balls);
    g.capsules = caps; g.cuboids = cubs; g.pairs = pairs; g.tilts = tilts; g.grids = grids;
    const bool ok_goals = goalsOKAlong<D>(mine, balls, x);
    std::printf("V %d %d %d\n", t, ok_goals ? 1 : 0, ok_goals && g.acceptable(x) ? 1 : 0);
    // no goals: the nine-argument builder with an empty list is the eight-argument one, bit for bit
    ConstraintBuilder<D> b8{W, balls, lines, caps, cubs, pairs, tilts, grids}, b9{W, balls, lines, caps, cubs, pairs, tilts, grids, {}};
    const auto [l8, A8, u8] = b8.withObstacles(c3d, x).build();
    const auto [l9, A9, u9] = b9.withObstacles(c3d, x).build();
    CHECK(sameBits(l8, l9) && sameBits(u8, u9) && A8.outer == A9.outer && A8.inner == A9.inner && sameBits(A8.values, A9.values));
    // ... and the rows before the goal rows are those of the eight-argument builder, bit for bit
    CHECK(l.size() == l8.size() + 4 * goals.size() && !std::memcmp(l.data(), l8.data(), (row0 + before) * sizeof(double)) &&
          !std::memcmp(u.data(), u8.data(), (row0 + before) * sizeof(double)));
    // what a planner does: the template copied, this trajectory's targets set, the rows written in place
    ConstraintBuilder<D> copy = tmpl;
    for (size_t k = 0; k < targets.size(); ++k) copy.setGoalTarget(k, targets[k]);
    const auto [lc, Ac, uc] = copy.withObstacles(c3d, x).build();
    CHECK(sameBits(lc, l) && sameBits(uc, u) && Ac.outer == A.outer && Ac.inner == A.inner && sameBits(Ac.values, A.values));
  }
  std::printf(fails ? "ROWS FAILED (%d)\n" : "ROWS OK\n", fails);
  return fails ? 1 : 0;
}

// ---- the 7-joint chain c7 of tests/dh_refs.py with its seven link balls; the tool axis is the z axis of the last frame.  The
// reach problem: from posture A the gripper ball goes to where it is at posture B, within a tolerance box, the tool axis within
// 10 degrees of straight down.  B is the seed: the fixed-end plan ends there, the goal plan wherever in that set it is cheapest.
constexpr size_t D7 = 7;
constexpr double kDeg = 3.14159265358979323846 / 180.0;
struct ReachProblems {
  mi_gomp_chain chain{};
  std::vector<RobotBall> balls;
  GraspGoal goal;
  Constraint<D7> pos, vel, acc;
  Constraint<3> c3d = constraints::any<3>();
  std::vector<Ctrl<D7>> starts, seeds;
  std::vector<GoalTarget> targets;
  explicit ReachProblems(int n) {
    const double H = 1.5707963267948966, pi = 3.14159265358979323846;
    chain.n_joints = 7;
    const double a[7] = {0, 0, 0.0825, -0.0825, 0, 0.088, 0}, d[7] = {0.333, 0, 0.316, 0, 0.384, 0, 0.107};
    const double alpha[7] = {-H, H, H, -H, H, H, 0.3}, theta0[7] = {0, 0, 0, 0.25, 0, 0, -0.7};
    for (int i = 0; i < 7; ++i) { chain.a[i] = a[i]; chain.d[i] = d[i]; chain.alpha[i] = alpha[i]; chain.theta0[i] = theta0[i]; }
    balls = {dhBall(chain, 2, {0, 0, 0}, 0.09), dhBall(chain, 3, {0, 0.05, -0.1}, 0.08), dhBall(chain, 4, {0.02, 0, 0.03}, 0.07),
             dhBall(chain, 5, {0, 0.04, -0.15}, 0.07), dhBall(chain, 6, {0.03, 0, 0}, 0.06), dhBall(chain, 7, {0, 0, -0.05}, 0.05),
             dhBall(chain, 7, {0.02, -0.01, 0.06}, 0.04, true)};
    goal = dhGoal(chain, 6, 7, {0, 0, 1});
    pos = constraints::inRange<D7>(constraints::of<D7>(-2 * pi), constraints::of<D7>(2 * pi));
    vel = constraints::inRange<D7>(constraints::of<D7>(-pi), constraints::of<D7>(pi));
    acc = constraints::inRange<D7>(constraints::of<D7>(-pi * 800 / 180), constraints::of<D7>(pi * 800 / 180));
    // the tool is within 0.2 degrees of vertical at both postures
    const double A[7] = {-0.273, 0.728, -0.584, -1.6, 0.101, 1.877, 1.025}, B[7] = {-1.283, 1.929, -2.018, -2.923, 1.301, 1.35, -0.775};
    for (int b = 0; b < n; ++b) {
      Ctrl<D7> s{}, e{};
      for (int j = 0; j < 7; ++j) { s[j] = A[j] + 0.004 * b * ((j % 3) - 1); e[j] = B[j] - 0.004 * b * ((j % 2) ? 1 : -1); }
      starts.push_back(s); seeds.push_back(e);
      const auto [x, y, z] = balls[6].fk(e.data());
      GoalTarget t;
      t.point = {x, y, z};
      t.tol = {0.03 + 0.005 * b, 0.03, 0.005};
      t.ref = {0, 0, -1};
      t.max_angle = (10 + 2 * b) * kDeg;
      targets.push_back(t);
    }
  }
};

// 0.5 x' P x of a plan as the QPs see it: the sum of the squared velocity differences (velocities in the second half, per step)
static double planCost(const QPVector &x, double time_step) {
  const size_t W = x.size() / 2 / D7;
  double c = 0.0;
  for (size_t j = 0; j < D7; ++j) {
    double prev = 0.0;
    for (size_t w = 0; w < W; ++w) {
      const double v = x[W * D7 + w * D7 + j] * time_step;
      c += (v - prev) * (v - prev);
      prev = v;
    }
    c += prev * prev;
  }
  return c;
}

static int run_checks() {
  ReachProblems pr(1);
  const GraspGoal &g = pr.goal;
  CHECK(g.ball == 6 && g.builtin_frame == 7 && (bool)g.axis && g.waypoint == 0);
  const GraspGoal flat = dhGoal(pr.chain, 2);
  CHECK(!flat.axis && flat.builtin_frame == 0 && !(flat == g) && g == pr.goal);
  // goalOK on a TABLE ball (p = q) and a 3-joint chain whose frame-2 axis (0, 1, 0) makes the angle |q_1| with +z
  mi_gomp_chain c3{};
  c3.n_joints = 3; c3.alpha[0] = 1.5707963267948966;
  const std::vector<RobotBall> table{tableBall({1, 0, 0, 0, 1, 0, 0, 0, 1}, 0.05, false)};
  GraspGoal t = dhGoal(c3, 0, 2, {0, 1, 0});
  t.target.point = {0.25, 0.0, -0.5};
  t.target.tol = {1.0 / 64, GOAL_FREE, 0.0};
  t.target.ref = {0, 0, 1};
  t.target.max_angle = 0.5;
  CHECK(t.cosLimit() == std::cos(0.5) && t.cosOK() == std::cos(0.5 + 1e-3));
  const double e = 1.0 / 64 + 1e-3;
  const double in1[3] = {0.25 + e - 1e-6, 0.4, -0.5 + 1e-3 - 1e-6}, out1[3] = {0.25 + e + 1e-6, 0.4, -0.5}, out2[3] = {0.25, 0.4, -0.5 - 1e-3 - 1e-6};
  const double far_y[3] = {0.25, -0.5 - 1e-3 + 1e-6, -0.5}, tipped[3] = {0.25, 0.5 + 1e-3 + 1e-6, -0.5}, nan_x[3] = {std::nan(""), 0.1, -0.5};
  CHECK(goalOK<3>(t, table, in1) && !goalOK<3>(t, table, out1) && !goalOK<3>(t, table, out2));
  CHECK(goalOK<3>(t, table, far_y) && !goalOK<3>(t, table, tipped) && !goalOK<3>(t, table, nan_x));
  GraspGoal wide = t;
  wide.target.max_angle = 3.1411;
  CHECK(wide.cosOK() == std::cos(3.14159265358979323846));               // the clamp at pi
  GraspGoal pos_only = dhGoal(c3, 0);
  pos_only.target = t.target;
  CHECK(goalOK<3>(pos_only, table, tipped));                               // no axis: the angle has no say
  QPVector x(2 * 3 * 4, 0.0);
  t.waypoint = 1;
  x[3] = 0.25; x[4] = 0.1; x[5] = -0.5;
  CHECK(goalsOKAlong<3>({t}, table, x) && goalsOKAlong<3>({}, table, x));
  x[5] = -0.6;
  CHECK(!goalsOKAlong<3>({t}, table, x));
  t.waypoint = 9;
  CHECK(!goalsOKAlong<3>({t}, table, x));                                  // a waypoint the trajectory does not have
  // goalWarmStart: the seed from the third-last waypoint on, zero velocities
  const QPVector ws = goalWarmStart<D7>(pr.starts[0], pr.seeds[0], 10);
  CHECK(ws.size() == 2 * 10 * D7);
  for (size_t j = 0; j < D7; ++j) {
    CHECK(ws[j] == pr.starts[0][j]);
    for (size_t w = 7; w < 10; ++w) CHECK(ws[w * D7 + j] == pr.seeds[0][j]);
    CHECK(ws[10 * D7 + j] == 0.0);
  }
  std::printf(fails ? "CHECKS FAILED (%d)\n" : "CHECKS OK\n", fails);
  return fails ? 1 : 0;
}

static void printPlan(const QPVector &x) {
  std::printf("P %zu", x.size());
  for (double v : x) std::printf(" %a", v);
  std::printf("\n");
}

static int run_plain(int W) {
  ReachProblems pr(1);
  GOMPSolver<D7, OracleQPSolver> o((size_t)W, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls, nullptr, false);
  auto [code, x] = o.run(pr.starts[0], pr.seeds[0]);
  std::printf("C %d %d %d %d\n", (int)code, o.segments_run, o.qp_solves, o.qp_updates);
  printPlan(x);
  return code == ExitCode::kOptimal ? 0 : 1;
}

// the angle between the goal's axis and its ref at waypoint w, radians
static double goalAngle(const GraspGoal &g, const QPVector &x, size_t w) {
  return std::acos(std::fmax(-1.0, std::fmin(1.0, goalCosine<D7>(g, x.data() + w * D7))));
}

static int run_plan(int W, const char *plain_file) {
  const int n = 2;
  ReachProblems pr(n);
  // ---- the sequential planner: fixed end and goal
  std::vector<QPVector> seq(n);
  std::vector<std::array<int, 3>> counters(n);
  for (int b = 0; b < n; ++b) {
    GOMPSolver<D7, OracleQPSolver> fixed((size_t)W, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls, nullptr, false);
    fixed.goal = pr.goal;                                           // run(start, end) does not look at it
    auto [cf, xf] = fixed.run(pr.starts[b], pr.seeds[b]);
    GOMPSolver<D7, OracleQPSolver> o((size_t)W, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls, nullptr, false);
    o.goal = pr.goal;
    auto [cg, xg] = o.run(pr.starts[b], pr.seeds[b], pr.targets[b]);
    CHECK(cf == ExitCode::kOptimal && cg == ExitCode::kOptimal);
    seq[b] = xg; counters[b] = {o.segments_run, o.qp_solves, o.qp_updates};
    const size_t Wf = xg.size() / 2 / D7, we = Wf - 3;
    GraspGoal g = pr.goal;
    g.waypoint = we; g.target = pr.targets[b];
    const auto [px, py, pz] = pr.balls[6].fk(xg.data() + we * D7);
    const double err[3] = {std::fabs(px - g.target.point[0]), std::fabs(py - g.target.point[1]), std::fabs(pz - g.target.point[2])};
    const double ang = goalAngle(g, xg, we);
    double turn = 0.0, move = 0.0;                                  // how far the chosen end point is from the seed
    for (size_t j = 0; j < D7; ++j) move = std::fmax(move, std::fabs(xg[we * D7 + j] - pr.seeds[b][j]));
    turn = xg[we * D7 + 6] - pr.seeds[b][6];
    std::printf("reach traj %d: fixed end: cost %.6f (%d solves) | goal: %s segments %d solves %d updates %d, %zu waypoints, cost %.6f, end point off the target by "
                "(%.2e, %.2e, %.2e) m, axis %.3f deg off (limit %.1f), %.3f rad from the seed (joint 7: %.3f)\n", b, planCost(xf, 0.1), fixed.qp_solves,
                ToString(cg).c_str(), o.segments_run, o.qp_solves, o.qp_updates, Wf, planCost(xg, 0.1), err[0], err[1], err[2], ang / kDeg, g.target.max_angle / kDeg, move, turn);
    for (int ax = 0; ax < 3; ++ax) CHECK(err[ax] <= g.target.tol[ax] + 1e-3);
    CHECK(ang <= g.target.max_angle + 1e-3);
    CHECK(o.acceptable(xg, pr.targets[b]) && goalOK<D7>(g, pr.balls, xg.data() + we * D7));
    for (size_t w = we; w < Wf; ++w) for (size_t j = 0; j < D7; ++j) CHECK(std::fabs(xg[w * D7 + j] - xg[we * D7 + j]) <= 1e-3);   // the last three coincide
    if (xg.size() == xf.size()) CHECK(planCost(xg, 0.1) <= planCost(xf, 0.1) * 1.05);   // (the same last horizon; different SQP paths: no theorem, a plausibility bound)
    CHECK(move > 1e-3);                                             // the planner chose its own end point
    if (b == 0 && plain_file) {                                     // a plan without goals: bit for bit the parent commit's
      std::ifstream in(plain_file);
      std::string tok;
      std::vector<double> want;
      while (in >> tok) want.push_back(std::strtod(tok.c_str(), nullptr));
      CHECK(!want.empty() && sameBits(want, xf));
      std::printf("fixed-end plan against the kept one: %zu numbers, %s\n", want.size(), sameBits(want, xf) ? "bit for bit" : "DIFFERENT");
    }
  }
  // ---- the lock-step and the continuous planner on oracle twins: the same decisions, the same bits
  BatchGOMPSolver<D7, OracleBatchSolver> batch((size_t)W, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls);
  batch.goal = pr.goal;
  auto rb = batch.run(pr.starts, pr.seeds, pr.targets);
  ContinuousGOMPSolver<D7, OracleContSolver> cont((size_t)W, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls);
  cont.goal = pr.goal;
  auto rc = cont.run(pr.starts, pr.seeds, pr.targets);
  for (int b = 0; b < n; ++b) {
    CHECK(rb[b].first == ExitCode::kOptimal && rc[b].first == ExitCode::kOptimal);
    CHECK(sameBits(rb[b].second, seq[b]) && sameBits(rc[b].second, seq[b]));
    // (a horizon that uses up its MAX_ITERATIONS rounds: the sequential and the continuous planner count the last round's update, which
    //  has no reader; the lock-step planner does not make it)
    CHECK(batch.segments_run[b] == counters[b][0] && batch.qp_solves[b] == counters[b][1] && batch.qp_updates[b] <= counters[b][2] &&
          batch.qp_updates[b] + batch.segments_run[b] >= counters[b][2]);
    CHECK(cont.segments_run[b] == counters[b][0] && cont.qp_solves[b] == counters[b][1] && cont.qp_updates[b] == counters[b][2]);
    std::printf("reach traj %d: lock-step %s, continuous %s: trajectories %s the sequential planner's\n", b, ToString(rb[b].first).c_str(), ToString(rc[b].first).c_str(),
                sameBits(rb[b].second, seq[b]) && sameBits(rc[b].second, seq[b]) ? "bit for bit" : "NOT");
  }
  // without targets both plan to the fixed end as before
  auto rb0 = batch.run(pr.starts, pr.seeds);
  CHECK(rb0[0].first == ExitCode::kOptimal);
  for (size_t j = 0; j < D7; ++j) CHECK(std::fabs(rb0[0].second[(rb0[0].second.size() / 2 / D7 - 3) * D7 + j] - pr.seeds[0][j]) <= 1e-3);
  // ---- the first QP of the goal run against the first QP of the fixed-end run, both linearised at goalWarmStart (the seed at
  // the third-last waypoint satisfies the goal, so the goal QP's feasible set holds the fixed-end QP's)
  {
    GOMPSolver<D7, OracleQPSolver> o((size_t)W, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls, nullptr, false);
    o.goal = pr.goal;
    const QPVector warm = goalWarmStart<D7>(pr.starts[0], pr.seeds[0], (size_t)W);
    GraspGoal g = pr.goal;
    g.waypoint = (size_t)W - 3; g.target = pr.targets[0];
    CHECK(goalOK<D7>(g, pr.balls, pr.seeds[0].data()));
    const QPMatrixSparse P = triDiagonalMatrix(2, -1, (int)(D7 * 2 * W), (int)(W * D7), (int)D7);
    const QPConstraints cf = o.firstConstraints(pr.starts[0], pr.seeds[0], (size_t)W, warm), cg = o.firstConstraints(pr.starts[0], pr.seeds[0], (size_t)W, warm, &pr.targets[0]);
    double obj_fixed[2], obj_goal = 0.0;
    const double eps[2] = {1e-5, 1e-7};                             // two oracle tolerances a factor 100 apart
    for (int k = 0; k < 2; ++k) {
      g_eps = eps[k];
      OracleQPSolver qf(cf, P);
      qf.setWarmStart(warm);
      CHECK(qf.solve().first == ExitCode::kOptimal);
      obj_fixed[k] = g_last_obj;
      if (k == 1) {
        OracleQPSolver qg(cg, P);
        qg.setWarmStart(warm);
        CHECK(qg.solve().first == ExitCode::kOptimal);
        obj_goal = g_last_obj;
      }
    }
    g_eps = 1e-3;
    const double margin = 10 * std::fabs(obj_fixed[0] - obj_fixed[1]);
    std::printf("first QP: fixed end %.12f (eps 1e-5), %.12f (eps 1e-7), goal %.12f (eps 1e-7); margin %.3e\n", obj_fixed[0], obj_fixed[1], obj_goal, margin);
    CHECK(obj_goal <= obj_fixed[1] + margin);
  }
  std::printf(fails ? "PLAN FAILED (%d)\n" : "PLAN OK\n", fails);
  return fails ? 1 : 0;
}

static int run_cont(int W) {
  const int n = 2;
  ReachProblems pr(n);
  ContinuousGOMPSolver<D7> host((size_t)W, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls), dev((size_t)W, 0.1, pr.pos, pr.vel, pr.acc, pr.c3d, {}, pr.balls);
  host.goal = dev.goal = pr.goal;
  dev.device_assembly = true;
  dev.dh_chain = pr.chain;
  auto rh = host.run(pr.starts, pr.seeds, pr.targets);
  auto rd = dev.run(pr.starts, pr.seeds, pr.targets);
  double worst = 0.0;
  int updates = 0, planned = 0;
  for (size_t b = 0; b < pr.starts.size(); ++b) {
    std::printf("reach traj %zu host: %s segments %d solves %d updates %d | device: %s %d %d %d\n", b, ToString(rh[b].first).c_str(), host.segments_run[b],
                host.qp_solves[b], host.qp_updates[b], ToString(rd[b].first).c_str(), dev.segments_run[b], dev.qp_solves[b], dev.qp_updates[b]);
    CHECK(rh[b].first == rd[b].first);
    CHECK(host.segments_run[b] == dev.segments_run[b] && host.qp_solves[b] == dev.qp_solves[b] && host.qp_updates[b] == dev.qp_updates[b]);
    CHECK(rh[b].second.size() == rd[b].second.size());
    for (size_t k = 0; k < rh[b].second.size() && k < rd[b].second.size(); ++k) worst = std::fmax(worst, std::fabs(rh[b].second[k] - rd[b].second[k]));
    updates += dev.qp_updates[b];
    if (rd[b].first == ExitCode::kOptimal) {
      ++planned;
      GraspGoal g = pr.goal;
      g.waypoint = rd[b].second.size() / 2 / D7 - 3; g.target = pr.targets[b];
      CHECK(goalOK<D7>(g, pr.balls, rd[b].second.data() + g.waypoint * D7));
    }
  }
  std::printf("reach: continuous planner with a grasp goal, device assembly vs host assembly: %zu trajectories (%d planned), %d re-linearisations on the device, "
              "max |dx| %.3e\n", pr.starts.size(), planned, updates, worst);
  CHECK(planned == n);
  CHECK(worst <= 1e-6);
  // the kept scenes are made again when the end condition changes: the same planner to the fixed end
  auto rn = dev.run(pr.starts, pr.seeds);
  for (size_t b = 0; b < pr.starts.size(); ++b) {
    CHECK(rn[b].first == ExitCode::kOptimal);
    const size_t we = rn[b].second.size() / 2 / D7 - 3;
    for (size_t j = 0; j < D7; ++j) CHECK(std::fabs(rn[b].second[we * D7 + j] - pr.seeds[b][j]) <= 1e-3);
  }
  std::printf(fails ? "CONT FAILED (%d)\n" : "CONT OK\n", fails);
  return fails ? 1 : 0;
}

int main(int argc, char **argv) {
  setenv("GPU_MAX_HW_QUEUES", "10", 0);                 // one hardware queue per horizon stage, as the planner examples set it
  if (argc > 2 && !std::strcmp(argv[1], "rows")) return run_rows(argv[2]);
  if (argc > 1 && !std::strcmp(argv[1], "checks")) return run_checks();
  if (argc > 1 && !std::strcmp(argv[1], "plan")) return run_plan(20, argc > 2 ? argv[2] : nullptr);
  if (argc > 1 && !std::strcmp(argv[1], "plain")) return run_plain(20);
  if (argc > 1 && !std::strcmp(argv[1], "cont")) return run_cont(20);
  std::printf("usage: gomp_goal rows FILE | checks | plan [FILE] | plain | cont\n");
  return 2;
}
