// gomp.hpp -- the callers of the solver path, SURVEY.md section 8(f) ranks 1-3, as a
// header-only C++17 layer on top of qp_solver.hpp (no Eigen):
//
//   constraints helpers      [REF] /root/reference/src/constraints/constraints.h:9-69
//   HorizontalLine           [REF] src/horizontal-line.h:6-104
//   RobotBall, linspace,
//   triDiagonalMatrix        [REF] src/utils.h:33-42,50-64,72-96
//   ConstraintBuilder<N>     [REF] src/constraints/constraint-builder.h:18-283
//   CapsuleObstacle          not in the reference: a segment swept by a sphere (posts, pipes, other robots' links; a == b: a sphere)
//   CuboidObstacle           not in the reference: an oriented box, optionally rounded (bin walls and floors, table tops, shelves)
//   BallPair                 not in the reference: two balls of the robot that must stay apart (self-collision)
//   TiltLimit                not in the reference: an axis of the robot that must stay within an angle of a world direction
//   DistanceGrid             not in the reference: a sensed world, a voxel grid of distances to the nearest surface
//   GraspGoal                not in the reference: where to arrive, in task space - a target box for a ball, a cone for an axis
//   GOMPSolver<N>            [REF] src/gomp-solver.h:13-201
//
// Same names, argument meaning, row layout and control flow as the reference (the known-answer
// tests of [REF] tests/test.cpp are replayed against it in tests/cpp/), written against plain
// containers.  GOMPSolver takes the QP backend as a template parameter: `QPSolver` (the MI355X
// path) by default; the parity test instantiates it with an oracle-backed twin.
// The reference prints every waypoint; here printing is off unless `verbose` is set.
#pragma once

#include <algorithm>
#include <array>
#include <memory>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <functional>
#include <map>
#include <optional>
#include <tuple>
#include <utility>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "qp_solver.hpp"

namespace miosqp_ref {

// ------------------------------------------------------------------ constraints.h
template <size_t N> using Vec = std::array<double, N>;
template <size_t N> using Bound = std::optional<Vec<N>>;
template <size_t N> using Constraint = std::pair<Bound<N>, Bound<N>>;
template <size_t N> using Ctrl = Vec<N>;
using Point = Vec<3>;
enum Axis : size_t { X, Y, Z };
constexpr std::array<Axis, 3> XYZ_AXES = {X, Y, Z};
constexpr double CENTIMETER = 0.01;
constexpr double ERROR = 1e-3;                         // [REF] src/utils.h:31

namespace constraints {
template <size_t N> Vec<N> of(double v) { Vec<N> r; r.fill(v); return r; }
template <size_t N> Constraint<N> inRange(Bound<N> low, Bound<N> upp) { return {low, upp}; }
template <size_t N> Constraint<N> equal(const Vec<N> &v) { return {v, v}; }
template <size_t N> Constraint<N> greaterEq(const Vec<N> &v) { return {v, std::nullopt}; }
template <size_t N> Constraint<N> lessEq(const Vec<N> &v) { return {std::nullopt, v}; }
template <size_t N> Constraint<N> any() { return {std::nullopt, std::nullopt}; }
template <size_t N> Constraint<N> eqZero() { return equal<N>(of<N>(0.0)); }
template <size_t N> Bound<N> scaled(const Bound<N> &b, double f) {
  if (!b) return std::nullopt;
  Vec<N> r = *b;
  for (double &x : r) x *= f;
  return r;
}
template <size_t N> Constraint<N> scaled(const Constraint<N> &c, double f) { return {scaled<N>(c.first, f), scaled<N>(c.second, f)}; }
}  // namespace constraints

// ------------------------------------------------------------------------ utils.h
using ForwardKinematicsFun = std::function<std::tuple<double, double, double>(double *)>;
using JacobianFun = std::function<void(double *, double *)>;          // out: 3 x N row-major, in: q
using InverseKinematics = std::function<int(double *, double, double, double)>;

struct RobotBall {
  RobotBall(ForwardKinematicsFun fk_, JacobianFun jac_, double radius_, bool is_gripper_ = false)
      : fk(std::move(fk_)), jacobian(std::move(jac_)), radius(radius_), is_gripper(is_gripper_) {}
  ForwardKinematicsFun fk;
  JacobianFun jacobian;
  double radius;
  bool is_gripper;
  // Not in the reference: when fk / jacobian are one of the kinematic models the library also has on the device
  // (mi_gomp_model in mi_osqp.h), naming it here lets the continuous planner re-linearise on the GPU (withBuiltin()).
  int builtin_model = 0;
  std::array<double, 12> builtin_param{};
  RobotBall &withBuiltin(int model, std::initializer_list<double> param = {}) {
    builtin_model = model;
    size_t k = 0;
    for (double v : param) if (k < builtin_param.size()) builtin_param[k++] = v;
    return *this;
  }
};

// n x n matrix with a on the diagonal and b on the +-diagonal_num diagonals for rows >= offset
// (both triangles are emitted, as the reference does)
inline QPMatrixSparse triDiagonalMatrix(double a, double b, int n, int offset = 0, int diagonal_num = 1) {
  std::map<std::pair<long long, long long>, double> cells;          // (col, row) -> value : CSC order
  for (int i = offset; i < n; ++i) {
    cells[{i, i}] = a;
    if (i + diagonal_num < n) cells[{i + diagonal_num, i}] = b;
    if (i - diagonal_num >= offset) cells[{i - diagonal_num, i}] = b;
  }
  QPMatrixSparse M;
  M.rows = M.cols = n;
  M.outer.assign(n + 1, 0);
  for (const auto &[cr, v] : cells) { M.outer[cr.first + 1]++; M.inner.push_back(cr.second); M.values.push_back(v); }
  for (int j = 0; j < n; ++j) M.outer[j + 1] += M.outer[j];
  return M;
}

template <size_t N>
QPVector linspace(const Vec<N> &a, const Vec<N> &b, size_t n_steps) {
  QPVector res(N * n_steps);
  for (size_t s = 0; s < n_steps; ++s)
    for (size_t j = 0; j < N; ++j) res[s * N + j] = (b[j] - a[j]) / double(n_steps - 1) * double(s) + a[j];
  return res;
}

// positions of a joint trajectory (first half of the vector) -> xyz, fk called once per waypoint in order
template <size_t N>
QPVector mapJointTrajectoryToXYZ(const QPVector &trajectory, const ForwardKinematicsFun &mapper) {
  const size_t waypoints = trajectory.size() / 2 / N;
  QPVector xyz(3 * waypoints);
  for (size_t w = 0; w < waypoints; ++w) {
    Vec<N> q;
    for (size_t j = 0; j < N; ++j) q[j] = trajectory[w * N + j];
    auto [x, y, z] = mapper(q.data());
    xyz[3 * w] = x; xyz[3 * w + 1] = y; xyz[3 * w + 2] = z;
  }
  return xyz;
}

// -------------------------------------------------------------- horizontal-line.h
class HorizontalLine {
 public:
  HorizontalLine(const std::array<double, 2> &direction, const Point &point, bool bypass_from_below = false)
      : A_(point), below_(bypass_from_below) {
    const double nrm = std::hypot(direction[0], direction[1]);
    D_ = {direction[0] / nrm, direction[1] / nrm, 0.0};
  }
  // perpendicular from P to the line: X - P with X = A + ((P-A).D) D
  Point getDistanceVec(const Point &P) const {
    double t = 0.0;
    for (int k = 0; k < 3; ++k) t += (P[k] - A_[k]) * D_[k];
    return {A_[0] + t * D_[0] - P[0], A_[1] + t * D_[1] - P[1], A_[2] + t * D_[2] - P[2]};
  }
  std::array<double, 2> getDistanceVecXY(const Point &P) const { Point d = getDistanceVec(P); return {d[0], d[1]}; }
  double getDistanceXY(const Point &P) const { auto d = getDistanceVecXY(P); return std::hypot(d[0], d[1]); }
  Point operator[](const Point &P) const { Point d = getDistanceVec(P); return {P[0] + d[0], P[1] + d[1], P[2] + d[2]}; }
  bool areOnOppositeSides(const Point &P, const Point &Q) const {
    auto a = getDistanceVecXY(P), b = getDistanceVecXY(Q);
    return a[0] * b[0] + a[1] * b[1] < 0;
  }
  // (for the device twin of this class, mi_gomp_line)
  std::array<double, 2> directionXY() const { return {D_[0], D_[1]}; }
  const Point &point() const { return A_; }
  bool isClose(const Point &P, const RobotBall &b) const { return getDistanceXY(P) < b.radius; }
  bool hasCollision(int waypoint, const QPVector &xyz, const RobotBall &b) const {
    const int waypoints = (int)xyz.size() / 3;
    auto at = [&](int w) { return Point{xyz[3 * w], xyz[3 * w + 1], xyz[3 * w + 2]}; };
    const Point p = at(waypoint);
    if (isClose(p, b)) return true;
    if (waypoint > 0 && areOnOppositeSides(at(waypoint - 1), p)) return true;
    if (waypoint + 1 < waypoints && areOnOppositeSides(p, at(waypoint + 1))) return true;
    return false;
  }
  bool isAbove(const Point &P, const RobotBall &b) const {
    return below_ ? (P[Z] - A_[Z]) <= -b.radius + ERROR : (P[Z] - A_[Z]) >= b.radius - ERROR;
  }
  bool bypassFromBelow() const { return below_; }

 private:
  Point D_{}, A_;
  bool below_;
};

// ------------------------------------------------------------- capsule obstacles (not in the reference)
// The segment a .. b swept by a sphere of radius `radius` (mi_gomp_capsule is its device twin, include/mi_osqp.h has the
// formulas).  A ball with centre P keeps the clearance |P - c| - (radius + ball.radius) >= 0 from it, c the point of the
// segment closest to P; its constraint row is the linearisation of that clearance in the joints and becomes active
// `margin` away from the surface.
class CapsuleObstacle {
 public:
  CapsuleObstacle(const Point &a_, const Point &b_, double radius_, double margin_ = 0.0) : a(a_), b(b_), radius(radius_), margin(margin_) {
    assert(radius >= 0.0 && margin >= 0.0);
  }
  static CapsuleObstacle sphere(const Point &centre, double radius, double margin = 0.0) { return {centre, centre, radius, margin}; }
  Point a, b;
  double radius, margin;
  // c = a + t (b - a), t = (P - a).(b - a) / |b - a|^2 clamped to [0, 1]; a for a == b
  Point closestPoint(const Point &P) const {
    const Point e{b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const double ee = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
    if (ee == 0.0) return a;
    const double t = std::fmin(1.0, std::fmax(0.0, ((P[0] - a[0]) * e[0] + (P[1] - a[1]) * e[1] + (P[2] - a[2]) * e[2]) / ee));
    return {a[0] + t * e[0], a[1] + t * e[1], a[2] + t * e[2]};
  }
  // P - c and its length
  Point offset(const Point &P) const { const Point c = closestPoint(P); return {P[0] - c[0], P[1] - c[1], P[2] - c[2]}; }
  double distance(const Point &P) const { const Point v = offset(P); return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
  double clearance(const Point &P, const RobotBall &ball) const { return distance(P) - (radius + ball.radius); }
  bool operator==(const CapsuleObstacle &o) const { return a == o.a && b == o.b && radius == o.radius && margin == o.margin; }
};
// the capsule part of isSolutionOK, for one ball at one waypoint (shared by the three drivers)
inline bool capsulesClear(const std::vector<CapsuleObstacle> &capsules, const Point &P, const RobotBall &ball) {
  bool res = true;
  for (const CapsuleObstacle &cap : capsules) if (!(cap.clearance(P, ball) >= -ERROR)) res = false;
  return res;
}

// ------------------------------------------------------------- cuboid obstacles (not in the reference)
// An oriented box with centre `centre`, orthonormal axes (the rows of `axes`, world coordinates) and half extents `half`
// along them, swept by a sphere of radius `radius` (mi_gomp_cuboid is its device twin, include/mi_osqp.h has the formulas in
// the order both sides compute them).  Outside, a ball is pushed along the unit vector from the closest point of the box -
// a face, an edge or a corner; inside or on the surface it leaves through the nearest face (the lowest axis on a tie).  Not
// the work-space box of the gripper balls: that is con_3d.
class CuboidObstacle {
 public:
  using Axes = std::array<double, 9>;
  CuboidObstacle(const Point &centre_, const Point &half_, double radius_ = 0.0, double margin_ = 0.0)
      : CuboidObstacle(centre_, Axes{1, 0, 0, 0, 1, 0, 0, 0, 1}, half_, radius_, margin_) {}
  static CuboidObstacle oriented(const Point &centre, const Axes &axes, const Point &half, double radius = 0.0, double margin = 0.0) {
    return CuboidObstacle(centre, axes, half, radius, margin);
  }
  Point centre;
  Axes axes;                                                // axes[3 k + i]: component i of axis k
  Point half;
  double radius, margin;
  // the signed distance of P from the sharp box and the unit normal at P, in world coordinates
  struct Probe { double sd; Point n; };
  Probe probe(const Point &P) const {
    const Point d{P[0] - centre[0], P[1] - centre[1], P[2] - centre[2]};
    Point y, c, v;
    for (size_t k = 0; k < 3; ++k) {
      y[k] = axes[3 * k] * d[0] + axes[3 * k + 1] * d[1] + axes[3 * k + 2] * d[2];
      c[k] = std::fmin(half[k], std::fmax(-half[k], y[k]));
      v[k] = y[k] - c[k];
    }
    const double out = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    Point nl{0.0, 0.0, 0.0};
    double sd;
    if (out > 1e-12) {
      sd = out;
      for (size_t k = 0; k < 3; ++k) nl[k] = v[k] / out;
    } else {
      size_t ks = 0;
      double slack = half[0] - std::fabs(c[0]);
      for (size_t k = 1; k < 3; ++k) if (half[k] - std::fabs(c[k]) < slack) { slack = half[k] - std::fabs(c[k]); ks = k; }
      sd = -slack;
      nl[ks] = c[ks] < 0.0 ? -1.0 : 1.0;
    }
    Probe r{sd, {}};
    for (size_t i = 0; i < 3; ++i) r.n[i] = nl[0] * axes[i] + nl[1] * axes[3 + i] + nl[2] * axes[6 + i];
    return r;
  }
  double signedDistance(const Point &P) const { return probe(P).sd; }
  Point normal(const Point &P) const { return probe(P).n; }
  double clearance(const Point &P, const RobotBall &ball) const { return probe(P).sd - (radius + ball.radius); }
  bool operator==(const CuboidObstacle &o) const { return centre == o.centre && axes == o.axes && half == o.half && radius == o.radius && margin == o.margin; }

 private:
  CuboidObstacle(const Point &centre_, const Axes &axes_, const Point &half_, double radius_, double margin_)
      : centre(centre_), axes(axes_), half(half_), radius(radius_), margin(margin_) {
    assert(half[0] >= 0.0 && half[1] >= 0.0 && half[2] >= 0.0 && radius >= 0.0 && margin >= 0.0);
    for (size_t i = 0; i < 3; ++i)
      for (size_t j = i; j < 3; ++j)
        assert(std::fabs(axes[3 * i] * axes[3 * j] + axes[3 * i + 1] * axes[3 * j + 1] + axes[3 * i + 2] * axes[3 * j + 2] - (i == j ? 1.0 : 0.0)) <= 1e-9);
  }
};
// the cuboid part of isSolutionOK, for one ball at one waypoint (shared by the three drivers)
inline bool cuboidsClear(const std::vector<CuboidObstacle> &cuboids, const Point &P, const RobotBall &ball) {
  bool res = true;
  for (const CuboidObstacle &cub : cuboids) if (!(cub.clearance(P, ball) >= -ERROR)) res = false;
  return res;
}

// ------------------------------------------------------------- distance grids: a sensed world (not in the reference)
// A box of n[0] x n[1] x n[2] nodes of spacing `cell`, axis-aligned in the world, node (0,0,0) at `origin`, each node holding
// the distance to the nearest surface (positive: free space, negative: inside material, possibly truncated), the x index
// fastest (mi_gomp_grid is its device twin, include/mi_osqp.h has the formulas in the order both sides compute them).  A ball
// keeps phi(P) - (offset + ball.radius) >= 0 with phi the trilinear interpolant; its row is the exact gradient of phi in the
// cell, NOT normalised, times the Jacobian.  Outside the box the grid says nothing.  Where the gradient vanishes (a flat,
// truncated region) the row is all zeros; active with phi below the reach its QP is primal infeasible - start outside the
// material, and truncate no lower than the margin.  The values are shared: copying a grid copies a pointer.
class DistanceGrid {
 public:
  using Values = std::shared_ptr<const std::vector<double>>;
  DistanceGrid(const Point &origin_, double cell_, const std::array<int, 3> &n_, Values values_, double offset_ = 0.0, double margin_ = 0.0)
      : origin(origin_), cell(cell_), n(n_), offset(offset_), margin(margin_), values(std::move(values_)) {
    assert(cell > 0.0 && n[0] >= 2 && n[1] >= 2 && n[2] >= 2 && offset >= 0.0 && margin >= 0.0);
    assert(values && values->size() == (size_t)n[0] * (size_t)n[1] * (size_t)n[2]);
  }
  DistanceGrid(const Point &origin_, double cell_, const std::array<int, 3> &n_, std::vector<double> values_, double offset_ = 0.0, double margin_ = 0.0)
      : DistanceGrid(origin_, cell_, n_, std::make_shared<const std::vector<double>>(std::move(values_)), offset_, margin_) {}
  // every node gets the minimum of the primitives' exact signed distances (their radii included)
  static DistanceGrid fromObstacles(const Point &origin, double cell, const std::array<int, 3> &n, const std::vector<CapsuleObstacle> &capsules,
                                    const std::vector<CuboidObstacle> &cuboids, double offset = 0.0, double margin = 0.0) {
    std::vector<double> v((size_t)n[0] * (size_t)n[1] * (size_t)n[2]);
    for (int iz = 0; iz < n[2]; ++iz)
      for (int iy = 0; iy < n[1]; ++iy)
        for (int ix = 0; ix < n[0]; ++ix) {
          const Point P{origin[0] + ix * cell, origin[1] + iy * cell, origin[2] + iz * cell};
          double d = INF;
          for (const CapsuleObstacle &c : capsules) d = std::fmin(d, c.distance(P) - c.radius);
          for (const CuboidObstacle &c : cuboids) d = std::fmin(d, c.signedDistance(P) - c.radius);
          v[((size_t)iz * (size_t)n[1] + (size_t)iy) * (size_t)n[0] + (size_t)ix] = d;
        }
    return DistanceGrid(origin, cell, n, std::move(v), offset, margin);
  }
  Point origin;
  double cell;
  std::array<int, 3> n;
  double offset, margin;
  Values values;
  double invCell() const { return 1.0 / cell; }
  struct Sample { bool inside; double phi; Point grad; };
  Sample sample(const Point &P) const {
    const double inv = invCell();
    double f[3];
    bool inside = true;
    for (size_t k = 0; k < 3; ++k) {
      f[k] = (P[k] - origin[k]) * inv;
      if (!(f[k] >= 0.0 && f[k] <= (double)(n[k] - 1))) inside = false;      // (a NaN is outside)
    }
    if (!inside) return {false, 0.0, {0.0, 0.0, 0.0}};
    size_t i[3];
    double t[3];
    for (size_t k = 0; k < 3; ++k) {
      const int ik = std::max(0, std::min(n[k] - 2, (int)std::floor(f[k])));
      i[k] = (size_t)ik;
      t[k] = f[k] - (double)ik;
    }
    const size_t sy = (size_t)n[0], sz = (size_t)n[0] * (size_t)n[1];
    const double *v = values->data() + (i[2] * sz + i[1] * sy + i[0]);
    const double v000 = v[0], v100 = v[1], v010 = v[sy], v110 = v[sy + 1], v001 = v[sz], v101 = v[sz + 1], v011 = v[sz + sy], v111 = v[sz + sy + 1];
    const double e00 = v100 - v000, e10 = v110 - v010, e01 = v101 - v001, e11 = v111 - v011;
    const double x00 = v000 + t[0] * e00, x10 = v010 + t[0] * e10, x01 = v001 + t[0] * e01, x11 = v011 + t[0] * e11;
    const double ey0 = x10 - x00, ey1 = x11 - x01;
    const double y0 = x00 + t[1] * ey0, y1 = x01 + t[1] * ey1;
    const double ex0 = e00 + t[1] * (e10 - e00), ex1 = e01 + t[1] * (e11 - e01);
    return {true, y0 + t[2] * (y1 - y0), {(ex0 + t[2] * (ex1 - ex0)) * inv, (ey0 + t[2] * (ey1 - ey0)) * inv, (y1 - y0) * inv}};
  }
  // phi - (offset + ball.radius); +INF outside the box: the grid says nothing there
  double clearance(const Point &P, const RobotBall &ball) const {
    const Sample s = sample(P);
    return s.inside ? s.phi - (offset + ball.radius) : INF;
  }
  bool operator==(const DistanceGrid &o) const {
    return origin == o.origin && cell == o.cell && n == o.n && offset == o.offset && margin == o.margin && (values == o.values || *values == *o.values);
  }
};
// the grid part of isSolutionOK, for one ball at one waypoint (shared by the three drivers)
inline bool gridsClear(const std::vector<DistanceGrid> &grids, const Point &P, const RobotBall &ball) {
  bool res = true;
  for (const DistanceGrid &gr : grids) if (!(gr.clearance(P, ball) >= -ERROR)) res = false;
  return res;
}

// ------------------------------------------------------------- ball pairs: self-collision (not in the reference)
// Balls a and b of the planner's ball list must keep |p_a - p_b| - (r_a + r_b) >= 0 (mi_gomp_pair is its device twin,
// include/mi_osqp.h has the formulas).  The row of a (pair, waypoint) is the linearisation of that clearance in the joints,
// n' (J_a - J_b) with n the unit vector from b to a, and becomes active `margin` away from contact.
struct BallPair {
  size_t a, b;
  double margin = 0.0;
  bool operator==(const BallPair &o) const { return a == o.a && b == o.b && margin == o.margin; }
};
// |p_a - p_b| - (r_a + r_b) of a pair; xyz_w[3 i .. 3 i + 2]: the centre of ball i at one waypoint
inline double pairClearance(const BallPair &pr, const std::vector<double> &xyz_w, const std::vector<RobotBall> &balls) {
  const double v0 = xyz_w[3 * pr.a] - xyz_w[3 * pr.b], v1 = xyz_w[3 * pr.a + 1] - xyz_w[3 * pr.b + 1], v2 = xyz_w[3 * pr.a + 2] - xyz_w[3 * pr.b + 2];
  return std::sqrt(v0 * v0 + v1 * v1 + v2 * v2) - (balls[pr.a].radius + balls[pr.b].radius);
}
// the pair part of isSolutionOK at one waypoint (shared by the three drivers)
inline bool pairsClear(const std::vector<BallPair> &pairs, const std::vector<double> &xyz_w, const std::vector<RobotBall> &balls) {
  bool res = true;
  for (const BallPair &pr : pairs) if (!(pairClearance(pr, xyz_w, balls) >= -ERROR)) res = false;
  return res;
}
// pairsClear at every waypoint of a joint trajectory (positions in the first half of the vector)
template <size_t N>
bool pairsClearAlong(const std::vector<BallPair> &pairs, const std::vector<RobotBall> &balls, const QPVector &trajectory) {
  if (pairs.empty()) return true;
  bool res = true;
  std::vector<double> xyz_w(3 * balls.size());
  for (size_t w = 0; w < trajectory.size() / 2 / N; ++w) {
    Vec<N> q;
    for (size_t j = 0; j < N; ++j) q[j] = trajectory[w * N + j];
    for (size_t i = 0; i < balls.size(); ++i) std::tie(xyz_w[3 * i], xyz_w[3 * i + 1], xyz_w[3 * i + 2]) = balls[i].fk(q.data());
    if (!pairsClear(pairs, xyz_w, balls)) res = false;
  }
  return res;
}

// ------------------------------------------------------------- tilt limits: "keep the tool upright" (not in the reference)
// A unit vector fixed in a link of the robot must stay within max_angle radians of the unit world vector `ref`:
// c(q) = u(q) . ref >= cos(max_angle) (mi_gomp_tilt is its device twin, include/mi_osqp.h has the formulas).  The row of a
// (tilt, waypoint) is the gradient of c in the joints, g_j = (du/dq_j) . ref, and becomes active `margin` radians inside the
// cone.  When u is parallel or antiparallel to ref the gradient vanishes and the row is all zeros: parallel it is inactive,
// antiparallel it is active with l = cos(max_angle) + 1 > 0 and the QP is primal infeasible - start inside the cone.
using AxisFun = std::function<void(const double *, double *, double *)>;   // in: q; out: u[3] and (non-null) dU, 3 x N row-major, column j = du/dq_j
struct TiltLimit {
  AxisFun axis;                               // the axis in the world and its derivative; any arm, not only DH chains
  std::array<double, 3> ref{0.0, 0.0, 1.0};
  double max_angle = 0.0, margin = 0.0;       // radians
  // as RobotBall::builtin_model: for an axis fixed in a frame of the planner's DH chain (dhTilt of dh_kinematics.hpp makes
  // one) the frame and the axis in it, which the device path reads; frame 0: none
  int builtin_frame = 0;
  std::array<double, 3> builtin_axis{};
  // the three thresholds, as mi_gomp_scene_create_tilts takes them
  double cosLimit() const { return std::cos(max_angle); }
  double cosActive() const { return std::cos(std::max(0.0, max_angle - margin)); }
  double cosOK() const { return std::cos(std::min(M_PI, max_angle + ERROR)); }
  bool operator==(const TiltLimit &o) const {   // (the callback cannot be compared: the kept device scenes hold the rest)
    return ref == o.ref && max_angle == o.max_angle && margin == o.margin && builtin_frame == o.builtin_frame && builtin_axis == o.builtin_axis;
  }
};
// c = u . ref at q, and (g non-null) its gradient g[N]
template <size_t N>
double tiltCosine(const TiltLimit &t, const double *q, double *g = nullptr) {
  double u[3];
  std::array<double, 3 * N> dU{};
  t.axis(q, u, g ? dU.data() : nullptr);
  if (g) for (size_t j = 0; j < N; ++j) g[j] = dU[0 * N + j] * t.ref[0] + dU[1 * N + j] * t.ref[1] + dU[2 * N + j] * t.ref[2];
  return u[0] * t.ref[0] + u[1] * t.ref[1] + u[2] * t.ref[2];
}
// the tilt part of isSolutionOK at one waypoint (shared by the three drivers): within max_angle + 1 mrad
template <size_t N>
bool tiltsOK(const std::vector<TiltLimit> &tilts, const double *q) {
  bool res = true;
  for (const TiltLimit &t : tilts) if (!(tiltCosine<N>(t, q) >= t.cosOK())) res = false;
  return res;
}
// tiltsOK at every waypoint of a joint trajectory (positions in the first half of the vector)
template <size_t N>
bool tiltsOKAlong(const std::vector<TiltLimit> &tilts, const QPVector &trajectory) {
  if (tilts.empty()) return true;
  bool res = true;
  for (size_t w = 0; w < trajectory.size() / 2 / N; ++w)
    if (!tiltsOK<N>(tilts, trajectory.data() + w * N)) res = false;
  return res;
}

// ------------------------------------------------------------- grasp goals: task-space targets (not in the reference)
// Where a trajectory has to arrive, said in task space instead of as one joint vector: at waypoint `waypoint` the centre of
// ball `ball` lies in the box point +- tol, and (with `axis` set) a unit vector fixed in a link stays within max_angle of the
// world vector `ref` - a suction cup on a cylinder is free to turn about its approach axis, a bin pick has a tolerance box,
// and the planner chooses the joints inside that set (mi_gomp_goal / mi_gomp_goal_value are the device twins,
// include/mi_osqp.h has the formulas).  ball, waypoint and axis are the structure every trajectory of a planner shares;
// GoalTarget is what one trajectory asks.  A goal owns four rows in the columns of its waypoint: x, y, z of the centre (the
// ball's radius does not enter) and the cosine's gradient; all are always active, there is no margin.  Where the axis is
// exactly opposite to ref the fourth row is all zeros with l > 0 and the QP is primal infeasible, as for tilt limits: seed on
// the right side - the joints the first linearisation is taken at must not point the axis away from ref.
constexpr double GOAL_FREE = 1e30;               // a half width from here on: that axis is free
struct GoalTarget {
  Point point{0.0, 0.0, 0.0};
  std::array<double, 3> tol{GOAL_FREE, GOAL_FREE, GOAL_FREE};      // half widths >= 0; 0: an equality
  std::array<double, 3> ref{0.0, 0.0, 1.0};                        // unit world vector (read only when the goal has an axis)
  double max_angle = M_PI / 2;                                     // in (0, pi), radians
  bool operator==(const GoalTarget &o) const { return point == o.point && tol == o.tol && ref == o.ref && max_angle == o.max_angle; }
};
struct GraspGoal {
  size_t ball = 0, waypoint = 0;
  AxisFun axis;                               // the axis in the world and its derivative; empty: a position-only goal
  // as TiltLimit::builtin_frame: for an axis fixed in a frame of the planner's DH chain (dhGoal of dh_kinematics.hpp makes
  // one) the frame and the axis in it, which the device path reads; frame 0 with `axis` empty: position only
  int builtin_frame = 0;
  std::array<double, 3> builtin_axis{};
  GoalTarget target;
  double cosLimit() const { return std::cos(target.max_angle); }
  double cosOK() const { return std::cos(std::min(M_PI, target.max_angle + ERROR)); }
  bool operator==(const GraspGoal &o) const {   // (the callback cannot be compared: the kept device scenes hold the rest)
    return ball == o.ball && waypoint == o.waypoint && bool(axis) == bool(o.axis) && builtin_frame == o.builtin_frame && builtin_axis == o.builtin_axis;
  }
};
// c = u . ref of a goal with an axis at q, and (g non-null) its gradient g[N]: tiltCosine's formulas
template <size_t N>
double goalCosine(const GraspGoal &gl, const double *q, double *g = nullptr) {
  double u[3];
  std::array<double, 3 * N> dU{};
  gl.axis(q, u, g ? dU.data() : nullptr);
  const std::array<double, 3> &ref = gl.target.ref;
  if (g) for (size_t j = 0; j < N; ++j) g[j] = dU[0 * N + j] * ref[0] + dU[1 * N + j] * ref[1] + dU[2 * N + j] * ref[2];
  return u[0] * ref[0] + u[1] * ref[1] + u[2] * ref[2];
}
// the goal part of isSolutionOK (shared by the three drivers): q the joints of the goal's waypoint; the centre within
// tol + 1 mm on every axis that is not free, the axis within max_angle + 1 mrad (a NaN fails both)
template <size_t N>
bool goalOK(const GraspGoal &gl, const std::vector<RobotBall> &balls, const double *q) {
  bool res = true;
  Vec<N> qq;
  for (size_t j = 0; j < N; ++j) qq[j] = q[j];
  const auto [x, y, z] = balls[gl.ball].fk(qq.data());
  const Point p{x, y, z};
  for (size_t ax = 0; ax < 3; ++ax)
    if (!(gl.target.tol[ax] >= GOAL_FREE) && !(std::fabs(p[ax] - gl.target.point[ax]) <= gl.target.tol[ax] + ERROR)) res = false;
  if (gl.axis && !(goalCosine<N>(gl, qq.data()) >= gl.cosOK())) res = false;
  return res;
}
// The joint-space warm start of a run towards a grasp goal: a straight line from `start` that reaches `seed` at the third-last
// waypoint and stays there (the end conditions make the last three waypoints coincide), zero velocities.  The first QP is
// then linearised at the seed itself: a seed that satisfies the goal is a feasible end point of it.
template <size_t N>
QPVector goalWarmStart(const Vec<N> &start, const Vec<N> &seed, size_t waypoints) {
  assert(waypoints >= 4);
  QPVector w = linspace<N>(start, seed, waypoints - 2);
  w.resize((waypoints - 3) * N);                            // (the line's last point is the seed to round-off: the seed itself)
  for (size_t k = 0; k < 3; ++k) w.insert(w.end(), seed.begin(), seed.end());
  w.resize(2 * waypoints * N, 0.0);
  return w;
}
// goalOK of every goal on a joint trajectory (positions in the first half of the vector)
template <size_t N>
bool goalsOKAlong(const std::vector<GraspGoal> &goals, const std::vector<RobotBall> &balls, const QPVector &trajectory) {
  bool res = true;
  for (const GraspGoal &gl : goals) {
    if (gl.waypoint >= trajectory.size() / 2 / N) { res = false; continue; }
    if (!goalOK<N>(gl, balls, trajectory.data() + gl.waypoint * N)) res = false;
  }
  return res;
}

// ------------------------------------------------------------- constraint-builder.h
// Rows: (W-1)*D velocity<->position links, then per variable boxes (positions W*D, velocities
// (W-1)*D, accelerations (W-2)*D), then D*W*(3 + (|obstacles| + |capsules| + |cuboids| + |grids|)*|balls|) rows for the linearised
// end-effector / obstacle constraints (allocated even when unused: bounds +-INF), then W*(|pairs| + |tilts|) + 4 |goals| rows more.  The
// populated 3-D rows come first: the blocks of the (ball, waypoint) pairs (work-space rows of a gripper ball, lines, capsules,
// cuboids, grids), then the ball pairs' rows, pair-major, then the tilt limits' rows, tilt-major, then four rows a grasp goal.
template <size_t N_DIM>
class ConstraintBuilder {
  using OptPair = std::pair<std::optional<double>, std::optional<double>>;

 public:
  ConstraintBuilder(size_t waypoints, std::vector<RobotBall> m, std::vector<HorizontalLine> obstacles, std::vector<CapsuleObstacle> capsules = {},
                    std::vector<CuboidObstacle> cuboids = {}, std::vector<BallPair> pairs = {}, std::vector<TiltLimit> tilts = {},
                    std::vector<DistanceGrid> grids = {}, std::vector<GraspGoal> goals = {})
      : W_(waypoints), balls_(std::move(m)), lines_(std::move(obstacles)), capsules_(std::move(capsules)), cuboids_(std::move(cuboids)),
        pairs_(std::move(pairs)), tilts_(std::move(tilts)), grids_(std::move(grids)), goals_(std::move(goals)) {
    for ([[maybe_unused]] const GraspGoal &gl : goals_) assert(gl.ball < balls_.size() && gl.waypoint < W_);
    for ([[maybe_unused]] const TiltLimit &t : tilts_) assert(t.axis && t.max_angle > 0.0 && t.max_angle < M_PI && t.margin >= 0.0);
    for ([[maybe_unused]] const BallPair &pr : pairs_) assert(pr.a < balls_.size() && pr.b < balls_.size() && pr.a != pr.b && pr.margin >= 0.0);
    cells_.reserve(N_DIM * W_ * (10 + 3 * balls_.size() * (1 + lines_.size() + capsules_.size() + cuboids_.size() + grids_.size()) + pairs_.size() + tilts_.size()) + 4 * N_DIM * goals_.size());
    lo_.reserve(N_DIM * W_ * (7 + (lines_.size() + capsules_.size() + cuboids_.size() + grids_.size()) * balls_.size()) + W_ * (pairs_.size() + tilts_.size()) + 4 * goals_.size()); up_.reserve(lo_.capacity());
    for (size_t t = 0; t + 1 < W_; ++t)                      // v_t - q_{t+1} + q_t = 0
      for (size_t j = 0; j < N_DIM; ++j) {
        lo_.push_back(-INF); up_.push_back(INF);
        put(lo_.size() - 1, {{nthVelocity(t) + j, 1.0}, {nthPos(t + 1) + j, -1.0}, {nthPos(t) + j, 1.0}}, {0.0, 0.0});
      }
    user_off_ = lo_.size();
    const size_t extra = N_DIM * (W_ + W_ - 1 + W_ - 2 + W_ * (3 + (lines_.size() + capsules_.size() + cuboids_.size() + grids_.size()) * balls_.size())) + W_ * (pairs_.size() + tilts_.size()) + 4 * goals_.size();
    lo_.resize(user_off_ + extra, -INF);
    up_.resize(user_off_ + extra, INF);
  }

  ConstraintBuilder &position(size_t i, const Constraint<N_DIM> &c) { return positions(i, i, c); }
  ConstraintBuilder &positions(size_t first, size_t last, const Constraint<N_DIM> &c) { return boxes(nthPos(first), nthPos(last), c); }
  ConstraintBuilder &velocity(size_t i, const Constraint<N_DIM> &c) { return velocities(i, i, c); }
  ConstraintBuilder &velocities(size_t first, size_t last, const Constraint<N_DIM> &c) {
    assert(first <= last && last < W_ - 1);
    return boxes(nthVelocity(first), nthVelocity(last), c);
  }
  ConstraintBuilder &accelerations(size_t first, size_t last, const Constraint<N_DIM> &c) {
    for (size_t i = first; i <= last; ++i) acceleration(i, c);
    return *this;
  }
  ConstraintBuilder &acceleration(size_t i, const Constraint<N_DIM> &c) {
    assert(i + 2 < W_);
    for (size_t j = 0; j < N_DIM; ++j)                          // l <= v_{t+1} - v_t <= u
      put(user_off_ + nthAcceleration(i) + j, {{nthVelocity(i + 1) + j, 1.0}, {nthVelocity(i) + j, -1.0}}, dim(j, c));
    return *this;
  }

  // (re-)linearise the 3-D rows around `trajectory`; the pattern never changes (dummy rows)
  ConstraintBuilder &withObstacles(const Constraint<3> &con_3d, const QPVector &trajectory) {
    size_t row = user_off_ + N_DIM * (W_ + W_ - 1 + W_ - 2);
    for (const RobotBall &ball : balls_) {
      const QPVector xyz = mapJointTrajectoryToXYZ<N_DIM>(trajectory, ball.fk);
      for (size_t w = 0; w < W_; ++w) {
        Vec<N_DIM> q;
        for (size_t j = 0; j < N_DIM; ++j) q[j] = trajectory[w * N_DIM + j];
        const Point p{xyz[3 * w], xyz[3 * w + 1], xyz[3 * w + 2]};
        std::array<double, 3 * N_DIM> J{};
        ball.jacobian(J.data(), q.data());
        auto Jq = [&](size_t axis) { double s = 0.0; for (size_t j = 0; j < N_DIM; ++j) s += J[axis * N_DIM + j] * q[j]; return s; };
        if (ball.is_gripper) {
          for (Axis axis : XYZ_AXES) {
            double lo = -INF, up = INF;
            if (con_3d.first) lo = (*con_3d.first)[axis] - p[axis] + Jq(axis);
            if (con_3d.second) up = (*con_3d.second)[axis] - p[axis] + Jq(axis);
            axisRow(row++, ball, axis, J, w, lo, up);
          }
        }
        for (const HorizontalLine &line : lines_) {
          if (line.hasCollision((int)w, xyz, ball)) {
            const double bound = line[p][Z] - p[Z] + Jq(Z);
            if (line.bypassFromBelow()) axisRow(row++, ball, Z, J, w, -INF, bound);
            else axisRow(row++, ball, Z, J, w, bound, INF);
          } else {
            axisRow(row++, ball, Z, J, w, -INF, INF);          // dummy: keeps the pattern constant
          }
        }
        for (const CapsuleObstacle &cap : capsules_) capsuleRow(row++, ball, cap, p, J, q, w);
        for (const CuboidObstacle &cub : cuboids_) cuboidRow(row++, ball, cub, p, J, q, w);
        for (const DistanceGrid &gr : grids_) gridRow(row++, ball, gr, p, J, q, w);
      }
    }
    for (const BallPair &pr : pairs_)                            // behind the block of the last ball, pair-major
      for (size_t w = 0; w < W_; ++w) pairRow(row++, pr, trajectory, w);
    for (const TiltLimit &t : tilts_)                            // behind the pair rows, tilt-major
      for (size_t w = 0; w < W_; ++w) tiltRow(row++, t, trajectory, w);
    for (const GraspGoal &gl : goals_) { goalRow(row, gl, trajectory); row += 4; }   // behind the tilt rows, goal-major, four a goal
    return *this;
  }

  // the cells and rows withObstacles() writes, with zero values and open bounds, without calling the balls' callbacks: the
  // sparsity pattern of every later build() (pattern analysis ahead of time, GOMPSolver::run)
  ConstraintBuilder &withObstaclePattern() {
    size_t row = user_off_ + N_DIM * (W_ + W_ - 1 + W_ - 2);
    const std::array<double, 3 * N_DIM> J{};
    for (const RobotBall &ball : balls_)
      for (size_t w = 0; w < W_; ++w) {
        if (ball.is_gripper) for (Axis axis : XYZ_AXES) axisRow(row++, ball, axis, J, w, -INF, INF);
        for (size_t k = 0; k < lines_.size() + capsules_.size() + cuboids_.size() + grids_.size(); ++k) axisRow(row++, ball, Z, J, w, -INF, INF);
      }
    for (size_t k = 0; k < pairs_.size() + tilts_.size(); ++k)
      for (size_t w = 0; w < W_; ++w, ++row) {
        for (size_t j = 0; j < N_DIM; ++j) set(nthPos(w) + j, row, 0.0);
        lo_[row] = -INF; up_[row] = INF;
      }
    for (const GraspGoal &gl : goals_)
      for (size_t r = 0; r < 4; ++r, ++row) {
        for (size_t j = 0; j < N_DIM; ++j) set(nthPos(gl.waypoint) + j, row, 0.0);
        lo_[row] = -INF; up_[row] = INF;
      }
    return *this;
  }

  // what this trajectory asks of goal k (a builder copied from a template: the structure stays, the values are its own);
  // the next withObstacles() writes the rows
  ConstraintBuilder &setGoalTarget(size_t k, const GoalTarget &target) {
    assert(k < goals_.size());
    assert(target.tol[0] >= 0.0 && target.tol[1] >= 0.0 && target.tol[2] >= 0.0);
    assert(!goals_[k].axis || (target.max_angle > 0.0 && target.max_angle < M_PI));
    goals_[k].target = target;
    return *this;
  }

  // sort and de-duplicate the write log now (build() does it on demand): a builder that serves as a template for copies
  ConstraintBuilder &normalised() { normalise(); return *this; }

  QPConstraints build() const {
    QPMatrixSparse A;
    A.rows = (long long)lo_.size(); A.cols = (long long)(2 * N_DIM * W_);
    A.outer.assign(A.cols + 1, 0);
    normalise();
    A.inner.reserve(cells_.size()); A.values.reserve(cells_.size());
    for (const Cell &c : cells_) { A.outer[c.col + 1]++; A.inner.push_back((long long)c.row); A.values.push_back(c.v); }
    for (long long j = 0; j < A.cols; ++j) A.outer[j + 1] += A.outer[j];
    return {lo_, A, up_};
  }

  size_t nthVelocity(size_t i) const { assert(i < W_ - 1); return W_ * N_DIM + i * N_DIM; }
  size_t nthPos(size_t i) const { assert(i < W_); return i * N_DIM; }
  size_t nthAcceleration(size_t i) const { assert(i < W_ - 2); return W_ * N_DIM + (W_ - 1) * N_DIM + i * N_DIM; }

 private:
  size_t W_, user_off_ = 0;
  std::vector<RobotBall> balls_;
  std::vector<HorizontalLine> lines_;
  std::vector<CapsuleObstacle> capsules_;
  std::vector<CuboidObstacle> cuboids_;
  std::vector<BallPair> pairs_;
  std::vector<TiltLimit> tilts_;
  std::vector<DistanceGrid> grids_;
  std::vector<GraspGoal> goals_;
  // (col, row) -> value, last write wins ([REF] constraint-builder.h:129).  A write log that is sorted into CSC
  // order and de-duplicated on demand: the builder runs once per trajectory, segment and re-linearisation,
  // and a std::map made it the bottleneck of the batched driver.
  struct Cell { size_t col, row; double v; };
  mutable std::vector<Cell> cells_;
  mutable bool sorted_ = true;
  void set(size_t col, size_t row, double v) {
    if (sorted_ && !cells_.empty()) {          // a write to an existing cell of a normalised builder (a copied template): in place
      auto it = std::lower_bound(cells_.begin(), cells_.end(), Cell{col, row, 0.0},
                                 [](const Cell &a, const Cell &b) { return a.col != b.col ? a.col < b.col : a.row < b.row; });
      if (it != cells_.end() && it->col == col && it->row == row) { it->v = v; return; }
    }
    cells_.push_back({col, row, v}); sorted_ = false;
  }
  void normalise() const {
    if (sorted_) return;
    // stable order by (col, row): a counting pass over the columns (2 N_DIM W of them, a handful of cells each), then an
    // insertion sort inside every column - the write order among equal (col, row) survives both
    // (scratch kept per thread: the builder runs thousands of times per second in the batched driver, and fresh
    //  buffers of this size come straight from mmap every time)
    const size_t ncol = 2 * N_DIM * W_;
    static thread_local std::vector<size_t> start, at;
    static thread_local std::vector<Cell> by_col;
    start.assign(ncol + 1, 0);
    for (const Cell &c : cells_) { assert(c.col < ncol); start[c.col + 1]++; }
    for (size_t j = 0; j < ncol; ++j) start[j + 1] += start[j];
    if (by_col.size() < cells_.size()) by_col.resize(cells_.size());
    at.assign(start.begin(), start.end() - 1);
    for (const Cell &c : cells_) by_col[at[c.col]++] = c;
    size_t o = 0;
    for (size_t j = 0; j < ncol; ++j) {
      Cell *b = by_col.data() + start[j], *e = by_col.data() + start[j + 1];
      for (Cell *p = b + 1; p < e; ++p) {
        const Cell c = *p;
        Cell *q = p;
        while (q > b && (q - 1)->row > c.row) { *q = *(q - 1); --q; }
        *q = c;
      }
      for (Cell *p = b; p < e; ++p) {
        if (p + 1 < e && (p + 1)->row == p->row) continue;    // a later write wins
        cells_[o++] = *p;
      }
    }
    cells_.resize(o);
    sorted_ = true;
  }
  std::vector<double> lo_, up_;

  static OptPair dim(size_t j, const Constraint<N_DIM> &c) {
    OptPair r;
    if (c.first) r.first = (*c.first)[j];
    if (c.second) r.second = (*c.second)[j];
    return r;
  }
  void put(size_t row, std::initializer_list<std::pair<size_t, double>> eq, OptPair b) {
    for (const auto &[col, coeff] : eq) set(col, row, coeff);
    if (b.first) lo_[row] = *b.first;
    if (b.second) up_[row] = *b.second;
    assert(lo_[row] <= up_[row]);
  }
  ConstraintBuilder &boxes(size_t first_start, size_t last_start, const Constraint<N_DIM> &c) {
    for (size_t s = first_start; s <= last_start; s += N_DIM)
      for (size_t j = 0; j < N_DIM; ++j) put(user_off_ + s + j, {{s + j, 1.0}}, dim(j, c));
    return *this;
  }
  void axisRow(size_t row, const RobotBall &ball, Axis axis, const std::array<double, 3 * N_DIM> &J, size_t waypoint,
               double low, double upp) {
    for (size_t j = 0; j < N_DIM; ++j) set(nthPos(waypoint) + j, row, J[axis * N_DIM + j]);
    lo_[row] = low + ball.radius;
    up_[row] = upp - ball.radius;
    assert(lo_[row] <= up_[row]);
  }
  // nrm' J with nrm = (p - c) / |p - c| (+Z when p sits on the segment), written whether the row is active or not; active
  // within `margin` of the surface: (R + r) - dist + (nrm' J) q <= (nrm' J) x, the ball's radius is part of the bound
  void capsuleRow(size_t row, const RobotBall &ball, const CapsuleObstacle &cap, const Point &p, const std::array<double, 3 * N_DIM> &J,
                  const Vec<N_DIM> &q, size_t waypoint) {
    const Point v = cap.offset(p);
    const double dist = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), reach = cap.radius + ball.radius;
    const bool far = dist > 1e-12;
    const Point nrm{far ? v[0] / dist : 0.0, far ? v[1] / dist : 0.0, far ? v[2] / dist : 1.0};
    double gq = 0.0;
    for (size_t j = 0; j < N_DIM; ++j) {
      const double g = nrm[0] * J[0 * N_DIM + j] + nrm[1] * J[1 * N_DIM + j] + nrm[2] * J[2 * N_DIM + j];
      set(nthPos(waypoint) + j, row, g);
      gq += g * q[j];
    }
    lo_[row] = dist - reach < cap.margin ? (reach - dist) + gq : -INF;
    up_[row] = INF;
  }
  // n' J with n the cuboid's normal at p (CuboidObstacle::probe), written whether the row is active or not; active within
  // `margin` of the surface: (R + r) - sd + (n' J) q <= (n' J) x, the ball's radius is part of the bound
  void cuboidRow(size_t row, const RobotBall &ball, const CuboidObstacle &cub, const Point &p, const std::array<double, 3 * N_DIM> &J,
                 const Vec<N_DIM> &q, size_t waypoint) {
    const auto [sd, nrm] = cub.probe(p);
    const double reach = cub.radius + ball.radius;
    double gq = 0.0;
    for (size_t j = 0; j < N_DIM; ++j) {
      const double g = nrm[0] * J[0 * N_DIM + j] + nrm[1] * J[1 * N_DIM + j] + nrm[2] * J[2 * N_DIM + j];
      set(nthPos(waypoint) + j, row, g);
      gq += g * q[j];
    }
    lo_[row] = sd - reach < cub.margin ? (reach - sd) + gq : -INF;
    up_[row] = INF;
  }
  // G' J with G the gradient of the grid's interpolant at p (DistanceGrid::sample), not normalised, written whether the row is
  // active or not; active within `margin`: (offset + r) - phi + (G' J) q <= (G' J) x.  Outside the box: a zero row, no bounds
  void gridRow(size_t row, const RobotBall &ball, const DistanceGrid &gr, const Point &p, const std::array<double, 3 * N_DIM> &J,
               const Vec<N_DIM> &q, size_t waypoint) {
    const DistanceGrid::Sample sm = gr.sample(p);
    const double reach = gr.offset + ball.radius;
    double gq = 0.0;
    for (size_t j = 0; j < N_DIM; ++j) {
      const double g = sm.inside ? sm.grad[0] * J[0 * N_DIM + j] + sm.grad[1] * J[1 * N_DIM + j] + sm.grad[2] * J[2 * N_DIM + j] : 0.0;
      set(nthPos(waypoint) + j, row, g);
      gq += g * q[j];
    }
    lo_[row] = sm.inside && sm.phi - reach < gr.margin ? (reach - sm.phi) + gq : -INF;
    up_[row] = INF;
  }
  // n' J_a - n' J_b with n = (p_a - p_b) / |p_a - p_b| (+Z when the centres coincide), written whether the row is active or
  // not; active within `margin` of contact: (r_a + r_b) - dist + (n' (J_a - J_b)) q <= (n' (J_a - J_b)) x
  void pairRow(size_t row, const BallPair &pr, const QPVector &trajectory, size_t waypoint) {
    const RobotBall &A = balls_[pr.a], &B = balls_[pr.b];
    Vec<N_DIM> q;
    for (size_t j = 0; j < N_DIM; ++j) q[j] = trajectory[waypoint * N_DIM + j];
    const auto [ax, ay, az] = A.fk(q.data());
    const auto [bx, by, bz] = B.fk(q.data());
    const Point v{ax - bx, ay - by, az - bz};
    const double dist = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), reach = A.radius + B.radius;
    const bool far = dist > 1e-12;
    const Point nrm{far ? v[0] / dist : 0.0, far ? v[1] / dist : 0.0, far ? v[2] / dist : 1.0};
    std::array<double, 3 * N_DIM> Ja{}, Jb{};
    A.jacobian(Ja.data(), q.data());
    B.jacobian(Jb.data(), q.data());
    double gq = 0.0;
    for (size_t j = 0; j < N_DIM; ++j) {
      const double g = (nrm[0] * Ja[0 * N_DIM + j] + nrm[1] * Ja[1 * N_DIM + j] + nrm[2] * Ja[2 * N_DIM + j]) -
                       (nrm[0] * Jb[0 * N_DIM + j] + nrm[1] * Jb[1 * N_DIM + j] + nrm[2] * Jb[2 * N_DIM + j]);
      set(nthPos(waypoint) + j, row, g);
      gq += g * q[j];
    }
    lo_[row] = dist - reach < pr.margin ? (reach - dist) + gq : -INF;
    up_[row] = INF;
  }
  // the gradient of c = u . ref, written whether the row is active or not; active within `margin` radians of the cone:
  // cos(max_angle) - c + g q <= g x, the linearisation of c(x) >= cos(max_angle) around q
  void tiltRow(size_t row, const TiltLimit &t, const QPVector &trajectory, size_t waypoint) {
    Vec<N_DIM> q, g;
    for (size_t j = 0; j < N_DIM; ++j) q[j] = trajectory[waypoint * N_DIM + j];
    const double c = tiltCosine<N_DIM>(t, q.data(), g.data());
    double gq = 0.0;
    for (size_t j = 0; j < N_DIM; ++j) {
      set(nthPos(waypoint) + j, row, g[j]);
      gq += g[j] * q[j];
    }
    lo_[row] = c < t.cosActive() ? (t.cosLimit() - c) + gq : -INF;
    up_[row] = INF;
  }
  // the four rows of a goal, from `row` on, in the columns of its waypoint: J[ax] with the box around the target point for
  // x, y, z (a free axis: no bounds), then the gradient of c = u . ref with cos(max_angle) - c + g q <= g x (no axis: zeros,
  // no bounds).  Always active.
  void goalRow(size_t row, const GraspGoal &gl, const QPVector &trajectory) {
    const size_t w = gl.waypoint;
    const RobotBall &ball = balls_[gl.ball];
    Vec<N_DIM> q, g;
    for (size_t j = 0; j < N_DIM; ++j) q[j] = trajectory[w * N_DIM + j];
    const auto [px, py, pz] = ball.fk(q.data());
    const Point p{px, py, pz};
    std::array<double, 3 * N_DIM> J{};
    ball.jacobian(J.data(), q.data());
    for (size_t ax = 0; ax < 3; ++ax) {
      double Jq = 0.0;
      for (size_t j = 0; j < N_DIM; ++j) {
        set(nthPos(w) + j, row + ax, J[ax * N_DIM + j]);
        Jq += J[ax * N_DIM + j] * q[j];
      }
      const bool free_axis = gl.target.tol[ax] >= GOAL_FREE;
      lo_[row + ax] = free_axis ? -INF : ((gl.target.point[ax] - gl.target.tol[ax]) - p[ax]) + Jq;
      up_[row + ax] = free_axis ? INF : ((gl.target.point[ax] + gl.target.tol[ax]) - p[ax]) + Jq;
    }
    double c = 0.0, gq = 0.0;
    g.fill(0.0);
    if (gl.axis) c = goalCosine<N_DIM>(gl, q.data(), g.data());
    for (size_t j = 0; j < N_DIM; ++j) {
      set(nthPos(w) + j, row + 3, g[j]);
      gq += g[j] * q[j];
    }
    lo_[row + 3] = gl.axis ? (gl.cosLimit() - c) + gq : -INF;
    up_[row + 3] = INF;
  }
};

// ------------------------------------------------------------------- gomp-solver.h
namespace detail {
template <class S, class = void> struct has_prefetch : std::false_type {};
template <class S>
struct has_prefetch<S, std::void_t<decltype(S::prefetch(std::declval<const QPConstraints &>(), std::declval<const QPMatrixSparse &>()))>> : std::true_type {};
}  // namespace detail
constexpr int MAX_ITERATIONS = 100;
constexpr int SEGMENTS = 10;

template <size_t N_DIM, class SolverT = QPSolver>
class GOMPSolver {
 public:
  GOMPSolver(size_t waypoints, double time_step, const Constraint<N_DIM> &pos_con, const Constraint<N_DIM> &vel_con,
             const Constraint<N_DIM> &acc_con, const Constraint<3> &con_3d, std::vector<HorizontalLine> obstacles,
             std::vector<RobotBall> m, InverseKinematics gripper_ik = nullptr, bool verbose = false)
      : max_waypoints(waypoints), time_step(time_step), pos_con(pos_con),
        vel_con(constraints::scaled<N_DIM>(vel_con, time_step)),
        acc_con(constraints::scaled<N_DIM>(acc_con, time_step * time_step)), con_3d(con_3d),
        obstacles(std::move(obstacles)), mappers(std::move(m)), gripper_ik(std::move(gripper_ik)), verbose(verbose) {
    assert(max_waypoints >= 4);
  }

  // horizon-shrinking outer loop: SEGMENTS QPs chains of W = max_waypoints * i / SEGMENTS waypoints
  std::pair<ExitCode, QPVector> run(Ctrl<N_DIM> start_pos, Ctrl<N_DIM> end_pos) {
    QPVector last_solution = calcWarmStart(start_pos, end_pos);
    ExitCode last_code = ExitCode::kUnknown;
    // Not in the reference: the horizons of this run are known now, and a solver backend that can analyse a sparsity pattern
    // ahead of time (SolverT::prefetch) does so for the later horizons on spare host threads while the first ones are solved.
    PrefetchJoiner prefetching;
    if constexpr (detail::has_prefetch<SolverT>::value) {
      if (prefetch_patterns && max_waypoints * N_DIM >= 600)
        for (int i = SEGMENTS - 1; i >= 1; --i) {
          const size_t waypoints = max_waypoints * i / SEGMENTS;
          if (waypoints < 4) continue;
          prefetching.threads.emplace_back([this, waypoints, start_pos, end_pos] {
            ConstraintBuilder<N_DIM> b = jointSpaceRows(start_pos, end_pos, waypoints);
            SolverT::prefetch(b.withObstaclePattern().build(), triDiagonalMatrix(2, -1, (int)(N_DIM * 2 * waypoints), (int)(waypoints * N_DIM), (int)N_DIM));
          });
        }
    }
    for (int i = SEGMENTS; i >= 1; --i) {
      const size_t waypoints = max_waypoints * i / SEGMENTS;
      if (waypoints < 4) break;                              // (max_waypoints < 40: the last horizons are too short for the end conditions)
      QPVector warm_start(waypoints * N_DIM * 2);
      // same slicing as the reference, including its quirk for i < SEGMENTS (the "velocity" half is
      // taken at offset W*D of the previous, longer solution)
      for (size_t k = 0; k < waypoints * N_DIM; ++k) {
        warm_start[k] = last_solution[k];
        warm_start[waypoints * N_DIM + k] = last_solution[waypoints * N_DIM + k];
      }
      auto [exit_code, solution] = run(start_pos, end_pos, waypoints, warm_start);
      ++segments_run;
      if (exit_code != ExitCode::kOptimal && exit_code != ExitCode::kUnknown) break;
      if (exit_code == ExitCode::kOptimal) { last_code = ExitCode::kOptimal; last_solution = solution; }
    }
    for (size_t k = last_solution.size() / 2; k < last_solution.size(); ++k) last_solution[k] /= time_step;
    return {last_code, last_solution};
  }

  // The same with a grasp goal for an end condition (`goal` names the ball and the axis): the third-last waypoint of every
  // horizon must reach `target` instead of one joint vector.  `seed` - joints that reach it, from any IK - is used only for
  // the joint-space warm start; the planner chooses the end point.  Zero end velocity and acceleration stay.
  std::pair<ExitCode, QPVector> run(Ctrl<N_DIM> start_pos, Ctrl<N_DIM> seed, const GoalTarget &target) {
    assert(goal);
    target_ = &target;
    auto res = run(start_pos, seed);
    target_ = nullptr;
    return res;
  }

  // SQP inner loop for one horizon
  std::pair<ExitCode, QPVector> run(Ctrl<N_DIM> start_pos, Ctrl<N_DIM> end_pos, size_t waypoints, const QPVector &warm_start) {
    ConstraintBuilder<N_DIM> builder = initConstraints(start_pos, end_pos, warm_start, waypoints);
    SolverT qp_solver{builder.build(), triDiagonalMatrix(2, -1, (int)(N_DIM * 2 * waypoints), (int)(waypoints * N_DIM), (int)N_DIM), verbose};
    qp_solver.setWarmStart(warm_start);
    QPVector last_solution = warm_start;
    ExitCode last_code = ExitCode::kUnknown;
    int i = 0;
    while (i++ < MAX_ITERATIONS) {
      auto [exit_code, solution] = qp_solver.solve();
      ++qp_solves;
      if (exit_code != ExitCode::kOptimal) { last_solution = solution; break; }      // there are no solutions
      if (isSolutionOK(solution)) { last_solution = solution; last_code = ExitCode::kOptimal; break; }
      qp_solver.update(builder.withObstacles(con_3d, solution).build());
      ++qp_updates;
    }
    return {last_code, last_solution};
  }

  // counters for tests / reporting
  int segments_run = 0, qp_solves = 0, qp_updates = 0;
  bool prefetch_patterns = true;
  // Not in the reference: capsule / sphere obstacles besides the lines; set before run()
  std::vector<CapsuleObstacle> capsules;
  // Not in the reference either: cuboid obstacles (oriented boxes); set before run()
  std::vector<CuboidObstacle> cuboids;
  // Self-collision: pairs of `mappers` balls that must stay apart (dhSelfPairs of dh_kinematics.hpp makes them); set before run()
  std::vector<BallPair> pairs;
  // Tilt limits: axes of the arm that must stay within an angle of a world direction (dhTilt of dh_kinematics.hpp makes them); set before run()
  std::vector<TiltLimit> tilts;
  // Distance grids: a sensed world, sampled trilinearly (DistanceGrid::fromObstacles makes one from primitives); set before run()
  std::vector<DistanceGrid> grids;
  // The structure of the grasp goal of run(start, seed, target): ball and axis (dhGoal of dh_kinematics.hpp makes one); its
  // waypoint is set by the planner, its target by the call.  run(start, end) does not look at it.
  std::optional<GraspGoal> goal;
  // (tests) the acceptance test that ends the SQP loop; with a target: that of run(start, seed, target)
  bool acceptable(const QPVector &q_trajectory) const { return isSolutionOK(q_trajectory); }
  bool acceptable(const QPVector &q_trajectory, const GoalTarget &target) {
    target_ = &target;
    const bool r = isSolutionOK(q_trajectory);
    target_ = nullptr;
    return r;
  }
  // (tests) the first QP of a horizon, as run() sets it up: constraints linearised around the warm start
  QPConstraints firstConstraints(const Ctrl<N_DIM> &start_pos, const Ctrl<N_DIM> &end_pos, size_t waypoints, const QPVector &warm_start,
                                 const GoalTarget *target = nullptr) {
    target_ = target;
    QPConstraints c = initConstraints(start_pos, end_pos, warm_start, waypoints).build();
    target_ = nullptr;
    return c;
  }

 private:
  struct PrefetchJoiner { std::vector<std::thread> threads; ~PrefetchJoiner() { for (auto &t : threads) t.join(); } };
  const size_t max_waypoints;
  const double time_step;
  const Constraint<N_DIM> pos_con, vel_con, acc_con;
  const Constraint<3> con_3d;
  const std::vector<HorizontalLine> obstacles;
  const std::vector<RobotBall> mappers;
  const InverseKinematics gripper_ik;
  const bool verbose;
  const GoalTarget *target_ = nullptr;       // run(start, seed, target) in progress

  // `goal` at the third-last of `waypoints` waypoints, asking for *target_
  std::vector<GraspGoal> goalsAt(size_t waypoints) const {
    if (!target_) return {};
    GraspGoal g = *goal;
    g.waypoint = waypoints - 3; g.target = *target_;
    return {g};
  }

  QPVector calcWarmStart(const Ctrl<N_DIM> &start_pos, const Ctrl<N_DIM> &end_pos) const {
    if (target_) return goalWarmStart<N_DIM>(start_pos, end_pos, max_waypoints);
    QPVector w = linspace<N_DIM>(start_pos, end_pos, max_waypoints);      // joint-space line, zero velocities
    w.resize(2 * max_waypoints * N_DIM, 0.0);
    return w;
  }

  ConstraintBuilder<N_DIM> initConstraints(const Ctrl<N_DIM> &start_pos, const Ctrl<N_DIM> &end_pos, const QPVector &warm_start,
                                           size_t waypoints) const {
    ConstraintBuilder<N_DIM> b = jointSpaceRows(start_pos, end_pos, waypoints);
    b.withObstacles(con_3d, warm_start);
    return b;
  }
  ConstraintBuilder<N_DIM> jointSpaceRows(const Ctrl<N_DIM> &start_pos, const Ctrl<N_DIM> &end_pos, size_t waypoints) const {
    assert(waypoints >= 4);
    ConstraintBuilder<N_DIM> b{waypoints, mappers, obstacles, capsules, cuboids, pairs, tilts, grids, goalsAt(waypoints)};
    b.position(0, constraints::equal<N_DIM>(start_pos))
        .positions(1, waypoints - 2, pos_con)
        .position(waypoints - 3, target_ ? pos_con : constraints::equal<N_DIM>(end_pos))
        .velocities(0, waypoints - 4, vel_con)
        .velocity(waypoints - 3, constraints::eqZero<N_DIM>())
        .accelerations(0, waypoints - 4, acc_con)
        .acceleration(waypoints - 3, constraints::eqZero<N_DIM>());
    return b;
  }

  bool isSolutionOK(const QPVector &q_trajectory) const {
    bool res = true;
    for (const RobotBall &ball : mappers) {
      const QPVector xyz = mapJointTrajectoryToXYZ<N_DIM>(q_trajectory, ball.fk);
      const int waypoints = (int)xyz.size() / 3;
      for (int w = 0; w < waypoints; ++w) {
        const Point p{xyz[3 * w], xyz[3 * w + 1], xyz[3 * w + 2]};
        if (verbose) std::printf("(%f, %f, %f)\n", p[X], p[Y], p[Z]);
        if (ball.is_gripper) {
          for (Axis axis : XYZ_AXES) {
            const double lo = con_3d.first ? (*con_3d.first)[axis] : -INF;
            const double up = con_3d.second ? (*con_3d.second)[axis] : INF;
            if (!(lo - ERROR <= p[axis] - ball.radius && p[axis] + ball.radius <= up + ERROR)) res = false;
          }
        }
        for (const HorizontalLine &line : obstacles)
          if (line.hasCollision(w, xyz, ball) && !line.isAbove(p, ball)) res = false;
        if (!capsulesClear(capsules, p, ball)) res = false;
        if (!cuboidsClear(cuboids, p, ball)) res = false;
        if (!gridsClear(grids, p, ball)) res = false;
      }
    }
    if (!pairsClearAlong<N_DIM>(pairs, mappers, q_trajectory)) res = false;
    if (!tiltsOKAlong<N_DIM>(tilts, q_trajectory)) res = false;
    if (target_ && !goalsOKAlong<N_DIM>(goalsAt(q_trajectory.size() / 2 / N_DIM), mappers, q_trajectory)) res = false;
    return res;
  }
};

// ------------------------------------------------------ batched driver ("many trajectories")
// B independent (start, end) pairs run the same horizon-shrinking / SQP schedule as GOMPSolver::run in
// LOCK-STEP on one BatchQPSolver: all trajectories of a segment share W, hence one sparsity pattern.  Each
// trajectory follows exactly the decisions the sequential driver would take for it (same QPs, same updates,
// same accepted solutions); trajectories that have finished a segment simply keep their constraints while the
// others re-linearise (their extra solves start from the converged iterate and stop at the first check).
template <size_t N_DIM, class BatchSolverT = BatchQPSolver>
class BatchGOMPSolver {
 public:
  BatchGOMPSolver(size_t waypoints, double time_step, const Constraint<N_DIM> &pos_con, const Constraint<N_DIM> &vel_con,
                  const Constraint<N_DIM> &acc_con, const Constraint<3> &con_3d, std::vector<HorizontalLine> obstacles,
                  std::vector<RobotBall> m, bool verbose = false)
      : max_waypoints(waypoints), time_step(time_step), pos_con(pos_con),
        vel_con(constraints::scaled<N_DIM>(vel_con, time_step)),
        acc_con(constraints::scaled<N_DIM>(acc_con, time_step * time_step)), con_3d(con_3d),
        obstacles(std::move(obstacles)), mappers(std::move(m)), verbose(verbose) {
    assert(max_waypoints >= 4);
  }

  std::vector<std::pair<ExitCode, QPVector>> run(const std::vector<Ctrl<N_DIM>> &starts, const std::vector<Ctrl<N_DIM>> &ends) {
    const size_t B = starts.size();
    assert(ends.size() == B && B > 0);
    std::vector<QPVector> last_solution(B);
    std::vector<ExitCode> last_code(B, ExitCode::kUnknown);
    std::vector<char> alive(B, 1);
    segments_run.assign(B, 0); qp_solves.assign(B, 0); qp_updates.assign(B, 0);
    batch_solves = 0;
    seconds_build = seconds_setup = seconds_solve = seconds_update = 0.0;
    using clk_ = std::chrono::steady_clock;
    auto since_ = [](clk_::time_point t) { return std::chrono::duration<double>(clk_::now() - t).count(); };
    for (size_t b = 0; b < B; ++b) {
      if (targets_) { last_solution[b] = goalWarmStart<N_DIM>(starts[b], ends[b], max_waypoints); continue; }
      last_solution[b] = linspace<N_DIM>(starts[b], ends[b], max_waypoints);      // joint-space line, zero velocities
      last_solution[b].resize(2 * max_waypoints * N_DIM, 0.0);
    }
    for (int i = SEGMENTS; i >= 1; --i) {
      const size_t waypoints = max_waypoints * i / SEGMENTS;
      if (waypoints < 4) break;                                // (max_waypoints < 40: the last horizons are too short for the end conditions)
      std::vector<size_t> ids;                                 // batch slot -> trajectory
      for (size_t b = 0; b < B; ++b) if (alive[b]) ids.push_back(b);
      if (ids.empty()) break;
      const size_t K = ids.size();
      std::vector<QPVector> warm(K), seg_solution(K);
      std::vector<ExitCode> seg_code(K, ExitCode::kUnknown);
      std::vector<ConstraintBuilder<N_DIM>> builders;
      std::vector<QPConstraints> cons(K);
      auto tb_ = clk_::now();
      // The joint-space rows of a segment differ between the trajectories only in the bounds of the first and the third-last
      // waypoint: they are laid down once (same calls, same order as initConstraints) and copied; each trajectory then
      // repeats its two position() calls - in the sequential order they are the last writes to those rows as well - and
      // adds its own obstacle rows.  Same QPConstraints as initConstraints(), a third of the time.
      const ConstraintBuilder<N_DIM> tmpl = jointSpaceTemplate(starts[ids[0]], ends[ids[0]], waypoints);
      builders.assign(K, ConstraintBuilder<N_DIM>{4, {}, {}});
      // the K trajectories are independent: their constraints are built by a few host threads
      parallel_for_(K, [&](size_t k) {
        const QPVector &prev = last_solution[ids[k]];
        warm[k].resize(waypoints * N_DIM * 2);
        for (size_t t = 0; t < waypoints * N_DIM; ++t) {        // same slicing as GOMPSolver::run
          warm[k][t] = prev[t];
          warm[k][waypoints * N_DIM + t] = prev[waypoints * N_DIM + t];
        }
        builders[k] = tmpl;
        builders[k].position(0, constraints::equal<N_DIM>(starts[ids[k]]));
        if (targets_) builders[k].setGoalTarget(0, (*targets_)[ids[k]]);
        else builders[k].position(waypoints - 3, constraints::equal<N_DIM>(ends[ids[k]]));
        builders[k].withObstacles(con_3d, warm[k]);
        cons[k] = builders[k].build();
        seg_solution[k] = warm[k];
      });
      seconds_build += since_(tb_);
      auto ts_ = clk_::now();
      // One solver per horizon segment, as the reference builds them ([REF] src/gomp-solver.h:61) - but kept across run()
      // calls: when this segment's P and A are those of the solver built for it earlier (joint-space rows: only the bounds
      // depend on the trajectory), the handle is put back into its post-construction state and given the new bounds
      // (BatchQPSolver::reinit: bitwise a fresh construction) instead of being analysed, uploaded and factored again.
      const QPMatrixSparse Pseg = triDiagonalMatrix(2, -1, (int)(N_DIM * 2 * waypoints), (int)(waypoints * N_DIM), (int)N_DIM);
      std::unique_ptr<BatchSolverT> &slot = solver_cache_[(size_t)(SEGMENTS - i)];
      if (reuse_solvers && slot && reinit_(*slot, cons, Pseg)) ++solver_reuses;
      else slot = std::make_unique<BatchSolverT>(cons, Pseg, verbose);
      BatchSolverT &qp = *slot;
      qp.setWarmStart(warm);
      seconds_setup += since_(ts_);
      std::vector<char> running(K, 1);
      size_t n_running = K;
      for (int it = 0; it < MAX_ITERATIONS && n_running; ++it) {
        auto tq_ = clk_::now();
        auto res = qp.solve();
        seconds_solve += since_(tq_);
        ++batch_solves;
        bool need_update = false;
        auto tu_ = clk_::now();
        for (size_t k = 0; k < K; ++k) {
          if (!running[k]) continue;
          ++qp_solves[ids[k]];
          const auto &[exit_code, solution] = res[k];
          if (exit_code != ExitCode::kOptimal) { seg_solution[k] = solution; running[k] = 0; --n_running; continue; }
          if (isSolutionOK(solution, ids[k])) { seg_solution[k] = solution; seg_code[k] = ExitCode::kOptimal; running[k] = 0; --n_running; continue; }
          if (it + 1 < MAX_ITERATIONS) {
            cons[k] = builders[k].withObstacles(con_3d, solution).build();
            ++qp_updates[ids[k]];
            need_update = true;
          }
        }
        if (need_update && n_running) qp.update(cons);
        seconds_update += since_(tu_);
      }
      for (size_t k = 0; k < K; ++k) {
        const size_t b = ids[k];
        ++segments_run[b];
        if (seg_code[k] != ExitCode::kOptimal && seg_code[k] != ExitCode::kUnknown) { alive[b] = 0; continue; }
        if (seg_code[k] == ExitCode::kOptimal) { last_code[b] = ExitCode::kOptimal; last_solution[b] = seg_solution[k]; }
      }
    }
    std::vector<std::pair<ExitCode, QPVector>> out(B);
    for (size_t b = 0; b < B; ++b) {
      for (size_t t = last_solution[b].size() / 2; t < last_solution[b].size(); ++t) last_solution[b][t] /= time_step;
      out[b] = {last_code[b], last_solution[b]};
    }
    return out;
  }

  // The same with a grasp goal for an end condition, as GOMPSolver::run(start, seed, target): `goal` names the ball and the
  // axis, targets[b] is what trajectory b asks, seeds[b] serves its joint-space warm start only.
  std::vector<std::pair<ExitCode, QPVector>> run(const std::vector<Ctrl<N_DIM>> &starts, const std::vector<Ctrl<N_DIM>> &seeds,
                                                 const std::vector<GoalTarget> &targets) {
    assert(goal && targets.size() == starts.size());
    targets_ = &targets;
    auto res = run(starts, seeds);
    targets_ = nullptr;
    return res;
  }
  std::optional<GraspGoal> goal;              // the structure of the goal of run(starts, seeds, targets); run(starts, ends) does not look at it

  // per-trajectory counters (comparable with GOMPSolver's) and the number of batched solves
  std::vector<int> segments_run, qp_solves, qp_updates;
  int batch_solves = 0;
  bool reuse_solvers = true;      // keep the per-segment solvers across run() calls (see run())
  std::vector<CapsuleObstacle> capsules;      // capsule / sphere obstacles besides the lines; set before run()
  std::vector<CuboidObstacle> cuboids;        // cuboid obstacles (oriented boxes); set before run()
  std::vector<BallPair> pairs;                // self-collision pairs of the balls; set before run()
  std::vector<TiltLimit> tilts;               // tilt limits; set before run()
  std::vector<DistanceGrid> grids;            // distance grids; set before run()
  int solver_reuses = 0;          // how often a kept solver was re-initialised instead of a new one being built
  // where the wall time of the last run() went: building constraints, QP setup (analysis + upload + factorisation),
  // batched solves, feasibility checks + re-linearisation + update
  double seconds_build = 0.0, seconds_setup = 0.0, seconds_solve = 0.0, seconds_update = 0.0;

 private:
  const size_t max_waypoints;
  const double time_step;
  const Constraint<N_DIM> pos_con, vel_con, acc_con;
  const Constraint<3> con_3d;
  const std::vector<HorizontalLine> obstacles;
  const std::vector<RobotBall> mappers;
  const bool verbose;
  const std::vector<GoalTarget> *targets_ = nullptr;      // run(starts, seeds, targets) in progress

  // `goal` at the third-last of `waypoints` waypoints (the targets are set per trajectory)
  std::vector<GraspGoal> goalsAt(size_t waypoints) const {
    if (!targets_) return {};
    GraspGoal g = *goal;
    g.waypoint = waypoints - 3;
    return {g};
  }

  std::array<std::unique_ptr<BatchSolverT>, SEGMENTS> solver_cache_;
  // (a batch solver type without reinit(), e.g. a test double, is always rebuilt)
  template <class S>
  static auto reinit_(S &s, const std::vector<QPConstraints> &cons, const QPMatrixSparse &P) -> decltype(s.reinit(cons, P)) { return s.reinit(cons, P); }
  static bool reinit_(...) { return false; }

  // body(k) for k in [0, count) on up to 16 host threads (the FK / Jacobian callbacks of the balls must be re-entrant,
  // which the reference's are: pure functions of the joint vector)
  template <class F>
  static void parallel_for_(size_t count, F &&body) {
    const size_t nt = std::min<size_t>({count, 16, std::max(1u, std::thread::hardware_concurrency())});
    if (nt <= 1) { for (size_t k = 0; k < count; ++k) body(k); return; }
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; ++t) th.emplace_back([&, t] { for (size_t k = t; k < count; k += nt) body(k); });
    for (auto &x : th) x.join();
  }

  // initConstraints of GOMPSolver ([REF] src/gomp-solver.h:98-110) without its last call (the obstacle rows), normalised
  ConstraintBuilder<N_DIM> jointSpaceTemplate(const Ctrl<N_DIM> &start_pos, const Ctrl<N_DIM> &end_pos, size_t waypoints) const {
    ConstraintBuilder<N_DIM> b{waypoints, mappers, obstacles, capsules, cuboids, pairs, tilts, grids, goalsAt(waypoints)};
    b.position(0, constraints::equal<N_DIM>(start_pos))
        .positions(1, waypoints - 2, pos_con)
        .position(waypoints - 3, targets_ ? pos_con : constraints::equal<N_DIM>(end_pos))
        .velocities(0, waypoints - 4, vel_con)
        .velocity(waypoints - 3, constraints::eqZero<N_DIM>())
        .accelerations(0, waypoints - 4, acc_con)
        .acceleration(waypoints - 3, constraints::eqZero<N_DIM>())
        .normalised();
    return b;
  }

  bool isSolutionOK(const QPVector &q_trajectory, size_t b) const {
    bool res = true;
    if (targets_) {                                               // the goal of trajectory b at the third-last waypoint
      std::vector<GraspGoal> gs = goalsAt(q_trajectory.size() / 2 / N_DIM);
      gs[0].target = (*targets_)[b];
      if (!goalsOKAlong<N_DIM>(gs, mappers, q_trajectory)) res = false;
    }
    for (const RobotBall &ball : mappers) {
      const QPVector xyz = mapJointTrajectoryToXYZ<N_DIM>(q_trajectory, ball.fk);
      const int waypoints = (int)xyz.size() / 3;
      for (int w = 0; w < waypoints; ++w) {
        const Point p{xyz[3 * w], xyz[3 * w + 1], xyz[3 * w + 2]};
        if (ball.is_gripper) {
          for (Axis axis : XYZ_AXES) {
            const double lo = con_3d.first ? (*con_3d.first)[axis] : -INF;
            const double up = con_3d.second ? (*con_3d.second)[axis] : INF;
            if (!(lo - ERROR <= p[axis] - ball.radius && p[axis] + ball.radius <= up + ERROR)) res = false;
          }
        }
        for (const HorizontalLine &line : obstacles)
          if (line.hasCollision(w, xyz, ball) && !line.isAbove(p, ball)) res = false;
        if (!capsulesClear(capsules, p, ball)) res = false;
        if (!cuboidsClear(cuboids, p, ball)) res = false;
        if (!gridsClear(grids, p, ball)) res = false;
      }
    }
    if (!pairsClearAlong<N_DIM>(pairs, mappers, q_trajectory)) res = false;
    if (!tiltsOKAlong<N_DIM>(tilts, q_trajectory)) res = false;
    return res;
  }
};

// ------------------------------------------------- continuous driver (SURVEY 8(f) rank 1 without the lock-step)
// The reference's loop is per trajectory: solve -> check -> re-linearise -> update -> solve again, one horizon after the
// other ([REF] src/gomp-solver.h:38-91).  BatchGOMPSolver advances B trajectories in lock-step and waits for the slowest
// QP of every round; here every trajectory walks through GOMPSolver::run on its own.  The ten horizons are ten STAGES:
// one ContinuousQPSolver (B slots, slot = trajectory) and one host thread each.  A trajectory entering a stage gets a
// freshly constructed QP in its slot (reinit: what [REF] src/gomp-solver.h:61-65 does), is warm-started and begun; the
// stage thread advances whatever is iterating in its solver, and as soon as ONE QP has finished its trajectory is
// checked, re-linearised and updated ([REF] :70-88) or handed to the next stage - while the other QPs keep iterating
// and the other stages run side by side on their own streams.  Every trajectory takes exactly the decisions of a
// sequential GOMPSolver::run: same QPs, same updates, same accepted solutions (tests/cpp/gomp_parity.cpp `cont`).
template <size_t N_DIM, class ContSolverT = ContinuousQPSolver>
class ContinuousGOMPSolver {
 public:
  ContinuousGOMPSolver(size_t waypoints, double time_step, const Constraint<N_DIM> &pos_con, const Constraint<N_DIM> &vel_con,
                       const Constraint<N_DIM> &acc_con, const Constraint<3> &con_3d, std::vector<HorizontalLine> obstacles,
                       std::vector<RobotBall> m, bool verbose = false)
      : max_waypoints(waypoints), time_step(time_step), pos_con(pos_con),
        vel_con(constraints::scaled<N_DIM>(vel_con, time_step)),
        acc_con(constraints::scaled<N_DIM>(acc_con, time_step * time_step)), con_3d(con_3d),
        obstacles(std::move(obstacles)), mappers(std::move(m)), verbose(verbose) {
    assert(max_waypoints >= 4);
  }

  std::vector<std::pair<ExitCode, QPVector>> run(const std::vector<Ctrl<N_DIM>> &starts, const std::vector<Ctrl<N_DIM>> &ends) {
    const size_t B = starts.size();
    assert(ends.size() == B && B > 0);
    starts_ = &starts; ends_ = &ends;
    const std::optional<GraspGoal> goal_now = targets_ ? goal : std::nullopt;
    if (!(capsules == scene_capsules_ && cuboids == scene_cuboids_ && pairs == scene_pairs_ && tilts == scene_tilts_ && grids == scene_grids_ && goal_now == scene_goal_)) {   // the kept scenes hold the capsules, cuboids, pairs and tilt limits of the run that made them
      for (Stage &st : stages_) if (st.scene) { mi_gomp_scene_free(st.scene); st.scene = nullptr; }
      scene_capsules_ = capsules;
      scene_cuboids_ = cuboids;
      scene_pairs_ = pairs;
      scene_tilts_ = tilts;
      scene_grids_ = grids;
      scene_goal_ = goal_now;
    }
    traj_.clear(); traj_.resize(B);
    segments_run.assign(B, 0); qp_solves.assign(B, 0); qp_updates.assign(B, 0);
    advances = 0; solver_reuses = 0;
    for (size_t b = 0; b < B; ++b) {
      if (targets_) traj_[b].last_solution = goalWarmStart<N_DIM>(starts[b], ends[b], max_waypoints);
      else {
        traj_[b].last_solution = linspace<N_DIM>(starts[b], ends[b], max_waypoints);      // joint-space line, zero velocities
        traj_[b].last_solution.resize(2 * max_waypoints * N_DIM, 0.0);
      }
      traj_[b].builder = std::make_unique<ConstraintBuilder<N_DIM>>(4, std::vector<RobotBall>{}, std::vector<HorizontalLine>{});
    }
    for (int s = 0; s < SEGMENTS; ++s) {
      stages_[s].waypoints = max_waypoints * (size_t)(SEGMENTS - s) / SEGMENTS;
      stages_[s].inbox.clear();
      stages_[s].first_admission = true;
      stages_[s].seconds_admit = stages_[s].seconds_wait = stages_[s].seconds_process = stages_[s].seconds_idle = 0.0;
      stages_[s].n_advances = 0;
    }
    for (size_t b = 0; b < B; ++b) stages_[0].inbox.push_back(b);
    finished_ = 0; failed_ = false;
    std::vector<std::thread> th;
    for (int s = 0; s < SEGMENTS; ++s) th.emplace_back([this, s, B] { stageLoop(s, B); });
    for (auto &t : th) t.join();
    std::vector<std::pair<ExitCode, QPVector>> out(B);
    for (size_t b = 0; b < B; ++b) {
      QPVector &x = traj_[b].last_solution;
      for (size_t t = x.size() / 2; t < x.size(); ++t) x[t] /= time_step;
      out[b] = {traj_[b].last_code, x};
    }
    return out;
  }

  // The same with a grasp goal for an end condition, as GOMPSolver::run(start, seed, target): `goal` names the ball and the
  // axis, targets[b] is what trajectory b asks, seeds[b] serves its joint-space warm start only.  On the device path the goal
  // goes into the scene (mi_gomp_scene_create_goals) and every arrival's target with it (mi_gomp_scene_set_goal_values).
  std::vector<std::pair<ExitCode, QPVector>> run(const std::vector<Ctrl<N_DIM>> &starts, const std::vector<Ctrl<N_DIM>> &seeds,
                                                 const std::vector<GoalTarget> &targets) {
    assert(goal && targets.size() == starts.size());
    targets_ = &targets;
    auto res = run(starts, seeds);
    targets_ = nullptr;
    return res;
  }
  // The structure of the goal of run(starts, seeds, targets); run(starts, ends) does not look at it.  The device path needs
  // its ball to name a built-in model and, if it has an axis, dh_chain and a goal made by dhGoal (builtin_frame >= 1).
  std::optional<GraspGoal> goal;

  // per-trajectory counters (comparable with GOMPSolver's)
  std::vector<int> segments_run, qp_solves, qp_updates;
  std::atomic<long> advances{0};       // advance() calls of all stages
  std::atomic<int> solver_reuses{0};   // stages whose solver was kept from the previous run()
  // Re-linearise on the device (mi_gomp_scene: FK / Jacobians of built-in kinematic models, row assembly, feasibility check,
  // update from device-resident rows) instead of on the stage's host thread.  Needs every ball to name its model
  // (RobotBall::withBuiltin; dhBall() does for the links of any serial arm, see dh_chain); the trajectories then agree with the host path to round-off (device sin / cos), not bitwise.
  bool device_assembly = false;
  // The DH chain of the balls made by dhBall() (include/mi_osqp/dh_kinematics.hpp, MI_GOMP_MODEL_DH_CHAIN): the device path
  // needs it next to them; without it such balls keep the planner on the host callbacks.
  std::optional<mi_gomp_chain> dh_chain;
  // Capsule / sphere obstacles besides the lines; set before run().  On the device path they go into the scene
  // (mi_gomp_scene_create_world).
  std::vector<CapsuleObstacle> capsules;
  // Cuboid obstacles (oriented boxes, optionally rounded); set before run().  On the device path they go into the scene
  // (mi_gomp_scene_create_cuboids).
  std::vector<CuboidObstacle> cuboids;
  // Self-collision pairs of the balls; set before run().  On the device path they go into the scene (mi_gomp_scene_create_pairs).
  std::vector<BallPair> pairs;
  // Tilt limits; set before run().  On the device path they go into the scene (mi_gomp_scene_create_tilts), which needs
  // dh_chain and limits made by dhTilt (builtin_frame set).
  std::vector<TiltLimit> tilts;
  // Distance grids; set before run().  On the device path they go into the scene (mi_gomp_scene_create_grids).
  std::vector<DistanceGrid> grids;
  // A new camera frame for grid k: new values of the same shape, on the host copy and in every kept device scene; between
  // run() calls.  false when k or the number of values is wrong, or a device scene refuses them.
  bool updateGrid(size_t k, std::vector<double> values) {
    if (k >= grids.size() || values.size() != grids[k].values->size()) return false;
    bool res = true;
    if (k < scene_grids_.size() && grids[k] == scene_grids_[k])
      for (Stage &st : stages_)
        if (st.scene && mi_gomp_scene_update_grid(st.scene, (int64_t)k, values.data()) != MI_OSQP_OK) res = false;
    if (!res) return false;
    grids[k].values = std::make_shared<const std::vector<double>>(std::move(values));
    if (k < scene_grids_.size()) scene_grids_[k].values = grids[k].values;
    return true;
  }
  int pipeline_depth = 1;              // 2: a stage enqueues its next advance before it looks at the previous one's results
  int segments_per_advance = 4;        // a launch runs on until a QP of the stage finishes, at most that many segments
  // per stage: {waypoints, advances, seconds admitting, waiting for the device, processing finished QPs, idle}
  std::vector<std::array<double, 6>> stageProfile() const {
    std::vector<std::array<double, 6>> r;
    for (const Stage &st : stages_) r.push_back({(double)st.waypoints, (double)st.n_advances, st.seconds_admit, st.seconds_wait, st.seconds_process, st.seconds_idle});
    return r;
  }

 private:
  const size_t max_waypoints;
  const double time_step;
  const Constraint<N_DIM> pos_con, vel_con, acc_con;
  const Constraint<3> con_3d;
  const std::vector<HorizontalLine> obstacles;
  const std::vector<RobotBall> mappers;
  const bool verbose;

  struct Traj {
    QPVector last_solution, warm, seg_solution;
    ExitCode last_code = ExitCode::kUnknown, seg_code = ExitCode::kUnknown;
    std::unique_ptr<ConstraintBuilder<N_DIM>> builder;
    QPConstraints cons;
    int sqp_it = 0;
  };
  struct Stage {
    size_t waypoints = 0;
    std::unique_ptr<ContSolverT> qp;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<size_t> inbox;                       // trajectories that have reached this horizon
    mi_gomp_scene *scene = nullptr;                 // device-side re-linearisation of this stage's solver (device_assembly)
    ~Stage() { if (scene) mi_gomp_scene_free(scene); }
    bool first_admission = true;
    // where the stage thread's time went in the last run(): preparing + admitting arrivals, waiting for the device in
    // poll(), checking / re-linearising / updating finished QPs, waiting for arrivals
    double seconds_admit = 0.0, seconds_wait = 0.0, seconds_process = 0.0, seconds_idle = 0.0;
    long n_advances = 0;
  };
  std::vector<Traj> traj_;
  std::array<Stage, SEGMENTS> stages_;
  std::vector<CapsuleObstacle> scene_capsules_;
  std::vector<CuboidObstacle> scene_cuboids_;
  std::vector<BallPair> scene_pairs_;
  std::vector<TiltLimit> scene_tilts_;
  std::vector<DistanceGrid> scene_grids_;
  std::optional<GraspGoal> scene_goal_;                // the goal structure of the kept scenes (none: they were made without)
  const std::vector<GoalTarget> *targets_ = nullptr;   // run(starts, seeds, targets) in progress
  // `goal` at the third-last of `waypoints` waypoints (the targets are set per trajectory)
  std::vector<GraspGoal> goalsAt(size_t waypoints) const {
    if (!targets_) return {};
    GraspGoal g = *goal;
    g.waypoint = waypoints - 3;
    return {g};
  }
  const std::vector<Ctrl<N_DIM>> *starts_ = nullptr, *ends_ = nullptr;
  std::atomic<size_t> finished_{0};
  std::atomic<bool> failed_{false};

  void wakeAll() { for (Stage &st : stages_) { std::lock_guard<std::mutex> lk(st.mu); st.cv.notify_all(); } }

  void stageLoop(int s, size_t B) {
    Stage &st = stages_[(size_t)s];
    const size_t W = st.waypoints;
    if (W < 4) return;                               // (max_waypoints < 40: too short for the end conditions; nothing is sent here, see process())
    const QPMatrixSparse P = triDiagonalMatrix(2, -1, (int)(N_DIM * 2 * W), (int)(W * N_DIM), (int)N_DIM);
    const ConstraintBuilder<N_DIM> tmpl = jointSpaceTemplate((*starts_)[0], (*ends_)[0], W);
    int in_flight = 0;                               // advances enqueued and not polled
    std::vector<size_t> arrivals;
    using clk_ = std::chrono::steady_clock;
    auto lap = [t = clk_::now()](double &acc) mutable { const auto now = clk_::now(); acc += std::chrono::duration<double>(now - t).count(); t = now; };
    double other = 0.0;
    while (finished_.load() < B && !failed_.load()) {
      // ---- trajectories that have reached this horizon: a freshly constructed QP each ([REF] src/gomp-solver.h:57-65)
      arrivals.clear();
      {
        std::unique_lock<std::mutex> lk(st.mu);
        const bool idle = in_flight == 0 && (!st.qp || st.qp->running() == 0);
        lap(other);
        if (idle) st.cv.wait(lk, [&] { return !st.inbox.empty() || finished_.load() >= B || failed_.load(); });
        lap(st.seconds_idle);
        while (!st.inbox.empty()) { arrivals.push_back(st.inbox.front()); st.inbox.pop_front(); }
      }
      if (!arrivals.empty()) { admit(st, P, tmpl, arrivals, B); lap(st.seconds_admit); }
      if (!st.qp) continue;
      // ---- one segment for everything that iterates here; the finished QPs decide the next step of their trajectories
      if (st.qp->running() > 0 && in_flight < pipeline_depth) {
        if (!st.qp->advance(segments_per_advance)) { failed_ = true; wakeAll(); break; }
        ++in_flight; ++advances; ++st.n_advances;
      }
      if (in_flight == 0) continue;
      if (in_flight < pipeline_depth && st.qp->running() > 0) continue;       // (fill the pipeline first)
      lap(other);
      const std::vector<long long> done = st.qp->poll();
      lap(st.seconds_wait);
      --in_flight;
      if (!done.empty()) { process(s, st, done, B); lap(st.seconds_process); }
    }
    // leave nothing enqueued behind
    while (st.qp && in_flight-- > 0) (void)st.qp->poll();
  }

  void admit(Stage &st, const QPMatrixSparse &P, const ConstraintBuilder<N_DIM> &tmpl, const std::vector<size_t> &arrivals, size_t B) {
    const size_t W = st.waypoints;
    auto prepare = [&](size_t k) {
      Traj &T = traj_[arrivals[k]];
      const QPVector &prev = T.last_solution;
      T.warm.resize(W * N_DIM * 2);
      for (size_t t = 0; t < W * N_DIM; ++t) {               // same slicing as GOMPSolver::run
        T.warm[t] = prev[t];
        T.warm[W * N_DIM + t] = prev[W * N_DIM + t];
      }
      *T.builder = tmpl;
      T.builder->position(0, constraints::equal<N_DIM>((*starts_)[arrivals[k]]));
      if (targets_) T.builder->setGoalTarget(0, (*targets_)[arrivals[k]]);
      else T.builder->position(W - 3, constraints::equal<N_DIM>((*ends_)[arrivals[k]]));
      T.builder->withObstacles(con_3d, T.warm);
      T.cons = T.builder->build();
      T.seg_solution = T.warm; T.seg_code = ExitCode::kUnknown; T.sqp_it = 0;
    };
    parallelFor(arrivals.size(), prepare);
    if (st.qp && !st.qp->compatible((long long)B, traj_[arrivals[0]].cons, P)) { if (st.scene) { mi_gomp_scene_free(st.scene); st.scene = nullptr; } st.qp.reset(); }
    if (st.qp) { if (st.first_admission) ++solver_reuses; }                       // (kept from the previous run(): every slot is re-initialised on arrival)
    else st.qp = std::make_unique<ContSolverT>((long long)B, traj_[arrivals[0]].cons, P, verbose);
    st.first_admission = false;
    if (useDevice() && !st.scene) makeScene(st);
    std::vector<long long> ids;
    std::vector<const QPConstraints *> cs;
    std::vector<const QPVector *> xs;
    for (size_t b : arrivals) { ids.push_back((long long)b); cs.push_back(&traj_[b].cons); xs.push_back(&traj_[b].warm); }
    st.qp->reinit(ids, cs);
    if (st.scene && targets_) {                                   // what the arrivals ask of the scene's goal
      std::vector<mi_gomp_goal_value> vals;
      for (size_t b : arrivals) {
        const GoalTarget &t = (*targets_)[b];
        mi_gomp_goal_value v{};
        for (int k = 0; k < 3; ++k) { v.point[k] = t.point[k]; v.tol[k] = t.tol[k]; v.ref[k] = t.ref[k]; }
        v.max_angle = t.max_angle;
        vals.push_back(v);
      }
      const int rc = mi_gomp_scene_set_goal_values(st.scene, (int64_t)ids.size(), reinterpret_cast<const int64_t *>(ids.data()), vals.data());
      if (rc != MI_OSQP_OK) { std::fprintf(stderr, "ContinuousGOMPSolver: goal values refused: %s (%s)\n", mi_osqp_error_name(rc), mi_osqp_last_error()); failed_ = true; wakeAll(); return; }
    }
    // (with a device scene the library keeps these rows on the device as well: the re-linearisations to come start from them)
    st.qp->setWarmStart(ids, xs);
    st.qp->begin(ids);
  }

  bool useDevice() const {
    if (!device_assembly) return false;
    for (const RobotBall &b : mappers) if (!b.builtin_model || (b.builtin_model == MI_GOMP_MODEL_DH_CHAIN && !dh_chain)) return false;
    for (const TiltLimit &t : tilts) if (t.builtin_frame < 1 || !dh_chain) return false;       // (a callback alone: the host path)
    if (targets_) {                                               // the goal's ball is one of the balls above; its axis as a tilt's
      if (goal->ball >= mappers.size()) return false;
      if (goal->axis && (goal->builtin_frame < 1 || !dh_chain)) return false;
    }
    return true;
  }
  void makeScene(Stage &st) {
    std::vector<mi_gomp_ball> balls;
    for (const RobotBall &b : mappers) {
      mi_gomp_ball g{};
      g.model = b.builtin_model; g.is_gripper = b.is_gripper ? 1 : 0; g.radius = b.radius;
      for (size_t k = 0; k < 12; ++k) g.param[k] = b.builtin_param[k];
      balls.push_back(g);
    }
    std::vector<mi_gomp_line> lines;
    for (const HorizontalLine &l : obstacles) {
      mi_gomp_line g{};
      g.dir[0] = l.directionXY()[0]; g.dir[1] = l.directionXY()[1];
      for (int k = 0; k < 3; ++k) g.point[k] = l.point()[k];
      g.below = l.bypassFromBelow() ? 1 : 0;
      lines.push_back(g);
    }
    double lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = con_3d.first ? (*con_3d.first)[k] : -INF; hi[k] = con_3d.second ? (*con_3d.second)[k] : INF; }
    std::vector<mi_gomp_capsule> caps;
    for (const CapsuleObstacle &c : capsules) {
      mi_gomp_capsule g{};
      for (int k = 0; k < 3; ++k) { g.a[k] = c.a[k]; g.b[k] = c.b[k]; }
      g.radius = c.radius; g.margin = c.margin;
      caps.push_back(g);
    }
    std::vector<mi_gomp_cuboid> cubs;
    for (const CuboidObstacle &c : cuboids) {
      mi_gomp_cuboid g{};
      for (int k = 0; k < 3; ++k) { g.centre[k] = c.centre[k]; g.half[k] = c.half[k]; }
      for (int k = 0; k < 9; ++k) g.axes[k] = c.axes[k];
      g.radius = c.radius; g.margin = c.margin;
      cubs.push_back(g);
    }
    std::vector<mi_gomp_pair> prs;
    for (const BallPair &p : pairs) prs.push_back(mi_gomp_pair{(int32_t)p.a, (int32_t)p.b, p.margin});
    std::vector<mi_gomp_tilt> tls;
    for (const TiltLimit &t : tilts) {
      mi_gomp_tilt g{};
      g.frame = (int32_t)t.builtin_frame;
      for (int k = 0; k < 3; k++) { g.axis[k] = t.builtin_axis[k]; g.ref[k] = t.ref[k]; }
      g.max_angle = t.max_angle; g.margin = t.margin;
      tls.push_back(g);
    }
    std::vector<mi_gomp_grid> grs;
    for (const DistanceGrid &d : grids) {
      mi_gomp_grid g{};
      for (int k = 0; k < 3; k++) { g.origin[k] = d.origin[k]; g.n[k] = (int32_t)d.n[k]; }
      g.cell = d.cell; g.offset = d.offset; g.margin = d.margin; g.values = d.values->data();
      grs.push_back(g);
    }
    std::vector<mi_gomp_goal> gls;
    for (const GraspGoal &g0 : goalsAt(st.waypoints)) {
      mi_gomp_goal g{};
      g.ball = (int32_t)g0.ball; g.waypoint = (int32_t)g0.waypoint; g.frame = g0.axis ? (int32_t)g0.builtin_frame : 0;
      for (int k = 0; k < 3; k++) g.axis[k] = g0.builtin_axis[k];
      gls.push_back(g);
    }
    const int rc = !gls.empty() ? mi_gomp_scene_create_goals(&st.scene, st.qp->handle(), (int64_t)N_DIM, (int64_t)st.waypoints, dh_chain ? &*dh_chain : nullptr,
                                                              (int64_t)balls.size(), balls.data(), (int64_t)lines.size(), lines.data(), (int64_t)caps.size(), caps.data(),
                                                              (int64_t)cubs.size(), cubs.data(), (int64_t)prs.size(), prs.data(), (int64_t)tls.size(), tls.data(),
                                                              (int64_t)grs.size(), grs.data(), (int64_t)gls.size(), gls.data(), lo, hi)
                   : !grs.empty() ? mi_gomp_scene_create_grids(&st.scene, st.qp->handle(), (int64_t)N_DIM, (int64_t)st.waypoints, dh_chain ? &*dh_chain : nullptr,
                                                              (int64_t)balls.size(), balls.data(), (int64_t)lines.size(), lines.data(), (int64_t)caps.size(), caps.data(),
                                                              (int64_t)cubs.size(), cubs.data(), (int64_t)prs.size(), prs.data(), (int64_t)tls.size(), tls.data(),
                                                              (int64_t)grs.size(), grs.data(), lo, hi)
                   : !tls.empty() ? mi_gomp_scene_create_tilts(&st.scene, st.qp->handle(), (int64_t)N_DIM, (int64_t)st.waypoints, dh_chain ? &*dh_chain : nullptr,
                                                              (int64_t)balls.size(), balls.data(), (int64_t)lines.size(), lines.data(), (int64_t)caps.size(), caps.data(),
                                                              (int64_t)cubs.size(), cubs.data(), (int64_t)prs.size(), prs.data(), (int64_t)tls.size(), tls.data(), lo, hi)
                   : !prs.empty() ? mi_gomp_scene_create_pairs(&st.scene, st.qp->handle(), (int64_t)N_DIM, (int64_t)st.waypoints, dh_chain ? &*dh_chain : nullptr,
                                                              (int64_t)balls.size(), balls.data(), (int64_t)lines.size(), lines.data(), (int64_t)caps.size(), caps.data(),
                                                              (int64_t)cubs.size(), cubs.data(), (int64_t)prs.size(), prs.data(), lo, hi)
                   : !cubs.empty() ? mi_gomp_scene_create_cuboids(&st.scene, st.qp->handle(), (int64_t)N_DIM, (int64_t)st.waypoints, dh_chain ? &*dh_chain : nullptr,
                                                                (int64_t)balls.size(), balls.data(), (int64_t)lines.size(), lines.data(), (int64_t)caps.size(), caps.data(),
                                                                (int64_t)cubs.size(), cubs.data(), lo, hi)
                   : !caps.empty() ? mi_gomp_scene_create_world(&st.scene, st.qp->handle(), (int64_t)N_DIM, (int64_t)st.waypoints, dh_chain ? &*dh_chain : nullptr,
                                                              (int64_t)balls.size(), balls.data(), (int64_t)lines.size(), lines.data(), (int64_t)caps.size(), caps.data(), lo, hi)
                   : dh_chain ? mi_gomp_scene_create_chain(&st.scene, st.qp->handle(), (int64_t)N_DIM, (int64_t)st.waypoints, &*dh_chain, (int64_t)balls.size(),
                                                         balls.data(), (int64_t)lines.size(), lines.data(), lo, hi)
                            : mi_gomp_scene_create(&st.scene, st.qp->handle(), (int64_t)N_DIM, (int64_t)st.waypoints, (int64_t)balls.size(), balls.data(),
                                                   (int64_t)lines.size(), lines.data(), lo, hi);
    if (rc != MI_OSQP_OK) std::fprintf(stderr, "ContinuousGOMPSolver: device scene failed (%s): falling back to the host path\n", mi_osqp_error_name(rc));
  }

  void process(int s, Stage &st, const std::vector<long long> &done, size_t B) {
    std::vector<long long> again;
    std::vector<const QPConstraints *> cs;
    std::vector<size_t> leaving;
    if (st.scene) {
      // the SQP step on the device: feasibility check, re-linearisation and update of the QPs whose trajectory is not accepted
      std::vector<long long> opt;
      std::vector<QPVector> sol;
      std::vector<double> xs;
      for (long long id : done) {
        const size_t b = (size_t)id;
        Traj &T = traj_[b];
        auto [exit_code, solution] = st.qp->result(id);
        ++qp_solves[b];
        if (exit_code != ExitCode::kOptimal) { T.seg_solution = std::move(solution); leaving.push_back(b); continue; }
        opt.push_back(id); xs.insert(xs.end(), solution.begin(), solution.end()); sol.push_back(std::move(solution));
      }
      std::vector<int32_t> ok(opt.size(), 0);
      if (!opt.empty()) {
        const int rc = mi_gomp_relinearise_some(st.scene, (int64_t)opt.size(), reinterpret_cast<const int64_t *>(opt.data()), xs.data(), ok.data());
        if (rc != MI_OSQP_OK) { std::fprintf(stderr, "ContinuousGOMPSolver: device re-linearisation failed: %s (%s)\n", mi_osqp_error_name(rc), mi_osqp_last_error()); failed_ = true; wakeAll(); return; }
      }
      for (size_t k = 0; k < opt.size(); ++k) {
        const size_t b = (size_t)opt[k];
        Traj &T = traj_[b];
        if (ok[k]) { T.seg_solution = std::move(sol[k]); T.seg_code = ExitCode::kOptimal; leaving.push_back(b); continue; }
        ++qp_updates[b];
        if (++T.sqp_it < MAX_ITERATIONS) again.push_back(opt[k]); else leaving.push_back(b);
      }
      if (!again.empty()) st.qp->begin(again);
      again.clear();
    } else
    for (long long id : done) {
      const size_t b = (size_t)id;
      Traj &T = traj_[b];
      auto [exit_code, solution] = st.qp->result(id);
      ++qp_solves[b];
      bool ends_here = true;
      if (exit_code != ExitCode::kOptimal) T.seg_solution = std::move(solution);                          // there are no solutions
      else if (isSolutionOK(solution, b)) { T.seg_solution = std::move(solution); T.seg_code = ExitCode::kOptimal; }
      else {
        // (the reference re-linearises and updates also in the last of its MAX_ITERATIONS rounds; that update has no reader)
        ++qp_updates[b];
        if (++T.sqp_it < MAX_ITERATIONS) {
          T.cons = T.builder->withObstacles(con_3d, solution).build();
          again.push_back(id); cs.push_back(&T.cons);
          ends_here = false;
        }
      }
      if (ends_here) leaving.push_back(b);
    }
    if (!again.empty()) { st.qp->update(again, cs); st.qp->begin(again); }
    for (size_t b : leaving) {
      Traj &T = traj_[b];
      ++segments_run[b];
      if (T.seg_code == ExitCode::kOptimal) { T.last_code = ExitCode::kOptimal; T.last_solution = T.seg_solution; }
      if (s + 1 < SEGMENTS && stages_[(size_t)s + 1].waypoints >= 4) {
        Stage &nx = stages_[(size_t)s + 1];
        { std::lock_guard<std::mutex> lk(nx.mu); nx.inbox.push_back(b); }
        nx.cv.notify_one();
      } else if (finished_.fetch_add(1) + 1 >= B) wakeAll();
    }
  }

  template <class F>
  static void parallelFor(size_t count, F &&body) {
    const size_t nt = std::min<size_t>({count / 8, 8, std::max(1u, std::thread::hardware_concurrency())});
    if (nt <= 1) { for (size_t k = 0; k < count; ++k) body(k); return; }
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; ++t) th.emplace_back([&, t] { for (size_t k = t; k < count; k += nt) body(k); });
    for (auto &x : th) x.join();
  }

  // initConstraints of GOMPSolver ([REF] src/gomp-solver.h:98-110) without its last call (the obstacle rows), normalised
  ConstraintBuilder<N_DIM> jointSpaceTemplate(const Ctrl<N_DIM> &start_pos, const Ctrl<N_DIM> &end_pos, size_t waypoints) const {
    ConstraintBuilder<N_DIM> b{waypoints, mappers, obstacles, capsules, cuboids, pairs, tilts, grids, goalsAt(waypoints)};
    b.position(0, constraints::equal<N_DIM>(start_pos))
        .positions(1, waypoints - 2, pos_con)
        .position(waypoints - 3, targets_ ? pos_con : constraints::equal<N_DIM>(end_pos))
        .velocities(0, waypoints - 4, vel_con)
        .velocity(waypoints - 3, constraints::eqZero<N_DIM>())
        .accelerations(0, waypoints - 4, acc_con)
        .acceleration(waypoints - 3, constraints::eqZero<N_DIM>())
        .normalised();
    return b;
  }

  bool isSolutionOK(const QPVector &q_trajectory, size_t b) const {
    bool res = true;
    if (targets_) {                                               // the goal of trajectory b at the third-last waypoint
      std::vector<GraspGoal> gs = goalsAt(q_trajectory.size() / 2 / N_DIM);
      gs[0].target = (*targets_)[b];
      if (!goalsOKAlong<N_DIM>(gs, mappers, q_trajectory)) res = false;
    }
    for (const RobotBall &ball : mappers) {
      const QPVector xyz = mapJointTrajectoryToXYZ<N_DIM>(q_trajectory, ball.fk);
      const int waypoints = (int)xyz.size() / 3;
      for (int w = 0; w < waypoints; ++w) {
        const Point p{xyz[3 * w], xyz[3 * w + 1], xyz[3 * w + 2]};
        if (ball.is_gripper) {
          for (Axis axis : XYZ_AXES) {
            const double lo = con_3d.first ? (*con_3d.first)[axis] : -INF;
            const double up = con_3d.second ? (*con_3d.second)[axis] : INF;
            if (!(lo - ERROR <= p[axis] - ball.radius && p[axis] + ball.radius <= up + ERROR)) res = false;
          }
        }
        for (const HorizontalLine &line : obstacles)
          if (line.hasCollision(w, xyz, ball) && !line.isAbove(p, ball)) res = false;
        if (!capsulesClear(capsules, p, ball)) res = false;
        if (!cuboidsClear(cuboids, p, ball)) res = false;
        if (!gridsClear(grids, p, ball)) res = false;
      }
    }
    if (!pairsClearAlong<N_DIM>(pairs, mappers, q_trajectory)) res = false;
    if (!tiltsOKAlong<N_DIM>(tilts, q_trajectory)) res = false;
    return res;
  }
};

}  // namespace miosqp_ref
