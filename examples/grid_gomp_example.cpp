// examples/grid_gomp_example.cpp -- a world that was measured, not described: the bin of cuboid_gomp_example.cpp as a distance grid.
//
// A depth camera does not deliver cuboids; it delivers a voxel grid of distances to the nearest surface.  A DistanceGrid is
// such a grid: n[0] x n[1] x n[2] nodes of one spacing, axis-aligned in the world, each holding a distance - positive in free
// space, negative inside material, possibly truncated.  Every collision ball of the arm gets one constraint row per grid and
// waypoint: the trilinear interpolant of the nodes around the ball's centre and its exact gradient in that cell, not
// normalised, times the ball's Jacobian.  Outside the box of the nodes the grid says nothing.  The row starts to constrain
// `margin` away from the surface, `offset` inflates the obstacles, and a trajectory is accepted when no ball is deeper than
// 1 mm in the interpolant.  The planner takes grids in `grids`; with device_assembly the rows are written by the GPU
// (mi_gomp_scene_create_grids), and updateGrid(k, values) hands every kept device scene a new camera frame.
//
// Here the grid is sampled from the bin's five cuboids (DistanceGrid::fromObstacles) - a distance transform of a depth image
// takes its place in a real cell.  The arm is planned once with the cuboids and once with the grid alone.
//
//   usage: grid_gomp_example [trajectories = 8] [waypoints = 40] [SQP step on the device: 0|1 = 1]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mi_osqp/dh_kinematics.hpp"
#include "mi_osqp/gomp.hpp"

namespace ref = miosqp_ref;
constexpr size_t kJoints = 7;

int main(int argc, char **argv) {
  setenv("GPU_MAX_HW_QUEUES", "10", 0);                 // one hardware queue per horizon stage
  const int n_traj = argc > 1 ? std::atoi(argv[1]) : 8;
  const size_t waypoints = argc > 2 ? (size_t)std::atoi(argv[2]) : 40;
  const bool on_device = argc > 3 ? std::atoi(argv[3]) != 0 : true;
  if (n_traj < 1 || waypoints < 10) { std::fprintf(stderr, "usage: grid_gomp_example [trajectories] [waypoints >= 10] [0|1]\n"); return 2; }

  const double pi = 3.14159265358979323846, H = pi / 2;
  mi_gomp_chain arm{};
  arm.n_joints = (int)kJoints;
  const double a[kJoints] = {0, 0, 0.0825, -0.0825, 0, 0.088, 0}, d[kJoints] = {0.333, 0, 0.316, 0, 0.384, 0, 0.107};
  const double alpha[kJoints] = {-H, H, H, -H, H, H, 0.3}, theta0[kJoints] = {0, 0, 0, 0.25, 0, 0, -0.7};
  for (size_t i = 0; i < kJoints; ++i) { arm.a[i] = a[i]; arm.d[i] = d[i]; arm.alpha[i] = alpha[i]; arm.theta0[i] = theta0[i]; }

  std::vector<ref::RobotBall> balls{ref::dhBall(arm, 3, {0, 0.05, -0.1}, 0.08),  ref::dhBall(arm, 4, {0.02, 0, 0.03}, 0.07),
                                    ref::dhBall(arm, 5, {0, 0.04, -0.15}, 0.07), ref::dhBall(arm, 6, {0.03, 0, 0}, 0.06),
                                    ref::dhBall(arm, 7, {0.02, -0.01, 0.06}, 0.04, true)};
  // the bin of cuboid_gomp_example.cpp: a floor and four walls
  const double cx = 0.62, cy = 0.37, in = 0.15, t = 0.01, z0 = 0.08, z1 = 0.24, margin = 0.03;
  std::vector<ref::CuboidObstacle> bin{
      ref::CuboidObstacle({cx, cy, z0 - t}, {in + 2 * t, in + 2 * t, t}, 0.0, margin),
      ref::CuboidObstacle({cx - in - t, cy, (z0 + z1) / 2}, {t, in + 2 * t, (z1 - z0) / 2}, 0.0, margin),
      ref::CuboidObstacle({cx + in + t, cy, (z0 + z1) / 2}, {t, in + 2 * t, (z1 - z0) / 2}, 0.0, margin),
      ref::CuboidObstacle({cx, cy - in - t, (z0 + z1) / 2}, {in, t, (z1 - z0) / 2}, 0.0, margin),
      ref::CuboidObstacle({cx, cy + in + t, (z0 + z1) / 2}, {in, t, (z1 - z0) / 2}, 0.0, margin)};
  // ... sampled every centimetre in a box 0.3 m around it (origin, cell, n, capsules, cuboids, offset, margin)
  const double cell = 0.01, around = 0.3;
  const std::array<int, 3> n{(int)std::lround((2 * (in + 2 * t) + 2 * around) / cell) + 1, (int)std::lround((2 * (in + 2 * t) + 2 * around) / cell) + 1,
                             (int)std::lround((z1 - (z0 - 2 * t) + 2 * around - 0.2) / cell) + 1};
  const ref::DistanceGrid sensed =
      ref::DistanceGrid::fromObstacles({cx - in - 2 * t - around, cy - in - 2 * t - around, z0 - 2 * t - (around - 0.2)}, cell, n, {}, bin, 0.0, margin);
  std::printf("the bin as a grid: %d x %d x %d nodes of %.0f mm\n", n[0], n[1], n[2], cell * 1e3);

  auto joint_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-2 * pi), ref::constraints::of<kJoints>(2 * pi));
  auto speed_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-pi), ref::constraints::of<kJoints>(pi));
  auto accel_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-pi * 800 / 180), ref::constraints::of<kJoints>(pi * 800 / 180));
  auto work_space = ref::constraints::inRange<3>(ref::Vec<3>{-ref::INF, -ref::INF, 0.1}, ref::Vec<3>{0.8, ref::INF, ref::INF});

  const double base[kJoints] = {0, 0.4, 0, -1.6, 0, 1.9, 0.6};
  std::vector<ref::Ctrl<kJoints>> from, to;
  for (int k = 0; k < n_traj; ++k) {
    ref::Ctrl<kJoints> s{}, e{};
    for (size_t j = 0; j < kJoints; ++j) { s[j] = base[j] + 0.02 * ((k + (int)j) % 3 - 1); e[j] = base[j] - 0.02 * ((k + 2 * (int)j) % 3 - 1); }
    s[0] = -0.5 + 0.1 * (k % 4); e[0] = 0.5 + 0.03 * (k % 4);          // from beside the bin ...
    e[1] = 0.8 - 0.03 * (k % 4);                                       // ... over the rim and down into it
    from.push_back(s); to.push_back(e);
  }

  // the true clearance from the bin's cuboids, whatever the planner saw
  auto clearance_of = [&](const ref::QPVector &x) {
    double clearance = ref::INF;
    const size_t W = x.size() / 2 / kJoints;
    for (const ref::RobotBall &ball : balls)
      for (size_t w = 0; w < W; ++w) {
        double q[kJoints];
        std::copy(x.begin() + (long)(w * kJoints), x.begin() + (long)((w + 1) * kJoints), q);
        auto [px, py, pz] = ball.fk(q);
        for (const ref::CuboidObstacle &c : bin) clearance = std::min(clearance, c.clearance({px, py, pz}, ball));
      }
    return clearance;
  };

  std::vector<std::vector<std::pair<ref::ExitCode, ref::QPVector>>> plans;
  int planned[2] = {0, 0};
  for (int with_grid = 0; with_grid < 2; ++with_grid) {
    ref::ContinuousGOMPSolver<kJoints> planner(waypoints, 0.1, joint_limits, speed_limits, accel_limits, work_space, {}, balls);
    if (with_grid) planner.grids = {sensed}; else planner.cuboids = bin;
    planner.device_assembly = on_device;
    planner.dh_chain = arm;
    plans.push_back(planner.run(from, to));
    for (int k = 0; k < n_traj; ++k) {
      const auto &[code, x] = plans.back()[(size_t)k];
      const double clearance = clearance_of(x);
      std::printf("%s, trajectory %d: %s, %d re-linearisations, minimum clearance from the bin %.4f m\n", with_grid ? "grid" : "cuboids", k,
                  ref::ToString(code).c_str(), planner.qp_updates[(size_t)k], clearance);
      planned[with_grid] += code == ref::ExitCode::kOptimal && clearance >= -1e-3 - cell / 2;      // (the interpolant rounds edges off by a fraction of a cell)
    }
  }
  double diff = 0.0;
  for (int k = 0; k < n_traj; ++k) {
    const ref::QPVector &xa = plans[0][(size_t)k].second, &xb = plans[1][(size_t)k].second;
    for (size_t i = 0; i < std::min(xa.size(), xb.size()) / 2; ++i) diff = std::max(diff, std::fabs(xa[i] - xb[i]));
  }
  std::printf("%d of %d trajectories planned with the cuboids, %d of %d trajectories planned with the grid alone (SQP step on the %s)\n", planned[0], n_traj,
              planned[1], n_traj, on_device ? "device" : "host threads");
  std::printf("largest difference between the two plans %.3e rad\n", diff);
  return planned[0] == n_traj && planned[1] == n_traj ? 0 : 1;
}
