// examples/cuboid_gomp_example.cpp -- what a picking cell is made of: the 7-joint arm of chain_gomp_example.cpp reaches over the
// rim of a bin and down into it.
//
// A CuboidObstacle is an oriented box - a centre, three orthonormal axes, three half extents (zero allowed: a plate) and an
// optional rounding radius: bin walls and floors, table tops, shelves, a camera post with a square section.  Every collision
// ball of the arm gets one constraint row per cuboid and waypoint: outside the box the ball is pushed along the unit vector
// from the closest point of a face, an edge or a corner; a ball whose centre is inside (a warm start that cuts a corner of
// the bin) leaves through the nearest face.  The row starts to constrain `margin` away from the surface - the tool against
// cutting through a wall between two waypoints - and a trajectory is accepted when no ball is deeper than 1 mm in any cuboid.
// The planner takes them in `cuboids`; with device_assembly the rows are written by the GPU (mi_gomp_scene_create_cuboids).
// The bin here is five cuboids: a floor and four walls.
//
//   usage: cuboid_gomp_example [trajectories = 8] [waypoints = 40] [SQP step on the device: 0|1 = 1]
#include <algorithm>
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
  if (n_traj < 1 || waypoints < 10) { std::fprintf(stderr, "usage: cuboid_gomp_example [trajectories] [waypoints >= 10] [0|1]\n"); return 2; }

  const double pi = 3.14159265358979323846, H = pi / 2;
  mi_gomp_chain arm{};
  arm.n_joints = (int)kJoints;
  const double a[kJoints] = {0, 0, 0.0825, -0.0825, 0, 0.088, 0}, d[kJoints] = {0.333, 0, 0.316, 0, 0.384, 0, 0.107};
  const double alpha[kJoints] = {-H, H, H, -H, H, H, 0.3}, theta0[kJoints] = {0, 0, 0, 0.25, 0, 0, -0.7};
  for (size_t i = 0; i < kJoints; ++i) { arm.a[i] = a[i]; arm.d[i] = d[i]; arm.alpha[i] = alpha[i]; arm.theta0[i] = theta0[i]; }

  std::vector<ref::RobotBall> balls{ref::dhBall(arm, 3, {0, 0.05, -0.1}, 0.08),  ref::dhBall(arm, 4, {0.02, 0, 0.03}, 0.07),
                                    ref::dhBall(arm, 5, {0, 0.04, -0.15}, 0.07), ref::dhBall(arm, 6, {0.03, 0, 0}, 0.06),
                                    ref::dhBall(arm, 7, {0.02, -0.01, 0.06}, 0.04, true)};
  // the bin: 0.30 x 0.30 inside around (0.62, 0.37), its floor's top at z = 0.08, its rim at z = 0.24, walls 0.02 thick.
  // (centre, half extents, rounding radius, margin); CuboidObstacle::oriented takes the axes as well
  const double cx = 0.62, cy = 0.37, in = 0.15, t = 0.01, z0 = 0.08, z1 = 0.24, margin = 0.03;
  std::vector<ref::CuboidObstacle> bin{
      ref::CuboidObstacle({cx, cy, z0 - t}, {in + 2 * t, in + 2 * t, t}, 0.0, margin),                              // floor
      ref::CuboidObstacle({cx - in - t, cy, (z0 + z1) / 2}, {t, in + 2 * t, (z1 - z0) / 2}, 0.0, margin),          // walls across x
      ref::CuboidObstacle({cx + in + t, cy, (z0 + z1) / 2}, {t, in + 2 * t, (z1 - z0) / 2}, 0.0, margin),
      ref::CuboidObstacle({cx, cy - in - t, (z0 + z1) / 2}, {in, t, (z1 - z0) / 2}, 0.0, margin),                  // walls across y
      ref::CuboidObstacle({cx, cy + in + t, (z0 + z1) / 2}, {in, t, (z1 - z0) / 2}, 0.0, margin)};
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

  ref::ContinuousGOMPSolver<kJoints> planner(waypoints, 0.1, joint_limits, speed_limits, accel_limits, work_space, {}, balls);
  planner.cuboids = bin;
  planner.device_assembly = on_device;
  planner.dh_chain = arm;
  auto plans = planner.run(from, to);

  int ok = 0;
  for (int k = 0; k < n_traj; ++k) {
    const auto &[code, x] = plans[(size_t)k];
    double clearance = ref::INF;                         // over all balls, waypoints and cuboids
    const size_t W = x.size() / 2 / kJoints;
    for (const ref::RobotBall &ball : balls)
      for (size_t w = 0; w < W; ++w) {
        double q[kJoints];
        std::copy(x.begin() + (long)(w * kJoints), x.begin() + (long)((w + 1) * kJoints), q);
        auto [px, py, pz] = ball.fk(q);
        for (const ref::CuboidObstacle &c : bin) clearance = std::min(clearance, c.clearance({px, py, pz}, ball));
      }
    std::printf("trajectory %d: %s, %d re-linearisations, minimum clearance %.4f m over %zu waypoints\n", k, ref::ToString(code).c_str(),
                planner.qp_updates[(size_t)k], clearance, W);
    ok += code == ref::ExitCode::kOptimal && clearance >= -1e-3;
  }
  std::printf("%d of %d trajectories planned into the bin, clear of its walls and floor (SQP step on the %s)\n", ok, n_traj, on_device ? "device" : "host threads");
  return ok == n_traj ? 0 : 1;
}
