// examples/grasp_gomp_example.cpp -- where to arrive, said in task space: the 7-joint arm of chain_gomp_example.cpp reaches into
// the bin of cuboid_gomp_example.cpp with its tool axis pointing down.
//
// A planner's end condition used to be one joint vector.  A suction cup on a box does not care how the wrist is turned about
// its own axis, and a pick has a tolerance: a GraspGoal says so.  Its structure names a collision ball (here the gripper ball)
// and, optionally, an axis fixed in a link (dhGoal: the z axis of the last frame, the tool axis); a GoalTarget says what one
// trajectory asks: the point the ball's centre has to reach, half widths per world axis (0: exactly, GOAL_FREE: anywhere), a
// world direction and the largest angle the axis may make with it.  The planner turns that into four constraint rows at the
// third-last waypoint of every horizon and chooses the joints itself; the joint vector it is given - from any IK - only seeds
// the warm start.  Seed on the right side: joints whose tool axis points away from the direction asked for give the solver a
// row it cannot satisfy.  With device_assembly the rows are written by the GPU (mi_gomp_scene_create_goals, the targets with
// mi_gomp_scene_set_goal_values).
//
// The arm plans twice from the same start: to the seed joints as a fixed goal, and to the grasp goal seeded with them.  The
// program prints both costs (the sum of squared velocity steps the QPs minimise) and how far the planner turned the tool about
// its own axis, which the goal leaves free.
//
//   usage: grasp_gomp_example [waypoints = 40] [SQP step on the device: 0|1 = 1]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mi_osqp/dh_kinematics.hpp"
#include "mi_osqp/gomp.hpp"

namespace ref = miosqp_ref;
constexpr size_t kJoints = 7;

// the sum of squared velocity steps of a plan, per time step: what the QPs minimise
static double cost(const ref::QPVector &x, double time_step) {
  const size_t W = x.size() / 2 / kJoints;
  double c = 0.0;
  for (size_t j = 0; j < kJoints; ++j) {
    double prev = 0.0;
    for (size_t w = 0; w < W; ++w) {
      const double v = x[W * kJoints + w * kJoints + j] * time_step;
      c += (v - prev) * (v - prev);
      prev = v;
    }
    c += prev * prev;
  }
  return c;
}

int main(int argc, char **argv) {
  setenv("GPU_MAX_HW_QUEUES", "10", 0);                 // one hardware queue per horizon stage
  const size_t waypoints = argc > 1 ? (size_t)std::atoi(argv[1]) : 40;
  const bool on_device = argc > 2 ? std::atoi(argv[2]) != 0 : true;
  if (waypoints < 10) { std::fprintf(stderr, "usage: grasp_gomp_example [waypoints >= 10] [0|1]\n"); return 2; }

  const double pi = 3.14159265358979323846, H = pi / 2;
  mi_gomp_chain arm{};
  arm.n_joints = (int)kJoints;
  const double a[kJoints] = {0, 0, 0.0825, -0.0825, 0, 0.088, 0}, d[kJoints] = {0.333, 0, 0.316, 0, 0.384, 0, 0.107};
  const double alpha[kJoints] = {-H, H, H, -H, H, H, 0.3}, theta0[kJoints] = {0, 0, 0, 0.25, 0, 0, -0.7};
  for (size_t i = 0; i < kJoints; ++i) { arm.a[i] = a[i]; arm.d[i] = d[i]; arm.alpha[i] = alpha[i]; arm.theta0[i] = theta0[i]; }

  std::vector<ref::RobotBall> balls{ref::dhBall(arm, 3, {0, 0.05, -0.1}, 0.08),  ref::dhBall(arm, 4, {0.02, 0, 0.03}, 0.07),
                                    ref::dhBall(arm, 5, {0, 0.04, -0.15}, 0.07), ref::dhBall(arm, 6, {0.03, 0, 0}, 0.06),
                                    ref::dhBall(arm, 7, {0.02, -0.01, 0.06}, 0.04, true)};
  const size_t gripper = 4;
  // the grasp posture an IK gave: the tool axis (z of frame 7) within a fifth of a degree of straight down
  const ref::Ctrl<kJoints> start{-1.0, 0.4, 0.0, -1.6, 0.0, 1.9, 0.6}, seed{-0.273, 0.728, -0.584, -1.6, 0.101, 1.877, 1.025};
  ref::Ctrl<kJoints> seed_q = seed;
  const auto [gx, gy, gz] = balls[gripper].fk(seed_q.data());

  // the bin of cuboid_gomp_example.cpp under the grasp point: 0.30 x 0.30 inside, walls 0.02 thick, here 0.10 deep (the forearm
  // passes over its rim); the gripper ball (radius 0.04) ends 0.08 above the floor
  const double cx = gx, cy = gy, in = 0.15, t = 0.01, z0 = gz - 0.08, z1 = z0 + 0.10, margin = 0.03;
  std::vector<ref::CuboidObstacle> bin{
      ref::CuboidObstacle({cx, cy, z0 - t}, {in + 2 * t, in + 2 * t, t}, 0.0, margin),                              // floor
      ref::CuboidObstacle({cx - in - t, cy, (z0 + z1) / 2}, {t, in + 2 * t, (z1 - z0) / 2}, 0.0, margin),          // walls across x
      ref::CuboidObstacle({cx + in + t, cy, (z0 + z1) / 2}, {t, in + 2 * t, (z1 - z0) / 2}, 0.0, margin),
      ref::CuboidObstacle({cx, cy - in - t, (z0 + z1) / 2}, {in, t, (z1 - z0) / 2}, 0.0, margin),                  // walls across y
      ref::CuboidObstacle({cx, cy + in + t, (z0 + z1) / 2}, {in, t, (z1 - z0) / 2}, 0.0, margin)};
  auto joint_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-2 * pi), ref::constraints::of<kJoints>(2 * pi));
  auto speed_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-pi), ref::constraints::of<kJoints>(pi));
  auto accel_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-pi * 800 / 180), ref::constraints::of<kJoints>(pi * 800 / 180));

  // the goal: the gripper ball within 20 mm sideways and 5 mm in height of where the seed puts it, the tool axis within
  // 5 degrees of straight down; how the wrist is turned about that axis is the planner's to choose
  ref::GoalTarget target;
  target.point = {gx, gy, gz};
  target.tol = {0.02, 0.02, 0.005};
  target.ref = {0.0, 0.0, -1.0};
  target.max_angle = 5 * pi / 180;

  ref::ContinuousGOMPSolver<kJoints> planner(waypoints, 0.1, joint_limits, speed_limits, accel_limits, ref::constraints::any<3>(), {}, balls);
  planner.cuboids = bin;
  planner.device_assembly = on_device;
  planner.dh_chain = arm;
  planner.goal = ref::dhGoal(arm, gripper, 7, {0, 0, 1});

  const auto fixed = planner.run({start}, {seed})[0];
  const int fixed_updates = planner.qp_updates[0];
  const auto grasp = planner.run({start}, {seed}, {target})[0];
  const int grasp_updates = planner.qp_updates[0];

  int ok = 0;
  if (fixed.first == ref::ExitCode::kOptimal) {
    ++ok;
    std::printf("planned to the fixed joint goal: %zu waypoints, %d re-linearisations\n", fixed.second.size() / 2 / kJoints, fixed_updates);
    std::printf("cost to the fixed joint goal %.6f\n", cost(fixed.second, 0.1));
  }
  if (grasp.first == ref::ExitCode::kOptimal) {
    const ref::QPVector &x = grasp.second;
    const size_t W = x.size() / 2 / kJoints, we = W - 3;
    ref::GraspGoal g = *planner.goal;
    g.waypoint = we; g.target = target;
    double q[kJoints];
    std::copy(x.begin() + (long)(we * kJoints), x.begin() + (long)((we + 1) * kJoints), q);
    const auto [px, py, pz] = balls[gripper].fk(q);
    const double angle = std::acos(std::fmax(-1.0, std::fmin(1.0, ref::goalCosine<kJoints>(g, q))));
    // the turn about the tool axis: the tool's x axis at the seed and at the chosen end point, seen along the seed's tool axis
    const double ex[3] = {1, 0, 0}, ez[3] = {0, 0, 1};
    double xs[3], xe[3], zs[3];
    mi_osqp::dh::axis(arm, seed.data(), 7, ex, xs, nullptr);
    mi_osqp::dh::axis(arm, seed.data(), 7, ez, zs, nullptr);
    mi_osqp::dh::axis(arm, q, 7, ex, xe, nullptr);
    const double cr[3] = {xs[1] * xe[2] - xs[2] * xe[1], xs[2] * xe[0] - xs[0] * xe[2], xs[0] * xe[1] - xs[1] * xe[0]};
    const double turn = std::atan2(cr[0] * zs[0] + cr[1] * zs[1] + cr[2] * zs[2], xs[0] * xe[0] + xs[1] * xe[1] + xs[2] * xe[2]);
    const bool inside = ref::goalOK<kJoints>(g, balls, q);
    ok += inside;
    std::printf("planned to the grasp goal: %zu waypoints, %d re-linearisations; the gripper ends (%.1f, %.1f, %.1f) mm from the target point, the tool axis %.2f degrees"
                " from straight down: %s the goal\n", W, grasp_updates, 1e3 * (px - gx), 1e3 * (py - gy), 1e3 * (pz - gz), angle * 180 / pi, inside ? "inside" : "OUTSIDE");
    std::printf("cost to the grasp goal %.6f\n", cost(x, 0.1));
    std::printf("turn about the tool axis chosen by the planner %.4f rad\n", turn);
  }
  std::printf("%d of 2 plans found (SQP step on the %s)\n", ok, on_device ? "device" : "host threads");
  return ok == 2 ? 0 : 1;
}
