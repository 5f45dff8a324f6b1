// examples/tilt_gomp_example.cpp -- keep the tool upright: the 7-joint arm of chain_gomp_example.cpp moves between two
// postures with the tool axis vertical at both ends; the straight joint-space line between them tips the tool 39 degrees over.
//
// A TiltLimit names a unit vector fixed in a link of the arm, a unit world vector and the largest angle between the two.
// Every (limit, waypoint) gets one constraint row, the linearisation of cos(tilt) >= cos(max_angle) in the joints; it starts
// to constrain `margin` radians inside the cone, and a trajectory is accepted when no waypoint is more than 1 mrad outside it.
// dhTilt() makes one for a vector fixed in a link frame of a DH chain.  The planner takes them in `tilts`; with
// device_assembly the rows are written by the GPU (mi_gomp_scene_create_tilts).  The same problems are planned without and
// with a limit of 15 degrees.  (Start inside the cone: where the axis is exactly opposite to the reference the row is all
// zeros and the QP infeasible.  The step is a plain SQP step: a start far outside the cone may not converge.)
//
//   usage: tilt_gomp_example [trajectories = 8] [waypoints = 40] [SQP step on the device: 0|1 = 1]
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
  if (n_traj < 1 || waypoints < 10) { std::fprintf(stderr, "usage: tilt_gomp_example [trajectories] [waypoints >= 10] [0|1]\n"); return 2; }

  const double pi = 3.14159265358979323846, H = pi / 2, deg = pi / 180;
  mi_gomp_chain arm{};
  arm.n_joints = (int)kJoints;
  const double a[kJoints] = {0, 0, 0.0825, -0.0825, 0, 0.088, 0}, d[kJoints] = {0.333, 0, 0.316, 0, 0.384, 0, 0.107};
  const double alpha[kJoints] = {-H, H, H, -H, H, H, 0.3}, theta0[kJoints] = {0, 0, 0, 0.25, 0, 0, -0.7};
  for (size_t i = 0; i < kJoints; ++i) { arm.a[i] = a[i]; arm.d[i] = d[i]; arm.alpha[i] = alpha[i]; arm.theta0[i] = theta0[i]; }

  std::vector<ref::RobotBall> balls{ref::dhBall(arm, 2, {0, 0, 0}, 0.09),        ref::dhBall(arm, 3, {0, 0.05, -0.1}, 0.08),
                                    ref::dhBall(arm, 4, {0.02, 0, 0.03}, 0.07),  ref::dhBall(arm, 5, {0, 0.04, -0.15}, 0.07),
                                    ref::dhBall(arm, 6, {0.03, 0, 0}, 0.06),     ref::dhBall(arm, 7, {0, 0, -0.05}, 0.05),
                                    ref::dhBall(arm, 7, {0.02, -0.01, 0.06}, 0.04, true)};
  // the tool axis is the z axis of the last frame and points down: within 15 degrees of -z, the row active from 5 degrees inside
  const ref::TiltLimit upright = ref::dhTilt(arm, 7, {0, 0, 1}, {0, 0, -1}, 15 * deg, 5 * deg);
  auto joint_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-2 * pi), ref::constraints::of<kJoints>(2 * pi));
  auto speed_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-pi), ref::constraints::of<kJoints>(pi));
  auto accel_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-pi * 800 / 180), ref::constraints::of<kJoints>(pi * 800 / 180));
  auto work_space = ref::constraints::any<3>();

  // the tool is within 0.2 degrees of vertical at both postures
  const double A[kJoints] = {-0.273, 0.728, -0.584, -1.6, 0.101, 1.877, 1.025}, B[kJoints] = {-1.283, 1.929, -2.018, -2.923, 1.301, 1.35, -0.775};
  std::vector<ref::Ctrl<kJoints>> from, to;
  for (int k = 0; k < n_traj; ++k) {
    ref::Ctrl<kJoints> s{}, e{};
    for (size_t j = 0; j < kJoints; ++j) { s[j] = A[j] + 0.004 * (k % 4) * ((int)(j % 3) - 1); e[j] = B[j] - 0.004 * (k % 4) * ((j % 2) ? 1 : -1); }
    from.push_back(s); to.push_back(e);
  }

  auto largest_tilt = [&](const ref::QPVector &x) {             // degrees, over all waypoints
    double worst = 0.0;
    for (size_t w = 0; w < x.size() / 2 / kJoints; ++w)
      worst = std::max(worst, std::acos(std::max(-1.0, std::min(1.0, ref::tiltCosine<kJoints>(upright, x.data() + w * kJoints)))));
    return worst / deg;
  };

  ref::ContinuousGOMPSolver<kJoints> planner(waypoints, 0.1, joint_limits, speed_limits, accel_limits, work_space, {}, balls);
  planner.device_assembly = on_device;
  planner.dh_chain = arm;
  int ok[2] = {0, 0};
  double worst[2] = {0.0, 0.0};
  const double allowed = (upright.max_angle + 1e-3) / deg;
  for (int with = 0; with < 2; ++with) {
    planner.tilts = with ? std::vector<ref::TiltLimit>{upright} : std::vector<ref::TiltLimit>{};
    auto plans = planner.run(from, to);
    for (int k = 0; k < n_traj; ++k) {
      const auto &[code, x] = plans[(size_t)k];
      const double tilt = largest_tilt(x);
      std::printf("trajectory %d %s the limit: %s, %d re-linearisations, largest tilt %.3f deg over %zu waypoints\n", k, with ? "with" : "without",
                  ref::ToString(code).c_str(), planner.qp_updates[(size_t)k], tilt, x.size() / 2 / kJoints);
      ok[with] += code == ref::ExitCode::kOptimal && (!with || tilt <= allowed);
      worst[with] = std::max(worst[with], tilt);
    }
  }
  std::printf("%d of %d trajectories planned without the limit, largest tilt without the limit %.3f deg: the tool tips over\n", ok[0], n_traj, worst[0]);
  std::printf("%d of %d trajectories planned with the limit, largest tilt with the limit %.3f deg (limit %.1f deg, SQP step on the %s)\n", ok[1], n_traj, worst[1],
              upright.max_angle / deg, on_device ? "device" : "host threads");
  return ok[0] == n_traj && ok[1] == n_traj && worst[0] > allowed ? 0 : 1;
}
