// examples/selfcollision_gomp_example.cpp -- the arm must not hit itself: the 7-joint arm of chain_gomp_example.cpp moves
// between two postures whose straight joint-space line folds the forearm through the shoulder.
//
// A BallPair names two of the planner's collision balls and a margin.  Every (pair, waypoint) gets one constraint row, the
// linearisation of |p_a - p_b| - (r_a + r_b) >= 0 in the joints; it starts to constrain `margin` away from contact, and a
// trajectory is accepted when no pair is deeper than 1 mm in each other.  dhSelfPairs() makes the usual list for an arm whose
// balls sit in the link frames of a DH chain: every two balls whose frames are at least two apart ("skip adjacent links").
// The planner takes them in `pairs`; with device_assembly the rows are written by the GPU (mi_gomp_scene_create_pairs).
// The same problems are planned without and with pairs: without them the result goes through the arm.
//
//   usage: selfcollision_gomp_example [trajectories = 8] [waypoints = 40] [SQP step on the device: 0|1 = 1]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <tuple>
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
  if (n_traj < 1 || waypoints < 10) { std::fprintf(stderr, "usage: selfcollision_gomp_example [trajectories] [waypoints >= 10] [0|1]\n"); return 2; }

  const double pi = 3.14159265358979323846, H = pi / 2;
  mi_gomp_chain arm{};
  arm.n_joints = (int)kJoints;
  const double a[kJoints] = {0, 0, 0.0825, -0.0825, 0, 0.088, 0}, d[kJoints] = {0.333, 0, 0.316, 0, 0.384, 0, 0.107};
  const double alpha[kJoints] = {-H, H, H, -H, H, H, 0.3}, theta0[kJoints] = {0, 0, 0, 0.25, 0, 0, -0.7};
  for (size_t i = 0; i < kJoints; ++i) { arm.a[i] = a[i]; arm.d[i] = d[i]; arm.alpha[i] = alpha[i]; arm.theta0[i] = theta0[i]; }

  // a ball per link frame 2 .. 7, as a real collision model places them, and the gripper's
  std::vector<ref::RobotBall> balls{ref::dhBall(arm, 2, {0, 0, 0}, 0.09),        ref::dhBall(arm, 3, {0, 0.05, -0.1}, 0.08),
                                    ref::dhBall(arm, 4, {0.02, 0, 0.03}, 0.07),  ref::dhBall(arm, 5, {0, 0.04, -0.15}, 0.07),
                                    ref::dhBall(arm, 6, {0.03, 0, 0}, 0.06),     ref::dhBall(arm, 7, {0, 0, -0.05}, 0.05),
                                    ref::dhBall(arm, 7, {0.02, -0.01, 0.06}, 0.04, true)};
  // every two balls whose frames are at least 2 apart, active from 3 cm: 14 pairs
  const std::vector<ref::BallPair> self = ref::dhSelfPairs(balls, 2, 0.03);
  auto joint_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-2 * pi), ref::constraints::of<kJoints>(2 * pi));
  auto speed_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-pi), ref::constraints::of<kJoints>(pi));
  auto accel_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-pi * 800 / 180), ref::constraints::of<kJoints>(pi * 800 / 180));
  auto work_space = ref::constraints::any<3>();

  // both postures keep every pair 5 cm apart or more; half way along the straight line between them the wrist is 13 cm deep
  // in the shoulder
  const double A[kJoints] = {-1.096, -0.205, -0.756, 1.077, 0.129, -2.249, -2.505}, B[kJoints] = {-0.746, -0.553, -0.574, 2.791, 0.213, -2.254, -2.375};
  std::vector<ref::Ctrl<kJoints>> from, to;
  for (int k = 0; k < n_traj; ++k) {
    ref::Ctrl<kJoints> s{}, e{};
    for (size_t j = 0; j < kJoints; ++j) { s[j] = A[j] + 0.01 * (k % 4) * ((int)(j % 3) - 1); e[j] = B[j] - 0.01 * (k % 4) * ((j % 2) ? 1 : -1); }
    from.push_back(s); to.push_back(e);
  }

  auto min_pair_clearance = [&](const ref::QPVector &x) {       // over all pairs and waypoints
    double clearance = ref::INF;
    std::vector<double> xyz(3 * balls.size());
    for (size_t w = 0; w < x.size() / 2 / kJoints; ++w) {
      double q[kJoints];
      std::copy(x.begin() + (long)(w * kJoints), x.begin() + (long)((w + 1) * kJoints), q);
      for (size_t i = 0; i < balls.size(); ++i) std::tie(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]) = balls[i].fk(q);
      for (const ref::BallPair &p : self) clearance = std::min(clearance, ref::pairClearance(p, xyz, balls));
    }
    return clearance;
  };

  ref::ContinuousGOMPSolver<kJoints> planner(waypoints, 0.1, joint_limits, speed_limits, accel_limits, work_space, {}, balls);
  planner.device_assembly = on_device;
  planner.dh_chain = arm;
  int ok[2] = {0, 0};
  double worst[2] = {ref::INF, ref::INF};
  for (int with = 0; with < 2; ++with) {
    planner.pairs = with ? self : std::vector<ref::BallPair>{};
    auto plans = planner.run(from, to);
    for (int k = 0; k < n_traj; ++k) {
      const auto &[code, x] = plans[(size_t)k];
      const double clearance = min_pair_clearance(x);
      std::printf("trajectory %d %s pairs: %s, %d re-linearisations, minimum pair clearance %.4f m over %zu waypoints\n", k, with ? "with" : "without",
                  ref::ToString(code).c_str(), planner.qp_updates[(size_t)k], clearance, x.size() / 2 / kJoints);
      ok[with] += code == ref::ExitCode::kOptimal && (!with || clearance >= -1e-3);
      worst[with] = std::min(worst[with], clearance);
    }
  }
  std::printf("%d of %d trajectories planned without pairs, minimum pair clearance without pairs %.4f m: the arm goes through itself\n", ok[0], n_traj, worst[0]);
  std::printf("%d of %d trajectories planned with pairs, minimum pair clearance with pairs %.4f m (%zu pairs, SQP step on the %s)\n", ok[1], n_traj, worst[1],
              self.size(), on_device ? "device" : "host threads");
  return ok[0] == n_traj && ok[1] == n_traj && worst[0] < -1e-3 ? 0 : 1;
}
