// examples/chain_gomp_example.cpp -- planning for an arm that is not the UR5e: any serial chain of revolute joints given by
// its standard DH table, with collision balls placed along the links.
//
// The reference binds forward kinematics and Jacobians as host callbacks ([REF] src/utils.h:21-22,33-42), one
// pair per ball, written by hand for one robot.  Here the arm is a table (mi_gomp_chain: a, d, alpha, theta0 per joint, with
// T_i = Rz(q_i + theta0_i) Tz(d_i) Tx(a_i) Rx(alpha_i)) and a ball is a frame and a centre in it: dhBall() makes the RobotBall
// - the callbacks for the host drivers, the model MI_GOMP_MODEL_DH_CHAIN for the device - and the planner gets the table
// (dh_chain), so that the whole SQP step runs on the GPU.  The scene: a 7-joint arm, balls on its upper arm, elbow, forearm
// and wrist, the gripper ball kept inside z >= 0.15 and x <= 0.75, and a bar along the x axis at height 0.2 to pass above.
//
//   usage: chain_gomp_example [trajectories = 16] [waypoints = 40] [SQP step on the device: 0|1 = 1]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mi_osqp/dh_kinematics.hpp"
#include "mi_osqp/gomp.hpp"

namespace ref = miosqp_ref;
constexpr size_t kJoints = 7;

int main(int argc, char **argv) {
  setenv("GPU_MAX_HW_QUEUES", "10", 0);                 // one hardware queue per horizon stage
  const int n_traj = argc > 1 ? std::atoi(argv[1]) : 16;
  const size_t waypoints = argc > 2 ? (size_t)std::atoi(argv[2]) : 40;
  const bool on_device = argc > 3 ? std::atoi(argv[3]) != 0 : true;
  if (n_traj < 1 || waypoints < 10) { std::fprintf(stderr, "usage: chain_gomp_example [trajectories] [waypoints >= 10] [0|1]\n"); return 2; }

  const double pi = 3.14159265358979323846, H = pi / 2;
  mi_gomp_chain arm{};
  arm.n_joints = (int)kJoints;
  const double a[kJoints] = {0, 0, 0.0825, -0.0825, 0, 0.088, 0}, d[kJoints] = {0.333, 0, 0.316, 0, 0.384, 0, 0.107};
  const double alpha[kJoints] = {-H, H, H, -H, H, H, 0.3}, theta0[kJoints] = {0, 0, 0, 0.25, 0, 0, -0.7};
  for (size_t i = 0; i < kJoints; ++i) { arm.a[i] = a[i]; arm.d[i] = d[i]; arm.alpha[i] = alpha[i]; arm.theta0[i] = theta0[i]; }

  // (chain, frame, centre in that frame, radius, gripper)
  std::vector<ref::RobotBall> balls{ref::dhBall(arm, 3, {0, 0.05, -0.1}, 0.08),  ref::dhBall(arm, 4, {0.02, 0, 0.03}, 0.07),
                                    ref::dhBall(arm, 5, {0, 0.04, -0.15}, 0.07), ref::dhBall(arm, 6, {0.03, 0, 0}, 0.06),
                                    ref::dhBall(arm, 7, {0.02, -0.01, 0.06}, 0.04, true)};
  std::vector<ref::HorizontalLine> bars{ref::HorizontalLine({1, 0}, {0.0, 0.0, 0.2}, /*bypass from below*/ false)};
  auto joint_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-2 * pi), ref::constraints::of<kJoints>(2 * pi));
  auto speed_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-pi), ref::constraints::of<kJoints>(pi));
  auto accel_limits = ref::constraints::inRange<kJoints>(ref::constraints::of<kJoints>(-pi * 800 / 180), ref::constraints::of<kJoints>(pi * 800 / 180));
  auto work_space = ref::constraints::inRange<3>(ref::Vec<3>{-ref::INF, -ref::INF, 0.15}, ref::Vec<3>{0.75, ref::INF, ref::INF});

  // start / goal pairs that swing the arm across the bar, lower and lower
  const double base[kJoints] = {0, 0.4, 0, -1.6, 0, 1.9, 0.6};
  std::vector<ref::Ctrl<kJoints>> from, to;
  for (int t = 0; t < n_traj; ++t) {
    ref::Ctrl<kJoints> s{}, e{};
    for (size_t j = 0; j < kJoints; ++j) { s[j] = base[j] + 0.02 * ((t + (int)j) % 3 - 1); e[j] = base[j] - 0.02 * ((t + 2 * (int)j) % 3 - 1); }
    s[0] = -1.0 + 0.05 * (t % 8); e[0] = 0.9 - 0.04 * (t % 8);
    s[1] += 0.08 * (t % 4); e[1] += 0.06 * (t % 3);
    from.push_back(s); to.push_back(e);
  }

  ref::ContinuousGOMPSolver<kJoints> planner(waypoints, 0.1, joint_limits, speed_limits, accel_limits, work_space, bars, balls);
  planner.device_assembly = on_device;
  planner.dh_chain = arm;                                // without it the chain balls keep the SQP step on the host threads
  using clock = std::chrono::steady_clock;
  auto t0 = clock::now();
  auto plans = planner.run(from, to);                    // first call: builds the ten per-horizon solvers
  const double first = std::chrono::duration<double>(clock::now() - t0).count();
  t0 = clock::now();
  plans = planner.run(from, to);
  const double again = std::chrono::duration<double>(clock::now() - t0).count();

  int ok = 0, solves = 0, relin = 0;
  for (int t = 0; t < n_traj; ++t) { ok += plans[(size_t)t].first == ref::ExitCode::kOptimal; solves += planner.qp_solves[(size_t)t]; relin += planner.qp_updates[(size_t)t]; }
  std::printf("%d of %d trajectories planned (%zu joints, %zu waypoints, SQP step on the %s)\n", ok, n_traj, kJoints, waypoints, on_device ? "device" : "host threads");
  std::printf("%d QP solves, %d re-linearisations; first run %.3f s, next run %.3f s = %.1f trajectories/s\n", solves, relin, first, again, n_traj / again);
  return ok == n_traj ? 0 : 1;
}
