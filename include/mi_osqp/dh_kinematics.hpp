// dh_kinematics.hpp -- forward kinematics / position Jacobians of any serial arm of revolute joints given by its standard
// DH table (mi_gomp_chain in mi_osqp.h), for collision balls fixed anywhere in a link frame: the host twin of the device
// model MI_GOMP_MODEL_DH_CHAIN.
//
//     T_i = Rz(q_i + theta0_i) Tz(d_i) Tx(a_i) Rx(alpha_i),  i = 0 .. n_joints-1     (as ur5e_kinematics.hpp, theta0 = 0 there)
//     frame k (1 <= k <= n_joints): after k joints, origin o_k, rotation R_k
//     a ball at c in frame k:  p = o_k + R_k c,  Jacobian column j = z_j x (p - o_j) for j < k, 0 for j >= k
//
//   mi_osqp::dh::point(chain, q, frame, c, p, J)       p[3] and (J non-null) the 3 x n_joints row-major Jacobian
//   miosqp_ref::dhBall(chain, frame, c, radius, grip)   a RobotBall whose callbacks call it and which names the device model,
//                                                       so ContinuousGOMPSolver (device_assembly, dh_chain = chain) can
//                                                       re-linearise on the GPU
//   miosqp_ref::dhSelfPairs(balls, gap, margin)         the self-collision pairs of such balls: frames at least `gap` apart
//   mi_osqp::dh::axis(chain, q, frame, a, u, dU)        a unit vector a fixed in frame k: u = R_k a and (dU non-null) the 3 x n_joints
//                                                       row-major derivative, column j = z_j x u for j < k, 0 for j >= k
//   miosqp_ref::dhTilt(chain, frame, axis, ref, max_angle, margin)   a TiltLimit on such a vector, which names the frame for the device
//   miosqp_ref::dhGoal(chain, ball, frame, axis)        the structure of a GraspGoal: ball `ball` of the planner's list and such a vector
//                                                       (frame 0: the position only)
#pragma once

#include <array>
#include <cmath>
#include <tuple>
#include <vector>

#include "../mi_osqp.h"
#include "gomp.hpp"

namespace mi_osqp {
namespace dh {

constexpr int kMaxJoints = 8;

inline void point(const mi_gomp_chain &ch, const double *q, int frame, const double c[3], double p[3], double *J /* 3 x n row-major, or null */) {
  const int n = ch.n_joints;
  double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, o[3] = {0, 0, 0};
  double oj[kMaxJoints][3], zj[kMaxJoints][3];
  for (int i = 0; i < frame && i < n && i < kMaxJoints; i++) {
    for (int r = 0; r < 3; r++) { oj[i][r] = o[r]; zj[i][r] = R[r][2]; }
    const double th = q[i] + ch.theta0[i];
    const double ct = std::cos(th), st = std::sin(th), ca = std::cos(ch.alpha[i]), sa = std::sin(ch.alpha[i]);
    const double T[3][4] = {{ct, -st * ca, st * sa, ch.a[i] * ct}, {st, ct * ca, -ct * sa, ch.a[i] * st}, {0.0, sa, ca, ch.d[i]}};
    double G[3][3], g[3];
    for (int r = 0; r < 3; r++) {
      for (int k = 0; k < 3; k++) G[r][k] = R[r][0] * T[0][k] + R[r][1] * T[1][k] + R[r][2] * T[2][k];
      g[r] = R[r][0] * T[0][3] + R[r][1] * T[1][3] + R[r][2] * T[2][3] + o[r];
    }
    for (int r = 0; r < 3; r++) { for (int k = 0; k < 3; k++) R[r][k] = G[r][k]; o[r] = g[r]; }
  }
  for (int r = 0; r < 3; r++) p[r] = o[r] + (R[r][0] * c[0] + R[r][1] * c[1] + R[r][2] * c[2]);
  if (!J) return;
  for (int j = 0; j < n; j++) {
    double col[3] = {0, 0, 0};
    if (j < frame) {
      const double r[3] = {p[0] - oj[j][0], p[1] - oj[j][1], p[2] - oj[j][2]};
      col[0] = zj[j][1] * r[2] - zj[j][2] * r[1];
      col[1] = zj[j][2] * r[0] - zj[j][0] * r[2];
      col[2] = zj[j][0] * r[1] - zj[j][1] * r[0];
    }
    for (int ax = 0; ax < 3; ax++) J[ax * n + j] = col[ax];
  }
}

// point() without the origins: rotations only (the host twin of the device's dh_axis; formulas at mi_gomp_tilt)
inline void axis(const mi_gomp_chain &ch, const double *q, int frame, const double a[3], double u[3], double *dU /* 3 x n row-major, or null */) {
  const int n = ch.n_joints;
  double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  double zj[kMaxJoints][3];
  for (int i = 0; i < frame && i < n && i < kMaxJoints; i++) {
    for (int r = 0; r < 3; r++) zj[i][r] = R[r][2];
    const double th = q[i] + ch.theta0[i];
    const double ct = std::cos(th), st = std::sin(th), ca = std::cos(ch.alpha[i]), sa = std::sin(ch.alpha[i]);
    const double T[3][3] = {{ct, -st * ca, st * sa}, {st, ct * ca, -ct * sa}, {0.0, sa, ca}};
    double G[3][3];
    for (int r = 0; r < 3; r++)
      for (int k = 0; k < 3; k++) G[r][k] = R[r][0] * T[0][k] + R[r][1] * T[1][k] + R[r][2] * T[2][k];
    for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) R[r][k] = G[r][k];
  }
  for (int r = 0; r < 3; r++) u[r] = R[r][0] * a[0] + R[r][1] * a[1] + R[r][2] * a[2];
  if (!dU) return;
  for (int j = 0; j < n; j++) {
    double col[3] = {0, 0, 0};
    if (j < frame) {
      col[0] = zj[j][1] * u[2] - zj[j][2] * u[1];
      col[1] = zj[j][2] * u[0] - zj[j][0] * u[2];
      col[2] = zj[j][0] * u[1] - zj[j][1] * u[0];
    }
    for (int ax = 0; ax < 3; ax++) dU[ax * n + j] = col[ax];
  }
}

}  // namespace dh
}  // namespace mi_osqp

namespace miosqp_ref {

// A collision ball of radius `radius` centred at c in frame `frame` of the chain.  fk / jacobian (3 x n_joints, row-major)
// are what the sequential, lock-step and host-assembling drivers call; the built-in model is what the device path reads.
inline RobotBall dhBall(const mi_gomp_chain &chain, int frame, const std::array<double, 3> &c, double radius, bool is_gripper = false) {
  ForwardKinematicsFun fk = [chain, frame, c](double *q) {
    double p[3];
    mi_osqp::dh::point(chain, q, frame, c.data(), p, nullptr);
    return std::tuple<double, double, double>{p[0], p[1], p[2]};
  };
  JacobianFun jac = [chain, frame, c](double *out, double *q) {
    double p[3];
    mi_osqp::dh::point(chain, q, frame, c.data(), p, out);
  };
  RobotBall b(std::move(fk), std::move(jac), radius, is_gripper);
  b.withBuiltin(MI_GOMP_MODEL_DH_CHAIN, {(double)frame, c[0], c[1], c[2]});
  return b;
}

// A tilt limit on the unit vector `axis` fixed in frame `frame` of the chain: it stays within max_angle radians of the unit
// world vector `ref`, the row starts to constrain `margin` radians inside the cone.  The callback is what the sequential,
// lock-step and host-assembling drivers call; frame and axis are what the device path reads.
inline TiltLimit dhTilt(const mi_gomp_chain &chain, int frame, const std::array<double, 3> &axis, const std::array<double, 3> &ref, double max_angle,
                        double margin = 0.0) {
  TiltLimit t;
  t.axis = [chain, frame, axis](const double *q, double *u, double *dU) { mi_osqp::dh::axis(chain, q, frame, axis.data(), u, dU); };
  t.ref = ref; t.max_angle = max_angle; t.margin = margin;
  t.builtin_frame = frame; t.builtin_axis = axis;
  return t;
}

// The structure of a grasp goal: ball `ball` of the planner's ball list reaches the target point, and the unit vector `axis`
// fixed in frame `frame` of the chain the target cone (frame 0: a position-only goal, `axis` is not read).  The waypoint is
// the planner's to set, the target the caller's (GoalTarget).  The callback is what the sequential, lock-step and
// host-assembling drivers call; frame and axis are what the device path reads.
inline GraspGoal dhGoal(const mi_gomp_chain &chain, size_t ball, int frame = 0, const std::array<double, 3> &axis = {0.0, 0.0, 1.0}) {
  GraspGoal g;
  g.ball = ball;
  if (frame >= 1) {
    g.axis = [chain, frame, axis](const double *q, double *u, double *dU) { mi_osqp::dh::axis(chain, q, frame, axis.data(), u, dU); };
    g.builtin_frame = frame; g.builtin_axis = axis;
  }
  return g;
}

// The usual "skip adjacent links" rule of a self-collision model: every pair (i, j), i < j, of dhBall balls of `balls` whose
// frames are at least `min_frame_gap` apart, in that order, with `margin`.  Balls of other models are left out.  (Two balls of
// one frame keep their distance whatever the joints do: a gap below 1 is taken as 1.)
inline std::vector<BallPair> dhSelfPairs(const std::vector<RobotBall> &balls, int min_frame_gap = 2, double margin = 0.0) {
  std::vector<BallPair> pairs;
  const int gap = min_frame_gap < 1 ? 1 : min_frame_gap;
  for (size_t i = 0; i < balls.size(); ++i)
    for (size_t j = i + 1; j < balls.size(); ++j) {
      if (balls[i].builtin_model != MI_GOMP_MODEL_DH_CHAIN || balls[j].builtin_model != MI_GOMP_MODEL_DH_CHAIN) continue;
      const int fi = (int)balls[i].builtin_param[0], fj = (int)balls[j].builtin_param[0];
      if ((fi > fj ? fi - fj : fj - fi) >= gap) pairs.push_back(BallPair{i, j, margin});
    }
  return pairs;
}

}  // namespace miosqp_ref
