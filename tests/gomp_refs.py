"""A plain high-precision reference of the device re-linearisation (a helper module of the tests, not a conftest).

What gomp_relinearise_kernel computes - the 3-D rows of ConstraintBuilder::withObstacles and the verdict of
GOMPSolver::isSolutionOK (include/mi_osqp.h, "GOMP re-linearisation on the device") - restated in Python from the
published formulas alone: forward kinematics and position Jacobians in mpmath at 50 digits (rounded to double at the
very end), the collision rule of HorizontalLine::hasCollision and the acceptance test with the quantity behind every
decision, so that a test can leave out the decisions no fp64 evaluation can be trusted with.  Nothing in the reference
part calls into libmi_osqp; the ctypes declarations of the mi_gomp_* entry points at the end take the library as an
argument (the package gains no API).

The same formulas run in np.float64 as well (`F64`): the distance between the two evaluations is the error an honest
fp64 implementation makes, and the tolerance of the GPU tests is derived from it (fp64_error, gpu_tolerance).

The three scenes of tests/test_gpu_gomp_scene.py are defined here (scene / scene_reference), so that
tests/test_gomp_refs.py can check their populations on the CPU before anything runs on a GPU."""
import ctypes as C
import functools
import json
import os

import mpmath
import numpy as np
import scipy.sparse as sp

from osqp_solver_amd import problems as PR

MP = mpmath.mp.clone()
MP.dps = 50

INF = 1e30                      # the reference's INF ([REF] src/utils.h) = OSQP_INFTY
ERROR = 1e-3                    # the reference's ERROR of isSolutionOK / isAbove
MARGIN = 1e-9                   # a decision closer than this to its threshold is not compared
FLANGE, WRIST3, ELBOW, YAW_2LINK, TABLE = 1, 2, 3, 4, 5        # mi_gomp_model
FIXED = -1                      # reference only: positions listed per waypoint in "points" (a stateful fk callback)
CLASSES = ("close", "prev", "next", "none")

# Universal Robots' published DH parameters of the UR5e (header of include/mi_osqp/ur5e_kinematics.hpp)
UR5E_A = (0.0, -0.425, -0.3922, 0.0, 0.0, 0.0)
UR5E_D = (0.1625, 0.0, 0.0, 0.1333, 0.0997, 0.0996)
UR5E_ALPHA_HALF_PI = (1, 0, 0, 1, -1, 0)                       # alpha in units of pi / 2
UR5E_FRAME = {FLANGE: 6, WRIST3: 5, ELBOW: 2}


class _MPArith:
    name = "mp"
    num, sin, cos, sqrt = MP.mpf, MP.sin, MP.cos, MP.sqrt

    @staticmethod
    def half_pi():
        return MP.pi / 2


class _F64Arith:
    name = "f64"
    num, sin, cos, sqrt = np.float64, np.sin, np.cos, np.sqrt

    @staticmethod
    def half_pi():
        return np.float64(np.pi / 2)


MPA, F64 = _MPArith, _F64Arith


# ------------------------------------------------------------------ kinematics

def ur5e_frames(q, K=MPA):
    """Origins o_0 .. o_6 and joint axes z_0 .. z_5 of the DH chain T_i = Rz(q_i) Tz(d_i) Tx(a_i) Rx(alpha_i)."""
    one, zero = K.num(1), K.num(0)
    R = [[one, zero, zero], [zero, one, zero], [zero, zero, one]]
    o = [zero, zero, zero]
    origins, axes = [], []
    for i in range(6):
        origins.append(list(o))
        axes.append([R[0][2], R[1][2], R[2][2]])
        ct, st = K.cos(K.num(q[i])), K.sin(K.num(q[i]))
        al = K.half_pi() * UR5E_ALPHA_HALF_PI[i]
        ca, sa = K.cos(al), K.sin(al)
        a, d = K.num(UR5E_A[i]), K.num(UR5E_D[i])
        T = [[ct, -st * ca, st * sa, a * ct], [st, ct * ca, -ct * sa, a * st], [zero, sa, ca, d]]
        Rn = [[R[r][0] * T[0][c] + R[r][1] * T[1][c] + R[r][2] * T[2][c] for c in range(3)] for r in range(3)]
        o = [R[r][0] * T[0][3] + R[r][1] * T[1][3] + R[r][2] * T[2][3] + o[r] for r in range(3)]
        R = Rn
    origins.append(list(o))
    return origins, axes


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def ur5e_point(q, frame, K=MPA, frames=None):
    """(p, J): the origin of `frame` and its 3 x 6 position Jacobian, column j = z_j x (p - o_j) for j < frame, else 0."""
    origins, axes = frames if frames is not None else ur5e_frames(q, K)
    p = origins[frame]
    J = [[K.num(0)] * 6 for _ in range(3)]
    for j in range(frame):
        col = _cross(axes[j], [p[k] - origins[j][k] for k in range(3)])
        for ax in range(3):
            J[ax][j] = col[ax]
    return list(p), J


def yaw_2link(q, param, K=MPA):
    """p = (r cos q0, r sin q0, Z0 + L1 sin q1 + L2 sin(q1 + q2)), r = L1 cos q1 + L2 cos(q1 + q2), and dp/dq."""
    L1, L2, Z0 = K.num(param[0]), K.num(param[1]), K.num(param[2])
    q0, q1, q12 = K.num(q[0]), K.num(q[1]), K.num(q[1]) + K.num(q[2])
    c0, s0, c1, s1, c12, s12 = K.cos(q0), K.sin(q0), K.cos(q1), K.sin(q1), K.cos(q12), K.sin(q12)
    r = L1 * c1 + L2 * c12
    dr1, dr2 = -L1 * s1 - L2 * s12, -L2 * s12
    p = [r * c0, r * s0, Z0 + L1 * s1 + L2 * s12]
    J = [[-r * s0, c0 * dr1, c0 * dr2], [r * c0, s0 * dr1, s0 * dr2], [K.num(0), L1 * c1 + L2 * c12, L2 * c12]]
    return p, J


def fk_jac(ball, q, w, K=MPA, cache=None):
    """(p, J[3][D]) of one ball at joint position q (waypoint w)."""
    model = ball["model"]
    if model in UR5E_FRAME:
        frames = None
        if cache is not None:
            key = (K.name, w)
            if key not in cache:
                cache[key] = ur5e_frames(q, K)
            frames = cache[key]
        return ur5e_point(q, UR5E_FRAME[model], K, frames)
    if model == YAW_2LINK:
        return yaw_2link(q, ball["param"], K)
    J = [[K.num(ball["param"][3 * ax + j]) for j in range(3)] for ax in range(3)]
    if model == TABLE:
        return [K.num(q[0]), K.num(q[1]), K.num(q[2])], J
    if model == FIXED:
        return [K.num(v) for v in ball["points"][w]], J
    raise ValueError(f"model {model}")


# ------------------------------------------------------------------ rows and verdict

def row_layout(D, W, balls, n_lines):
    """(row0, populated 3-D rows): ball-major, then waypoint, then the three box rows of a gripper ball, then the lines."""
    row0 = (W - 1) * D + D * (3 * W - 3)
    return row0, W * sum((3 if b["gripper"] else 0) + n_lines for b in balls)


def _present(con, ax, lower):
    if con is None:
        return False
    return con[ax] > -1e29 if lower else con[ax] < 1e29


def _dist_xy(line_n, P):
    """HorizontalLine::getDistanceVecXY: X - P in the plane, X = A + ((P - A) . D) D, D horizontal and of unit length."""
    A, Dn = line_n
    t = (P[0] - A[0]) * Dn[0] + (P[1] - A[1]) * Dn[1]
    return [A[0] + t * Dn[0] - P[0], A[1] + t * Dn[1] - P[1]]


def distance_vec(line, P, K=MPA):
    """HorizontalLine::getDistanceVec: the perpendicular X - P from P to the line, all three components."""
    dx, dy = K.num(line["dir"][0]), K.num(line["dir"][1])
    nrm = K.sqrt(dx * dx + dy * dy)
    A, P = [K.num(v) for v in line["point"]], [K.num(v) for v in P]
    return _dist_xy((A, [dx / nrm, dy / nrm]), P) + [A[2] - P[2]]


_GEOM = {}


def _evaluate(D, W, balls, lines, con_lo, con_hi, traj, K, margin):
    traj = np.ascontiguousarray(traj, np.float64)
    key = (D, W, json.dumps([balls, lines, None if con_lo is None else list(con_lo), None if con_hi is None else list(con_hi)]),
           traj.tobytes(), K.name, margin)
    if key in _GEOM:
        return _GEOM[key]
    num, f = K.num, float
    err, inf, mg = num(ERROR), num(INF), num(margin)
    lines_n = []
    for ln in lines:
        dx, dy = num(ln["dir"][0]), num(ln["dir"][1])
        nrm = K.sqrt(dx * dx + dy * dy)
        lines_n.append(([num(v) for v in ln["point"]], [dx / nrm, dy / nrm]))
    cache = {}
    rows = dict(vals=[], l=[], u=[], l_scale=[], u_scale=[], cls=[], ball=[], w=[], kind=[], near=[])
    decisions, margins = [], []
    ok, uncertain_fail, definite_fail, causes = True, False, False, set()

    def compare(kind, b, w, idx, slack, decision_near=False):
        nonlocal ok, uncertain_fail, definite_fail
        near = abs(slack) < mg
        margins.append(dict(kind=kind, ball=b, w=w, idx=idx, slack=f(slack), near=bool(near or decision_near)))
        if slack < 0:
            ok = False
            causes.add(kind)
        if near or (decision_near and not slack >= mg):
            uncertain_fail = True
        elif slack < 0 and not decision_near:
            definite_fail = True

    for bi, ball in enumerate(balls):
        r = num(ball["radius"])
        pos, jac = [], []
        for w in range(W):
            p, J = fk_jac(ball, traj[w * D:(w + 1) * D], w, K, cache)
            pos.append(p)
            jac.append(J)
        for w in range(W):
            p, J = pos[w], jac[w]
            q = [num(v) for v in traj[w * D:(w + 1) * D]]
            Jq = [sum((J[ax][j] * q[j] for j in range(D)), num(0)) for ax in range(3)]
            Jq_abs = [sum((abs(J[ax][j] * q[j]) for j in range(D)), num(0)) for ax in range(3)]

            def put(axis, low, upp, low_scale, upp_scale, cls, kind, near):
                rows["vals"].append([f(J[axis][j]) for j in range(D)])
                rows["l"].append(f(low + r)); rows["u"].append(f(upp - r))
                rows["l_scale"].append(f(low_scale)); rows["u_scale"].append(f(upp_scale))
                rows["cls"].append(cls); rows["ball"].append(bi); rows["w"].append(w); rows["kind"].append(kind); rows["near"].append(near)

            if ball["gripper"]:
                for ax in range(3):
                    low, upp, ls, us = -inf, inf, num(0), num(0)
                    if _present(con_lo, ax, True):
                        c = num(con_lo[ax])
                        low, ls = c - p[ax] + Jq[ax], abs(c) + abs(p[ax]) + Jq_abs[ax] + r
                        compare("box_low", bi, w, ax, (p[ax] - r) - (c - err))
                    if _present(con_hi, ax, False):
                        c = num(con_hi[ax])
                        upp, us = c - p[ax] + Jq[ax], abs(c) + abs(p[ax]) + Jq_abs[ax] + r
                        compare("box_high", bi, w, ax, (c + err) - (p[ax] + r))
                    put(ax, low, upp, ls, us, "box", ax, False)
            for li, ln in enumerate(lines):
                A = lines_n[li][0]
                dp = _dist_xy(lines_n[li], p)
                close_q = K.sqrt(dp[0] * dp[0] + dp[1] * dp[1]) - r
                prev_q = next_q = None
                near = abs(close_q) < mg
                cls = "none"
                if close_q < 0:
                    cls = "close"
                else:
                    if w > 0:
                        dn = _dist_xy(lines_n[li], pos[w - 1])
                        prev_q = dn[0] * dp[0] + dn[1] * dp[1]
                        near = near or abs(prev_q) < mg
                        if prev_q < 0:
                            cls = "prev"
                    if cls == "none" and w + 1 < W:
                        dn = _dist_xy(lines_n[li], pos[w + 1])
                        next_q = dp[0] * dn[0] + dp[1] * dn[1]
                        near = near or abs(next_q) < mg
                        if next_q < 0:
                            cls = "next"
                near = bool(near)
                decisions.append(dict(ball=bi, w=w, line=li, cls=cls, near=near, close=f(close_q),
                                      prev=None if prev_q is None else f(prev_q), next=None if next_q is None else f(next_q)))
                below = bool(ln.get("below"))
                height = p[2] - A[2]
                slack = (-r + err) - height if below else height - (r - err)
                if cls != "none":
                    bound = A[2] - p[2] + Jq[2]
                    scale = abs(A[2]) + abs(p[2]) + Jq_abs[2] + r
                    if below:
                        put(2, -inf, bound, num(0), scale, cls, 3 + li, near)
                    else:
                        put(2, bound, inf, scale, num(0), cls, 3 + li, near)
                    compare("not_below" if below else "not_above", bi, w, li, slack, near)
                else:
                    put(2, -inf, inf, num(0), num(0), cls, 3 + li, near)
                    if near and not slack >= mg:          # it might collide after all, and would then not pass
                        uncertain_fail = True
    out = {k: np.array(v) if k not in ("cls",) else v for k, v in rows.items()}
    out["vals"] = np.array(rows["vals"], np.float64).reshape(len(rows["l"]), D)
    out.update(decisions=decisions, margins=margins, ok=ok, causes=causes,
               verdict_excluded=bool(uncertain_fail and not definite_fail))
    _GEOM[key] = out
    return out


def with_obstacles(D, W, balls, lines, con_lo, con_hi, traj, margin=MARGIN, K=MPA):
    """The populated 3-D rows of ConstraintBuilder::withObstacles(con_3d, traj), in the reference's order.

    balls: dicts {"model", "gripper", "radius", "param"}; lines: dicts {"dir", "point", "below"}; con_lo / con_hi: three
    numbers each (+-1e30 = that side absent) or None; traj: the 2 D W vector of which only the W positions are read.
    Returns a dict of arrays over the rows: vals[rows][D] (the entries in the columns of q_w), l, u, the term scales
    l_scale / u_scale (sum of the absolute values of the terms of a bound, 0 where the side is +-1e30), cls ("box",
    "close", "prev", "next", "none"), ball, w, kind (0..2 = box axis, 3 + i = line i), near (a decision of the row is
    within `margin` of its threshold: its l and u are not compared) - and "decisions": per (ball, waypoint, line) the
    class and the quantities behind it (close = distance - radius, prev / next = the dot products of the perpendiculars,
    None where the rule does not get that far)."""
    return _evaluate(D, W, balls, lines, con_lo, con_hi, traj, K, margin)


def solution_ok(D, W, balls, lines, con_lo, con_hi, traj, margin=MARGIN, K=MPA):
    """GOMPSolver::isSolutionOK(traj): (ok, details).  details: "margins" - every comparison made with its slack (>= 0:
    passed; kinds box_low, box_high, not_above, not_below), "causes" - the kinds that failed, "verdict_excluded" - the
    verdict hangs on a decision or comparison within `margin` of its threshold and no other comparison settles it."""
    e = _evaluate(D, W, balls, lines, con_lo, con_hi, traj, K, margin)
    return e["ok"], dict(margins=e["margins"], causes=e["causes"], verdict_excluded=e["verdict_excluded"])


# ------------------------------------------------------------------ the batch a scene sits on

def scene_problem(D, W, balls, n_lines, B, over_allocate, starts=None, ends=None, seed=4100):
    """B QPs in the layout BatchSolver takes: the joint-space rows of GOMPSolver::run's QP (PR.GompBuilder, as
    PR.gomp_qp builds them), then the populated 3-D rows - D entries of 1.0 in the columns of q_w, bounds -+1e30 - and,
    with over_allocate, the all-zero rows up to the reference's D W (3 + lines balls) ([REF] constraint-builder.h:43-44).
    "aidx"[row][j]: where entry j of populated row `row` sits in the CSC value array."""
    row0, rows3d = row_layout(D, W, balls, n_lines)
    m = row0 + (D * W * (3 + n_lines * len(balls)) if over_allocate else rows3d)
    n = 2 * D * W
    rng = np.random.default_rng(seed)
    starts = rng.uniform(-1, 1, (B, D)) if starts is None else np.asarray(starts, float)
    ends = rng.uniform(-1, 1, (B, D)) if ends is None else np.asarray(ends, float)
    q_lim, v_lim, a_lim, ts = 2 * np.pi, np.pi, np.pi * 800 / 180, 0.1
    pos_con = PR.in_range(np.full(D, -q_lim), np.full(D, q_lim))
    vel_con = PR.scaled(PR.in_range(np.full(D, -v_lim), np.full(D, v_lim)), ts)
    acc_con = PR.scaled(PR.in_range(np.full(D, -a_lim), np.full(D, a_lim)), ts * ts)
    zero = PR.equal(np.zeros(D))
    r3, c3 = [], []
    r = row0
    for ball in balls:
        for w in range(W):
            for _ in range((3 if ball["gripper"] else 0) + n_lines):
                r3 += [r] * D
                c3 += list(range(w * D, (w + 1) * D))
                r += 1
    A0, ls, us, Axs, aidx = None, [], [], [], None
    for b in range(B):
        bld = PR.GompBuilder(D, W)
        bld.position(0, PR.equal(starts[b])).positions(1, W - 2, pos_con)
        if W >= 4:
            (bld.position(W - 3, PR.equal(ends[b])).velocities(0, W - 4, vel_con).velocity(W - 3, zero)
                .accelerations(0, W - 4, acc_con).acceleration(W - 3, zero))
        l, A, u = bld.build()
        J = sp.coo_matrix(A[:row0])
        rows, cols = np.concatenate([J.row, r3]), np.concatenate([J.col, c3])
        vals = np.concatenate([J.data, np.ones(len(r3))])
        tag = sp.csc_matrix((np.arange(1, len(vals) + 1, dtype=float), (rows, cols)), shape=(m, n))
        tag.sort_indices()
        src = tag.data.astype(np.int64) - 1                       # csc slot -> triplet
        if A0 is None:
            A0 = sp.csc_matrix((vals[src], tag.indices, tag.indptr), shape=(m, n))
            where = np.empty(len(vals), np.int64)
            where[src] = np.arange(len(vals))
            aidx = where[len(J.data):].reshape(rows3d, D)
        Axs.append(vals[src])
        ls.append(np.concatenate([l[:row0], np.full(m - row0, -INF)]))
        us.append(np.concatenate([u[:row0], np.full(m - row0, INF)]))
    P = sp.csc_matrix(PR.tri_diagonal_matrix(2.0, -1.0, n, D * W, D))
    P.sort_indices()
    return dict(n=n, m=m, P=P, A=A0, Px=np.tile(P.data, (B, 1)), Ax=np.array(Axs), q=None, l=np.array(ls), u=np.array(us),
                row0=row0, rows3d=rows3d, aidx=aidx, starts=starts, ends=ends)


def reference_rows(pr, b, ref):
    """(Ax, l, u) of QP b of a scene_problem with the populated 3-D rows replaced by a with_obstacles result."""
    Ax, l, u = pr["Ax"][b].copy(), pr["l"][b].copy(), pr["u"][b].copy()
    Ax[pr["aidx"]] = ref["vals"]
    l[pr["row0"]:pr["row0"] + pr["rows3d"]] = ref["l"]
    u[pr["row0"]:pr["row0"] + pr["rows3d"]] = ref["u"]
    return Ax, l, u


# ------------------------------------------------------------------ the scenes of the GPU tests

E20 = 2.0 ** -20


def grid(v):
    """v rounded to a multiple of 2^-30: every coordinate of scene T is such a number below 16 in magnitude and every
    Jacobian entry a multiple of 1/4 below 16, so each product and sum of the rows is exact in fp64 in any order."""
    return round(v * 2.0 ** 30) / 2.0 ** 30


def _ball(model, gripper, radius, param=()):
    return dict(model=model, gripper=bool(gripper), radius=float(radius), param=[float(v) for v in param] + [0.0] * (12 - len(param)))


T_TABLES = ([1, .25, 0, 0, 1, .5, .25, 0, 1], [2, 0, .5, .25, 1, 0, 0, .75, 1], [1, 0, .25, .5, 2, 0, 0, .25, 1.5], [.5, .25, 0, 0, 1.5, .25, .75, 0, 2])
T_LINES = [dict(dir=[1.0, 0.0], point=[0.0, 0.5, 1.0], below=False), dict(dir=[0.0, 1.0], point=[0.5, 0.0, 2.0], below=True)]
T_LO, T_HI = [-4.0, -INF, -2.0], [INF, 4.0, INF]
_HI, _LO, _Z = 3.0, -2.0, 1.5


def _t_balls(four):
    b = [_ball(TABLE, 1, 1 / 16, T_TABLES[0]), _ball(TABLE, 0, 1 / 8, T_TABLES[1]), _ball(TABLE, 1, 0, T_TABLES[2])]
    return b + [_ball(TABLE, 0, 1 / 4, T_TABLES[3])] if four else b


def _with_velocities(pos, ts=0.1):
    W, D = pos.shape
    vel = np.zeros((W, D))
    vel[:-1] = (pos[1:] - pos[:-1]) / ts
    return np.concatenate([pos.reshape(-1), vel.reshape(-1)])


def _t_thresholds(rmax):
    rg = 1 / 16                                                   # the larger gripper radius: the box binds it first
    return dict(zA=grid(1 + rmax - ERROR), zB=grid(2 - rmax + ERROR), x=grid(-4 - ERROR + rg), y=grid(4 + ERROR - rg), z=grid(-2 - ERROR + rg))


def _t_tour(W, th, s, zA=+1, zB=-1, xc=+1, yc=-1, zc=+1):
    """Crosses line 0 at waypoints 9|10 + s and line 1 at 19|20 + s at the acceptance heights -+ 2^-20, touches the box
    at x (30 + s), y (35 + s: a spike across line 0 and back) and z (40 + s) at -+1e-3 -+ 2^-20."""
    p = np.tile([_HI, _HI, _Z], (W, 1))
    p[10 + s:, 1] = _LO
    p[9 + s:11 + s, 2] = th["zA"] + zA * E20
    p[20 + s:, 0] = _LO
    p[19 + s:21 + s, 2] = th["zB"] + zB * E20
    p[30 + s, 0] = th["x"] + xc * E20
    p[35 + s, 1] = th["y"] + yc * E20
    p[40 + s, 2] = th["z"] + zc * E20
    return p


def _t_trajectories(W, rmax):
    th = _t_thresholds(rmax)
    ra, rb = 1 / 16, 1 / 8
    if W == 2:
        pts = [
            [(th["x"] + E20, .5 - ra * (1 - E20), _Z), (th["x"] + E20, .5 + rb * (1 + E20), _Z)],         # close (r = 1/16, 1/8) | just not close: prev
            [(3, .5, th["zA"] + E20), (3, _HI, _Z)],                                           # on line 0: close, or (r = 0) dot = 0: none
            [(_HI, 3, _Z), (.5 - ra * (1 - E20), 3, th["zB"] - E20)],                          # line 1 crossed (r = 0) or close at the far side
            [(3, _LO, th["zA"] - E20), (3, _HI, _Z)],                              # line 0 crossed 2^-20 too low
            [(_HI, 3, _Z), (_LO, 3, th["zB"] + E20)],                              # line 1 crossed 2^-20 too high
            [(3, .5 + ra * (1 - E20), _Z), (.5 - ra * (1 - E20), th["y"] - E20, _Z)],         # close to line 0, then to line 1
            [(th["x"] - E20, 3, _Z), (_HI, 3, _Z)],                                # 2^-20 outside the box in x, line 1 crossed
            [(3, th["y"] + E20, _Z), (3, _LO, _Z)],                                # 2^-20 outside the box in y, line 0 crossed
            ]
        return np.array([_with_velocities(np.array(p, float)) for p in pts])
    out = []
    p = np.tile([_HI, _HI, _Z], (W, 1))                           # 0: line 0 crossed at both ends, close at 40 (and 42 for r = 1/8 only)
    p[0, 1] = p[W - 1, 1] = _LO
    p[40, 1], p[42, 1] = .5 + ra * (1 - E20), .5 + ra * (1 + E20)
    out.append(p)
    p = np.tile([_HI, _HI, _Z], (W, 1))                           # 1: close at waypoint 0, line 1 crossed at W-3 | W-2
    p[0, 1], p[1, 1] = .5 + ra * (1 - E20), .5 + rb * (1 + E20)
    p[W - 2:, 0] = _LO
    out.append(p)
    out.append(_t_tour(W, th, 0, zA=-1))                          # 2: not above line 0
    out.append(_t_tour(W, th, 1))                                 # 3: every threshold passed by 2^-20
    out.append(_t_tour(W, th, 2, zB=+1))                          # 4: not below line 1
    out.append(_t_tour(W, th, 3, xc=-1))                          # 5: box, lower x
    out.append(_t_tour(W, th, 4, yc=+1))                          # 6: box, upper y
    p = np.tile([_HI, _HI, _Z], (W, 1))                           # 7: a waypoint exactly on line 0 (dot = 0), line 0 crossed at W-4 | W-3
    p[20, 1] = .5
    p[21:W - 3, 1] = _LO
    p[50, 0], p[52, 0] = .5 + rb * (1 - E20), .5 + ra * (1 - E20)
    p[W - 1, 0] = .5 + ra * (1 - E20)
    out.append(p)
    return np.array([_with_velocities(q) for q in out])


Y_PARAMS = ([0.4, 0.3, 0.2], [0.3, 0.25, 0.2])
U_DIAGONAL = dict(dir=[1.0, 1.0], point=[-0.35, 0.0, 0.75], below=True)


def _sweep(W, a, b, lift, speed=1.0, lift_joint=1):
    """The joint-space sweeps of the planner tests: a straight line from a to b, reached at waypoint (W - 3) / speed, joint 1
    lifted by lift sin(pi t).  A fast sweep steps over a line without a waypoint close to it: classes prev and next."""
    t = np.minimum(1.0, speed * np.arange(W) / (W - 3.0))[:, None]
    pos = a + t * (np.asarray(b) - a)
    pos[:, lift_joint] += lift * np.sin(np.pi * t[:, 0])
    return pos


def _jump(W, a, b, lo, hi):
    """From a towards b up to the fraction lo of the way over the first half of the waypoints, from the fraction hi on over the
    second half: the step in the middle crosses a line with no waypoint close to it (classes next and prev)."""
    h = W // 2
    t = np.concatenate([np.linspace(0.0, lo, h), np.linspace(hi, 1.0, W - h)])[:, None]
    return a + t * (np.asarray(b) - a)


def _u_trajectories(W, seed):
    rng = np.random.default_rng(seed)
    U = lambda *s: rng.uniform(-1.0, 1.0, s)
    up = np.array([np.pi / 2, -np.pi / 2, 0, 0, 0, 0])
    out = []
    for k in range(8):
        if k < 3:                                                 # the planner tests' sweeps across the bar
            a, b = 0.4 * U(6), 0.4 * U(6)
            b[0] += np.pi * (1.0 if k % 2 else 0.3)
            out.append(_sweep(W, a, b, -1.2 if k == 1 else 0.0))
        elif k < 5:                                               # built to cross both lines in one step of the yaw: stretched out low
            cfg = [[-0.35, 0.5, 0, 0, 0], [-1.3, 0.6, 0.3, 0, 0]][k - 3]          # (under the bar) / high (over the diagonal line)
            a = np.array([-3.0] + cfg) + 0.02 * U(6)
            b = a + np.array([1.6, 0.05, -0.05, 0.1, 0, 0]) if k == 3 else a + np.array([1.4, 0.05, 0.0, 0.1, 0, 0])
            out.append(_jump(W, a, b, 0.125, 0.875) if k == 3 else _jump(W, a, b, 0.15, 0.86))
        else:                                                     # small motions around the upright pose, clear of everything
            a = up + 0.15 * U(6)
            out.append(_sweep(W, a, a + 0.15 * U(6), 0.0))
    return np.array([_with_velocities(p) for p in out])


def _y_trajectories(W, seed):
    rng = np.random.default_rng(seed)
    U = lambda: rng.uniform(-1.0, 1.0)
    out = []
    for k in range(8):
        a = np.array([-0.8 + 0.3 * U(), 0.3 + 0.2 * U(), 0.4 + 0.2 * U()])
        b = np.array([0.8 + 0.3 * U(), 0.3 + 0.2 * U(), 0.4 + 0.2 * U()])
        if k == 5:                                                # dips under the floor z >= 0.05
            a[1], b[1] = -0.9, -0.2
        if k == 6:                                                # stretches out past the upper x
            a[1:], b[1:] = [0.1, 0.1], [0.1, 0.2]
        if k in (2, 3):                                           # steps over the bar, low (2) or arched over it (3)
            p = _jump(W, a, b, 0.3, 0.7)
            p[:, 1] += (0.9 if k == 3 else 0.0) * np.sin(np.pi * np.linspace(0, 1, W))
            out.append(p)
        else:
            out.append(_sweep(W, a, b, 0.9 if k % 2 else 0.0))
    return np.array([_with_velocities(p) for p in out])


@functools.lru_cache(maxsize=None)
def scene(name):
    """name: "T86", "T64", "T2", "U", "Y".  A dict with D, W, balls, lines, con_lo, con_hi, trajs[8][2 D W], margin."""
    if name[0] == "T":
        W = int(name[1:])
        balls = _t_balls(W == 64)
        return dict(name=name, D=3, W=W, balls=balls, lines=T_LINES, con_lo=T_LO, con_hi=T_HI, margin=0.0,
                    trajs=_t_trajectories(W, max(b["radius"] for b in balls)))
    if name == "U":
        W = 90
        balls = [_ball(ELBOW, 0, 0.10), _ball(WRIST3, 0, 0.15), _ball(FLANGE, 1, 0.05)]
        lines = [dict(dir=[0.0, 1.0], point=[0.3, 0.0, 0.35], below=False), U_DIAGONAL]
        return dict(name=name, D=6, W=W, balls=balls, lines=lines, con_lo=[-INF, -0.4, -INF], con_hi=None, margin=MARGIN,
                    trajs=_u_trajectories(W, 31))
    if name == "Y":
        W = 130
        balls = [_ball(YAW_2LINK, 1, 0.03, Y_PARAMS[0]), _ball(YAW_2LINK, 0, 0.06, Y_PARAMS[1])]
        lines = [dict(dir=[1.0, 0.0], point=[0.6, 0.0, 0.55], below=False)]
        return dict(name=name, D=3, W=W, balls=balls, lines=lines, con_lo=[-INF, -INF, 0.05], con_hi=[0.66, INF, INF], margin=MARGIN,
                    trajs=_y_trajectories(W, 57))
    raise KeyError(name)


SCENES = ("T86", "T64", "T2", "U", "Y")


@functools.lru_cache(maxsize=None)
def scene_reference(name, K=MPA):
    """with_obstacles of the scene's eight trajectories (a list of its result dicts, solution_ok's fields included)."""
    s = scene(name)
    return [with_obstacles(s["D"], s["W"], s["balls"], s["lines"], s["con_lo"], s["con_hi"], t, s["margin"], K) for t in s["trajs"]]


@functools.lru_cache(maxsize=None)
def fp64_error(name):
    """(values, bounds): the worst distance of the np.float64 evaluation of the reference's formulas from the mpmath one
    over the scene's trajectories - absolute for the matrix values, divided by the bound's term scale for the bounds.
    Rows with a decision within the margin, and rows whose class differs between the two, are left out."""
    ev = eb = 0.0
    for hi, lo in zip(scene_reference(name), scene_reference(name, F64)):
        ev = max(ev, float(np.max(np.abs(hi["vals"] - lo["vals"]))))
        same = np.array([a == b for a, b in zip(hi["cls"], lo["cls"])]) & ~hi["near"]
        for side in ("l", "u"):
            sc = hi[side + "_scale"]
            use = same & (sc > 0)
            if use.any():
                eb = max(eb, float(np.max(np.abs(hi[side] - lo[side])[use] / sc[use])))
    return ev, eb


def gpu_tolerance(name):
    """(absolute tolerance of a matrix value, tolerance of a bound per unit of its term scale): 32 x fp64_error - a
    different order of operations and device sin / cos 1-2 ulp off - and never looser than 1e-13."""
    ev, eb = fp64_error(name)
    return min(32 * ev, 1e-13), min(32 * eb, 1e-13)


SOLVED_QP = 5                   # scene T86: the trajectory 2^-20 outside the box in x; its re-linearised QP is solved


@functools.lru_cache(maxsize=None)
def scene_batch(name, over_allocate=False):
    """scene_problem for the scene's eight trajectories: QP b starts at trajectory b's first waypoint and is pinned to its
    waypoint W - 3 at the end, as a planner sets a segment up."""
    s = scene(name)
    D, W = s["D"], s["W"]
    ends = s["trajs"][:, (W - 3) * D:(W - 2) * D] if W >= 4 else None
    return scene_problem(D, W, s["balls"], len(s["lines"]), 8, over_allocate, starts=s["trajs"][:, :D], ends=ends)


def populations(name):
    """Counts a test can assert on and print: rows per collision class (per ball, and at the two ends), verdicts, causes, exclusions."""
    s, ref = scene(name), scene_reference(name)
    nb, nl, W = len(s["balls"]), len(s["lines"]), s["W"]
    cls = {c: np.zeros((nb, nl), int) for c in CLASSES}
    ends = {c: np.zeros(nb, int) for c in CLASSES}
    near = total = 0
    for e in ref:
        for d in e["decisions"]:
            cls[d["cls"]][d["ball"], d["line"]] += 1
            ends[d["cls"]][d["ball"]] += d["w"] in (0, W - 1)
            near += d["near"]
            total += 1
    causes = {}
    for e in ref:
        for c in e["causes"]:
            causes[c] = causes.get(c, 0) + 1
    return dict(cls=cls, ends=ends, near=near, decisions=total, accepted=sum(e["ok"] for e in ref), rejected=sum(not e["ok"] for e in ref),
                causes=causes, verdicts_excluded=sum(e["verdict_excluded"] for e in ref),
                near_comparisons=sum(m["near"] for e in ref for m in e["margins"]))


# ------------------------------------------------------------------ ctypes: the mi_gomp_* entry points (tests only)

class Ball(C.Structure):
    _fields_ = [("model", C.c_int32), ("is_gripper", C.c_int32), ("radius", C.c_double), ("param", C.c_double * 12)]


class Line(C.Structure):
    _fields_ = [("dir", C.c_double * 2), ("point", C.c_double * 3), ("below", C.c_int32), ("reserved", C.c_int32)]


def declare(L):
    """argtypes of the seven mi_gomp_* entry points on a loaded libmi_osqp (M.lib())."""
    ip, dp, vp, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int32)
    L.mi_gomp_scene_create.argtypes = [C.POINTER(vp), vp, C.c_int64, C.c_int64, C.c_int64, C.POINTER(Ball), C.c_int64, C.POINTER(Line), dp, dp]
    L.mi_gomp_scene_free.argtypes = [vp]
    L.mi_gomp_scene_free.restype = None
    L.mi_gomp_scene_set_rows.argtypes = [vp, C.c_int64, ip, dp, dp, dp]
    L.mi_gomp_scene_get_rows.argtypes = [vp, C.c_int64, dp, dp, dp]
    L.mi_gomp_assemble_some.argtypes = [vp, C.c_int64, ip, dp, i32p]
    L.mi_gomp_relinearise_some.argtypes = [vp, C.c_int64, ip, dp, i32p]
    for f in ("create", "set_rows", "get_rows"):
        getattr(L, "mi_gomp_scene_" + f).restype = C.c_int
    L.mi_gomp_assemble_some.restype = L.mi_gomp_relinearise_some.restype = C.c_int
    return L


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ids(ids):
    a = np.ascontiguousarray(ids, np.int64)
    return a, a.ctypes.data_as(C.POINTER(C.c_int64))


def c_balls(balls):
    arr = (Ball * max(len(balls), 1))()
    for k, b in enumerate(balls):
        arr[k].model, arr[k].is_gripper, arr[k].radius = int(b["model"]), int(b["gripper"]), float(b["radius"])
        for j, v in enumerate(b["param"]):
            arr[k].param[j] = v
    return arr


def c_lines(lines):
    arr = (Line * max(len(lines), 1))()
    for k, ln in enumerate(lines):
        arr[k].dir[0], arr[k].dir[1] = ln["dir"]
        for j in range(3):
            arr[k].point[j] = ln["point"][j]
        arr[k].below = int(bool(ln.get("below")))
    return arr


class GompScene:
    """mi_gomp_scene on the handle of a BatchSolver.  `rc` is the code of mi_gomp_scene_create; a refused scene has ptr None."""

    def __init__(self, L, solver, D, W, balls, lines, con_lo, con_hi):
        self.L, self.solver = declare(L), solver
        self.ptr = C.c_void_p()
        lo = None if con_lo is None else np.ascontiguousarray(con_lo, np.float64)
        hi = None if con_hi is None else np.ascontiguousarray(con_hi, np.float64)
        self.rc = L.mi_gomp_scene_create(C.byref(self.ptr), solver._h, D, W, len(balls), c_balls(balls), len(lines), c_lines(lines), _dp(lo), _dp(hi))

    def close(self):
        if self.ptr:
            self.L.mi_gomp_scene_free(self.ptr)
            self.ptr = C.c_void_p()

    def set_rows(self, ids, Ax, l, u):
        ids, p = _ids(ids)
        Ax, l, u = (np.ascontiguousarray(a, np.float64) for a in (Ax, l, u))
        return self.L.mi_gomp_scene_set_rows(self.ptr, len(ids), p, _dp(Ax), _dp(l), _dp(u))

    def get_rows(self, b):
        A = np.empty(self.solver._Ap[-1])
        l, u = np.empty(self.solver.m), np.empty(self.solver.m)
        rc = self.L.mi_gomp_scene_get_rows(self.ptr, b, _dp(A), _dp(l), _dp(u))
        assert rc == 0, rc
        return A, l, u

    def _launch(self, fn, ids, x):
        ids, p = _ids(ids)
        x = np.ascontiguousarray(x, np.float64)
        ok = np.full(len(ids), -1, np.int32)
        rc = fn(self.ptr, len(ids), p, _dp(x), ok.ctypes.data_as(C.POINTER(C.c_int32)))
        return rc, ok

    def assemble_some(self, ids, x):
        return self._launch(self.L.mi_gomp_assemble_some, ids, x)

    def relinearise_some(self, ids, x):
        return self._launch(self.L.mi_gomp_relinearise_some, ids, x)


def load_kats():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gomp_scene_kats.json")) as f:
        return json.load(f)
