"""Grasp goals (mi_gomp_goal / mi_gomp_goal_value, GraspGoal) beside tests/grid_refs.py, tests/tilt_refs.py, tests/pair_refs.py,
tests/cuboid_refs.py, tests/capsule_refs.py, tests/gomp_refs.py and tests/dh_refs.py: a helper module of the tests, not a conftest.

A goal has a structure every QP of a scene shares - a ball b, a waypoint w, optionally a frame k of the scene's chain and a
unit `axis` in it - and values per QP: a target `point`, half widths tol[3] >= 0 (>= 1e30: a free axis, 0: an equality), a unit
world vector `ref` and max_angle in (0, pi).  It owns four rows, their entries in the columns of q_w.  With p = fk_b(q_w), J the
ball's Jacobian and Jq_ax = sum_j J[ax][j] q_w[j], j ascending (include/mi_osqp.h has the same definition, restated here from
it alone), in this order of operations:

    rows 0 .. 2 (ax = x, y, z) hold J[ax][j]
        a free axis:  l = -1e30, u = +1e30
        otherwise     l = ((point_ax - tol_ax) - p_ax) + Jq_ax,   u = ((point_ax + tol_ax) - p_ax) + Jq_ax
        accepted only if |p_ax - point_ax| <= tol_ax + 1e-3 on every axis that is not free
    row 3, k = 0:  zeros (written), l = -1e30, u = +1e30, no say in the verdict
    row 3, k >= 1: c and g_j those of tilt_refs.tilt_cosine; the row holds g_j,
        l = (cos_lim - c) + sum_j g_j q_w[j], u = +1e30; accepted only if c >= cos_ok
        cos_lim = cos(max_angle), cos_ok = cos(min(pi, max_angle + 1e-3)): two fp64 numbers, taken when the values are set

in mpmath at 50 digits and in np.float64 (gomp_refs.MPA / F64).  There is no margin: every row is always active, so no row
hangs on an activity threshold and `near` is False for all of them.  A verdict is excluded when a comparison that decides it
lies within NEAR = 1e-9 of its threshold.  The goal rows follow the tilt rows, goal-major: row0 + every earlier row + 4 k + r.
The term scale of a position bound is |point| + tol + |p| + sum_j |J q_j|, of an axis bound 1 + sum_j |g_j q_j|.

The rows before the goal rows, and their part of the verdict, are grid_refs'.  The scenes of tests/test_gpu_goals.py are defined
here so that tests/test_goal_refs.py can check them on the CPU first; the ctypes declarations take the library as an argument."""
import ctypes as C
import functools
import json
import os

import numpy as np
import scipy.sparse as sp

import capsule_refs as K
import cuboid_refs as X
import dh_refs as DH
import gomp_refs as G
import grid_refs as R
import pair_refs as P
import tilt_refs as T
from osqp_solver_amd import problems as PR

NEAR = K.NEAR
E20 = K.E20
FREE = 1e30
CLASSES = ("box", "free", "axis", "zero")


def goal(ball, waypoint, frame=0, axis=(0.0, 0.0, 1.0)):
    return dict(ball=int(ball), waypoint=int(waypoint), frame=int(frame), axis=[float(v) for v in axis])


def value(point, tol, ref=(0.0, 0.0, 1.0), max_angle=np.pi / 2):
    return dict(point=[float(v) for v in point], tol=[float(v) for v in tol], ref=[float(v) for v in ref], max_angle=float(max_angle))


def threshold_angles(v):
    """The two angles whose cosines a QP's goal holds, formed in fp64 as the host forms them: max_angle, min(pi, max_angle + 1e-3)."""
    ma = np.float64(v["max_angle"])
    return float(ma), float(min(np.float64(np.pi), ma + np.float64(G.ERROR)))


def thresholds(v, K_=G.MPA):
    """(cos_lim, cos_ok) in K_'s numbers.  They are fp64 numbers handed on as data: the mpmath kit takes the correctly rounded
    cosine of the fp64 angle, the fp64 kit np.cos (tilt_refs.thresholds)."""
    if K_ is G.MPA:
        return tuple(K_.num(float(G.MP.cos(G.MP.mpf(a)))) for a in threshold_angles(v))
    return tuple(K_.num(K_.cos(K_.num(a))) for a in threshold_angles(v))


# ------------------------------------------------------------------ the four rows of one goal

def goal_rows(chain, balls, gl, v, traj, D, K_=G.MPA, cache=None):
    """The four rows of goal `gl` with the values `v` on trajectory `traj`: a list of four dicts with vals[D], l, u, l_scale,
    u_scale, cls, and the comparisons of the verdict as dicts (kind "goal_pos" / "goal_axis", slack in K_'s numbers)."""
    num = K_.num
    w = gl["waypoint"]
    qf = traj[w * D:(w + 1) * D]
    q = [num(x) for x in qf]
    p, J = G.fk_jac(balls[gl["ball"]], qf, w, K_, cache)
    rows, comps = [], []
    err = num(G.ERROR)
    for ax in range(3):
        Jq = sum((J[ax][j] * q[j] for j in range(D)), num(0))
        pt, tol = num(v["point"][ax]), num(v["tol"][ax])
        vals = [float(J[ax][j]) for j in range(D)]
        if v["tol"][ax] >= FREE:
            rows.append(dict(vals=vals, l=-G.INF, u=G.INF, l_scale=0.0, u_scale=0.0, cls="free"))
            continue
        low, upp = ((pt - tol) - p[ax]) + Jq, ((pt + tol) - p[ax]) + Jq
        scale = abs(pt) + tol + abs(p[ax]) + sum((abs(J[ax][j] * q[j]) for j in range(D)), num(0))
        rows.append(dict(vals=vals, l=float(low), u=float(upp), l_scale=float(scale), u_scale=float(scale), cls="box"))
        comps.append(dict(kind="goal_pos", ax=ax, slack=(tol + err) - abs(p[ax] - pt)))
    if gl["frame"] == 0:
        rows.append(dict(vals=[0.0] * D, l=-G.INF, u=G.INF, l_scale=0.0, u_scale=0.0, cls="zero"))
    else:
        rots = DH.chain_frames(chain, qf, K_)[1]
        c, _, g = T.tilt_cosine(rots, dict(frame=gl["frame"], axis=gl["axis"], ref=v["ref"]), K_)
        cos_lim, cos_ok = thresholds(v, K_)
        gq = sum((g[j] * q[j] for j in range(D)), num(0))
        scale = 1 + sum((abs(g[j] * q[j]) for j in range(D)), num(0))
        rows.append(dict(vals=[float(x) for x in g], l=float((cos_lim - c) + gq), u=G.INF, l_scale=float(scale), u_scale=0.0, cls="axis", c=float(c)))
        comps.append(dict(kind="goal_axis", ax=-1, slack=c - cos_ok))
    return rows, comps


_CACHE = {}


def with_obstacles(D, W, chain, balls, lines, capsules, cuboids, pairs, tilts, grids, goals, values, con_lo, con_hi, traj, margin=G.MARGIN, K_=G.MPA):
    """grid_refs.with_obstacles with the four rows of every goal behind the tilt rows, goal-major; values[k]: what this QP asks of
    goal k.  The arrays over the rows are those of grid_refs (for a goal row: cls "box" / "free" / "axis" / "zero", ball = the
    goal's ball, w = its waypoint, near False) with "goal" (the goal's index, -1 for the other rows) besides; ok / causes (with
    "goal") / verdict_excluded / margins cover the whole acceptance test; goal_rows0 = the rows before the first goal row."""
    traj = np.ascontiguousarray(traj, np.float64)
    key = (D, W, json.dumps([chain, [{k: v for k, v in b.items() if k != "chain"} for b in balls], lines, capsules, cuboids, pairs, tilts, grids, goals, values,
                             None if con_lo is None else list(con_lo), None if con_hi is None else list(con_hi)]), traj.tobytes(), K_.name, margin)
    if key in _CACHE:
        return _CACHE[key]
    base = R.with_obstacles(D, W, chain, balls, lines, capsules, cuboids, pairs, tilts, grids, con_lo, con_hi, traj, margin, K_)
    num = K_.num
    nb = len(base["l"])
    keys = ("l", "u", "l_scale", "u_scale", "cls", "ball", "w", "pair", "near", "tilt", "c", "grid", "inside", "phi")
    rows = {k: list(base[k]) for k in keys}
    rows["vals"] = [list(r) for r in base["vals"]]
    rows["goal"] = [-1] * nb
    comparisons = []
    ok_goal, uncertain, definite = True, False, False
    cache = {}
    assert len(values) == len(goals)
    for k, (gl, v) in enumerate(zip(goals, values)):
        assert 0 <= gl["ball"] < len(balls) and 0 <= gl["waypoint"] < W
        four, comps = goal_rows(chain, balls, gl, v, traj, D, K_, cache)
        for e in four:
            rows["vals"].append(e["vals"]); rows["l"].append(e["l"]); rows["u"].append(e["u"])
            rows["l_scale"].append(e["l_scale"]); rows["u_scale"].append(e["u_scale"])
            rows["cls"].append(e["cls"]); rows["ball"].append(gl["ball"]); rows["w"].append(gl["waypoint"]); rows["pair"].append(-1)
            rows["near"].append(False); rows["tilt"].append(-1); rows["c"].append(e.get("c", np.nan))
            rows["grid"].append(-1); rows["inside"].append(False); rows["phi"].append(np.nan); rows["goal"].append(k)
        for cmp_ in comps:
            slack = cmp_["slack"]
            near = bool(abs(slack) < num(NEAR))
            comparisons.append(dict(kind=cmp_["kind"], ball=gl["ball"], w=gl["waypoint"], idx=k, ax=cmp_["ax"], slack=float(slack), near=near))
            if slack < 0:
                ok_goal = False
            if near:
                uncertain = True
            elif slack < 0:
                definite = True
    out = {k: (v if k == "cls" else np.array(v)) for k, v in rows.items() if k != "vals"}
    out["vals"] = np.array(rows["vals"], np.float64).reshape(len(rows["l"]), D)
    out["near"] = np.array(rows["near"], bool)
    definite = definite or (not base["ok"] and not base["verdict_excluded"])
    uncertain = uncertain or base["verdict_excluded"]
    causes = set(base["causes"]) | ({"goal"} if not ok_goal else set())
    out.update(margins=base["margins"] + comparisons, ok=bool(base["ok"] and ok_goal), ok_goal=ok_goal, causes=causes,
               verdict_excluded=bool(uncertain and not definite), block_rows=base["block_rows"], tilt_rows0=base["tilt_rows0"], goal_rows0=nb)
    _CACHE[key] = out
    return out


# ------------------------------------------------------------------ the scenes of the GPU tests

H = DH.H
B = 8


def _unit(v):
    v = np.asarray(v, float)
    return (v / np.sqrt(v @ v)).tolist()


# scene G7: tilt_refs' T7 (the 7-joint chain, 40 waypoints, 7 balls, 14 pairs, 7 tilts) with a goal of the gripper ball and the
# z axis of frame 7 at waypoint 37 = W - 3 and a position-only goal of ball 3 at waypoint 20; every QP asks something else
G7_GOALS = [goal(6, 37, 7, (0, 0, 1)), goal(3, 20)]


def _random_values(seed, goals, chain, balls, trajs, D):
    """Per QP and goal: a point near where the ball is on that QP's trajectory (so some boxes hold and some do not), half widths
    from {0, 1/128, 1/16, free}, a reference direction near where the axis points and a cone that sometimes holds."""
    rng = np.random.default_rng(seed)
    out = []
    for b, t in enumerate(trajs):
        per = []
        kind = b % 2 == 0                                          # the even QPs ask what their trajectory nearly gives
        for gl in goals:
            w = gl["waypoint"]
            qf = t[w * D:(w + 1) * D]
            p, _ = G.fk_jac(balls[gl["ball"]], qf, w, G.F64, None)
            point = [float(p[ax]) + float(rng.choice([0.0, 0.004, -0.006] if kind else [0.0, 0.004, -0.05, 0.3])) for ax in range(3)]
            tol = [float(rng.choice([1 / 128, 1 / 16, FREE] if kind else [0.0, 1 / 128, 1 / 16, FREE])) for _ in range(3)]
            if gl["frame"] >= 1:
                rots = DH.chain_frames(chain, qf, G.F64)[1]
                u = [float(sum(rots[gl["frame"]][r][c] * gl["axis"][c] for c in range(3))) for r in range(3)]
                ref = _unit(np.array(u) + rng.uniform(-0.6, 0.6, 3) * (0.2 if kind else 1.0))
                ma = float(rng.uniform(0.5, 1.2) if kind else rng.uniform(0.2, 1.2))
            else:
                ref, ma = _unit(rng.uniform(-1, 1, 3)), float(rng.uniform(0.2, 3.0))
            per.append(value(point, tol, ref, ma))
        out.append(per)
    return out


# scene G8: 8 joints, 2 waypoints, one ball of frame 8; goals at waypoints 0 and 1, one with frame 8 (the last joint) and one
# with frame 1 (a one-column gradient)
G8_GOALS = [goal(0, 0, 8, (0.28, 0, 0.96)), goal(0, 1, 1, (0.6, 0.0, 0.8))]

# scene GF, the flips: three joints, the TABLE ball with the identity table (p = q) and a chain whose frame 2 depends on joints 0
# and 1 only: alpha_0 = pi / 2, so the axis (0, 1, 0) of frame 2 makes the angle |q_1| with +z.  Goal 0 (waypoint 1) has that
# axis, goal 1 (waypoint 2) is about the position alone.
CF3 = DH.chain((0, 0, 0), (0, 0, 0), (H, 0, 0), (0, 0, 0))
GF_W = 4
GF_GOALS = [goal(0, 1, 2, (0, 1, 0)), goal(0, 2)]
GF_TOL, GF_MAX = 1 / 64, 0.5
GF_BASE = np.array([[0.25, 1 / 16, -0.5], [0.375, 1 / 16, -0.25], [0.5, 0.125, 0.125], [0.5, 0.125, 0.125]])


def _gf():
    """(trajectories, values) of scene GF.  QP b: what flips, and which way."""
    k_pos, k_ang = GF_TOL + G.ERROR, GF_MAX + G.ERROR
    trajs, vals = [], []
    free = [FREE] * 3

    def case(q1_w1, err, tol1, tol0=free, off0=(0.0, 0.0, 0.0)):
        p = GF_BASE.copy()
        p[:, 0] += len(trajs) / 32                                # every QP its own trajectory
        p[1, 1] = q1_w1
        trajs.append(G._with_velocities(p))
        vals.append([value([p[1, ax] + off0[ax] for ax in range(3)], tol0, (0, 0, 1), GF_MAX),
                     value([p[2, ax] + err[ax] for ax in range(3)], tol1, (0, 0, 1), 1.0)])

    tol = [GF_TOL] * 3
    case(1 / 16, (k_pos - E20, 0, 0), tol)                        # 0: x off by tol + 1e-3 - 2^-20: accepted
    case(1 / 16, (k_pos + E20, 0, 0), tol)                        # 1: ... + 2^-20: rejected, by that axis alone
    case(1 / 16, (0, -(k_pos - E20), 0), tol)                     # 2: y, the other side: accepted
    case(1 / 16, (0, 0, -(k_pos + E20)), tol)                     # 3: z, the other side: rejected
    case(k_ang - E20, (0, 0, 0), tol)                             # 4: the angle at max_angle + 1e-3 - 2^-20: accepted
    case(-(k_ang + E20), (0, 0, 0), tol)                          # 5: ... + 2^-20 on the other side of the cone: rejected
    case(1 / 16, (7.0, 0, 0.004), [FREE, GF_TOL, GF_TOL])         # 6: x free and far off: accepted
    case(1 / 16, (G.ERROR - E20, 0, -(G.ERROR + E20)), [0.0] * 3,  # 7: tol = 0, equalities: x inside the 1 mm, z outside: rejected;
         tol0=[0.0, FREE, 0.0], off0=(G.ERROR - E20, 0.5, 0.0))   # goal 0: equalities in x and z, inside
    return np.array(trajs), vals


# scene GX, exact: the TABLE ball with the identity table and tilt_refs' chain CE (alpha = 0 and theta0 = -q in joints 0 and 1, so
# R_1 = R_2 = I in fp64 at every waypoint; joint 2 moves freely, dyadic).  Every number of the position rows is dyadic; c, g and
# g q of the axis rows need no rounding, cos_lim - c is exact (cos_lim within a factor 2 of c) and the one sum behind it rounds
# once: compared bit for bit.  Six waypoints: the QPs pin waypoint 0 and waypoints 3 .. 5, so the goals of waypoints 1 and 2 leave
# the solver something to choose.  Goal 0: the x axis of frame 2 at waypoint 1; goal 1: position only (frame 0: the zero row) at
# waypoint 2; goal 2: the y axis of frame 1 at waypoint 3, for the antiparallel case.
GX_W = 6
GX_GOALS = [goal(0, 1, 2, (1, 0, 0)), goal(0, 2), goal(0, 3, 1, (0, 1, 0))]
GX_ANGLES = (1.0, 0.75, 0.9375, 0.5, 1.0, 0.6875, 0.875, 0.9375)
GX_ANTI = 5                                                     # the QP whose goal 2 points away from its ref


def _gx_trajectories():
    rng = np.random.default_rng(23)
    out = []
    for _ in range(B):
        p = np.empty((GX_W, 3))
        p[:, 0], p[:, 1] = T.TE_Q
        p[:, 2] = rng.integers(-16, 17, GX_W) / 32.0
        out.append(p)
    return np.array([G._with_velocities(p) for p in out])


def _gx():
    trajs = _gx_trajectories()
    vals = []
    for b, t in enumerate(trajs):
        q = t[:3 * GX_W].reshape(GX_W, 3)
        ref0 = (0.6, 0.8, 0.0) if b % 2 == 0 else (0.8, 0.6, 0.0)
        tol = [[0.25, 0.0, FREE], [0.5, 0.125, 0.0625], [FREE, FREE, 2.0], [0.0, 0.0, 0.0]][b % 4]
        off = [(b - 3) / 16, (b % 3) / 32, -(b % 2) / 8]
        vals.append([value(q[1] + np.array(off), tol, ref0, GX_ANGLES[b]),
                     value(q[2] - np.array(off), tol[::-1]),
                     value(q[3], [FREE] * 3, (0.0, -1.0, 0.0) if b == GX_ANTI else (-0.8, 0.6, 0.0), 1.0 if b % 2 else 0.9375)])
    return trajs, vals


# scene GM, the row order: tilt_refs' TM (a gripper ball's work-space rows, two lines, a capsule, a cuboid, two pairs, two tilts on
# the 3-joint chain of dh_refs) with grid_refs' GM grid and two goals behind them all
GM_GOALS = [goal(0, 1, 3, (0, 0, 1)), goal(1, 2, 1, (0, 0.6, 0.8))]

SCENES = ("G7", "G8", "GF", "GX", "GM")
EXACT = ("GX",)


@functools.lru_cache(maxsize=None)
def scene(name):
    """name: one of SCENES.  A dict as grid_refs.scene gives, with "goals" and "values" ([QP][goal]) besides."""
    none = dict(lines=[], capsules=[], cuboids=[], pairs=[], tilts=[], grids=[], con_lo=None, con_hi=None, margin=G.MARGIN)
    if name == "G7":
        s = dict(T.scene("T7"), name=name, grids=[], goals=G7_GOALS)
        return dict(s, values=_random_values(71, G7_GOALS, s["chain"], s["balls"], s["trajs"], s["D"]))
    if name == "G8":
        s = dict(none, name=name, D=8, W=2, chain=DH.C8, balls=[DH.chain_ball(DH.C8, 8, (0, 0, 0.02), 0, 0.04)], goals=G8_GOALS, trajs=DH._c8_trajectories())
        return dict(s, values=_random_values(81, G8_GOALS, s["chain"], s["balls"], s["trajs"], 8))
    if name == "GF":
        trajs, vals = _gf()
        return dict(none, name=name, D=3, W=GF_W, chain=CF3, balls=[G._ball(G.TABLE, 0, 1 / 16, K.IDENTITY)], goals=GF_GOALS, trajs=trajs, values=vals)
    if name == "GX":
        trajs, vals = _gx()
        return dict(none, name=name, D=3, W=GX_W, chain=T.CE, balls=[G._ball(G.TABLE, 0, 1 / 16, K.IDENTITY)], goals=GX_GOALS, trajs=trajs, values=vals)
    if name == "GM":
        s = dict(T.scene("TM"), name=name, grids=[R.gm_grid()], goals=GM_GOALS)
        return dict(s, values=_random_values(91, GM_GOALS, s["chain"], s["balls"], s["trajs"], s["D"]))
    raise KeyError(name)


def reference(s, b, K_=G.MPA, values=None, traj=None):
    """with_obstacles of trajectory b of scene dict `s` with QP b's values (or `values` / `traj` in their place)."""
    return with_obstacles(s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["pairs"], s["tilts"], s["grids"], s["goals"],
                          s["values"][b] if values is None else values, s["con_lo"], s["con_hi"], s["trajs"][b] if traj is None else traj, s["margin"], K_)


@functools.lru_cache(maxsize=None)
def scene_reference(name, K_=G.MPA):
    """Trajectory b with the values of QP b, b = 0 .. 7."""
    s = scene(name)
    return [reference(s, b, K_) for b in range(B)]


@functools.lru_cache(maxsize=None)
def fp64_error(name):
    """dh_refs.fp64_error for the scenes of this module: the np.float64 evaluation of the formulas against the mpmath one."""
    ev = eb = 0.0
    for hi, lo in zip(scene_reference(name), scene_reference(name, G.F64)):
        v, b = DH.row_distance(hi, lo)
        ev, eb = max(ev, v), max(eb, b)
    return ev, eb


def gpu_tolerance(name):
    """The project's rule (tilt_refs.gpu_tolerance): 32 x fp64_error, never looser than 1e-13.  (0, 0) for the exact scene."""
    ev, eb = fp64_error(name)
    return min(32 * ev, 1e-13), min(32 * eb, 1e-13)


def scene_problem(D, W, balls, n_per_ball, n_pairs, goals, n_qps, over_allocate, starts=None, ends=None, seed=4100):
    """pair_refs.scene_problem with four rows a goal behind the pair (and tilt) rows, each with entries in the columns of its goal's
    waypoint.  over_allocate: the all-zero rows of ConstraintBuilder's allocation come after the goal rows."""
    row0, block_rows = G.row_layout(D, W, balls, n_per_ball)
    rows3d = block_rows + W * n_pairs + 4 * len(goals)
    m = row0 + (D * W * (3 + n_per_ball * len(balls)) + W * n_pairs + 4 * len(goals) if over_allocate else rows3d)
    n = 2 * D * W
    rng = np.random.default_rng(seed)
    starts = rng.uniform(-1, 1, (n_qps, D)) if starts is None else np.asarray(starts, float)
    ends = rng.uniform(-1, 1, (n_qps, D)) if ends is None else np.asarray(ends, float)
    q_lim, v_lim, a_lim, ts = 2 * np.pi, np.pi, np.pi * 800 / 180, 0.1
    pos_con = PR.in_range(np.full(D, -q_lim), np.full(D, q_lim))
    vel_con = PR.scaled(PR.in_range(np.full(D, -v_lim), np.full(D, v_lim)), ts)
    acc_con = PR.scaled(PR.in_range(np.full(D, -a_lim), np.full(D, a_lim)), ts * ts)
    zero = PR.equal(np.zeros(D))
    r3, c3 = [], []
    r = row0

    def row_at(w):
        nonlocal r
        r3.extend([r] * D)
        c3.extend(range(w * D, (w + 1) * D))
        r += 1

    for ball in balls:
        for w in range(W):
            for _ in range((3 if ball["gripper"] else 0) + n_per_ball):
                row_at(w)
    for _ in range(n_pairs):
        for w in range(W):
            row_at(w)
    for gl in goals:
        for _ in range(4):
            row_at(gl["waypoint"])
    assert r == row0 + rows3d
    A0, ls, us, Axs, aidx = None, [], [], [], None
    for b in range(n_qps):
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
        ls.append(np.concatenate([l[:row0], np.full(m - row0, -G.INF)]))
        us.append(np.concatenate([u[:row0], np.full(m - row0, G.INF)]))
    Pm = sp.csc_matrix(PR.tri_diagonal_matrix(2.0, -1.0, n, D * W, D))
    Pm.sort_indices()
    return dict(n=n, m=m, P=Pm, A=A0, Px=np.tile(Pm.data, (n_qps, 1)), Ax=np.array(Axs), q=None, l=np.array(ls), u=np.array(us),
                row0=row0, rows3d=rows3d, block_rows=block_rows, aidx=aidx, starts=starts, ends=ends)


@functools.lru_cache(maxsize=None)
def scene_batch(name, over_allocate=False, with_goals=True):
    """scene_problem for the scene's eight trajectories (with_goals False: the same scene without its goal rows)."""
    s = scene(name)
    D, W = s["D"], s["W"]
    starts = s.get("starts", s["trajs"][:, :D])
    ends = (s["starts"] if "starts" in s else s["trajs"][:, (W - 3) * D:(W - 2) * D]) if W >= 4 else None
    return scene_problem(D, W, s["balls"], len(s["lines"]) + len(s["capsules"]) + len(s["cuboids"]) + len(s["grids"]), len(s["pairs"]) + len(s["tilts"]),
                         s["goals"] if with_goals else [], B, over_allocate, starts=starts, ends=ends)


def populations(name):
    """Counts a test can assert on and print: goal rows per class, rejecting comparisons per kind, verdicts, causes, exclusions."""
    ref = scene_reference(name)
    cells = {c: 0 for c in CLASSES}
    rejecting = dict(goal_pos=0, goal_axis=0)
    for e in ref:
        for k in range(len(e["l"])):
            if e["goal"][k] >= 0:
                cells[e["cls"][k]] += 1
        for m in e["margins"]:
            if m["kind"] in rejecting:
                rejecting[m["kind"]] += bool(m["slack"] < 0)
    return dict(cells=cells, rejecting=rejecting, goal_rows=sum(cells.values()), accepted=sum(e["ok"] for e in ref), rejected=sum(not e["ok"] for e in ref),
                accepted_by_the_goals=sum(e["ok_goal"] for e in ref), rejected_by_a_goal_alone=sum(e["causes"] == {"goal"} for e in ref),
                verdicts_excluded=sum(e["verdict_excluded"] for e in ref),
                near_comparisons=sum(m["near"] for e in ref for m in e["margins"] if m["kind"] in rejecting),
                near_rows=sum(int(e["near"][e["goal"] >= 0].sum()) for e in ref))


# ------------------------------------------------------------------ the known answers in tests/golden/goal_kats.json

KAT_SCENES = ("GF", "GX", "GM")


def kats_now():
    """What tests/golden/goal_kats.json holds, computed now: per scene the goals and per QP its values, its trajectory, the four rows
    of every goal (vals, l, u as JSON numbers: the shortest decimal that reads back as the same double), the verdict of the goals
    alone and of the whole scene, by the mpmath reference."""
    out = {}
    for name in KAT_SCENES:
        s = scene(name)
        cases = []
        for b, e in enumerate(scene_reference(name)):
            g0 = e["goal_rows0"]
            cases.append(dict(values=s["values"][b], traj=[float(x) for x in s["trajs"][b]], vals=[[float(x) for x in row] for row in e["vals"][g0:]],
                              l=[float(x) for x in e["l"][g0:]], u=[float(x) for x in e["u"][g0:]], ok_goal=bool(e["ok_goal"]), ok=bool(e["ok"]),
                              rows_before=int(g0)))
        out[name] = dict(goals=s["goals"], cases=cases)
    return out


def kats_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "goal_kats.json")


def load_kats():
    with open(kats_path()) as f:
        return json.load(f)


# ------------------------------------------------------------------ ctypes: mi_gomp_scene_create_goals, _set_goal_values (tests only)

class Goal(C.Structure):
    _fields_ = [("ball", C.c_int32), ("waypoint", C.c_int32), ("frame", C.c_int32), ("reserved", C.c_int32), ("axis", C.c_double * 3)]


class GoalValue(C.Structure):
    _fields_ = [("point", C.c_double * 3), ("tol", C.c_double * 3), ("ref", C.c_double * 3), ("max_angle", C.c_double)]


def c_goals(goals):
    arr = (Goal * max(len(goals), 1))()
    for k, gl in enumerate(goals):
        arr[k].ball, arr[k].waypoint, arr[k].frame = gl["ball"], gl["waypoint"], gl["frame"]
        for i in range(3):
            arr[k].axis[i] = gl["axis"][i]
    return arr


def c_values(values):
    """values: [QP][goal] dicts -> a flat array, QP-major."""
    flat = [v for per in values for v in per]
    arr = (GoalValue * max(len(flat), 1))()
    for k, v in enumerate(flat):
        arr[k].max_angle = v["max_angle"]
        for i in range(3):
            arr[k].point[i], arr[k].tol[i], arr[k].ref[i] = v["point"][i], v["tol"][i], v["ref"][i]
    return arr


def declare(L):
    R.declare(L)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    L.mi_gomp_scene_create_goals.argtypes = [C.POINTER(vp), vp, C.c_int64, C.c_int64, C.POINTER(DH.Chain), C.c_int64, C.POINTER(G.Ball), C.c_int64,
                                             C.POINTER(G.Line), C.c_int64, C.POINTER(K.Capsule), C.c_int64, C.POINTER(X.Cuboid), C.c_int64, C.POINTER(P.Pair),
                                             C.c_int64, C.POINTER(T.Tilt), C.c_int64, C.POINTER(R.Grid), C.c_int64, C.POINTER(Goal), dp, dp]
    L.mi_gomp_scene_create_goals.restype = C.c_int
    L.mi_gomp_scene_set_goal_values.argtypes = [vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(GoalValue)]
    L.mi_gomp_scene_set_goal_values.restype = C.c_int
    return L


def create_goals(L, handle, D, W, ch, balls, lines, capsules, cuboids, pairs, tilts, grids, goals, con_lo=None, con_hi=None, n_goals=None, null_goals=False,
                 null_out=False):
    """(rc, scene pointer) of mi_gomp_scene_create_goals; ch: a Chain, a chain dict or None.  n_goals / null_goals / null_out
    override what is passed (the refusals).  The pointer starts as a value that is not NULL, so a refusal shows that it was
    cleared."""
    ptr = C.c_void_p(1)
    lo = None if con_lo is None else np.ascontiguousarray(con_lo, np.float64)
    hi = None if con_hi is None else np.ascontiguousarray(con_hi, np.float64)
    cc = DH.c_chain(ch) if isinstance(ch, dict) else ch
    arr, keep = R.c_grids(grids)
    rc = L.mi_gomp_scene_create_goals(None if null_out else C.byref(ptr), handle, D, W, None if cc is None else C.byref(cc), len(balls), G.c_balls(balls),
                                      len(lines), G.c_lines(lines), len(capsules), K.c_capsules(capsules), len(cuboids), X.c_cuboids(cuboids),
                                      len(pairs), P.c_pairs(pairs), len(tilts), T.c_tilts(tilts), len(grids), arr,
                                      len(goals) if n_goals is None else n_goals, None if null_goals else c_goals(goals), G._dp(lo), G._dp(hi))
    del keep
    return rc, ptr


class GoalScene(G.GompScene):
    """gomp_refs.GompScene made by mi_gomp_scene_create_goals."""

    def __init__(self, L, solver, s, goals=None):
        self.L, self.solver = declare(L), solver
        self.rc, self.ptr = create_goals(L, solver._h, s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["pairs"],
                                         s["tilts"], s["grids"], s["goals"] if goals is None else goals, s["con_lo"], s["con_hi"])

    def set_goal_values(self, ids, values):
        ids, p = G._ids(ids)
        return self.L.mi_gomp_scene_set_goal_values(self.ptr, len(ids), p, c_values(values))
