"""Cuboid obstacles (mi_gomp_cuboid, CuboidObstacle) beside tests/capsule_refs.py, tests/gomp_refs.py and tests/dh_refs.py: a
helper module of the tests, not a conftest.

A cuboid is an oriented box - centre o, orthonormal axes u_0, u_1, u_2 (the rows of `axes`), half extents h_k >= 0 - swept by a
sphere of radius R.  For a ball with centre p = fk(q_w), radius r and 3 x D position Jacobian J (include/mi_osqp.h has the same
definition, restated here from it alone):

    d_k   = p_k - o_k
    y_k   = u_k0 d_0 + u_k1 d_1 + u_k2 d_2
    c_k   = min(h_k, max(-h_k, y_k))
    v_k   = y_k - c_k,  out = sqrt(v_0^2 + v_1^2 + v_2^2)
    out > 1e-12:  sd = out,  nl_k = v_k / out
    otherwise:    slack_k = h_k - |c_k|,  k* = the smallest k with slack_k = min(slack),  sd = -slack_k*,
                  nl = e_k* times (c_k* < 0 ? -1 : +1)
    n_i   = nl_0 u_0i + nl_1 u_1i + nl_2 u_2i
    reach = R + r,  s = sd - reach
    g_j   = n_x J[x][j] + n_y J[y][j] + n_z J[z][j]                     written whether the row is active or not
    s < margin:  l = (reach - sd) + sum_j g_j q_w[j],  u = +1e30          otherwise  l = -1e30, u = +1e30
    accepted only if s >= -ERROR at every (ball, waypoint, cuboid)

in mpmath at 50 digits and in np.float64 (gomp_refs.MPA / F64).  The box, line and capsule rows and their part of the verdict
are capsule_refs' (with gomp_refs and dh_refs behind it); this module computes the cuboid rows and merges them in the
library's row order: per ball and waypoint the three work-space rows of a gripper ball, the lines, the capsules, then the
cuboids.

A row is `near` when it hangs on a threshold: |s - margin| below NEAR, `out` nonzero and below NEAR, and in the inside case
a nonzero gap between the two smallest slacks below NEAR or a nonzero |c_k*| below NEAR (the side of the face).  A gap or a
c_k* of exactly zero is not a threshold but the tie rule itself (the lowest axis, the + side): scene XT pins it with numbers
that are exact in fp64.

The scenes of tests/test_gpu_cuboids.py are defined here so that tests/test_cuboid_refs.py can check their populations on the
CPU first; the ctypes declarations of mi_gomp_scene_create_cuboids take the library as an argument."""
import ctypes as C
import functools
import json
import os

import numpy as np

import capsule_refs as K
import dh_refs as DH
import gomp_refs as G

NEAR = K.NEAR
CLASSES = ("active", "none")
REGIONS = ("face", "edge", "corner", "inside")        # 1, 2, 3 coordinates of p beyond the half extents; none (out <= 1e-12)
AXIS_ALIGNED = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def cuboid(centre, half, radius=0.0, margin=0.0, axes=AXIS_ALIGNED):
    return dict(centre=[float(v) for v in centre], axes=[float(v) for v in axes], half=[float(v) for v in half], radius=float(radius),
                margin=float(margin))


def rotation(rz, ry, rx=0.0):
    """The rows of Rz(rz) Ry(ry) Rx(rx) transposed, i.e. the axes of a box turned by these angles: nine doubles, orthonormal to a
    few 1e-17."""
    cz, sz, cy, sy, cx, sx = np.cos(rz), np.sin(rz), np.cos(ry), np.sin(ry), np.cos(rx), np.sin(rx)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return [float(v) for v in (Rz @ Ry @ Rx).T.reshape(-1)]


def capsule_as_cuboid(cap):
    """The cuboid that is the capsule `cap` (a != b): half = (|b - a| / 2, 0, 0), u_0 along b - a, centre (a + b) / 2, radius R.
    u_1, u_2 complete u_0 to an orthonormal frame (they multiply zero half extents and enter the rows only through v)."""
    a, b = np.array(cap["a"]), np.array(cap["b"])
    e = b - a
    ln = float(np.sqrt(e @ e))
    u0 = e / ln
    t = np.eye(3)[int(np.argmin(np.abs(u0)))]
    u1 = t - (t @ u0) * u0
    u1 /= np.sqrt(u1 @ u1)
    u2 = np.cross(u0, u1)
    return cuboid((a + b) / 2, (ln / 2, 0.0, 0.0), cap["radius"], cap["margin"], list(u0) + list(u1) + list(u2))


# ------------------------------------------------------------------ one cuboid row

def probe(cub, p, K_=G.MPA):
    """(sd, n, region, out, slack_gap, c_star): signed distance from the sharp box, world normal, which of REGIONS, the distance
    outside, in the inside case the gap between the two smallest slacks and the c of the chosen axis (else None)."""
    num = K_.num
    o, u, h = [num(v) for v in cub["centre"]], [num(v) for v in cub["axes"]], [num(v) for v in cub["half"]]
    d = [p[k] - o[k] for k in range(3)]
    y = [u[3 * k] * d[0] + u[3 * k + 1] * d[1] + u[3 * k + 2] * d[2] for k in range(3)]
    c = [min(h[k], max(-h[k], y[k])) for k in range(3)]
    v = [y[k] - c[k] for k in range(3)]
    out = K_.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    gap = c_star = None
    if out > num(1e-12):
        sd = out
        nl = [v[k] / out for k in range(3)]
        region = REGIONS[sum(1 for k in range(3) if v[k] != 0) - 1]
    else:
        slack = [h[k] - abs(c[k]) for k in range(3)]
        ks = 0
        for k in (1, 2):
            if slack[k] < slack[ks]:
                ks = k
        sd = -slack[ks]
        nl = [num(0), num(0), num(0)]
        nl[ks] = num(-1) if c[ks] < 0 else num(1)
        srt = sorted(slack)
        gap, c_star, region = srt[1] - srt[0], c[ks], "inside"
    n = [nl[0] * u[i] + nl[1] * u[3 + i] + nl[2] * u[6 + i] for i in range(3)]
    return sd, n, region, out, gap, c_star


def cuboid_row(cub, p, J, q, r, K_=G.MPA):
    """The row of one (ball, waypoint, cuboid): a dict with vals[D], l, u, l_scale, cls, region, near, s (the clearance), out and
    dn = |p - o| (for the capsule cross-check)."""
    num = K_.num
    D = len(q)
    sd, n, region, out, gap, c_star = probe(cub, p, K_)
    reach = num(cub["radius"]) + r
    s = sd - reach
    g = [n[0] * J[0][j] + n[1] * J[1][j] + n[2] * J[2][j] for j in range(D)]
    gq = sum((g[j] * q[j] for j in range(D)), num(0))
    margin = num(cub["margin"])
    active = s < margin
    near = abs(s - margin) < num(NEAR) or (out != 0 and out < num(NEAR))
    if region == "inside":
        near = near or (gap != 0 and gap < num(NEAR)) or (c_star != 0 and abs(c_star) < num(NEAR))
    low = (reach - sd) + gq if active else -num(G.INF)
    scale = reach + abs(sd) + sum((abs(g[j] * q[j]) for j in range(D)), num(0)) if active else num(0)
    o = [num(v) for v in cub["centre"]]
    dn = K_.sqrt(sum(((p[k] - o[k]) * (p[k] - o[k]) for k in range(3)), num(0)))
    return dict(vals=[float(x) for x in g], l=float(low), u=G.INF, l_scale=float(scale), cls="active" if active else "none", region=region,
                near=bool(near), s=float(s), s_hi=s, out=float(out), dn=float(dn))


# ------------------------------------------------------------------ rows and verdict of a scene

_CACHE = {}


def _evaluate(D, W, balls, lines, capsules, cuboids, con_lo, con_hi, traj, K_, margin):
    traj = np.ascontiguousarray(traj, np.float64)
    key = (D, W, json.dumps([[{k: v for k, v in b.items() if k != "chain"} for b in balls], lines, capsules, cuboids,
                             None if con_lo is None else list(con_lo), None if con_hi is None else list(con_hi)]),
           id(balls[0].get("chain")) if balls else 0, traj.tobytes(), K_.name, margin)
    if key in _CACHE:
        return _CACHE[key]
    base = K.with_obstacles(D, W, balls, lines, capsules, con_lo, con_hi, traj, margin, K_)
    num, mg, err = K_.num, K_.num(margin), K_.num(G.ERROR)
    nl, nc, nx = len(lines), len(capsules), len(cuboids)
    keys = ("l", "u", "l_scale", "u_scale", "cls", "ball", "w", "kind", "near", "clamp", "s")
    rows = {k: [] for k in keys + ("vals", "region", "out", "dn")}
    comparisons = []
    ok_cub, uncertain, definite = True, False, False
    cache = {}
    src = 0                                                  # next row of `base`
    for bi, ball in enumerate(balls):
        r = num(ball["radius"])
        for w in range(W):
            for _ in range((3 if ball["gripper"] else 0) + nl + nc):
                for k in keys:
                    rows[k].append(base[k][src])
                rows["vals"].append(base["vals"][src])
                rows["region"].append(None); rows["out"].append(np.nan); rows["dn"].append(np.nan)
                src += 1
            if not nx:
                continue
            qf = traj[w * D:(w + 1) * D]
            p, J = G.fk_jac(ball, qf, w, K_, cache)
            q = [num(x) for x in qf]
            for xi, cub in enumerate(cuboids):
                e = cuboid_row(cub, p, J, q, r, K_)
                rows["vals"].append(e["vals"]); rows["l"].append(e["l"]); rows["u"].append(e["u"])
                rows["l_scale"].append(e["l_scale"]); rows["u_scale"].append(0.0)
                rows["cls"].append(e["cls"]); rows["ball"].append(bi); rows["w"].append(w); rows["kind"].append(3 + nl + nc + xi)
                rows["near"].append(e["near"]); rows["clamp"].append(None); rows["s"].append(e["s"])
                rows["region"].append(e["region"]); rows["out"].append(e["out"]); rows["dn"].append(e["dn"])
                slack = e["s_hi"] + err                       # s >= -ERROR
                near = bool(abs(slack) < num(NEAR))
                comparisons.append(dict(kind="cuboid", ball=bi, w=w, idx=xi, slack=float(slack), near=near))
                if slack < 0:
                    ok_cub = False
                if near:
                    uncertain = True
                elif slack < 0:
                    definite = True
    assert src == len(base["l"])
    out = {k: (v if k in ("cls", "clamp", "region") else np.array(v)) for k, v in rows.items()}
    out["vals"] = np.array(rows["vals"], np.float64).reshape(len(rows["l"]), D)
    out["near"] = np.array(rows["near"], bool)
    definite = definite or (not base["ok"] and not base["verdict_excluded"])
    uncertain = uncertain or base["verdict_excluded"]
    causes = set(base["causes"]) | ({"cuboid"} if not ok_cub else set())
    out.update(decisions=base["decisions"], margins=base["margins"] + comparisons, ok=bool(base["ok"] and ok_cub), causes=causes,
               verdict_excluded=bool(uncertain and not definite))
    _CACHE[key] = out
    return out


def with_obstacles(D, W, balls, lines, capsules, cuboids, con_lo, con_hi, traj, margin=G.MARGIN, K_=G.MPA):
    """capsule_refs.with_obstacles with cuboid rows after the capsules of every (ball, waypoint) block.  The arrays over the rows
    are those of capsule_refs (cls "active" / "none" and kind 3 + |lines| + |capsules| + i for cuboid i), with "region" (which of
    REGIONS, None for the other rows), "out" and "dn" (nan for the other rows) besides; ok / causes (with "cuboid") /
    verdict_excluded / margins cover the whole acceptance test.  A verdict within NEAR of -ERROR is excluded."""
    return _evaluate(D, W, balls, lines, capsules, cuboids, con_lo, con_hi, traj, K_, margin)


# ------------------------------------------------------------------ the scenes of the GPU tests

E20 = K.E20
IDENTITY = K.IDENTITY
XT_O = (1.0, 0.5, 0.25)                                     # the common centre of XT's cuboids
XT_H, XT_RA, XT_MA = 1 / 4, 1 / 8, 1 / 8                   # cuboid 0: an axis-aligned cube, rounded, with a margin
XT_B_AXES = [0, 1, 0, 0, 0, 1, -1, 0, 0]                   # cuboid 1: u_0 = +y, u_1 = +z, u_2 = -x: a signed permutation, not symmetric
XT_B_THIN = 1 / 64
XT_B_HALF = (1.0, 1.0, XT_B_THIN)                          # a slab 2 x 2 in y and z, 1/32 thick in x (transposed axes: thin in y); sharp, margin 0
XT_RB, XT_RB1 = 1 / 16, 1 / 32                             # radii of balls 0 and 1
XT_FAR = 2.0
XT_ACCEPT = G.grid(XT_RA + XT_RB - G.ERROR)                # distance from cuboid 0's face at which ball 0 has s = -ERROR, on the 2^-30 grid
XP_R, XP_M, XP_RB = 1 / 8, 1 / 8, 1 / 16                   # scene XP: the point cuboid's radius and margin, the ball's radius
XP_AXES = [0, 1, 0, 0, 0, -1, 1, 0, 0]                     # u_0 = +y, u_1 = -z, u_2 = +x (left-handed)
XP_ACCEPT = G.grid(XP_R + XP_RB - G.ERROR)


def _tour(W, *special):
    p = np.tile(XT_O, (W, 1))
    p[:, 0] += XT_FAR
    for w, off in special:
        p[w] = np.array(XT_O) + np.array(off, float)
    return p


def _ax(axis, d):
    v = [0.0, 0.0, 0.0]
    v[axis] = d
    return v


def _xt_trajectories():
    """Every waypoint is either on an axis through XT_O at a dyadic distance or inside both cuboids: v has at most one nonzero
    component, so out is that component's magnitude and every row is exact in fp64 in any order of operations (all numbers on
    the 2^-30 grid below 16).  Cuboid 1 holds the plane x = o_x within 1 of the centre: an accepted trajectory stays on the x
    axis or leaves that plane's slab."""
    W = 8
    act = XT_H + XT_RA + XT_RB + XT_MA                       # |x - o_x| at which ball 0 has s = margin from cuboid 0
    b0 = XT_B_THIN + XT_RB                                # ... s = 0 from cuboid 1 (margin 0, sharp)
    out = [
        _tour(W, *[(w, _ax(w // 2, (1 - 2 * (w % 2)) * 3 / 16)) for w in range(6)]),     # 0: inside cuboid 0, nearest to +x, -x, +y, -y, +z, -z in turn
        _tour(W, (1, (0, 0, 0)), (3, (0, -1 / 8, -1 / 8)), (5, (0, 1 / 8, 1 / 8))),       # 1: at o: three-way tie; two-way ties (y and z), c_2 of cuboid 1 = -0.0
        _tour(W, (2, _ax(0, XT_H)), (4, _ax(2, -XT_H)), (6, _ax(0, XT_B_THIN))),       # 2: on the faces +x, -z of cuboid 0 and on the face of cuboid 1 (out = 0, sd = 0)
        _tour(W, (1, _ax(0, act - E20)), (4, _ax(0, -(act + E20)))),                      # 3: s = margin -+ 2^-20 (ball 0, cuboid 0): active | not; accepted
        _tour(W, (2, _ax(0, XT_H + XT_ACCEPT + E20))),                                     # 4: s = -ERROR + 2^-20: accepted
        _tour(W, (2, _ax(0, XT_H + XT_ACCEPT - E20))),                                     # 5: s = -ERROR - 2^-20: rejected, by that cuboid row alone
        _tour(W, (1, _ax(0, b0 - E20)), (3, _ax(0, -(b0 + E20)))),                        # 6: s = -+ 2^-20 of cuboid 1 (margin 0) for ball 0: active | not
        _tour(W, (0, _ax(0, -1 / 2)), (5, _ax(1, 1.5)), (6, _ax(2, -1.5))),               # 7: active from outside (-x); beyond cuboid 1's +u_0 and -u_1 faces; accepted
    ]
    return np.array([G._with_velocities(p) for p in out])


def _xp_trajectories():
    """As XT: every waypoint on an axis through the point cuboid's centre at a dyadic distance."""
    W = 4
    act = XP_R + XP_RB + XP_M
    out = [
        _tour(W, (1, (0, 0, 0))),                                                          # 0: on the point: out = 0, normal +u_0 = +y
        _tour(W, (1, _ax(0, act - E20)), (2, _ax(0, -(act + E20)))),                      # 1: s = margin -+ 2^-20
        _tour(W, (1, _ax(2, XP_ACCEPT + E20))),                                            # 2: s = -ERROR + 2^-20: accepted
        _tour(W, (1, _ax(2, XP_ACCEPT - E20))),                                            # 3: s = -ERROR - 2^-20: rejected
        _tour(W, (2, _ax(1, 1 / 4))),                                                      # 4: active, normal +y
        _tour(W, (2, _ax(1, -1 / 4))),                                                     # 5: ... -y
        _tour(W, (1, _ax(2, 1 / 4)), (2, _ax(2, -1 / 4))),                                # 6: ... +z, -z
        _tour(W),                                                                          # 7: far from it
    ]
    return np.array([G._with_velocities(p) for p in out])


X7_CAPSULES = [K.K7_CAPSULES[1]]                                                           # the vertical post
X7_CUBOIDS = [cuboid((0.55, -0.12, 0.65), (0.09, 0.06, 0.05), 0.0, 0.05, rotation(0.5, 0.3, 0.2)),    # turned about z, y and x: in the sweep of the forearm
              cuboid((-0.7, 0.3, 0.4), (0.12, 0.1, 0.0), 0.0, 0.06),                                 # a plate (zero half extent in z)
              cuboid((0.4, 0.8, 0.35), (0.05, 0.08, 0.2), 0.03, 0.04, rotation(0.2, 0.0))]            # rounded, turned about z
X8_CUBOIDS = [cuboid((0.45, 0.55, 0.45), (0.06, 0.05, 0.08), 0.02, 0.1, rotation(0.4, -0.2, 0.3))]
XM_CAPSULES = [K.KM_CAPSULES[0]]
XM_CUBOIDS = [cuboid((0.0, 0.125, 0.25), (0.5, 0.375, 0.25), 0.0, 0.125, rotation(0.6, 0.25)),
              cuboid((0.375, -0.5, -0.25), (0.25, 0.25, 0.375), 0.125, 0.25)]


def _xm_trajectories(W):
    rng = np.random.default_rng(2310)
    out = []
    for k in range(8):
        a, b = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
        out.append(a + np.linspace(0.0, 1.0, W)[:, None] * (b - a))
    return np.array([G._with_velocities(p) for p in out])


SCENES = ("X7", "X8", "XT", "XM", "XP")
EXACT = ("XT", "XP")


@functools.lru_cache(maxsize=None)
def scene(name):
    """name: one of SCENES.  A dict as capsule_refs.scene gives, with "cuboids" besides."""
    if name == "X7":
        c7 = DH.scene("C7")
        return dict(c7, name=name, lines=[DH.LINE0], capsules=X7_CAPSULES, cuboids=X7_CUBOIDS)
    if name == "X8":
        balls = [DH.chain_ball(DH.C8, 8, (0, 0, 0.02), 0, 0.04)]
        return dict(name=name, D=8, W=2, chain=DH.C8, balls=balls, lines=[], capsules=[], cuboids=X8_CUBOIDS, con_lo=None, con_hi=None, margin=G.MARGIN,
                    trajs=DH._c8_trajectories())
    if name == "XT":
        balls = [G._ball(G.TABLE, 0, XT_RB, IDENTITY), G._ball(G.TABLE, 0, XT_RB1, IDENTITY)]
        cubs = [cuboid(XT_O, (XT_H, XT_H, XT_H), XT_RA, XT_MA), cuboid(XT_O, XT_B_HALF, 0.0, 0.0, XT_B_AXES)]
        return dict(name=name, D=3, W=8, chain=None, balls=balls, lines=[], capsules=[], cuboids=cubs, con_lo=None, con_hi=None, margin=G.MARGIN,
                    trajs=_xt_trajectories())
    if name == "XP":
        balls = [G._ball(G.TABLE, 0, XP_RB, IDENTITY)]
        cubs = [cuboid(XT_O, (0.0, 0.0, 0.0), XP_R, XP_M, XP_AXES)]
        return dict(name=name, D=3, W=4, chain=None, balls=balls, lines=[], capsules=[], cuboids=cubs, con_lo=None, con_hi=None, margin=G.MARGIN,
                    trajs=_xp_trajectories())
    if name == "XM":
        W = 4
        balls = [G._ball(G.TABLE, 1, 1 / 16, G.T_TABLES[0]), G._ball(G.TABLE, 0, 1 / 8, G.T_TABLES[1])]
        return dict(name=name, D=3, W=W, chain=None, balls=balls, lines=G.T_LINES, capsules=XM_CAPSULES, cuboids=XM_CUBOIDS,
                    con_lo=[-0.75, -G.INF, -0.875], con_hi=[G.INF, 0.875, G.INF], margin=G.MARGIN, trajs=_xm_trajectories(W))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def k7_as_cuboid():
    """Scene K7 of capsule_refs with its slanted capsule (the last) replaced by the equivalent cuboid: the capsule cross-check."""
    k7 = K.scene("K7")
    return dict(k7, name="K7X", capsules=k7["capsules"][:2], cuboids=[capsule_as_cuboid(k7["capsules"][2])])


def _scene(name):
    return k7_as_cuboid() if name == "K7X" else scene(name)


@functools.lru_cache(maxsize=None)
def scene_reference(name, K_=G.MPA):
    """with_obstacles of the scene's eight trajectories ("K7X": k7_as_cuboid())."""
    s = _scene(name)
    return [with_obstacles(s["D"], s["W"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["con_lo"], s["con_hi"], t, s["margin"], K_)
            for t in s["trajs"]]


@functools.lru_cache(maxsize=None)
def fp64_error(name):
    """dh_refs.fp64_error for the scenes of this module: the np.float64 evaluation of the formulas against the mpmath one."""
    ev = eb = 0.0
    for hi, lo in zip(scene_reference(name), scene_reference(name, G.F64)):
        v, b = DH.row_distance(hi, lo)
        ev, eb = max(ev, v), max(eb, b)
    return ev, eb


def gpu_tolerance(name):
    """The project's rule (gomp_refs.gpu_tolerance): 32 x fp64_error, never looser than 1e-13.  (0, 0) for the exact scenes."""
    ev, eb = fp64_error(name)
    return min(32 * ev, 1e-13), min(32 * eb, 1e-13)


@functools.lru_cache(maxsize=None)
def scene_batch(name, over_allocate=False):
    """gomp_refs.scene_problem for the scene's eight trajectories; a cuboid takes a row per (ball, waypoint) as a line does."""
    s = _scene(name)
    D, W = s["D"], s["W"]
    ends = s["trajs"][:, (W - 3) * D:(W - 2) * D] if W >= 4 else None
    return G.scene_problem(D, W, s["balls"], len(s["lines"]) + len(s["capsules"]) + len(s["cuboids"]), 8, over_allocate, starts=s["trajs"][:, :D], ends=ends)


def populations(name):
    """Counts a test can assert on and print: cuboid rows per (region, class) and cuboid, verdicts, causes, exclusions."""
    s, ref = _scene(name), scene_reference(name)
    nx = len(s["cuboids"])
    first = 3 + len(s["lines"]) + len(s["capsules"])
    cells = {(g, c): np.zeros(nx, int) for g in REGIONS for c in CLASSES}
    near = rows = 0
    causes = {}
    for e in ref:
        for k in range(len(e["l"])):
            near += bool(e["near"][k])
            if e["region"][k] is None:
                continue
            cells[(e["region"][k], e["cls"][k])][int(e["kind"][k]) - first] += 1
            rows += 1
        for c in e["causes"]:
            causes[c] = causes.get(c, 0) + 1
    return dict(cells=cells, near=near, cuboid_rows=rows, accepted=sum(e["ok"] for e in ref), rejected=sum(not e["ok"] for e in ref),
                causes=causes, verdicts_excluded=sum(e["verdict_excluded"] for e in ref),
                near_comparisons=sum(m["near"] for e in ref for m in e["margins"]))


# ------------------------------------------------------------------ the known answers in tests/golden/cuboid_kats.json

KAT_SCENES = ("XT", "XP", "XM")


def kats_now():
    """What tests/golden/cuboid_kats.json holds, computed now: per scene and trajectory the rows (vals, l, u as JSON numbers: the
    shortest decimal that reads back as the same double) and the verdict of the mpmath reference."""
    out = {}
    for name in KAT_SCENES:
        out[name] = [dict(vals=[[float(x) for x in row] for row in e["vals"]], l=[float(x) for x in e["l"]], u=[float(x) for x in e["u"]],
                          ok=bool(e["ok"])) for e in scene_reference(name)]
    return out


def kats_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cuboid_kats.json")


def load_kats():
    with open(kats_path()) as f:
        return json.load(f)


# ------------------------------------------------------------------ ctypes: mi_gomp_scene_create_cuboids (tests only)

class Cuboid(C.Structure):
    _fields_ = [("centre", C.c_double * 3), ("axes", C.c_double * 9), ("half", C.c_double * 3), ("radius", C.c_double), ("margin", C.c_double)]


def c_cuboids(cuboids):
    arr = (Cuboid * max(len(cuboids), 1))()
    for k, cb in enumerate(cuboids):
        for j in range(3):
            arr[k].centre[j], arr[k].half[j] = cb["centre"][j], cb["half"][j]
        for j in range(9):
            arr[k].axes[j] = cb["axes"][j]
        arr[k].radius, arr[k].margin = cb["radius"], cb["margin"]
    return arr


def declare(L):
    K.declare(L)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    L.mi_gomp_scene_create_cuboids.argtypes = [C.POINTER(vp), vp, C.c_int64, C.c_int64, C.POINTER(DH.Chain), C.c_int64, C.POINTER(G.Ball), C.c_int64,
                                               C.POINTER(G.Line), C.c_int64, C.POINTER(K.Capsule), C.c_int64, C.POINTER(Cuboid), dp, dp]
    L.mi_gomp_scene_create_cuboids.restype = C.c_int
    return L


def create_cuboids(L, handle, D, W, ch, balls, lines, capsules, cuboids, con_lo=None, con_hi=None, n_cuboids=None, null_cuboids=False):
    """(rc, scene pointer) of mi_gomp_scene_create_cuboids; ch: a Chain, a chain dict or None.  n_cuboids / null_cuboids override
    what is passed for the cuboid count and array (the refusals)."""
    ptr = C.c_void_p()
    lo = None if con_lo is None else np.ascontiguousarray(con_lo, np.float64)
    hi = None if con_hi is None else np.ascontiguousarray(con_hi, np.float64)
    cc = DH.c_chain(ch) if isinstance(ch, dict) else ch
    rc = L.mi_gomp_scene_create_cuboids(C.byref(ptr), handle, D, W, None if cc is None else C.byref(cc), len(balls), G.c_balls(balls), len(lines),
                                        G.c_lines(lines), len(capsules), K.c_capsules(capsules), len(cuboids) if n_cuboids is None else n_cuboids,
                                        None if null_cuboids else c_cuboids(cuboids), G._dp(lo), G._dp(hi))
    return rc, ptr


class CuboidScene(G.GompScene):
    """gomp_refs.GompScene made by mi_gomp_scene_create_cuboids."""

    def __init__(self, L, solver, D, W, ch, balls, lines, capsules, cuboids, con_lo, con_hi):
        self.L, self.solver = declare(L), solver
        self.rc, self.ptr = create_cuboids(L, solver._h, D, W, ch, balls, lines, capsules, cuboids, con_lo, con_hi)
