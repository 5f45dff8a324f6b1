"""Capsule and sphere obstacles (mi_gomp_capsule, CapsuleObstacle) beside tests/gomp_refs.py and tests/dh_refs.py: a helper
module of the tests, not a conftest.

A capsule is the segment a .. b swept by a sphere of radius R; a == b is a sphere.  For a ball with centre p = fk(q_w), radius r
and 3 x D position Jacobian J (include/mi_osqp.h has the same definition, restated here from it alone):

    c    = a                                  when e.e == 0, e = b - a
         = a + t e,  t = min(1, max(0, (p - a).e / e.e))   otherwise
    v    = p - c,  dist = |v|,  s = dist - (R + r)
    nrm  = v / dist  when dist > 1e-12,  (0, 0, 1)  otherwise
    g_j  = nrm_x J[x][j] + nrm_y J[y][j] + nrm_z J[z][j]                 written whether the row is active or not
    s < margin:  l = (R + r) - dist + sum_j g_j q_w[j],  u = +1e30       otherwise  l = -1e30, u = +1e30
    accepted only if s >= -ERROR at every (ball, waypoint, capsule)

in mpmath at 50 digits and in np.float64 (gomp_refs.MPA / F64).  The box and line rows, their classes and their part of the
verdict are gomp_refs' own (with dh_refs' chain model); this module computes the capsule rows and merges the two in the
library's row order: per ball and waypoint the three box rows of a gripper ball, the lines, then the capsules.

The scenes of tests/test_gpu_capsules.py are defined here so that tests/test_capsule_refs.py can check their populations on
the CPU first; the ctypes declarations of mi_gomp_scene_create_world take the library as an argument."""
import ctypes as C
import functools
import json
import os

import numpy as np

import dh_refs as DH
import gomp_refs as G

NEAR = 1e-9                     # a row whose activity or normal hangs on a quantity closer than this to its threshold
CLASSES = ("active", "none")
CLAMPS = ("point", "low", "inside", "high")       # a == b; t clamped at 0; 0 < t < 1; t clamped at 1


def capsule(a, b, radius, margin):
    return dict(a=[float(v) for v in a], b=[float(v) for v in b], radius=float(radius), margin=float(margin))


def sphere(centre, radius, margin):
    return capsule(centre, centre, radius, margin)


# ------------------------------------------------------------------ one capsule row

def closest(cap, p, K=G.MPA):
    """(c, clamp): the point of the segment closest to p and which of CLAMPS it is."""
    a, b = [K.num(v) for v in cap["a"]], [K.num(v) for v in cap["b"]]
    e = [b[k] - a[k] for k in range(3)]
    ee = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
    if ee == 0:
        return a, "point"
    t = ((p[0] - a[0]) * e[0] + (p[1] - a[1]) * e[1] + (p[2] - a[2]) * e[2]) / ee
    clamp = "low" if t <= 0 else ("high" if t >= 1 else "inside")
    t = min(K.num(1), max(K.num(0), t))
    return [a[k] + t * e[k] for k in range(3)], clamp


def distance(cap, p, K=G.MPA):
    c, _ = closest(cap, p, K)
    v = [p[k] - c[k] for k in range(3)]
    return K.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def capsule_row(cap, p, J, q, r, K=G.MPA):
    """The row of one (ball, waypoint, capsule): a dict with vals[D], l, u, l_scale, cls, clamp, near, s (the clearance)."""
    num = K.num
    D = len(q)
    c, clamp = closest(cap, p, K)
    v = [p[k] - c[k] for k in range(3)]
    dist = K.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    reach = num(cap["radius"]) + r
    s = dist - reach
    nrm = [v[k] / dist for k in range(3)] if dist > num(1e-12) else [num(0), num(0), num(1)]
    g = [nrm[0] * J[0][j] + nrm[1] * J[1][j] + nrm[2] * J[2][j] for j in range(D)]
    gq = sum((g[j] * q[j] for j in range(D)), num(0))
    margin = num(cap["margin"])
    active = s < margin
    near = bool(abs(s - margin) < num(NEAR) or (dist != 0 and dist < num(NEAR)))
    low = reach - dist + gq if active else -num(G.INF)
    scale = reach + dist + sum((abs(g[j] * q[j]) for j in range(D)), num(0)) if active else num(0)
    return dict(vals=[float(x) for x in g], l=float(low), u=G.INF, l_scale=float(scale), cls="active" if active else "none", clamp=clamp,
                near=near, s=float(s), s_hi=s)


# ------------------------------------------------------------------ rows and verdict of a scene

_CACHE = {}


def _evaluate(D, W, balls, lines, capsules, con_lo, con_hi, traj, K, margin):
    traj = np.ascontiguousarray(traj, np.float64)
    key = (D, W, json.dumps([[{k: v for k, v in b.items() if k != "chain"} for b in balls], lines, capsules,
                             None if con_lo is None else list(con_lo), None if con_hi is None else list(con_hi)]),
           id(balls[0].get("chain")) if balls else 0, traj.tobytes(), K.name, margin)
    if key in _CACHE:
        return _CACHE[key]
    base = G.with_obstacles(D, W, balls, lines, con_lo, con_hi, traj, margin, K)
    num, mg, err = K.num, K.num(margin), K.num(G.ERROR)
    nl, nc = len(lines), len(capsules)
    rows = dict(vals=[], l=[], u=[], l_scale=[], u_scale=[], cls=[], ball=[], w=[], kind=[], near=[], clamp=[], s=[])
    comparisons = []
    ok_caps, uncertain, definite = True, False, False
    cache = {}
    src = 0                                                  # next row of `base`
    for bi, ball in enumerate(balls):
        r = num(ball["radius"])
        for w in range(W):
            for _ in range((3 if ball["gripper"] else 0) + nl):
                for k in ("l", "u", "l_scale", "u_scale", "cls", "ball", "w", "kind", "near"):
                    rows[k].append(base[k][src])
                rows["vals"].append(base["vals"][src])
                rows["clamp"].append(None)
                rows["s"].append(np.nan)
                src += 1
            if not nc:
                continue
            qf = traj[w * D:(w + 1) * D]
            p, J = G.fk_jac(ball, qf, w, K, cache)
            q = [num(x) for x in qf]
            for ci, cap in enumerate(capsules):
                e = capsule_row(cap, p, J, q, r, K)
                rows["vals"].append(e["vals"]); rows["l"].append(e["l"]); rows["u"].append(e["u"])
                rows["l_scale"].append(e["l_scale"]); rows["u_scale"].append(0.0)
                rows["cls"].append(e["cls"]); rows["ball"].append(bi); rows["w"].append(w); rows["kind"].append(3 + nl + ci)
                rows["near"].append(e["near"]); rows["clamp"].append(e["clamp"]); rows["s"].append(e["s"])
                slack = e["s_hi"] + err                       # s >= -ERROR
                near = bool(abs(slack) < mg)
                comparisons.append(dict(kind="capsule", ball=bi, w=w, idx=ci, slack=float(slack), near=near))
                if slack < 0:
                    ok_caps = False
                if near:
                    uncertain = True
                elif slack < 0:
                    definite = True
    assert src == len(base["l"])
    out = {k: (v if k in ("cls", "clamp") else np.array(v)) for k, v in rows.items()}
    out["vals"] = np.array(rows["vals"], np.float64).reshape(len(rows["l"]), D)
    out["near"] = np.array(rows["near"], bool)
    # gomp_refs' verdict: excluded = uncertain and not definite; a rejected verdict that is not excluded has a definite cause
    definite = definite or (not base["ok"] and not base["verdict_excluded"])
    uncertain = uncertain or base["verdict_excluded"]
    causes = set(base["causes"]) | ({"capsule"} if not ok_caps else set())
    out.update(decisions=base["decisions"], margins=base["margins"] + comparisons, ok=bool(base["ok"] and ok_caps), causes=causes,
               verdict_excluded=bool(uncertain and not definite))
    _CACHE[key] = out
    return out


def with_obstacles(D, W, balls, lines, capsules, con_lo, con_hi, traj, margin=G.MARGIN, K=G.MPA):
    """gomp_refs.with_obstacles with capsule rows after the lines of every (ball, waypoint) block.  The arrays over the rows are
    those of gomp_refs (cls "active" / "none" and kind 3 + |lines| + i for capsule i), with "clamp" (which part of the segment
    is closest, None for the other rows) and "s" (the clearance, nan for the other rows) besides; ok / causes (with
    "capsule") / verdict_excluded / margins cover the whole acceptance test."""
    return _evaluate(D, W, balls, lines, capsules, con_lo, con_hi, traj, K, margin)


# ------------------------------------------------------------------ the scenes of the GPU tests

E20, E30 = 2.0 ** -20, 2.0 ** -30
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1]
KT_C = (1.0, 0.5, 0.25)                                      # centre of KT's sphere and first end of its short segment
KT_R0, KT_M0, KT_RB, KT_RB1 = 1 / 4, 1 / 8, 1 / 16, 1 / 32   # capsule 0: radius, margin; radii of balls 0 and 1
KT_FAR = 2.0
KT_ACCEPT = G.grid(KT_R0 + KT_RB - G.ERROR)                  # distance at which ball 0 has s = -ERROR from capsule 0, on the 2^-30 grid


def _kt_trajectories():
    """Every waypoint sits on an axis through KT_C, at a dyadic distance: each row of the scene is exact in fp64 in any order of
    operations (|v| = the one component, normal = +-unit vector, all sums of numbers on the 2^-30 grid below 16)."""
    W = 6

    def tour(*special, far=(0, KT_FAR)):
        p = np.tile(KT_C, (W, 1))
        p[:, far[0]] += far[1]
        for w, axis, d in special:
            p[w] = KT_C
            p[w, axis] += d
        return p

    act = KT_R0 + KT_RB + KT_M0                               # distance at which ball 0 has s = margin from capsule 0
    out = [
        tour((2, 0, 0.0)),                                    # 0: on the sphere's centre and the segment's end: dist == 0, normal +Z
        tour((1, 0, act - E20), (4, 0, act + E20)),           # 1: s = margin -+ 2^-20 (ball 0, capsule 0): active | not; accepted
        tour((2, 1, KT_ACCEPT + E20), far=(1, 0.5)),          # 2: s = -ERROR + 2^-20: accepted
        tour((2, 1, KT_ACCEPT - E20), far=(1, 0.5)),          # 3: s = -ERROR - 2^-20: rejected (its re-linearised QP has a solution)
        tour((1, 0, KT_RB - E20), (3, 0, KT_RB + E20)),       # 4: s = -+ 2^-20 of capsule 1 (margin 0, radius 0) for ball 0: active | not
        tour((0, 2, 0.5), (2, 2, -0.5)),                      # 5: beyond the ends of the short segment: t clamped at 1 | 0
        tour((1, 1, -0.34375), (2, 2, -0.421875), (4, 0, -0.328125)),      # 6: active rows with normals -y, -z, -x; accepted
        tour((0, 1, 0.375), (3, 0, 0.34375), (5, 2, KT_R0 + KT_RB)),       # 7: ... +y, +x, +z, the last with ball 0 on the surface (s = 0)
    ]
    return np.array([G._with_velocities(p) for p in out])


K7_CAPSULES = [sphere((0.66, -0.1, 0.55), 0.06, 0.05),                                # in the sweep of the forearm and the wrist
               capsule((0.3, 0.75, 0.0), (0.3, 0.75, 0.6), 0.04, 0.04),                # a vertical post
               capsule((-0.7, 0.3, 0.42), (-0.64, 0.42, 0.56), 0.03, 0.06)]            # a slanted pipe
K8_CAPSULES = [sphere((0.45, 0.55, 0.45), 0.08, 0.1)]
KM_CAPSULES = [capsule((-0.5, -0.5, 0.2), (0.5, 0.5, 0.4), 0.125, 0.25), sphere((0.25, -0.5, 0.0), 0.25, 0.125)]


def _km_trajectories(W):
    rng = np.random.default_rng(1905)
    out = []
    for k in range(8):
        a, b = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
        out.append(a + np.linspace(0.0, 1.0, W)[:, None] * (b - a))
    return np.array([G._with_velocities(p) for p in out])


SCENES = ("K7", "K8", "KT", "KM")


@functools.lru_cache(maxsize=None)
def scene(name):
    """name: "K7", "K8", "KT", "KM".  A dict as dh_refs.scene gives, with "capsules" besides ("chain" None without chain balls)."""
    if name == "K7":
        c7 = DH.scene("C7")
        return dict(c7, name=name, lines=[DH.LINE0], capsules=K7_CAPSULES)
    if name == "K8":
        balls = [DH.chain_ball(DH.C8, 8, (0, 0, 0.02), 0, 0.04)]
        return dict(name=name, D=8, W=2, chain=DH.C8, balls=balls, lines=[], capsules=K8_CAPSULES, con_lo=None, con_hi=None, margin=G.MARGIN,
                    trajs=DH._c8_trajectories())
    if name == "KT":
        balls = [G._ball(G.TABLE, 0, KT_RB, IDENTITY), G._ball(G.TABLE, 0, KT_RB1, IDENTITY)]
        caps = [sphere(KT_C, KT_R0, KT_M0), capsule(KT_C, (KT_C[0], KT_C[1], KT_C[2] + E30), 0.0, 0.0)]
        return dict(name=name, D=3, W=6, chain=None, balls=balls, lines=[], capsules=caps, con_lo=None, con_hi=None, margin=G.MARGIN, trajs=_kt_trajectories())
    if name == "KM":
        W = 4
        balls = [G._ball(G.TABLE, 1, 1 / 16, G.T_TABLES[0]), G._ball(G.TABLE, 0, 1 / 8, G.T_TABLES[1])]
        return dict(name=name, D=3, W=W, chain=None, balls=balls, lines=G.T_LINES, capsules=KM_CAPSULES, con_lo=[-0.75, -G.INF, -0.875], con_hi=[G.INF, 0.875, G.INF],
                    margin=G.MARGIN, trajs=_km_trajectories(W))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def scene_reference(name, K=G.MPA):
    """with_obstacles of the scene's eight trajectories."""
    s = scene(name)
    return [with_obstacles(s["D"], s["W"], s["balls"], s["lines"], s["capsules"], s["con_lo"], s["con_hi"], t, s["margin"], K) for t in s["trajs"]]


@functools.lru_cache(maxsize=None)
def fp64_error(name):
    """dh_refs.fp64_error for the scenes of this module: the np.float64 evaluation of the formulas against the mpmath one."""
    ev = eb = 0.0
    for hi, lo in zip(scene_reference(name), scene_reference(name, G.F64)):
        v, b = DH.row_distance(hi, lo)
        ev, eb = max(ev, v), max(eb, b)
    return ev, eb


def gpu_tolerance(name):
    """The project's rule (gomp_refs.gpu_tolerance): 32 x fp64_error, never looser than 1e-13.  (0, 0) for scene KT: exact."""
    ev, eb = fp64_error(name)
    return min(32 * ev, 1e-13), min(32 * eb, 1e-13)


@functools.lru_cache(maxsize=None)
def scene_batch(name, over_allocate=False):
    """gomp_refs.scene_problem for the scene's eight trajectories; a capsule takes a row per (ball, waypoint) as a line does."""
    s = scene(name)
    D, W = s["D"], s["W"]
    ends = s["trajs"][:, (W - 3) * D:(W - 2) * D] if W >= 4 else None
    return G.scene_problem(D, W, s["balls"], len(s["lines"]) + len(s["capsules"]), 8, over_allocate, starts=s["trajs"][:, :D], ends=ends)


def populations(name):
    """Counts a test can assert on and print: capsule rows per class and clamp case and capsule, verdicts, causes, exclusions."""
    s, ref = scene(name), scene_reference(name)
    nc, nl = len(s["capsules"]), len(s["lines"])
    cls = {c: np.zeros(nc, int) for c in CLASSES}
    clamp = {c: np.zeros(nc, int) for c in CLAMPS}
    near = rows = 0
    causes = {}
    for e in ref:
        for k in range(len(e["l"])):
            if e["clamp"][k] is None:
                near += bool(e["near"][k])
                continue
            ci = int(e["kind"][k]) - 3 - nl
            cls[e["cls"][k]][ci] += 1
            clamp[e["clamp"][k]][ci] += 1
            near += bool(e["near"][k])
            rows += 1
        for c in e["causes"]:
            causes[c] = causes.get(c, 0) + 1
    return dict(cls=cls, clamp=clamp, near=near, capsule_rows=rows, accepted=sum(e["ok"] for e in ref), rejected=sum(not e["ok"] for e in ref),
                causes=causes, verdicts_excluded=sum(e["verdict_excluded"] for e in ref),
                near_comparisons=sum(m["near"] for e in ref for m in e["margins"]))


# ------------------------------------------------------------------ the known answers in tests/golden/capsule_kats.json

KAT_SCENES = ("KT", "KM")


def kats_now():
    """What tests/golden/capsule_kats.json holds, computed now: per scene and trajectory the rows (vals, l, u as JSON numbers: the
    shortest decimal that reads back as the same double) and the verdict of the mpmath reference."""
    out = {}
    for name in KAT_SCENES:
        out[name] = [dict(vals=[[float(x) for x in row] for row in e["vals"]], l=[float(x) for x in e["l"]], u=[float(x) for x in e["u"]],
                          ok=bool(e["ok"])) for e in scene_reference(name)]
    return out


def kats_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capsule_kats.json")


def load_kats():
    with open(kats_path()) as f:
        return json.load(f)


# ------------------------------------------------------------------ ctypes: mi_gomp_scene_create_world (tests only)

class Capsule(C.Structure):
    _fields_ = [("a", C.c_double * 3), ("b", C.c_double * 3), ("radius", C.c_double), ("margin", C.c_double)]


def c_capsules(capsules):
    arr = (Capsule * max(len(capsules), 1))()
    for k, cp in enumerate(capsules):
        for j in range(3):
            arr[k].a[j], arr[k].b[j] = cp["a"][j], cp["b"][j]
        arr[k].radius, arr[k].margin = cp["radius"], cp["margin"]
    return arr


def declare(L):
    DH.declare(L)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    L.mi_gomp_scene_create_world.argtypes = [C.POINTER(vp), vp, C.c_int64, C.c_int64, C.POINTER(DH.Chain), C.c_int64, C.POINTER(G.Ball), C.c_int64,
                                             C.POINTER(G.Line), C.c_int64, C.POINTER(Capsule), dp, dp]
    L.mi_gomp_scene_create_world.restype = C.c_int
    return L


def create_world(L, handle, D, W, ch, balls, lines, capsules, con_lo=None, con_hi=None, n_capsules=None, null_capsules=False):
    """(rc, scene pointer) of mi_gomp_scene_create_world; ch: a Chain, a chain dict or None.  n_capsules / null_capsules override
    what is passed for the capsule count and array (the refusals)."""
    ptr = C.c_void_p()
    lo = None if con_lo is None else np.ascontiguousarray(con_lo, np.float64)
    hi = None if con_hi is None else np.ascontiguousarray(con_hi, np.float64)
    cc = DH.c_chain(ch) if isinstance(ch, dict) else ch
    rc = L.mi_gomp_scene_create_world(C.byref(ptr), handle, D, W, None if cc is None else C.byref(cc), len(balls), G.c_balls(balls), len(lines),
                                      G.c_lines(lines), len(capsules) if n_capsules is None else n_capsules,
                                      None if null_capsules else c_capsules(capsules), G._dp(lo), G._dp(hi))
    return rc, ptr


class WorldScene(G.GompScene):
    """gomp_refs.GompScene made by mi_gomp_scene_create_world."""

    def __init__(self, L, solver, D, W, ch, balls, lines, capsules, con_lo, con_hi):
        self.L, self.solver = declare(L), solver
        self.rc, self.ptr = create_world(L, solver._h, D, W, ch, balls, lines, capsules, con_lo, con_hi)
