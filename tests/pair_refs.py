"""Self-collision pairs (mi_gomp_pair, BallPair) beside tests/cuboid_refs.py, tests/capsule_refs.py, tests/gomp_refs.py and
tests/dh_refs.py: a helper module of the tests, not a conftest.

A pair joins balls a and b of the scene and has a margin.  At waypoint w, with p_a, p_b the two centres, J_a, J_b the 3 x D
position Jacobians and r_a, r_b the radii (include/mi_osqp.h has the same definition, restated here from it alone):

    v      = p_a - p_b,  dist = sqrt(v_x^2 + v_y^2 + v_z^2)
    dist > 1e-12:  n = v / dist          otherwise  n = (0, 0, 1)
    reach  = r_a + r_b,  s = dist - reach
    g_j    = (n_x Ja[x][j] + n_y Ja[y][j] + n_z Ja[z][j]) - (n_x Jb[x][j] + n_y Jb[y][j] + n_z Jb[z][j])
             written whether the row is active or not
    s < margin:  l = (reach - dist) + sum_j g_j q_w[j],  u = +1e30        otherwise  l = -1e30, u = +1e30
    accepted only if s >= -ERROR at every (pair, waypoint)

in mpmath at 50 digits and in np.float64 (gomp_refs.MPA / F64).  The rows of the (ball, waypoint) blocks and their part of the
verdict are cuboid_refs' (with capsule_refs, gomp_refs and dh_refs behind it); this module computes the pair rows and puts them
behind the block of the last ball, pair-major: the row of (pair k, waypoint w) is row0 + the rows of all blocks + k W + w.

A row is `near` when |s - margin| < NEAR, or when dist is nonzero and below NEAR.  A verdict within NEAR of -ERROR is excluded.
The term scale of a bound is reach + dist + sum_j |g_j q_j|.

The scenes of tests/test_gpu_pairs.py are defined here so that tests/test_pair_refs.py can check their populations on the CPU
first; the ctypes declarations of mi_gomp_scene_create_pairs take the library as an argument."""
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
from osqp_solver_amd import problems as PR

NEAR = K.NEAR
CLASSES = ("active", "none")


def pair(a, b, margin=0.0):
    return dict(a=int(a), b=int(b), margin=float(margin))


def self_pairs(balls, min_frame_gap=2, margin=0.0):
    """What dhSelfPairs of dh_kinematics.hpp gives: every (i, j), i < j, of chain balls whose frames are at least min_frame_gap
    apart."""
    out = []
    for i in range(len(balls)):
        for j in range(i + 1, len(balls)):
            if balls[i]["model"] != DH.DH_CHAIN or balls[j]["model"] != DH.DH_CHAIN:
                continue
            if abs(int(balls[i]["param"][0]) - int(balls[j]["param"][0])) >= max(min_frame_gap, 1):
                out.append(pair(i, j, margin))
    return out


# ------------------------------------------------------------------ one pair row

def pair_row(pa, Ja, ra, pb, Jb, rb, q, margin, K_=G.MPA):
    """The row of one (pair, waypoint): a dict with vals[D], l, u, l_scale, cls, near, s (the clearance), s_hi (s in K_'s
    numbers) and dist."""
    num = K_.num
    D = len(q)
    v = [pa[k] - pb[k] for k in range(3)]
    dist = K_.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    n = [v[k] / dist for k in range(3)] if dist > num(1e-12) else [num(0), num(0), num(1)]
    reach = ra + rb
    s = dist - reach
    g = [(n[0] * Ja[0][j] + n[1] * Ja[1][j] + n[2] * Ja[2][j]) - (n[0] * Jb[0][j] + n[1] * Jb[1][j] + n[2] * Jb[2][j]) for j in range(D)]
    gq = sum((g[j] * q[j] for j in range(D)), num(0))
    mg = num(margin)
    active = s < mg
    near = abs(s - mg) < num(NEAR) or (dist != 0 and dist < num(NEAR))
    low = (reach - dist) + gq if active else -num(G.INF)
    scale = reach + dist + sum((abs(g[j] * q[j]) for j in range(D)), num(0)) if active else num(0)
    return dict(vals=[float(x) for x in g], l=float(low), u=G.INF, l_scale=float(scale), cls="active" if active else "none", near=bool(near),
                s=float(s), s_hi=s, dist=float(dist))


# ------------------------------------------------------------------ rows and verdict of a scene

_CACHE = {}


def _evaluate(D, W, balls, lines, capsules, cuboids, pairs, con_lo, con_hi, traj, K_, margin):
    traj = np.ascontiguousarray(traj, np.float64)
    key = (D, W, json.dumps([[{k: v for k, v in b.items() if k != "chain"} for b in balls], lines, capsules, cuboids, pairs,
                             None if con_lo is None else list(con_lo), None if con_hi is None else list(con_hi)]),
           id(balls[0].get("chain")) if balls else 0, traj.tobytes(), K_.name, margin)
    if key in _CACHE:
        return _CACHE[key]
    base = X.with_obstacles(D, W, balls, lines, capsules, cuboids, con_lo, con_hi, traj, margin, K_)
    num, err = K_.num, K_.num(G.ERROR)
    nb = len(base["l"])
    keys = ("l", "u", "l_scale", "u_scale", "cls", "ball", "w", "kind", "near", "clamp", "s", "region", "out", "dn")
    rows = {k: list(base[k]) for k in keys}
    rows["vals"] = [list(r) for r in base["vals"]]
    rows["pair"] = [-1] * nb
    rows["dist"] = [np.nan] * nb
    comparisons = []
    ok_pair, uncertain, definite = True, False, False
    cache = {}
    for k, pr in enumerate(pairs):
        A, Bb = balls[pr["a"]], balls[pr["b"]]
        for w in range(W):
            qf = traj[w * D:(w + 1) * D]
            pa, Ja = G.fk_jac(A, qf, w, K_, cache)
            pb, Jb = G.fk_jac(Bb, qf, w, K_, cache)
            e = pair_row(pa, Ja, num(A["radius"]), pb, Jb, num(Bb["radius"]), [num(x) for x in qf], pr["margin"], K_)
            rows["vals"].append(e["vals"]); rows["l"].append(e["l"]); rows["u"].append(e["u"])
            rows["l_scale"].append(e["l_scale"]); rows["u_scale"].append(0.0)
            rows["cls"].append(e["cls"]); rows["ball"].append(-1); rows["w"].append(w); rows["kind"].append(-1)
            rows["near"].append(e["near"]); rows["clamp"].append(None); rows["s"].append(e["s"])
            rows["region"].append(None); rows["out"].append(np.nan); rows["dn"].append(np.nan)
            rows["pair"].append(k); rows["dist"].append(e["dist"])
            slack = e["s_hi"] + err                           # s >= -ERROR
            near = bool(abs(slack) < num(NEAR))
            comparisons.append(dict(kind="pair", ball=-1, w=w, idx=k, slack=float(slack), near=near))
            if slack < 0:
                ok_pair = False
            if near:
                uncertain = True
            elif slack < 0:
                definite = True
    out = {k: (v if k in ("cls", "clamp", "region") else np.array(v)) for k, v in rows.items() if k != "vals"}
    out["vals"] = np.array(rows["vals"], np.float64).reshape(len(rows["l"]), D)
    out["near"] = np.array(rows["near"], bool)
    definite = definite or (not base["ok"] and not base["verdict_excluded"])
    uncertain = uncertain or base["verdict_excluded"]
    causes = set(base["causes"]) | ({"pair"} if not ok_pair else set())
    out.update(decisions=base["decisions"], margins=base["margins"] + comparisons, ok=bool(base["ok"] and ok_pair), causes=causes,
               verdict_excluded=bool(uncertain and not definite), block_rows=nb)
    _CACHE[key] = out
    return out


def with_obstacles(D, W, balls, lines, capsules, cuboids, pairs, con_lo, con_hi, traj, margin=G.MARGIN, K_=G.MPA):
    """cuboid_refs.with_obstacles with the pair rows behind the block of the last ball, pair-major.  The arrays over the rows are
    those of cuboid_refs (for a pair row: cls "active" / "none", ball -1, kind -1), with "pair" (the pair's index, -1 for the other
    rows) and "dist" (nan for the other rows) besides; ok / causes (with "pair") / verdict_excluded / margins cover the whole
    acceptance test; block_rows = the number of rows before the first pair row."""
    return _evaluate(D, W, balls, lines, capsules, cuboids, pairs, con_lo, con_hi, traj, K_, margin)


# ------------------------------------------------------------------ the batch a scene sits on

def scene_problem(D, W, balls, n_per_ball, n_pairs, B, over_allocate, starts=None, ends=None, seed=4100):
    """gomp_refs.scene_problem with W n_pairs rows behind the blocks of the (ball, waypoint) pairs, pair-major; pair rows are not
    per ball, so that function cannot make them.  over_allocate: the all-zero rows of ConstraintBuilder's allocation,
    D W (3 + n_per_ball balls) + W n_pairs rows from row0 on, come after the pair rows."""
    row0, block_rows = G.row_layout(D, W, balls, n_per_ball)
    rows3d = block_rows + W * n_pairs
    m = row0 + (D * W * (3 + n_per_ball * len(balls)) + W * n_pairs if over_allocate else rows3d)
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
            for _ in range((3 if ball["gripper"] else 0) + n_per_ball):
                r3 += [r] * D
                c3 += list(range(w * D, (w + 1) * D))
                r += 1
    for _ in range(n_pairs):
        for w in range(W):
            r3 += [r] * D
            c3 += list(range(w * D, (w + 1) * D))
            r += 1
    assert r == row0 + rows3d
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
        ls.append(np.concatenate([l[:row0], np.full(m - row0, -G.INF)]))
        us.append(np.concatenate([u[:row0], np.full(m - row0, G.INF)]))
    P = sp.csc_matrix(PR.tri_diagonal_matrix(2.0, -1.0, n, D * W, D))
    P.sort_indices()
    return dict(n=n, m=m, P=P, A=A0, Px=np.tile(P.data, (B, 1)), Ax=np.array(Axs), q=None, l=np.array(ls), u=np.array(us),
                row0=row0, rows3d=rows3d, block_rows=block_rows, aidx=aidx, starts=starts, ends=ends)


# ------------------------------------------------------------------ the scenes of the GPU tests

E20 = K.E20
P7_MARGIN = 0.08
# the folded postures of the 7-joint chain: forearm and wrist balls inside the shoulder ball (pairs (0, 5), (0, 4), (0, 6), (0, 3))
FOLD7 = (np.array([2.78, 0.99, 1.54, 2.65, 0.13, 0.02, -0.55]), np.array([-0.98, -0.42, -0.7, 2.12, 0.18, -2.47, -2.6]),
         np.array([1.75, -1.47, 0.24, 1.89, -2.75, 0.25, -2.19]), np.array([0.68, 0.39, 2.6, 2.8, -1.48, -2.27, 0.51]))
START7 = DH.BASE7 + np.array([0.2, 0, 0, 0, 0, 0, 0])          # BASE7 turned off the plane y = 0, in which line 0 lies
# (posture, how far the sweep goes from BASE7 towards it)
P7_SWEEPS = ((0, 1.0), (1, 1.0), (2, 1.0), (3, 0.9), (0, 0.8), (1, 0.85), (2, 0.9), (3, 0.75))


def _p7_trajectories(W):
    """Eight straight joint-space sweeps from START7 (dh_refs.BASE7 turned by 0.2 about the first joint) towards the folded postures: four (nearly) all the way in, four part of it."""
    out = []
    for k, f in P7_SWEEPS:
        t = np.linspace(0.0, 1.0, W)[:, None]
        out.append(START7 + t * f * (FOLD7[k] - START7))
    return np.array([G._with_velocities(p) for p in out])


# scene PT: exact.  TABLE balls sit at p = q, FIXED balls (yaw + 2-link with both link lengths zero: p = (0, 0, base height) and
# J = 0 whatever q is, exact in any arithmetic) on the z axis; every waypoint is on the z axis at a dyadic height, so every
# separation is along z, dist is the one component's magnitude and n = +-e_z exactly.
PT_Z = (1.0, -1.0, 3.0)                                      # heights of the fixed balls 3, 4, 5
PT_R = (1 / 16, 0.0, 0.0, 1 / 8, 0.0, 1 / 32)              # radii: TABLE balls 0, 1, 2; fixed balls 3, 4, 5
PT_MA = 1 / 8
PT_FAR = 8.0
PT_PAIRS = [pair(0, 3, PT_MA),                              # 0: a TABLE ball and a fixed ball, margin 1/8
            pair(3, 0, PT_MA),                              # 1: the same two the other way round: g changes sign, the bound does not
            pair(0, 5, 0.0),                                # 2: margin 0
            pair(1, 2, PT_MA),                              # 3: two TABLE balls: always coincident, reach 0: accepted, n = +z
            pair(1, 4, PT_MA)]                              # 4: reach 0 against a fixed ball: coincident at q = (0, 0, -1), accepted
PT_REACH0, PT_REACH2 = PT_R[0] + PT_R[3], PT_R[0] + PT_R[5]
PT_ACCEPT = G.grid(PT_REACH0 - G.ERROR)                      # |z - 1| at which pair 0 has s = -ERROR, on the 2^-30 grid


def _pt_tour(W, *special):
    p = np.zeros((W, 3))
    p[:, 2] = PT_FAR
    for w, z in special:
        p[w, 2] = z
    return p


def _pt_trajectories():
    W = 6
    act0 = PT_REACH0 + PT_MA                                 # |z - 1| at which pairs 0 and 1 have s = margin
    out = [
        _pt_tour(W, (1, PT_Z[0] + act0 - E20), (3, PT_Z[0] - (act0 + E20))),              # 0: s = margin -+ 2^-20 (margin 1/8): active from above | not, from below
        _pt_tour(W, (2, PT_Z[2] + PT_REACH2 - E20), (4, PT_Z[2] - (PT_REACH2 + E20))),    # 1: s = -+ 2^-20 of pair 2 (margin 0): active | not
        _pt_tour(W, (2, PT_Z[0] + PT_ACCEPT + E20)),                                       # 2: s = -ERROR + 2^-20: accepted
        _pt_tour(W, (2, PT_Z[0] + PT_ACCEPT - E20)),                                       # 3: s = -ERROR - 2^-20: rejected, by that pair alone
        _pt_tour(W, (1, PT_Z[1]), (4, PT_Z[1] - 1 / 4)),                                   # 4: pair 4 coincident with reach 0: accepted, n = +z; then 1/4 below: not active
        _pt_tour(W, (3, PT_Z[0])),                                                         # 5: pair 0 coincident with reach 3/16: rejected, n = +z
        _pt_tour(W, (1, PT_Z[0] - 1 / 4), (2, PT_Z[0] + 1 / 4)),                           # 6: active from below and from above; accepted
        _pt_tour(W),                                                                       # 7: far from everything
    ]
    return np.array([G._with_velocities(p) for p in out])


def _fixed_ball(z, radius):
    return G._ball(G.YAW_2LINK, 0, radius, [0.0, 0.0, z])


PM_PAIRS = [pair(0, 2, 0.75), pair(2, 1, 0.5)]

SCENES = ("P7", "P8", "PT", "PM")
EXACT = ("PT",)


@functools.lru_cache(maxsize=None)
def scene(name):
    """name: one of SCENES.  A dict as cuboid_refs.scene gives, with "pairs" besides."""
    if name == "P7":
        x7 = X.scene("X7")
        return dict(x7, name=name, cuboids=[], con_lo=None, con_hi=None, pairs=self_pairs(x7["balls"], 2, P7_MARGIN), trajs=_p7_trajectories(x7["W"]))
    if name == "P8":
        c8 = DH.scene("C8")
        return dict(name=name, D=8, W=2, chain=DH.C8, balls=c8["balls"], lines=[], capsules=[], cuboids=[], pairs=[pair(0, 1, 0.5)], con_lo=None,
                    con_hi=None, margin=G.MARGIN, trajs=DH._c8_trajectories())
    if name == "PT":
        balls = [G._ball(G.TABLE, 0, PT_R[0], G.T_TABLES[0]), G._ball(G.TABLE, 0, PT_R[1], G.T_TABLES[1]), G._ball(G.TABLE, 0, PT_R[2], G.T_TABLES[2]),
                 _fixed_ball(PT_Z[0], PT_R[3]), _fixed_ball(PT_Z[1], PT_R[4]), _fixed_ball(PT_Z[2], PT_R[5])]
        return dict(name=name, D=3, W=6, chain=None, balls=balls, lines=[], capsules=[], cuboids=[], pairs=PT_PAIRS, con_lo=None, con_hi=None,
                    margin=G.MARGIN, trajs=_pt_trajectories())
    if name == "PM":
        xm = X.scene("XM")
        balls = list(xm["balls"]) + [G._ball(G.YAW_2LINK, 0, 1 / 16, G.Y_PARAMS[0])]
        return dict(xm, name=name, balls=balls, cuboids=xm["cuboids"][:1], pairs=PM_PAIRS)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def scene_reference(name, K_=G.MPA):
    """with_obstacles of the scene's eight trajectories."""
    s = scene(name)
    return [with_obstacles(s["D"], s["W"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["pairs"], s["con_lo"], s["con_hi"], t, s["margin"], K_)
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
    """The project's rule (gomp_refs.gpu_tolerance): 32 x fp64_error, never looser than 1e-13.  (0, 0) for the exact scene."""
    ev, eb = fp64_error(name)
    return min(32 * ev, 1e-13), min(32 * eb, 1e-13)


@functools.lru_cache(maxsize=None)
def scene_batch(name, over_allocate=False):
    """scene_problem for the scene's eight trajectories."""
    s = scene(name)
    D, W = s["D"], s["W"]
    ends = s["trajs"][:, (W - 3) * D:(W - 2) * D] if W >= 4 else None
    return scene_problem(D, W, s["balls"], len(s["lines"]) + len(s["capsules"]) + len(s["cuboids"]), len(s["pairs"]), 8, over_allocate,
                         starts=s["trajs"][:, :D], ends=ends)


def populations(name):
    """Counts a test can assert on and print: pair rows per class and pair, rejecting pair rows, verdicts, causes, exclusions."""
    s, ref = scene(name), scene_reference(name)
    npair = len(s["pairs"])
    cells = {c: np.zeros(npair, int) for c in CLASSES}
    rejecting = np.zeros(npair, int)
    near = rows = 0
    causes, only_pair = {}, 0
    for e in ref:
        for k in range(len(e["l"])):
            near += bool(e["near"][k])
            if e["pair"][k] < 0:
                continue
            cells[e["cls"][k]][int(e["pair"][k])] += 1
            rejecting[int(e["pair"][k])] += bool(e["s"][k] < -G.ERROR)
            rows += 1
        for c in e["causes"]:
            causes[c] = causes.get(c, 0) + 1
        only_pair += e["causes"] == {"pair"}
    return dict(cells=cells, rejecting=rejecting, near=near, pair_rows=rows, accepted=sum(e["ok"] for e in ref), rejected=sum(not e["ok"] for e in ref),
                causes=causes, rejected_by_a_pair_alone=only_pair, verdicts_excluded=sum(e["verdict_excluded"] for e in ref),
                near_comparisons=sum(m["near"] for e in ref for m in e["margins"]))


# ------------------------------------------------------------------ the known answers in tests/golden/pair_kats.json

KAT_SCENES = ("PT", "PM")


def kats_now():
    """What tests/golden/pair_kats.json holds, computed now: per scene and trajectory the rows (vals, l, u as JSON numbers: the
    shortest decimal that reads back as the same double) and the verdict of the mpmath reference."""
    out = {}
    for name in KAT_SCENES:
        out[name] = [dict(vals=[[float(x) for x in row] for row in e["vals"]], l=[float(x) for x in e["l"]], u=[float(x) for x in e["u"]],
                          ok=bool(e["ok"])) for e in scene_reference(name)]
    return out


def kats_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_kats.json")


def load_kats():
    with open(kats_path()) as f:
        return json.load(f)


# ------------------------------------------------------------------ ctypes: mi_gomp_scene_create_pairs (tests only)

class Pair(C.Structure):
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("margin", C.c_double)]


def c_pairs(pairs):
    arr = (Pair * max(len(pairs), 1))()
    for k, pr in enumerate(pairs):
        arr[k].a, arr[k].b, arr[k].margin = pr["a"], pr["b"], pr["margin"]
    return arr


def declare(L):
    X.declare(L)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    L.mi_gomp_scene_create_pairs.argtypes = [C.POINTER(vp), vp, C.c_int64, C.c_int64, C.POINTER(DH.Chain), C.c_int64, C.POINTER(G.Ball), C.c_int64,
                                             C.POINTER(G.Line), C.c_int64, C.POINTER(K.Capsule), C.c_int64, C.POINTER(X.Cuboid), C.c_int64, C.POINTER(Pair),
                                             dp, dp]
    L.mi_gomp_scene_create_pairs.restype = C.c_int
    return L


def create_pairs(L, handle, D, W, ch, balls, lines, capsules, cuboids, pairs, con_lo=None, con_hi=None, n_pairs=None, null_pairs=False, out=True):
    """(rc, scene pointer) of mi_gomp_scene_create_pairs; ch: a Chain, a chain dict or None.  n_pairs / null_pairs override what is
    passed for the pair count and array (the refusals).  The pointer starts as a value that is not NULL, so a refusal shows that it
    was cleared."""
    ptr = C.c_void_p(1)
    lo = None if con_lo is None else np.ascontiguousarray(con_lo, np.float64)
    hi = None if con_hi is None else np.ascontiguousarray(con_hi, np.float64)
    cc = DH.c_chain(ch) if isinstance(ch, dict) else ch
    rc = L.mi_gomp_scene_create_pairs(C.byref(ptr), handle, D, W, None if cc is None else C.byref(cc), len(balls), G.c_balls(balls), len(lines),
                                      G.c_lines(lines), len(capsules), K.c_capsules(capsules), len(cuboids), X.c_cuboids(cuboids),
                                      len(pairs) if n_pairs is None else n_pairs, None if null_pairs else c_pairs(pairs), G._dp(lo), G._dp(hi))
    return rc, ptr


class PairScene(G.GompScene):
    """gomp_refs.GompScene made by mi_gomp_scene_create_pairs."""

    def __init__(self, L, solver, D, W, ch, balls, lines, capsules, cuboids, pairs, con_lo, con_hi):
        self.L, self.solver = declare(L), solver
        self.rc, self.ptr = create_pairs(L, solver._h, D, W, ch, balls, lines, capsules, cuboids, pairs, con_lo, con_hi)
