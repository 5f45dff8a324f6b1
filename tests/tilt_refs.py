"""Tilt limits (mi_gomp_tilt, TiltLimit) beside tests/pair_refs.py, tests/cuboid_refs.py, tests/capsule_refs.py,
tests/gomp_refs.py and tests/dh_refs.py: a helper module of the tests, not a conftest.

The unit vector `axis`, fixed in frame k of the scene's chain (1 <= k <= n_joints), must stay within max_angle radians of the
unit world vector `ref`.  At waypoint w, q = q_w, with R_k the rotation of frame k (R_0 = I) and z_j the third column of R_j
(include/mi_osqp.h has the same definition, restated here from it alone), in this order of operations:

    u_r = R_k[r][0] axis_0 + R_k[r][1] axis_1 + R_k[r][2] axis_2
    c   = u_x ref_x + u_y ref_y + u_z ref_z
    h_j = z_j x u,  g_j = h_jx ref_x + h_jy ref_y + h_jz ref_z  for j < k,  g_j = 0 for j >= k
              written whether the row is active or not
    cos_lim = cos(max_angle),  cos_act = cos(max(0, max_angle - margin)),  cos_ok = cos(min(pi, max_angle + 1e-3))
              three fp64 numbers, taken once when the scene is created and handed on as data
    c < cos_act:  l = (cos_lim - c) + sum_j g_j q_w[j],  u = +1e30        otherwise  l = -1e30, u = +1e30
    accepted only if c >= cos_ok at every (tilt, waypoint)

in mpmath at 50 digits and in np.float64 (gomp_refs.MPA / F64).  max_angle and margin enter as the doubles the C-ABI receives.
The rows of the (ball, waypoint) blocks and of the pairs, and their part of the verdict, are pair_refs' (with cuboid_refs,
capsule_refs, gomp_refs and dh_refs behind it); this module computes the tilt rows and puts them behind the pair rows,
tilt-major: the row of (tilt k, waypoint w) is row0 + the rows of all blocks + W n_pairs + k W + w.

A row is `near` when |c - cos_act| < NEAR.  A verdict is excluded when some |c - cos_ok| < NEAR.  The term scale of a bound is
1 + sum_j |g_j q_j|: cos_lim and c are sums of products of numbers of size <= 1, so their error is absolute.

The scenes of tests/test_gpu_tilts.py are defined here so that tests/test_tilt_refs.py can check their populations on the CPU
first; the ctypes declarations of mi_gomp_scene_create_tilts take the library as an argument."""
import ctypes as C
import functools
import json
import os

import numpy as np

import capsule_refs as K
import cuboid_refs as X
import dh_refs as DH
import gomp_refs as G
import pair_refs as P

NEAR = K.NEAR
CLASSES = ("active", "none")
E20 = K.E20


def tilt(frame, axis, ref, max_angle, margin=0.0):
    return dict(frame=int(frame), axis=[float(v) for v in axis], ref=[float(v) for v in ref], max_angle=float(max_angle), margin=float(margin))


def threshold_angles(t):
    """The three angles whose cosines a scene holds, formed in fp64 as the host forms them: max_angle, max(0, max_angle - margin),
    min(pi, max_angle + 1e-3)."""
    ma, mg = np.float64(t["max_angle"]), np.float64(t["margin"])
    return float(ma), float(max(np.float64(0.0), ma - mg)), float(min(np.float64(np.pi), ma + np.float64(G.ERROR)))


def thresholds(t, K_=G.MPA):
    """(cos_lim, cos_act, cos_ok) of a tilt in K_'s numbers.  They are fp64 numbers, taken once when the scene is created and
    handed on as data: the mpmath kit takes the correctly rounded cosine of the fp64 angle, the fp64 kit np.cos."""
    if K_ is G.MPA:
        return tuple(K_.num(float(G.MP.cos(G.MP.mpf(a)))) for a in threshold_angles(t))
    return tuple(K_.num(K_.cos(K_.num(a))) for a in threshold_angles(t))


# ------------------------------------------------------------------ one tilt row

def tilt_cosine(rots, t, K_=G.MPA):
    """(c, u, g[n]) of a tilt from the rotations R_0 .. R_n of the chain (dh_refs.chain_frames)."""
    num = K_.num
    n = len(rots) - 1
    Rk, a, ref = rots[t["frame"]], [num(v) for v in t["axis"]], [num(v) for v in t["ref"]]
    u = [Rk[r][0] * a[0] + Rk[r][1] * a[1] + Rk[r][2] * a[2] for r in range(3)]
    c = u[0] * ref[0] + u[1] * ref[1] + u[2] * ref[2]
    g = [num(0)] * n
    for j in range(t["frame"]):
        z = [rots[j][0][2], rots[j][1][2], rots[j][2][2]]
        h = G._cross(z, u)
        g[j] = h[0] * ref[0] + h[1] * ref[1] + h[2] * ref[2]
    return c, u, g


def tilt_row(rots, q, t, K_=G.MPA):
    """The row of one (tilt, waypoint): a dict with vals[D], l, u, l_scale, cls, near, c, c_hi (c in K_'s numbers) and slack
    (c - cos_ok in K_'s numbers)."""
    num = K_.num
    D = len(q)
    c, _, g = tilt_cosine(rots, t, K_)
    cos_lim, cos_act, cos_ok = thresholds(t, K_)
    gq = sum((g[j] * q[j] for j in range(D)), num(0))
    active = c < cos_act
    near = abs(c - cos_act) < num(NEAR)
    low = (cos_lim - c) + gq if active else -num(G.INF)
    scale = 1 + sum((abs(g[j] * q[j]) for j in range(D)), num(0)) if active else num(0)
    return dict(vals=[float(x) for x in g], l=float(low), u=G.INF, l_scale=float(scale), cls="active" if active else "none", near=bool(near),
                c=float(c), c_hi=c, slack=c - cos_ok)


# ------------------------------------------------------------------ rows and verdict of a scene

_CACHE = {}


def _evaluate(D, W, chain, balls, lines, capsules, cuboids, pairs, tilts, con_lo, con_hi, traj, K_, margin):
    traj = np.ascontiguousarray(traj, np.float64)
    key = (D, W, json.dumps([chain, [{k: v for k, v in b.items() if k != "chain"} for b in balls], lines, capsules, cuboids, pairs, tilts,
                             None if con_lo is None else list(con_lo), None if con_hi is None else list(con_hi)]), traj.tobytes(), K_.name, margin)
    if key in _CACHE:
        return _CACHE[key]
    base = P.with_obstacles(D, W, balls, lines, capsules, cuboids, pairs, con_lo, con_hi, traj, margin, K_)
    num = K_.num
    nb = len(base["l"])
    rows = {k: list(base[k]) for k in ("l", "u", "l_scale", "u_scale", "cls", "ball", "w", "pair", "near")}
    rows["vals"] = [list(r) for r in base["vals"]]
    rows["tilt"] = [-1] * nb
    rows["c"] = [np.nan] * nb
    comparisons = []
    ok_tilt, uncertain, definite = True, False, False
    frames = {}
    for k, t in enumerate(tilts):
        assert chain is not None and 1 <= t["frame"] <= len(chain["a"]) == D
        for w in range(W):
            qf = traj[w * D:(w + 1) * D]
            if w not in frames:
                frames[w] = DH.chain_frames(chain, qf, K_)[1]
            e = tilt_row(frames[w], [num(x) for x in qf], t, K_)
            rows["vals"].append(e["vals"]); rows["l"].append(e["l"]); rows["u"].append(e["u"])
            rows["l_scale"].append(e["l_scale"]); rows["u_scale"].append(0.0)
            rows["cls"].append(e["cls"]); rows["ball"].append(-1); rows["w"].append(w); rows["pair"].append(-1)
            rows["near"].append(e["near"]); rows["tilt"].append(k); rows["c"].append(e["c"])
            slack = e["slack"]                                # c >= cos_ok
            near = bool(abs(slack) < num(NEAR))
            comparisons.append(dict(kind="tilt", ball=-1, w=w, idx=k, slack=float(slack), near=near))
            if slack < 0:
                ok_tilt = False
            if near:
                uncertain = True
            elif slack < 0:
                definite = True
    out = {k: (v if k == "cls" else np.array(v)) for k, v in rows.items() if k != "vals"}
    out["vals"] = np.array(rows["vals"], np.float64).reshape(len(rows["l"]), D)
    out["near"] = np.array(rows["near"], bool)
    definite = definite or (not base["ok"] and not base["verdict_excluded"])
    uncertain = uncertain or base["verdict_excluded"]
    causes = set(base["causes"]) | ({"tilt"} if not ok_tilt else set())
    out.update(margins=base["margins"] + comparisons, ok=bool(base["ok"] and ok_tilt), causes=causes,
               verdict_excluded=bool(uncertain and not definite), block_rows=base["block_rows"], tilt_rows0=nb)
    _CACHE[key] = out
    return out


def with_obstacles(D, W, chain, balls, lines, capsules, cuboids, pairs, tilts, con_lo, con_hi, traj, margin=G.MARGIN, K_=G.MPA):
    """pair_refs.with_obstacles with the tilt rows behind the pair rows, tilt-major.  The arrays over the rows: vals, l, u, l_scale,
    u_scale, cls, ball, w, pair, near as pair_refs gives them (for a tilt row: cls "active" / "none", ball -1, pair -1), with
    "tilt" (the tilt's index, -1 for the other rows) and "c" (nan for the other rows) besides; ok / causes (with "tilt") /
    verdict_excluded / margins cover the whole acceptance test; tilt_rows0 = the number of rows before the first tilt row."""
    return _evaluate(D, W, chain, balls, lines, capsules, cuboids, pairs, tilts, con_lo, con_hi, traj, K_, margin)


# ------------------------------------------------------------------ the scenes of the GPU tests

H = DH.H
# scene T7: pair_refs' P7 with one tilt per frame 1 .. 7: (axis in the frame, world reference, max_angle, margin)
T7_TILTS = [tilt(1, (1, 0, 0), (1, 0, 0), 1.0, 0.4), tilt(2, (0, 0, 1), (0, 0, 1), 1.2, 0.4), tilt(3, (0, 1, 0), (0, 0, 1), 1.6, 0.5),
            tilt(4, (0, 0, 1), (0.6, 0.0, 0.8), 2.1, 0.6), tilt(5, (1, 0, 0), (0, 0, 1), 3.13, 1.0), tilt(6, (0, 0, 1), (0, 0.28, -0.96), 1.85, 0.3),
            tilt(7, (0, 0, 1), (0, 0, -1), 1.95, 0.35)]

# scene T8: 8 joints, 2 waypoints, one ball without rows, a tilt in frame 8 and one in frame 1
T8_TILTS = [tilt(8, (0.28, 0, 0.96), (0, 0, -1), 0.55, 0.2), tilt(1, (0.6, 0.0, 0.8), (1, 0, 0), 1.8, 0.5)]

# scene TF, the flips: a 2-joint chain with alpha_0 = pi / 2; the axis (0, 1, 0) of frame 2 makes the angle |q_1| with +z
CF = DH.chain((0, 0), (0, 0), (H, 0), (0, 0))
TF_MAX0, TF_MG0, TF_MAX1 = 0.5, 1 / 8, 0.75
TF_TILTS = [tilt(2, (0, 1, 0), (0, 0, 1), TF_MAX0, TF_MG0),     # 0: margin 1/8: active beyond 0.375, accepted up to 0.501
            tilt(2, (0, 1, 0), (0, 0, 1), TF_MAX1, 0.0)]        # 1: margin 0: active beyond 0.75, accepted up to 0.751
TF_W = 4
FAR_IN = 1 / 16


def _tf_tour(q0, *special):
    p = np.zeros((TF_W, 2))
    p[:, 0] = q0
    p[:, 1] = FAR_IN
    for w, a in special:
        p[w, 1] = a
    return p


def _tf_trajectories():
    a0, a1 = TF_MAX0 - TF_MG0, TF_MAX1
    k0, k1 = TF_MAX0 + G.ERROR, TF_MAX1 + G.ERROR
    out = [
        _tf_tour(0.0, (1, a0 - E20), (2, a0 + E20)),             # 0: tilt 0 at max_angle - margin -+ 2^-20: inactive | active; accepted
        _tf_tour(0.7, (1, -(a0 - E20)), (3, -(a0 + E20))),       # 1: the same on the other side of the cone, the arm turned
        _tf_tour(-1.1, (0, a1 - E20), (2, a1 + E20)),            # 2: tilt 1 (margin 0) at max_angle -+ 2^-20: inactive | active; tilt 0 rejects
        _tf_tour(0.3, (2, k0 - E20)),                            # 3: tilt 0 at max_angle + 1e-3 - 2^-20: accepted
        _tf_tour(0.3, (2, k0 + E20)),                            # 4: ... + 2^-20: rejected, by that waypoint alone
        _tf_tour(2.0, (1, -(k0 - E20))),                         # 5: accepted on the other side
        _tf_tour(-0.4, (3, k1 - E20), (1, -(k0 + E20))),         # 6: tilt 1 inside its 1 mrad, tilt 0 rejects
        _tf_tour(0.9, (0, k1 + E20)),                            # 7: tilt 1 beyond it
    ]
    return np.array([G._with_velocities(p) for p in out])


# scenes TE / TEA, exact: alpha = 0 and theta0 = -q in joints 0 and 1, so R_1 = R_2 = I in fp64 at every waypoint; the third
# joint moves freely (dyadic) behind every tilt's frame.  Every vector is dyadic or dotted exactly: c, g and g q need no rounding.
TE_Q = (0.5, -0.25)
CE = DH.chain((0, 0, 0), (0, 0, 0), (0, 0, 0), (-TE_Q[0], -TE_Q[1], 0))
TE_START = (1.0, 0.5)                                           # where the QPs' end conditions sit: the linearised rows hold there
TE_TILTS = [tilt(2, (1, 0, 0), (0.6, 0.8, 0), 0.875, 0.25),     # 0: c = 0.6 < cos(0.876): rejected; active, g = (0.8, 0.8, 0)
            tilt(1, (1, 0, 0), (1, 0, 0), 0.5, 0.25),           # 1: u = ref: c = 1, the row all zeros, inactive
            tilt(2, (1, 0, 0), (0.6, 0.8, 0), 1.5, 0.25),       # 2: the row of tilt 0, inactive: written all the same
            tilt(1, (0, 1, 0), (-0.8, 0.6, 0), 1.0, 0.5)]       # 3: frame 1: c = 0.6, g = (0.8, 0, 0); active (cos(0.5) > 0.6), accepted
TEA_TILTS = TE_TILTS + [tilt(2, (0, 1, 0), (0, -1, 0), 0.5, 0.0)]   # 4: u = -ref: c = -1, the row all zeros, active, l = cos(0.5) + 1
TE_ANGLES = sorted({a for t in TEA_TILTS for a in threshold_angles(t)})
TE_W = 4


def _te_trajectories():
    rng = np.random.default_rng(17)
    out = []
    for k in range(8):
        p = np.empty((TE_W, 3))
        p[:, 0], p[:, 1] = TE_Q
        p[:, 2] = rng.integers(-64, 65, TE_W) / 32.0
        out.append(p)
    return np.array([G._with_velocities(p) for p in out])


# scene TM, the row order: pair_refs' PM (a gripper ball's work-space rows, two lines, a capsule, a cuboid, two pairs) with the
# 3-joint chain of dh_refs and two tilts behind them
TM_TILTS = [tilt(3, (0, 0, 1), (0, 0, 1), 1.6, 0.1), tilt(1, (0, 0.6, 0.8), (0.28, 0, 0.96), 1.3, 0.2)]

SCENES = ("T7", "T8", "TF", "TE", "TEA", "TM")
EXACT = ("TE", "TEA")


@functools.lru_cache(maxsize=None)
def scene(name):
    """name: one of SCENES.  A dict as pair_refs.scene gives, with "tilts" besides; "starts": where the QPs of the batch begin
    and end when that is not the trajectories' first waypoint."""
    if name == "T7":
        return dict(P.scene("P7"), name=name, tilts=T7_TILTS)
    if name == "T8":
        return dict(name=name, D=8, W=2, chain=DH.C8, balls=[DH.chain_ball(DH.C8, 8, (0, 0, 0.02), 0, 0.04)], lines=[], capsules=[], cuboids=[], pairs=[],
                    tilts=T8_TILTS, con_lo=None, con_hi=None, margin=G.MARGIN, trajs=DH._c8_trajectories())
    if name == "TF":
        return dict(name=name, D=2, W=TF_W, chain=CF, balls=[DH.chain_ball(CF, 2, (0, 0, 0), 0, 0.05)], lines=[], capsules=[], cuboids=[], pairs=[],
                    tilts=TF_TILTS, con_lo=None, con_hi=None, margin=G.MARGIN, trajs=_tf_trajectories())
    if name in ("TE", "TEA"):
        trajs = _te_trajectories()
        starts = np.array([[TE_START[0], TE_START[1], t[2]] for t in trajs])
        return dict(name=name, D=3, W=TE_W, chain=CE, balls=[DH.chain_ball(CE, 2, (0, 0, 0), 0, 0.05)], lines=[], capsules=[], cuboids=[], pairs=[],
                    tilts=TE_TILTS if name == "TE" else TEA_TILTS, con_lo=None, con_hi=None, margin=G.MARGIN, trajs=trajs, starts=starts)
    if name == "TM":
        return dict(P.scene("PM"), name=name, chain=DH.C3, tilts=TM_TILTS)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def scene_reference(name, K_=G.MPA):
    """with_obstacles of the scene's eight trajectories."""
    s = scene(name)
    return [with_obstacles(s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["pairs"], s["tilts"], s["con_lo"],
                           s["con_hi"], t, s["margin"], K_) for t in s["trajs"]]


@functools.lru_cache(maxsize=None)
def fp64_error(name):
    """dh_refs.fp64_error for the scenes of this module: the np.float64 evaluation of the formulas against the mpmath one."""
    ev = eb = 0.0
    for hi, lo in zip(scene_reference(name), scene_reference(name, G.F64)):
        v, b = DH.row_distance(hi, lo)
        ev, eb = max(ev, v), max(eb, b)
    return ev, eb


def gpu_tolerance(name):
    """The project's rule (pair_refs.gpu_tolerance): 32 x fp64_error, never looser than 1e-13.  (0, 0) for the exact scenes."""
    ev, eb = fp64_error(name)
    return min(32 * ev, 1e-13), min(32 * eb, 1e-13)


@functools.lru_cache(maxsize=None)
def scene_batch(name, over_allocate=False):
    """pair_refs.scene_problem for the scene's eight trajectories: a tilt's W rows are laid out as a pair's, behind them."""
    s = scene(name)
    D, W = s["D"], s["W"]
    starts = s.get("starts", s["trajs"][:, :D])
    ends = (s["starts"] if "starts" in s else s["trajs"][:, (W - 3) * D:(W - 2) * D]) if W >= 4 else None
    return P.scene_problem(D, W, s["balls"], len(s["lines"]) + len(s["capsules"]) + len(s["cuboids"]), len(s["pairs"]) + len(s["tilts"]), 8,
                           over_allocate, starts=starts, ends=ends)


def populations(name):
    """Counts a test can assert on and print: tilt rows per class and tilt, rejecting tilt rows, verdicts, causes, exclusions."""
    s, ref = scene(name), scene_reference(name)
    nt = len(s["tilts"])
    cells = {c: np.zeros(nt, int) for c in CLASSES}
    rejecting = np.zeros(nt, int)
    near = rows = 0
    causes, only_tilt = {}, 0
    for e in ref:
        for k in range(len(e["l"])):
            near += bool(e["near"][k])
            if e["tilt"][k] < 0:
                continue
            cells[e["cls"][k]][int(e["tilt"][k])] += 1
            rows += 1
        for m in e["margins"]:
            if m["kind"] == "tilt":
                rejecting[m["idx"]] += bool(m["slack"] < 0)
        for c in e["causes"]:
            causes[c] = causes.get(c, 0) + 1
        only_tilt += e["causes"] == {"tilt"}
    return dict(cells=cells, rejecting=rejecting, near=near, tilt_rows=rows, accepted=sum(e["ok"] for e in ref), rejected=sum(not e["ok"] for e in ref),
                causes=causes, rejected_by_a_tilt_alone=only_tilt, verdicts_excluded=sum(e["verdict_excluded"] for e in ref),
                near_comparisons=sum(m["near"] for e in ref for m in e["margins"]))


# ------------------------------------------------------------------ the known answers in tests/golden/tilt_kats.json

KAT_SCENES = ("TF", "TE", "TEA", "TM")


def kats_now():
    """What tests/golden/tilt_kats.json holds, computed now: per scene and trajectory the rows (vals, l, u as JSON numbers: the
    shortest decimal that reads back as the same double) and the verdict of the mpmath reference."""
    out = {}
    for name in KAT_SCENES:
        out[name] = [dict(vals=[[float(x) for x in row] for row in e["vals"]], l=[float(x) for x in e["l"]], u=[float(x) for x in e["u"]],
                          ok=bool(e["ok"])) for e in scene_reference(name)]
    return out


def kats_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tilt_kats.json")


def load_kats():
    with open(kats_path()) as f:
        return json.load(f)


# ------------------------------------------------------------------ ctypes: mi_gomp_scene_create_tilts (tests only)

class Tilt(C.Structure):
    _fields_ = [("frame", C.c_int32), ("reserved", C.c_int32), ("axis", C.c_double * 3), ("ref", C.c_double * 3), ("max_angle", C.c_double),
                ("margin", C.c_double)]


def c_tilts(tilts):
    arr = (Tilt * max(len(tilts), 1))()
    for k, t in enumerate(tilts):
        arr[k].frame, arr[k].max_angle, arr[k].margin = t["frame"], t["max_angle"], t["margin"]
        for i in range(3):
            arr[k].axis[i], arr[k].ref[i] = t["axis"][i], t["ref"][i]
    return arr


def declare(L):
    P.declare(L)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    L.mi_gomp_scene_create_tilts.argtypes = [C.POINTER(vp), vp, C.c_int64, C.c_int64, C.POINTER(DH.Chain), C.c_int64, C.POINTER(G.Ball), C.c_int64,
                                             C.POINTER(G.Line), C.c_int64, C.POINTER(K.Capsule), C.c_int64, C.POINTER(X.Cuboid), C.c_int64, C.POINTER(P.Pair),
                                             C.c_int64, C.POINTER(Tilt), dp, dp]
    L.mi_gomp_scene_create_tilts.restype = C.c_int
    return L


def create_tilts(L, handle, D, W, ch, balls, lines, capsules, cuboids, pairs, tilts, con_lo=None, con_hi=None, n_tilts=None, null_tilts=False):
    """(rc, scene pointer) of mi_gomp_scene_create_tilts; ch: a Chain, a chain dict or None.  n_tilts / null_tilts override what is
    passed for the tilt count and array (the refusals).  The pointer starts as a value that is not NULL, so a refusal shows that it
    was cleared."""
    ptr = C.c_void_p(1)
    lo = None if con_lo is None else np.ascontiguousarray(con_lo, np.float64)
    hi = None if con_hi is None else np.ascontiguousarray(con_hi, np.float64)
    cc = DH.c_chain(ch) if isinstance(ch, dict) else ch
    rc = L.mi_gomp_scene_create_tilts(C.byref(ptr), handle, D, W, None if cc is None else C.byref(cc), len(balls), G.c_balls(balls), len(lines),
                                      G.c_lines(lines), len(capsules), K.c_capsules(capsules), len(cuboids), X.c_cuboids(cuboids),
                                      len(pairs), P.c_pairs(pairs), len(tilts) if n_tilts is None else n_tilts, None if null_tilts else c_tilts(tilts),
                                      G._dp(lo), G._dp(hi))
    return rc, ptr


class TiltScene(G.GompScene):
    """gomp_refs.GompScene made by mi_gomp_scene_create_tilts."""

    def __init__(self, L, solver, D, W, ch, balls, lines, capsules, cuboids, pairs, tilts, con_lo, con_hi):
        self.L, self.solver = declare(L), solver
        self.rc, self.ptr = create_tilts(L, solver._h, D, W, ch, balls, lines, capsules, cuboids, pairs, tilts, con_lo, con_hi)
