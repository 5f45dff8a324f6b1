"""The DH-chain ball model (MI_GOMP_MODEL_DH_CHAIN) beside tests/gomp_refs.py: a helper module of the tests, not a conftest.

A serial chain of revolute joints given by its standard DH table, T_i = Rz(q_i + theta0_i) Tz(d_i) Tx(a_i) Rx(alpha_i), with
balls fixed at a centre c in frame k (the frame after k joints): p = o_k + R_k c, Jacobian column j = z_j x (p - o_j) for
j < k and 0 for j >= k - restated here from those formulas alone in mpmath at 50 digits and in np.float64 (gomp_refs.MPA /
F64).  alpha and theta0 enter as the doubles the C-ABI receives: the reference is exact for the numbers the library is given.

gomp_refs._evaluate calls the module-level gomp_refs.fk_jac; importing this module rebinds it to a wrapper that serves balls
of model 6 (their dict carries the chain under "chain") and hands every other model to the original, so the row rule, the
collision classes and the verdict are gomp_refs' own and a scene may mix chain balls with the built-in models.

The scenes of tests/test_gpu_gomp_chain.py are defined here (scene / scene_reference) so that tests/test_dh_refs.py can check
their populations on the CPU first; the ctypes declarations of mi_gomp_scene_create_chain take the library as an argument."""
import ctypes as C
import functools

import numpy as np

import gomp_refs as G

DH_CHAIN = 6                    # mi_gomp_model
H = np.pi / 2
MAXD = 8


def chain(a, d, alpha, theta0):
    n = len(a)
    assert len(d) == len(alpha) == len(theta0) == n and 1 <= n <= MAXD
    return dict(a=[float(v) for v in a], d=[float(v) for v in d], alpha=[float(v) for v in alpha], theta0=[float(v) for v in theta0])


C7 = chain((0, 0, 0.0825, -0.0825, 0, 0.088, 0), (0.333, 0, 0.316, 0, 0.384, 0, 0.107), (-H, H, H, -H, H, H, 0.3), (0, 0, 0, 0.25, 0, 0, -0.7))
C8 = chain(C7["a"] + [0.05], C7["d"] + [0.1], C7["alpha"] + [0.0], C7["theta0"] + [0.0])
UR5E = chain(G.UR5E_A, G.UR5E_D, [k * H for k in G.UR5E_ALPHA_HALF_PI], [0.0] * 6)
C3 = chain((0, 0.4, 0.3), (0.2, 0, 0), (H, 0.1, -0.2), (0, 0.3, 0))          # the mixed scene's 3-joint chain


# ------------------------------------------------------------------ kinematics

def chain_frames(ch, q, K=G.MPA):
    """Origins o_0 .. o_n and rotations R_0 .. R_n (lists of rows) of the chain at q: frame k is the frame after k joints."""
    one, zero = K.num(1), K.num(0)
    R = [[one, zero, zero], [zero, one, zero], [zero, zero, one]]
    o = [zero, zero, zero]
    origins, rots = [list(o)], [R]
    for i in range(len(ch["a"])):
        th = K.num(q[i]) + K.num(ch["theta0"][i])
        ct, st = K.cos(th), K.sin(th)
        al = K.num(ch["alpha"][i])
        ca, sa = K.cos(al), K.sin(al)
        a, d = K.num(ch["a"][i]), K.num(ch["d"][i])
        T = [[ct, -st * ca, st * sa, a * ct], [st, ct * ca, -ct * sa, a * st], [zero, sa, ca, d]]
        Rn = [[R[r][0] * T[0][c] + R[r][1] * T[1][c] + R[r][2] * T[2][c] for c in range(3)] for r in range(3)]
        o = [R[r][0] * T[0][3] + R[r][1] * T[1][3] + R[r][2] * T[2][3] + o[r] for r in range(3)]
        R = Rn
        origins.append(list(o))
        rots.append(R)
    return origins, rots


def chain_point(ch, q, frame, c, K=G.MPA, frames=None):
    """(p, J[3][n]) of the point c of frame `frame`: p = o_k + R_k c, column j = z_j x (p - o_j) for j < frame, else 0."""
    n = len(ch["a"])
    assert 1 <= frame <= n
    origins, rots = frames if frames is not None else chain_frames(ch, q, K)
    Rk, c = rots[frame], [K.num(v) for v in c]
    p = [origins[frame][r] + (Rk[r][0] * c[0] + Rk[r][1] * c[1] + Rk[r][2] * c[2]) for r in range(3)]
    J = [[K.num(0)] * n for _ in range(3)]
    for j in range(frame):
        z = [rots[j][0][2], rots[j][1][2], rots[j][2][2]]
        col = G._cross(z, [p[k] - origins[j][k] for k in range(3)])
        for ax in range(3):
            J[ax][j] = col[ax]
    return p, J


_builtin_fk_jac = getattr(G.fk_jac, "_builtin", G.fk_jac)


def fk_jac(ball, q, w, K=G.MPA, cache=None):
    """gomp_refs.fk_jac with model 6: (p, J[3][D]) of one ball at joint position q (waypoint w)."""
    if ball["model"] != DH_CHAIN:
        return _builtin_fk_jac(ball, q, w, K, cache)
    frames = None
    if cache is not None:
        key = (K.name, w, "dh")
        if key not in cache:
            cache[key] = chain_frames(ball["chain"], q, K)
        frames = cache[key]
    frame = int(ball["param"][0])
    assert frame == ball["param"][0]
    return chain_point(ball["chain"], q, frame, ball["param"][1:4], K, frames)


fk_jac._builtin = _builtin_fk_jac
G.fk_jac = fk_jac               # (one chain per scene: the cache of _evaluate is per scene and trajectory)


def chain_ball(ch, frame, centre, gripper, radius):
    b = G._ball(DH_CHAIN, gripper, radius, [float(frame)] + [float(v) for v in centre])
    b["chain"] = ch
    return b


# ------------------------------------------------------------------ the scenes of the GPU tests

LINE0 = dict(dir=[1.0, 0.0], point=[0.0, 0.0, 0.2], below=False)
LINE1 = dict(dir=[1.0, 1.0], point=[0.4, 0.0, 0.9], below=True)
BOX_LO, BOX_HI = [-G.INF, -G.INF, 0.15], [0.75, G.INF, G.INF]
BASE7 = np.array([0, 0.4, 0, -1.6, 0, 1.9, 0.6])


def _c7_trajectories(W):
    rng = np.random.default_rng(71)
    U = lambda *s: rng.uniform(-1, 1, s)
    base = BASE7
    out = []
    for k in range(8):
        if k < 3:
            a, b = base + 0.3 * U(7), base + 0.3 * U(7)
            a[0] += -1.2
            b[0] += 1.2 * (1.0 if k % 2 else 0.4)
            pos = G._sweep(W, a, b, -0.7 if k == 1 else 0.0)
        elif k < 5:
            a = base + 0.05 * U(7)
            a[0] = -1.0
            b = a.copy()
            b[0] = 1.0
            b[1] += 0.1
            if k == 4:
                a[1] += 0.9
                b[1] += 0.9
                a[3] += 0.9
                b[3] += 0.9
            pos = G._jump(W, a, b, 0.2, 0.8)
        else:
            a = base + 0.1 * U(7)
            a[0] = 2.5
            b = a + 0.1 * U(7)
            if k == 7:
                b[1] += 1.3
            pos = G._sweep(W, a, b, 0.0)
        out.append(pos)
    return np.array([G._with_velocities(p) for p in out])


def _c8_trajectories():
    rng = np.random.default_rng(88)
    base8 = np.append(BASE7, 0.0)
    out = []
    for k in range(8):
        a = base8 + 0.3 * rng.uniform(-1, 1, 8)
        b = base8 + 0.3 * rng.uniform(-1, 1, 8)
        a[0] += -1.0 if k % 2 == 0 else 0.6
        b[0] += 1.0 if k < 4 else 0.9
        if k in (2, 6):
            a[1] += 0.9
            a[3] += 0.9
        out.append(np.array([a, b]))
    return np.array([G._with_velocities(p) for p in out])


def _m3_trajectories(W):
    rng = np.random.default_rng(33)
    out = []
    for k in range(8):
        a, b = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
        out.append(a + np.linspace(0.0, 1.0, W)[:, None] * (b - a))
    return np.array([G._with_velocities(p) for p in out])


SCENES = ("C7", "C8", "UC")


@functools.lru_cache(maxsize=None)
def scene(name):
    """name: "C7", "C8", "UC" (scene U of gomp_refs through the chain), "M3" (a chain ball beside a TABLE ball, D = 3).
    A dict as gomp_refs.scene gives, with "chain" besides."""
    if name == "C7":
        W = 40
        spec = [(2, (0, 0, 0), 0, 0.09), (3, (0, 0.05, -0.1), 0, 0.08), (4, (0.02, 0, 0.03), 0, 0.07), (5, (0, 0.04, -0.15), 0, 0.07),
                (6, (0.03, 0, 0), 0, 0.06), (7, (0, 0, -0.05), 0, 0.05), (7, (0.02, -0.01, 0.06), 1, 0.04)]
        return dict(name=name, D=7, W=W, chain=C7, balls=[chain_ball(C7, *s) for s in spec], lines=[LINE0, LINE1], con_lo=BOX_LO, con_hi=BOX_HI,
                    margin=G.MARGIN, trajs=_c7_trajectories(W))
    if name == "C8":
        balls = [chain_ball(C8, 1, (0.1, 0, 0), 0, 0.05), chain_ball(C8, 8, (0, 0, 0.02), 1, 0.04)]
        return dict(name=name, D=8, W=2, chain=C8, balls=balls, lines=[LINE0], con_lo=BOX_LO, con_hi=BOX_HI, margin=G.MARGIN, trajs=_c8_trajectories())
    if name == "UC":
        u = G.scene("U")
        balls = [chain_ball(UR5E, G.UR5E_FRAME[b["model"]], (0, 0, 0), b["gripper"], b["radius"]) for b in u["balls"]]
        return dict(u, name=name, chain=UR5E, balls=balls)
    if name == "M3":
        W = 5
        balls = [chain_ball(C3, 3, (0.05, 0.0, 0.02), 1, 0.03), G._ball(G.TABLE, 0, 1 / 8, G.T_TABLES[1]), chain_ball(C3, 2, (0.0, 0.1, 0.0), 0, 0.05)]
        return dict(name=name, D=3, W=W, chain=C3, balls=balls, lines=[dict(dir=[1.0, 0.0], point=[0.0, 0.1, 0.3], below=False)],
                    con_lo=[-G.INF, -G.INF, 0.0], con_hi=None, margin=G.MARGIN, trajs=_m3_trajectories(W))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def scene_reference(name, K=G.MPA):
    """gomp_refs.with_obstacles of the scene's eight trajectories."""
    s = scene(name)
    return [G.with_obstacles(s["D"], s["W"], s["balls"], s["lines"], s["con_lo"], s["con_hi"], t, s["margin"], K) for t in s["trajs"]]


def row_distance(hi, lo):
    """(values, bounds) between two evaluations of one trajectory's rows, as gomp_refs.fp64_error measures them: absolute for
    the matrix values, per term scale for the bounds, without the rows near a decision or of different classes."""
    ev = float(np.max(np.abs(hi["vals"] - lo["vals"])))
    eb = 0.0
    same = np.array([a == b for a, b in zip(hi["cls"], lo["cls"])]) & ~hi["near"]
    for side in ("l", "u"):
        sc = hi[side + "_scale"]
        use = same & (sc > 0)
        if use.any():
            eb = max(eb, float(np.max(np.abs(hi[side] - lo[side])[use] / sc[use])))
    return ev, eb


@functools.lru_cache(maxsize=None)
def fp64_error(name):
    """gomp_refs.fp64_error for the scenes of this module."""
    ev = eb = 0.0
    for hi, lo in zip(scene_reference(name), scene_reference(name, G.F64)):
        v, b = row_distance(hi, lo)
        ev, eb = max(ev, v), max(eb, b)
    return ev, eb


def gpu_tolerance(name):
    """The project's rule (gomp_refs.gpu_tolerance): 32 x fp64_error, never looser than 1e-13."""
    ev, eb = fp64_error(name)
    return min(32 * ev, 1e-13), min(32 * eb, 1e-13)


@functools.lru_cache(maxsize=None)
def scene_batch(name, over_allocate=False):
    s = scene(name)
    D, W = s["D"], s["W"]
    ends = s["trajs"][:, (W - 3) * D:(W - 2) * D] if W >= 4 else None
    return G.scene_problem(D, W, s["balls"], len(s["lines"]), 8, over_allocate, starts=s["trajs"][:, :D], ends=ends)


def populations(name):
    """gomp_refs.populations for the scenes of this module."""
    s, ref = scene(name), scene_reference(name)
    nb, nl, W = len(s["balls"]), len(s["lines"]), s["W"]
    cls = {c: np.zeros((nb, nl), int) for c in G.CLASSES}
    near = total = 0
    for e in ref:
        for d in e["decisions"]:
            cls[d["cls"]][d["ball"], d["line"]] += 1
            near += d["near"]
            total += 1
    causes = {}
    for e in ref:
        for c in e["causes"]:
            causes[c] = causes.get(c, 0) + 1
    return dict(cls=cls, near=near, decisions=total, accepted=sum(e["ok"] for e in ref), rejected=sum(not e["ok"] for e in ref), causes=causes,
                verdicts_excluded=sum(e["verdict_excluded"] for e in ref), near_comparisons=sum(m["near"] for e in ref for m in e["margins"]))


# ------------------------------------------------------------------ ctypes: mi_gomp_scene_create_chain (tests only)

class Chain(C.Structure):
    _fields_ = [("n_joints", C.c_int32), ("reserved", C.c_int32), ("a", C.c_double * MAXD), ("d", C.c_double * MAXD),
                ("alpha", C.c_double * MAXD), ("theta0", C.c_double * MAXD)]


def c_chain(ch, n_joints=None):
    out = Chain()
    out.n_joints = len(ch["a"]) if n_joints is None else n_joints
    for k in ("a", "d", "alpha", "theta0"):
        for i, v in enumerate(ch[k]):
            getattr(out, k)[i] = v
    return out


def declare(L):
    G.declare(L)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    L.mi_gomp_scene_create_chain.argtypes = [C.POINTER(vp), vp, C.c_int64, C.c_int64, C.POINTER(Chain), C.c_int64, C.POINTER(G.Ball), C.c_int64,
                                             C.POINTER(G.Line), dp, dp]
    L.mi_gomp_scene_create_chain.restype = C.c_int
    L.mi_osqp_last_error.restype = C.c_char_p
    return L


def create_chain(L, handle, D, W, ch, balls, lines, con_lo=None, con_hi=None):
    """(rc, scene pointer) of mi_gomp_scene_create_chain; ch: a Chain, a chain dict or None."""
    ptr = C.c_void_p()
    lo = None if con_lo is None else np.ascontiguousarray(con_lo, np.float64)
    hi = None if con_hi is None else np.ascontiguousarray(con_hi, np.float64)
    cc = c_chain(ch) if isinstance(ch, dict) else ch
    rc = L.mi_gomp_scene_create_chain(C.byref(ptr), handle, D, W, None if cc is None else C.byref(cc), len(balls), G.c_balls(balls), len(lines),
                                      G.c_lines(lines), G._dp(lo), G._dp(hi))
    return rc, ptr


class ChainScene(G.GompScene):
    """gomp_refs.GompScene made by mi_gomp_scene_create_chain."""

    def __init__(self, L, solver, D, W, ch, balls, lines, con_lo, con_hi):
        self.L, self.solver = declare(L), solver
        self.rc, self.ptr = create_chain(L, solver._h, D, W, ch, balls, lines, con_lo, con_hi)
