"""CPU: the DH-chain ball model before anything runs on a GPU - the reference of tests/dh_refs.py against its own forward
kinematics and against scene U of gomp_refs, the populations of the scenes of tests/test_gpu_gomp_chain.py, the fp64 error
from which their GPU tolerance is derived, the QPs that test solves, the C-ABI of mi_gomp_scene_create_chain as far as it
needs no handle, and the host twin include/mi_osqp/dh_kinematics.hpp.

Measured here (np.float64 evaluation of the formulas against the mpmath one over the eight trajectories of each scene; values
absolute, bounds divided by the sum of the absolute values of their terms):

    scene C7 (7 joints, W = 40, 7 balls = 280 pairs, 2 lines):  values 3.3e-16, bounds 3.3e-16
    scene C8 (8 joints, W = 2, 2 balls, 1 line):                values 2.8e-16, bounds 2.5e-16
    scene UC (scene U through the chain):                       values 3.3e-16, bounds 3.2e-16
    scene M3 (3 joints, a chain ball beside a TABLE ball):      values 2.2e-16, bounds 2.8e-16

-> GPU tolerance 32 x the figure (about 1e-14), never looser than 1e-13.  UC's mpmath rows against U's (alpha = the double
nearest k pi/2 against the exact k pi/2): values within 1.2e-16, bounds within 1.2e-16 of their term scale (asserted: 1.2e-16
and 2.3e-16), same classes and verdicts.  Populations: C7 3 accepted / 5 rejected with all four causes, every class on both
lines; C8 4 / 4 with box_low, box_high and not_above; no decision within the margin 1e-9, no verdict excluded.  The rejected
QPs of C7 on the oracle (scaling 0, warm start = the trajectory): QPs 1 and 2 optimal after 75 and 25 iterations, QPs 0, 4 and
7 primal infeasible.  Chain Jacobians against central differences of the chain FK (h = 1e-15, 50 digits): worst below 1e-20.
Run with -s to see the figures."""
import ctypes as C
import os
import re
import subprocess

import mpmath
import numpy as np
import pytest

import dh_refs as DH
import gomp_refs as G

MP = G.MP
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NULL = 1, 6                               # MI_OSQP_ERR_INVALID_DATA, MI_OSQP_ERR_NULL


def test_jacobians_equal_central_differences_of_the_chain_forward_kinematics():
    rng = np.random.default_rng(6)
    h = MP.mpf("1e-15")
    worst = MP.mpf(0)
    for ch in (DH.C7, DH.C8):
        n = len(ch["a"])
        q = rng.uniform(-np.pi, np.pi, n)
        for frame in range(1, n + 1):
            c = rng.uniform(-0.2, 0.2, 3)
            assert np.all(c != 0)
            _, J = DH.chain_point(ch, q, frame, c)
            for j in range(n):
                qp, qm = [MP.mpf(v) for v in q], [MP.mpf(v) for v in q]
                qp[j] += h
                qm[j] -= h
                a, b = DH.chain_point(ch, qp, frame, c)[0], DH.chain_point(ch, qm, frame, c)[0]
                worst = max(worst, max(abs(J[ax][j] - (a[ax] - b[ax]) / (2 * h)) for ax in range(3)))
                if j >= frame:
                    assert all(J[ax][j] == 0 for ax in range(3))
    print(f"\nchain Jacobian against central differences (h = 1e-15, {MP.dps} digits): worst {mpmath.nstr(worst, 3)}")
    assert MP.dps >= 40 and worst <= MP.mpf("1e-20")


def test_the_wrapper_serves_model_6_and_delegates_the_rest():
    assert G.fk_jac is DH.fk_jac
    q = [0.3, -0.2, 0.5, 0.1, -0.4, 0.2]
    for model, frame in G.UR5E_FRAME.items():
        p, J = G.fk_jac(G._ball(model, 0, 0.1), q, 0)
        p0, J0 = G.ur5e_point(q, frame)
        assert p == p0 and J == J0
    ball = G._ball(G.YAW_2LINK, 1, 0.03, G.Y_PARAMS[0])
    assert G.fk_jac(ball, q[:3], 0) == G.yaw_2link(q[:3], ball["param"])
    with pytest.raises(ValueError):
        G.fk_jac(G._ball(7, 0, 0.1), q, 0)
    # the first ball of C7 sits on the axis of joint 2: nothing moves it but joint 0... and that one it does not move either
    s = DH.scene("C7")
    _, J = G.fk_jac(s["balls"][0], s["trajs"][0][:7], 0)
    assert all(abs(J[ax][j]) < MP.mpf("1e-40") for ax in range(3) for j in range(7))


def test_scene_UC_reproduces_scene_U():
    u, uc = G.scene_reference("U"), DH.scene_reference("UC")
    ev = eb = 0.0
    for a, b in zip(u, uc):
        assert a["cls"] == b["cls"] and a["ok"] == b["ok"] and a["causes"] == b["causes"]
        assert a["verdict_excluded"] == b["verdict_excluded"] and np.array_equal(a["near"], b["near"])
        v, bb = DH.row_distance(a, b)
        ev, eb = max(ev, v), max(eb, bb)
    tv, tb = G.gpu_tolerance("U")
    print(f"\nscene UC against scene U (mpmath both): values {ev:.3e}, bounds {eb:.3e} of their term scale; U's GPU tolerance {tv:.3e} / {tb:.3e}")
    assert ev <= 1.2e-16 and eb <= 2.3e-16


@pytest.mark.parametrize("name", ["C7", "C8"])
def test_scene_populations(name):
    s, p = DH.scene(name), DH.populations(name)
    W, nb, nl = s["W"], len(s["balls"]), len(s["lines"])
    print(f"\nscene {name}: D = {s['D']}, W = {W}, {nb} balls ({nb * W} pairs), {nl} lines; accepted {p['accepted']}, rejected {p['rejected']},"
          f" causes {dict(sorted(p['causes'].items()))}")
    for c in G.CLASSES:
        print(f"  {c:5s}: rows per ball and line {p['cls'][c].tolist()}")
    print(f"  decisions within the margin {s['margin']:g}: {p['near']} of {p['decisions']}; comparisons of the verdict within it:"
          f" {p['near_comparisons']}; verdicts excluded: {p['verdicts_excluded']}")
    assert len(s["trajs"]) == 8 and s["trajs"].shape[1] == 2 * s["D"] * W
    assert len({t.tobytes() for t in s["trajs"]}) == 8
    assert p["accepted"] >= 2 and p["rejected"] >= 2
    assert p["verdicts_excluded"] <= 1 and p["near"] <= 0.01 * p["decisions"]          # the caps
    assert p["verdicts_excluded"] == 0 and p["near"] == 0 and p["near_comparisons"] == 0  # and what the committed trajectories give
    if name == "C7":
        assert nb * W == 280 > 256
        assert (p["accepted"], p["rejected"]) == (3, 5)
        assert set(p["causes"]) == {"box_low", "box_high", "not_above", "not_below"}
        for li in range(nl):
            for c in ("close", "prev", "next"):
                assert p["cls"][c][:, li].sum() >= 1, (c, li)
    else:
        assert (s["D"], W) == (8, 2)
        assert (p["accepted"], p["rejected"]) == (4, 4)
        assert set(p["causes"]) == {"box_low", "box_high", "not_above"}
        for c in G.CLASSES:
            assert p["cls"][c].sum() >= 1, c


@pytest.mark.parametrize("name", ["C7", "C8", "UC", "M3"])
def test_fp64_error_and_gpu_tolerance(name):
    ev, eb = DH.fp64_error(name)
    tv, tb = DH.gpu_tolerance(name)
    print(f"\nscene {name}: fp64 error of the formulas: values {ev:.3e} (absolute), bounds {eb:.3e} (per term scale); GPU tolerance {tv:.3e} / {tb:.3e}")
    assert 0.0 < ev <= 1e-13 / 32 and 0.0 < eb <= 1e-13 / 32
    assert tv == 32 * ev and tb == 32 * eb


def test_the_rejected_qps_of_scene_C7_on_the_oracle():
    """The QPs that tests/test_gpu_gomp_chain.py solves after mi_gomp_relinearise_some: two have an optimum, three are infeasible."""
    from oracle import oracle as O
    s, ref, pr = DH.scene("C7"), DH.scene_reference("C7"), DH.scene_batch("C7")
    got = {}
    for b in range(8):
        if ref[b]["ok"]:
            continue
        Ax, l, u = G.reference_rows(pr, b, ref[b])
        A = pr["A"].copy()
        A.data = Ax
        o = O.OracleQPSolver(pr["P"], None, pr["A"], pr["l"][b], pr["u"][b], scaling=0)
        o.update(l, A, u)
        o.set_warm_start(s["trajs"][b])
        st, _ = o.solve()
        got[b] = st
        print(f"\noracle on the re-linearised QP {b} of scene C7: status {st}, {o.info().iter} iterations")
    assert got == {0: -3, 1: 1, 2: 1, 4: -3, 7: -3}


# ------------------------------------------------------------------ the C-ABI, as far as it needs no handle

def test_abi_entry_point_enum_and_struct():
    import osqp_solver_amd as M
    with open(os.path.join(ROOT, "include", "mi_osqp.h")) as f:
        src = f.read()
    assert re.search(r"\bMI_GOMP_MODEL_DH_CHAIN\s*=\s*6\b", src)
    assert re.search(r"typedef struct \{ int32_t n_joints; int32_t reserved; double a\[8\], d\[8\], alpha\[8\], theta0\[8\]; \} mi_gomp_chain;", src)
    assert re.search(r"\bint mi_gomp_scene_create_chain\(mi_gomp_scene \*\*out, mi_osqp_batch \*h, int64_t dims, int64_t waypoints,\s*"
                     r"const mi_gomp_chain \*chain, int64_t n_balls, const mi_gomp_ball \*balls,", src)
    assert C.sizeof(DH.Chain) == 264
    assert hasattr(M.lib(), "mi_gomp_scene_create_chain")


def test_refusals_that_need_no_handle():
    import osqp_solver_amd as M
    L = DH.declare(M.lib())
    s = DH.scene("C8")
    balls, lines = s["balls"], s["lines"]

    def refused(code, ch, bl=balls, D=8, why=None):
        rc, ptr = DH.create_chain(L, None, D, 2, ch, bl, lines, s["con_lo"], s["con_hi"])
        assert rc == code and not ptr, (rc, ptr, L.mi_osqp_last_error())
        if why:
            assert why in L.mi_osqp_last_error().decode(), L.mi_osqp_last_error()

    refused(NULL, None, why="no chain")                                       # a chain ball, no chain
    refused(INVALID, DH.c_chain(DH.C8, 0), why="n_joints")
    refused(INVALID, DH.c_chain(DH.C8, 9), why="n_joints")
    refused(INVALID, DH.c_chain(DH.C8, -1), why="n_joints")
    refused(INVALID, DH.C7, why="dims")                                       # n_joints = 7, dims = 8
    refused(INVALID, DH.C8, D=7, why="dims")
    for key, bad in (("a", np.inf), ("d", -np.inf), ("alpha", np.nan), ("theta0", np.nan)):
        ch = {k: list(v) for k, v in DH.C8.items()}
        ch[key][7] = bad
        refused(INVALID, ch, why="not finite")
    for k, bad in ((1, np.nan), (3, np.inf), (0, np.nan)):
        b = dict(balls[1], param=list(balls[1]["param"]))
        b["param"][k] = bad
        refused(INVALID, DH.C8, [balls[0], b], why="not finite")
    refused(INVALID, DH.C8, [balls[0], dict(balls[1], radius=np.nan)], why="not finite")
    for frame in (0.0, 9.0, 2.5, -1.0, 1e300):
        b = dict(balls[1], param=[frame] + list(balls[1]["param"][1:]))
        refused(INVALID, DH.C8, [b, balls[0]], why="param[0]")
    refused(NULL, DH.C8)                                                      # all of it in order: the handle is missing
    cc = DH.c_chain(DH.C8)
    assert L.mi_gomp_scene_create_chain(None, None, 8, 2, C.byref(cc), len(balls), G.c_balls(balls), 1, G.c_lines(lines), None, None) == NULL
    out = C.c_void_p()
    assert L.mi_gomp_scene_create_chain(C.byref(out), None, 8, 2, C.byref(cc), len(balls), None, 1, G.c_lines(lines), None, None) == NULL and not out
    assert L.mi_gomp_scene_create_chain(C.byref(out), None, 8, 2, C.byref(cc), len(balls), G.c_balls(balls), 1, None, None, None) == NULL and not out


# ------------------------------------------------------------------ the host twin, include/mi_osqp/dh_kinematics.hpp

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import osqp_solver_amd as M
    from oracle import oracle as O
    M.lib(); O.lib()
    out = tmp_path_factory.mktemp("gomp_chain") / "gomp_chain"
    libdir, ordir = os.path.join(ROOT, "osqp-solver_amd"), os.path.join(ROOT, "oracle", "_build")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gomp_chain.cpp"),
                    "-o", str(out), "-L" + libdir, "-lmi_osqp", "-L" + ordir, "-loracle_osqp", "-fopenmp", "-pthread",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath," + ordir], check=True)
    return str(out)


@pytest.mark.parametrize("name", ["C8", "UC"])
def test_host_twin_against_the_reference(exe, name, tmp_path):
    s = DH.scene(name)
    ch, D, W, balls = s["chain"], s["D"], s["W"], s["balls"]
    Q = np.concatenate([t[:D * W].reshape(W, D) for t in s["trajs"]])
    hx = lambda vals: " ".join(float(v).hex() for v in vals)
    text = [str(D)] + [hx(ch[k]) for k in ("a", "d", "alpha", "theta0")] + [str(len(balls))]
    text += [f"{int(b['param'][0])} {hx(b['param'][1:4])}" for b in balls] + [str(len(Q))] + [hx(q) for q in Q]
    path = tmp_path / "points.txt"
    path.write_text("\n".join(text) + "\n")
    r = subprocess.run([exe, "host", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST OK" in r.stdout, r.stdout[-2000:] + r.stderr
    rows = {"P": [], "U": []}
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] in rows:
            rows[t[0]].append([float.fromhex(v) for v in t[2:]])
    got = np.array(rows["P"]).reshape(len(Q), len(balls), 3 + 3 * D)
    tv, _ = DH.gpu_tolerance(name)
    want = np.empty_like(got)
    for w, q in enumerate(Q):
        frames = DH.chain_frames(ch, q)
        for b, ball in enumerate(balls):
            p, J = DH.chain_point(ch, q, int(ball["param"][0]), ball["param"][1:4], frames=frames)
            want[w, b] = [float(v) for v in p] + [float(J[ax][j]) for ax in range(3) for j in range(D)]
    worst = float(np.max(np.abs(got - want)))
    print(f"\nscene {name}: dh::point against the reference over {len(Q)} positions x {len(balls)} balls: worst {worst:.3e} (tolerance {tv:.3e})")
    assert worst <= tv
    if name == "UC":                                                          # and ur5e_kinematics.hpp's own functions give the same points
        own = np.array(rows["U"]).reshape(got.shape)
        d_own = float(np.max(np.abs(own - got)))
        print(f"  ur5e_kinematics.hpp against dh::point: worst {d_own:.3e}")
        assert d_own <= tv and float(np.max(np.abs(own - want))) <= tv
    else:
        assert not rows["U"]


def test_chain_planner_on_the_oracle_backend(exe):
    """The planning problems of `gomp_chain cont` through the sequential driver on the oracle: the dhBall callbacks alone."""
    r = subprocess.run([exe, "oracle"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ORACLE OK" in r.stdout, r.stdout + r.stderr
