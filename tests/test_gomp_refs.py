"""CPU: the reference of the device re-linearisation (tests/gomp_refs.py) against the reference project's known answers
(tests/golden/gomp_scene_kats.json), against its own kinematics, and - before anything runs on a GPU - the inputs of
tests/test_gpu_gomp_scene.py: which collision classes, verdicts and rejection causes each scene holds, how many decisions
sit within the exclusion margin, and the fp64 error from which the GPU tolerance is derived.

Measured here (np.float64 evaluation of the reference's formulas against its mpmath evaluation, over the eight trajectories
of each scene; values absolute, bounds divided by the sum of the absolute values of their terms):

    scene U (UR5e, W = 90):        values 3.3e-16, bounds 3.2e-16   -> GPU tolerance 1.07e-14 / 1.02e-14 x term scale
    scene Y (yaw + 2 links, 130):  values 2.2e-16, bounds 2.4e-16   -> GPU tolerance 7.1e-15 / 7.6e-15 x term scale
    scene T (table, dyadic):       0, 0                             -> bitwise

(32 x the figure, never looser than 1e-13; the project's figure for the device against its host twin is 1e-12.)
Run with -s to see the figures and the population of every scene."""
import mpmath
import numpy as np
import pytest

import gomp_refs as G

MP = G.MP


@pytest.fixture(scope="module")
def kats():
    return G.load_kats()


def test_line_known_answers(kats):
    k = kats["line_x_axis"]
    line = dict(dir=k["dir"], point=k["point"], below=False)
    for c in k["distance"]:
        d = G.distance_vec(line, c["p"])
        n2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        assert float(MP.sqrt(n2)) == (c["norm"] if "norm" in c else np.sqrt(c["norm_squared"]))
    for c in k["distance_xy"]:
        d = G.distance_vec(line, c["p"])
        assert float(MP.sqrt(d[0] * d[0] + d[1] * d[1])) == c["norm"]
    p = k["closest"]["p"]
    d = G.distance_vec(line, p)
    assert [float(MP.mpf(p[i]) + d[i]) for i in range(3)] == k["closest"]["expected"]


def test_row_known_answers(kats):
    for k in kats["rows"]:
        D, W = k["dims"], k["waypoints"]
        ball = dict(model=G.FIXED if k["points"] else G.TABLE, gripper=k["gripper"], radius=k["radius"], param=k["table"] + [0.0] * 3,
                    points=k["points"])
        r = G.with_obstacles(D, W, [ball], [], k["con"]["lo"], k["con"]["hi"], np.array(k["trajectory"], float))
        assert list(r["l"]) == k["l"] and list(r["u"]) == k["u"], k["test"]
        assert G.row_layout(D, W, [ball], 0) == ((W - 1) * D + D * (3 * W - 3), 3 * W)
        if k["A"] is not None:
            dense = np.zeros((3 * W, 2 * D * W))
            for i in range(3 * W):
                dense[i, r["w"][i] * D:(r["w"][i] + 1) * D] = r["vals"][i]
            np.testing.assert_array_equal(dense, np.array(k["A"], float), err_msg=k["test"])


def test_ur5e_zero_pose():
    p, _ = G.ur5e_point([0.0] * 6, 6)
    assert np.allclose([float(v) for v in p], [-0.8172, -0.2329, 0.0628], rtol=0, atol=1e-15)


def _central_differences(fk, q, D):
    h = MP.mpf("1e-15")
    cols = []
    for j in range(D):
        qp, qm = [MP.mpf(v) for v in q], [MP.mpf(v) for v in q]
        qp[j] += h
        qm[j] -= h
        cols.append([(a - b) / (2 * h) for a, b in zip(fk(qp), fk(qm))])
    return cols


def test_jacobians_equal_central_differences_of_the_forward_kinematics():
    rng = np.random.default_rng(5)
    worst = MP.mpf(0)
    for _ in range(4):
        q = rng.uniform(-np.pi, np.pi, 6)
        for frame in (6, 5, 2):
            _, J = G.ur5e_point(q, frame)
            cd = _central_differences(lambda x: G.ur5e_point(x, frame)[0], q, 6)
            worst = max(worst, max(abs(J[ax][j] - cd[j][ax]) for ax in range(3) for j in range(6)))
        for param in G.Y_PARAMS:
            _, J = G.yaw_2link(q[:3], param)
            cd = _central_differences(lambda x: G.yaw_2link(x, param)[0], q[:3], 3)
            worst = max(worst, max(abs(J[ax][j] - cd[j][ax]) for ax in range(3) for j in range(3)))
    print(f"\nJacobian against central differences (h = 1e-15, {MP.dps} digits): worst {mpmath.nstr(worst, 3)}")
    assert MP.dps >= 40 and worst <= MP.mpf("1e-20")


def test_fp64_error_and_gpu_tolerance():
    for name in G.SCENES:
        ev, eb = G.fp64_error(name)
        tv, tb = G.gpu_tolerance(name)
        print(f"\nscene {name}: fp64 error of the formulas: values {ev:.3e} (absolute), bounds {eb:.3e} (per term scale);"
              f" GPU tolerance {tv:.3e} / {tb:.3e}")
        if name[0] == "T":
            assert ev == 0.0 and eb == 0.0                # every number a dyadic rational: exact in fp64
        else:
            assert 0.0 < ev <= 1e-13 / 32 and 0.0 < eb <= 1e-13 / 32     # the GPU tolerance ends up well under the 1e-12 of the host twin
            assert tv == 32 * ev and tb == 32 * eb


@pytest.mark.parametrize("name", G.SCENES)
def test_scene_populations(name):
    s, ref, p = G.scene(name), G.scene_reference(name), G.populations(name)
    W, nb, nl = s["W"], len(s["balls"]), len(s["lines"])
    print(f"\nscene {name}: D = {s['D']}, W = {W}, {nb} balls ({nb * W} pairs), {nl} lines; accepted {p['accepted']}, rejected {p['rejected']},"
          f" causes {dict(sorted(p['causes'].items()))}")
    for c in G.CLASSES:
        print(f"  {c:5s}: rows per ball and line {p['cls'][c].tolist()}, of them at w = 0 or W - 1 per ball {p['ends'][c].tolist()}")
    print(f"  decisions within the margin {s['margin']:g}: {p['near']} of {p['decisions']}; comparisons of the verdict within it:"
          f" {p['near_comparisons']}; verdicts excluded: {p['verdicts_excluded']}")
    assert len(s["trajs"]) == 8 and s["trajs"].shape[1] == 2 * s["D"] * W
    assert len({t.tobytes() for t in s["trajs"]}) == 8                       # distinct trajectories
    assert p["accepted"] >= 2 and p["rejected"] >= 2
    assert p["verdicts_excluded"] <= 1
    allowed = {"not_below" if ln["below"] else "not_above" for ln in s["lines"]}
    allowed |= {"box_low"} if any(G._present(s["con_lo"], ax, True) for ax in range(3)) else set()
    allowed |= {"box_high"} if any(G._present(s["con_hi"], ax, False) for ax in range(3)) else set()
    assert set(p["causes"]) == allowed
    if name[0] == "T":
        assert p["near"] == 0 and p["near_comparisons"] == 0 and p["verdicts_excluded"] == 0
        if name != "T2":
            assert nb * W >= 256
        for b, ball in enumerate(s["balls"]):
            for c in G.CLASSES:
                if c == "close" and ball["radius"] == 0:
                    assert p["cls"][c][b].sum() == 0                          # a distance is never below 0
                    continue
                assert p["cls"][c][b].sum() >= 4, (c, b)
                assert p["ends"][c][b] >= 1, (c, b)                           # at w = 0 or w = W - 1
        # each class that can occur there at w = 0 and at w = W - 1, and on both sides of the pass boundary (pairs 255 | 256)
        seen = {(d["ball"] * W + d["w"], d["cls"]) for e in ref for d in e["decisions"]}
        at = lambda w: {c for e in ref for d in e["decisions"] if d["w"] == w for c in [d["cls"]]}
        assert at(0) == {"close", "next", "none"} and at(W - 1) == {"close", "prev", "none"}
        if name == "T86":
            for pair in (255, 256):                                          # ball 2 has radius 0: never close
                assert {c for e, c in seen if e == pair} == {"prev", "next", "none"}
            assert {c for e, c in seen if e == 257} == {"prev", "none"}
        if name == "T64":
            assert nb * W == 256 and {c for e, c in seen if e == 255} == {"close", "prev", "none"}
        # the placements the scene is built around: a neighbour exactly on a line, distances of radius (1 -+ 2^-20)
        assert any(d["prev"] == 0.0 or d["next"] == 0.0 for e in ref for d in e["decisions"] if d["cls"] == "none")
        rel = {round(d["close"] / s["balls"][d["ball"]]["radius"] * 2 ** 20) for e in ref for d in e["decisions"]
               if s["balls"][d["ball"]]["radius"] > 0 and abs(d["close"]) < 1e-5}
        assert {-1, 1} <= rel
        slacks = {m["kind"]: set() for e in ref for m in e["margins"]}
        for e in ref:
            for m in e["margins"]:
                if abs(m["slack"]) < 2e-6:
                    slacks[m["kind"]].add(np.sign(m["slack"]))
        assert all(v == {-1.0, 1.0} for v in slacks.values()), slacks       # every threshold from both sides, 2^-20 away
    else:
        assert nb * W > 256
        assert p["near"] <= 0.01 * p["decisions"]
        for li in range(nl):
            assert p["cls"]["prev"][:, li].sum() >= 1 and p["cls"]["next"][:, li].sum() >= 1 and p["cls"]["close"][:, li].sum() >= 1


def test_scene_problem_layout():
    s = G.scene("Y")
    for over in (False, True):
        pr = G.scene_problem(s["D"], s["W"], s["balls"], len(s["lines"]), 3, over)
        row0, rows3d = G.row_layout(s["D"], s["W"], s["balls"], len(s["lines"]))
        D, W = s["D"], s["W"]
        assert pr["m"] == row0 + (D * W * (3 + len(s["lines"]) * len(s["balls"])) if over else rows3d) and pr["n"] == 2 * D * W
        A = pr["A"].toarray()
        assert np.all(A[row0:row0 + rows3d].sum(axis=1) == D) and np.all(A[row0 + rows3d:] == 0)
        # row r of waypoint w holds its D entries in the columns of q_w, and aidx finds them in the CSC value array
        tagged = pr["A"].copy()
        tagged.data = np.arange(len(tagged.data), dtype=float)
        T = tagged.toarray()
        r = row0
        for ball in s["balls"]:
            for w in range(W):
                for _ in range((3 if ball["gripper"] else 0) + len(s["lines"])):
                    assert np.array_equal(T[r, w * D:(w + 1) * D], pr["aidx"][r - row0])
                    r += 1
        assert np.all(pr["l"][:, row0:] == -1e30) and np.all(pr["u"][:, row0:] == 1e30)


def test_the_solved_qp_of_scene_T_is_solvable():
    """The QP that tests/test_gpu_gomp_scene.py solves after a re-linearisation: the oracle finds an optimum."""
    from oracle import oracle as O
    s, ref = G.scene("T86"), G.scene_reference("T86")
    pr = G.scene_batch("T86")
    b = G.SOLVED_QP
    assert not ref[b]["ok"]
    Ax, l, u = G.reference_rows(pr, b, ref[b])
    A = pr["A"].copy()
    A.data = Ax
    o = O.OracleQPSolver(pr["P"], None, pr["A"], pr["l"][b], pr["u"][b], scaling=0)
    o.update(l, A, u)
    o.set_warm_start(s["trajs"][b])
    st, x = o.solve()
    print(f"\noracle on the re-linearised QP {b} of scene T86: status {st}, {o.info().iter} iterations")
    assert st == 1
