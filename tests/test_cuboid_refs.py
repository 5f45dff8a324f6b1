"""CPU: cuboid obstacles before anything runs on a GPU - the reference of tests/cuboid_refs.py against its own known answers
(tests/golden/cuboid_kats.json) and against capsule_refs (a cuboid with two zero half extents is a capsule), the populations of
the scenes of tests/test_gpu_cuboids.py and the fp64 error from which their GPU tolerance is derived.

Measured here (np.float64 evaluation of the formulas against the mpmath one over the eight trajectories of each scene; values
absolute, bounds divided by the sum of the absolute values of their terms):

    scene X7 (7 joints, W = 40, 7 balls = 280 pairs, 1 line, 1 capsule, 3 cuboids):  values 3.1e-15, bounds 6.6e-15
    scene X8 (8 joints, W = 2, 1 ball, 1 cuboid):                                    values 1.2e-15, bounds 5.4e-16
    scene XT (TABLE model, identity, dyadic numbers; a cube and a permuted slab):    values 0, bounds 0 (exact)
    scene XM (gripper ball with work-space limits, 2 lines, 1 capsule, 2 cuboids):   values 8.9e-16, bounds 4.9e-16
    scene XP (as XT, one point cuboid with permuted axes):                           values 0, bounds 0 (exact)

-> GPU tolerance 32 x the figure, never looser than 1e-13; scenes XT and XP are compared bit for bit.  Populations: X7 3
accepted / 5 rejected (trajectory 5 by a cuboid alone; the accepted ones have active cuboid rows), X8 5 / 3, XT 3 / 5, XM 0 / 8,
XP 6 / 2.  Over X7 and XM every region (face, edge, corner, inside) occurs active, and face, edge and corner inactive.  An
inactive inside row cannot be committed: inside, s = sd - reach <= 0 and the row is inactive only when s >= margin >= 0, that
is at s = margin = 0 exactly - a row ON its threshold, which the rule for the committed trajectories (no row within 1e-9 of a
threshold) excludes; the test asserts that none occurs.  No row within 1e-9 of a threshold, no verdict excluded.

Scene XT holds two cuboids, as asked: with one centre for both, the cube carries the three-way tie, the six faces, the two-way
ties and the points on faces, the permuted slab the transposition check, c_k* = -0.0 and margin 0.  A point cuboid forces every
waypoint of an exact scene onto the lines through its centre (anywhere else `out` is a square root of two or three squares),
which the two-way tie cannot be on - so the point cuboid has the small exact scene XP to itself.  Run with -s to see the figures."""
import json

import mpmath
import numpy as np
import pytest

import capsule_refs as K
import cuboid_refs as X
import gomp_refs as G

MP = G.MP


@pytest.mark.parametrize("name", X.SCENES)
def test_fp64_error_and_gpu_tolerance(name):
    ev, eb = X.fp64_error(name)
    tv, tb = X.gpu_tolerance(name)
    print(f"\nscene {name}: fp64 error of the formulas: values {ev:.3e} (absolute), bounds {eb:.3e} (per term scale); GPU tolerance {tv:.3e} / {tb:.3e}")
    assert tv == min(32 * ev, 1e-13) and tb == min(32 * eb, 1e-13)
    if name in X.EXACT:
        assert ev == 0.0 and eb == 0.0 and (tv, tb) == (0.0, 0.0)              # exact in any order of operations
        for hi, lo in zip(X.scene_reference(name), X.scene_reference(name, G.F64)):
            for k in ("vals", "l", "u"):
                assert np.array_equal(hi[k].view(np.int64), lo[k].view(np.int64))
            assert hi["ok"] == lo["ok"] and hi["cls"] == lo["cls"] and hi["region"] == lo["region"]
    else:
        assert 0.0 < ev <= 1e-14 and 0.0 < eb <= 1e-14                         # (X7: 32 x the figure passes 1e-13, so 1e-13 it is)


@pytest.mark.parametrize("name", X.SCENES)
def test_scene_populations(name):
    s, p = X.scene(name), X.populations(name)
    W, nb, nl, nc, nx = s["W"], len(s["balls"]), len(s["lines"]), len(s["capsules"]), len(s["cuboids"])
    print(f"\nscene {name}: D = {s['D']}, W = {W}, {nb} balls ({nb * W} pairs), {nl} lines, {nc} capsules, {nx} cuboids; accepted {p['accepted']},"
          f" rejected {p['rejected']}, causes {dict(sorted(p['causes'].items()))}")
    for g in X.REGIONS:
        print(f"  {g:6s}: rows per cuboid active {p['cells'][(g, 'active')].tolist()}, none {p['cells'][(g, 'none')].tolist()}")
    print(f"  rows within 1e-9 of a threshold: {p['near']}; comparisons of the verdict within the margin: {p['near_comparisons']}; verdicts excluded: {p['verdicts_excluded']}")
    assert len(s["trajs"]) == 8 and s["trajs"].shape[1] == 2 * s["D"] * W
    assert len({t.tobytes() for t in s["trajs"]}) == 8
    assert p["cuboid_rows"] == 8 * nb * W * nx
    assert p["verdicts_excluded"] == 0 and p["near"] == 0 and p["near_comparisons"] == 0          # the share allowed on the GPU is zero
    assert p["causes"].get("cuboid", 0) >= 1
    assert np.all(sum(p["cells"][(g, "active")] for g in X.REGIONS) >= 1)                         # every cuboid has active rows
    assert np.all(p["cells"][("inside", "none")] == 0)                                             # (module docstring)
    ref = X.scene_reference(name)
    if name == "X7":
        assert (s["D"], W, nb * W, nl, nc, nx) == (7, 40, 280, 1, 1, 3) and nb * W > 256
        assert (p["accepted"], p["rejected"]) == (3, 5)
        assert any(e["causes"] == {"cuboid"} for e in ref)                    # rejected by a cuboid and nothing else
        assert any(e["ok"] and any(c == "active" and g is not None for c, g in zip(e["cls"], e["region"])) for e in ref)      # active and accepted
        a0, a1, a2 = (np.array(c["axes"]).reshape(3, 3) for c in s["cuboids"])
        assert np.all(np.abs(a0) > 0.01)                                      # not axis-aligned in any coordinate
        assert s["cuboids"][1]["half"][2] == 0.0 and s["cuboids"][2]["radius"] > 0.0
    elif name == "X8":
        assert (s["D"], W, nb, nl, nc, nx) == (8, 2, 1, 0, 0, 1)
        assert p["accepted"] >= 1 and p["rejected"] >= 1
    elif name == "XT":
        assert (s["D"], W, nb, nl, nc, nx) == (3, 8, 2, 0, 0, 2)
        assert [e["ok"] for e in ref] == [False, False, False, True, True, False, False, True]
        assert s["cuboids"][0]["axes"] == X.AXIS_ALIGNED
        ax = np.array(s["cuboids"][1]["axes"]).reshape(3, 3)
        assert set(np.abs(ax).reshape(-1)) == {0.0, 1.0} and np.array_equal(ax @ ax.T, np.eye(3)) and not np.array_equal(ax, ax.T)
    elif name == "XP":
        assert (s["D"], W, nb, nl, nc, nx) == (3, 4, 1, 0, 0, 1) and s["cuboids"][0]["half"] == [0.0, 0.0, 0.0] and s["cuboids"][0]["radius"] > 0
        assert [e["ok"] for e in ref] == [False, True, True, False, True, True, True, True]
    else:
        assert nl == 2 and nc == 1 and nx == 2 and s["balls"][0]["gripper"] and not s["balls"][1]["gripper"]
        assert {"box_low", "box_high", "not_above", "capsule", "cuboid"} <= set(p["causes"])
        # the order of a gripper ball's block: three work-space rows, two lines, one capsule, two cuboids
        e = ref[0]
        assert [int(k) for k in e["kind"][:8]] == [0, 1, 2, 3, 4, 5, 6, 7] and e["cls"][:3] == ["box"] * 3
        assert e["region"][:6] == [None] * 6 and None not in e["region"][6:8] and e["clamp"][5] is not None and e["clamp"][6:8] == [None, None]
        assert [int(k) for k in e["kind"][8 * W:8 * W + 5]] == [3, 4, 5, 6, 7]


def test_every_region_and_class_occurs_over_X7_and_XM():
    cells = {k: 0 for k in X.populations("X7")["cells"]}
    for name in ("X7", "XM"):
        for k, v in X.populations(name)["cells"].items():
            cells[k] += int(v.sum())
    print("\nX7 + XM, cuboid rows by (region, class):", cells)
    for g in X.REGIONS:
        assert cells[(g, "active")] >= 1, g
        if g != "inside":                                                     # inside and inactive: only ON the threshold (module docstring)
            assert cells[(g, "none")] >= 1, g
    refs = X.scene_reference("X7") + X.scene_reference("XM")
    assert any(e["causes"] == {"cuboid"} for e in refs) and any(e["ok"] for e in refs)


def _row(e, ball, w, kind):
    k = [i for i in range(len(e["l"])) if (e["ball"][i], e["w"][i], e["kind"][i]) == (ball, w, kind)]
    assert len(k) == 1
    return k[0]


def test_the_exact_cases_of_scene_XT():
    s, ref = X.scene("XT"), X.scene_reference("XT")
    o, T = X.XT_O, s["trajs"]
    rA, r0, r1, h = X.XT_RA, X.XT_RB, X.XT_RB1, X.XT_H
    # 0: strictly inside the cube, nearest to +x, -x, +y, -y, +z, -z in turn: normal +-e_k, sd = -slack = -1/16
    e = ref[0]
    for w in range(6):
        n = [0.0, 0.0, 0.0]
        n[w // 2] = 1.0 - 2 * (w % 2)
        for ball, r in ((0, r0), (1, r1)):
            k = _row(e, ball, w, 3)
            assert e["vals"][k].tolist() == n and e["region"][k] == "inside" and e["cls"][k] == "active"
            assert e["s"][k] == -1 / 16 - (rA + r) and e["l"][k] == (rA + r) + 1 / 16 + n[w // 2] * T[0][3 * w + w // 2]
    # 1: the centre of the cube: three-way tie, k* = 0, sign +; in the slab c_2 = 0: +u_2 = -x
    e = ref[1]
    k, kb = _row(e, 0, 1, 3), _row(e, 0, 1, 4)
    assert e["vals"][k].tolist() == [1.0, 0.0, 0.0] and e["s"][k] == -h - (rA + r0) and e["l"][k] == (rA + r0) + h + o[0]
    assert e["vals"][kb].tolist() == [-1.0, 0.0, 0.0] and e["s"][kb] == -1 / 64 - r0 and e["l"][kb] == r0 + 1 / 64 - o[0]
    #    two-way ties between y and z: the lower axis wins, signed by c_1; in the slab y_2 = -0.0 (every term of it) at waypoint 3
    k, kb = _row(e, 0, 3, 3), _row(e, 0, 3, 4)
    assert e["vals"][k].tolist() == [0.0, -1.0, 0.0] and e["s"][k] == -1 / 8 - (rA + r0)
    assert e["vals"][kb].tolist() == [-1.0, 0.0, 0.0] and e["s"][kb] == -1 / 64 - r0
    k = _row(e, 1, 5, 3)
    assert e["vals"][k].tolist() == [0.0, 1.0, 0.0] and e["s"][k] == -1 / 8 - (rA + r1)
    # 2: on a face: out = 0, sd = 0, the face's outward normal
    e = ref[2]
    for w, kind, n, reach in ((2, 3, [1.0, 0.0, 0.0], rA + r0), (4, 3, [0.0, 0.0, -1.0], rA + r0), (6, 4, [1.0, 0.0, 0.0], r0)):
        k = _row(e, 0, w, kind)
        assert e["vals"][k].tolist() == n and e["region"][k] == "inside" and e["out"][k] == 0.0 and e["s"][k] == -reach and e["cls"][k] == "active"
    # 3: s = margin -+ 2^-20 for ball 0 and the cube
    e = ref[3]
    k, k2 = _row(e, 0, 1, 3), _row(e, 0, 4, 3)
    assert e["s"][k] == X.XT_MA - X.E20 and e["cls"][k] == "active" and e["vals"][k].tolist() == [1.0, 0.0, 0.0]
    assert e["l"][k] == (rA + r0) - (rA + r0 + X.XT_MA - X.E20) + T[3][3 * 1]
    assert e["s"][k2] == X.XT_MA + X.E20 and e["cls"][k2] == "none" and e["l"][k2] == -G.INF and e["vals"][k2].tolist() == [-1.0, 0.0, 0.0]
    assert e["ok"]
    # 4, 5: s = -ERROR -+ 2^-20 (on the 2^-30 grid) decides the verdict and nothing else does
    for b, sign in ((4, +1), (5, -1)):
        e = ref[b]
        k = _row(e, 0, 2, 3)
        assert e["s"][k] == X.XT_ACCEPT + sign * X.E20 - (rA + r0)
        assert abs(e["s"][k] + G.ERROR - sign * X.E20) < 2.0 ** -30
        assert e["ok"] == (sign > 0)
        assert len([m for m in e["margins"] if m["slack"] < 0]) == (0 if sign > 0 else 1)
    # 6: margin 0, sharp: active at s = -2^-20, not at +2^-20
    e = ref[6]
    k, k2 = _row(e, 0, 1, 4), _row(e, 0, 3, 4)
    assert (e["s"][k], e["cls"][k], e["s"][k2], e["cls"][k2]) == (-X.E20, "active", X.E20, "none")
    assert e["vals"][k].tolist() == [1.0, 0.0, 0.0] and e["vals"][k2].tolist() == [-1.0, 0.0, 0.0]
    # 7: the slab's faces along u_0 = +y and u_1 = +z, from outside: a transposed `axes` has -z and +x there
    e = ref[7]
    assert e["vals"][_row(e, 0, 5, 4)].tolist() == [0.0, 1.0, 0.0] and e["vals"][_row(e, 0, 6, 4)].tolist() == [0.0, 0.0, -1.0]
    assert e["s"][_row(e, 0, 5, 4)] == 0.5 - r0 and e["ok"]
    k = _row(e, 0, 0, 3)
    assert e["cls"][k] == "active" and e["s"][k] == 1 / 4 - (rA + r0) and e["vals"][k].tolist() == [-1.0, 0.0, 0.0]


def test_the_exact_cases_of_scene_XP():
    s, ref = X.scene("XP"), X.scene_reference("XP")
    reach = X.XP_R + X.XP_RB
    e = ref[0]                                                                # on the point: out = 0, +u_0 = +y, sd = 0
    k = _row(e, 0, 1, 3)
    assert e["vals"][k].tolist() == [0.0, 1.0, 0.0] and e["out"][k] == 0.0 and e["s"][k] == -reach and e["l"][k] == reach + X.XT_O[1]
    e = ref[1]
    k, k2 = _row(e, 0, 1, 3), _row(e, 0, 2, 3)
    assert (e["s"][k], e["cls"][k], e["s"][k2], e["cls"][k2]) == (X.XP_M - X.E20, "active", X.XP_M + X.E20, "none")
    assert ref[2]["ok"] and not ref[3]["ok"] and ref[3]["causes"] == {"cuboid"}
    assert ref[5]["vals"][_row(ref[5], 0, 2, 3)].tolist() == [0.0, -1.0, 0.0]
    assert ref[6]["vals"][_row(ref[6], 0, 1, 3)].tolist() == [0.0, 0.0, 1.0] and ref[6]["vals"][_row(ref[6], 0, 2, 3)].tolist() == [0.0, 0.0, -1.0]


def test_minus_zero_takes_the_plus_side():
    """c_k* = -0.0 in fp64: the slab of XT at p = o + (0, -1/8, -1/8) has y_2 = (-1)(+0) + 0 (-1/8) + 0 (-1/8) = -0.0."""
    cub = X.scene("XT")["cuboids"][1]
    p = [np.float64(X.XT_O[0]), np.float64(X.XT_O[1] - 1 / 8), np.float64(X.XT_O[2] - 1 / 8)]
    sd, n, region, out, gap, c_star = X.probe(cub, p, G.F64)
    assert c_star == 0.0 and np.signbit(c_star) and region == "inside" and [float(v) for v in n] == [-1.0, 0.0, 0.0] and sd == -1 / 64


def test_a_cuboid_with_two_zero_half_extents_is_the_capsule():
    """Scene K7 of capsule_refs with each capsule that is not a sphere replaced by the cuboid half = (|b - a| / 2, 0, 0), u_0
    along b - a, centre (a + b) / 2: the rows equal capsule_refs' wherever out > NEAR.  The vertical post's axes are exact and its
    rows agree to mpmath accuracy; the slanted capsule's axes are rounded to double, each component off by at most 2^-53, which
    moves the closest point by at most 3 x 2^-53 |p - o| per coordinate and the unit normal by that over `out`: the bound per
    row is 64 x 2^-53 (1 + |p - o| / out) times the largest Jacobian entry (values) and times the term scale (bounds)."""
    s = K.scene("K7")
    D, W = s["D"], s["W"]
    worst = {1: 0.0, 2: 0.0}
    n = 0
    for ci in (1, 2):
        cap = s["capsules"][ci]
        cub = X.capsule_as_cuboid(cap)
        ax = np.array(cub["axes"]).reshape(3, 3)
        assert np.max(np.abs(ax @ ax.T - np.eye(3))) <= 1e-15 and cub["half"][1:] == [0.0, 0.0]
        for b in (0, 2, 5, 7):
            t = s["trajs"][b]
            for ball in s["balls"][::3]:
                for w in range(0, W, 3):
                    qf = t[w * D:(w + 1) * D]
                    p, J = G.fk_jac(ball, qf, w)
                    q, r = [MP.mpf(v) for v in qf], MP.mpf(ball["radius"])
                    a, c = K.capsule_row(cap, p, J, q, r), X.cuboid_row(cub, p, J, q, r)
                    if not c["out"] > X.NEAR:
                        continue
                    jmax = max(abs(float(J[i][j])) for i in range(3) for j in range(D))
                    amp = 64 * 2.0 ** -53 * (1 + c["dn"] / c["out"])
                    tol_v, tol_b = (1e-40, 1e-40) if ci == 1 else (amp * jmax, amp * max(a["l_scale"], 1.0))
                    ev = float(np.max(np.abs(np.array(a["vals"]) - np.array(c["vals"]))))
                    assert a["cls"] == c["cls"] and ev <= tol_v + 2.0 ** -52 * jmax, (ci, b, w, ev, tol_v)          # (both rounded to double at the end)
                    if a["cls"] == "active":
                        assert abs(a["l"] - c["l"]) <= tol_b + 2.0 ** -52 * a["l_scale"], (ci, b, w)
                    else:
                        assert a["l"] == c["l"] == -G.INF
                    assert abs(a["s"] - c["s"]) <= amp + 2.0 ** -52
                    worst[ci] = max(worst[ci], ev)
                    n += 1
    print(f"\ncuboid (|b - a| / 2, 0, 0) against the capsule on K7, {n} rows: worst value difference, post {worst[1]:.3e}, slanted {worst[2]:.3e}")
    assert n >= 200


def test_known_answers_equal_what_the_reference_computes_now():
    assert X.load_kats() == json.loads(json.dumps(X.kats_now()))


def test_no_cuboids_is_capsule_refs_own_result():
    s = K.scene("KM")
    for t in s["trajs"][:2]:
        a = K.with_obstacles(s["D"], s["W"], s["balls"], s["lines"], s["capsules"], s["con_lo"], s["con_hi"], t, s["margin"])
        b = X.with_obstacles(s["D"], s["W"], s["balls"], s["lines"], s["capsules"], [], s["con_lo"], s["con_hi"], t, s["margin"])
        for k in ("vals", "l", "u", "l_scale", "u_scale"):
            assert np.array_equal(a[k], b[k])
        assert a["cls"] == b["cls"] and a["ok"] == b["ok"] and a["causes"] == b["causes"] and a["verdict_excluded"] == b["verdict_excluded"]


def test_the_rejected_qps_of_scene_XT_on_the_oracle():
    """The QPs that tests/test_gpu_cuboids.py solves after mi_gomp_relinearise_some, on the reference's rows."""
    from oracle import oracle as O
    s, ref, pr = X.scene("XT"), X.scene_reference("XT"), X.scene_batch("XT")
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
        print(f"\noracle on the re-linearised QP {b} of scene XT: status {st}, {o.info().iter} iterations")
    assert sorted(got) == [0, 1, 2, 5, 6] and got[5] == 1                     # QP 5, 2^-20 too deep, has a solution
