"""CPU: self-collision pairs before anything runs on a GPU - the reference of tests/pair_refs.py against its own known answers
(tests/golden/pair_kats.json), the populations of the scenes of tests/test_gpu_pairs.py and the fp64 error from which their
GPU tolerance is derived.

Measured here (np.float64 evaluation of the formulas against the mpmath one over the eight trajectories of each scene; values
absolute, bounds divided by the sum of the absolute values of their terms):

    scene P7 (7 joints, W = 40, 7 balls = 280 ball items, 14 pairs = 560 pair items, 1 line, 1 capsule):  values 3.9e-16, bounds 1.0e-15
    scene P8 (8 joints, W = 2, 2 balls, 1 pair):                                                          values 2.8e-16, bounds 1.4e-16
    scene PT (TABLE balls and fixed balls on the z axis, dyadic numbers):                                 values 0, bounds 0 (exact)
    scene PM (gripper ball with work-space limits, 2 lines, 1 capsule, 1 cuboid, 3 balls, 2 pairs):       values 8.9e-16, bounds 5.5e-16

-> GPU tolerance 32 x the figure, never looser than 1e-13; scene PT is compared bit for bit.  Populations of P7: 4 accepted / 4
rejected, trajectories 0 and 3 by a pair alone; seven distinct pairs have active rows, the accepted trajectories too; no row
within 1e-9 of a threshold, no verdict excluded.  The fixed balls of PT are yaw + 2-link balls whose two link lengths are zero:
their centre is (0, 0, base height) and their Jacobian zero at every q, exactly, so the TABLE balls can move along the z axis
from waypoint to waypoint and every separation stays along that axis.  Run with -s to see the figures."""
import json

import numpy as np
import pytest

import cuboid_refs as X
import gomp_refs as G
import pair_refs as P


@pytest.mark.parametrize("name", P.SCENES)
def test_fp64_error_and_gpu_tolerance(name):
    ev, eb = P.fp64_error(name)
    tv, tb = P.gpu_tolerance(name)
    print(f"\nscene {name}: fp64 error of the formulas: values {ev:.3e} (absolute), bounds {eb:.3e} (per term scale); GPU tolerance {tv:.3e} / {tb:.3e}")
    assert tv == min(32 * ev, 1e-13) and tb == min(32 * eb, 1e-13)
    if name in P.EXACT:
        assert ev == 0.0 and eb == 0.0 and (tv, tb) == (0.0, 0.0)              # exact in any order of operations
        for hi, lo in zip(P.scene_reference(name), P.scene_reference(name, G.F64)):
            for k in ("vals", "l", "u"):
                assert np.array_equal(hi[k], lo[k])
            assert hi["ok"] == lo["ok"] and hi["cls"] == lo["cls"]
    else:
        assert 0.0 < ev <= 1e-14 and 0.0 < eb <= 1e-14


@pytest.mark.parametrize("name", P.SCENES)
def test_scene_populations(name):
    s, p = P.scene(name), P.populations(name)
    W, nb, nl, nc, nx, npair = s["W"], len(s["balls"]), len(s["lines"]), len(s["capsules"]), len(s["cuboids"]), len(s["pairs"])
    print(f"\nscene {name}: D = {s['D']}, W = {W}, {nb} balls ({nb * W} ball items), {npair} pairs ({npair * W} pair items), {nl} lines, {nc} capsules,"
          f" {nx} cuboids; accepted {p['accepted']}, rejected {p['rejected']} ({p['rejected_by_a_pair_alone']} by a pair alone),"
          f" causes {dict(sorted(p['causes'].items()))}")
    print(f"  pair rows per pair: active {p['cells']['active'].tolist()}, none {p['cells']['none'].tolist()}, rejecting {p['rejecting'].tolist()}")
    print(f"  rows within 1e-9 of a threshold: {p['near']}; comparisons of the verdict within the margin: {p['near_comparisons']}; verdicts excluded: {p['verdicts_excluded']}")
    assert len(s["trajs"]) == 8 and s["trajs"].shape[1] == 2 * s["D"] * W
    assert len({t.tobytes() for t in s["trajs"]}) == 8
    assert p["pair_rows"] == 8 * npair * W
    assert p["verdicts_excluded"] == 0 and p["near"] == 0 and p["near_comparisons"] == 0          # no case is left out on the GPU
    ref = P.scene_reference(name)
    for e in ref:                                                             # pair-major, behind the block of the last ball
        assert np.array_equal(e["pair"][e["block_rows"]:], np.repeat(np.arange(npair), W)) and np.all(e["pair"][:e["block_rows"]] == -1)
        assert np.array_equal(e["w"][e["block_rows"]:], np.tile(np.arange(W), npair))
    if name == "P7":
        assert (s["D"], W, nb * W, npair * W, nl, nc, nx) == (7, 40, 280, 560, 1, 1, 0)
        assert nb * W > 256 and npair * W > 2 * 256 and (npair * W) % 256 != 0    # both sides of the stride, a last partial round
        assert [(q["a"], q["b"]) for q in s["pairs"]] == [(0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (1, 3), (1, 4), (1, 5), (1, 6), (2, 4), (2, 5), (2, 6),
                                                          (3, 5), (3, 6)]
        assert p["cells"]["active"].sum() >= 1 and p["cells"]["none"].sum() >= 1 and p["rejecting"].sum() >= 1
        assert int(np.sum(p["cells"]["active"] > 0)) >= 4                     # at least four distinct pairs have active rows
        assert p["accepted"] >= 2 and p["rejected"] >= 2
        assert p["rejected_by_a_pair_alone"] >= 1
        assert any(e["ok"] and any(c == "active" and k >= 0 for c, k in zip(e["cls"], e["pair"])) for e in ref)      # active and accepted
    elif name == "P8":
        assert (s["D"], W, nb, npair, nl, nc, nx) == (8, 2, 2, 1, 0, 0, 0)
        assert p["cells"]["active"].sum() >= 1 and p["cells"]["none"].sum() >= 1
    elif name == "PT":
        assert (s["D"], W, nb, npair) == (3, 6, 6, 5) and nl == nc == nx == 0
        assert [e["ok"] for e in ref] == [True, True, True, False, True, False, True, True]
        assert ref[3]["causes"] == {"pair"} and ref[5]["causes"] == {"pair"}
    else:
        assert nl == 2 and nc == 1 and nx == 1 and npair == 2 and s["balls"][0]["gripper"] and not s["balls"][1]["gripper"]
        assert np.all(p["cells"]["active"] >= 1) and np.all(p["cells"]["none"] >= 1)
        e = ref[0]                                                            # the order: a gripper ball's block, ..., then the pairs
        assert [int(k) for k in e["kind"][:7]] == [0, 1, 2, 3, 4, 5, 6] and e["cls"][:3] == ["box"] * 3
        assert e["block_rows"] == W * (7 + 4 + 4) and len(e["l"]) == e["block_rows"] + 2 * W


def _row(e, pair, w):
    k = [i for i in range(len(e["l"])) if (e["pair"][i], e["w"][i]) == (pair, w)]
    assert len(k) == 1
    return k[0]


def test_the_exact_cases_of_scene_PT():
    s, ref = P.scene("PT"), P.scene_reference("PT")
    T = s["trajs"]
    tz = [G.T_TABLES[k][6:9] for k in range(3)]                               # the z rows of the TABLE balls' Jacobians
    r03, r05, ma = P.PT_REACH0, P.PT_REACH2, P.PT_MA
    z = lambda b, w: T[b][3 * w + 2]
    # 0: s = margin -+ 2^-20 for pairs 0 and 1 (margin 1/8): active above the fixed ball, inactive below it.  (a, b) and (b, a)
    #    apart from each other: n changes sign and so does J_a - J_b, so the row and the bound are the same, bit for bit (the
    #    derivative of a distance does not know which end is called a)
    e = ref[0]
    k0, k1 = _row(e, 0, 1), _row(e, 1, 1)
    assert e["s"][k0] == ma - P.E20 == e["s"][k1] and e["cls"][k0] == e["cls"][k1] == "active"
    assert e["vals"][k0].tolist() == tz[0] == e["vals"][k1].tolist()
    assert e["l"][k0] == e["l"][k1] == (r03 - (r03 + ma - P.E20)) + tz[0][2] * z(0, 1)
    k0, k1 = _row(e, 0, 3), _row(e, 1, 3)
    assert e["s"][k0] == ma + P.E20 == e["s"][k1] and e["cls"][k0] == e["cls"][k1] == "none" and e["l"][k0] == e["l"][k1] == -G.INF
    assert e["vals"][k0].tolist() == [-v for v in tz[0]] == e["vals"][k1].tolist()                # below: n = -z; written though inactive
    assert e["ok"]
    # 1: margin 0: active at s = -2^-20, not at +2^-20
    e = ref[1]
    k, k2 = _row(e, 2, 2), _row(e, 2, 4)
    assert (e["s"][k], e["cls"][k], e["s"][k2], e["cls"][k2]) == (-P.E20, "active", P.E20, "none")
    assert e["l"][k] == (r05 - (r05 - P.E20)) + tz[0][2] * z(1, 2) and e["ok"]
    # 2, 3: s = -ERROR -+ 2^-20 (on the 2^-30 grid) decides the verdict and nothing else does
    for b, sign in ((2, +1), (3, -1)):
        e = ref[b]
        k = _row(e, 0, 2)
        assert e["s"][k] == P.PT_ACCEPT + sign * P.E20 - r03
        assert abs(e["s"][k] + G.ERROR - sign * P.E20) < 2.0 ** -30
        assert e["ok"] == (sign > 0)
        assert len([m for m in e["margins"] if m["slack"] < 0]) == (0 if sign > 0 else 2)         # pairs 0 and 1 are one pair of balls
    # 3 (pair index): two TABLE balls: always coincident, reach 0: accepted, n = +z, g = the difference of the z rows
    for b, e in enumerate(ref):
        for w in range(s["W"]):
            k = _row(e, 3, w)
            assert e["dist"][k] == 0.0 and e["s"][k] == 0.0 and e["cls"][k] == "active"
            assert e["vals"][k].tolist() == [u - v for u, v in zip(tz[1], tz[2])]
            assert e["l"][k] == (tz[1][2] - tz[2][2]) * z(b, w)
    # 4: coincident with a fixed ball, reach 0: accepted, n = +z; 1/4 below it: inactive, n = -z
    e = ref[4]
    k, k2 = _row(e, 4, 1), _row(e, 4, 4)
    assert e["dist"][k] == 0.0 and e["s"][k] == 0.0 and e["cls"][k] == "active" and e["vals"][k].tolist() == tz[1] and e["ok"]
    assert e["l"][k] == tz[1][2] * z(4, 1)
    assert e["s"][k2] == 1 / 4 and e["cls"][k2] == "none" and e["vals"][k2].tolist() == [-v for v in tz[1]]
    # 5: coincident with reach 3/16: rejected, n = +z whichever ball is called a: here (a, b) and (b, a) do differ in sign
    e = ref[5]
    k, k1 = _row(e, 0, 3), _row(e, 1, 3)
    assert e["dist"][k] == 0.0 and e["s"][k] == -r03 and not e["ok"] and e["vals"][k].tolist() == tz[0] and e["l"][k] == r03 + tz[0][2] * z(5, 3)
    assert e["dist"][k1] == 0.0 and e["vals"][k1].tolist() == [-v for v in tz[0]] and e["l"][k1] == r03 - tz[0][2] * z(5, 3)
    # 6: active from below and from above
    e = ref[6]
    k, k2 = _row(e, 0, 1), _row(e, 0, 2)
    assert e["vals"][k].tolist() == [-v for v in tz[0]] and e["vals"][k2].tolist() == tz[0] and e["cls"][k] == e["cls"][k2] == "active"
    assert e["l"][k] == (r03 - 1 / 4) - tz[0][2] * z(6, 1) and e["l"][k2] == (r03 - 1 / 4) + tz[0][2] * z(6, 2)


def test_known_answers_equal_what_the_reference_computes_now():
    assert P.load_kats() == json.loads(json.dumps(P.kats_now()))


def test_no_pairs_is_cuboid_refs_own_result():
    s = X.scene("XM")
    for t in s["trajs"][:2]:
        a = X.with_obstacles(s["D"], s["W"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["con_lo"], s["con_hi"], t, s["margin"])
        b = P.with_obstacles(s["D"], s["W"], s["balls"], s["lines"], s["capsules"], s["cuboids"], [], s["con_lo"], s["con_hi"], t, s["margin"])
        for k in ("vals", "l", "u", "l_scale", "u_scale"):
            assert np.array_equal(a[k], b[k])
        assert a["cls"] == b["cls"] and a["ok"] == b["ok"] and a["causes"] == b["causes"] and a["verdict_excluded"] == b["verdict_excluded"]


def test_scene_problem_without_pairs_is_gomp_refs_own():
    s = X.scene("XM")
    n_per = len(s["lines"]) + len(s["capsules"]) + len(s["cuboids"])
    for over in (False, True):
        a = G.scene_problem(3, s["W"], s["balls"], n_per, 8, over, starts=s["trajs"][:, :3])
        b = P.scene_problem(3, s["W"], s["balls"], n_per, 0, 8, over, starts=s["trajs"][:, :3])
        assert a["m"] == b["m"] and np.array_equal(a["aidx"], b["aidx"]) and np.array_equal(a["Ax"], b["Ax"]) and np.array_equal(a["l"], b["l"])
        assert np.array_equal(a["A"].indices, b["A"].indices) and np.array_equal(a["A"].indptr, b["A"].indptr)
    pm = P.scene_batch("PM", True)
    assert pm["m"] > pm["row0"] + pm["rows3d"] and pm["rows3d"] == pm["block_rows"] + 2 * P.scene("PM")["W"]


def test_the_rejected_qps_of_scene_PT_on_the_oracle():
    """The QPs that tests/test_gpu_pairs.py solves after mi_gomp_relinearise_some, on the reference's rows."""
    from oracle import oracle as O
    s, ref, pr = P.scene("PT"), P.scene_reference("PT"), P.scene_batch("PT")
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
        print(f"\noracle on the re-linearised QP {b} of scene PT: status {st}, {o.info().iter} iterations")
    assert sorted(got) == [3, 5]
