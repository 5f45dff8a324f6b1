"""CPU: capsule and sphere obstacles before anything runs on a GPU - the reference of tests/capsule_refs.py against central
differences and its own known answers (tests/golden/capsule_kats.json), the populations of the scenes of
tests/test_gpu_capsules.py and the fp64 error from which their GPU tolerance is derived.

Measured here (np.float64 evaluation of the formulas against the mpmath one over the eight trajectories of each scene; values
absolute, bounds divided by the sum of the absolute values of their terms):

    scene K7 (7 joints, W = 40, 7 balls = 280 pairs, 1 line, 3 capsules):  values 1.6e-15, bounds 3.1e-15
    scene K8 (8 joints, W = 2, 1 ball, 1 sphere):                          values 6.4e-16, bounds 7.5e-16
    scene KT (TABLE model, identity, dyadic numbers on axes):              values 0, bounds 0 (exact)
    scene KM (gripper ball with box, 2 lines, 2 capsules):                 values 1.1e-15, bounds 6.4e-16

-> GPU tolerance 32 x the figure (2e-14 .. 1e-13; the normal v / |v| loses the digits that p - c cancels), never looser than
1e-13; scene KT is compared bit for bit.  Populations: K7 3 accepted / 5 rejected (causes box_low, box_high, not_above,
capsule; trajectory 5 by a capsule alone), active rows on every capsule and, on the slanted one, with t clamped at 0, inside
and clamped at 1; K8 6 / 2; KT 5 / 3 (of its three re-linearised QPs the oracle finds one optimal after 25 iterations and two
infeasible); KM 2 / 6.  No row within 1e-9 of a threshold, no verdict excluded.  Capsule rows against central differences of
dist(fk(q)) (h = 1e-15, 50 digits): worst below 1e-20.  Run with -s to see the figures."""
import json

import mpmath
import numpy as np
import pytest

import capsule_refs as K
import dh_refs as DH
import gomp_refs as G

MP = G.MP


@pytest.mark.parametrize("name", K.SCENES)
def test_fp64_error_and_gpu_tolerance(name):
    ev, eb = K.fp64_error(name)
    tv, tb = K.gpu_tolerance(name)
    print(f"\nscene {name}: fp64 error of the formulas: values {ev:.3e} (absolute), bounds {eb:.3e} (per term scale); GPU tolerance {tv:.3e} / {tb:.3e}")
    assert tv == min(32 * ev, 1e-13) and tb == min(32 * eb, 1e-13)
    if name == "KT":
        assert ev == 0.0 and eb == 0.0                                        # exact in any order of operations
        for hi, lo in zip(K.scene_reference(name), K.scene_reference(name, G.F64)):
            for k in ("vals", "l", "u"):
                assert np.array_equal(hi[k].view(np.int64), lo[k].view(np.int64))
            assert hi["ok"] == lo["ok"] and hi["cls"] == lo["cls"]
    else:
        assert 0.0 < ev <= 1e-13 / 32 and 0.0 < eb <= 1e-13 / 32


@pytest.mark.parametrize("name", K.SCENES)
def test_scene_populations(name):
    s, p = K.scene(name), K.populations(name)
    W, nb, nl, nc = s["W"], len(s["balls"]), len(s["lines"]), len(s["capsules"])
    print(f"\nscene {name}: D = {s['D']}, W = {W}, {nb} balls ({nb * W} pairs), {nl} lines, {nc} capsules; accepted {p['accepted']}, rejected {p['rejected']},"
          f" causes {dict(sorted(p['causes'].items()))}")
    for c in K.CLASSES:
        print(f"  {c:6s}: rows per capsule {p['cls'][c].tolist()}")
    for c in K.CLAMPS:
        print(f"  {c:6s}: rows per capsule {p['clamp'][c].tolist()}")
    print(f"  rows within 1e-9 of a threshold: {p['near']}; comparisons of the verdict within the margin: {p['near_comparisons']}; verdicts excluded: {p['verdicts_excluded']}")
    assert len(s["trajs"]) == 8 and s["trajs"].shape[1] == 2 * s["D"] * W
    assert len({t.tobytes() for t in s["trajs"]}) == 8
    assert p["capsule_rows"] == 8 * nb * W * nc
    assert p["verdicts_excluded"] == 0 and p["near"] == 0 and p["near_comparisons"] == 0          # the share allowed on the GPU is zero
    assert p["accepted"] >= 2 and p["rejected"] >= 2 and p["causes"].get("capsule", 0) >= 1
    for c in K.CLASSES:
        assert np.all(p["cls"][c] >= 1), c                                    # every capsule has active and inactive rows
    ref = K.scene_reference(name)
    if name == "K7":
        assert (s["D"], W, nb * W, nl, nc) == (7, 40, 280, 1, 3) and nb * W > 256
        assert (p["accepted"], p["rejected"]) == (3, 5)
        assert set(p["causes"]) == {"box_low", "box_high", "not_above", "capsule"}
        assert any(e["causes"] == {"capsule"} for e in ref)                   # rejected by a capsule and nothing else
        assert p["clamp"]["point"].tolist() == [8 * 280, 0, 0]
        assert p["clamp"]["inside"][1] >= 1 and p["clamp"]["high"][1] >= 1   # the post: beside it and above its top
        active = {c: 0 for c in K.CLAMPS}
        for e in ref:
            for k in range(len(e["l"])):
                if e["kind"][k] == 3 + nl + 2 and e["cls"][k] == "active":
                    active[e["clamp"][k]] += 1
        print(f"  slanted capsule, active rows by clamp case: {active}")
        assert active["low"] >= 1 and active["inside"] >= 1 and active["high"] >= 1
        assert any(e["ok"] and any(c == "active" for c in e["cls"]) for e in ref)                 # active and accepted
    elif name == "K8":
        assert (s["D"], W, nb, nl, nc) == (8, 2, 1, 0, 1)
        assert (p["accepted"], p["rejected"]) == (6, 2)
    elif name == "KT":
        assert (s["D"], W, nb, nl, nc) == (3, 6, 2, 0, 2)
        assert [e["ok"] for e in ref] == [False, True, True, False, False, True, True, True]
        assert p["clamp"]["point"][0] == 8 * 12 and p["clamp"]["low"][1] >= 1 and p["clamp"]["high"][1] >= 1
    else:
        assert nl == 2 and nc == 2 and s["balls"][0]["gripper"] and not s["balls"][1]["gripper"]
        assert {"box_low", "box_high", "not_above", "capsule"} <= set(p["causes"])
        # the order of a gripper ball's block: three box rows, two lines, two capsules
        e = ref[0]
        assert [int(k) for k in e["kind"][:7]] == [0, 1, 2, 3, 4, 5, 6] and e["cls"][:3] == ["box"] * 3 and e["clamp"][:5] == [None] * 5
        assert [int(k) for k in e["kind"][7 * W:7 * W + 4]] == [3, 4, 5, 6]


def _row(e, ball, w, kind):
    k = [i for i in range(len(e["l"])) if (e["ball"][i], e["w"][i], e["kind"][i]) == (ball, w, kind)]
    assert len(k) == 1
    return k[0]


def test_the_exact_cases_of_scene_KT():
    s, ref = K.scene("KT"), K.scene_reference("KT")
    c, T = K.KT_C, s["trajs"]
    # 0: the ball centres on the sphere's centre: normal +Z, l = reach + q_z, for both capsules (the second has margin 0, radius 0)
    e = ref[0]
    for ball, r in ((0, K.KT_RB), (1, K.KT_RB1)):
        for kind, R in ((3, K.KT_R0), (4, 0.0)):
            k = _row(e, ball, 2, kind)
            assert e["vals"][k].tolist() == [0.0, 0.0, 1.0] and e["cls"][k] == "active" and e["s"][k] == -(R + r)
            assert e["l"][k] == (R + r) + c[2] and e["u"][k] == G.INF
    assert not e["ok"]
    # 1: s = margin -+ 2^-20 for ball 0 and the sphere
    e = ref[1]
    k, k2 = _row(e, 0, 1, 3), _row(e, 0, 4, 3)
    assert e["s"][k] == K.KT_M0 - K.E20 and e["cls"][k] == "active" and e["vals"][k].tolist() == [1.0, 0.0, 0.0]
    assert e["l"][k] == (K.KT_R0 + K.KT_RB) - (K.KT_R0 + K.KT_RB + K.KT_M0 - K.E20) + T[1][3 * 1]
    assert e["s"][k2] == K.KT_M0 + K.E20 and e["cls"][k2] == "none" and e["l"][k2] == -G.INF and e["vals"][k2].tolist() == [1.0, 0.0, 0.0]
    assert e["ok"]
    # 2, 3: s = -ERROR -+ 2^-20 (on the 2^-30 grid) decides the verdict and nothing else does
    for b, sign in ((2, +1), (3, -1)):
        e = ref[b]
        k = _row(e, 0, 2, 3)
        assert e["s"][k] == G.grid(K.KT_R0 + K.KT_RB - G.ERROR) + sign * K.E20 - (K.KT_R0 + K.KT_RB)
        assert abs(e["s"][k] + G.ERROR - sign * K.E20) < 2.0 ** -30
        assert e["ok"] == (sign > 0)
        bad = [m for m in e["margins"] if m["slack"] < 0]
        assert len(bad) == (0 if sign > 0 else 1)
    # 4: margin 0, radius 0: active at s = -2^-20, not at +2^-20
    e = ref[4]
    k, k2 = _row(e, 0, 1, 4), _row(e, 0, 3, 4)
    assert (e["s"][k], e["cls"][k], e["s"][k2], e["cls"][k2]) == (-K.E20, "active", K.E20, "none")
    # 5: the segment of length 2^-30 beside the sphere at its first end: t clamped at 1 | 0, the distances differ by 2^-30
    e = ref[5]
    k, k2 = _row(e, 1, 0, 4), _row(e, 1, 2, 4)
    assert (e["clamp"][k], e["clamp"][k2]) == ("high", "low")
    assert e["s"][k] == 0.5 - K.E30 - K.KT_RB1 and e["s"][k2] == 0.5 - K.KT_RB1
    assert e["s"][_row(e, 1, 0, 3)] == 0.5 - K.KT_R0 - K.KT_RB1
    assert e["vals"][k].tolist() == [0.0, 0.0, 1.0] and e["vals"][k2].tolist() == [0.0, 0.0, -1.0]
    # 7: ball 0 on the surface: s = 0, active, accepted
    e = ref[7]
    k = _row(e, 0, 5, 3)
    assert e["s"][k] == 0.0 and e["cls"][k] == "active" and e["l"][k] == T[7][3 * 5 + 2] and e["ok"]


def test_capsule_rows_equal_central_differences_of_the_distance():
    s = K.scene("K7")
    D, h = s["D"], MP.mpf("1e-15")
    worst, n = MP.mpf(0), 0
    for b, w in ((0, 22), (2, 13), (5, 3), (6, 30), (7, 8), (7, 31)):
        qf = s["trajs"][b][w * D:(w + 1) * D]
        for ball in s["balls"][1::2]:
            p, J = G.fk_jac(ball, qf, w)
            for cap in s["capsules"]:
                g = K.capsule_row(cap, p, J, [MP.mpf(v) for v in qf], MP.mpf(ball["radius"]))
                _, clamp = K.closest(cap, p)
                for j in range(D):
                    qp, qm = [MP.mpf(v) for v in qf], [MP.mpf(v) for v in qf]
                    qp[j] += h
                    qm[j] -= h
                    pp, pm = G.fk_jac(ball, qp, w)[0], G.fk_jac(ball, qm, w)[0]
                    assert K.closest(cap, pp)[1] == K.closest(cap, pm)[1] == clamp      # not across a kink of the distance
                    fd = (K.distance(cap, pp) - K.distance(cap, pm)) / (2 * h)
                    nrm = [(p[k] - K.closest(cap, p)[0][k]) / K.distance(cap, p) for k in range(3)]
                    exact = nrm[0] * J[0][j] + nrm[1] * J[1][j] + nrm[2] * J[2][j]
                    worst = max(worst, abs(exact - fd))
                    assert abs(float(exact) - g["vals"][j]) <= 1e-300 + 2.0 ** -52 * abs(float(exact))
                    n += 1
    print(f"\ncapsule rows against central differences of dist(fk(q)) (h = 1e-15, {MP.dps} digits), {n} entries: worst {mpmath.nstr(worst, 3)}")
    assert MP.dps >= 40 and n == 6 * 3 * 3 * D and worst <= MP.mpf("1e-20")


def test_known_answers_equal_what_the_reference_computes_now():
    assert K.load_kats() == json.loads(json.dumps(K.kats_now()))


def test_no_capsules_is_gomp_refs_own_result():
    s = DH.scene("M3")
    for t in s["trajs"][:2]:
        a = G.with_obstacles(s["D"], s["W"], s["balls"], s["lines"], s["con_lo"], s["con_hi"], t, s["margin"])
        b = K.with_obstacles(s["D"], s["W"], s["balls"], s["lines"], [], s["con_lo"], s["con_hi"], t, s["margin"])
        for k in ("vals", "l", "u", "l_scale", "u_scale"):
            assert np.array_equal(a[k], b[k])
        assert a["cls"] == b["cls"] and a["ok"] == b["ok"] and a["causes"] == b["causes"] and a["verdict_excluded"] == b["verdict_excluded"]


def test_the_rejected_qps_of_scene_KT_on_the_oracle():
    """The QPs that tests/test_gpu_capsules.py solves after mi_gomp_relinearise_some: one has an optimum, two are infeasible
    (their pinned waypoints sit inside the sphere)."""
    from oracle import oracle as O
    s, ref, pr = K.scene("KT"), K.scene_reference("KT"), K.scene_batch("KT")
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
        print(f"\noracle on the re-linearised QP {b} of scene KT: status {st}, {o.info().iter} iterations")
    assert got == {0: -3, 3: 1, 4: -3}
