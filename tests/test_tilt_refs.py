"""CPU: tilt limits before anything runs on a GPU - the reference of tests/tilt_refs.py against mpmath's own derivative of
c(q) and its own known answers (tests/golden/tilt_kats.json), the populations of the scenes of tests/test_gpu_tilts.py and the
fp64 error from which their GPU tolerance is derived.

Measured here (np.float64 evaluation of the formulas against the mpmath one over the eight trajectories of each scene; values
absolute, bounds divided by 1 + sum_j |g_j q_j|):

    scene T7 (7 joints, W = 40, 7 balls, 14 pairs = 560 pair rows, 7 tilts = 280 tilt items, 1 line, 1 capsule):  values 4.4e-16, bounds 1.0e-15
    scene T8 (8 joints, W = 2, 1 ball without rows, tilts in frames 8 and 1):                                     values 3.3e-16, bounds 2.0e-16
    scene TF (2 joints, alpha_0 = pi / 2, the flips of activity and verdict at -+ 2^-20 rad):                     values 5.6e-17, bounds 7.3e-17
    scenes TE, TEA (identity rotations, dyadic or exactly dotted vectors):                                        values 0, bounds 0 (exact)
    scene TM (gripper ball with work-space limits, 2 lines, 1 capsule, 1 cuboid, 3 balls, 2 pairs, 2 tilts):      values 8.9e-16, bounds 5.5e-16

-> GPU tolerance 32 x the figure, never looser than 1e-13; TE and TEA are compared bit for bit.  No row of a committed trajectory
is within 1e-9 of its threshold and no verdict is excluded: the share of comparisons a GPU test may leave out is zero.
Populations of T7: 2 accepted / 6 rejected, two by a tilt alone; every tilt has active and inactive rows, five of the seven
reject somewhere.  The gradient of the definition agrees with mpmath's own derivative of c(q) to 1.6e-41.  Run with -s to see
the figures."""
import json
import math

import numpy as np
import pytest

import dh_refs as DH
import gomp_refs as G
import pair_refs as P
import tilt_refs as T

MP = G.MP


def test_gradient_against_mpmaths_own_derivative():
    """g_j of the definition against d c / d q_j taken by mpmath (central differences at 50 digits) on the 7- and 8-joint chains."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for ch, n in ((DH.C7, 7), (DH.C8, 8)):
        for _ in range(3):
            q = rng.uniform(-2.5, 2.5, n)
            for frame in range(1, n + 1):
                a, r = rng.normal(size=3), rng.normal(size=3)
                t = T.tilt(frame, a / np.linalg.norm(a), r / np.linalg.norm(r), 1.0, 0.1)
                c, _, g = T.tilt_cosine(DH.chain_frames(ch, q)[1], t)
                for j in range(n):
                    f = lambda x: T.tilt_cosine(DH.chain_frames(ch, [MP.mpf(float(v)) if i != j else x for i, v in enumerate(q)])[1], t)[0]
                    d = MP.diff(f, MP.mpf(float(q[j])), h=MP.mpf(10) ** -20)
                    worst = max(worst, float(abs(d - g[j])))
                    if j >= frame:
                        assert g[j] == 0
    print(f"\ngradient of the definition against mpmath's derivative of c(q): largest difference {worst:.3e}")
    assert worst <= 1e-30


def test_the_tilt_angle_of_scene_TF_is_the_second_joint():
    for t in T.scene("TF")["trajs"]:
        for w in range(T.TF_W):
            q = t[2 * w:2 * w + 2]
            c = T.tilt_cosine(DH.chain_frames(T.CF, q)[1], T.TF_TILTS[0])[0]
            assert abs(MP.acos(c) - abs(MP.mpf(float(q[1])))) < 1e-15


@pytest.mark.parametrize("name", T.SCENES)
def test_fp64_error_and_gpu_tolerance(name):
    ev, eb = T.fp64_error(name)
    tv, tb = T.gpu_tolerance(name)
    print(f"\nscene {name}: fp64 error of the formulas: values {ev:.3e} (absolute), bounds {eb:.3e} (per term scale); GPU tolerance {tv:.3e} / {tb:.3e}")
    assert tv == min(32 * ev, 1e-13) and tb == min(32 * eb, 1e-13)
    if name in T.EXACT:
        assert ev == 0.0 and eb == 0.0 and (tv, tb) == (0.0, 0.0)              # exact in any order of operations
        for hi, lo in zip(T.scene_reference(name), T.scene_reference(name, G.F64)):
            for k in ("vals", "l", "u"):
                assert np.array_equal(hi[k], lo[k])
            assert hi["ok"] == lo["ok"] and hi["cls"] == lo["cls"]
    else:
        assert 0.0 < ev <= 1e-14 and 0.0 < eb <= 1e-14


def test_the_cosines_of_the_exact_scenes_are_correctly_rounded():
    """The thresholds are taken in fp64 by whoever creates the scene: for the bit-for-bit scenes np.cos and the C library's cos
    must both give mpmath's correctly rounded cosine at every angle used."""
    for a in T.TE_ANGLES:
        assert float(MP.cos(MP.mpf(a))) == float(np.cos(np.float64(a))) == math.cos(a), a


@pytest.mark.parametrize("name", T.SCENES)
def test_scene_populations(name):
    s, p = T.scene(name), T.populations(name)
    W, nb, npair, nt = s["W"], len(s["balls"]), len(s["pairs"]), len(s["tilts"])
    print(f"\nscene {name}: D = {s['D']}, W = {W}, {nb} balls, {npair} pairs ({npair * W} pair rows), {nt} tilts ({nt * W} tilt items);"
          f" accepted {p['accepted']}, rejected {p['rejected']} ({p['rejected_by_a_tilt_alone']} by a tilt alone), causes {dict(sorted(p['causes'].items()))}")
    print(f"  tilt rows per tilt: active {p['cells']['active'].tolist()}, none {p['cells']['none'].tolist()}, rejecting {p['rejecting'].tolist()}")
    print(f"  rows within 1e-9 of a threshold: {p['near']}; comparisons of the verdict within the margin: {p['near_comparisons']}; verdicts excluded: {p['verdicts_excluded']}")
    assert len(s["trajs"]) == 8 and s["trajs"].shape[1] == 2 * s["D"] * W
    assert len({t.tobytes() for t in s["trajs"]}) == 8
    assert p["tilt_rows"] == 8 * nt * W
    assert p["verdicts_excluded"] == 0 and p["near"] == 0 and p["near_comparisons"] == 0          # no case is left out on the GPU
    for t in s["tilts"]:
        assert abs(np.linalg.norm(t["axis"]) - 1) <= 1e-9 and abs(np.linalg.norm(t["ref"]) - 1) <= 1e-9 and 0 < t["max_angle"] < np.pi - G.ERROR
    ref = T.scene_reference(name)
    for e in ref:                                                             # tilt-major, behind the pair rows
        r0 = e["tilt_rows0"]
        assert r0 == e["block_rows"] + npair * W and len(e["l"]) == r0 + nt * W
        assert np.array_equal(e["tilt"][r0:], np.repeat(np.arange(nt), W)) and np.all(e["tilt"][:r0] == -1)
        assert np.array_equal(e["w"][r0:], np.tile(np.arange(W), nt))
        for k in range(r0, len(e["l"])):                                      # nothing from the tilt's frame on
            assert np.all(e["vals"][k][s["tilts"][int(e["tilt"][k])]["frame"]:] == 0.0)
    if name == "T7":
        assert (s["D"], W, nb * W, npair * W, nt * W) == (7, 40, 280, 560, 280)
        assert nt * W > 256 and (nt * W) % 256 != 0                           # both sides of the stride, a last partial round
        assert [t["frame"] for t in s["tilts"]] == [1, 2, 3, 4, 5, 6, 7]
        assert np.all(p["cells"]["active"] >= 1) and np.all(p["cells"]["none"] >= 1) and int(np.sum(p["rejecting"] > 0)) >= 4
        assert p["accepted"] >= 2 and p["rejected"] >= 2 and p["rejected_by_a_tilt_alone"] >= 1
        assert any(e["ok"] and any(c == "active" and k >= 0 for c, k in zip(e["cls"], e["tilt"])) for e in ref)      # active and accepted
    elif name == "T8":
        assert (s["D"], W, nb, npair) == (8, 2, 1, 0) and [t["frame"] for t in s["tilts"]] == [8, 1]
        assert ref[0]["tilt_rows0"] == 0                                      # the ball has no rows: nothing but tilt rows
        assert np.all(p["cells"]["active"] >= 1) and np.all(p["cells"]["none"] >= 1) and np.all(p["rejecting"] >= 1)
        assert p["accepted"] >= 2 and p["rejected"] >= 2
        assert any(e["vals"][k][7] != 0.0 for e in ref for k in range(W))      # the last joint's column
    elif name == "TF":
        assert [e["ok"] for e in ref] == [True, True, False, True, False, True, False, False]
    elif name in T.EXACT:
        assert not any(e["ok"] for e in ref) and all(e["causes"] == {"tilt"} for e in ref)
    else:
        assert npair == 2 and s["balls"][0]["gripper"] and np.all(p["cells"]["active"] >= 1) and np.all(p["cells"]["none"] >= 1)
        base = P.scene_reference("PM")
        for e, b in zip(ref, base):                                           # the rows before the tilts are pair_refs' own
            assert np.array_equal(e["vals"][:e["tilt_rows0"]], b["vals"]) and np.array_equal(e["l"][:e["tilt_rows0"]], b["l"])


def _row(e, tilt, w):
    k = [i for i in range(len(e["l"])) if (e["tilt"][i], e["w"][i]) == (tilt, w)]
    assert len(k) == 1
    return k[0]


def test_the_flips_of_scene_TF():
    s, ref = T.scene("TF"), T.scene_reference("TF")
    cls = lambda b, tilt, w: ref[b]["cls"][_row(ref[b], tilt, w)]
    assert (cls(0, 0, 1), cls(0, 0, 2)) == ("none", "active") and (cls(1, 0, 1), cls(1, 0, 3)) == ("none", "active")      # margin 1/8
    assert (cls(2, 1, 0), cls(2, 1, 2)) == ("none", "active")                                                             # margin 0
    assert all(cls(b, 1, w) == "none" for b in (0, 1, 3, 4, 5) for w in range(T.TF_W))
    slack = lambda b, tilt, w: [m["slack"] for m in ref[b]["margins"] if m["kind"] == "tilt" and (m["idx"], m["w"]) == (tilt, w)][0]
    assert 0 < slack(3, 0, 2) < 1e-6 and -1e-6 < slack(4, 0, 2) < 0 and 0 < slack(5, 0, 1) < 1e-6                        # 2^-20 rad either way
    assert 0 < slack(6, 1, 3) < 1e-6 and -1e-6 < slack(7, 1, 0) < 0
    assert ref[4]["causes"] == {"tilt"} and sum(m["slack"] < 0 for m in ref[4]["margins"]) == 1
    assert len(s["tilts"]) == 2 and (s["tilts"][0]["margin"], s["tilts"][1]["margin"]) == (1 / 8, 0.0)


def test_the_exact_cases_of_scenes_TE_and_TEA():
    s, ref = T.scene("TEA"), T.scene_reference("TEA")
    q0, q1 = T.TE_Q
    for b, e in enumerate(ref):
        for w in range(T.TE_W):
            k = _row(e, 0, w)                                                 # c = 0.6 beyond the cone: active, rejected
            assert e["c"][k] == 0.6 and e["vals"][k].tolist() == [0.8, 0.8, 0.0] and e["cls"][k] == "active"
            assert e["l"][k] == (math.cos(0.875) - 0.6) + (0.8 * q0 + 0.8 * q1)
            k = _row(e, 1, w)                                                 # u = ref: a zero row, inactive
            assert e["c"][k] == 1.0 and e["vals"][k].tolist() == [0.0, 0.0, 0.0] and (e["cls"][k], e["l"][k]) == ("none", -G.INF)
            k = _row(e, 2, w)                                                 # inactive: the gradient all the same
            assert e["vals"][k].tolist() == [0.8, 0.8, 0.0] and (e["cls"][k], e["l"][k]) == ("none", -G.INF)
            k = _row(e, 3, w)                                                 # frame 1: nothing in the second column
            assert e["c"][k] == 0.6 and e["vals"][k].tolist() == [0.8, 0.0, 0.0] and e["l"][k] == (math.cos(1.0) - 0.6) + 0.8 * q0
            k = _row(e, 4, w)                                                 # u = -ref: a zero row, active: 0 >= cos_lim + 1
            assert e["c"][k] == -1.0 and e["vals"][k].tolist() == [0.0, 0.0, 0.0] and e["cls"][k] == "active"
            assert e["l"][k] == math.cos(0.5) + 1.0 > 0.0
    for e, f in zip(ref, T.scene_reference("TE")):                            # TE: the same without the last tilt
        n = len(f["l"])
        assert np.array_equal(e["vals"][:n], f["vals"]) and np.array_equal(e["l"][:n], f["l"]) and n == 4 * T.TE_W


def test_known_answers_equal_what_the_reference_computes_now():
    assert T.load_kats() == json.loads(json.dumps(T.kats_now()))


def test_no_tilts_is_pair_refs_own_result():
    s = P.scene("PM")
    for t in s["trajs"][:2]:
        a = P.with_obstacles(s["D"], s["W"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["pairs"], s["con_lo"], s["con_hi"], t, s["margin"])
        b = T.with_obstacles(s["D"], s["W"], None, s["balls"], s["lines"], s["capsules"], s["cuboids"], s["pairs"], [], s["con_lo"], s["con_hi"], t, s["margin"])
        for k in ("vals", "l", "u", "l_scale", "u_scale"):
            assert np.array_equal(a[k], b[k])
        assert a["cls"] == b["cls"] and a["ok"] == b["ok"] and a["causes"] == b["causes"] and a["verdict_excluded"] == b["verdict_excluded"]
    tm = T.scene_batch("TM", True)
    assert tm["m"] > tm["row0"] + tm["rows3d"] and tm["rows3d"] == tm["block_rows"] + (2 + 2) * s["W"]


def test_the_rejected_qps_of_the_exact_scenes_on_the_oracle():
    """The QPs that tests/test_gpu_tilts.py solves after mi_gomp_relinearise_some, on the reference's rows: those of TE are
    solved, those of TEA, with the antiparallel tilt's row 0 >= cos_lim + 1, are primal infeasible."""
    from oracle import oracle as O
    for name in T.EXACT:
        s, ref, pr = T.scene(name), T.scene_reference(name), T.scene_batch(name)
        for b in (0, 5):
            Ax, l, u = G.reference_rows(pr, b, ref[b])
            A = pr["A"].copy()
            A.data = Ax
            o = O.OracleQPSolver(pr["P"], None, pr["A"], pr["l"][b], pr["u"][b], scaling=0)
            o.update(l, A, u)
            o.set_warm_start(s["trajs"][b])
            st, _ = o.solve()
            print(f"\noracle on the re-linearised QP {b} of scene {name}: status {st}, {o.info().iter} iterations")
            assert st == (1 if name == "TE" else -3), (name, b, st)
