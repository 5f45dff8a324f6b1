"""CPU: grasp goals before anything runs on a GPU - the reference of tests/goal_refs.py against mpmath's own derivatives of the
ball's centre and of c(q), its own known answers (tests/golden/goal_kats.json), the populations of the scenes of
tests/test_gpu_goals.py and the fp64 error from which their GPU tolerance is derived.

Measured here (np.float64 evaluation of the formulas against the mpmath one over the eight QPs of each scene; values absolute,
bounds divided by their term scale |point| + tol + |p| + sum_j |J q_j| or 1 + sum_j |g_j q_j|):

    scene G7 (7 joints, W = 40, 7 balls, 14 pairs, 7 tilts; goals at waypoints 37 (frame 7) and 20 (position only)):  values 4.4e-16, bounds 1.0e-15
    scene G8 (8 joints, W = 2, 1 ball without rows; goals at waypoints 0 (frame 8) and 1 (frame 1)):                  values 2.8e-16, bounds 2.1e-16
    scene GF (3 joints, the TABLE ball, the flips of the verdict at -+ 2^-20 m and rad, a free axis, tol = 0):         values 5.6e-17, bounds 4.5e-17
    scene GX (the TABLE ball, identity rotations, dyadic or exactly dotted numbers; frame 0; the antiparallel case):  values 0, bounds 0 (exact)
    scene GM (gripper ball with work-space limits, 2 lines, 1 capsule, 1 cuboid, 1 grid, 2 pairs, 2 tilts, 2 goals):   values 8.9e-16, bounds 5.5e-16

-> GPU tolerance 32 x the figure, never looser than 1e-13; GX is compared bit for bit.  Goal rows are always active, so no row
hangs on an activity threshold; no comparison of a verdict of a committed trajectory is within 1e-9 of its threshold and no
verdict is excluded: the share of verdicts a GPU test may leave out is zero, and the tests assert that.  The rows of the
definition, rounded to fp64, agree with mpmath's own derivatives to half an ulp.  Run with -s to see the figures."""
import json
import math

import numpy as np
import pytest

import dh_refs as DH
import gomp_refs as G
import goal_refs as Q
import tilt_refs as T

MP = G.MP


def test_gradients_against_mpmaths_own_derivatives():
    """Rows 0 .. 2 against d p_ax / d q_j and row 3 against d c / d q_j, both taken by mpmath (central differences at 50 digits),
    on the 8-joint chain: a ball of frame 8 and of frame 3, the axis in frames 8 and 1."""
    rng = np.random.default_rng(9)
    worst_p = worst_c = 0.0
    ch, n = DH.C8, 8
    for frame_ball, frame_axis in ((8, 8), (3, 1), (5, 4)):
        ball = DH.chain_ball(ch, frame_ball, (0.02, -0.01, 0.06), 0, 0.04)
        q = rng.uniform(-2.5, 2.5, n)
        traj = np.concatenate([q, q, np.zeros(2 * n)])
        a, r = rng.normal(size=3), rng.normal(size=3)
        gl = Q.goal(0, 1, frame_axis, a / np.linalg.norm(a))
        v = Q.value((0.1, 0.2, 0.3), (0.01, 0.0, 0.5), r / np.linalg.norm(r), 1.0)
        rows, _ = Q.goal_rows(ch, [ball], gl, v, traj, n)
        for j in range(n):
            at = lambda x: [MP.mpf(float(t)) if i != j else x for i, t in enumerate(q)]
            for ax in range(3):
                d = MP.diff(lambda x: DH.chain_point(ch, at(x), frame_ball, ball["param"][1:4])[0][ax], MP.mpf(float(q[j])), h=MP.mpf(10) ** -20)
                worst_p = max(worst_p, abs(float(d) - rows[ax]["vals"][j]))
                if j >= frame_ball:
                    assert rows[ax]["vals"][j] == 0.0
            tl = dict(frame=frame_axis, axis=gl["axis"], ref=v["ref"])
            d = MP.diff(lambda x: T.tilt_cosine(DH.chain_frames(ch, at(x))[1], tl)[0], MP.mpf(float(q[j])), h=MP.mpf(10) ** -20)
            worst_c = max(worst_c, abs(float(d) - rows[3]["vals"][j]))
            if j >= frame_axis:
                assert rows[3]["vals"][j] == 0.0
    print(f"\nrows of the definition against mpmath's derivatives (after rounding the rows to fp64): position {worst_p:.3e}, axis {worst_c:.3e}")
    assert worst_p <= 4e-16 and worst_c <= 4e-16                              # the rows are returned as doubles: half an ulp of numbers below 2


@pytest.mark.parametrize("name", Q.SCENES)
def test_fp64_error_and_gpu_tolerance(name):
    ev, eb = Q.fp64_error(name)
    tv, tb = Q.gpu_tolerance(name)
    print(f"\nscene {name}: fp64 error of the formulas: values {ev:.3e} (absolute), bounds {eb:.3e} (per term scale); GPU tolerance {tv:.3e} / {tb:.3e}")
    assert tv == min(32 * ev, 1e-13) and tb == min(32 * eb, 1e-13)
    if name in Q.EXACT:
        assert ev == 0.0 and eb == 0.0 and (tv, tb) == (0.0, 0.0)              # exact in any order of operations
        for hi, lo in zip(Q.scene_reference(name), Q.scene_reference(name, G.F64)):
            for k in ("vals", "l", "u"):
                assert np.array_equal(hi[k], lo[k])
            assert hi["ok"] == lo["ok"] and hi["cls"] == lo["cls"]
    else:
        assert 0.0 < ev <= 1e-14 and 0.0 < eb <= 1e-14


def test_the_cosines_of_the_exact_scene_are_correctly_rounded():
    """The thresholds are taken in fp64 by whoever sets the values: for the bit-for-bit scene np.cos and the C library's cos must
    both give mpmath's correctly rounded cosine at every angle used."""
    angles = sorted({a for per in Q.scene("GX")["values"] for v in per for a in Q.threshold_angles(v)})
    assert len(angles) >= 10
    for a in angles:
        assert float(MP.cos(MP.mpf(a))) == float(np.cos(np.float64(a))) == math.cos(a), a


@pytest.mark.parametrize("name", Q.SCENES)
def test_scene_populations(name):
    s, p = Q.scene(name), Q.populations(name)
    W, ng = s["W"], len(s["goals"])
    print(f"\nscene {name}: D = {s['D']}, W = {W}, {len(s['balls'])} balls, {ng} goals; accepted {p['accepted']}, rejected {p['rejected']}"
          f" ({p['rejected_by_a_goal_alone']} by a goal alone), accepted by the goals {p['accepted_by_the_goals']}")
    print(f"  goal rows per class: {p['cells']}, rejecting comparisons {p['rejecting']}")
    print(f"  comparisons of the verdict within 1e-9 of a threshold: {p['near_comparisons']}; rows near a threshold: {p['near_rows']}; verdicts excluded:"
          f" {p['verdicts_excluded']} of 8 (share {p['verdicts_excluded'] / 8:.0%})")
    assert len(s["trajs"]) == Q.B and s["trajs"].shape[1] == 2 * s["D"] * W and len(s["values"]) == Q.B
    assert len({t.tobytes() for t in s["trajs"]}) == Q.B
    assert len({json.dumps(v) for v in s["values"]}) == Q.B                  # every QP asks something else
    assert p["goal_rows"] == Q.B * 4 * ng
    assert p["verdicts_excluded"] == 0 and p["near_comparisons"] == 0 and p["near_rows"] == 0      # the share of excluded verdicts is 0
    for e in Q.scene_reference(name):
        assert not e["verdict_excluded"] and not e["near"].any()
        for m in e["margins"]:
            if m["kind"] in ("goal_pos", "goal_axis"):
                assert abs(m["slack"]) >= 1e-9
    for per in s["values"]:
        for gl, v in zip(s["goals"], per):
            assert all(t >= 0 for t in v["tol"])
            if gl["frame"] >= 1:
                assert abs(np.linalg.norm(v["ref"]) - 1) <= 1e-9 and abs(np.linalg.norm(gl["axis"]) - 1) <= 1e-9 and 0 < v["max_angle"] < np.pi - G.ERROR
    ref = Q.scene_reference(name)
    for e in ref:                                                             # goal-major, four rows each, behind the tilt rows
        r0 = e["goal_rows0"]
        assert r0 == e["tilt_rows0"] + len(s["tilts"]) * W and len(e["l"]) == r0 + 4 * ng
        assert np.array_equal(e["goal"][r0:], np.repeat(np.arange(ng), 4)) and np.all(e["goal"][:r0] == -1)
        for k, gl in enumerate(s["goals"]):
            assert np.all(e["w"][r0 + 4 * k:r0 + 4 * k + 4] == gl["waypoint"])
            assert e["cls"][r0 + 4 * k + 3] == ("axis" if gl["frame"] >= 1 else "zero")
            if gl["frame"] >= 1:
                assert np.all(e["vals"][r0 + 4 * k + 3][gl["frame"]:] == 0.0)   # nothing from the axis' frame on
    if name == "G7":
        assert (s["D"], W, len(s["balls"]), len(s["pairs"]), len(s["tilts"])) == (7, 40, 7, 14, 7)
        assert [(g["waypoint"], g["frame"]) for g in s["goals"]] == [(37, 7), (20, 0)]
        assert 2 <= p["accepted_by_the_goals"] <= 6 and all(p["cells"][c] >= 8 for c in Q.CLASSES)
    elif name == "G8":
        assert (s["D"], W, len(s["balls"])) == (8, 2, 1) and [(g["waypoint"], g["frame"]) for g in s["goals"]] == [(0, 8), (1, 1)]
        assert ref[0]["goal_rows0"] == 0                                      # the ball has no rows: nothing but goal rows
        assert any(e["vals"][3][7] != 0.0 for e in ref)                       # the last joint's column of the frame-8 axis row
        assert all(np.count_nonzero(e["vals"][7]) == 1 and e["vals"][7][0] != 0.0 for e in ref)      # frame 1: a one-column gradient
        assert p["accepted"] >= 2 and p["rejected"] >= 2
    elif name == "GF":
        assert [e["ok"] for e in ref] == [True, False, True, False, True, False, True, False]
        assert all(e["causes"] == {"goal"} for e in ref if not e["ok"])
    elif name == "GX":
        anti = ref[Q.GX_ANTI]
        r0 = anti["goal_rows0"]
        assert not anti["vals"][r0 + 11].any() and anti["l"][r0 + 11] == float(np.cos(np.float64(s["values"][Q.GX_ANTI][2]["max_angle"]))) + 1.0 > 0      # primal infeasible
        assert all(not e["vals"][e["goal_rows0"] + 7].any() and e["l"][e["goal_rows0"] + 7] == -G.INF for e in ref)                                          # frame 0: zeros
        assert p["accepted"] >= 2 and p["rejected"] >= 4
    elif name == "GM":
        assert ref[0]["goal_rows0"] == 88 and len(s["lines"]) == 2 and len(s["grids"]) == 1 and len(s["pairs"]) == 2 and len(s["tilts"]) == 2
        assert s["balls"][0]["gripper"]


def test_the_flips_of_scene_GF():
    """2^-20 m or rad decide the verdict, on either side, per axis; a free axis has no say; tol = 0 gives l == u."""
    s, ref = Q.scene("GF"), Q.scene_reference("GF")
    slack = lambda b, kind, ax: [m["slack"] for m in ref[b]["margins"] if m["kind"] == kind and m["ax"] == ax and m["idx"] == (0 if kind == "goal_axis" else 1)][0]
    for b, ax, sign in ((0, 0, 1), (1, 0, -1), (2, 1, 1), (3, 2, -1)):
        assert abs(slack(b, "goal_pos", ax) - sign * Q.E20) <= 1e-15
    assert 0 < slack(4, "goal_axis", -1) < 2e-6 and -2e-6 < slack(5, "goal_axis", -1) < 0
    r0 = ref[6]["goal_rows0"]
    assert ref[6]["cls"][r0 + 4] == "free" and ref[6]["l"][r0 + 4] == -G.INF and ref[6]["u"][r0 + 4] == G.INF and ref[6]["ok"]
    assert np.array_equal(ref[7]["l"][r0 + 4:r0 + 7], ref[7]["u"][r0 + 4:r0 + 7])                  # equalities
    for b in range(Q.B):                                                      # the angle of goal 0 is |q_1| at waypoint 1
        q = s["trajs"][b][3:6]
        c = ref[b]["c"][ref[b]["goal_rows0"] + 3]
        assert abs(math.acos(c) - abs(q[1])) < 1e-12


@pytest.mark.parametrize("name", Q.KAT_SCENES)
def test_known_answers(name):
    """tests/golden/goal_kats.json is what the reference computes now, number for number."""
    now = json.loads(json.dumps(Q.kats_now()[name]))
    kept = Q.load_kats()[name]
    assert now == kept
    assert len(kept["cases"]) == Q.B and all(len(c["l"]) == 4 * len(kept["goals"]) for c in kept["cases"])


def test_the_kept_fixed_end_plan():
    p = Q.load_kats()["plain_plan"]
    assert p["code"] == 0 and p["updates"] == 0 and len(p["x"]) % 14 == 0 and all(math.isfinite(float.fromhex(v)) for v in p["x"])
