"""CPU: the mpmath reference of the distance grids (tests/grid_refs.py) checked on its own - the scenes' populations (no near row,
no excluded verdict: the cap is zero), the exact scenes, the flips, the known answers, the fp64 error the GPU tolerance is
built on, and the face regions in which a re-sampled box gives the cuboid's rows."""
import json

import numpy as np
import pytest

import cuboid_refs as X
import gomp_refs as G
import grid_refs as R

# fp64_error (values, bounds) of the np.float64 restatement against mpmath, as measured; the GPU tolerance is 32 x these, never
# looser than 1e-13
FP64_ERROR = {"GT": (0.0, 0.0), "GP": (0.0, 0.0), "G8": (3.5e-17, 2.2e-16), "G7": (1.9e-15, 3.7e-15), "GM": (8.9e-16, 4.9e-16)}


@pytest.mark.parametrize("name", R.SCENES + ("GX",))
def test_no_near_row_and_no_excluded_verdict(name):
    pop = R.populations(name)
    print(name, pop)
    assert pop["near"] == 0 and pop["near_comparisons"] == 0 and pop["verdicts_excluded"] == 0
    s = R.scene(name)
    assert pop["grid_rows"] == 8 * s["W"] * len(s["balls"]) * len(s["grids"])


def test_populations_of_the_scenes():
    gt = R.populations("GT")
    assert gt["cells"]["active"].tolist() == [3, 1] and gt["cells"]["none"].tolist() == [14, 2] and gt["cells"]["outside"].tolist() == [47, 61]
    assert gt["accepted"] == 7 and gt["rejected_by_a_grid_alone"] == 1
    g7 = R.populations("G7")
    assert all(g7["cells"][c][0] > 20 for c in R.CLASSES)                     # the big grid: every class
    assert g7["cells"]["outside"][1] > 10 * (g7["cells"]["active"][1] + g7["cells"]["none"][1]) > 0      # the small grid: most balls outside
    assert g7["rejecting"][0] > 0
    g8 = R.populations("G8")
    assert g8["cells"]["active"][0] > 0 and g8["cells"]["none"][0] > 0
    gm = R.populations("GM")
    assert all(gm["cells"][c][0] > 0 for c in R.CLASSES)
    s = R.scene("G7")
    assert (s["W"] * len(s["balls"]), len(s["lines"]), len(s["capsules"]), len(s["cuboids"]), len(s["pairs"]), len(s["tilts"])) == (280, 1, 1, 1, 2, 1)


def test_gt_values_have_no_symmetry_and_are_dyadic():
    v = R._gt_values()
    assert v.shape == (5, 4, 3) and np.array_equal(v * 8, np.round(v * 8))
    for axes in [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]:        # (a permutation of the axes changes the shape)
        assert not np.array_equal(v, np.flip(v, axes))
    assert len(set(v[3:5, 2:4, 1:3].reshape(-1))) == 1


@pytest.mark.parametrize("name", R.EXACT + ("GX",))
def test_exact_scenes_are_exact_in_fp64(name):
    assert R.fp64_error(name) == (0.0, 0.0)
    for hi, lo in zip(R.scene_reference(name), R.scene_reference(name, G.F64)):
        assert np.array_equal(hi["vals"], lo["vals"]) and np.array_equal(hi["l"], lo["l"]) and hi["cls"] == lo["cls"] and hi["ok"] == lo["ok"]


@pytest.mark.parametrize("name", R.SCENES)
def test_fp64_error_figures(name):
    ev, eb = R.fp64_error(name)
    print(name, ev, eb)
    assert ev <= FP64_ERROR[name][0] and eb <= FP64_ERROR[name][1]
    if name not in R.EXACT:
        assert ev >= FP64_ERROR[name][0] / 4 and eb >= FP64_ERROR[name][1] / 4      # the figures above are what was measured


def _rows(name, traj, grid_index=0):
    """{w: (cls, vals, l, inside)} of grid `grid_index` for the one ball of scene GT / GP."""
    s, e = R.scene(name), R.scene_reference(name)[traj]
    ng = len(s["grids"])
    return {w: (e["cls"][w * ng + grid_index], e["vals"][w * ng + grid_index].tolist(), float(e["l"][w * ng + grid_index]), bool(e["inside"][w * ng + grid_index]))
            for w in range(s["W"])}


def test_the_cases_of_scene_GT():
    s = R.scene("GT")
    a = s["grids"][0]
    r0 = _rows("GT", 0)
    # a node: phi is its value, the gradient the forward differences of the upper cell
    inside, phi, Gr, _ = R.sample(a, [G.MP.mpf(x) for x in R._gt_point((1, 1, 1))])
    assert inside and phi == R.node(a, 1, 1, 1)
    assert [float(x) for x in Gr] == [(R.node(a, 2, 1, 1) - phi) * 4, (R.node(a, 1, 2, 1) - phi) * 4, (R.node(a, 1, 1, 2) - phi) * 4]
    # a point on a cell face belongs to the upper cell: f_x = 1 exactly, the x difference is that of nodes 1 .. 2
    inside, phi, Gr, f = R.sample(a, [G.MP.mpf(x) for x in R._gt_point((1, 1.5, 2.25))])
    lo = [R.node(a, 1, 1, 2), R.node(a, 2, 1, 2), R.node(a, 1, 2, 2), R.node(a, 2, 2, 2), R.node(a, 1, 1, 3), R.node(a, 2, 1, 3), R.node(a, 1, 2, 3), R.node(a, 2, 2, 3)]
    ex = [lo[1] - lo[0], lo[3] - lo[2], lo[5] - lo[4], lo[7] - lo[6]]
    assert float(Gr[0]) == ((ex[0] + ex[1]) / 2 * 0.75 + (ex[2] + ex[3]) / 2 * 0.25) * 4
    # the last node of each axis: inside, in cell n_k - 2 with t = 1: phi is the node's value
    for f, nd in (((2, 1, 1), (2, 1, 1)), ((1, 3, 1), (1, 3, 1)), ((1, 1, 4), (1, 1, 4)), ((2, 3, 4), (2, 3, 4))):
        inside, phi, _, _ = R.sample(a, [G.MP.mpf(x) for x in R._gt_point(f)])
        assert inside and phi == R.node(a, *nd)
    assert all(r0[w][3] for w in range(1, 7)) and not r0[0][3] and not r0[7][3]
    # 2^-20 outside on either side of each axis: zero rows without bounds, and no verdict though node (0,0,0) is in the material
    r1 = _rows("GT", 1)
    assert all(r1[w] == ("outside", [0.0, 0.0, 0.0], -G.INF, False) for w in range(8))
    assert R.scene_reference("GT")[1]["ok"] and R.node(a, 0, 0, 0) - R.GT_R < -G.ERROR
    # mid-cell
    inside, phi, Gr, f = R.sample(a, [G.MP.mpf(x) for x in R._gt_point((0.25, 1.5, 2.75))])
    assert [float(x) - int(x) for x in f] == [0.25, 0.5, 0.75]
    # the flat cell: G = 0, the rows all zeros and inactive
    r3 = _rows("GT", 3)
    assert all(r3[w] == ("none", [0.0, 0.0, 0.0], -G.INF, True) for w in (1, 3, 5, 6))
    # the flips: activity at s = margin -+ 2^-20 (grid A, margin 1/8; grid B, margin 0), the verdict at s = -ERROR -+ 2^-20
    r4 = _rows("GT", 4)
    assert (r4[1][0], r4[2][0]) == ("active", "none") and r4[1][1][0] == r4[2][1][0] == 1.0      # written all the same
    r7 = _rows("GT", 7, 1)
    assert (r7[1][0], r7[2][0], r7[5][0]) == ("active", "none", "none") and r7[1][1] == [1.0, 0.0, 0.0]
    ok = [e["ok"] for e in R.scene_reference("GT")]
    assert ok == [True] * 6 + [False, True]
    assert R.scene_reference("GT")[6]["causes"] == {"grid"}
    m5 = [m for m in R.scene_reference("GT")[5]["margins"] if m["kind"] == "grid" and m["w"] == 2][0]
    m6 = [m for m in R.scene_reference("GT")[6]["margins"] if m["kind"] == "grid" and m["w"] == 2][0]
    assert 0 < m5["slack"] < 2 * R.E20 and -2 * R.E20 < m6["slack"] < 0
    # scene GP: margin 0
    p4 = _rows("GP", 4)
    assert (p4[1][0], p4[2][0]) == ("active", "none")


def test_known_answers():
    now = json.loads(json.dumps(R.kats_now()))
    assert now == R.load_kats()


def test_from_obstacles_is_the_primitives_distance_at_the_nodes():
    g = R.g7_grids()[0]
    # a node inside the box: minus the distance to the nearest face; all values finite, some negative
    v = np.array(g["values"])
    assert np.isfinite(v).all() and (v < 0).any() and (v > 0.2).any()
    o, c = g["origin"], g["cell"]
    P = [np.float64(o[0]) + 5 * np.float64(c), np.float64(o[1]) + 3 * np.float64(c), np.float64(o[2]) + 1 * np.float64(c)]
    assert R.node(g, 5, 3, 1) == min(R._capsule_distance(R.G7_CAP, np.array(P)) - 0.03, float(X.probe(R.G7_BOX, P, G.F64)[0]))


def test_a_resampled_box_gives_the_cuboids_rows_in_the_face_regions():
    """Scene GX against scene XT of cuboid_refs, cuboid 0: where face_region_exact() holds, the grid's row is the cuboid's."""
    gx, xt = R.scene_reference("GX"), X.scene_reference("XT")
    s = R.scene("GX")
    W, nb = s["W"], len(s["balls"])
    same = differs = 0
    for t in range(8):
        for bi in range(nb):
            for w in range(W):
                p = s["trajs"][t][3 * w:3 * w + 3]
                kg = bi * W + w
                kx = (bi * W + w) * 2                                            # XT has two cuboids per block
                if not R.face_region_exact(p):
                    differs += 1
                    continue
                same += 1
                assert gx[t]["vals"][kg].tolist() == xt[t]["vals"][kx].tolist() and gx[t]["l"][kg] == xt[t]["l"][kx], (t, bi, w)
    print("face-region points", same, "others", differs)
    assert same >= 10
