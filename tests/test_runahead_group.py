"""CPU: the run-ahead group of a rho-update point (host_core.hpp runahead_group, DESIGN.md section 3 "Run-ahead").

The group is chosen among the tiles that are still active, by the scale-free score pri_res / median(pri_res) + dua_res /
median(dua_res) of the check that has just run (medians over the active tiles), descending, ties by tile index.  It uses
nothing but those residuals.  The fixture tests/golden/runahead_residuals.json holds what the oracle recorded for a fixed
sample of the headline batch (problems.random_box_qp(1024, value_seed=1000), every fourth QP): pri_res / dua_res after 100
iterations of the QPs that have not finished by then, and the iteration count of their full solve.  Every QP of the sample that
needs more than 125 iterations must sit inside a group of half the sample's active count."""
import json
import os

import numpy as np
import pytest

import osqp_solver_amd as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "runahead_residuals.json")


def test_order_is_descending_score():
    tiles = [3, 5, 8, 9, 12]
    pri = [1.0, 4.0, 2.0, 1.0, 1.0]
    dua = [1.0, 1.0, 1.0, 8.0, 2.0]
    # medians (upper of the sorted values): pri 1.0, dua 1.0 -> scores 2, 5, 3, 9, 3
    assert M.debug_runahead_group(tiles, pri, dua, 5, 1) == [9, 5, 8, 12, 3]
    assert M.debug_runahead_group(tiles, pri, dua, 2, 1) == [9, 5]


def test_score_is_scale_free():
    rng = np.random.default_rng(7)
    tiles = list(range(0, 80, 2))
    pri, dua = rng.lognormal(size=40), rng.lognormal(size=40)
    g = M.debug_runahead_group(tiles, pri, dua, 10, 1)
    assert g == M.debug_runahead_group(tiles, 1e-9 * pri, 1e7 * dua, 10, 1)
    assert len(g) == 10 and len(set(g)) == 10 and set(g) <= set(tiles)


def test_ties_go_to_the_lower_tile():
    tiles = [7, 2, 11, 4]           # (any order of the input)
    one = [1.0] * 4
    assert M.debug_runahead_group(tiles, one, one, 3, 1) == [2, 4, 7]
    assert M.debug_runahead_group(tiles, [1.0, 1.0, 2.0, 1.0], one, 3, 1) == [11, 2, 4]


def test_fewer_active_tiles_than_the_minimum_give_no_group():
    tiles, r = list(range(9)), [1.0] * 9
    assert M.debug_runahead_group(tiles, r, r, 4, 10) == []
    assert M.debug_runahead_group(tiles, r, r, 4, 9) == [0, 1, 2, 3]


def test_empty_input_and_empty_group():
    assert M.debug_runahead_group([], [], [], 8, 0) == []
    assert M.debug_runahead_group([1, 2], [1.0, 2.0], [1.0, 2.0], 0, 1) == []


def test_group_larger_than_the_active_set_takes_every_tile():
    assert M.debug_runahead_group([4, 6], [1.0, 3.0], [1.0, 1.0], 128, 1) == [6, 4]


def test_zero_and_nan_residuals_have_a_place():
    # a zero median cannot scale: residuals above it count as infinitely far, those at it as 0; NaN ranks first
    g = M.debug_runahead_group([0, 1, 2, 3], [0.0, 0.0, 0.0, 1.0], [1.0, 2.0, 1.0, 1.0], 4, 1)
    assert g == [3, 1, 0, 2]
    g = M.debug_runahead_group([0, 1, 2], [1.0, float("nan"), 2.0], [1.0, 1.0, 1.0], 3, 1)
    assert g == [1, 2, 0]


def test_bad_arguments_are_refused():
    with pytest.raises(M.MiOsqpError):
        M.debug_runahead_group([1, 1], [1.0, 1.0], [1.0, 1.0], 1, 1)          # a tile twice
    with pytest.raises(M.MiOsqpError):
        M.debug_runahead_group([1, 2], [1.0, -1.0], [1.0, 1.0], 1, 1)         # a negative residual


def test_late_qps_of_the_headline_sample_sit_in_a_group_of_half_the_active_count():
    with open(GOLDEN) as f:
        g = json.load(f)
    qps, pri, dua, iters = g["qp"], g["pri_res"], g["dua_res"], g["iterations"]
    assert len(qps) == len(pri) == len(dua) == len(iters) and len(qps) >= 100
    assert all(it > 100 for it in iters)                    # the active set after iteration 100
    late = {q for q, it in zip(qps, iters) if it > 125}
    assert len(late) >= 3, late                              # the sample holds late QPs at all
    group = M.debug_runahead_group(qps, pri, dua, len(qps) // 2, 1)
    assert len(group) == len(qps) // 2
    rank = {q: r for r, q in enumerate(group)}
    print("late QPs and their ranks:", sorted((rank.get(q, -1), q) for q in late), "of", len(qps), "active")
    assert late <= set(group), sorted(late - set(group))
