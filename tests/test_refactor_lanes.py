"""CPU: the chunk lanes of a pipelined refactorisation (host_core.hpp refactor_lanes, DESIGN.md section 3 "Pipelined
refactorisation").  A lane is a stream that runs factor -> tail -> iterate of its chunks one after the other; chunks on
different lanes run side by side.  For every input:
  * every chunk is on exactly one lane, and the refactorisation chunks of a lane are in ascending order;
  * the iterate of every tile is ordered behind the tail of every chunk that holds one of the tile's flagged QPs - by the
    lane's own order, or by a listed wait for a chunk on another lane;
  * the scratch ranges of chunks on different lanes are disjoint and inside what the scratch holds;
  * one lane is the two-stream form: the chunks in order, no waits, every chunk's scratch at 0."""
import numpy as np
import pytest

import osqp_solver_amd as M


def _check(flagged, active, bt, chunk_qps, lanes, chunk0_first, scratch_slots=None):
    work, tiles = M.debug_refactor_chunks(flagged, active, bt, chunk_qps)
    rl = M.debug_refactor_lanes(flagged, active, bt, chunk_qps, lanes, chunk0_first=chunk0_first, scratch_slots=scratch_slots)
    k, L = len(work), rl["n_lanes"]
    assert 1 <= L <= min(lanes, max(1, k - 1))
    assert sorted(c for o in rl["order"] for c in o) == list(range(k))          # exactly one lane each
    for l, o in enumerate(rl["order"]):
        assert all(rl["lane_of"][c] == l for c in o)
        ref = [c for c in o if c]
        assert ref == sorted(ref)
    if L == 1:
        assert rl["order"] == [list(range(k))] and rl["waits"] == [] and all(b == 0 for b, _ in rl["scratch"])
    else:
        assert all(rl["lane_of"][c] == (c - 1) % L for c in range(1, k))
        o0 = rl["order"][rl["lane_of"][0]]
        if chunk0_first:
            assert rl["lane_of"][0] == L - 1 and o0[0] == 0
        else:
            assert o0[-1] == 0 and len(o0) - 1 == min(len([c for c in o if c]) for o in rl["order"])
    # ordering: tail of chunk d before the iterate of chunk c
    pos = {c: i for o in rl["order"] for i, c in enumerate(o)}

    def behind(c, d):
        if L == 1:
            return d <= c          # stream I waits for the event of chunk c on stream R, which runs the chunks in order
        return (rl["lane_of"][c] == rl["lane_of"][d] and pos[d] <= pos[c]) or (c, d) in rl["waits"]
    chunk_of_qp = {q: c for c, w in enumerate(work) for q in w}
    for c, tl in enumerate(tiles):
        for t in tl:
            for q in range(t * bt, (t + 1) * bt):
                if q in chunk_of_qp:
                    assert behind(c, chunk_of_qp[q]), (t, q, c, chunk_of_qp[q], rl)
    for c, d in rl["waits"]:
        assert 1 <= d < c and rl["lane_of"][c] != rl["lane_of"][d]
    # scratch
    for c in range(1, k):
        b, n = rl["scratch"][c]
        assert b % bt == 0 and n >= len(work[c]) and n % bt == 0
        if scratch_slots is not None:
            assert b + n <= scratch_slots
        for d in range(1, c):
            if rl["lane_of"][c] != rl["lane_of"][d]:
                b2, n2 = rl["scratch"][d]
                assert b + n <= b2 or b2 + n2 <= b, (c, d, rl["scratch"])
    return work, tiles, rl


@pytest.mark.parametrize("bt", [1, 2, 4])
@pytest.mark.parametrize("lanes", [1, 2, 3])
@pytest.mark.parametrize("chunk0_first", [False, True])
def test_random_flags(bt, lanes, chunk0_first):
    rng = np.random.default_rng(1000 * bt + 10 * lanes + chunk0_first)
    seen_chunks, seen_waits = set(), 0
    for n_chunks in range(1, 9):
        for n_slots in (40, 203):
            for p_act, p_flag in ((1.0, 0.6), (0.6, 0.6), (0.9, 1.0)):
                act = rng.random(n_slots) < p_act
                flg = (rng.random(n_slots) < p_flag) & (act | (rng.random(n_slots) < 0.02))
                flagged, active = np.flatnonzero(flg).tolist(), np.flatnonzero(act).tolist()
                if not flagged:
                    continue
                chunk_qps = (len(flagged) + n_chunks - 1) // n_chunks
                work, _, rl = _check(flagged, active, bt, chunk_qps, lanes, chunk0_first)
                seen_chunks.add(len(work) - 1)
                seen_waits += len(rl["waits"])
                assert rl["n_lanes"] == min(lanes, len(work) - 1)
    assert seen_chunks >= set(range(1, 9)), seen_chunks
    assert (seen_waits > 0) == (bt > 1 and lanes > 1)


def test_tile_of_two_split_over_two_lanes():
    # tile 1 = QPs 2, 3, the chunk border between them: its iterate (chunk 2, lane 1) waits for chunk 1's tail on lane 0
    _, tiles, rl = _check([0, 2, 3, 7], [0, 1, 2, 3, 4, 5, 7], 2, 2, 2, False)
    assert tiles == [[2], [0], [1, 3]]
    assert rl["order"] == [[1], [2, 0]] and rl["waits"] == [(2, 1)]
    assert rl["scratch"] == [(0, 0), (0, 2), (2, 2)]
    _, _, rl = _check([0, 2, 3, 7], [0, 1, 2, 3, 4, 5, 7], 2, 2, 2, True)
    assert rl["order"] == [[1], [0, 2]] and rl["waits"] == [(2, 1)]


def test_headline_shape():
    """605 flagged of 634 active QPs, one QP per tile, 3 x 202: one chunk per lane, chunk 0 behind the last lane's chunk."""
    rng = np.random.default_rng(7)
    active = np.sort(rng.choice(1024, 634, replace=False))
    flagged = np.sort(rng.choice(active, 605, replace=False))
    _, _, rl = _check(flagged.tolist(), active.tolist(), 1, 202, 3, False, scratch_slots=1028)
    assert rl["order"] == [[1], [2], [3, 0]] and rl["waits"] == []
    assert rl["scratch"] == [(0, 0), (0, 202), (202, 202), (404, 201)]
    _, _, rl = _check(flagged.tolist(), active.tolist(), 1, 101, 3, True, scratch_slots=1028)
    assert rl["order"] == [[1, 4], [2, 5], [0, 3, 6]]


def test_scratch_too_small_for_the_padded_list_falls_back_to_one_lane():
    # 9 flagged QPs in chunks of 2 at four slots per workgroup: 5 chunks padded to 4 slots each = 20 slots
    flagged = list(range(9))
    _, _, rl = _check(flagged, flagged, 4, 2, 3, False, scratch_slots=20)
    assert rl["n_lanes"] == 3
    _, _, rl = _check(flagged, flagged, 4, 2, 3, False, scratch_slots=16)
    assert rl["n_lanes"] == 1


def test_bad_arguments_are_refused():
    with pytest.raises(M.MiOsqpError):
        M.debug_refactor_lanes([0], [0], 1, 1, 0)
    with pytest.raises(M.MiOsqpError):
        M.debug_refactor_lanes([0], [0], 1, 1, 4)
    with pytest.raises(M.MiOsqpError):
        M.debug_refactor_lanes([0], [0], 1, 1, 2, kbt=0)
