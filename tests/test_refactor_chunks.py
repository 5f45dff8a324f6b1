"""CPU: the chunking of a pipelined refactorisation (host_core.hpp refactor_chunks, DESIGN.md section 3 "Pipelined
refactorisation").  The flagged QPs of a rho-update point are refactored chunk after chunk while the tiles of earlier chunks
already iterate, so for every input:
  * every active tile is in exactly one chunk;
  * no tile comes before the chunk of its LAST flagged QP (the tile would iterate on a factor not yet written);
  * chunk 0 - which starts at once - holds exactly the active tiles without a flagged QP;
  * the refactorisation chunks partition the flagged QPs in order, chunk 0 refactors nothing."""
import numpy as np
import pytest

import osqp_solver_amd as M


def _check(flagged, active, bt, chunk_qps, max_chunks=8):
    work, tiles = M.debug_refactor_chunks(flagged, active, bt, chunk_qps, max_chunks)
    assert len(work) == len(tiles) and 1 <= len(work) <= max_chunks + 1
    assert work[0] == []
    assert [q for w in work for q in w] == list(flagged)                      # a partition, in order
    assert all(len(w) > 0 for w in work[1:])
    if len(work) > 2:                                                          # even chunks, the last takes the remainder
        assert len({len(w) for w in work[1:-1]}) == 1 and len(work[-1]) <= len(work[1])
        assert len(work[1]) >= chunk_qps
    chunk_of_qp = {q: c for c, w in enumerate(work) for q in w}
    active_tiles = sorted({q // bt for q in active})
    assert sorted(t for tl in tiles for t in tl) == active_tiles               # exactly one chunk each
    for c, tl in enumerate(tiles):
        assert tl == sorted(tl)
        for t in tl:
            need = [chunk_of_qp[q] for q in range(t * bt, (t + 1) * bt) if q in chunk_of_qp]
            assert c == (max(need) if need else 0), (t, c, need)              # not before its last flagged QP - and not later
    flagged_tiles = {q // bt for q in flagged}
    assert tiles[0] == [t for t in active_tiles if t not in flagged_tiles]
    return work, tiles


@pytest.mark.parametrize("bt", [1, 2, 4])
@pytest.mark.parametrize("chunk_qps", [1, 3, 7, 256, 10 ** 6])
def test_random_flags(bt, chunk_qps):
    rng = np.random.default_rng(100 * bt + chunk_qps % 97)
    for n_slots in (1, 5, 64, 1024, 1030):
        for p_act, p_flag in ((1.0, 0.6), (0.6, 0.6), (0.3, 0.05), (0.9, 1.0), (0.5, 0.0)):
            act = rng.random(n_slots) < p_act
            flg = (rng.random(n_slots) < p_flag) & (act | (rng.random(n_slots) < 0.02))   # a few finished at max_iter and flagged
            _check(np.flatnonzero(flg).tolist(), np.flatnonzero(act).tolist(), bt, chunk_qps)


def test_headline_shape():
    """605 flagged of 634 active QPs, one QP per tile, chunks of 256: 256 + 256 + 93, and 29 tiles start at once."""
    rng = np.random.default_rng(7)
    active = np.sort(rng.choice(1024, 634, replace=False))
    flagged = np.sort(rng.choice(active, 605, replace=False))
    work, tiles = _check(flagged.tolist(), active.tolist(), 1, 256)
    assert [len(w) for w in work] == [0, 256, 256, 93] and [len(t) for t in tiles] == [29, 256, 256, 93]
    work, tiles = _check(flagged.tolist(), active.tolist(), 1, (605 + 2) // 3)
    assert [len(w) for w in work] == [0, 202, 202, 201]


def test_tile_of_two_with_one_flagged_qp_and_a_tile_split_over_chunks():
    # tile 0: QP 0 flagged, QP 1 not; tile 1: both flagged, the chunk border between them; tile 2: none; tile 3: QP 7 only
    work, tiles = _check([0, 2, 3, 7], [0, 1, 2, 3, 4, 5, 7], 2, 2)
    assert work == [[], [0, 2], [3, 7]] and tiles == [[2], [0], [1, 3]]


def test_more_chunks_than_allowed_grow_the_chunk():
    work, tiles = _check(list(range(100)), list(range(100)), 1, 3, max_chunks=8)
    assert len(work) == 9 and len(work[1]) == 13


def test_bad_arguments_are_refused():
    with pytest.raises(M.MiOsqpError):
        M.debug_refactor_chunks([0], [0], 0, 1)
    with pytest.raises(M.MiOsqpError):
        M.debug_refactor_chunks([0], [0], 1, 0)
