"""Host only: the default chunk size of a pipelined region (host_core.hpp region_chunk_qps, through
mi_osqp_debug_region_chunks).  nq flagged QPs in the region's work list, gw flagged QPs of the run-ahead chain that refactors
beside it, n_cus CUs: with rounds = ceil((nq + gw) / n_cus), n_even = rounds (gw = 0) or 2 rounds - 1 (gw > 0) even chunks -
at most kPipeChunks = 8 and at most nq - of ceil(nq / n_even) QPs.  Without a chain that is the rule the region had before
there was one."""
import pytest

import osqp_solver_amd as M

K_PIPE_CHUNKS = 8


def _ceil(a, b):
    return -(-a // b)


def _rule(nq, gw, n_cus):
    rounds = _ceil(nq + gw, n_cus)
    n_even = max(1, min(2 * rounds - 1 if gw > 0 else rounds, K_PIPE_CHUNKS, max(1, nq)))
    return max(1, _ceil(nq, n_even))


# (nq, n_cus) -> QPs per chunk; the headline batch without and with the group's 107 flagged QPs taken out
PARENT = [((605, 256), 202), ((496, 256), 248), ((1, 256), 1), ((256, 256), 256), ((257, 256), 129), ((512, 256), 256),
          ((513, 256), 171), ((1024, 256), 256), ((2048, 256), 256), ((41, 8), 7), ((41, 16), 14), ((32, 4), 4), ((7, 1), 1),
          ((100, 304), 100), ((700, 304), 234)]


@pytest.mark.parametrize("case, want", PARENT)
def test_without_a_chain_it_is_the_fewest_even_chunks_of_one_qp_per_cu(case, want):
    nq, n_cus = case
    q, k = M.debug_region_chunks(nq, 0, n_cus)
    assert q == _ceil(nq, _ceil(nq, n_cus)) == want
    assert k == _ceil(nq, q)


def test_beside_a_chain_twice_the_rounds_less_one():
    assert M.debug_region_chunks(496, 107, 256) == (100, 5)          # the headline batch: three rounds, 4 x 100 + 96
    assert M.debug_region_chunks(496, 16, 256) == (166, 3)           # 512 workgroups: two rounds
    assert M.debug_region_chunks(496, 17, 256) == (100, 5)
    assert M.debug_region_chunks(200, 107, 256) == (67, 3)
    assert M.debug_region_chunks(200, 56, 256) == (200, 1)           # one round: one chunk
    assert M.debug_region_chunks(1200, 107, 256) == (150, 8)         # six rounds: eleven chunks asked, eight given
    for nq in (1, 2, 5, 41, 255, 256, 257, 496, 605, 1024, 5000):
        for gw in (1, 6, 107, 128, 256, 3000):
            for n_cus in (1, 4, 8, 64, 256, 304):
                q, k = M.debug_region_chunks(nq, gw, n_cus)
                assert q == _rule(nq, gw, n_cus), (nq, gw, n_cus)
                assert k == _ceil(nq, q)


def test_never_more_than_the_events_hold_and_never_an_empty_chunk():
    assert M.debug_region_chunks(33, 0, 4) == (5, 7)          # nine rounds: eight chunks of ceil(33 / 8), as refactor_chunks cut them before
    for nq in list(range(0, 70)) + [255, 256, 257, 2047, 2048, 2049, 100000, 2 ** 31 - 1]:
        for gw in (0, 1, 107, 100000):
            for n_cus in (1, 2, 3, 8, 256):
                q, k = M.debug_region_chunks(nq, gw, n_cus)
                assert q >= 1 and k <= K_PIPE_CHUNKS, (nq, gw, n_cus, q, k)
                assert k == _ceil(nq, q) and (k - 1) * q < max(nq, 1), (nq, gw, n_cus, q, k)       # the last chunk holds a QP
                work, _ = M.debug_refactor_chunks(list(range(min(nq, 300))), [], 1, q) if nq <= 300 else ([], None)
                assert all(len(w) >= 1 for w in work[1:])


def test_bad_arguments():
    with pytest.raises(M.MiOsqpError):
        M.debug_region_chunks(-1, 0, 8)
    with pytest.raises(M.MiOsqpError):
        M.debug_region_chunks(8, -1, 8)
    with pytest.raises(M.MiOsqpError):
        M.debug_region_chunks(8, 0, 0)
