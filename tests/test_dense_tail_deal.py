"""CPU: the deal of the dense-tail product's tasks over the waves of a tile (host_core.cpp build_dense_tail).

The tasks of all phases are dealt round robin, every phase starting where the one before it ended, so that they spread
over the waves as evenly as they can.  For tails of k rows forced (MI_OSQP_DENSE_TAIL) on patterns large enough to hold
them, laid out for 8 and for 16 waves per tile (MI_OSQP_THREADS), the host entry of tests/test_host_schedule.py
(mi_osqp_debug_host_kkt_solve) must
  * accept the schedule in its replay (which fails on two tasks of a phase that collide, on a wave that does not pass every
    phase barrier and on a task nobody runs) and reproduce the direct solve,
  * report min(nw, tasks) waves with at least one task and no wave with more than ceil(tasks / nw) tasks,
  * stream k * k / 2 slots."""
import numpy as np
import pytest

import osqp_solver_amd as M
from osqp_solver_amd import problems as PR


def _n_tasks(k):
    nb = k // 64
    return nb * (nb + 1) // 2          # the 64 x 64 blocks I >= J of the k x k matrix


@pytest.mark.parametrize("nw", [8, 16])
@pytest.mark.parametrize("k", [64, 128, 256, 448, 512])
def test_forced_tail_is_dealt_evenly_and_replays(k, nw, monkeypatch):
    monkeypatch.setenv("MI_OSQP_DENSE_TAIL", str(k))
    monkeypatch.setenv("MI_OSQP_THREADS", str(64 * nw))
    # the pattern tests/test_host_schedule.py forces its tails on; N = 2676 takes every size up to 512 (config 3 picks 448 by
    # itself but refuses small forced tails: too many entries of L left in the tail rows for tail_kernel's 16-bit tables)
    P, (l, A, u), _ = PR.gomp_qp(6, 50, np.zeros(6), np.ones(6))
    n, m = A.shape[1], A.shape[0]
    rhs = np.random.default_rng(11).standard_normal(n + m)
    s_sched, s_direct, st = M.debug_host_kkt_solve(P, A, l, u, rhs)      # raises when the replay refuses
    assert np.max(np.abs(s_sched - s_direct)) <= 1e-8 * np.max(np.abs(s_direct))
    assert st["threads_per_block"] == 64 * nw
    assert st["dense_tail_rows"] == k
    tasks = _n_tasks(k)
    print(f"k {k} nw {nw}: tasks {st['dense_tail_tasks']}, waves used {st['dense_tail_waves_used']}, "
          f"most per wave {st['dense_tail_wave_tasks_max']}, slots {st['dense_tail_slots']}")
    assert st["dense_tail_tasks"] == tasks
    assert st["dense_tail_waves_used"] == min(nw, tasks)
    assert st["dense_tail_wave_tasks_max"] <= -(-tasks // nw)
    assert st["dense_tail_slots"] == k * k // 2
