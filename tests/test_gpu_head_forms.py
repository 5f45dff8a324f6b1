"""GPU (-m gpu): the two forms of the resident head of S^-1 ("Resident head of S^-1").

An iterate launch of a handle with the head runs one of two instantiations of the kernel: the DEEP RING (8 register + 8 LDS
steps resident, a product ring of 16 steps) or the LONG HEAD (24 + 8 steps resident, a ring of 8).  host_core.hpp
iterate_form picks one per launch from the tiles the launch iterates; MI_OSQP_RF_FORM = 1 / 2 forces one for the whole
handle, MI_OSQP_RF_LONG_MIN sets the threshold (both read at setup).  All forms consume the stream in stream order with the
same fmas and rotations, so every case builds the solver once per form - streamed (MI_OSQP_STREAM_FACTOR=1), deep ring
forced, long head forced - and asks for
  * bitwise equal x, y, iteration counts, exit codes and rho updates between the three;
  * the long form's agreement with the oracle by the criteria of tests/test_gpu_resident_factor.py: same exit code, same
    iteration count, x within 1e-6."""
import functools

import numpy as np
import pytest

import osqp_solver_amd as M
from oracle import oracle as O
from osqp_solver_amd import problems as PR

pytestmark = pytest.mark.gpu
TOL_X = 1e-6
ST2EXIT = {1: 0, -3: 1, -4: 2, 2: 3, 3: 4, 4: 5, -2: 6, -7: 9, -10: 10}
SMALL = dict(n=96, mg=64, nnz_per_row=6)
HEAD_DEEP, HEAD_LONG = 16, 32
FORMS = {"streamed": {"MI_OSQP_STREAM_FACTOR": "1"}, "deep": {"MI_OSQP_RF_FORM": "1"}, "long": {"MI_OSQP_RF_FORM": "2"}}
SWITCHES = ("MI_OSQP_STREAM_FACTOR", "MI_OSQP_RF_FORM", "MI_OSQP_RF_LONG_MIN")


def _run(monkeypatch, pr, env, **kw):
    """One solver under `env` (on top of what the test has set): (info, x, y, stats after the solve)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)
    info = s.solve()
    st = s.stats()
    print(env, {k: st[k] for k in ("tile", "threads_per_block", "dense_tail_rows", "dense_tail_tasks", "dense_tail_waves_used",
                                   "dense_tail_wave_tasks_max", "resident_factor_steps", "lds_bytes_factor",
                                   "iterate_launches_deep_ring", "iterate_launches_long_head")})
    return info, s.primal().copy(), s.dual().copy(), st


def _same(a, b, what):
    (i0, x0, y0, _), (i1, x1, y1, _) = a, b
    assert [i.iter for i in i0] == [i.iter for i in i1], what
    assert [i.exit_code for i in i0] == [i.exit_code for i in i1], what
    assert [i.rho_updates for i in i0] == [i.rho_updates for i in i1], what
    np.testing.assert_array_equal(x0, x1, err_msg=f"x, {what}")
    np.testing.assert_array_equal(y0, y1, err_msg=f"y, {what}")


def _three_forms(monkeypatch, pr, **kw):
    """The three forced forms, compared bit for bit; returns the long form's result."""
    out = {f: _run(monkeypatch, pr, env, **kw) for f, env in FORMS.items()}
    st = {f: out[f][3] for f in out}
    assert st["streamed"]["resident_factor_steps"] == 0 and st["streamed"]["lds_bytes_factor"] == 0
    assert st["streamed"]["iterate_launches_deep_ring"] == 0 and st["streamed"]["iterate_launches_long_head"] == 0
    assert st["deep"]["resident_factor_steps"] == HEAD_DEEP and st["long"]["resident_factor_steps"] == HEAD_LONG
    assert st["deep"]["lds_bytes_factor"] == st["long"]["lds_bytes_factor"] == 16 * 8 * 64 * 8       # 16 waves x 8 steps x 512 B
    assert st["deep"]["iterate_launches_deep_ring"] > 0 and st["deep"]["iterate_launches_long_head"] == 0
    assert st["long"]["iterate_launches_long_head"] > 0 and st["long"]["iterate_launches_deep_ring"] == 0
    for f in ("deep", "long"):
        assert st[f]["resident_state"] == 1 and st[f]["tile"] == 1 and st[f]["threads_per_block"] == 1024
    _same(out["streamed"], out["deep"], "streamed against the deep ring")
    _same(out["streamed"], out["long"], "streamed against the long head")
    return out["long"]


@functools.lru_cache(maxsize=None)
def _headline(B):
    """The headline shape (n = 512, m = 1024) and its oracle solutions, computed once for the tests that use it."""
    pr = PR.random_box_qp(B)
    ref = []
    for b in range(B):
        P, A = PR.qp_matrices(pr, b)
        o = O.OracleQPSolver(P, pr["q"][b], A, pr["l"][b], pr["u"][b])
        st, xo = o.solve()
        ref.append((st, xo, o.info()))
    return pr, ref


def _oracle(pr, b, **kw):
    P, A = PR.qp_matrices(pr, b)
    return O.OracleQPSolver(P, None if pr["q"] is None else pr["q"][b], A, pr["l"][b], pr["u"][b], **kw)


def _meets_oracle(info, x, b, st, xo, io):
    print(f"QP {b}: status {info[b].status_val} / {st}, iter {info[b].iter} / {io.iter}, "
          f"|x - x_oracle| {np.max(np.abs(x[b] - xo)) if not np.any(np.isnan(xo)) else float('nan'):.3e}")
    assert info[b].status_val == st and info[b].exit_code == ST2EXIT[st], (b, info[b].status_val, st)
    assert info[b].iter == io.iter, (b, info[b].iter, io.iter)
    if np.any(np.isnan(xo)):
        assert np.all(np.isnan(x[b]))
    else:
        assert np.max(np.abs(x[b] - xo)) <= TOL_X, (b, np.max(np.abs(x[b] - xo)))


@pytest.mark.parametrize("k", [64, 128, 512])
def test_forced_tails(k, monkeypatch):
    """MI_OSQP_DENSE_TAIL = k on the random box pattern of tests/test_gpu_resident_factor.py: 1, 3 and 36 tasks.  One task:
    fifteen waves keep nothing.  First tasks that are 32-step diagonal blocks: the long head is the whole task - the flush
    comes before the ring starts, and a wave whose only task it is streams nothing after the first iteration - while the deep
    ring's head of 16 leaves one revolution of 16.  k = 512: waves with three tasks."""
    monkeypatch.setenv("MI_OSQP_DENSE_TAIL", str(k))
    B = 4
    pr = PR.random_box_qp(B, n=256, mg=128, nnz_per_row=6)
    info, x, y, st = _three_forms(monkeypatch, pr)
    assert st["dense_tail_rows"] == k
    assert st["dense_tail_tasks"] == {64: 1, 128: 3, 512: 36}[k]
    if k == 64:
        assert st["dense_tail_waves_used"] == 1
    if k == 512:
        assert st["dense_tail_wave_tasks_max"] >= 3
    for b in range(B):
        o = _oracle(pr, b)
        s, xo = o.solve()
        _meets_oracle(info, x, b, s, xo, o.info())


def test_headline_shape_refactors_at_iteration_100(monkeypatch):
    """n = 512, m = 1024, dense tail of 448 rows: the QPs that pass iteration 100 get a new rho and a new S^-1 there, which the
    head of the next launch - of either form - must pick up."""
    B = 6
    pr, ref = _headline(B)
    info, x, y, st = _three_forms(monkeypatch, pr)
    assert any(i.rho_updates >= 1 and i.iter > 100 for i in info), [(i.iter, i.rho_updates) for i in info]
    for b, (s, xo, io) in enumerate(ref):
        _meets_oracle(info, x, b, s, xo, io)
        assert info[b].rho_updates == io.rho_updates


def test_one_solve_changes_form_between_its_launches(monkeypatch):
    """MI_OSQP_RF_LONG_MIN = B: the launches in which every tile still iterates take the long head, the launches after the
    first QP has finished the deep ring.  Every launch reloads its head, so the result is bitwise that of either form alone."""
    B = 6
    pr, ref = _headline(B)
    mixed = _run(monkeypatch, pr, {"MI_OSQP_RF_LONG_MIN": str(B)})
    st = mixed[3]
    assert len({i.iter for i in mixed[0]}) > 1, [i.iter for i in mixed[0]]       # the QPs finish in different launches
    assert st["resident_factor_steps"] == HEAD_LONG
    assert st["iterate_launches_long_head"] > 0 and st["iterate_launches_deep_ring"] > 0, st
    _same(mixed, _run(monkeypatch, pr, FORMS["long"]), "mixed against the long head")
    _same(mixed, _run(monkeypatch, pr, FORMS["deep"]), "mixed against the deep ring")
    for b, (s, xo, io) in enumerate(ref):
        _meets_oracle(mixed[0], mixed[1], b, s, xo, io)


def test_one_qp_loses_its_inertia_at_the_rho_update(monkeypatch):
    """The construction of tests/test_gpu_resident_factor.py: P of one QP is indefinite only so far that the KKT matrix keeps
    its inertia at rho = 0.1 and loses it with the smaller rho of iteration 50.  That QP's launches get null descriptors
    (its head, 32 steps of it, is zeros), it ends kNonConvex (-7) with a NaN solution; the healthy QPs next to it stay
    bitwise equal in all three forms."""
    monkeypatch.setenv("MI_OSQP_DENSE_TAIL", "64")
    kw = dict(eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=50)
    B, bad = 6, 2
    pr = PR.random_box_qp(B, **SMALL)
    Pp = pr["P"]
    diag = Pp.indices == np.repeat(np.arange(Pp.shape[1]), np.diff(Pp.indptr))
    pr["Px"][bad][diag] -= 1.32
    info, x, y, st = _three_forms(monkeypatch, pr, **kw)
    for b in range(B):
        o = _oracle(pr, b, **kw)
        s, xo = o.solve()
        if b == bad:
            assert s == -7 and o.info().iter == 50                      # the construction holds
            assert info[b].status_val == -7 and info[b].exit_code == 9 and info[b].iter == 50
            assert np.all(np.isnan(x[b])) and np.all(np.isnan(y[b]))
        _meets_oracle(info, x, b, s, xo, o.info())
