"""GPU (-m gpu): the resident head of S^-1 in the resident iterate ("Resident head of S^-1").

A tile of one QP that keeps its ADMM state in LDS and has a dense tail also keeps the first steps of every wave's first
product task of the S^-1 stream in registers and LDS across the iterations of a launch; MI_OSQP_STREAM_FACTOR=1 (read at
setup) keeps the form that streams all of S^-1 in every iteration.  Both forms evaluate the same sums in the same order, so
every case builds the solver twice and asks for two things:
  * the two forms agree BIT FOR BIT in x, y, the iteration counts, the exit codes and the rho updates;
  * the resident form meets the oracle by the project's usual criteria (tests/test_gpu_parity.py): same exit code, same
    iteration count, x within 1e-6."""
import numpy as np
import pytest

import osqp_solver_amd as M
from oracle import oracle as O
from osqp_solver_amd import problems as PR

pytestmark = pytest.mark.gpu
TOL_X = 1e-6
ST2EXIT = {1: 0, -3: 1, -4: 2, 2: 3, 3: 4, 4: 5, -2: 6, -7: 9, -10: 10}
SMALL = dict(n=96, mg=64, nnz_per_row=6)


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _both_forms(monkeypatch, pr, run, expect_head=True, **kw):
    """run(solver) -> list of (info, x, y), once per form; returns the resident form's list after the bitwise comparison."""
    out = {}
    for form in ("streamed", "resident"):
        if form == "streamed":
            monkeypatch.setenv("MI_OSQP_STREAM_FACTOR", "1")
        else:
            monkeypatch.delenv("MI_OSQP_STREAM_FACTOR", raising=False)
        s = _solver(pr, **kw)
        st = s.stats()
        print(form, {k: st[k] for k in ("tile", "threads_per_block", "dense_tail_rows", "dense_tail_tasks", "dense_tail_waves_used",
                                        "resident_state", "lds_bytes_iterate", "resident_factor_steps", "lds_bytes_factor")})
        if form == "resident" and expect_head:
            assert st["resident_factor_steps"] > 0 and st["lds_bytes_factor"] > 0, st
            assert st["resident_state"] == 1 and st["tile"] == 1 and st["dense_tail_rows"] > 0 and st["threads_per_block"] == 1024
            assert st["lds_bytes_iterate"] == st["lds_bytes"] + 8 * (2 * st["n"] + 6 * st["m"] + st["N"])
            assert st["lds_bytes_iterate"] + st["lds_bytes_factor"] <= 159 * 1024
        else:
            assert st["resident_factor_steps"] == 0 and st["lds_bytes_factor"] == 0, (form, st)
        out[form] = run(s)
    assert len(out["streamed"]) == len(out["resident"])
    for k, ((i0, x0, y0), (i1, x1, y1)) in enumerate(zip(out["streamed"], out["resident"])):
        assert [i.iter for i in i0] == [i.iter for i in i1], k
        assert [i.exit_code for i in i0] == [i.exit_code for i in i1], k
        assert [i.rho_updates for i in i0] == [i.rho_updates for i in i1], k
        assert [i.status_polish for i in i0] == [i.status_polish for i in i1], k
        np.testing.assert_array_equal(x0, x1, err_msg=f"x of solve {k}")
        np.testing.assert_array_equal(y0, y1, err_msg=f"y of solve {k}")
    return out["resident"]


def _solve(s):
    info = s.solve()
    return info, s.primal().copy(), s.dual().copy()


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


def test_headline_shape_keeps_a_head_and_refactors_at_iteration_100(monkeypatch):
    """n = 512, m = 1024 (config 3, dense tail of 448 rows: 28 tasks on 16 waves): the QPs that pass iteration 100 get a new
    rho and a new S^-1 there, which the head of the next launch must pick up."""
    B = 6
    pr = PR.random_box_qp(B)
    (info, x, y), = _both_forms(monkeypatch, pr, lambda s: [_solve(s)])
    assert any(i.rho_updates >= 1 and i.iter > 100 for i in info), [(i.iter, i.rho_updates) for i in info]
    for b in range(B):
        o = _oracle(pr, b)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())
        assert info[b].rho_updates == o.info().rho_updates


@pytest.mark.parametrize("k", [64, 128, 256, 512])
def test_forced_tails(k, monkeypatch):
    """MI_OSQP_DENSE_TAIL = k: 1, 3, 10 and 36 tasks - fewer tasks than waves (waves without a task keep nothing), first
    tasks that are diagonal blocks of 32 steps (the head is the whole task) and waves with three tasks.  The random box
    pattern tests/test_host_schedule.py forces its tails on, at a size (N = 640) that holds 512 tail rows."""
    monkeypatch.setenv("MI_OSQP_DENSE_TAIL", str(k))
    B = 4
    pr = PR.random_box_qp(B, n=256, mg=128, nnz_per_row=6)
    seen = {}

    def run(s):
        seen.update(s.stats())
        return [_solve(s)]
    (info, x, y), = _both_forms(monkeypatch, pr, run)
    assert seen["dense_tail_rows"] == k
    for b in range(B):
        o = _oracle(pr, b)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())


def test_one_qp_loses_its_inertia_at_the_rho_update(monkeypatch):
    """The construction of tests/test_gpu_refactor_pipeline.py: P of one QP is indefinite only so far that the KKT matrix keeps
    its inertia at rho = 0.1 and loses it with the smaller rho of iteration 50.  That QP's launches get null descriptors
    (its head is zeros), it ends kNonConvex (-7) with a NaN solution; the healthy QPs next to it stay bitwise equal."""
    monkeypatch.setenv("MI_OSQP_DENSE_TAIL", "64")
    kw = dict(eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=50)
    B, bad = 6, 2
    pr = PR.random_box_qp(B, **SMALL)
    Pp = pr["P"]
    diag = Pp.indices == np.repeat(np.arange(Pp.shape[1]), np.diff(Pp.indptr))
    pr["Px"][bad][diag] -= 1.32
    (info, x, y), = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], **kw)
    for b in range(B):
        o = _oracle(pr, b, **kw)
        st, xo = o.solve()
        if b == bad:
            assert st == -7 and o.info().iter == 50                      # the construction holds
            assert info[b].status_val == -7 and info[b].exit_code == 9 and info[b].iter == 50
            assert np.all(np.isnan(x[b])) and np.all(np.isnan(y[b]))
        _meets_oracle(info, x, b, st, xo, o.info())


@pytest.mark.parametrize("max_iter", [30, 26])
def test_max_iter_that_is_no_multiple_of_the_check_interval(max_iter, monkeypatch):
    """max_iter = 30: launches of 25 and 5 iterations; max_iter = 26: the second launch has ONE iteration, which loads the
    head and never reuses it."""
    B = 4
    pr = PR.random_box_qp(B)
    kw = dict(max_iter=max_iter, eps_abs=1e-10, eps_rel=1e-10)
    (info, x, y), = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], **kw)
    assert all(i.iter == max_iter for i in info)
    for b in range(B):
        o = _oracle(pr, b, **kw)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())


def test_warm_second_solve_and_bounds_updated_on_the_device_between_solves(monkeypatch):
    import torch
    B = 5
    pr = PR.random_box_qp(B)
    l2, u2 = pr["l"] * 0.8, pr["u"] * 0.7

    def run(s):
        r = [_solve(s), _solve(s)]
        s.update_bounds_device(torch.tensor(l2, device="cuda"), torch.tensor(u2, device="cuda"))
        r.append(_solve(s))
        return r
    res = _both_forms(monkeypatch, pr, run)
    assert not np.array_equal(res[1][1], res[2][1])
    for b in range(B):
        o = _oracle(pr, b)
        for k in range(3):
            if k == 2:
                o.update_bounds_only(l2[b], u2[b])
            st, xo = o.solve()
            _meets_oracle(res[k][0], res[k][1], b, st, xo, o.info())


def test_handle_with_polishing(monkeypatch):
    """polish = 1 on a small handle with a forced tail: the ADMM loop keeps the head, the polish kernels keep their form.  The
    oracle does not polish: both sides run to 1e-8, where the polished and the plain solution agree far within 1e-6."""
    monkeypatch.setenv("MI_OSQP_DENSE_TAIL", "64")
    B = 4
    pr = PR.random_box_qp(B, **SMALL)
    kw = dict(eps_abs=1e-8, eps_rel=1e-8)
    (info, x, y), = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], polish=1, **kw)
    assert any(i.status_polish == 1 for i in info), [i.status_polish for i in info]
    for b in range(B):
        o = _oracle(pr, b, **kw)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())


def test_two_qps_per_tile_keep_the_streaming_form(monkeypatch):
    """MI_OSQP_TILE=2: the head exists for tiles of one QP only."""
    monkeypatch.setenv("MI_OSQP_TILE", "2")
    monkeypatch.setenv("MI_OSQP_DENSE_TAIL", "64")
    B = 8
    pr = PR.random_box_qp(B, **SMALL)
    kw = dict(eps_abs=1e-6, eps_rel=1e-6)
    (info, x, y), = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], expect_head=False, **kw)
    for b in range(B):
        o = _oracle(pr, b, **kw)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())


def test_streamed_state_has_no_head(monkeypatch):
    """MI_OSQP_STREAM_STATE=1 with the default factor setting: no resident state, so no resident head."""
    monkeypatch.setenv("MI_OSQP_STREAM_STATE", "1")
    B = 3
    pr = PR.random_box_qp(B)
    (info, x, y), = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], expect_head=False)
    for b in range(B):
        o = _oracle(pr, b)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())
