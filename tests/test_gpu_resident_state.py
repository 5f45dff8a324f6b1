"""GPU (-m gpu): the resident form of the iterate ("Resident state").

Where the ADMM state of a tile (x, q, z, y, rho_inv, rho_vec, l, u) and D^-1 fit LDS beside the solve vector, iterate_kernel
loads them once per segment and stores x, z, y after the segment's last iteration; MI_OSQP_STREAM_STATE=1 (read at setup)
keeps the form that streams them from global memory in every iteration.  Both forms evaluate the same expressions in the
same order, so every case asks for two things:
  * the two forms agree BIT FOR BIT in x, y, the iteration counts and the exit codes;
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


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _both_forms(monkeypatch, pr, run, expect_resident=1, **kw):
    """run(solver) -> list of (info, x, y), once per form; returns the resident form's list after the bitwise comparison."""
    out = {}
    for form in ("streamed", "resident"):
        if form == "streamed":
            monkeypatch.setenv("MI_OSQP_STREAM_STATE", "1")
        else:
            monkeypatch.delenv("MI_OSQP_STREAM_STATE", raising=False)
        s = _solver(pr, **kw)
        st = s.stats()
        assert st["resident_state"] == (expect_resident if form == "resident" else 0), (form, st)
        if st["resident_state"]:
            assert st["lds_bytes_iterate"] == st["lds_bytes"] + 8 * st["tile"] * (2 * st["n"] + 6 * st["m"] + st["N"])
            assert st["lds_bytes_iterate"] <= 159 * 1024 and st["threads_per_block"] == 1024
        else:
            assert st["lds_bytes_iterate"] == st["lds_bytes"]
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


def test_headline_shape_fits_and_refactors_at_iteration_100(monkeypatch):
    """n = 512, m = 1024 (config 3): the state fits; adaptive_rho is on, the QPs that pass iteration 100 get a new rho there
    and with it new rho_vec / rho_inv / D^-1, which the next segment must pick up."""
    B = 6
    pr = PR.random_box_qp(B)
    (info, x, y), = _both_forms(monkeypatch, pr, lambda s: [_solve(s)])
    assert any(i.rho_updates >= 1 and i.iter > 100 for i in info), [(i.iter, i.rho_updates) for i in info]
    for b in range(B):
        o = _oracle(pr, b)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())
        assert info[b].rho_updates == o.info().rho_updates


def test_gomp_shape_does_not_fit_and_keeps_the_streaming_form(monkeypatch):
    """7 DOF x 100 waypoints (config 4: 2n + 6m + N = 41 k doubles per QP): no room, today's kernel."""
    B = 3
    pr = PR.gomp_batch(B, 7, 100)

    def run(s):
        s.warm_start_x(pr["warm"])
        return [_solve(s)]
    (info, x, y), = _both_forms(monkeypatch, pr, run, expect_resident=0)
    for b in (0, B - 1):
        o = _oracle(pr, b)
        o.set_warm_start(pr["warm"][b])
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())


def test_two_qps_per_tile_finishing_in_different_segments(monkeypatch):
    """MI_OSQP_TILE=2: the QP of a tile that has finished keeps its x / z / y while its neighbour iterates on - the second,
    warm-started solve continues from exactly those iterates, z included."""
    monkeypatch.setenv("MI_OSQP_TILE", "2")
    B = 8
    pr = PR.random_box_qp(B, n=96, mg=64, nnz_per_row=6)
    kw = dict(eps_abs=1e-6, eps_rel=1e-6)
    r1, r2 = _both_forms(monkeypatch, pr, lambda s: [_solve(s), _solve(s)], **kw)
    info, x, y = r1
    seg = [(i.iter + 24) // 25 for i in info]
    assert any(seg[2 * t] != seg[2 * t + 1] for t in range(B // 2)), [i.iter for i in info]
    for b in range(B):
        o = _oracle(pr, b, **kw)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())
        np.testing.assert_allclose(y[b], o.y, atol=1e-5)
        st, xo = o.solve()
        _meets_oracle(r2[0], r2[1], b, st, xo, o.info())


def test_max_iter_that_is_no_multiple_of_the_check_interval(monkeypatch):
    """max_iter = 30, check_termination = 25: a segment of 25 and one of 5 iterations."""
    B = 4
    pr = PR.random_box_qp(B)
    kw = dict(max_iter=30, eps_abs=1e-10, eps_rel=1e-10)
    (info, x, y), = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], **kw)
    assert all(i.iter == 30 for i in info)
    for b in range(B):
        o = _oracle(pr, b, **kw)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())


def test_warm_second_solve_and_bounds_updated_on_the_device_between_solves(monkeypatch):
    """The second solve starts from the stored x, z, y; new bounds written by update_bounds_device reach the next segment."""
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
    """polish = 1: the ADMM loop of such a handle runs the resident form, the polish kernels keep their LDS size.  The oracle
    does not polish: both sides run to 1e-8, where the polished and the plain solution agree far within 1e-6."""
    B = 4
    pr = PR.random_box_qp(B, n=96, mg=64, nnz_per_row=6)
    kw = dict(eps_abs=1e-8, eps_rel=1e-8)
    (info, x, y), = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], polish=1, **kw)
    assert any(i.status_polish == 1 for i in info), [i.status_polish for i in info]
    for b in range(B):
        o = _oracle(pr, b, **kw)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())
