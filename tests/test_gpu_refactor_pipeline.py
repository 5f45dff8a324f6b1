"""GPU (-m gpu): the pipelined refactorisation at a rho-update point ("Pipelined refactorisation").

A work list longer than the CU count is refactored in chunks on one stream while the tiles whose factors are written already
run the next segment's iterations on a second stream; MI_OSQP_REFACTOR_PIPELINE=0 / 1 (read at setup) selects the serial form
- every factor first, then one iterate launch - or the pipelined one.  No arithmetic changes, so every case asks for two things:
  * the two forms agree BIT FOR BIT in x, y, the iteration counts, the exit codes, the rho updates and the polish status;
  * the pipelined form meets the oracle by the project's usual criteria (tests/test_gpu_parity.py): same exit code, same
    iteration count, x within 1e-6 (large batches: a sample of QPs spread over the batch - the oracle runs on the host).
stats()["pipelined_refactors"] tells whether a rho-update point took the pipelined form.  The small cases lower the
threshold (MI_OSQP_REFACTOR_PIPELINE_MIN) and set the chunk size (MI_OSQP_REFACTOR_CHUNK_QPS with MI_OSQP_REFACTOR_CHUNKS=0);
their pattern is below the size at which a short work list shares a QP between workgroups, so both forms run the same
factor_kernel form."""
import numpy as np
import pytest

import osqp_solver_amd as M
from oracle import oracle as O
from osqp_solver_amd import problems as PR

pytestmark = pytest.mark.gpu
TOL_X = 1e-6
ST2EXIT = {1: 0, -3: 1, -4: 2, 2: 3, 3: 4, 4: 5, -2: 6, -7: 9, -10: 10}
SMALL = dict(n=96, mg=64, nnz_per_row=6)
KW50 = dict(eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=50)      # nearly every QP of the small pattern updates rho at iteration 50


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _small_chunks(monkeypatch, longer_than, chunk_qps):
    monkeypatch.setenv("MI_OSQP_REFACTOR_PIPELINE_MIN", str(longer_than))
    monkeypatch.setenv("MI_OSQP_REFACTOR_CHUNKS", "0")
    monkeypatch.setenv("MI_OSQP_REFACTOR_CHUNK_QPS", str(chunk_qps))


def _both_forms(monkeypatch, pr, run, **kw):
    """run(solver) -> list of (info, x, y), once per form; returns the pipelined form's list after the bitwise comparison."""
    out = {}
    for form in ("serial", "pipelined"):
        monkeypatch.setenv("MI_OSQP_REFACTOR_PIPELINE", "0" if form == "serial" else "1")
        s = _solver(pr, **kw)
        out[form] = run(s)
        n_pipe = s.stats()["pipelined_refactors"]
        print(f"{form}: {n_pipe} pipelined rho-update points")
        assert (n_pipe >= 1) if form == "pipelined" else (n_pipe == 0), (form, n_pipe)
    assert len(out["serial"]) == len(out["pipelined"])
    for k, ((i0, x0, y0), (i1, x1, y1)) in enumerate(zip(out["serial"], out["pipelined"])):
        assert [i.iter for i in i0] == [i.iter for i in i1], k
        assert [i.exit_code for i in i0] == [i.exit_code for i in i1], k
        assert [i.rho_updates for i in i0] == [i.rho_updates for i in i1], k
        assert [i.status_polish for i in i0] == [i.status_polish for i in i1], k
        np.testing.assert_array_equal(x0, x1, err_msg=f"x of solve {k}")
        np.testing.assert_array_equal(y0, y1, err_msg=f"y of solve {k}")
    return out["pipelined"]


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


def _sample(B, k=8):
    return sorted(set(np.linspace(0, B - 1, k).astype(int).tolist()))


def test_config3_batch_at_the_default_threshold(monkeypatch):
    """n = 512, m = 1024 (config 3), 512 QPs: more than half of them pass iteration 100 and change rho there - a work list
    longer than the CU count, cut by the default chunking; the QPs that finish before iteration 100 never see it."""
    B = 512
    pr = PR.random_box_qp(B)
    (info, x, y), = _both_forms(monkeypatch, pr, lambda s: [_solve(s)])
    n_upd = sum(i.rho_updates >= 1 and i.iter > 100 for i in info)
    print("QPs that refactored and went on:", n_upd)
    assert n_upd > 256 and any(i.iter <= 100 for i in info)
    for b in _sample(B):
        o = _oracle(pr, b)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())
        assert info[b].rho_updates == o.info().rho_updates


def test_work_list_that_does_not_divide_into_the_chunks(monkeypatch):
    """41 QPs in chunks of 7: a last chunk of another length (and work lists of other lengths at the later rho updates)."""
    _small_chunks(monkeypatch, 4, 7)
    monkeypatch.setenv("MI_OSQP_TILE", "1")
    B = 41
    pr = PR.random_box_qp(B, **SMALL)
    (info, x, y), = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], **KW50)
    n_flagged = 0
    for b in range(B):
        o = _oracle(pr, b, **KW50)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())
        assert info[b].rho_updates == o.info().rho_updates
        o50 = _oracle(pr, b, **dict(KW50, max_iter=50))
        o50.solve()
        n_flagged += o50.info().rho_updates >= 1
    print("QPs that change rho at iteration 50:", n_flagged)
    assert n_flagged > 7 and n_flagged % 7 != 0, n_flagged


def test_two_qps_per_tile_where_only_one_is_flagged(monkeypatch):
    """MI_OSQP_TILE=2, no dense tail: tiles of which one QP changes rho at iteration 50 while its neighbour iterates on with
    its old factor - the tile waits for the chunk of the flagged one."""
    _small_chunks(monkeypatch, 4, 5)
    monkeypatch.setenv("MI_OSQP_TILE", "2")
    monkeypatch.setenv("MI_OSQP_DENSE_TAIL", "0")
    B = 24
    pr = PR.random_box_qp(B, **SMALL)
    seen = {}

    def run(s):
        seen.update(s.stats())
        return [_solve(s)]
    (info, x, y), = _both_forms(monkeypatch, pr, run, **KW50)
    assert seen["tile"] == 2 and seen["dense_tail_rows"] == 0, seen
    flagged_at_50 = []
    for b in range(B):
        o = _oracle(pr, b, **KW50)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())
        assert info[b].rho_updates == o.info().rho_updates
        o50 = _oracle(pr, b, **dict(KW50, max_iter=50))
        o50.solve()
        flagged_at_50.append(o50.info().rho_updates >= 1)
    mixed = [t for t in range(B // 2) if flagged_at_50[2 * t] != flagged_at_50[2 * t + 1] and min(info[2 * t].iter, info[2 * t + 1].iter) > 50]
    print("tiles with one flagged QP at iteration 50:", mixed)
    assert mixed


def test_streaming_state_form(monkeypatch):
    """MI_OSQP_STREAM_STATE=1: the iterate that streams the ADMM state from global memory takes the tile list as well."""
    _small_chunks(monkeypatch, 4, 9)
    monkeypatch.setenv("MI_OSQP_STREAM_STATE", "1")
    B = 30
    pr = PR.random_box_qp(B, **SMALL)
    seen = {}

    def run(s):
        seen.update(s.stats())
        return [_solve(s)]
    (info, x, y), = _both_forms(monkeypatch, pr, run, **KW50)
    assert seen["resident_state"] == 0
    for b in range(B):
        o = _oracle(pr, b, **KW50)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())


def test_warm_second_solve_and_reset_then_solve(monkeypatch):
    """The second solve starts from the iterates and factors the pipelined region left; after a reset the first solve repeats
    bit for bit."""
    _small_chunks(monkeypatch, 4, 8)
    B = 26
    pr = PR.random_box_qp(B, **SMALL)

    def run(s):
        r = [_solve(s), _solve(s)]
        s.reset()
        r.append(_solve(s))
        return r
    res = _both_forms(monkeypatch, pr, run, **KW50)
    assert [i.iter for i in res[0][0]] == [i.iter for i in res[2][0]]
    np.testing.assert_array_equal(res[0][1], res[2][1])
    np.testing.assert_array_equal(res[0][2], res[2][2])
    for b in range(B):
        o = _oracle(pr, b, **KW50)
        for k in range(2):
            st, xo = o.solve()
            _meets_oracle(res[k][0], res[k][1], b, st, xo, o.info())


def test_handle_with_polishing(monkeypatch):
    """polish = 1: the polish refactorisation keeps the serial form; the ADMM loop before it is pipelined.  The oracle does
    not polish: both sides run to 1e-8, where the polished and the plain solution agree far within 1e-6."""
    _small_chunks(monkeypatch, 4, 6)
    B = 20
    pr = PR.random_box_qp(B, **SMALL)
    kw = dict(eps_abs=1e-8, eps_rel=1e-8, adaptive_rho_interval=50)
    (info, x, y), = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], polish=1, **kw)
    assert any(i.status_polish == 1 for i in info), [i.status_polish for i in info]
    for b in range(B):
        o = _oracle(pr, b, **kw)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())


def test_one_qp_loses_its_inertia_at_the_rho_update(monkeypatch):
    """As tests/test_gpu_multi.py isolates a QP with an indefinite P - here P is indefinite only so far that the KKT matrix
    keeps its inertia at rho = 0.1 and loses it with the smaller rho of iteration 50 (the oracle: kNonConvex at iteration
    50).  That QP sits in a pipelined chunk: its tile must not iterate on the half-written factor, it ends kNonConvex with
    a NaN solution at iteration 50, and every other QP is bit for bit the serial form's."""
    _small_chunks(monkeypatch, 4, 5)
    B, bad = 24, 2
    pr = PR.random_box_qp(B, **SMALL)
    Pp = pr["P"]
    diag = Pp.indices == np.repeat(np.arange(Pp.shape[1]), np.diff(Pp.indptr))
    pr["Px"][bad][diag] -= 1.32
    (info, x, y), = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], **KW50)
    for b in range(B):
        o = _oracle(pr, b, **KW50)
        st, xo = o.solve()
        if b == bad:
            assert st == -7 and o.info().iter == 50                      # the construction holds
            assert info[b].status_val == -7 and info[b].exit_code == 9 and info[b].iter == 50
            assert np.all(np.isnan(x[b])) and np.all(np.isnan(y[b]))
        _meets_oracle(info, x, b, st, xo, o.info())


def test_solve_on_the_callers_stream_followed_by_work_on_it(monkeypatch):
    """solve_device on a stream of the caller: the two internal streams fork from it and join it again, so a kernel the
    caller enqueues behind the solve reads the final d_x without any synchronisation of its own."""
    import torch
    _small_chunks(monkeypatch, 4, 7)
    B = 33
    pr = PR.random_box_qp(B, **SMALL)

    def run(s):
        st = torch.cuda.Stream()
        d_x = torch.zeros(B, pr["n"], dtype=torch.float64, device="cuda")
        d_status = torch.zeros(B, dtype=torch.int32, device="cuda"); d_iters = torch.zeros_like(d_status)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            s.solve_device(d_x, d_status, d_iters, stream=st.cuda_stream)
            twice = d_x * 2.0
        st.synchronize()
        info = s.info()
        assert d_iters.cpu().tolist() == [i.iter for i in info]
        np.testing.assert_array_equal(d_x.cpu().numpy(), s.primal())
        np.testing.assert_array_equal(twice.cpu().numpy(), 2.0 * s.primal())
        return [(info, s.primal().copy(), s.dual().copy())]
    (info, x, y), = _both_forms(monkeypatch, pr, run, **KW50)
    for b in range(B):
        o = _oracle(pr, b, **KW50)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())
