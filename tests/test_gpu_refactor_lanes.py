"""GPU (-m gpu): chunk lanes of the pipelined refactorisation ("Pipelined refactorisation").

MI_OSQP_REFACTOR_LANES = 1 .. 3 (read at setup): with one lane the refactorisation chunks run on one stream and the chunk
iterates on a second one; with more, every lane is a stream that runs factor -> tail -> iterate of its own chunks, chunks of
different lanes side by side on scratch of their own, and a tile whose flagged QPs sit on different lanes waits for both.
No arithmetic changes, so every case runs the serial form (MI_OSQP_REFACTOR_PIPELINE=0) and lanes 1, 2, 3 and asks that
all four agree BIT FOR BIT in x, y, the iteration counts, the exit codes, the rho updates and the polish status.
stats()["pipelined_refactors"] tells whether a rho-update point took the pipelined form, stats()["refactor_lanes"] the most
lanes one of them ran on: what was asked for, or the number of refactorisation chunks where there are fewer.
The shapes are those of tests/test_gpu_refactor_pipeline.py (its pattern stays below the size at which a short work list
shares a QP between workgroups, so all forms run the same factor_kernel form); one case meets the oracle by the project's
usual criteria (same exit code, same iteration count, x within 1e-6)."""
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
FORMS = ("serial", 1, 2, 3)


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _small_chunks(monkeypatch, longer_than, chunk_qps):
    monkeypatch.setenv("MI_OSQP_REFACTOR_PIPELINE_MIN", str(longer_than))
    monkeypatch.setenv("MI_OSQP_REFACTOR_CHUNKS", "0")
    monkeypatch.setenv("MI_OSQP_REFACTOR_CHUNK_QPS", str(chunk_qps))


def _all_forms(monkeypatch, pr, run, max_chunks, **kw):
    """run(solver) -> list of (info, x, y), once per form; max_chunks: the most refactorisation chunks of a rho-update point of
    this case.  Returns the three-lane form's list after the bitwise comparison with the serial form."""
    out = {}
    for form in FORMS:
        monkeypatch.setenv("MI_OSQP_REFACTOR_PIPELINE", "0" if form == "serial" else "1")
        monkeypatch.setenv("MI_OSQP_REFACTOR_LANES", "1" if form == "serial" else str(form))
        s = _solver(pr, **kw)
        out[form] = run(s)
        st = s.stats()
        print(f"{form}: {st['pipelined_refactors']} pipelined rho-update points on up to {st['refactor_lanes']} lanes")
        if form == "serial":
            assert st["pipelined_refactors"] == 0 and st["refactor_lanes"] == 0, st
        else:
            assert st["pipelined_refactors"] >= 1 and st["refactor_lanes"] == min(form, max_chunks), (form, st)
    for form in FORMS[1:]:
        assert len(out["serial"]) == len(out[form])
        for k, ((i0, x0, y0), (i1, x1, y1)) in enumerate(zip(out["serial"], out[form])):
            assert [i.iter for i in i0] == [i.iter for i in i1], (form, k)
            assert [i.exit_code for i in i0] == [i.exit_code for i in i1], (form, k)
            assert [i.rho_updates for i in i0] == [i.rho_updates for i in i1], (form, k)
            assert [i.status_polish for i in i0] == [i.status_polish for i in i1], (form, k)
            np.testing.assert_array_equal(x0, x1, err_msg=f"x of solve {k}, lanes {form}")
            np.testing.assert_array_equal(y0, y1, err_msg=f"y of solve {k}, lanes {form}")
    return out[3]


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


def _state_at_50(pr, B):
    """(flagged, active) at the first rho-update point, from the oracle: the QPs that change rho at iteration 50 / go on after it."""
    flagged, active = [], []
    for b in range(B):
        o50 = _oracle(pr, b, **dict(KW50, max_iter=50))
        st, _ = o50.solve()
        if o50.info().rho_updates >= 1:
            flagged.append(b)
        if st == -2:
            active.append(b)
    return flagged, active


def test_more_chunks_than_lanes(monkeypatch):
    """41 QPs in chunks of 7: six chunks at iteration 50, so every lane runs several chains one after the other on the scratch
    of their own chunks; the work lists of the later rho updates have other lengths.  Meets the oracle."""
    _small_chunks(monkeypatch, 4, 7)
    monkeypatch.setenv("MI_OSQP_TILE", "1")
    B = 41
    pr = PR.random_box_qp(B, **SMALL)
    flagged, active = _state_at_50(pr, B)
    print("QPs that change rho at iteration 50:", len(flagged))
    assert len(flagged) > 5 * 7
    (info, x, y), = _all_forms(monkeypatch, pr, lambda s: [_solve(s)], 6, **KW50)
    for b in range(B):
        o = _oracle(pr, b, **KW50)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())
        assert info[b].rho_updates == o.info().rho_updates


def test_fewer_chunks_than_lanes(monkeypatch):
    """9 QPs in chunks of 7: two chunks - the third lane stays unused."""
    _small_chunks(monkeypatch, 4, 7)
    B = 9
    pr = PR.random_box_qp(B, **SMALL)
    flagged, _ = _state_at_50(pr, B)
    assert 7 < len(flagged) <= 9, flagged
    _all_forms(monkeypatch, pr, lambda s: [_solve(s)], 2, **KW50)


def test_tile_of_two_with_flagged_qps_on_different_lanes(monkeypatch):
    """MI_OSQP_TILE=2, no dense tail, chunks of 5: a tile whose two flagged QPs sit in neighbouring chunks - on different lanes -
    iterates only behind both tails (a cross-lane wait of the lane function)."""
    _small_chunks(monkeypatch, 4, 5)
    monkeypatch.setenv("MI_OSQP_TILE", "2")
    monkeypatch.setenv("MI_OSQP_DENSE_TAIL", "0")
    B = 24
    pr = PR.random_box_qp(B, **SMALL)
    flagged, active = _state_at_50(pr, B)
    work, _ = M.debug_refactor_chunks(flagged, active, 2, 5)
    for lanes in (2, 3):
        rl = M.debug_refactor_lanes(flagged, active, 2, 5, lanes, kbt=1)
        print(f"lanes {lanes}: order {rl['order']}, cross-lane waits {rl['waits']}")
        assert rl["n_lanes"] == lanes and rl["waits"], rl
    seen = {}

    def run(s):
        seen.update(s.stats())
        return [_solve(s)]
    (info, x, y), = _all_forms(monkeypatch, pr, run, len(work) - 1, **KW50)
    assert seen["tile"] == 2 and seen["dense_tail_rows"] == 0, seen
    assert all(info[b].iter > 50 for b in active)


def test_dense_tail_with_one_qp_per_tile(monkeypatch):
    """MI_OSQP_TILE=1 and the default dense tail: tail_assemble_kernel / tail_kernel of chunks on different lanes keep their
    Schur complements at their own offsets."""
    _small_chunks(monkeypatch, 4, 6)
    monkeypatch.setenv("MI_OSQP_TILE", "1")
    B = 29
    pr = PR.random_box_qp(B, **SMALL)
    seen = {}

    def run(s):
        seen.update(s.stats())
        return [_solve(s)]
    flagged, _ = _state_at_50(pr, B)
    assert len(flagged) > 2 * 6
    _all_forms(monkeypatch, pr, run, (len(flagged) + 5) // 6, **KW50)
    assert seen["tile"] == 1 and seen["dense_tail_rows"] > 0, seen


def test_one_qp_loses_its_inertia_at_the_rho_update(monkeypatch):
    """The construction of tests/test_gpu_refactor_pipeline.py: QP 2 keeps its inertia at rho = 0.1 and loses it with the rho of
    iteration 50.  The device ends it there - kNonConvex at iteration 50, NaN x and y - every other QP is bit for bit the
    serial form's, and a second solve remembers it."""
    _small_chunks(monkeypatch, 4, 5)
    B, bad = 24, 2
    pr = PR.random_box_qp(B, **SMALL)
    Pp = pr["P"]
    diag = Pp.indices == np.repeat(np.arange(Pp.shape[1]), np.diff(Pp.indptr))
    pr["Px"][bad][diag] -= 1.32
    o = _oracle(pr, bad, **KW50)
    st, _ = o.solve()
    assert st == -7 and o.info().iter == 50                      # the construction holds
    (info, x, y), (info2, x2, y2) = _all_forms(monkeypatch, pr, lambda s: [_solve(s), _solve(s)], 5, **KW50)
    assert info[bad].status_val == -7 and info[bad].exit_code == 9 and info[bad].iter == 50
    assert np.all(np.isnan(x[bad])) and np.all(np.isnan(y[bad]))
    assert all(info[b].status_val == 1 for b in range(B) if b != bad)
    assert info2[bad].status_val == -7 and info2[bad].exit_code == 9      # (its iteration count: whatever the serial form reports)
    assert np.all(np.isnan(x2[bad])) and np.all(np.isnan(y2[bad]))
    assert all(info2[b].status_val == 1 for b in range(B) if b != bad)


def test_warm_second_solve_and_reset_then_solve(monkeypatch):
    """The second solve starts from the iterates and factors the lanes left; after a reset the first solve repeats bit for bit."""
    _small_chunks(monkeypatch, 4, 8)
    B = 26
    pr = PR.random_box_qp(B, **SMALL)

    def run(s):
        r = [_solve(s), _solve(s)]
        s.reset()
        r.append(_solve(s))
        return r
    res = _all_forms(monkeypatch, pr, run, 3, **KW50)
    assert [i.iter for i in res[0][0]] == [i.iter for i in res[2][0]]
    np.testing.assert_array_equal(res[0][1], res[2][1])
    np.testing.assert_array_equal(res[0][2], res[2][2])


def test_solve_on_the_callers_stream_followed_by_work_on_it(monkeypatch):
    """solve_device on a stream of the caller: the lanes fork from it and join it again, so a kernel the caller enqueues
    behind the solve reads the final d_x without any synchronisation of its own."""
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
    _all_forms(monkeypatch, pr, run, 4, **KW50)
