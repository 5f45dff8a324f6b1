"""GPU (-m gpu): run-ahead of the likely stragglers at a pipelined rho-update point ("Run-ahead").

With MI_OSQP_RUNAHEAD on, the tiles furthest from convergence leave the pipelined region and run their refactorisation and
the segments behind it as a chain on the solve stream beside the lanes, without a host turn; whoever the chain leaves
unfinished goes on alone once everyone else is done.  No arithmetic changes - every QP sees the same kernels on the same data in the same
order - so every case runs MI_OSQP_RUNAHEAD=0 and 1 and asks that both agree BIT FOR BIT in x, y, the exit codes, the
iteration counts, the rho updates and the polish status, and that last_solve_stats() reports the same refactorisations.
stats()["runahead_regions"] / ["runahead_tiles"] tell that the form ran, ["runahead_left"] that members went on behind
their chain.  The batches are the small dense-tail ones of tests/test_gpu_refactor_lanes.py (one QP per tile), with
MI_OSQP_REFACTOR_PIPELINE_MIN and MI_OSQP_RUNAHEAD_MIN lowered and groups of a few tiles; what the group will hold is
predicted from the oracle's residuals with the same group function."""
import numpy as np
import pytest

import osqp_solver_amd as M
from oracle import oracle as O
from osqp_solver_amd import problems as PR

pytestmark = pytest.mark.gpu
SMALL = dict(n=96, mg=64, nnz_per_row=6)
KW50 = dict(eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=50)      # nearly every QP updates rho at iteration 50
KW25 = dict(eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=25)      # two thirds of the QPs update rho at iteration 25


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _env(monkeypatch, tiles, longer_than=4, chunk_qps=7, end=None):
    monkeypatch.setenv("MI_OSQP_TILE", "1")
    monkeypatch.setenv("MI_OSQP_REFACTOR_PIPELINE_MIN", str(longer_than))
    monkeypatch.setenv("MI_OSQP_REFACTOR_CHUNKS", "0")
    monkeypatch.setenv("MI_OSQP_REFACTOR_CHUNK_QPS", str(chunk_qps))
    monkeypatch.setenv("MI_OSQP_RUNAHEAD_MIN", "4")
    monkeypatch.setenv("MI_OSQP_RUNAHEAD_TILES", str(tiles))
    if end is None:
        monkeypatch.delenv("MI_OSQP_RUNAHEAD_END", raising=False)
    else:
        monkeypatch.setenv("MI_OSQP_RUNAHEAD_END", str(end))


def _solve(s):
    info = s.solve()
    return info, s.primal().copy(), s.dual().copy(), s.last_solve_stats()


def _both(monkeypatch, pr, run, tiles, **kw):
    """run(solver) -> list of (info, x, y, last_solve_stats), with run-ahead off and on.  Returns (the list of the run with
    run-ahead on, its stats()) after the bitwise comparison."""
    out, st = {}, {}
    for on in (0, 1):
        monkeypatch.setenv("MI_OSQP_RUNAHEAD", str(on))
        s = _solver(pr, **kw)
        out[on] = run(s)
        st[on] = s.stats()
        print(f"run-ahead {on}: " + ", ".join(f"{k} {st[on][k]}" for k in ("pipelined_refactors", "refactor_lanes", "runahead_regions",
                                                                      "runahead_tiles", "runahead_left", "runahead_missed")))
    assert st[0]["pipelined_refactors"] >= 1 and st[0]["runahead_regions"] == 0 and st[0]["runahead_tiles"] == 0, st[0]
    assert st[1]["runahead_regions"] >= 1 and st[1]["runahead_tiles"] == tiles * st[1]["runahead_regions"], st[1]
    assert st[1]["refactor_lanes"] <= 2
    assert len(out[0]) == len(out[1])
    for k, ((i0, x0, y0, l0), (i1, x1, y1, l1)) in enumerate(zip(out[0], out[1])):
        assert [i.iter for i in i0] == [i.iter for i in i1], k
        assert [i.exit_code for i in i0] == [i.exit_code for i in i1], k
        assert [i.rho_updates for i in i0] == [i.rho_updates for i in i1], k
        assert [i.status_polish for i in i0] == [i.status_polish for i in i1], k
        np.testing.assert_array_equal(x0, x1, err_msg=f"x of solve {k}")
        np.testing.assert_array_equal(y0, y1, err_msg=f"y of solve {k}")
        if l0 is not None:
            assert l0["total_iters"] == l1["total_iters"] and l0["refactors"] == l1["refactors"], (k, l0, l1)
    return out[1], st[1]


def _oracle(pr, b, **kw):
    P, A = PR.qp_matrices(pr, b)
    return O.OracleQPSolver(P, pr["q"][b], A, pr["l"][b], pr["u"][b], **kw)


def _predicted_group(pr, B, at, size, **kw):
    """The group the oracle's residuals at iteration `at` give, and per QP (updates rho at `at`, iterations, rho updates)."""
    act, pri, dua, per = [], [], [], {}
    for b in range(B):
        o = _oracle(pr, b, **dict(kw, max_iter=at))
        st, _ = o.solve()
        i = o.info()
        full = _oracle(pr, b, **kw)
        full.solve()
        per[b] = (i.rho_updates >= 1, full.info().iter, full.info().rho_updates)
        # running behind the check of `at`: at max_iter the oracle reports -2 / 2 - or, where the rho update of that very
        # iteration loses the inertia, -7 with the update counted and the residuals of that check
        if st in (-2, 2) or (st == -7 and i.iter == at and i.rho_updates >= 1 and max(i.pri_res, i.dua_res) < 1e30):
            act.append(b); pri.append(i.pri_res); dua.append(i.dua_res)
    group = M.debug_runahead_group(act, pri, dua, size, 4)
    print(f"predicted group at iteration {at}: {group}; (flagged, iterations, rho updates): {[per[t] for t in group]}")
    return group, per


def test_group_of_flagged_and_unflagged_tiles_and_leftovers_behind_the_chain(monkeypatch):
    """Rho interval 25: the group of iteration 25 holds tiles that update rho there and tiles that do not; its chain ends at
    iteration 75 with members that need 100, which go on alone; a QP outside the group needs 175 iterations."""
    _env(monkeypatch, 6)
    B = 41
    pr = PR.random_box_qp(B, **SMALL)
    group, per = _predicted_group(pr, B, 25, 6, **KW25)
    assert {per[t][0] for t in group} == {True, False}            # the construction holds
    assert any(per[t][1] > 75 for t in group) and any(per[b][1] > 100 for b in range(B) if b not in group)
    (res,), st = _both(monkeypatch, pr, lambda s: [_solve(s)], 6, **KW25)
    assert [i.iter for i in res[0]] == [per[b][1] for b in range(B)]
    assert st["runahead_regions"] == 1 and st["runahead_left"] >= 1 and st["runahead_missed"] >= 1, st


def test_second_rho_update_inside_the_chain(monkeypatch):
    """Rho interval 50: the chain of iteration 50 runs to 150 over the rho-update point 100, where a member changes rho again:
    its refactorisation comes from the work list built on the device."""
    _env(monkeypatch, 6)
    B = 41
    pr = PR.random_box_qp(B, **SMALL)
    group, per = _predicted_group(pr, B, 50, 6, **KW50)
    assert any(per[t][2] >= 2 and per[t][1] > 100 for t in group)  # the construction holds
    (res,), st = _both(monkeypatch, pr, lambda s: [_solve(s)], 6, **KW50)
    assert [i.rho_updates for i in res[0]] == [per[b][2] for b in range(B)]
    assert [i.iter for i in res[0]] == [per[b][1] for b in range(B)]
    assert st["runahead_left"] == 0, st                            # every member finishes by iteration 150


def test_chain_cut_after_one_segment(monkeypatch):
    """MI_OSQP_RUNAHEAD_END=1: the chain ends with the region, at iteration 75; all its members go on with the host loop."""
    _env(monkeypatch, 6, end=1)
    B = 41
    pr = PR.random_box_qp(B, **SMALL)
    (res,), st = _both(monkeypatch, pr, lambda s: [_solve(s)], 6, **KW50)
    assert st["runahead_left"] == 6, st
    assert all(i.status_val == 1 for i in res[0])


@pytest.mark.parametrize("max_iter", [120, 100])
def test_max_iter_inside_the_chain(monkeypatch, max_iter):
    """The chain ends at max_iter - 120: between two checks; 100: on a rho-update point, where a member that changes rho ends
    finished AND flagged, and the host refactors it at that iteration."""
    _env(monkeypatch, 6)
    B = 41
    pr = PR.random_box_qp(B, **SMALL)
    (res,), st = _both(monkeypatch, pr, lambda s: [_solve(s)], 6, **dict(KW50, max_iter=max_iter))
    assert max(i.iter for i in res[0]) == max_iter
    assert any(i.exit_code != 0 for i in res[0])                   # someone ran into max_iter
    assert st["runahead_left"] == 0, st


def _pin_with_negative_curvature(pr, b, S):
    """QP b gets x_0 pinned (l_0 = u_0: row 0 of A = [I; G] becomes an equality, rho_vec = 1e3 rho) and P_00 -= S.  Without
    scaling its KKT matrix keeps its inertia while 1e3 rho outweighs S and loses it in the refactorisation that brings rho below
    S / 1e3 - with finite residuals at the check in front of it, so the QP is still running and asks for that refactorisation."""
    Pp = pr["P"]
    diag = np.flatnonzero(Pp.indices == np.repeat(np.arange(Pp.shape[1]), np.diff(Pp.indptr)))
    pr["Px"][b][diag[0]] -= S
    pr["l"][b][0] = pr["u"][b][0] = 0.5 * (pr["l"][b][0] + pr["u"][b][0])


# (settings, the QP, S, the iteration of the refactorisation that fails, the rho updates it has counted by then)
INERTIA = {"first": (dict(eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=25, rho=100.0, scaling=0), 8, 20000.0, 25, 1),
           "inside": (dict(eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=50, rho=3.0, scaling=0), 12, 900.0, 100, 2)}


@pytest.mark.parametrize("where", ["first", "inside"])
def test_a_member_loses_its_inertia_in_the_chains_refactorisation(monkeypatch, where):
    """A member of the group whose refactorisation fails - "first": the chain's first one, at the rho-update point that sends
    the group ahead; "inside": the one from the device-built work list at the rho-update point inside the chain.  The QP is
    running at the check in front (the oracle ends it kNonConvex AT the rho update, having counted it, with finite residuals)
    and is a member of the group the oracle's residuals predict.  The chain ends it there - kNonConvex at that iteration, NaN
    x and y - every other QP is bit for bit that of MI_OSQP_RUNAHEAD=0, and the second solve ends it at iteration 0: the host
    has learnt of the failure from the chain's marks."""
    kw, bad, S, at, updates = INERTIA[where]
    _env(monkeypatch, 6, longer_than=1, chunk_qps=5)
    B = 24
    pr = PR.random_box_qp(B, **SMALL)
    _pin_with_negative_curvature(pr, bad, S)
    o = _oracle(pr, bad, **kw)
    st, _ = o.solve()
    i = o.info()
    print(f"oracle: status {st} at iteration {i.iter}, {i.rho_updates} rho updates, pri_res {i.pri_res:.3g}, dua_res {i.dua_res:.3g}")
    assert st == -7 and i.iter == at and i.rho_updates == updates and max(i.pri_res, i.dua_res) < 1e20      # the construction holds
    group, per = _predicted_group(pr, B, kw["adaptive_rho_interval"], 6, **kw)
    assert bad in group, (bad, group)                              # ... and the QP runs ahead
    (r1, r2), st = _both(monkeypatch, pr, lambda s: [_solve(s), _solve(s)], 6, **kw)
    for info, x, y, _ in (r1, r2):
        assert info[bad].status_val == -7 and info[bad].exit_code == 9
        assert np.all(np.isnan(x[bad])) and np.all(np.isnan(y[bad]))
        assert all(info[b].status_val == 1 for b in range(B) if b != bad)
    assert r1[0][bad].iter == at and r1[0][bad].rho_updates == updates
    assert r2[0][bad].iter == 0


def test_warm_second_solve_and_reset_then_solve(monkeypatch):
    _env(monkeypatch, 6, chunk_qps=8)
    B = 26
    pr = PR.random_box_qp(B, **SMALL)

    def run(s):
        r = [_solve(s), _solve(s)]
        s.reset()
        r.append(_solve(s))
        return r
    res, _ = _both(monkeypatch, pr, run, 6, **KW50)
    assert [i.iter for i in res[0][0]] == [i.iter for i in res[2][0]]
    np.testing.assert_array_equal(res[0][1], res[2][1])
    np.testing.assert_array_equal(res[0][2], res[2][2])


def test_solve_on_the_callers_stream_followed_by_work_on_it(monkeypatch):
    """solve_device on a stream of the caller: the chain runs on it, the lanes fork from it and join it behind the chain."""
    import torch
    _env(monkeypatch, 6)
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
        return [(info, s.primal().copy(), s.dual().copy(), None)]
    _both(monkeypatch, pr, run, 6, **KW50)


def test_polish_behind_a_solve_that_ran_ahead(monkeypatch):
    _env(monkeypatch, 6)
    B = 29
    pr = PR.random_box_qp(B, **SMALL)
    (res,), _ = _both(monkeypatch, pr, lambda s: [_solve(s)], 6, **dict(KW50, polish=1))
    assert any(i.status_polish == 1 for i in res[0])
