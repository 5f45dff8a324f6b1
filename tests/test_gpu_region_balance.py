"""GPU (-m gpu): the region of a pipelined rho-update point beside a run-ahead chain ("Pipelined
refactorisation" / "Run-ahead").

MI_OSQP_REGION_PRIORITY = 1 creates the chunk lanes at the least stream priority, = 2 runs the chain on a stream of its own at
the greatest; MI_OSQP_LANE_CHECKS = 1 lets every lane fail and check its own chunks, so that only the flag copy follows the
join; without MI_OSQP_REFACTOR_CHUNKS / _CHUNK_QPS the chunk size counts the chain's refactorisation in the first round
(mi_osqp_debug_region_chunks).  None of it changes arithmetic - every QP sees the same kernels on the same data in the same
order - so every case compares against the run with both switches at 0 and asks that x, y, the exit codes, the iteration
counts, the rho updates, the polish status and last_solve_stats() agree BIT FOR BIT; stats()["region_priority"] /
["region_lane_checks"] / ["region_chunks"] tell the form of the last region.  The batches are the small dense-tail ones of
tests/test_gpu_runahead.py (one QP per tile, MI_OSQP_REFACTOR_PIPELINE_MIN and MI_OSQP_RUNAHEAD_MIN lowered, groups of six)."""
import numpy as np
import pytest

import osqp_solver_amd as M
from oracle import oracle as O
from osqp_solver_amd import problems as PR

pytestmark = pytest.mark.gpu
SMALL = dict(n=96, mg=64, nnz_per_row=6)
KW50 = dict(eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=50)      # nearly every QP updates rho at iteration 50
TILES = 6
FORMS = [(p, c) for p in (0, 1, 2) for c in (0, 1)]                    # (MI_OSQP_REGION_PRIORITY, MI_OSQP_LANE_CHECKS)
ON = [(0, 1), (2, 1)]                                                  # the forms of the cases the lanes' own checks can get wrong


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _env(monkeypatch, form, longer_than=4, chunk_qps=7, runahead=1, cus=None, tiles=TILES):
    monkeypatch.setenv("MI_OSQP_TILE", "1")
    monkeypatch.setenv("MI_OSQP_REFACTOR_PIPELINE_MIN", str(longer_than))
    monkeypatch.setenv("MI_OSQP_RUNAHEAD", str(runahead))
    monkeypatch.setenv("MI_OSQP_RUNAHEAD_MIN", "4")
    monkeypatch.setenv("MI_OSQP_RUNAHEAD_TILES", str(tiles))
    monkeypatch.delenv("MI_OSQP_RUNAHEAD_END", raising=False)
    monkeypatch.delenv("MI_OSQP_REFACTOR_LANES", raising=False)
    monkeypatch.delenv("MI_OSQP_REFACTOR_CHUNK0", raising=False)
    if chunk_qps is None:       # the default chunk rule
        monkeypatch.delenv("MI_OSQP_REFACTOR_CHUNKS", raising=False)
        monkeypatch.delenv("MI_OSQP_REFACTOR_CHUNK_QPS", raising=False)
    else:
        monkeypatch.setenv("MI_OSQP_REFACTOR_CHUNKS", "0")
        monkeypatch.setenv("MI_OSQP_REFACTOR_CHUNK_QPS", str(chunk_qps))
    if cus is None:
        monkeypatch.delenv("MI_OSQP_ASSUME_CUS", raising=False)
    else:
        monkeypatch.setenv("MI_OSQP_ASSUME_CUS", str(cus))
    monkeypatch.setenv("MI_OSQP_REGION_PRIORITY", str(form[0]))
    monkeypatch.setenv("MI_OSQP_LANE_CHECKS", str(form[1]))


def _solve(s):
    info = s.solve()
    return info, s.primal().copy(), s.dual().copy(), s.last_solve_stats()


def _same(ref, got, what=""):
    """Lists of (info, x, y, last_solve_stats): bit for bit the same solves."""
    assert len(ref) == len(got)
    for k, ((i0, x0, y0, l0), (i1, x1, y1, l1)) in enumerate(zip(ref, got)):
        for f in ("iter", "exit_code", "status_val", "rho_updates", "status_polish"):
            assert [getattr(i, f) for i in i0] == [getattr(i, f) for i in i1], (what, k, f)
        np.testing.assert_array_equal(x0, x1, err_msg=f"{what}: x of solve {k}")
        np.testing.assert_array_equal(y0, y1, err_msg=f"{what}: y of solve {k}")
        if l0 is not None:
            assert l0["total_iters"] == l1["total_iters"] and l0["refactors"] == l1["refactors"], (what, k, l0, l1)


def _says(st, form, runahead=True):
    print(", ".join(f"{k} {st[k]}" for k in ("pipelined_refactors", "refactor_lanes", "runahead_regions", "runahead_tiles", "region_priority",
                                              "region_lane_checks", "region_chunks")))
    assert st["pipelined_refactors"] >= 1 and st["region_chunks"] >= 1, st
    assert (st["runahead_regions"] >= 1) == runahead, st
    assert (st["region_priority"], st["region_lane_checks"]) == form, st


def _against_zero(monkeypatch, pr, run, form, env=None, **kw):
    """run(solver) -> list of (info, x, y, last_solve_stats) with both switches at 0 and in `form`; returns the latter and its
    stats() after the bitwise comparison."""
    out = {}
    for f in ((0, 0), form):
        _env(monkeypatch, f, **(env or {}))
        s = _solver(pr, **kw)
        out[f] = run(s)
        st = s.stats()
        _says(st, f)
        s.__del__()
    _same(out[(0, 0)], out[form], f"form {form}")
    return out[form], st


# ---- every form against the run with both switches at 0
_matrix = {}


def _matrix_run(monkeypatch, form):
    if form not in _matrix:
        _env(monkeypatch, form)
        s = _solver(PR.random_box_qp(41, **SMALL), **KW50)
        _matrix[form] = ([_solve(s)], s.stats())
        s.__del__()
    return _matrix[form]


@pytest.mark.parametrize("form", FORMS)
def test_every_form_is_bit_for_bit_the_run_with_both_switches_off(monkeypatch, form):
    """Rho interval 50, 41 QPs: the region of iteration 50 runs beside a chain that refactors again at iteration 100."""
    ref, st0 = _matrix_run(monkeypatch, (0, 0))
    got, st = _matrix_run(monkeypatch, form)
    _says(st0, (0, 0))
    _says(st, form)
    _same(ref, got, f"form {form}")
    assert st["region_chunks"] == st0["region_chunks"] and st["refactor_lanes"] == st0["refactor_lanes"] == 2
    assert max(i.iter for i in got[0][0]) > 100 and all(i.status_val == 1 for i in got[0][0])


# ---- the default chunk rule
def _oracle(pr, b, **kw):
    P, A = PR.qp_matrices(pr, b)
    return O.OracleQPSolver(P, pr["q"][b], A, pr["l"][b], pr["u"][b], **kw)


def _at_the_check_of(pr, B, at, **kw):
    """From the oracle, behind the check of iteration `at`: the running QPs in descending run-ahead score, and who of them
    updates rho there."""
    act, pri, dua, flagged = [], [], [], set()
    for b in range(B):
        o = _oracle(pr, b, **dict(kw, max_iter=at))
        st, _ = o.solve()
        i = o.info()
        if st in (-2, 2) or (st == -7 and i.iter == at and i.rho_updates >= 1 and max(i.pri_res, i.dua_res) < 1e30):
            act.append(b); pri.append(i.pri_res); dua.append(i.dua_res)
            if i.rho_updates >= 1:
                flagged.add(b)
    return M.debug_runahead_group(act, pri, dua, len(act), 4), flagged


def test_default_chunks_count_the_chains_refactorisation(monkeypatch):
    """Neither MI_OSQP_REFACTOR_CHUNKS nor _CHUNK_QPS, MI_OSQP_ASSUME_CUS = 8, max_iter 100: the one region of the solve, at
    iteration 50, takes the chunks mi_osqp_debug_region_chunks gives for its work list, the group's flagged QPs and 8 CUs -
    and run-ahead on and off agree bit for bit."""
    B, cus = 41, 8
    pr = PR.random_box_qp(B, **SMALL)
    kw = dict(KW50, max_iter=100)
    ranked, flagged = _at_the_check_of(pr, B, 50, **KW50)
    gw = len(flagged & set(ranked[:TILES]))
    assert 1 <= gw and len(flagged) - gw > 4 and len(ranked) > TILES           # the construction holds: both have work
    out, chunks = {}, {}
    for on in (0, 1):
        _env(monkeypatch, (0, 0), chunk_qps=None, runahead=on, cus=cus)
        s = _solver(pr, **kw)
        out[on] = [_solve(s)]
        st = s.stats()
        _says(st, (0, 0), runahead=bool(on))
        assert st["pipelined_refactors"] == 1, st
        chunks[on] = st["region_chunks"]
        s.__del__()
    _same(out[0], out[1], "run-ahead")
    assert chunks[0] == M.debug_region_chunks(len(flagged), 0, cus)[1] > 1
    assert chunks[1] == M.debug_region_chunks(len(flagged) - gw, gw, cus)[1] > 1
    print(f"{len(flagged)} flagged QPs, {gw} of them in the group: {chunks[0]} chunks without the chain, {chunks[1]} beside it")


# ---- what the lanes' own checks can get wrong
@pytest.mark.parametrize("form", ON)
def test_max_iter_at_the_regions_last_iteration(monkeypatch, form):
    """max_iter = 100 = the end of the region's segment: the lanes' checks end the QPs still running there, and those that
    change rho at iteration 100 end finished AND flagged - the host refactors them."""
    pr = PR.random_box_qp(41, **SMALL)
    (res,), st = _against_zero(monkeypatch, pr, lambda s: [_solve(s)], form, **dict(KW50, max_iter=100))
    assert max(i.iter for i in res[0]) == 100 and any(i.exit_code != 0 for i in res[0])
    assert st["pipelined_refactors"] == 1, st


def _pin_with_negative_curvature(pr, b, S):
    """QP b gets x_0 pinned (l_0 = u_0: row 0 of A = [I; G] becomes an equality, rho_vec = 1e3 rho) and P_00 -= S.  Without
    scaling its KKT matrix keeps its inertia while 1e3 rho outweighs S and loses it in the refactorisation that brings rho below
    S / 1e3 - with finite residuals at the check in front of it, so the QP is still running and asks for that refactorisation."""
    Pp = pr["P"]
    diag = np.flatnonzero(Pp.indices == np.repeat(np.arange(Pp.shape[1]), np.diff(Pp.indptr)))
    pr["Px"][b][diag[0]] -= S
    pr["l"][b][0] = pr["u"][b][0] = 0.5 * (pr["l"][b][0] + pr["u"][b][0])


INERTIA = dict(eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=25, rho=100.0, scaling=0)


@pytest.mark.parametrize("form", ON)
def test_a_qp_of_the_region_loses_its_inertia(monkeypatch, form):
    """The construction of tests/test_gpu_runahead.py (a pinned x_0 with negative curvature: the refactorisation of iteration
    25 loses the inertia), with six other QPs scaled so that they score above that QP and it stays in the region: the
    lane that refactors its chunk fails it in front of the chunk's iterate and check.  kNonConvex at iteration 25 with one
    rho update counted, NaN x and y that no iterate touched, and at iteration 0 of the second solve."""
    B, bad, S, at = 24, 8, 20000.0, 25
    pr = PR.random_box_qp(B, **SMALL)
    _pin_with_negative_curvature(pr, bad, S)
    for b in range(TILES):          # q, l, u and with them the residuals of six other QPs times 1000: they score above the pinned QP
        pr["q"][b] *= 1e3; pr["l"][b] *= 1e3; pr["u"][b] *= 1e3
    o = _oracle(pr, bad, **INERTIA)
    st, _ = o.solve()
    i = o.info()
    assert st == -7 and i.iter == at and i.rho_updates == 1 and max(i.pri_res, i.dua_res) < 1e20      # the construction holds
    ranked, flagged = _at_the_check_of(pr, B, at, **INERTIA)
    print(f"QP {bad} is number {ranked.index(bad)} of {len(ranked)} running QPs by score; {len(flagged)} update rho")
    assert bad in flagged and sorted(ranked[:TILES]) == list(range(TILES))                            # ... and the QP stays in the region
    (r1, r2), stats = _against_zero(monkeypatch, pr, lambda s: [_solve(s), _solve(s)], form, env=dict(longer_than=1, chunk_qps=5), **INERTIA)
    assert stats["runahead_tiles"] == TILES * stats["runahead_regions"], stats
    for info, x, y, _ in (r1, r2):
        assert info[bad].status_val == -7 and info[bad].exit_code == 9
        assert np.all(np.isnan(x[bad])) and np.all(np.isnan(y[bad]))
        assert all(info[b].status_val == 1 for b in range(B) if b != bad)
    assert r1[0][bad].iter == at and r1[0][bad].rho_updates == 1
    assert r2[0][bad].iter == 0


@pytest.mark.parametrize("form", ON)
def test_warm_second_solve_and_reset_then_solve(monkeypatch, form):
    pr = PR.random_box_qp(26, **SMALL)

    def run(s):
        r = [_solve(s), _solve(s)]
        s.reset()
        r.append(_solve(s))
        return r
    res, _ = _against_zero(monkeypatch, pr, run, form, env=dict(chunk_qps=8), **KW50)
    assert [i.iter for i in res[0][0]] == [i.iter for i in res[2][0]]
    np.testing.assert_array_equal(res[0][1], res[2][1])
    np.testing.assert_array_equal(res[0][2], res[2][2])


@pytest.mark.parametrize("form", ON)
def test_solve_on_the_callers_stream_followed_by_work_on_it(monkeypatch, form):
    """solve_device on a stream of the caller: lanes (and the chain's stream) fork from it and join it; what the caller
    enqueues behind the solve reads the x of the lanes' own checks."""
    import torch
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
    _against_zero(monkeypatch, pr, run, form, **KW50)


@pytest.mark.parametrize("form", ON)
def test_polish_behind_a_solve_whose_lanes_checked(monkeypatch, form):
    pr = PR.random_box_qp(29, **SMALL)
    (res,), _ = _against_zero(monkeypatch, pr, lambda s: [_solve(s)], form, **dict(KW50, polish=1))
    assert any(i.status_polish == 1 for i in res[0])


# ---- pooled streams keep the priority they were created with
def test_a_handle_never_gets_pooled_lanes_of_another_priority(monkeypatch):
    """Handles one after the other, each closed before the next is set up (its streams go to the pool and come back), with
    MI_OSQP_REGION_PRIORITY 1, 2, 0, 1, 0: every solve is that of the run with both switches at 0 on fresh streams, and every
    handle reports its own form."""
    ref, _ = _matrix_run(monkeypatch, (0, 0))
    pr = PR.random_box_qp(41, **SMALL)
    for prio in (1, 2, 0, 1, 0):
        _env(monkeypatch, (prio, 0))
        s = _solver(pr, **KW50)
        got = [_solve(s)]
        _says(s.stats(), (prio, 0))
        s.__del__()
        _same(ref, got, f"priority {prio} behind another handle")
