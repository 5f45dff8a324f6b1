"""GPU (-m gpu): the index words of the resident iterate in registers ("Index words in registers").

A tile that keeps its ADMM state in LDS walks the same entries of pinv and xloc in every iteration; where a thread's trips
fit the caps (host_core.hpp index_words_fit) it loads them once per launch and keeps them, so that the D^-1 pass and the
vector step issue no global load.  MI_OSQP_INDEX_LOADS=1 (read at setup) keeps the form that loads them in every iteration.
The vector step has one source for both forms (kernels.hip x_step / zy_step), so every case builds the solver once per form
- loads, registers, registers with the deep ring of the resident head forced (MI_OSQP_RF_FORM=1) - and asks for:
  * the three forms agree BIT FOR BIT in x, y, the iteration counts, the exit codes and the rho updates;
  * the register form and the deep-ring form meet the oracle by the project's usual criteria (tests/test_gpu_parity.py):
    same exit code, same iteration count, x within 1e-6 (identical outputs: one comparison serves both)."""
import numpy as np
import pytest

import osqp_solver_amd as M
from oracle import oracle as O
from osqp_solver_amd import problems as PR

pytestmark = pytest.mark.gpu
TOL_X = 1e-6
ST2EXIT = {1: 0, -3: 1, -4: 2, 2: 3, 3: 4, 4: 5, -2: 6, -7: 9, -10: 10}
SMALL = dict(n=96, mg=64, nnz_per_row=6)
MID = dict(n=256, mg=128, nnz_per_row=6)
# (the two forms of the head are bitwise equal, tests/test_gpu_head_forms.py)
FORMS = {"loads": {"MI_OSQP_INDEX_LOADS": "1"}, "registers": {}, "deep": {"MI_OSQP_RF_FORM": "1"}}
SWITCHES = ("MI_OSQP_INDEX_LOADS", "MI_OSQP_STREAM_FACTOR", "MI_OSQP_STREAM_STATE", "MI_OSQP_DENSE_TAIL", "MI_OSQP_TILE", "MI_OSQP_RF_FORM")


def _solver(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _both_forms(monkeypatch, pr, run, env=None, expect_registers=True, **kw):
    """run(solver) -> list of (info, x, y), once per form; returns (the register form's list, its stats) after the bitwise
    comparison of all three forms.  expect_registers = False: a handle whose index words do not fit - every run takes the
    loading form."""
    out, stats = {}, {}
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    for form in FORMS:
        for k in ("MI_OSQP_INDEX_LOADS", "MI_OSQP_RF_FORM"):
            monkeypatch.delenv(k, raising=False)
        for k, v in {**(env or {}), **FORMS[form]}.items():
            monkeypatch.setenv(k, v)
        s = _solver(pr, **kw)
        st = stats[form] = s.stats()
        print(form, {k: st[k] for k in ("tile", "threads_per_block", "n", "m", "dense_tail_rows", "resident_state",
                                        "resident_factor_steps", "resident_index_words")})
        fit = M.debug_index_words_fit(st["n"], st["m"], tile=st["tile"], threads=st["threads_per_block"],
                                      resident_state=st["resident_state"] == 1)[0]
        assert st["resident_index_words"] == (1 if form != "loads" and fit else 0), (form, fit, st)
        if form != "loads":
            assert st["resident_state"] == 1 and fit == expect_registers, (fit, st)
        out[form] = run(s)
    for form in ("registers", "deep"):
        assert len(out["loads"]) == len(out[form])
        for k, ((i0, x0, y0), (i1, x1, y1)) in enumerate(zip(out["loads"], out[form])):
            assert [i.iter for i in i0] == [i.iter for i in i1], (form, k)
            assert [i.exit_code for i in i0] == [i.exit_code for i in i1], (form, k)
            assert [i.rho_updates for i in i0] == [i.rho_updates for i in i1], (form, k)
            np.testing.assert_array_equal(x0, x1, err_msg=f"x of solve {k}, {form}")
            np.testing.assert_array_equal(y0, y1, err_msg=f"y of solve {k}, {form}")
    return out["registers"], stats["registers"]


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


def _all_meet_oracle(pr, B, info, x, **kw):
    for b in range(B):
        o = _oracle(pr, b, **kw)
        st, xo = o.solve()
        _meets_oracle(info, x, b, st, xo, o.info())


@pytest.mark.parametrize("env", [{}, {"MI_OSQP_RF_FORM": "1"}, {"MI_OSQP_STREAM_FACTOR": "1"}], ids=["long_head", "deep_ring", "streamed_factor"])
def test_headline_shape_two_xloc_trips_and_a_refactorisation_at_iteration_100(env, monkeypatch):
    """n = 512, m = 1024 at 1024 threads: two trips of xloc, half the threads without an x row, every thread a z / y row; the
    QPs that pass iteration 100 get a new rho and a new factor there.  Once per instantiation: both forms of the resident
    head and (MI_OSQP_STREAM_FACTOR=1) the resident state alone, whose kkt_middle streams all of S^-1."""
    B = 6
    pr = PR.random_box_qp(B)
    ((info, x, y),), st = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], env=env)
    assert st["n"] == 512 and st["m"] == 1024 and st["threads_per_block"] == 1024 and st["tile"] == 1
    assert (st["resident_factor_steps"] > 0) == ("MI_OSQP_STREAM_FACTOR" not in env)
    assert any(i.rho_updates >= 1 and i.iter > 100 for i in info), [(i.iter, i.rho_updates) for i in info]
    _all_meet_oracle(pr, B, info, x)


@pytest.mark.parametrize("tail", ["default", "0"])
def test_fewer_rows_than_threads(tail, monkeypatch):
    """N = 256 at 1024 threads: most threads own no row at all and most waves have an empty sweep stream; with the tail the
    analysis picks and with none (MI_OSQP_DENSE_TAIL=0: the D^-1 pass over all rows)."""
    B = 4
    pr = PR.random_box_qp(B, **SMALL)
    ((info, x, y),), st = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], env={} if tail == "default" else {"MI_OSQP_DENSE_TAIL": tail})
    if tail == "0":
        assert st["dense_tail_rows"] == 0
    _all_meet_oracle(pr, B, info, x)


@pytest.mark.parametrize("k", [64, 512])
def test_forced_tails(k, monkeypatch):
    """MI_OSQP_DENSE_TAIL = 64 / 512 at N = 640: one task (waves without a product task, a first task that is all head) and
    36 tasks; with 512 tail rows most rows of the D^-1 pass are tail rows."""
    B = 4
    pr = PR.random_box_qp(B, **MID)
    ((info, x, y),), st = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], env={"MI_OSQP_DENSE_TAIL": str(k)})
    assert st["dense_tail_rows"] == k
    _all_meet_oracle(pr, B, info, x)


@pytest.mark.parametrize("max_iter", [30, 26])
def test_max_iter_that_is_no_multiple_of_the_check_interval(max_iter, monkeypatch):
    """max_iter = 30: launches of 25 and 5 iterations; max_iter = 26: the second launch has ONE iteration - the words are
    loaded, used once, and the call's first iteration is the one that stores x, z and y."""
    B = 4
    pr = PR.random_box_qp(B)
    kw = dict(max_iter=max_iter, eps_abs=1e-10, eps_rel=1e-10)
    ((info, x, y),), _ = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], **kw)
    assert all(i.iter == max_iter for i in info)
    _all_meet_oracle(pr, B, info, x, **kw)


@pytest.mark.parametrize("tile", [1, 2])
def test_qps_that_finish_early_beside_qps_that_go_on(tile, monkeypatch):
    """eps = 1e-2 on the N = 640 pattern: QPs finish at iterations 25, 50 and 75, so launches see finished tiles (which leave
    at once) and, with two QPs per tile, finished QPs inside a tile that iterates on."""
    B = 8
    pr = PR.random_box_qp(B, **MID)
    kw = dict(eps_abs=1e-2, eps_rel=1e-2)
    ((info, x, y),), st = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], env={"MI_OSQP_TILE": str(tile)}, **kw)
    assert st["tile"] == tile
    iters = [i.iter for i in info]
    assert min(iters) == 25 and 50 in iters and max(iters) >= 75, iters
    if tile == 2:
        assert any(iters[t] != iters[t + 1] for t in range(0, B, 2)), iters
    _all_meet_oracle(pr, B, info, x, **kw)


def test_one_qp_loses_its_inertia_at_the_rho_update(monkeypatch):
    """The construction of tests/test_gpu_resident_factor.py: the launches of the QP that fails its refactorisation at
    iteration 50 get null descriptors; it ends kNonConvex (-7) with a NaN solution, its neighbours stay bitwise equal."""
    kw = dict(eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=50)
    B, bad = 6, 2
    pr = PR.random_box_qp(B, **SMALL)
    Pp = pr["P"]
    diag = Pp.indices == np.repeat(np.arange(Pp.shape[1]), np.diff(Pp.indptr))
    pr["Px"][bad][diag] -= 1.32
    ((info, x, y),), _ = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], env={"MI_OSQP_DENSE_TAIL": "64"}, **kw)
    for b in range(B):
        o = _oracle(pr, b, **kw)
        st, xo = o.solve()
        if b == bad:
            assert st == -7 and o.info().iter == 50                      # the construction holds
            assert info[b].status_val == -7 and info[b].exit_code == 9 and info[b].iter == 50
            assert np.all(np.isnan(x[b])) and np.all(np.isnan(y[b]))
        _meets_oracle(info, x, b, st, xo, o.info())


def test_warm_second_solve_and_a_reset_between_two_solves(monkeypatch):
    B = 4
    pr = PR.random_box_qp(B)

    def run(s):
        r = [_solve(s), _solve(s)]
        s.reset()
        r.append(_solve(s))
        return r
    res, _ = _both_forms(monkeypatch, pr, run)
    assert [i.iter for i in res[2][0]] == [i.iter for i in res[0][0]]
    np.testing.assert_array_equal(res[2][1], res[0][1])
    np.testing.assert_array_equal(res[2][2], res[0][2])
    for b in range(B):
        o = _oracle(pr, b)
        for k in range(2):
            st, xo = o.solve()
            _meets_oracle(res[k][0], res[k][1], b, st, xo, o.info())


def test_resident_state_whose_trips_exceed_the_cap_keeps_loading(monkeypatch):
    """n = 600, m = 1100 at 1024 threads: the state is resident, but the z / y rows need two trips per thread - over the cap,
    so the handle reports resident_index_words = 0 and runs what the switch-off run runs."""
    B = 3
    pr = PR.random_box_qp(B, n=600, mg=500, nnz_per_row=6)
    ((info, x, y),), st = _both_forms(monkeypatch, pr, lambda s: [_solve(s)], expect_registers=False)
    assert st["resident_state"] == 1 and st["resident_index_words"] == 0 and st["m"] > st["threads_per_block"]
    _all_meet_oracle(pr, B, info, x)
