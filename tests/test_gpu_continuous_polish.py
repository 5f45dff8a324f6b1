"""GPU (-m gpu): polishing on demand in the continuous mode (mi_osqp.h mi_osqp_batch_polish_some).

The contract: for every QP the result of solve_begin_some / advance / poll + polish_some - x, y, obj_val, pri_res, dua_res,
iter, rho_updates, status_polish and the active set - equals BIT FOR BIT the result of a blocking solve() of a handle with
the same data and polish = 1; a QP that is never listed equals its plain blocking solve (polish = 0), whatever happens to
its tile partner.  The blocking polish itself is pinned by tests/test_gpu_polish.py (scipy, the oracle at 1e-10).

A reference is computed once per (batch, tile, dense tail) and kept as plain arrays: the first blocking solve with polish,
the second one (the warm re-solve from the polished points) and the plain solve."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exit_cases as EC                                                         # noqa: E402
import osqp_solver_amd as M                                                     # noqa: E402
from osqp_solver_amd import problems as PR                                      # noqa: E402

pytestmark = pytest.mark.gpu
B1 = 11
FIRST, SECOND = [0, 2, 3, 7, 10], [1, 4, 5, 6, 8, 9]          # the staggered begins of test_gpu_continuous.py
_BATCH, _REF = {}, {}


def _batch(name):
    if name not in _BATCH:
        _BATCH[name] = {"box": lambda: PR.random_box_qp(B1, n=96, mg=64, nnz_per_row=6),
                        "box_tail": lambda: PR.random_box_qp(8, n=128, mg=96, nnz_per_row=6),
                        "gomp": lambda: PR.gomp_batch(6, 3, 12)}[name]()
    return _BATCH[name]


def _make(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _env(monkeypatch, tile, tail="", ring=""):
    for k in ("MI_OSQP_TILE", "MI_OSQP_DENSE_TAIL", "MI_OSQP_CONT_RING_KB"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MI_OSQP_TILE", str(tile))
    if tail:
        monkeypatch.setenv("MI_OSQP_DENSE_TAIL", tail)
    if ring:
        monkeypatch.setenv("MI_OSQP_CONT_RING_KB", ring)


def _snap(s, info):
    return dict(info=list(info), x=s.primal().copy(), y=s.dual().copy(), act=s.polish_active().copy())


def _reference(name, tile, tail=""):
    """Blocking results for the environment in force (_env first): pol = solve() with polish = 1, pol2 = its second solve(),
    plain = solve() with polish = 0.  At least one QP of pol must have an accepted polish: a test that polishes nothing
    proves nothing."""
    key = (name, tile, tail)
    if key not in _REF:
        pr = _batch(name)
        r1 = _make(pr, polish=1)
        assert r1.stats()["tile"] == tile
        if tail:
            print(f"{name}: dense tail of {r1.stats()['dense_tail_rows']} rows")
        pol = _snap(r1, r1.solve())
        pol2 = _snap(r1, r1.solve())
        r0 = _make(pr)
        plain = _snap(r0, r0.solve())
        print(f"{name} tile {tile} tail '{tail}': status_val {[i.status_val for i in pol['info']]} iter {[i.iter for i in pol['info']]} "
              f"status_polish {[i.status_polish for i in pol['info']]}, second solve {[i.status_polish for i in pol2['info']]}")
        _REF[key] = dict(pol=pol, pol2=pol2, plain=plain)
    ref = _REF[key]
    accepted = [q for q, i in enumerate(ref["pol"]["info"]) if i.status_polish == 1]
    assert accepted, "the reference accepts no polish"
    for q in accepted:                                 # an accepted polish moves the solution: the comparisons tell the two apart
        assert not np.array_equal(ref["pol"]["x"][q], ref["plain"]["x"][q]), q
    return ref


def _same_qp(s, q, ref, what=""):
    """QP q of the continuous handle s (its getters of the continuous mode) against QP q of a reference snapshot"""
    a, b = s.info_some([q])[0], ref["info"][q]
    for f in ("status_val", "exit_code", "iter", "rho_updates", "status_polish", "obj_val", "pri_res", "dua_res", "rho"):
        assert getattr(a, f) == getattr(b, f), (what, q, f, getattr(a, f), getattr(b, f))
    assert np.array_equal(s.primal_some([q])[0], ref["x"][q], equal_nan=True), (what, q, "x")
    assert np.array_equal(s.dual_some([q])[0], ref["y"][q], equal_nan=True), (what, q, "y")


class _Driver:
    """advance / poll loop that polishes every QP of `wanted` as soon as poll() reports it kOptimal, while the others go on"""

    def __init__(self, s, wanted):
        self.s, self.wanted = s, set(wanted)
        self.begun, self.solved, self.polishing, self.polished = set(), [], set(), []
        self.partner_running = []          # (q, partner): polish calls that fell while the tile partner was still in its solve

    def begin(self, ids):
        self.s.solve_begin_some(ids)
        self.begun |= set(ids)

    def step(self):
        s = self.s
        s.advance(1)
        fin = [int(q) for q in s.poll(True)]
        assert len(set(fin)) == len(fin)
        again = [q for q in fin if q in self.polishing]
        new = [q for q in fin if q not in self.polishing]
        assert not set(new) & set(self.solved), "a solve was reported twice"
        self.polishing -= set(again); self.polished += again
        self.solved += new
        info = s.info_some(new)
        todo = [q for q, i in zip(new, info) if i.status_val == 1 and q in self.wanted]
        assert all(i.status_polish == 0 for i in info)          # the report of the solve carries no polish
        if todo:
            in_solve = self.begun - set(self.solved)
            self.partner_running += [(q, q ^ 1) for q in todo if (q ^ 1) in in_solve]
            before = s.running()
            s.polish_some(todo)
            assert s.running() == before + len(todo)
            self.polishing |= set(todo)
        return fin

    def drain(self, max_advances=400):
        for _ in range(max_advances):
            if not self.s.running():
                return
            self.step()
        raise AssertionError("continuous solve did not finish")


def _staggered_polished_run(s, wanted):
    d = _Driver(s, wanted)
    d.begin(FIRST)
    d.step(); d.step()
    d.begin(SECOND)                                    # these start two segments later
    d.drain()
    assert sorted(d.solved) == list(range(s.B))
    return d


def _check_all(s, d, ref, skipped=()):
    optimal = [q for q in range(s.B) if ref["pol"]["info"][q].status_val == 1]
    assert sorted(d.polished) == sorted(set(optimal) - set(skipped))
    for q in range(s.B):
        _same_qp(s, q, ref["plain"] if q in skipped else ref["pol"], "continuous getters")


@pytest.mark.parametrize("tile", [1, 2])
def test_staggered_solves_polished_as_reported_equal_blocking_polish_bitwise(tile, monkeypatch):
    _env(monkeypatch, tile)
    ref = _reference("box", tile)
    s = _make(_batch("box"))
    assert s.stats()["tile"] == tile
    skipped = (3, 6)                                   # never listed: they must end as their plain blocking solve
    d = _staggered_polished_run(s, set(range(B1)) - set(skipped))
    print(f"tile {tile}: solves reported {d.solved}, polishes reported {d.polished}, polished next to a running partner {d.partner_running}")
    _check_all(s, d, ref, skipped)
    if tile == 2:
        assert d.partner_running, "no polish call fell while the tile partner was still iterating"
    # a blocking getter ends the continuous mode: the whole-batch getters and the active sets
    x, y, info, act = s.primal(), s.dual(), s.info(), s.polish_active()
    for q in range(B1):
        r = ref["plain"] if q in skipped else ref["pol"]
        assert np.array_equal(x[q], r["x"][q]) and np.array_equal(y[q], r["y"][q]), q
        assert info[q].status_polish == r["info"][q].status_polish, q
        assert np.array_equal(act[q], r["act"][q]), q


@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("name", ["box_tail", "gomp"])
def test_dense_tail_polish_factor_through_the_list_path_bitwise(name, tile, monkeypatch):
    _env(monkeypatch, tile, tail="64")
    ref = _reference(name, tile, "64")
    pr = _batch(name)
    s = _make(pr)
    assert s.stats()["dense_tail_rows"] == 64          # both patterns: the polish factor goes through the dense-tail kernels
    B = s.B
    d = _Driver(s, range(B))
    d.begin(list(range(0, B, 2)))
    d.step()
    d.begin(list(range(1, B, 2)))
    d.drain()
    _check_all(s, d, ref)
    act = s.polish_active()                            # inside the mode: it waits for the stream and does not leave the mode
    assert np.array_equal(act, ref["pol"]["act"])
    assert np.array_equal(s.primal_some(range(B)), ref["pol"]["x"], equal_nan=True)


def _solved_handle(pr):
    """every QP solved in the continuous mode, nothing polished; returns (handle, kOptimal ids)"""
    s = _make(pr)
    s.solve_begin_some(range(s.B))
    for _ in range(400):
        if not s.running():
            break
        s.advance(1); s.poll(True)
    assert not s.running()
    return s, [q for q, i in enumerate(s.info_some(range(s.B))) if i.status_val == 1]


def test_reporting_protocol_second_report_through_the_next_advance(monkeypatch):
    _env(monkeypatch, 2)
    ref = _reference("box", 2)
    s, opt = _solved_handle(_batch("box"))
    assert len(opt) >= 7
    ids, g1, g2 = opt[:3], opt[3:5], opt[5:7]
    # an advance enqueued BEFORE the polish call publishes the old epoch: its poll reports none of them
    s.advance(1)
    s.polish_some(ids)
    assert s.running() == len(ids)
    act = s.polish_active()                            # before any report: the call waits for the enqueued polish, the mode goes on
    for q in ids:
        assert np.array_equal(act[q], ref["pol"]["act"][q]) and np.any(act[q] != 0), q
    assert s.running() == len(ids)
    assert list(s.poll(True)) == [] and s.running() == len(ids)
    with pytest.raises(M.MiOsqpError):
        s.warm_start_x_some(ids[:1], np.zeros(s.n))    # they count as running: no per-QP call accepts them
    # the next advance has nothing to iterate and reports exactly them
    s.advance(1)
    assert sorted(s.poll(True)) == sorted(ids) and s.running() == 0
    st = s.last_polish_stats()
    assert st["polished"] == len(ids) and st["seconds"] == 0.0
    assert st["accepted"] == sum(ref["pol"]["info"][q].status_polish == 1 for q in ids)
    for q in ids:
        _same_qp(s, q, ref["pol"], "one call")
    # two calls before one advance: the second neither re-polishes the first one's QPs nor wipes their results
    s.polish_some(g1)
    s.polish_some(g2)
    assert s.running() == len(g1) + len(g2)
    s.advance(1)
    assert sorted(s.poll(True)) == sorted(g1 + g2) and s.running() == 0
    for q in g1 + g2:
        _same_qp(s, q, ref["pol"], "two calls")
    for q in set(range(B1)) - set(ids + g1 + g2):      # the rest: untouched
        _same_qp(s, q, ref["plain"], "not listed")


def test_accepted_polish_is_the_next_warm_start(monkeypatch):
    _env(monkeypatch, 2)
    ref = _reference("box", 2)
    s, opt = _solved_handle(_batch("box"))
    s.polish_some(opt)
    s.advance(1)
    assert sorted(s.poll(True)) == sorted(opt)
    acc = [q for q in opt if s.info_some([q])[0].status_polish == 1]
    assert acc == [q for q in opt if ref["pol"]["info"][q].status_polish == 1] and acc
    s.solve_begin_some(acc)
    fin = []
    for _ in range(50):
        if not s.running():
            break
        s.advance(1); fin += list(s.poll(True))
    assert sorted(fin) == sorted(acc)
    for q, i in zip(acc, s.info_some(acc)):            # the polished point satisfies the termination check at once
        assert i.iter == s.settings.check_termination and i.exit_code == 0 and i.status_polish == 0, (q, i.iter, i.exit_code)
    # the reference's second solve() polishes again: so does this handle, and the results are the same bits
    s.polish_some(acc)
    s.advance(1)
    assert sorted(s.poll(True)) == sorted(acc)
    for q in acc:
        _same_qp(s, q, ref["pol2"], "second solve")


def test_refusals_change_nothing(monkeypatch):
    _env(monkeypatch, 2)
    ref = _reference("box", 2)
    base = _batch("box")
    kinds = ["feas"] * B1
    kinds[4] = "pinf"                                  # QP 4 ends primal infeasible; the other QPs are those of the reference
    pr = EC.apply_kinds(base, kinds)
    s = _make(pr)

    def refused(ids):
        before = s.running()
        with pytest.raises(M.MiOsqpError) as e:
            s.polish_some(ids)
        assert e.value.code == 1 and s.running() == before
        assert b"polish_some" in M.lib().mi_osqp_last_error()

    refused([0])                                       # the handle is not in the continuous mode
    s.solve_begin_some(range(B1))
    assert s.running() == B1
    refused([0])                                       # still running
    s.polish_some([])                                  # nothing happens
    assert s.running() == B1
    for _ in range(400):
        if not s.running():
            break
        s.advance(1); s.poll(True)
    info = s.info_some(range(B1))
    assert info[4].exit_code != 0 and all(info[q].status_val == 1 for q in (0, 1, 2, 5, 7))
    refused([4])                                       # not kOptimal
    refused([0, 4])                                    # all or nothing: QP 0 stays polishable
    refused([0, 0])                                    # listed twice
    refused([B1]); refused([-1]); refused([0, B1])     # out of range
    assert M.lib().mi_osqp_batch_polish_some(s._h, 2, None) == 6 and s.running() == 0      # no ids
    s.warm_start_x_some([1], s.primal_some([1]))
    refused([1])                                       # its iterate was changed
    s.update_q_some([2], pr["q"][2])
    refused([2])                                       # its data was changed
    assert s.running() == 0
    s.polish_some([0])                                 # after all that, a valid call gives the reference's bits
    refused([0])                                       # enqueued: running
    s.advance(1)
    assert list(s.poll(True)) == [0]
    _same_qp(s, 0, ref["pol"], "after refusals")
    refused([0])                                       # polished already: once per solve
    refused([5, 0])
    s.polish_some([7, 5])
    s.advance(1)
    assert sorted(s.poll(True)) == [5, 7]
    for q in (5, 7):
        _same_qp(s, q, ref["pol"], "after refusals")
    s.solve_begin_some([0])                            # a new solve makes it polishable again once it is reported
    refused([0])
    s.advance(1)
    assert list(s.poll(True)) == [0]
    s.polish_some([0])
    s.advance(1)
    assert list(s.poll(True)) == [0]
    _same_qp(s, 0, ref["pol2"], "second solve")
    s.primal()                                         # leaves the continuous mode
    refused([5])


def test_leaving_the_mode_finds_every_enqueued_polish_executed(monkeypatch):
    _env(monkeypatch, 2)
    ref = _reference("box", 2)
    s, opt = _solved_handle(_batch("box"))
    reported, pending = opt[: len(opt) // 2], opt[len(opt) // 2:]
    s.polish_some(reported)
    s.advance(1)
    assert sorted(s.poll(True)) == sorted(reported)
    s.polish_some(pending)                             # enqueued, never polled
    x, y, info, act = s.primal(), s.dual(), s.info(), s.polish_active()
    for q in range(B1):
        r = ref["pol"]
        assert np.array_equal(x[q], r["x"][q], equal_nan=True) and np.array_equal(y[q], r["y"][q], equal_nan=True), q
        for f in ("status_val", "iter", "rho_updates", "status_polish", "obj_val", "pri_res", "dua_res"):
            assert getattr(info[q], f) == getattr(r["info"][q], f), (q, f)
        assert np.array_equal(act[q], r["act"][q]), q
    assert s.running() == 0
    i2 = s.solve()                                     # a blocking solve of the polish = 0 handle: nothing is polished any more
    assert all(i.status_polish == 0 for i in i2) and s.last_polish_stats()["polished"] == 0


def test_a_staging_ring_that_wraps_every_few_calls_changes_nothing(monkeypatch):
    """Every QP runs its own loop of ROUNDS rounds - new rows and bounds, a warm start, a solve, a polish as soon as the solve
    is reported, the next round as soon as the polish is reported - so the QPs drift apart and the updates of some fall
    while the polishes of others are enqueued.  The staging ring is barely larger than one whole-batch update
    (MI_OSQP_CONT_RING_KB): the ids of the polish calls share it with the rows of the updates, which make it wrap about once
    per round of the batch.  ring_wraps() shows that it happened, also with a polish enqueued and not reported.
    Reference: the same rounds, blocking, on a handle with polish = 1 (its own: the rounds change it)."""
    ROUNDS = 8
    _env(monkeypatch, 2, ring="1")
    M.lib().mi_osqp_release_device_cache()             # (no kept pinned block, possibly larger, becomes the ring)
    pr = _batch("box")
    n = pr["n"]
    rng = np.random.default_rng(11)
    data = [None]
    for rnd in range(ROUNDS):
        data.append((pr["Ax"] * (1.0 + 0.1 * rng.standard_normal(pr["Ax"].shape)), pr["l"] * (1.0 + 0.04 * rnd),
                     pr["u"] * (1.0 - 0.02 * rnd), 0.1 * rng.standard_normal((B1, n))))
    ref = _make(pr, polish=1)
    refs = [_snap(ref, ref.solve())]
    for Ax2, l2, u2, xw in data[1:]:
        ref.update_A_bounds(Ax2, l2, u2); ref.warm_start_x(xw)
        refs.append(_snap(ref, ref.solve()))
    accepted = sum(i.status_polish == 1 for r in refs for i in r["info"])
    assert accepted > 0
    s = _make(pr)
    assert s.stats()["tile"] == 2
    round_of, polishing, finished_rounds = [0] * B1, set(), 0
    wraps_with_a_polish_pending = 0
    s.solve_begin_some(range(B1))
    for _ in range(2000):
        if not s.running():
            break
        s.advance(1)
        fin = [int(q) for q in s.poll(True)]
        info = s.info_some(fin)
        over = [q for q, i in zip(fin, info) if q in polishing or i.status_val != 1]      # polished, or nothing to polish
        todo = [q for q in fin if q not in over]
        polishing -= set(over)
        for q in over:
            _same_qp(s, q, refs[round_of[q]], f"round {round_of[q]}")
            finished_rounds += 1
        if todo:
            s.polish_some(todo)
            polishing |= set(todo)
        nxt = [q for q in over if round_of[q] < ROUNDS]
        if nxt:
            for q in nxt:
                round_of[q] += 1
            rows = [np.stack([data[round_of[q]][k][q] for q in nxt]) for k in range(4)]
            w0 = s.ring_wraps()
            s.update_A_bounds_some(nxt, rows[0], rows[1], rows[2])
            s.warm_start_x_some(nxt, rows[3])
            if polishing:
                wraps_with_a_polish_pending += s.ring_wraps() - w0
            s.solve_begin_some(nxt)
    assert not s.running() and finished_rounds == B1 * (ROUNDS + 1) and round_of == [ROUNDS] * B1
    print(f"ring wraps {s.ring_wraps()}, {wraps_with_a_polish_pending} of them with a polish enqueued and not reported; "
          f"{accepted} polishes accepted in the reference")
    # the ring (solver.hip cont_enter, rounded up to pages) holds at most `ring` bytes, a round stages at least the new rows and
    # bounds and the scaled values of A of every QP, and a span never straddles the end: at least staged / ring wraps
    nnzA, nnzP, m = pr["A"].nnz, pr["P"].nnz, pr["m"]
    ring = -(-((nnzA + nnzP + 2 * m + n + 16) * 8 * B1 + (64 << 10)) // 4096) * 4096
    staged = ROUNDS * B1 * 8 * (nnzA + 2 * m + nnzA)
    assert staged // ring >= 4, (staged, ring)
    assert s.ring_wraps() >= staged // ring
    assert wraps_with_a_polish_pending >= 1            # (the sequence is deterministic: some QPs' rows wrap behind a polish)
