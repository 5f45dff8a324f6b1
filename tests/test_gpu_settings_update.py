"""GPU (-m gpu): settings updates after setup (README "Settings updates"; mi_osqp.h "settings updates") on every solve path.

Criteria.  "Oracle" is test_gpu_parity._compare against an oracle set up with the settings in question (status, exit code,
iteration count, rho updates, x to 1e-6).  "Bitwise" is np.array_equal on x and y and equal info fields against a handle that
was SET UP with those settings: setup, reinit_some and the refactorisation are bit-identical (mi_osqp.h, reset / reinit_some),
and an update changes nothing else.  One info field is exempt where an update follows a solve: the count of rho updates is
kept across a settings update (upstream restarts it in data updates only), so it is the earlier count plus the fresh handle's.

Data: 11 QPs of random_box_qp(n=96, mg=64) - a ragged last tile for tiles of 2 and 4 - with eight equality rows (rho vector
1e3 * rho) and eight free rows (rho vector at its minimum).  The oracle needs 50-125 iterations for them with the default
settings (two QPs with a rho update), 25-50 with rho = 0.7, 125-150 and a rho update each with rho = 0.01, 125-175 with eps 1e-6,
110-180 with eps 1e-6 / check_termination 10 / alpha 1.4 at an interval of 100 - and 70-110 with the interval "auto" would give
for check_termination 10, so a moved interval shows.  With max_iter = 60 eight of them stop at iteration 60 (the oracle reports
them solved-inaccurate, status 2: the closing check of OSQP uses ten times the tolerances) and three are solved at 50."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import osqp_solver_amd as M                                                     # noqa: E402
from oracle.kkt_check import sym_from_any                                       # noqa: E402
from osqp_solver_amd import problems as PR                                      # noqa: E402
from test_gpu_continuous import _drain                                          # noqa: E402
from test_gpu_parity import _compare, _oracle_batch                             # noqa: E402
from test_settings_update_abi import build_shim_settings, run_shim_settings     # noqa: E402

pytestmark = pytest.mark.gpu
B, N_VAR = 11, 96
TIGHT = dict(eps_abs=1e-6, eps_rel=1e-6, check_termination=10, alpha=1.4)
DEFAULTS = dict(eps_abs=1e-3, eps_rel=1e-3, check_termination=25, alpha=1.6, max_iter=4000, scaled_termination=0)
INFO_FIELDS = [k for k, _ in M.Info._fields_]
_CACHE = {}


def _data():
    if "pr" not in _CACHE:
        pr = PR.random_box_qp(B, n=N_VAR, mg=64, nnz_per_row=6)
        n = N_VAR
        mid = 0.5 * (pr["l"][:, n:n + 8] + pr["u"][:, n:n + 8])
        pr["l"][:, n:n + 8] = mid; pr["u"][:, n:n + 8] = mid
        pr["l"][:, n + 8:n + 16] = -1e30; pr["u"][:, n + 8:n + 16] = 1e30
        _CACHE["pr"] = pr
    return _CACHE["pr"]


def _oracle(idx=None, **settings):
    """the oracle's results for the common data with these settings, computed once"""
    idx = list(range(B)) if idx is None else list(idx)
    key = ("oracle", tuple(idx), tuple(sorted(settings.items())))
    if key not in _CACHE:
        _CACHE[key] = _oracle_batch(_data(), idx, **settings)
    return _CACHE[key]


def _env(monkeypatch, tile=None, **env):
    for k in ("MI_OSQP_TILE", "MI_OSQP_GLOBAL_XS", "MI_OSQP_GROUPS", "MI_OSQP_GROUP_THREADS", "MI_OSQP_DENSE_TAIL"):
        monkeypatch.delenv(k, raising=False)
    if tile:
        monkeypatch.setenv("MI_OSQP_TILE", str(tile))
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _make(pr=None, **kw):
    pr = _data() if pr is None else pr
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _result(s):
    return s.info(), s.primal().copy(), s.dual().copy()


def _solve(s):
    s.solve()
    return _result(s)


def _same_info(a, b, skip=()):
    for k in INFO_FIELDS:
        if k not in skip:
            va, vb = getattr(a, k), getattr(b, k)
            assert va == vb or (va != va and vb != vb), (k, va, vb)


def _bitwise(ra, rb, idx=None, skip=()):
    (ia, xa, ya), (ib, xb, yb) = ra, rb
    for b in (range(len(ia)) if idx is None else idx):
        _same_info(ia[b], ib[b], skip)
        assert np.array_equal(xa[b], xb[b], equal_nan=True) and np.array_equal(ya[b], yb[b], equal_nan=True), b


def _fields(s):
    return {k: getattr(s, k) for k, _ in M.Settings._fields_}


def _refused(code, call, *args, **kw):
    with pytest.raises(M.MiOsqpError) as e:
        call(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


# ------------------------------------------------------------------ 1. termination fields
@pytest.mark.parametrize("tile", [1, 2, 4])
def test_termination_fields_updated_equal_a_setup_with_them(tile, monkeypatch):
    _env(monkeypatch, tile)
    s = _make()
    assert s.stats()["tile"] == tile
    first = _solve(s)
    _compare(first[0], first[1], _oracle(), range(B))
    assert _fields(s.settings())["adaptive_rho_interval"] == 100            # the resolved "auto"
    cases = [(TIGHT, False), (dict(DEFAULTS, max_iter=60), True), (dict(DEFAULTS, scaled_termination=1), False)]
    for upd, capped in cases:
        now = s.update_settings(**upd)
        want = dict(_fields(M.default_settings(adaptive_rho_interval=100, **upd)), warm_start=1)
        assert _fields(now) == want and _fields(s.settings()) == want and s.settings.check_termination == want["check_termination"]
        s.reset()
        got = _solve(s)
        kw = {k: v for k, v in upd.items() if DEFAULTS.get(k, None) != v}
        fresh = _solve(_make(adaptive_rho_interval=100, **kw))
        print(f"tile {tile} {kw}: iterations {[i.iter for i in got[0]]}, rho updates {[i.rho_updates for i in got[0]]}")
        _bitwise(got, fresh)
        _compare(got[0], got[1], _oracle(adaptive_rho_interval=100, **kw), range(B))
        if capped:                    # (which status the cap gives is the oracle's word, above)
            assert max(i.iter for i in got[0]) == 60 and sum(i.iter == 60 for i in got[0]) >= 8
    # a refused update - a fixed field changed, an invalid value - changes nothing
    before = _fields(s.settings())
    s.reset(); ref = _solve(s)
    for bad in (dict(sigma=1e-5), dict(scaling=5), dict(adaptive_rho=0), dict(adaptive_rho_interval=50), dict(adaptive_rho_tolerance=3.0),
                dict(alpha=2.0), dict(eps_abs=1e-6, alpha=2.0), dict(eps_abs=0.0, eps_rel=0.0), dict(max_iter=0)):
        _refused(2, s.update_settings, **bad)
    assert _fields(s.settings()) == before
    s.update_settings(adaptive_rho_interval=0)                               # the interval setup derived from 0: accepted, kept
    assert _fields(s.settings()) == before
    s.reset()
    _bitwise(_solve(s), ref)


def test_an_explicit_interval_is_fixed_and_zero_is_not_accepted_for_it():
    s = _make(adaptive_rho_interval=50)
    _refused(2, s.update_settings, adaptive_rho_interval=0)
    _refused(2, s.update_settings, adaptive_rho_interval=100)
    assert s.update_settings(check_termination=10).adaptive_rho_interval == 50


# ------------------------------------------------------------------ 2. warm re-solve
def test_tightened_tolerances_continue_from_the_solution_and_keep_the_count_of_rho_updates():
    pr = _data()
    s = _make()
    i1 = s.solve()
    base = [i.rho_updates for i in i1]
    assert max(base) >= 1, base                                    # (else a restarted count could not show)
    s.update_settings(eps_abs=1e-6, eps_rel=1e-6)
    i2, x, y = _solve(s)
    for b in range(B):
        assert i2[b].exit_code == M.K_OPTIMAL and i2[b].iter > 0 and i2[b].rho_updates >= base[b], (b, i2[b].iter, i2[b].rho_updates, base[b])
        P, A = PR.qp_matrices(pr, b)
        Pf = sym_from_any(P)
        Ax = A @ x[b]
        z = np.clip(Ax, pr["l"][b], pr["u"][b])
        pri, dua = np.max(np.abs(Ax - z)), np.max(np.abs(Pf @ x[b] + pr["q"][b] + A.T @ y[b]))
        eps_pri = 1e-6 + 1e-6 * max(np.max(np.abs(Ax)), np.max(np.abs(z)))
        eps_dua = 1e-6 + 1e-6 * max(np.max(np.abs(Pf @ x[b])), np.max(np.abs(A.T @ y[b])), np.max(np.abs(pr["q"][b])))
        print(f"QP {b}: iter {i2[b].iter}, rho updates {base[b]} -> {i2[b].rho_updates}, pri {pri:.3e} / {eps_pri:.3e}, dua {dua:.3e} / {eps_dua:.3e}")
        assert pri <= eps_pri * (1 + 1e-9) and dua <= eps_dua * (1 + 1e-9), (b, pri, eps_pri, dua, eps_dua)


# ------------------------------------------------------------------ 3. scalar rho before any solve
@pytest.mark.parametrize("dense_tail", [None, "0"])
@pytest.mark.parametrize("r", [0.7, 0.01])
def test_scalar_rho_before_any_solve_equals_a_setup_with_it(r, dense_tail, monkeypatch):
    _env(monkeypatch, **({} if dense_tail is None else {"MI_OSQP_DENSE_TAIL": dense_tail}))
    s = _make()
    print("dense_tail_rows", s.stats()["dense_tail_rows"])
    if dense_tail == "0":
        assert s.stats()["dense_tail_rows"] == 0
    assert s.update_settings(rho=r).rho == r
    got = _solve(s)
    fresh = _solve(_make(rho=r))
    print(f"rho {r}: iterations {[i.iter for i in got[0]]}, rho updates {[i.rho_updates for i in got[0]]}")
    _bitwise(got, fresh)
    _compare(got[0], got[1], _oracle(rho=r), range(B))


def test_scalar_rho_is_clamped_and_invalid_values_change_nothing():
    s = _make()
    ref = _solve(s)
    before = _fields(s.settings())
    for bad in (0.0, -1.0, float("nan")):
        _refused(2, s.update_settings, rho=bad)
    assert _fields(s.settings()) == before
    s.reset()
    _bitwise(_solve(s), ref)
    s.refactor_time()
    assert s.update_settings(rho=1e9).rho == 1e6 and s.settings().rho == 1e6
    f_ms, t_ms, launches, qps = s.refactor_time()
    print(f"scalar rho update of {B} QPs: factor_kernel {f_ms:.3f} ms, dense tail {t_ms:.3f} ms, {launches} launch(es), {qps} QPs")
    assert qps == B and launches == 1                              # one refactorisation of every QP, nothing else
    assert all(i.rho == 1e6 for i in s.info())
    assert s.update_settings(rho=1e-9).rho == 1e-6
    s.update_settings(rho=0.1)
    s.reset()                                                      # the snapshot was retaken: rho = 0.1 for every QP, cold
    _bitwise(_solve(s), ref)


# ------------------------------------------------------------------ 4. scalar rho after a solve
def test_scalar_rho_after_a_solve_equals_a_setup_with_it_given_the_same_warm_starts():
    s = _make()
    i1, x1, y1 = _solve(s)
    base = [i.rho_updates for i in i1]
    s.update_settings(rho=0.7)
    assert all(i.rho == 0.7 for i in s.info()) and [i.rho_updates for i in s.info()] == base
    s.warm_start_x(x1); s.warm_start_y(y1)
    got = _solve(s)
    f = _make(rho=0.7)
    cold = _solve(f)
    f2 = _make(rho=0.7)
    f2.warm_start_x(x1); f2.warm_start_y(y1)
    fresh = _solve(f2)
    _bitwise(got, fresh, skip=("rho_updates",))
    assert [i.rho_updates for i in got[0]] == [base[b] + fresh[0][b].rho_updates for b in range(B)]
    s.reset()                                                      # back to the state after the update: rho = 0.7, cold, count 0
    _bitwise(_solve(s), cold)
    _compare(cold[0], cold[1], _oracle(rho=0.7), range(B))


# ------------------------------------------------------------------ 5. one rho per QP
@pytest.mark.parametrize("tile", [1, 2, 4])
def test_rho_each_gives_every_qp_its_own_rho(tile, monkeypatch):
    _env(monkeypatch, tile)
    rho = 0.01 * 3.0 ** np.arange(B)
    s = _make()
    assert s.stats()["tile"] == tile
    s.update_rho_each(rho)
    assert [i.rho for i in s.info()] == list(rho) and s.settings().rho == 0.1
    got = _solve(s)
    print(f"tile {tile}: iterations {[i.iter for i in got[0]]}, rho updates {[i.rho_updates for i in got[0]]}")
    for b in range(B):
        _compare(got[0], got[1], _oracle(idx=[b], rho=float(rho[b])), [b])
    # isolation: QP 0 does not see the other ten values
    s2 = _make()
    perm = rho.copy(); perm[1:] = rho[1:][::-1] * 1.5
    s2.update_rho_each(perm)
    _bitwise(got, _solve(s2), idx=[0])
    before = [i.rho for i in s2.info()]
    for bad in (0.0, -0.1, float("nan")):
        v = rho.copy(); v[B - 1] = bad
        _refused(2, s2.update_rho_each, v)
    assert [i.rho for i in s2.info()] == before
    # cross-check with the adapted rho of a solved handle: H carries on from its solution with tight tolerances, F is set up
    # tight and given H's rho, x and y
    H = _make()
    ih, xh, yh = _solve(H)
    F = _make(eps_abs=1e-6, eps_rel=1e-6)
    F.update_rho_each([i.rho for i in ih])
    F.warm_start_x(xh); F.warm_start_y(yh)
    H.update_settings(eps_abs=1e-6, eps_rel=1e-6)
    H.warm_start_x(xh); H.warm_start_y(yh)
    rf, rh = _solve(F), _solve(H)
    _bitwise(rf, rh, skip=("rho_updates",))
    assert [i.rho_updates for i in rh[0]] == [ih[b].rho_updates + rf[0][b].rho_updates for b in range(B)]


# ------------------------------------------------------------------ 6. single large QP
class _Single:
    """one QP through mi_osqp_setup / mi_osqp_update_settings / mi_osqp_solve"""

    def __init__(self, pr, b=0):
        L = M.lib()
        P, A = PR.qp_matrices(pr, b)
        self.n = pr["n"]
        a = lambda v, t: np.ascontiguousarray(v, dtype=t)
        ip, dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_int64)), lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
        Pp, Pi, Px = a(P.indptr, np.int64), a(P.indices, np.int64), a(P.data, np.float64)
        Ap, Ai, Ax = a(A.indptr, np.int64), a(A.indices, np.int64), a(A.data, np.float64)
        q, l, u = a(pr["q"][b], np.float64), a(pr["l"][b], np.float64), a(pr["u"][b], np.float64)
        self._h = C.c_void_p()
        s = M.default_settings()
        rc = L.mi_osqp_setup(C.byref(self._h), self.n, A.shape[0], ip(Pp), ip(Pi), dp(Px), dp(q), ip(Ap), ip(Ai), dp(Ax), dp(l), dp(u), C.byref(s))
        assert rc == 0, rc

    def update_settings(self, **fields):
        L, s = M.lib(), M.Settings()
        assert L.mi_osqp_get_settings(self._h, C.byref(s)) == 0
        for k, v in fields.items():
            setattr(s, k, v)
        rc = L.mi_osqp_update_settings(self._h, C.byref(s))
        assert L.mi_osqp_get_settings(self._h, C.byref(s)) == 0
        return rc, s

    def solve(self):
        L, info, x = M.lib(), M.Info(), np.empty(self.n)
        assert L.mi_osqp_solve(self._h, C.byref(info)) == 0
        assert L.mi_osqp_get_primal(self._h, x.ctypes.data_as(C.POINTER(C.c_double))) == 0
        return [info], x[None]

    def close(self):
        M.lib().mi_osqp_free(self._h)


@pytest.mark.parametrize("form", ["one_workgroup", "groups16", "grid40"])
def test_single_large_qp_forms_take_a_settings_update(form, monkeypatch):
    _env(monkeypatch, MI_OSQP_GLOBAL_XS="1", **({} if form == "grid40" else {"MI_OSQP_GROUPS": "0" if form == "one_workgroup" else "16"}))
    pr = PR.grid_qp(40) if form == "grid40" else {k: (v[:1] if k in ("Px", "Ax", "q", "l", "u") else v) for k, v in _data().items()}
    kw = dict(rho=0.7, eps_abs=1e-6, eps_rel=1e-6)
    s = _Single(pr)
    try:
        rc, now = s.update_settings(**kw)
        assert rc == 0 and (now.rho, now.eps_abs, now.eps_rel) == (0.7, 1e-6, 1e-6)
        assert s.update_settings(rho=-1.0)[0] == 2 and s.update_settings(sigma=1e-3)[0] == 2
        info, x = s.solve()
    finally:
        s.close()
    print(form, "iterations", info[0].iter, "rho updates", info[0].rho_updates)
    _compare(info, x, _oracle_batch(pr, [0], **kw), [0])


# ------------------------------------------------------------------ 7. continuous mode
@pytest.mark.parametrize("tile", [2, 4])
def test_rho_some_and_settings_in_the_continuous_mode(tile, monkeypatch):
    _env(monkeypatch, tile)
    pr = _data()
    even, odd = list(range(0, B, 2)), list(range(1, B, 2))         # every tile of 2 or 4 holds QPs of both lists
    rho = np.full(B, 0.1); rho[odd] = 0.01 * 3.0 ** np.array(odd)
    plain = _solve(_make())                                        # the iterating QPs without the call
    blocking = _make()
    blocking.update_rho_each(rho)
    upd = _solve(blocking)                                         # the updated QPs on a blocking handle
    _bitwise(upd, plain, idx=even)                                 # (a refactorisation with the rho in force is neutral)
    s = _make()
    assert s.stats()["tile"] == tile
    s.solve_begin_some(even)
    s.advance(1)
    fin = list(s.poll(True))
    assert fin == [] and s.running() == len(even)
    # refusals: all or nothing, nothing enqueued
    _refused(1, s.update_rho_some, [1, 0], [0.5, 0.5])             # 0 is running
    _refused(1, s.update_rho_some, [1, 3, 1], [0.5, 0.5, 0.5])     # repeated
    _refused(1, s.update_rho_some, [1, B], [0.5, 0.5])             # out of range
    _refused(1, s.update_rho_some, [-1], [0.5])
    for bad in (0.0, -2.0, float("nan")):
        _refused(2, s.update_rho_some, [1, 3], [0.5, bad])
    _refused(1, s.update_settings, max_iter=60)                    # QPs are running
    assert s.running() == len(even) and s.settings().max_iter == 4000
    s.update_rho_some(odd, rho[odd])                               # the idle tile partners, behind the advance in flight
    assert s.running() == len(even)
    s.solve_begin_some(odd)
    fin += _drain(s)
    assert sorted(fin) == list(range(B))
    got = (s.info_some(range(B)), s.primal_some(range(B)), s.dual_some(range(B)))
    print(f"tile {tile}: iterations {[i.iter for i in got[0]]}, rho {[i.rho for i in got[0]]}")
    _bitwise(got, plain, idx=even, skip=("status_polish",))
    _bitwise(got, upd, idx=odd, skip=("status_polish",))
    # idle: the settings update is accepted and the handle stays in the continuous mode
    assert s.update_settings(max_iter=60).max_iter == 60
    assert s.running() == 0 and s.primal_some([0]).shape == (1, N_VAR)          # (refused outside the mode)
    s.reinit_some(range(B), pr["Ax"], pr["l"], pr["u"])
    s.solve_begin_some(range(B))
    assert sorted(_drain(s)) == list(range(B))
    got60 = (s.info_some(range(B)), s.primal_some(range(B)), s.dual_some(range(B)))
    ref60 = _solve(_make(max_iter=60))
    assert max(i.iter for i in ref60[0]) == 60 and sum(i.iter == 60 for i in ref60[0]) >= 8        # (segments of gcd(60, 25, 100) = 5)
    _bitwise(got60, ref60)
    # a rho changed with the settings while idle in the mode is update_rho_some over all QPs
    assert s.update_settings(rho=0.7, max_iter=4000, warm_start=0).rho == 0.7          # (cold starts: the state of a fresh setup)
    assert s.running() == 0 and s.primal_some([0]).shape == (1, N_VAR)
    s.solve_begin_some(range(B))
    assert sorted(_drain(s)) == list(range(B))
    got07 = (s.info_some(range(B)), s.primal_some(range(B)), s.dual_some(range(B)))
    _bitwise(got07, _solve(_make(rho=0.7)))


def test_a_new_rho_ends_polishability():
    s = _make()
    s.solve_begin_some(range(B))
    _drain(s)
    assert all(i.exit_code == M.K_OPTIMAL for i in s.info_some(range(B)))
    s.update_rho_some([2, 5], [0.3, 0.3])
    _refused(1, s.polish_some, [2])
    s.polish_some([0, 1])
    s.advance(1)
    assert sorted(s.poll(True)) == [0, 1]


# ------------------------------------------------------------------ 8. other forms
def test_two_shards_on_one_device_equal_the_single_handle():
    pr = _data()
    rho = 0.01 * 3.0 ** np.arange(B)
    m = M.MultiBatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], devices=(0, 0))
    s = _make()
    for h in (m, s):
        now = h.update_settings(eps_abs=1e-5, eps_rel=1e-5, rho=0.3)
        assert (now.eps_abs, now.rho, now.adaptive_rho_interval) == (1e-5, 0.3, 100)
        _refused(2, h.update_settings, sigma=1e-3)
    rm = (m.solve(), m.primal(), m.dual()); rs = _solve(s)
    _bitwise(rm, rs)
    _compare(rs[0], rs[1], _oracle(eps_abs=1e-5, eps_rel=1e-5, rho=0.3), range(B))
    m.update_rho_each(rho); s.update_rho_each(rho)
    bad = rho.copy(); bad[B - 1] = 0.0                             # in the second shard: no shard changes
    _refused(2, m.update_rho_each, bad)
    assert [i.rho for i in m.info()] == list(rho) and m.settings().rho == 0.3
    rm = (m.solve(), m.primal(), m.dual()); rs = _solve(s)
    _bitwise(rm, rs)


def test_solve_device_after_an_update_matches_solve():
    import torch
    pr = _data()
    a, b = _make(), _make()
    for h in (a, b):
        h.update_settings(rho=0.7, eps_abs=1e-5, eps_rel=1e-5)
    ia, xa, _ = _solve(a)
    xd = torch.empty(B, pr["n"], dtype=torch.float64, device="cuda")
    st = torch.empty(B, dtype=torch.int32, device="cuda"); it = torch.empty_like(st)
    b.solve_device(xd, st, it)
    assert np.array_equal(xd.cpu().numpy(), xa)
    assert it.cpu().tolist() == [i.iter for i in ia] and st.cpu().tolist() == [i.status_val for i in ia]
    _bitwise(_result(b), (ia, xa, a.dual()))


def test_shim_update_sequence_matches_the_python_binding(tmp_path):
    out, log = run_shim_settings(build_shim_settings(tmp_path))
    assert out["init_ok"] is True, log
    assert out["before_init"] == ["FAILED_PRECONDITION"] * 14
    assert out["status"] == ["OK"] * 4 and out["refused"] == ["INVALID_ARGUMENT"] * 6 and out["after_init"] == ["OK"] * 14, out
    P = sp.csc_matrix(np.array([[4.0, 1.0], [1.0, 2.0]])); A = sp.csc_matrix(np.array([[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]]))
    l = np.array([1.0, 0.0, 0.0]); u = np.array([1.0, 0.7, 0.7])
    s = M.BatchSolver(P, P.data, np.array([1.0, 1.0]), A, A.data, l, u)
    c1 = s.solve()[0]; x1 = s.primal()[0].copy()
    s.update_settings(eps_abs=1e-6); s.update_settings(eps_rel=1e-6); s.update_settings(max_iter=3000); s.update_settings(rho=0.7)
    c2 = s.solve()[0]; x2, y2 = s.primal()[0].copy(), s.dual()[0].copy()
    c3 = s.solve()[0]
    assert out["codes"] == [M.EXIT_NAMES[c.exit_code] for c in (c1, c2, c3)]
    assert out["iters"] == [c1.iter, c2.iter, c3.iter] and c2.iter > 0
    for k, v in (("x1", x1), ("x2", x2), ("y2", y2)):
        assert np.array_equal(np.array(out[k]), v), k              # same library, same kernels: bitwise
