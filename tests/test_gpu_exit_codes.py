"""GPU (-m gpu): every exit code of the termination check (kernels.hip check_body: E12 / E14) on every launch form.

The problem families are those of tests/exit_cases.py, pinned on the CPU by tests/test_exit_case_references.py: primal
infeasible by an interval argument, dual infeasible along a ray without curvature, and the three inaccurate codes plus
kMaxIterations from the same families at max_iter = 147 (cases whose oracle status has a margin).  Every QP of every
batch is compared with the oracle as test_gpu_parity._compare does (status, exit code, iteration count, rho updates, x
to 1e-6, pri_res / obj_val to 1e-6 relative; duals to test_gpu_parity's 1e-5) and, where the code carries no solution,
x AND y are NaN, obj_val is +1e30 (primal) / -1e30 (dual) and status_polish is 0.

Forms (check_body instantiations, kernels.hip MI_DISPATCH / launch_advance):
  tile1 / tile2 / tile4   check_kernel<BT, 512 or 1024, false>, one reduction class per QP of a tile
  global_g0               MI_OSQP_GLOBAL_XS, MI_OSQP_GROUPS=0: check_kernel<1, 512, true>, one workgroup
  wide_g16                MI_OSQP_GLOBAL_XS, 16 workgroups: check_kernel<1, 512, true, true>, grid_reduce (slots 4 and 5)
  continuous              check_body inlined into advance_kernel<BT, NT>
  shards / device_io      MultiBatchSolver on two shards of one device; solve_device outputs
Each form prints the exit codes it observed and compared, and asserts that they are all of 0..6."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exit_cases as EC                                                         # noqa: E402
import osqp_solver_amd as M                                                     # noqa: E402
from osqp_solver_amd import problems as PR                                      # noqa: E402
from test_gpu_continuous import _drain, _same                                   # noqa: E402
from test_gpu_parity import ST2EXIT, TOL_X, _compare, _oracle_batch             # noqa: E402

pytestmark = pytest.mark.gpu
NO_SOLUTION = (3, 4, -3, -4)
_REF = {}


@pytest.fixture(scope="module")
def base():
    return PR.random_box_qp(EC.BASE_B, **EC.BASE_SHAPE)


def _env(monkeypatch, tile=None, **env):
    for k in ("MI_OSQP_TILE", "MI_OSQP_GLOBAL_XS", "MI_OSQP_GROUPS", "MI_OSQP_GROUP_THREADS", "MI_OSQP_THREADS",
              "MI_OSQP_DENSE_TAIL", "MI_OSQP_HOST_RUIZ", "MI_OSQP_DEVICE_RUIZ"):
        monkeypatch.delenv(k, raising=False)
    if tile:
        monkeypatch.setenv("MI_OSQP_TILE", str(tile))
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _make(pr, **kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)


def _ref(key, pr, kw):
    """oracle results of a batch, solved once per module run: [(status, x, info, oracle)]"""
    if key not in _REF:
        ref = _oracle_batch(pr, range(pr["Ax"].shape[0]), **kw)
        _REF[key] = [(st, x, o.info(), o.y.copy()) for st, x, _, o in ref]
    return _REF[key]


def _check(info, x, y, ref, seen, polish_off=True):
    """all B QPs against the oracle; the exit codes go into `seen`"""
    B = len(ref)
    assert len(info) == B and x.shape[0] == B and y.shape[0] == B
    _compare(info, x, [(st, xo, io, None) for st, xo, io, _ in ref], range(B))
    for b, (st, xo, io, yo) in enumerate(ref):
        if st in NO_SOLUTION:
            assert np.all(np.isnan(xo)) and np.all(np.isnan(x[b])) and np.all(np.isnan(y[b])), b
            assert info[b].obj_val == (1e30 if st in (3, -3) else -1e30), (b, info[b].obj_val)
            assert info[b].status_polish == 0
        else:
            assert np.max(np.abs(y[b] - yo)) <= 1e-5, (b, np.max(np.abs(y[b] - yo)))
        if polish_off:
            assert info[b].status_polish == 0
        seen.add(int(info[b].exit_code))


def _table(form, seen, want=range(7)):
    print(f"\nexit codes observed and compared on {form}: " + ", ".join(f"{c} {M.EXIT_NAMES[c]}" for c in sorted(seen)))
    assert set(want) <= seen, (form, sorted(seen))


def _fields(i):
    return (i.iter, i.status_val, i.exit_code, i.obj_val, i.pri_res, i.dua_res, i.rho_updates, i.rho_estimate, i.rho, i.status_polish)


def _same_fields(a, b):
    return all((p == q) or (p != p and q != q) for p, q in zip(_fields(a), _fields(b)))


# ---- tiles of 1, 2, 4 QPs ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [1, 2, 4])
def test_rotated_kinds_in_mixed_tiles(tile, base, monkeypatch):
    """feas / pinf / dinf rotated through every class position of a tile (B = 11: ragged last tile), a batch whose first
    tile is infeasible throughout; scaling 10 and 0, scaled_termination 0 and 1, non-default certificate tolerances.
    Isolation: the feasible QPs of a mixed batch give BITWISE what they give between feasible neighbours (same tile, same
    B) - a reduction that leaks across the QP classes of a tile shows here even where it moves no status."""
    _env(monkeypatch, tile)
    seen = set()
    plain = EC.take(base, np.arange(EC.EXACT_B))
    for sname, kw in EC.EXACT_SETTINGS.items():
        batches = EC.exact_batches(base)
        if sname not in ("default", "s0"):
            batches = [batches[1], batches[4]]                  # one rotation and the infeasible tile for the other settings
        sp_ = _make(plain, **kw)
        ip, xp, yp = sp_.solve(), sp_.primal(), sp_.dual()
        for bname, pr, kinds in batches:
            ref = _ref(("exact", sname, bname), pr, kw)
            assert [r[0] for r in ref] == [EC.KIND_STATUS[k] for k in kinds]
            s = _make(pr, **kw)
            assert s.stats()["tile"] == tile
            info, x, y = s.solve(), s.primal(), s.dual()
            _check(info, x, y, ref, seen)
            for b, k in enumerate(kinds):
                if k == "feas":
                    assert _same_fields(info[b], ip[b]), (sname, bname, b, _fields(info[b]), _fields(ip[b]))
                    assert np.array_equal(x[b], xp[b]) and np.array_equal(y[b], yp[b]), (sname, bname, b)
    _table(f"tile{tile} (exact codes, rotated)", seen, want=(0, 1, 2))


@pytest.mark.parametrize("name", sorted(EC.ALL_CODES))
@pytest.mark.parametrize("tile", [1, 2, 4])
def test_all_codes_side_by_side_in_one_batch(tile, name, base, monkeypatch):
    """One handle, one max_iter (147: not a multiple of check_termination = 25; `ct0`: check_termination = 0, only the
    closing check runs), 13 QPs that end with the statuses 1, 2, 3, 4, -2, -3, -4 next to each other in the tiles."""
    _env(monkeypatch, tile)
    pr, kw, expect = EC.all_codes_batch(base, name)
    ref = _ref(("all", name), pr, kw)
    assert [r[0] for r in ref] == expect and set(expect) == set(EC.STATUSES)
    s = _make(pr, **kw)
    assert s.stats()["tile"] == tile and s.stats()["batch"] == 13
    seen = set()
    _check(s.solve(), s.primal(), s.dual(), ref, seen)
    _table(f"tile{tile} [{name}]", seen)


# ---- one QP with a global solve vector: one workgroup, and the dataflow form on 16 -----------------------------------------

@pytest.mark.parametrize("groups", [0, 16])
def test_global_vector_forms_every_code(groups, base, monkeypatch):
    """B = 1, MI_OSQP_GLOBAL_XS=1.  MI_OSQP_GROUPS=0: check_kernel<1, 512, true> in one workgroup; 16: the wide dataflow
    instantiation check_kernel<1, 512, true, true> on 16 workgroups (solver.hip derive_shape / launch_check) - every norm,
    sum and `viol` goes through grid_reduce, the exact decision through scratch slot 4, the approximate one through 5."""
    _env(monkeypatch, 1, MI_OSQP_GLOBAL_XS="1", MI_OSQP_GROUPS=str(groups))
    seen = set()
    for name in ("s10", "s0"):
        expect = [s[3] for s in EC.ALL_CODES[name][1]]
        slots = [expect.index(st) for st in EC.STATUSES]             # one QP per status
        for slot in slots:
            pr, kw, want = EC.all_codes_batch(base, name, slots=[slot])
            ref = _ref(("one", name, slot), pr, kw)
            assert [r[0] for r in ref] == want
            s = _make(pr, **kw)
            st = s.stats()
            assert st["tile"] == 1 and st["solve_groups"] == groups
            _check(s.solve(), s.primal(), s.dual(), ref, seen)
    _table(f"global vector, {groups} groups", seen)


@pytest.mark.parametrize("name", sorted(EC.GRID_CASES))
def test_grid_qp_on_the_dataflow_grid(name, monkeypatch):
    """The 40 x 40 grid through the single-large-QP path as in test_single_large_qp_infeasible_and_rho_updates_on_the_grid
    (which stays): the wide dataflow instantiation check_kernel<1, 512, true, true> on the default 32 workgroups."""
    _env(monkeypatch, None, MI_OSQP_GLOBAL_XS="1")
    pr, kw, want = EC.grid_case(PR.grid_qp(40), name)
    ref = _ref(("grid", name), pr, kw)
    assert ref[0][0] == want
    s = _make(pr, **kw)
    assert s.stats()["solve_groups"] > 1
    seen = set()
    _check(s.solve(), s.primal(), s.dual(), ref, seen)
    _table(f"grid 40 x 40, dataflow [{name}]", seen, want=(ST2EXIT[want],))


def test_dual_infeasible_with_32_bit_index_words():
    """grid_qp(150): n + m = 89 700, wide by size (32-bit index words, 128 workgroups).  The oracle needs a quarter of a
    minute for its setup, so its status is asserted here and not in the CPU file."""
    pr = EC.apply_kinds(PR.grid_qp(150), ["dinf"], grid=True)
    ref = _ref(("grid150", "dinf"), pr, {})
    assert ref[0][0] == -4
    s = _make(pr)
    st = s.stats()
    assert st["N"] == 89700 and st["tile"] == 1 and st["solve_groups"] > 1
    seen = set()
    _check(s.solve(), s.primal(), s.dual(), ref, seen)
    _table("grid 150 x 150, dataflow", seen, want=(2,))


# ---- continuous mode ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [1, 2, 4])
def test_continuous_mode_equals_blocking_bitwise_for_every_code(tile, base, monkeypatch):
    _env(monkeypatch, tile)
    pr, kw, expect = EC.all_codes_batch(base, "s10")
    B = len(expect)
    ref = _ref(("all", "s10"), pr, kw)
    assert [r[0] for r in ref] == expect
    blocking = _make(pr, **kw)
    ib, xb, yb = blocking.solve(), blocking.primal(), blocking.dual()
    seen = set()
    _check(ib, xb, yb, ref, set())
    s = _make(pr, **kw)
    assert s.stats()["tile"] == tile
    first, second = [0, 2, 3, 5, 8, 11], [1, 4, 6, 7, 9, 10, 12]           # partners of a tile begin at different launches
    s.solve_begin_some(first)
    s.advance(1); done = list(s.poll(True))
    s.advance(1); done += list(s.poll(True))
    s.solve_begin_some(second)
    done += _drain(s)
    assert sorted(done) == list(range(B))
    info, x, y = s.info_some(range(B)), s.primal_some(range(B)), s.dual_some(range(B))
    for b in range(B):
        _same(info[b], x[b], ib[b], xb[b])
        assert info[b].exit_code == ib[b].exit_code and info[b].status_polish == 0
        assert np.array_equal(y[b], yb[b], equal_nan=True)
        if expect[b] in NO_SOLUTION:
            assert np.all(np.isnan(x[b])) and np.all(np.isnan(y[b]))
    _check(info, x, y, ref, seen)
    _table(f"continuous, tile{tile}", seen)


# ---- shards, device I/O ------------------------------------------------------------------------------------------------

def test_shards_and_device_outputs(base, monkeypatch):
    import torch
    _env(monkeypatch, 2)
    pr, kw, expect = EC.all_codes_batch(base, "s10")
    B = len(expect)
    ref = _ref(("all", "s10"), pr, kw)
    one = _make(pr, **kw)
    i1, x1, y1 = one.solve(), one.primal(), one.dual()
    mb = M.MultiBatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], devices=(0, 0), **kw)
    assert len(mb.shards()) == 2
    im, xm, ym = mb.solve(), mb.primal(), mb.dual()
    seen = set()
    _check(im, xm, ym, ref, seen)
    for b in range(B):
        assert _same_fields(im[b], i1[b]), (b, _fields(im[b]), _fields(i1[b]))
    assert np.array_equal(xm, x1, equal_nan=True) and np.array_equal(ym, y1, equal_nan=True)
    _table("shards (0, 0)", seen)
    dev = _make(pr, **kw)
    xd = torch.full((B, pr["n"]), 7.0, dtype=torch.float64, device="cuda")
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda"); it = torch.full_like(st, -5)
    dev.solve_device(xd, st, it)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == expect and it.cpu().tolist() == [r[2].iter for r in ref]
    assert np.array_equal(xd.cpu().numpy(), x1, equal_nan=True)
    for b in range(B):
        assert bool(np.all(np.isnan(xd[b].cpu().numpy()))) == (expect[b] in NO_SOLUTION)
    seen = set()
    _check(dev.info(), dev.primal(), dev.dual(), ref, seen)
    _table("solve_device", seen)


# ---- sequences after an infeasible exit ----------------------------------------------------------------------------------

def _oracles(pr, kw):
    """([(status, x, info, y)] of a first solve, the oracle objects - to be taken through further calls)"""
    ref = _oracle_batch(pr, range(pr["Ax"].shape[0]), **kw)
    return [(st, x, io, o.y.copy()) for st, x, io, o in ref], [r[3] for r in ref]


@pytest.mark.parametrize("how", ["update_bounds", "update_A_bounds", "update_bounds_device"])
@pytest.mark.parametrize("tile", [1, 4])
def test_infeasible_then_feasible_bounds_follows_the_oracle(tile, how, base, monkeypatch):
    """An infeasible exit zeroes x, y and z of that QP (upstream's cold start in store_solution) while its neighbours keep
    their iterates; the bounds then go back to the generated boxes (the dinf QPs keep their P and q: with the box on x0
    they are bounded) and every QP is solved again: the oracle taken through the same calls."""
    import torch
    _env(monkeypatch, tile)
    _, pr, kinds = EC.exact_batches(base)[0]
    B = len(kinds)
    l2, u2 = base["l"][:B], base["u"][:B]
    s = _make(pr)
    first, ors = _oracles(pr, {})
    seen = set()
    _check(s.solve(), s.primal(), s.dual(), first, seen)
    assert seen == {0, 1, 2}
    if how == "update_bounds":
        s.update_bounds(l2, u2)
    elif how == "update_A_bounds":
        s.update_A_bounds(pr["Ax"], l2, u2)
    else:
        s.update_bounds_device(torch.tensor(l2, device="cuda"), torch.tensor(u2, device="cuda"))
    second = []
    for b, o in enumerate(ors):
        if how == "update_A_bounds":
            o.update(l2[b], PR.qp_matrices(pr, b)[1], u2[b])
        else:
            o.update_bounds_only(l2[b], u2[b])
        st, x = o.solve()
        second.append((st, x, o.info(), o.y.copy()))
    assert all(r[0] == 1 for r in second)
    _check(s.solve(), s.primal(), s.dual(), second, seen)


@pytest.mark.parametrize("tile", [1, 2])
def test_second_solve_and_reset_after_infeasible_exits(tile, base, monkeypatch):
    _env(monkeypatch, tile)
    _, pr, kinds = EC.exact_batches(base)[2]
    s = _make(pr)
    first, ors = _oracles(pr, {})
    i1, x1, y1 = s.solve(), s.primal().copy(), s.dual().copy()
    _check(i1, x1, y1, first, set())
    second = []
    for o in ors:                                           # nothing changed: the same code again, from the cold start
        st, x = o.solve()
        second.append((st, x, o.info(), o.y.copy()))
    assert [r[0] for r in second] == [EC.KIND_STATUS[k] for k in kinds]
    i2 = s.solve()
    _check(i2, s.primal(), s.dual(), second, set())
    s.reset()
    i3 = s.solve()
    fresh = _make(pr)
    i4 = fresh.solve()
    for b in range(len(kinds)):
        assert _same_fields(i3[b], i4[b]) and _same_fields(i3[b], i1[b]), b
    assert np.array_equal(s.primal(), fresh.primal(), equal_nan=True) and np.array_equal(s.dual(), fresh.dual(), equal_nan=True)
    assert np.array_equal(s.primal(), x1, equal_nan=True) and np.array_equal(s.dual(), y1, equal_nan=True)


def test_feasible_handle_made_dual_infeasible_by_objective_updates(base, monkeypatch):
    """update_P (explicit zeros, same pattern) + update_q + free rows.  The oracle has no update_P: as
    test_gpu_objective_update.py explains, OSQP's semantics coincide with a fresh setup for a handle that has not solved
    yet with scaling off - that case is compared with a fresh oracle; a handle that has solved (scaling on) must still
    report the code, NaN outputs and -1e30."""
    _env(monkeypatch, 2)
    B = 5
    feas = EC.take(base, np.arange(B))
    kinds = ["dinf", "feas", "dinf", "dinf", "feas"]
    target = EC.apply_kinds(feas, kinds)
    ref = _ref(("objupd", "s0"), target, dict(scaling=0))
    assert [r[0] for r in ref] == [EC.KIND_STATUS[k] for k in kinds]
    s = _make(feas, scaling=0)
    s.update_bounds(target["l"], target["u"]); s.update_P(target["Px"]); s.update_q(target["q"])
    seen = set()
    _check(s.solve(), s.primal(), s.dual(), ref, seen)
    s2 = _make(feas)
    assert all(i.status_val == 1 for i in s2.solve())
    s2.update_bounds(target["l"], target["u"]); s2.update_P(target["Px"]); s2.update_q(target["q"])
    info, x, y = s2.solve(), s2.primal(), s2.dual()
    for b, k in enumerate(kinds):
        assert info[b].status_val == EC.KIND_STATUS[k] and info[b].exit_code == ST2EXIT[EC.KIND_STATUS[k]]
        if k == "dinf":
            assert np.all(np.isnan(x[b])) and np.all(np.isnan(y[b])) and info[b].obj_val == -1e30


# ---- polish on -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [1, 2])
def test_only_optimal_qps_are_polished(tile, base, monkeypatch):
    _env(monkeypatch, tile)
    pr, kw, expect = EC.all_codes_batch(base, "s10")
    ref = _ref(("all", "s10"), pr, kw)
    off, on = _make(pr, **kw), _make(pr, polish=1, **kw)
    i0, i1 = off.solve(), on.solve()
    x0, y0, x1, y1 = off.primal(), off.dual(), on.primal(), on.dual()
    assert on.last_polish_stats()["polished"] == expect.count(1) and off.last_polish_stats()["polished"] == 0
    _check(i0, x0, y0, ref, set())
    for b, st in enumerate(expect):
        assert i1[b].status_val == st
        if st != 1:
            assert i1[b].status_polish == 0
            assert _same_fields(i1[b], i0[b]), (b, _fields(i1[b]), _fields(i0[b]))
            assert np.array_equal(x1[b], x0[b], equal_nan=True) and np.array_equal(y1[b], y0[b], equal_nan=True)
        else:
            assert i1[b].status_polish in (1, -1)
