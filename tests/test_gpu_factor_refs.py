"""GPU (-m gpu): the device refactorisation (kernels.hip factor_kernel, tail_assemble_kernel, tail_kernel) held to the long-double
KKT solve of tests/factor_refs.py at every dense-tail size, on two patterns, on packed work lists and where a tail loses its
inertia.

One observable: kkt_solve_device, one call per right-hand side with (B, n + m) per call.  Every QP gets its Gaussian vector and
one unit vector per 16-row tile column of the tail, placed by the handle's own ordering() (factor_refs.rhs_set).  The reference
is built from the raw data, the handle's own scaling() and info().rho, once per (QP, scaling, rho); the four measures of a solve
(err_x, err_y, bwd_x, bwd_y) must stay within FACTOR_BOUND of the case (pattern, tail rows, rho) - 32 x the error of the fp64
twins, per measure (tests/test_factor_refs.py pins it).  Every case prints its worst ratio and where it occurred before it
asserts.  The measured ratios are in DESIGN.md section 6."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_refs as F                                                         # noqa: E402
import osqp_solver_amd as M                                                     # noqa: E402

pytestmark = pytest.mark.gpu
ENV = ("MI_OSQP_TILE", "MI_OSQP_GLOBAL_XS", "MI_OSQP_GROUPS", "MI_OSQP_DENSE_TAIL", "MI_OSQP_RELAX", "MI_OSQP_HOST_RUIZ",
       "MI_OSQP_DEVICE_RUIZ", "MI_OSQP_STREAM_FACTOR")

def make(pr, monkeypatch, tile, tail, **kw):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if tile:
        monkeypatch.setenv("MI_OSQP_TILE", str(tile))
    if tail is not None:
        monkeypatch.setenv("MI_OSQP_DENSE_TAIL", str(tail))
    s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)
    st = s.stats()
    assert (tile == 0 or st["tile"] == tile) and (tail is None or st["dense_tail_rows"] == tail), (st["tile"], st["dense_tail_rows"])
    return s


def device_solves(s, rhs):
    """[B, R, N] solutions of the right-hand sides rhs [B, R, N]: one kkt_solve_device per right-hand side"""
    import torch
    out = np.empty_like(rhs)
    for j in range(rhs.shape[1]):
        t = torch.tensor(np.ascontiguousarray(rhs[:, j]), device="cuda")
        sol = torch.full_like(t, np.nan)
        torch.cuda.synchronize()                                   # (the fill runs on torch's stream, the op on the handle's own)
        s.kkt_solve_device(t, sol)
        out[:, j] = sol.cpu().numpy()
    return out


_SYSTEMS = {}


def system(pr, b, D, E, c, rho):
    """the reference system of QP b, once per (data, scaling, rho)"""
    key = tuple(np.ascontiguousarray(v).tobytes() for v in (pr["Px"][b], pr["Ax"][b], pr["l"][b], pr["u"][b], D, E)) + (float(c), float(rho))
    if key not in _SYSTEMS:
        _SYSTEMS[key] = F.system_of(pr, b, D, E, c, rho)
    return _SYSTEMS[key]


def right_hand_sides(s, k, pattern):
    """([B, R, N] right-hand sides, the R labels): factor_refs.rhs_set of every QP in the handle's own elimination order - which
    is the recorded one the twins were measured in"""
    perm = s.ordering()
    np.testing.assert_array_equal(perm, F.handle_order(pattern, k))
    sets = [F.rhs_set(perm, k, F.seed_of(k, b)) for b in range(s.B)]
    return np.stack([r for r, _ in sets]), sets[0][1]


def check(s, pr, pattern, k, rho, label, qps=None, sols=None, rhs=None):
    """Solve every right-hand side on every QP; compare the QPs `qps` (default: all) with the reference at the handle's scaling
    and at rho [B], which info() must report.  Returns the solutions."""
    qps = list(range(s.B)) if qps is None else list(qps)
    D, E, c = s.scaling()
    got_rho = [i.rho for i in s.info()]
    assert got_rho == [float(r) for r in rho], (label, got_rho, list(rho))
    rhs, labels = right_hand_sides(s, k, pattern) if rhs is None else rhs
    sols = device_solves(s, rhs) if sols is None else sols
    worst, where = 0.0, None
    for b in qps:
        sy = system(pr, b, D[b], E[b], c[b], rho[b])
        name = F.case_name(pattern, k, rho[b])
        for r, sol, lab in zip(rhs[b], sols[b], labels):
            ratio, m = F.ratio(sy.measures(sol, r), name)
            if not ratio < worst:
                worst, where = ratio, (b, lab, m, name)
    print(f"factor {label}: worst ratio {worst:.3f} at {where}")
    assert worst <= 1.0, (label, worst, where)
    return sols


# ------------------------------------------------------------------ a. every tail size, three states
@pytest.mark.parametrize("k", F.TAILS)
def test_every_tail_size(k, monkeypatch):
    """tail_kernel<1, 4> up to 128 rows, <2, 4> up to 256 (the panel staged once), <3, 4> at 320 and 384 (the first sizes with
    the panel staged in halves), <4, 4> at 448 and 512; odd and even k / 64 of the product's deal.  After setup (rho 0.1); after
    update_rho_each (a refactorisation of all four at once) and update_rho_some of QPs 1 and 2 (a device work list with
    unlisted neighbours); after refactor_device(), bitwise what it was before."""
    pr = F.data("box")
    s = make(pr, monkeypatch, 1, k)
    rhs = right_hand_sides(s, k, "box")
    check(s, pr, "box", k, [F.RHO0] * F.BOX_B, f"box k {k} setup", rhs=rhs)
    rho = np.array(F.RHOS)
    s.update_rho_each(rho)
    check(s, pr, "box", k, rho, f"box k {k} update_rho_each", rhs=rhs)
    for b, r in F.RHO_SOME:
        rho[b] = r
    s.update_rho_some([b for b, _ in F.RHO_SOME], [r for _, r in F.RHO_SOME])
    before = check(s, pr, "box", k, rho, f"box k {k} update_rho_some", rhs=rhs)
    s.refactor_device()
    after = device_solves(s, rhs[0])
    np.testing.assert_array_equal(before, after)
    check(s, pr, "box", k, rho, f"box k {k} refactor_device", sols=after, rhs=rhs)
    s.close()


@pytest.mark.parametrize("k", F.CLASS_TAILS)
def test_after_new_values_on_the_device(k, monkeypatch):
    """update_P_A_bounds_device with other values: the device Ruiz runs ahead of the factor"""
    import torch
    pr, new = F.data("box"), F.data("other")
    s = make(pr, monkeypatch, 1, k)
    before = s.scaling()
    Pp, Pi = s.P_upper_pattern()
    assert np.array_equal(Pp, pr["P"].indptr) and np.array_equal(Pi, pr["P"].indices)        # (P is passed as its upper triangle)
    s.update_P_A_bounds_device(*(torch.tensor(new[key], device="cuda") for key in ("Px", "Ax", "l", "u")))
    assert not np.array_equal(before[0], s.scaling()[0])
    check(s, new, "box", k, [F.RHO0] * F.BOX_B, f"box k {k} update_P_A_bounds_device")
    s.close()


# ------------------------------------------------------------------ b. the GOMP pattern
@pytest.mark.parametrize("k", F.GOMP_TAILS)
def test_gomp_pattern(k, monkeypatch):
    """structural zeros in S and a tail that cuts through supernodes; free rows at RHO_MIN and equality rows at 1e3 rho"""
    pr = F.data("gomp")
    s = make(pr, monkeypatch, 1, k)
    check(s, pr, "gomp", k, [F.RHO0] * F.GOMP_B, f"gomp k {k} setup")
    s.update_rho_each(np.array(F.GOMP_RHO_EACH))
    check(s, pr, "gomp", k, F.GOMP_RHO_EACH, f"gomp k {k} update_rho_each")
    s.close()


# ------------------------------------------------------------------ c. packed work lists
def packed_sample(B, tile):
    """the first tile, the middle tile, the last full tile and the lone last QP"""
    assert B % tile == 1
    mid = (B // tile // 2) * tile
    return sorted({*range(tile), *range(mid, mid + tile), *range(B - 1 - tile, B - 1), B - 1})


@pytest.mark.parametrize("tile,k", [(2, 0), (2, 64), (4, 0), (4, 64)], ids=lambda v: str(v))
def test_packed_work_lists(tile, k, monkeypatch):
    """B = 4 x CU count + 1 QPs of n = 96, m = 160: a work list longer than the CU count makes device_refactor_slots pack kbt =
    tile QPs per workgroup (its `nq <= n_cus` rule - this case rests on it), so factor_kernel<2> / <4> and the interleaved
    addressing of the tail kernels run, with a last workgroup that is padded.  At setup and after update_rho_each with rho
    cycling through RHOS.  A fixed sample of QPs is held to the bound on every right-hand side.  Every other QP is held to the
    bound through its Gaussian vector, in the two residual measures, which need K alone: the tiles of 2 and 4 do not promise the
    bits of a tile of 1 (they differ on every QP), and a reference solve of 1000 more QPs would take this case 45 s.  (All forms
    are forced: at this B the default is a tile of 1 with 64 tail rows, which packs nothing.)"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 4 * cus + 1
    assert B > cus
    pr = F.data(f"small{B}")
    s = make(pr, monkeypatch, tile, k)
    sample = packed_sample(B, tile)
    rhs = right_hand_sides(s, k, "small")
    rho = np.array([F.RHOS[b % 4] for b in range(B)])
    rest = np.setdiff1d(np.arange(B), sample)
    for state in ("setup", "update_rho_each"):
        if state == "update_rho_each":
            s.update_rho_each(rho)
        now = rho if state == "update_rho_each" else np.full(B, F.RHO0)
        sols = check(s, pr, "small", k, now, f"packed tile {tile} k {k} {state}", sample, rhs=rhs)
        D, E, c = s.scaling()
        worst, where = 0.0, None
        for b in rest:
            sy = F.system_of(pr, b, D[b], E[b], c[b], now[b])
            ratio, m = F.ratio(sy.residuals(sols[b, 0], rhs[0][b, 0]), F.case_name("small", k, now[b]))
            if not ratio < worst:
                worst, where = ratio, (int(b), m)
        print(f"factor packed tile {tile} k {k} {state}, the other {len(rest)} QPs: worst ratio {worst:.3f} at {where}")
        assert worst <= 1.0, (state, worst, where)
    s.close()


# ------------------------------------------------------------------ d. inertia lost in the tail
@pytest.mark.parametrize("k", F.CLASS_TAILS)
def test_inertia_lost_in_the_tail(k, monkeypatch):
    """One case per tail_kernel instantiation the lost-inertia tests at 64 rows do not reach.  QP 2 has the diagonal of P lowered
    on four variables that ordering() places in the tail, so far that K keeps inertia (n, m) at rho = 10 and loses it at 1e-3
    (factor_refs.inertia_batch; both signs verified here with the handle's own scaling): the leading factor keeps its pivots
    and the wrong ones are met by tail_kernel's own count.  At rho = 10 all four QPs meet the bound; after update_rho_each with
    1e-3 for QP 2 its solve ends kNonConvex (-7) with NaN x and y, and its neighbours' KKT solves and solves are bitwise those
    of a handle that never held the change."""
    box = F.data("box")
    kw = dict(rho=F.INERTIA_RHO[0])
    plain = make(box, monkeypatch, 1, k, **kw)
    perm = plain.ordering()
    bad, variables, amount = F.inertia_batch(perm, k)
    print(f"k = {k}: diagonal of P lowered by {amount} on variables {variables}")
    s = make(bad, monkeypatch, 1, k, **kw)
    np.testing.assert_array_equal(s.ordering(), perm)
    D, E, c = s.scaling()
    q = F.INERTIA_QP
    for rho, keeps in zip(F.INERTIA_RHO, (True, False)):
        assert (F.reduced_min_eig(F.system_of(bad, q, D[q], E[q], c[q], rho)) > 0) == keeps, rho
    rhs = right_hand_sides(s, k, "box")
    check(s, bad, "box", k, [F.INERTIA_RHO[0]] * F.BOX_B, f"inertia k {k} at rho 10", rhs=rhs)
    rho = np.full(F.BOX_B, F.INERTIA_RHO[0])
    rho[q] = F.INERTIA_RHO[1]
    others = [b for b in range(F.BOX_B) if b != q]
    results = []
    for h in (s, plain):
        h.update_rho_each(rho)
        sols = device_solves(h, rhs[0][:, :1])
        info = h.solve()
        results.append((sols, info, h.primal(), h.dual()))
    (sols, info, x, y), (sols0, info0, x0, y0) = results
    assert info[q].status_val == -7 and np.all(np.isnan(x[q])) and np.all(np.isnan(y[q])), (info[q].status_val, x[q][:4])
    for b in others:
        assert (info[b].status_val, info[b].iter) == (info0[b].status_val, info0[b].iter), b
    np.testing.assert_array_equal(sols[others], sols0[others])
    np.testing.assert_array_equal(x[others], x0[others])
    np.testing.assert_array_equal(y[others], y0[others])
    s.close()
    plain.close()
