"""GPU (-m gpu): the infeasibility certificates (kernels.hip check_body, block E14; mi_osqp.h mi_osqp_get_prim_inf_cert) on
every launch form.

Problems are those of tests/exit_cases.py (random_box_qp(12, n=96, mg=64, nnz_per_row=6): n = 96, m = 160, so a stride
mix-up between n and m shows; grid_qp(40) for the global forms), the oracle results those test_gpu_exit_codes.py compares
with, the reference certificates those of tests/cert_refs.py (pinned on the CPU by tests/test_cert_refs.py).  Per form,
each QP:
  statuses -3 / 3   max|v| == 1.0 exactly; v == 0 on free rows, v <= 0 where only u is infinite, v >= 0 where only l is;
                    the dual certificate of that QP is all NaN
  statuses -4 / 4   max|v| == 1.0 exactly; the primal certificate of that QP is all NaN
  both, where the certificate is in the caller's space (scaled_termination = 0 or scaling = 0): OSQP's infeasibility
                    conditions in the caller's data at the tolerance of the exit (cert_refs.check_conditions)
  both, all settings: max|v - v_ref| <= 1e-6 (TOL_X of test_gpu_parity on a unit-norm vector) against the oracle-derived
                    reference; the largest difference of every form is printed
  any other status  both certificates all NaN
and x, y, info still pass test_gpu_exit_codes._check."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_refs as CR                                                          # noqa: E402
import exit_cases as EC                                                         # noqa: E402
import osqp_solver_amd as M                                                     # noqa: E402
from osqp_solver_amd import problems as PR                                      # noqa: E402
from test_gpu_continuous import _drain                                          # noqa: E402
from test_gpu_exit_codes import _check, _env, _make, _ref                       # noqa: E402
from test_gpu_parity import TOL_X                                               # noqa: E402

pytestmark = pytest.mark.gpu
TOL_CERT = TOL_X                       # 1e-6


@pytest.fixture(scope="module")
def base():
    return PR.random_box_qp(EC.BASE_B, **EC.BASE_SHAPE)


def _same_bits(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _check_certs(form, key, pr, kw, ref, info, pv, dv):
    """every QP of a solved batch: statuses as the oracle's, certificates as the module docstring says"""
    B = len(ref)
    assert pv.shape == (B, pr["m"]) and dv.shape == (B, pr["n"])
    statuses = [r[0] for r in ref]
    refs = CR.references(key, pr, kw, statuses, [r[2].iter for r in ref])
    worst = 0.0
    for b, st in enumerate(statuses):
        assert info[b].status_val == st, (form, b, info[b].status_val, st)
        if st in CR.PRIMAL:
            v = pv[b]
            assert np.all(np.isnan(dv[b])), (form, b)
        elif st in CR.DUAL:
            v = dv[b]
            assert np.all(np.isnan(pv[b])), (form, b)
        else:
            assert np.all(np.isnan(pv[b])) and np.all(np.isnan(dv[b])), (form, b, st)
            continue
        CR.check_shape(v, pr, b, st)
        if not CR.leaves_scaled_space(kw):
            CR.check_conditions(v, pr, b, kw, st)
        diff = float(np.max(np.abs(v - refs[b])))
        print(f"  {form} QP {b} status {st}: max|v - v_ref| = {diff:.3e}")
        worst = max(worst, diff)
        assert diff <= TOL_CERT, (form, b, st, diff)
    print(f"largest certificate difference on {form}: {worst:.3e}")
    return worst


def _solve_and_check(form, key, pr, kw, ref, s):
    info, x, y = s.solve(), s.primal(), s.dual()
    pv, dv = s.prim_inf_cert(), s.dual_inf_cert()
    _check(info, x, y, ref, set())
    _check_certs(form, key, pr, kw, ref, info, pv, dv)
    return info, pv, dv


# ---- tiles of 1, 2, 4 QPs ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["s10", "s10_st", "s0", "ct0"])
@pytest.mark.parametrize("tile", [1, 2, 4])
def test_all_codes_side_by_side(tile, name, base, monkeypatch):
    """13 QPs with all seven statuses next to each other in the tiles, a ragged last tile"""
    _env(monkeypatch, tile)
    pr, kw, expect = EC.all_codes_batch(base, name)
    ref = _ref(("all", name), pr, kw)
    assert [r[0] for r in ref] == expect
    s = _make(pr, **kw)
    assert s.stats()["tile"] == tile
    # before the first solve everything is NaN
    assert np.all(np.isnan(s.prim_inf_cert())) and np.all(np.isnan(s.dual_inf_cert()))
    _solve_and_check(f"tile{tile} [{name}]", ("all", name), pr, kw, ref, s)


@pytest.mark.parametrize("sname", ["default", "inf_tol"])
@pytest.mark.parametrize("tile", [1, 2, 4])
def test_rotated_kinds_and_an_infeasible_tile(tile, sname, base, monkeypatch):
    _env(monkeypatch, tile)
    kw = EC.EXACT_SETTINGS[sname]
    batches = EC.exact_batches(base)
    for bname, pr, kinds in (batches[1], batches[4]):
        ref = _ref(("exact", sname, bname), pr, kw)
        assert [r[0] for r in ref] == [EC.KIND_STATUS[k] for k in kinds]
        _solve_and_check(f"tile{tile} [{sname}, {bname}]", ("exact", sname, bname), pr, kw, ref, _make(pr, **kw))


@pytest.mark.parametrize("tile", [1, 4])
def test_streamed_state_gives_the_same_bits(tile, base, monkeypatch):
    """MI_OSQP_STREAM_STATE=1: the iterate that keeps the ADMM state in global memory leaves the same delta_x / delta_y"""
    _env(monkeypatch, tile)
    pr, kw, expect = EC.all_codes_batch(base, "s10")
    ref = _ref(("all", "s10"), pr, kw)
    monkeypatch.delenv("MI_OSQP_STREAM_STATE", raising=False)
    _, p0, d0 = _solve_and_check(f"tile{tile} resident state", ("all", "s10"), pr, kw, ref, _make(pr, **kw))
    monkeypatch.setenv("MI_OSQP_STREAM_STATE", "1")
    s = _make(pr, **kw)
    assert s.stats()["resident_state"] == 0
    _, p1, d1 = _solve_and_check(f"tile{tile} streamed state", ("all", "s10"), pr, kw, ref, s)
    assert _same_bits(p0, p1) and _same_bits(d0, d1)


# ---- one QP with a global solve vector -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pinf", "dinf", "dinf_s0", "dinf_inacc"])
@pytest.mark.parametrize("groups", [0, 16])
def test_grid_qp_on_the_global_forms(groups, name, monkeypatch):
    """grid_qp(40) with MI_OSQP_GLOBAL_XS=1: one workgroup (MI_OSQP_GROUPS=0), and the dataflow form on 16 workgroups, where
    tid / nthr of the certificate loop run over the grid"""
    _env(monkeypatch, 1, MI_OSQP_GLOBAL_XS="1", MI_OSQP_GROUPS=str(groups))
    pr, kw, want = EC.grid_case(PR.grid_qp(40), name)
    ref = _ref(("grid", name), pr, kw)
    assert ref[0][0] == want
    s = _make(pr, **kw)
    assert s.stats()["solve_groups"] == groups
    _solve_and_check(f"grid 40 x 40, {groups} groups [{name}]", ("grid", name), pr, kw, ref, s)


# ---- continuous mode, shards, device I/O -----------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [1, 2, 4])
def test_continuous_mode(tile, base, monkeypatch):
    """check_body inlined into advance_kernel, the certificates in pinned host memory: the *_some getters return bitwise what
    the blocking getters return for the same data - those of the same handle, which end the continuous mode, and those of
    a handle that solved the batch with mi_osqp_batch_solve"""
    _env(monkeypatch, tile)
    pr, kw, expect = EC.all_codes_batch(base, "s10")
    B = len(expect)
    ref = _ref(("all", "s10"), pr, kw)
    blocking = _make(pr, **kw)
    _, pb, db = _solve_and_check(f"tile{tile} blocking", ("all", "s10"), pr, kw, ref, blocking)
    s = _make(pr, **kw)
    s.solve_begin_some([0, 2, 3, 5, 8, 11])
    ids = list(range(B))
    assert np.all(np.isnan(s.prim_inf_cert_some(ids))) and np.all(np.isnan(s.dual_inf_cert_some(ids)))      # nothing has finished
    s.advance(1); done = list(s.poll(True))
    s.solve_begin_some([1, 4, 6, 7, 9, 10, 12])
    done += _drain(s)
    assert sorted(done) == ids
    info = s.info_some(ids)
    ps, ds = s.prim_inf_cert_some(ids), s.dual_inf_cert_some(ids)
    _check(info, s.primal_some(ids), s.dual_some(ids), ref, set())
    _check_certs(f"continuous, tile{tile}", ("all", "s10"), pr, kw, ref, info, ps, ds)
    assert _same_bits(ps, pb) and _same_bits(ds, db)
    order = [12, 3, 3, 0]
    assert _same_bits(s.prim_inf_cert_some(order), ps[order]) and _same_bits(s.dual_inf_cert_some(order), ds[order])
    with pytest.raises(M.MiOsqpError):
        s.prim_inf_cert_some([B])
    assert _same_bits(s.prim_inf_cert(), ps) and _same_bits(s.dual_inf_cert(), ds)        # (ends the continuous mode)
    with pytest.raises(M.MiOsqpError):
        s.dual_inf_cert_some([0])                                                         # not in the continuous mode


def test_shards_and_solve_device(base, monkeypatch):
    import torch
    _env(monkeypatch, 2)
    pr, kw, expect = EC.all_codes_batch(base, "s10")
    B = len(expect)
    ref = _ref(("all", "s10"), pr, kw)
    _, p1, d1 = _solve_and_check("one handle", ("all", "s10"), pr, kw, ref, _make(pr, **kw))
    mb = M.MultiBatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], devices=(0, 0), **kw)
    assert len(mb.shards()) == 2
    info = mb.solve()
    pm, dm = mb.prim_inf_cert(), mb.dual_inf_cert()
    _check_certs("shards (0, 0)", ("all", "s10"), pr, kw, ref, info, pm, dm)
    assert _same_bits(pm, p1) and _same_bits(dm, d1)
    dev = _make(pr, **kw)
    xd = torch.full((B, pr["n"]), 7.0, dtype=torch.float64, device="cuda")
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda"); it = torch.full_like(st, -5)
    dev.solve_device(xd, st, it)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == expect
    pd, dd = dev.prim_inf_cert(), dev.dual_inf_cert()
    _check_certs("solve_device", ("all", "s10"), pr, kw, ref, dev.info(), pd, dd)
    assert _same_bits(pd, p1) and _same_bits(dd, d1)


# ---- lifetime --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [1, 4])
def test_a_certificate_lives_until_the_next_finished_solve_of_its_qp(tile, base, monkeypatch):
    """Solve; give one primal infeasible QP its generated (feasible) bounds back - the update clears nothing -; solve again:
    that QP ends kOptimal and both of its certificates read NaN, nothing stale is served.  The other QPs solve a second
    time, and their certificates are those of that second solve.  Where it repeats the first one - the dual infeasible
    QPs: an infeasible exit cold-starts the QP, and they end after 25 iterations, before any rho update - the certificate
    is bitwise the one from before.  A primal infeasible QP whose rho was adapted in the first solve starts the second one
    with the adapted rho and ends at another iteration (the oracle: 500 then 275), so its certificate is a new vector:
    it must again have unit norm, the signs and satisfy OSQP's conditions."""
    _env(monkeypatch, tile)
    bname, pr, kinds = EC.exact_batches(base)[1]
    B = len(kinds)
    ref = _ref(("exact", "default", bname), pr, {})
    s = _make(pr)
    assert np.all(np.isnan(s.prim_inf_cert())) and np.all(np.isnan(s.dual_inf_cert()))
    i1, p1, d1 = _solve_and_check(f"tile{tile} first solve", ("exact", "default", bname), pr, {}, ref, s)
    b = kinds.index("pinf")
    l2, u2 = pr["l"].copy(), pr["u"].copy()
    l2[b], u2[b] = base["l"][b], base["u"][b]
    s.update_bounds(l2, u2)
    assert _same_bits(s.prim_inf_cert(), p1) and _same_bits(s.dual_inf_cert(), d1)
    s.warm_start_x(np.zeros((B, pr["n"])))
    assert _same_bits(s.prim_inf_cert(), p1) and _same_bits(s.dual_inf_cert(), d1)
    i2 = s.solve()
    p2, d2 = s.prim_inf_cert(), s.dual_inf_cert()
    assert i2[b].status_val == 1 and np.all(np.isnan(p2[b])) and np.all(np.isnan(d2[b]))
    now = dict(pr, l=l2, u=u2)
    repeated = 0
    for q, k in enumerate(kinds):
        if q == b:
            continue
        assert i2[q].status_val == EC.KIND_STATUS[k], (q, i2[q].status_val)
        if k == "feas":
            assert np.all(np.isnan(p2[q])) and np.all(np.isnan(d2[q]))
            continue
        v = p2[q] if k == "pinf" else d2[q]
        assert np.all(np.isnan(d2[q] if k == "pinf" else p2[q]))
        if i2[q].iter == i1[q].iter and i1[q].rho_updates == 0:
            assert _same_bits(p2[q], p1[q]) and _same_bits(d2[q], d1[q]), q
            repeated += 1
        else:
            CR.check_shape(v, now, q, i2[q].status_val)
            CR.check_conditions(v, now, q, {}, i2[q].status_val)
            assert not _same_bits(v, p1[q] if k == "pinf" else d1[q]), q           # (the second solve wrote the row again)
    assert repeated >= 2


@pytest.mark.parametrize("tile", [1, 4])
def test_fixed_rho_second_solve_keeps_rewrites_and_clears_certificates(tile, base, monkeypatch):
    """The lifetime rule where a second solve repeats the first: adaptive_rho = 0, rho = 10 (every QP of the rotation batch
    still ends with its exact code; an infeasible exit cold-starts the QP and rho does not move).  Between two solves one
    primal infeasible QP gets its generated, feasible bounds back and a second one has the bounds of its infeasible row
    moved by 1, so that it stays infeasible with other data.  After the second solve
      the first reads NaN in both certificates,
      the second holds the certificate of its NEW problem: compared with the oracle-derived reference of that problem
          (with rho fixed a fresh oracle on the new data takes the iterations of the second solve) - a row left over from
          the first solve would be the certificate of the old bounds,
      every other QP's certificates are bitwise the ones from before."""
    _env(monkeypatch, tile)
    kw = dict(adaptive_rho=0, rho=10.0)
    bname, pr, kinds = EC.exact_batches(base)[1]
    n = pr["n"]
    ref = _ref(("exact", "rho10", bname), pr, kw)
    assert [r[0] for r in ref] == [EC.KIND_STATUS[k] for k in kinds]
    s = _make(pr, **kw)
    i1, p1, d1 = _solve_and_check(f"tile{tile} fixed rho, first solve", ("exact", "rho10", bname), pr, kw, ref, s)
    pinf = [q for q, k in enumerate(kinds) if k == "pinf"]
    cleared, moved = pinf[0], pinf[1]
    l2, u2 = pr["l"].copy(), pr["u"].copy()
    l2[cleared], u2[cleared] = base["l"][cleared], base["u"][cleared]
    l2[moved, n] += 1.0; u2[moved, n] += 1.0
    now = dict(pr, l=l2, u=u2)
    ref2 = _ref(("exact", "rho10", bname, "moved"), now, kw)
    assert ref2[cleared][0] == 1 and ref2[moved][0] == -3
    s.update_bounds(l2, u2)
    assert _same_bits(s.prim_inf_cert(), p1) and _same_bits(s.dual_inf_cert(), d1)
    i2 = s.solve()
    p2, d2 = s.prim_inf_cert(), s.dual_inf_cert()
    assert i2[cleared].status_val == 1 and np.all(np.isnan(p2[cleared])) and np.all(np.isnan(d2[cleared]))
    assert i2[moved].status_val == -3 and i2[moved].iter == ref2[moved][2].iter
    want = CR.reference(now, moved, kw, -3, int(ref2[moved][2].iter))
    CR.check_shape(p2[moved], now, moved, -3)
    CR.check_conditions(p2[moved], now, moved, kw, -3)
    diff = float(np.max(np.abs(p2[moved] - want)))
    print(f"tile{tile} fixed rho, moved QP {moved}: max|v - v_ref| = {diff:.3e}; against the certificate of the old bounds "
          f"{float(np.max(np.abs(p1[moved] - want))):.3e}")
    assert diff <= TOL_CERT and np.all(np.isnan(d2[moved]))
    assert not _same_bits(p2[moved], p1[moved])
    for q in range(len(kinds)):
        if q not in (cleared, moved):
            assert i2[q].status_val == i1[q].status_val
            assert _same_bits(p2[q], p1[q]) and _same_bits(d2[q], d1[q]), q


def test_continuous_begin_and_reinit_withdraw_the_certificate_at_once(base, monkeypatch):
    """A QP that has not finished a solve reads NaN in the continuous mode too: from the begin of its next solve, and from a
    reinit of its slot, the *_some getters serve nothing of the previous solve - before any poll()."""
    _env(monkeypatch, 2)
    pr, kw, expect = EC.all_codes_batch(base, "s10")
    B = len(expect)
    ids = list(range(B))
    s = _make(pr, **kw)
    s.solve_begin_some(ids)
    assert sorted(_drain(s)) == ids
    i1, p1, d1 = s.info_some(ids), s.prim_inf_cert_some(ids), s.dual_inf_cert_some(ids)
    assert [i.status_val for i in i1] == expect
    q, r = expect.index(-3), expect.index(-4)
    s.update_A_bounds_some([q], pr["Ax"][[q]], pr["l"][[q]], pr["u"][[q]])          # an update clears nothing
    assert _same_bits(s.prim_inf_cert_some(ids), p1) and _same_bits(s.dual_inf_cert_some(ids), d1)
    s.reinit_some([q], pr["Ax"][[q]], pr["l"][[q]], pr["u"][[q]])
    s.solve_begin_some([r])
    p2, d2 = s.prim_inf_cert_some(ids), s.dual_inf_cert_some(ids)
    assert np.all(np.isnan(p2[q])) and np.all(np.isnan(d2[r]))
    keep = [b for b in ids if b not in (q, r)]
    assert _same_bits(p2[keep], p1[keep]) and _same_bits(d2[keep], d1[keep])
    assert s.info_some([r])[0].status_val == -4                                          # (the last report stays readable)
    assert _drain(s) == [r]
    i3 = s.info_some([r])[0]
    assert i3.status_val == -4
    v = s.dual_inf_cert_some([r])[0]
    CR.check_shape(v, pr, r, -4)
    CR.check_conditions(v, pr, r, kw, -4)
    if i3.iter == i1[r].iter and i1[r].rho_updates == 0:
        assert _same_bits(v, d1[r])
    assert np.all(np.isnan(s.prim_inf_cert_some([q])))
