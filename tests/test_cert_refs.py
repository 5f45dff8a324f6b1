"""CPU: the oracle-derived reference certificates of tests/cert_refs.py, which tests/test_gpu_certificates.py compares the
device's certificates with.

For every infeasible slot of exit_cases.ALL_CODES (all four settings), for the first rotation batch of
exit_cases.exact_batches under all five EXACT_SETTINGS and for the grid cases the GPU file uses: the two extra oracle
runs end with a solution at exactly k and k - 1 iterations (cert_refs._iterate asserts it), and the derived vector has
unit infinity norm, the signs of the bound-type projection and - where it lives in the caller's space - satisfies OSQP's
infeasibility conditions in the caller's data at the tolerance of the exit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_refs as CR                                                          # noqa: E402
import exit_cases as EC                                                         # noqa: E402
from oracle import oracle as O                                                  # noqa: E402
from osqp_solver_amd import problems as PR                                      # noqa: E402

GRID_NAMES = ("pinf", "dinf", "dinf_s0", "dinf_inacc")


@pytest.fixture(scope="module")
def base():
    return PR.random_box_qp(EC.BASE_B, **EC.BASE_SHAPE)


def _solve(pr, kw):
    out = []
    for b in range(pr["Ax"].shape[0]):
        P, A = PR.qp_matrices(pr, b)
        o = O.OracleQPSolver(P, pr["q"][b], A, pr["l"][b], pr["u"][b], **kw)
        st, _ = o.solve()
        out.append((st, int(o.info().iter)))
    return out


def _pin(key, pr, kw, expect):
    res = _solve(pr, kw)
    assert [r[0] for r in res] == expect
    refs = CR.references(key, pr, kw, [r[0] for r in res], [r[1] for r in res])
    assert sorted(refs) == [b for b, st in enumerate(expect) if st in CR.PRIMAL + CR.DUAL]
    for b, v in refs.items():
        assert v.shape == ((pr["m"] if expect[b] in CR.PRIMAL else pr["n"]),)
        CR.check_shape(v, pr, b, expect[b], exact=False, tol=1e-15)
        if not CR.leaves_scaled_space(kw):
            CR.check_conditions(v, pr, b, kw, expect[b])
    return refs


@pytest.mark.parametrize("name", sorted(EC.ALL_CODES))
def test_references_of_the_all_codes_batch(name, base):
    pr, kw, expect = EC.all_codes_batch(base, name)
    refs = _pin(("all", name), pr, kw, expect)
    assert {expect[b] for b in refs} == {3, 4, -3, -4}


@pytest.mark.parametrize("sname", sorted(EC.EXACT_SETTINGS))
def test_references_of_a_rotation_batch(sname, base):
    bname, pr, kinds = EC.exact_batches(base)[1]
    assert bname == "rot1"
    _pin(("exact", sname, bname), pr, EC.EXACT_SETTINGS[sname], [EC.KIND_STATUS[k] for k in kinds])


@pytest.mark.parametrize("name", GRID_NAMES)
def test_references_of_the_grid_cases(name):
    pr, kw, want = EC.grid_case(PR.grid_qp(40), name)
    _pin(("grid", name), pr, kw, [want])


def test_projection_and_space():
    l = np.array([-1e30, -1e30, 0.0, 0.0]); u = np.array([1e30, 1.0, 1e30, 1.0])
    assert CR.project(np.array([2.0, -3.0, -4.0, 5.0]), l, u).tolist() == [0.0, 0.0, -4.0, 5.0]
    assert CR.project(np.array([-2.0, 3.0, 4.0, -5.0]), l, u).tolist() == [0.0, 3.0, 0.0, -5.0]
    assert CR.leaves_scaled_space(dict(scaled_termination=1)) and not CR.leaves_scaled_space(dict(scaling=0, scaled_termination=1))
    assert not CR.leaves_scaled_space({})
