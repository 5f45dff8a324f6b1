"""include/osqp++.h: primal_infeasibility_certificate() / dual_infeasibility_certificate() of the osqp-cpp-shaped shim
(tests/cpp/osqp_shim_certificates.cpp, compiled against tests/cpp/eigen_standin like the other shim programs).

A two-variable primal infeasible QP - x0 + x1 in [3, 4] over the unit box, whose certificate is (-1, 1, 1) up to the
signs' magnitudes: a negative multiplier on the row whose lower bound cannot be met, positive ones on the two upper
bounds that stand in its way - and a one-variable unbounded one - minimise x subject to x <= 0, whose ray is -1."""
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_solver_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    M.lib()
    exe = str(tmp_path / "shim_certificates")
    cmd = ["g++", "-std=c++17", "-O1", "-DNDEBUG", "-I", os.path.join(ROOT, "tests", "cpp", "eigen_standin"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "osqp_shim_certificates.cpp"),
           "-L", os.path.join(ROOT, "osqp-solver_amd"), "-lmi_osqp", "-Wl,-rpath," + os.path.join(ROOT, "osqp-solver_amd"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def _run(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]), res.stdout


def _vec(a):
    return np.array([np.nan if v is None else v for v in a], float)


def test_shim_certificate_accessors_compile_and_are_empty_before_init(tmp_path, gpu_available):
    out, log = _run(_build(tmp_path))
    assert out["uninitialised_entries"] == 0
    if not gpu_available:
        assert out["init_ok"] is False and out["pinf"] is None and out["dinf"] is None


@pytest.mark.gpu
def test_shim_certificates_have_unit_norm_and_the_expected_signs(tmp_path):
    out, log = _run(_build(tmp_path))
    assert out["init_ok"] is True, log
    p, d = out["pinf"], out["dinf"]
    # before the first Solve(): NaN, of the right lengths
    assert np.all(np.isnan(_vec(p["prim_before"]))) and len(p["prim_before"]) == 3 and len(p["dual_before"]) == 2
    assert np.all(np.isnan(_vec(p["dual_before"]))) and np.all(np.isnan(_vec(d["prim_before"]))) and np.all(np.isnan(_vec(d["dual_before"])))
    # primal infeasible
    assert p["code"] == "kPrimalInfeasible"
    v = _vec(p["prim"])
    assert np.max(np.abs(v)) == 1.0 and v[0] < 0 and v[1] > 0 and v[2] > 0, v
    l, u = np.array([3.0, 0.0, 0.0]), np.array([4.0, 1.0, 1.0])
    A = np.array([[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]])
    assert u @ np.maximum(v, 0) + l @ np.minimum(v, 0) < -1e-4 and np.max(np.abs(A.T @ v)) < 1e-4
    assert np.all(np.isnan(_vec(p["dual"]))) and np.all(np.isnan(_vec(p["x"])))
    # dual infeasible
    assert d["code"] == "kDualInfeasible"
    assert _vec(d["dual"]).tolist() == [-1.0]
    assert np.all(np.isnan(_vec(d["prim"]))) and np.all(np.isnan(_vec(d["x"])))
    # the same library through the Python binding: bitwise
    s = M.QPSolver((l, sp.csc_matrix(A), u), sp.identity(2, format="csc"), q=np.zeros(2))
    code, _ = s.solve()
    assert M.EXIT_NAMES[code] == p["code"] and s.info().iter == p["iter"]
    assert np.array_equal(s.prim_inf_cert(), v) and np.all(np.isnan(s.dual_inf_cert()))
    s1 = M.QPSolver((np.array([-1e30]), sp.csc_matrix(np.array([[1.0]])), np.array([0.0])), sp.csc_matrix(([0.0], ([0], [0])), shape=(1, 1)),
                    q=np.array([1.0]))
    code, _ = s1.solve()
    assert M.EXIT_NAMES[code] == d["code"] and s1.info().iter == d["iter"]
    assert s1.dual_inf_cert().tolist() == [-1.0] and np.all(np.isnan(s1.prim_inf_cert()))
