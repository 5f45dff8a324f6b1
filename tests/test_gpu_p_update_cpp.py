"""GPU (-m gpu): the C++ facades' P updates (include/mi_osqp/qp_solver.hpp).  tests/cpp/p_update_facade.cpp compiles
BatchQPSolver's device forms and drives per-QP P updates through ContinuousQPSolver; its solutions must be the Python
binding's bit for bit - the same library runs underneath."""
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_solver_amd as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _drain(s, max_advances=400):
    for _ in range(max_advances):
        if not s.running():
            return
        s.advance(1)
        s.poll(True)
    raise AssertionError("continuous solve did not finish")


def test_the_facade_program_compiles_and_matches_the_python_binding_bitwise(tmp_path):
    M.lib()
    libdir = os.path.join(ROOT, "osqp-solver_amd")
    exe = str(tmp_path / "p_update_facade")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "p_update_facade.cpp"),
           "-L", libdir, "-lmi_osqp", "-pthread", "-Wl,-rpath," + libdir, "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["thrown"] == 4 and out["pattern_ok"] is True, out
    # the same calls through the Python binding
    P = sp.csc_matrix((np.array([4.0, 1.0, 3.0, 0.5, 2.0]), np.array([0, 0, 1, 1, 2]), np.array([0, 1, 3, 5])), shape=(3, 3))
    A = sp.csc_matrix((np.ones(6), np.array([0, 1, 0, 2, 0, 3]), np.array([0, 2, 4, 6])), shape=(4, 3))
    l, u = np.array([1.0, 0.0, 0.0, 0.0]), np.array([1.0, 0.7, 0.7, 0.7])
    tile = lambda a: np.tile(a, (2, 1))
    s = M.BatchSolver(P, tile(P.data), None, A, tile(A.data), tile(l), tile(u))
    s.update_P_some([1], np.array([[2.0, -0.5, 5.0, 1.5, 3.0]]))
    s.solve_begin_some([0, 1]); _drain(s)
    i01, x01 = s.info_some([0, 1]), s.primal_some([0, 1]).copy()
    s.update_P_A_bounds_some([0], np.array([[3.0, 0.25, 2.0, -0.75, 4.0]]), np.array([[1.0, 1.0, 2.0, 1.0, 0.5, 1.0]]),
                             l[None], np.array([[1.0, 0.6, 0.8, 0.9]]))
    s.solve_begin_some([0]); _drain(s)
    i2, x2 = s.info_some([0]), s.primal_some([0]).copy()
    assert out["codes"] == [i01[0].exit_code, i01[1].exit_code, i2[0].exit_code] == [0, 0, 0]
    assert out["iters"] == [i01[0].iter, i01[1].iter, i2[0].iter]
    for k, v in (("x0", x01[0]), ("x1", x01[1]), ("x2", x2[0])):
        assert np.array_equal(np.array(out[k]), v), k
    assert not np.array_equal(x01[0], x01[1]) and not np.array_equal(x01[0], x2[0])      # (the updates matter)
