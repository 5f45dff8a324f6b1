"""CPU: polishing on demand in the continuous mode (mi_osqp.h mi_osqp_batch_polish_some) is exported, declared, bound in
Python and in the C++ facade, and refuses null arguments before any device access."""
import os

import osqp_solver_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NULL = 6


def test_polish_some_is_exported_declared_and_bound():
    L = M.lib()
    assert hasattr(L, "mi_osqp_batch_polish_some")
    assert L.mi_osqp_batch_polish_some.argtypes, "mi_osqp_batch_polish_some has no argtypes in osqp_solver_amd.lib()"
    header = open(os.path.join(ROOT, "include", "mi_osqp.h")).read()
    assert "int mi_osqp_batch_polish_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids);" in header
    assert callable(getattr(M.BatchSolver, "polish_some", None))
    facade = open(os.path.join(ROOT, "include", "mi_osqp", "qp_solver.hpp")).read()
    assert "bool polish(const std::vector<long long> &ids)" in facade and "mi_osqp_batch_polish_some(" in facade


def test_null_arguments_give_err_null_without_a_gpu():
    L = M.lib()
    assert L.mi_osqp_batch_polish_some(None, 0, None) == ERR_NULL
    assert L.mi_osqp_batch_polish_some(None, 3, None) == ERR_NULL
