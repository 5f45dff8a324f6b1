"""CPU: the objective updates and dual warm starts (README "Objective updates") are exported, bound in Python, refuse null
arguments before any device access, and the osqp++ shim implements SetObjectiveVector, UpdateObjectiveMatrix,
UpdateObjectiveAndConstraintMatrices, SetDualWarmStart and SetWarmStart(x, y) with osqp-cpp's statuses."""
import json
import os
import subprocess

import pytest

import osqp_solver_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCH = ["mi_osqp_batch_update_q", "mi_osqp_batch_update_q_device", "mi_osqp_batch_update_P", "mi_osqp_batch_update_P_A",
         "mi_osqp_batch_warm_start_y", "mi_osqp_batch_update_q_some", "mi_osqp_batch_warm_start_y_some"]
SINGLE = ["mi_osqp_update_q", "mi_osqp_update_P", "mi_osqp_update_P_A", "mi_osqp_warm_start_y"]
MULTI = ["mi_osqp_multi_batch_update_q", "mi_osqp_multi_batch_update_P", "mi_osqp_multi_batch_update_P_A",
         "mi_osqp_multi_batch_warm_start_y"]
ERR_NULL = 6


def test_every_objective_entry_point_is_exported_bound_and_declared():
    L = M.lib()
    header = open(os.path.join(ROOT, "include", "mi_osqp.h")).read()
    for name in BATCH + SINGLE + MULTI:
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes, f"{name} has no argtypes in osqp_solver_amd.lib()"
        assert name + "(" in header, name
    for meth in ("update_q", "update_q_device", "update_q_some", "update_P", "update_P_A", "warm_start_y", "warm_start_y_some"):
        assert callable(getattr(M.BatchSolver, meth, None)), meth
    for meth in ("update_q", "update_P", "update_P_A", "warm_start_y"):
        assert callable(getattr(M.MultiBatchSolver, meth, None)), meth


def test_null_handles_and_arrays_give_err_null_without_a_gpu():
    L = M.lib()
    assert L.mi_osqp_batch_update_q(None, None) == ERR_NULL
    assert L.mi_osqp_batch_update_q_device(None, None, None) == ERR_NULL
    assert L.mi_osqp_batch_update_P(None, None, None, None) == ERR_NULL
    assert L.mi_osqp_batch_update_P_A(None, None, None, None, None, None, None) == ERR_NULL
    assert L.mi_osqp_batch_warm_start_y(None, None) == ERR_NULL
    assert L.mi_osqp_batch_update_q_some(None, 0, None, None) == ERR_NULL
    assert L.mi_osqp_batch_warm_start_y_some(None, 0, None, None) == ERR_NULL
    assert L.mi_osqp_update_q(None, None) == ERR_NULL
    assert L.mi_osqp_update_P(None, None, None, None) == ERR_NULL
    assert L.mi_osqp_update_P_A(None, None, None, None, None, None, None) == ERR_NULL
    assert L.mi_osqp_warm_start_y(None, None) == ERR_NULL
    assert L.mi_osqp_multi_batch_update_q(None, None) == ERR_NULL
    assert L.mi_osqp_multi_batch_update_P(None, None, None, None) == ERR_NULL
    assert L.mi_osqp_multi_batch_update_P_A(None, None, None, None, None, None, None) == ERR_NULL
    assert L.mi_osqp_multi_batch_warm_start_y(None, None) == ERR_NULL


def build_shim_objective(tmp_path):
    M.lib()
    exe = str(tmp_path / "shim_objective")
    cmd = ["g++", "-std=c++17", "-O1", "-DNDEBUG", "-I", os.path.join(ROOT, "tests", "cpp", "eigen_standin"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "osqp_shim_objective.cpp"),
           "-L", os.path.join(ROOT, "osqp-solver_amd"), "-lmi_osqp", "-Wl,-rpath," + os.path.join(ROOT, "osqp-solver_amd"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run_shim_objective(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]), res.stdout


def test_shim_objective_calls_before_init_are_failed_precondition(tmp_path, gpu_available):
    out, log = run_shim_objective(build_shim_objective(tmp_path))
    assert out["before_init"] == ["FAILED_PRECONDITION"] * 5, out
    assert "UNIMPLEMENTED" not in log
    if not gpu_available:
        assert out["init_ok"] is False
