"""CPU: the settings, entry points and shim mapping of solution polishing (README "Polishing").  No GPU needed: the new
settings are validated before any device access, and the shim must reach the device (not refuse polish) in Init."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_solver_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_polish_defaults():
    s = M.default_settings()
    assert (s.polish, s.polish_refine_iter, s.delta) == (0, 3, 1e-6)
    assert M.Info().status_polish == 0


@pytest.mark.parametrize("bad", [dict(delta=0.0), dict(delta=-1e-6), dict(polish_refine_iter=-1), dict(polish=2)])
def test_invalid_polish_settings_are_refused_without_a_device(bad):
    P = sp.eye(2).tocsc(); A = sp.eye(2).tocsc()
    with pytest.raises(M.MiOsqpError) as e:
        M.BatchSolver(P, P.data, None, A, A.data, [0.0, 0.0], [1.0, 1.0], **{"polish": 1, **bad})
    assert e.value.code == 2          # MI_OSQP_ERR_INVALID_SETTINGS, before the device error a CPU machine would give


def test_polish_entry_points_are_exported():
    L = M.lib()
    for name in ("mi_osqp_batch_last_polish_stats", "mi_osqp_batch_get_polish_active"):
        assert hasattr(L, name)
    assert L.mi_osqp_batch_last_polish_stats(None, None, None, None) == 6         # MI_OSQP_ERR_NULL
    assert L.mi_osqp_batch_get_polish_active(None, None) == 6


def test_settings_struct_layout_matches_the_header():
    # the three polish fields follow `verbose`, the info field follows `rho`
    assert M.Settings.polish.offset == M.Settings.verbose.offset + 8
    assert M.Settings.delta.offset == M.Settings.polish.offset + 16 and C.sizeof(M.Settings) == M.Settings.delta.offset + 8
    assert M.Info.status_polish.offset == M.Info.rho.offset + 8


def build_shim_polish(tmp_path):
    M.lib()
    exe = str(tmp_path / "shim_polish")
    cmd = ["g++", "-std=c++17", "-O1", "-DNDEBUG", "-I", os.path.join(ROOT, "tests", "cpp", "eigen_standin"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "osqp_shim_polish.cpp"),
           "-L", os.path.join(ROOT, "osqp-solver_amd"), "-lmi_osqp", "-Wl,-rpath," + os.path.join(ROOT, "osqp-solver_amd"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run_shim_polish(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]), res.stdout


def test_shim_accepts_polish_and_reaches_the_device(tmp_path, gpu_available):
    if gpu_available:
        pytest.skip("a GPU is present")
    out, log = run_shim_polish(build_shim_polish(tmp_path))
    assert "UNIMPLEMENTED" not in log, log
    assert out["init_ok"] is False and "device error" in log          # Init went as far as the device
    assert out["code"] == "kUnknown"
