"""CPU: settings updates after setup (README "Settings updates") are exported, bound in Python and in the C++ facades,
refuse null arguments before any device access, and decide what may change - mi_osqp_settings_update_check, the host function
mi_osqp_*_update_settings consults before it touches anything - as OSQP 0.6.x's osqp_update_* do; the osqp++ shim has the
fourteen Update* methods with osqp-cpp's statuses."""
import json
import math
import os
import subprocess

import pytest

import osqp_solver_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCH = ["mi_osqp_batch_get_settings", "mi_osqp_batch_update_settings", "mi_osqp_batch_update_rho_each", "mi_osqp_batch_update_rho_some"]
SINGLE = ["mi_osqp_get_settings", "mi_osqp_update_settings"]
MULTI = ["mi_osqp_multi_batch_get_settings", "mi_osqp_multi_batch_update_settings", "mi_osqp_multi_batch_update_rho_each"]
ERR_SETTINGS, ERR_NULL = 2, 6

# a valid new value for every field that has an osqp_update_*; the fields without one
CHANGEABLE = dict(rho=0.7, max_iter=60, eps_abs=1e-6, eps_rel=1e-6, eps_prim_inf=1e-5, eps_dual_inf=1e-5, alpha=1.4,
                  scaled_termination=1, check_termination=10, warm_start=0, polish=1, polish_refine_iter=5, delta=1e-7, verbose=1)
FIXED = dict(sigma=1e-5, scaling=0, adaptive_rho=0, adaptive_rho_interval=50, adaptive_rho_tolerance=4.0)
# every value validate_settings (and tests/test_polish_settings.py) names as invalid, on a changeable field
INVALID = [dict(rho=0.0), dict(rho=-1.0), dict(rho=math.nan), dict(max_iter=0), dict(max_iter=-5), dict(check_termination=-1),
           dict(eps_abs=-1e-3), dict(eps_rel=-1e-3), dict(eps_abs=0.0, eps_rel=0.0), dict(eps_prim_inf=0.0), dict(eps_prim_inf=math.nan),
           dict(eps_dual_inf=0.0), dict(eps_dual_inf=-1.0), dict(alpha=0.0), dict(alpha=2.0), dict(alpha=math.nan),
           dict(scaled_termination=2), dict(warm_start=2), dict(warm_start=-1), dict(polish=2), dict(polish_refine_iter=-1),
           dict(delta=0.0), dict(delta=-1e-6), dict(delta=math.nan)]


def in_force():
    """what get_settings returns after a default setup: the "auto" interval resolved to 4 * check_termination"""
    return M.default_settings(adaptive_rho_interval=100)


def wanted(**fields):
    s = in_force()
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def test_every_settings_entry_point_is_exported_bound_and_declared():
    L = M.lib()
    header = open(os.path.join(ROOT, "include", "mi_osqp.h")).read()
    for name in ["mi_osqp_settings_update_check"] + BATCH + SINGLE + MULTI:
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes, f"{name} has no argtypes in osqp_solver_amd.lib()"
        assert name + "(" in header, name
    for meth in ("update_settings", "update_rho_each", "update_rho_some"):
        assert callable(getattr(M.BatchSolver, meth, None)), meth
    for meth in ("update_settings", "update_rho_each"):
        assert callable(getattr(M.MultiBatchSolver, meth, None)), meth
    assert callable(getattr(M.QPSolver, "update_settings", None))
    assert callable(M.HandleSettings()), "solver.settings must be callable: settings() returns the settings in force"
    facade = open(os.path.join(ROOT, "include", "mi_osqp", "qp_solver.hpp")).read()
    for text in ("void updateSettings(const mi_osqp_settings &s)", "void updateRho(const std::vector<double> &rho)",
                 "bool updateRho(const std::vector<long long> &ids, const std::vector<double> &rho)"):
        assert text in facade, text


def test_null_handles_and_arguments_give_err_null_without_a_gpu():
    L = M.lib()
    s = M.default_settings()
    assert L.mi_osqp_settings_update_check(None, None) == ERR_NULL
    assert L.mi_osqp_settings_update_check(s, None) == ERR_NULL and L.mi_osqp_settings_update_check(None, s) == ERR_NULL
    for name in ("mi_osqp_batch_get_settings", "mi_osqp_batch_update_settings", "mi_osqp_get_settings", "mi_osqp_update_settings",
                 "mi_osqp_multi_batch_get_settings", "mi_osqp_multi_batch_update_settings"):
        assert getattr(L, name)(None, None) == ERR_NULL, name
        assert getattr(L, name)(None, s) == ERR_NULL, name
    assert L.mi_osqp_batch_update_rho_each(None, None) == ERR_NULL
    assert L.mi_osqp_multi_batch_update_rho_each(None, None) == ERR_NULL
    assert L.mi_osqp_batch_update_rho_some(None, 0, None, None) == ERR_NULL


def test_unchanged_settings_are_accepted():
    assert M.settings_update_check(in_force(), in_force()) == 0
    assert M.settings_update_check(M.default_settings(adaptive_rho=0), M.default_settings(adaptive_rho=0)) == 0


@pytest.mark.parametrize("field", sorted(CHANGEABLE))
def test_each_changeable_field_changed_alone_is_accepted(field):
    assert getattr(in_force(), field) != CHANGEABLE[field]
    assert M.settings_update_check(in_force(), wanted(**{field: CHANGEABLE[field]})) == 0


def test_all_changeable_fields_at_once_and_a_rho_beyond_the_clamp_are_accepted():
    assert M.settings_update_check(in_force(), wanted(**CHANGEABLE)) == 0
    assert M.settings_update_check(in_force(), wanted(rho=1e9)) == 0 and M.settings_update_check(in_force(), wanted(rho=1e-9)) == 0


@pytest.mark.parametrize("field", sorted(FIXED))
def test_each_fixed_field_changed_alone_is_refused(field):
    assert getattr(in_force(), field) != FIXED[field]
    assert M.settings_update_check(in_force(), wanted(**{field: FIXED[field]})) == ERR_SETTINGS
    assert field in M.lib().mi_osqp_last_error().decode()
    # ... also next to a valid change of a changeable field
    assert M.settings_update_check(in_force(), wanted(eps_abs=1e-6, **{field: FIXED[field]})) == ERR_SETTINGS


def test_interval_zero_stands_for_the_resolved_auto_interval():
    assert M.settings_update_check(in_force(), wanted(adaptive_rho_interval=0)) == 0
    assert M.settings_update_check(in_force(), wanted(adaptive_rho_interval=0, check_termination=10)) == 0
    assert M.settings_update_check(in_force(), wanted(adaptive_rho_interval=-1)) == ERR_SETTINGS


@pytest.mark.parametrize("bad", INVALID, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_each_invalid_value_is_refused(bad):
    assert M.settings_update_check(in_force(), wanted(**bad)) == ERR_SETTINGS
    assert M.lib().mi_osqp_last_error().decode()


def test_one_zero_tolerance_is_valid_both_are_not():
    assert M.settings_update_check(in_force(), wanted(eps_abs=0.0)) == 0
    assert M.settings_update_check(in_force(), wanted(eps_rel=0.0)) == 0
    assert M.settings_update_check(in_force(), wanted(eps_abs=0.0, eps_rel=0.0)) == ERR_SETTINGS
    assert M.settings_update_check(wanted(eps_abs=0.0), wanted(eps_rel=0.0)) == 0         # (the result is what counts)
    assert M.settings_update_check(wanted(eps_abs=0.0), wanted(eps_abs=0.0, eps_rel=0.0)) == ERR_SETTINGS


def build_shim_settings(tmp_path):
    M.lib()
    exe = str(tmp_path / "shim_settings")
    cmd = ["g++", "-std=c++17", "-O1", "-DNDEBUG", "-I", os.path.join(ROOT, "tests", "cpp", "eigen_standin"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "osqp_shim_settings.cpp"),
           "-L", os.path.join(ROOT, "osqp-solver_amd"), "-lmi_osqp", "-Wl,-rpath," + os.path.join(ROOT, "osqp-solver_amd"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run_shim_settings(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]), res.stdout


def test_shim_update_calls_before_init_are_failed_precondition(tmp_path, gpu_available):
    out, log = run_shim_settings(build_shim_settings(tmp_path))
    assert out["before_init"] == ["FAILED_PRECONDITION"] * 14, out
    assert "UNIMPLEMENTED" not in log
    if not gpu_available:
        assert out["init_ok"] is False
