"""CPU: the device-resident and per-QP P updates (README "Objective updates") are exported with the signatures of mi_osqp.h,
bound in Python, present in the facades, and refuse null arguments before any device access."""
import ctypes as C
import os
import re

import osqp_solver_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NULL = 6

DECLARED = {
    "mi_osqp_batch_get_P_upper_pattern":
        "int mi_osqp_batch_get_P_upper_pattern(mi_osqp_batch *h, int64_t *colptr, int64_t *rowidx, int64_t *nnz_out);",
    "mi_osqp_batch_update_P_device":
        "int mi_osqp_batch_update_P_device(mi_osqp_batch *h, const double *d_Pv, void *stream);",
    "mi_osqp_batch_update_P_A_bounds_device":
        "int mi_osqp_batch_update_P_A_bounds_device(mi_osqp_batch *h, const double *d_Pv, const double *d_Av, const double *d_l, "
        "const double *d_u, void *stream);",
    "mi_osqp_batch_update_P_some":
        "int mi_osqp_batch_update_P_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *P_val);",
    "mi_osqp_batch_update_P_A_bounds_some":
        "int mi_osqp_batch_update_P_A_bounds_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *P_val, "
        "const double *A_val, const double *l, const double *u);",
}


def _header_without_comments():
    text = open(os.path.join(ROOT, "include", "mi_osqp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"\s+", " ", text).replace(" )", ")")


def test_entry_points_are_exported_bound_and_declared():
    L = M.lib()
    header = _header_without_comments()
    ip, dp, vp, i64 = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_void_p, C.c_int64
    bound = {"mi_osqp_batch_get_P_upper_pattern": [vp, ip, ip, ip], "mi_osqp_batch_update_P_device": [vp] * 3,
             "mi_osqp_batch_update_P_A_bounds_device": [vp] * 6, "mi_osqp_batch_update_P_some": [vp, i64, ip, dp],
             "mi_osqp_batch_update_P_A_bounds_some": [vp, i64, ip, dp, dp, dp, dp]}
    for name, decl in DECLARED.items():
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes == bound[name], name
        assert decl in header, decl


def test_null_handle_gives_err_null_without_a_gpu():
    L = M.lib()
    v = (C.c_double * 4)()
    ids = (C.c_int64 * 2)(0, 1)
    nnz = C.c_int64(-5)
    dev = C.cast(v, C.c_void_p)
    assert L.mi_osqp_batch_get_P_upper_pattern(None, ids, ids, C.byref(nnz)) == ERR_NULL
    assert nnz.value == -5
    assert L.mi_osqp_batch_update_P_device(None, dev, None) == ERR_NULL
    assert L.mi_osqp_batch_update_P_A_bounds_device(None, dev, dev, dev, dev, None) == ERR_NULL
    assert L.mi_osqp_batch_update_P_some(None, 2, ids, v) == ERR_NULL
    assert L.mi_osqp_batch_update_P_A_bounds_some(None, 2, ids, v, v, v, v) == ERR_NULL


def test_null_arrays_are_refused_before_the_handle_is_looked_at():
    """The block of zeros standing in for the handle is never read: a refused call cannot have enqueued anything."""
    L = M.lib()
    fake = C.cast((C.c_char * 64)(), C.c_void_p)
    v = (C.c_double * 4)()
    ids = (C.c_int64 * 2)(0, 1)
    assert L.mi_osqp_batch_get_P_upper_pattern(fake, ids, ids, None) == ERR_NULL
    assert L.mi_osqp_batch_update_P_device(fake, None, None) == ERR_NULL
    assert L.mi_osqp_batch_update_P_some(fake, 2, ids, None) == ERR_NULL
    for missing in range(4):
        args = [v, v, v, v]
        args[missing] = None
        assert L.mi_osqp_batch_update_P_A_bounds_some(fake, 2, ids, *args) == ERR_NULL, missing


def test_the_mixed_null_rule_of_update_P_A_bounds_device():
    """P alone, (A, l, u) alone or all four: every other combination is MI_OSQP_ERR_NULL, decided before the handle is read."""
    L = M.lib()
    fake = C.cast((C.c_char * 64)(), C.c_void_p)
    v = (C.c_double * 4)()
    dev = C.cast(v, C.c_void_p)
    for mask in range(16):
        Pv, Av, l, u = (dev if mask & (1 << k) else None for k in range(4))
        rest = [x is not None for x in (Av, l, u)]
        if all(rest) or (Pv is not None and not any(rest)):
            continue                                           # the three accepted forms need a device
        assert L.mi_osqp_batch_update_P_A_bounds_device(fake, Pv, Av, l, u, None) == ERR_NULL, mask


def test_python_methods_layer_and_facades_exist():
    for meth in ("P_upper_pattern", "update_P_device", "update_P_A_bounds_device", "update_P_some", "update_P_A_bounds_some"):
        assert callable(getattr(M.BatchSolver, meth, None)), meth
    import inspect
    from osqp_solver_amd import qp_layer as QL
    assert list(inspect.signature(QL.qp_layer).parameters) == ["solver", "q", "Ax", "l", "u", "Px"]
    assert inspect.signature(QL.qp_layer).parameters["Px"].default is None
    layer = open(os.path.join(ROOT, "osqp-solver_amd", "qp_layer.py")).read()
    for text in ("update_P_A_bounds_device", "update_A_bounds_device", "dict(dP=dP)"):
        assert text in layer, text
    assert "there is no device-side P update" not in layer
    facade = open(os.path.join(ROOT, "include", "mi_osqp", "qp_solver.hpp")).read()
    for text in ("void updatePDevice(const double *d_Pv, void *stream = nullptr)",
                 "void updateDevice(const double *d_Pv, const double *d_Av, const double *d_l, const double *d_u, void *stream = nullptr)",
                 "void updateP(const std::vector<long long> &ids, const std::vector<const QPVector *> &Ps)",
                 "mi_osqp_batch_update_P_A_bounds_some"):
        assert text in facade, text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Not covered: per-QP P updates in the continuous mode, device-resident P input." not in design


C_PROGRAM = r"""
/* include/mi_osqp.h against the compiled library: every entry point is assigned to a pointer of the specified type (another
   type does not compile under -Werror), linked, and called with a null handle, which needs no device. */
#include <stdint.h>
#include <stdio.h>
#include "mi_osqp.h"
int main(void) {
  int (*pat)(mi_osqp_batch *, int64_t *, int64_t *, int64_t *) = mi_osqp_batch_get_P_upper_pattern;
  int (*pd)(mi_osqp_batch *, const double *, void *) = mi_osqp_batch_update_P_device;
  int (*pabd)(mi_osqp_batch *, const double *, const double *, const double *, const double *, void *) = mi_osqp_batch_update_P_A_bounds_device;
  int (*ps)(mi_osqp_batch *, int64_t, const int64_t *, const double *) = mi_osqp_batch_update_P_some;
  int (*pabs)(mi_osqp_batch *, int64_t, const int64_t *, const double *, const double *, const double *, const double *) =
      mi_osqp_batch_update_P_A_bounds_some;
  double v[4] = {0, 0, 0, 0};
  int64_t ids[2] = {0, 1}, nnz = 7;
  printf("%d %d %d %d %d %d\n", pat(0, 0, 0, &nnz), pd(0, v, 0), pabd(0, v, v, v, v, 0), ps(0, 2, ids, v), pabs(0, 2, ids, v, v, v, v), (int)nnz);
  return 0;
}
"""


def test_header_declarations_compile_link_and_run_against_the_library(tmp_path):
    import subprocess
    M.lib()
    libdir = os.path.join(ROOT, "osqp-solver_amd")
    src, exe = tmp_path / "p_update_abi.c", tmp_path / "p_update_abi"
    src.write_text(C_PROGRAM)
    cmd = ["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", libdir, "-lmi_osqp",
           "-Wl,-rpath," + libdir, "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.split() == [str(ERR_NULL)] * 5 + ["7"], res.stdout
