"""CPU: the adjoint derivative (README "Adjoint derivative") is exported with the signatures of mi_osqp.h, bound in Python,
present in the facades, and refuses a null handle before any device access."""
import os
import re

import osqp_solver_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NULL = 6
ERR_INVALID_DATA = 1

DECLARED = {
    "mi_osqp_adjoint":
        "int mi_osqp_adjoint(mi_osqp_solver *h, const double *dx, const double *dy, double *dq, double *dP, double *dA, "
        "double *dl, double *du, int32_t *status);",
    "mi_osqp_batch_adjoint":
        "int mi_osqp_batch_adjoint(mi_osqp_batch *h, const double *dx, const double *dy, double *dq, double *dP, double *dA, "
        "double *dl, double *du, int32_t *status);",
    "mi_osqp_batch_adjoint_device":
        "int mi_osqp_batch_adjoint_device(mi_osqp_batch *h, const double *d_dx, const double *d_dy, double *d_dq, double *d_dP, "
        "double *d_dA, double *d_dl, double *d_du, int32_t *d_status, void *stream);",
}


def _header_without_comments():
    text = open(os.path.join(ROOT, "include", "mi_osqp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"\s+", " ", text).replace(" )", ")")


def test_entry_points_are_exported_bound_and_declared():
    import ctypes as C
    L = M.lib()
    header = _header_without_comments()
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    host = [vp] + [dp] * 7 + [C.POINTER(C.c_int32)]
    for name, decl in DECLARED.items():
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes == ([vp] * 10 if name.endswith("_device") else host), name
        assert decl in header, decl


def test_header_names_the_osqp_functions_it_replaces():
    text = open(os.path.join(ROOT, "include", "mi_osqp.h")).read()
    for name in ("osqp_adjoint_derivative_compute", "osqp_adjoint_derivative_get_mat", "osqp_adjoint_derivative_get_vec",
                 "mi_osqp_batch_get_polish_active afterwards returns the active set the adjoint used"):
        assert name in text, name


def test_null_handle_gives_err_null_without_a_gpu():
    import ctypes as C
    L = M.lib()
    v = (C.c_double * 4)()
    st = (C.c_int32 * 1)()
    assert L.mi_osqp_adjoint(None, v, v, v, v, v, v, v, st) == ERR_NULL
    assert L.mi_osqp_adjoint(None, None, None, None, None, None, None, None, None) == ERR_NULL
    assert L.mi_osqp_batch_adjoint(None, v, None, v, None, None, None, None, st) == ERR_NULL
    assert L.mi_osqp_batch_adjoint_device(None, None, None, None, None, None, None, None, None, None) == ERR_NULL


def test_wrong_arguments_are_refused_before_the_handle_is_looked_at():
    """dx missing, or an output that aliases an input: refused with the handle untouched (the block of zeros standing in for
    it here is never read), so nothing can have been enqueued."""
    import ctypes as C
    L = M.lib()
    fake = C.cast((C.c_char * 64)(), C.c_void_p)
    v, w = (C.c_double * 4)(), (C.c_double * 4)()
    dev = lambda a: C.cast(a, C.c_void_p)
    assert L.mi_osqp_batch_adjoint(fake, None, v, v, None, None, None, None, None) == ERR_NULL
    assert "dx" in L.mi_osqp_last_error().decode()
    assert L.mi_osqp_batch_adjoint_device(fake, None, dev(v), dev(w), None, None, None, None, None, None) == ERR_NULL
    for out in range(5):
        args = [None] * 5
        args[out] = dev(v)
        assert L.mi_osqp_batch_adjoint_device(fake, dev(v), dev(w), *args, None, None) == ERR_INVALID_DATA, out
        assert L.mi_osqp_batch_adjoint_device(fake, dev(w), dev(v), *args, None, None) == ERR_INVALID_DATA, out
    assert "aliases" in L.mi_osqp_last_error().decode()


def test_python_methods_layer_and_facade_exist():
    for meth in ("adjoint", "adjoint_device"):
        assert callable(getattr(M.BatchSolver, meth, None)), meth
    assert callable(getattr(M.QPSolver, "adjoint", None))
    layer = open(os.path.join(ROOT, "osqp-solver_amd", "qp_layer.py")).read()
    for text in ("class QPFunction(torch.autograd.Function)", "update_q_device", "update_A_bounds_device", "solve_device",
                 "adjoint_device", "needs_input_grad"):
        assert text in layer, text
    assert len(layer.splitlines()) <= 80                      # a thin layer: no solver logic
    facade = open(os.path.join(ROOT, "include", "mi_osqp", "qp_solver.hpp")).read()
    for text in ("struct QPAdjoint", "QPAdjoint adjointDerivative(const QPVector &dx, const QPVector &dy = {})"):
        assert text in facade, text


C_PROGRAM = r"""
/* include/mi_osqp.h against the compiled library: the three entry points are assigned to pointers of the specified type (a
   declaration of another type does not compile under -Werror), linked, and called with a null handle, which needs no device. */
#include <stdint.h>
#include <stdio.h>
#include "mi_osqp.h"
int main(void) {
  int (*s)(mi_osqp_solver *, const double *, const double *, double *, double *, double *, double *, double *, int32_t *) = mi_osqp_adjoint;
  int (*b)(mi_osqp_batch *, const double *, const double *, double *, double *, double *, double *, double *, int32_t *) = mi_osqp_batch_adjoint;
  int (*d)(mi_osqp_batch *, const double *, const double *, double *, double *, double *, double *, double *, int32_t *, void *) =
      mi_osqp_batch_adjoint_device;
  double v[4] = {0, 0, 0, 0};
  int32_t st = 7;
  printf("%d %d %d %d\n", s(0, v, v, v, v, v, v, v, &st), b(0, v, 0, v, 0, 0, 0, 0, &st), d(0, v, 0, v, 0, 0, 0, 0, &st, 0), (int)st);
  return 0;
}
"""

CPP_PROGRAM = r"""
// the C++ facade compiles with its new method (never run: a QPSolver needs a device)
#include "mi_osqp/qp_solver.hpp"
miosqp_ref::QPAdjoint probe(miosqp_ref::QPSolver &s, const miosqp_ref::QPVector &g) { return s.adjointDerivative(g); }
int main() { return 0; }
"""


def test_header_declarations_compile_link_and_run_against_the_library(tmp_path):
    import subprocess
    M.lib()
    libdir = os.path.join(ROOT, "osqp-solver_amd")
    src, exe = tmp_path / "adjoint_abi.c", tmp_path / "adjoint_abi"
    src.write_text(C_PROGRAM)
    cmd = ["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", libdir, "-lmi_osqp",
           "-Wl,-rpath," + libdir, "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.split() == [str(ERR_NULL)] * 3 + ["7"], res.stdout       # (a refused call writes no status)
    src, exe = tmp_path / "adjoint_facade.cpp", tmp_path / "adjoint_facade"
    src.write_text(CPP_PROGRAM)
    cmd = ["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", libdir, "-lmi_osqp",
           "-Wl,-rpath," + libdir, "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
