"""oracle/ref_build.py -- compiles the reference's own code into oracle/_ref/ (TEST INFRASTRUCTURE ONLY).

The reference's headers are never copied into this repository: where the reference checkout is available to
build() ([REF] = $MI_OSQP_REFERENCE_DIR, default /root/reference), its src/osqp-wrapper.h is
compiled UNCHANGED against include/osqp++.h into oracle/_ref/osqp_shim_ref (tests/cpp/osqp_shim_test.cpp with
-DMI_REF_WRAPPER).  tests/test_osqp_shim.py runs that binary; nothing else reads the reference."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
OUT = os.path.join(_HERE, "_ref")
SHIM_REF = os.path.join(OUT, "osqp_shim_ref")


def reference_dir():
    return os.environ.get("MI_OSQP_REFERENCE_DIR", "/root/reference")


def build_shim_ref(verbose=False):
    """Returns the binary's path, or None when the reference is not available (nothing is built then)."""
    wrapper = os.path.join(reference_dir(), "src", "osqp-wrapper.h")
    if not os.access(wrapper, os.R_OK):
        return None
    src = os.path.join(_ROOT, "tests", "cpp", "osqp_shim_test.cpp")
    deps = [wrapper, src, os.path.join(_ROOT, "include", "osqp++.h"), os.path.join(_ROOT, "include", "mi_osqp.h")]
    if os.path.exists(SHIM_REF) and all(os.path.getmtime(d) <= os.path.getmtime(SHIM_REF) for d in deps):
        return SHIM_REF
    os.makedirs(OUT, exist_ok=True)
    libdir = os.path.join(_ROOT, "osqp-solver_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-DNDEBUG", f'-DMI_REF_WRAPPER="{wrapper}"',
           "-I", os.path.join(_ROOT, "tests", "cpp", "eigen_standin"), "-I", os.path.join(_ROOT, "include"), src,
           "-L", libdir, "-lmi_osqp", "-Wl,-rpath,$ORIGIN/../../osqp-solver_amd", "-o", SHIM_REF]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return SHIM_REF
