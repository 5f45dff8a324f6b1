"""osqp-solver_amd -- MI355X-native OSQP ADMM core behind the reference's QPSolver API.

Python here is only the test/bench harness language (the reference is C++; its
drop-in is include/mi_osqp.h + include/mi_osqp/qp_solver.hpp).  This module is
a ctypes binding of the C-ABI; it never computes anything itself and never
touches oracle/.  If libmi_osqp.so cannot be built/loaded, import fails loudly.
"""
import ctypes as C
import os

import numpy as np

# torch bundles its own HIP runtime (same SONAME as /opt/rocm's).  Whichever is
# loaded first wins for the whole process, and torch cannot initialise on top of
# the system one -- so when torch is installed it must be imported before
# libmi_osqp.so is dlopen'ed.  torch is plumbing here (device tensors, streams,
# torch.distributed); the library itself does not need it.
try:
    import torch  # noqa: F401
except ImportError:  # pragma: no cover
    torch = None

from . import build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

EXIT_NAMES = ["kOptimal", "kPrimalInfeasible", "kDualInfeasible", "kOptimalInaccurate",
              "kPrimalInfeasibleInaccurate", "kDualInfeasibleInaccurate", "kMaxIterations",
              "kInterrupted", "kTimeLimitReached", "kNonConvex", "kUnknown"]
K_OPTIMAL = 0


class Settings(C.Structure):
    _fields_ = [("rho", C.c_double), ("sigma", C.c_double), ("scaling", C.c_int64),
                ("adaptive_rho", C.c_int64), ("adaptive_rho_interval", C.c_int64),
                ("adaptive_rho_tolerance", C.c_double), ("max_iter", C.c_int64),
                ("eps_abs", C.c_double), ("eps_rel", C.c_double), ("eps_prim_inf", C.c_double),
                ("eps_dual_inf", C.c_double), ("alpha", C.c_double), ("scaled_termination", C.c_int64),
                ("check_termination", C.c_int64), ("warm_start", C.c_int64), ("verbose", C.c_int64),
                ("polish", C.c_int64), ("polish_refine_iter", C.c_int64), ("delta", C.c_double)]


class Info(C.Structure):
    _fields_ = [("iter", C.c_int64), ("status_val", C.c_int64), ("exit_code", C.c_int64),
                ("obj_val", C.c_double), ("pri_res", C.c_double), ("dua_res", C.c_double),
                ("rho_updates", C.c_int64), ("rho_estimate", C.c_double), ("rho", C.c_double),
                ("status_polish", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Stats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in
                ("n", "m", "N", "batch", "tile", "n_tiles", "nnz_P_triu", "nnz_A", "nnz_KKT", "nnz_L",
                 "n_supernodes", "n_blocks", "fwd_levels", "bwd_levels", "fwd_slots", "bwd_slots",
                 "chk_slots", "lds_bytes", "threads_per_block", "dense_tail_rows", "dense_tail_slots")] + \
               [(k, C.c_double) for k in ("setup_seconds_host", "setup_seconds_factor", "setup_seconds_upload")] + \
               [("nnz_L_before_tail", C.c_int64), ("solve_groups", C.c_int64), ("solve_group_threads", C.c_int64),
                ("resident_state", C.c_int64), ("lds_bytes_iterate", C.c_int64), ("pipelined_refactors", C.c_int64),
                ("resident_factor_steps", C.c_int64), ("lds_bytes_factor", C.c_int64),
                ("dense_tail_tasks", C.c_int64), ("dense_tail_waves_used", C.c_int64), ("dense_tail_wave_tasks_max", C.c_int64),
                ("refactor_lanes", C.c_int64),
                ("iterate_launches_deep_ring", C.c_int64), ("iterate_launches_long_head", C.c_int64),
                ("runahead_regions", C.c_int64), ("runahead_tiles", C.c_int64), ("runahead_left", C.c_int64),
                ("runahead_missed", C.c_int64),
                ("region_priority", C.c_int64), ("region_lane_checks", C.c_int64), ("region_chunks", C.c_int64),
                ("resident_index_words", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MiOsqpError(RuntimeError):
    def __init__(self, code, where):
        self.code = int(code)
        L = lib()
        msg = L.mi_osqp_error_name(int(code)).decode()
        extra = L.mi_osqp_last_error().decode()
        super().__init__(f"{where}: error {int(code)} ({msg}) {extra}")


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libmi_osqp.so")
        if os.environ.get("MI_OSQP_LIBRARY"):      # (tests: the diagnostic twin of the library, build.build_debug)
            path = os.environ["MI_OSQP_LIBRARY"]
        else:
            try:
                path = _build.build()
            except Exception as e:  # hipcc missing on this machine: use the shipped .so or fail
                if not os.path.exists(path):
                    raise ImportError(f"libmi_osqp.so missing and could not be built: {e}") from e
        L = C.CDLL(path)
        ip, dp, vp = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_void_p
        L.mi_osqp_default_settings.argtypes = [C.POINTER(Settings)]
        for f in ("mi_osqp_exit_code_name", "mi_osqp_error_name"):
            getattr(L, f).restype = C.c_char_p; getattr(L, f).argtypes = [C.c_int64]
        L.mi_osqp_version.restype = C.c_char_p
        L.mi_osqp_last_error.restype = C.c_char_p
        L.mi_osqp_batch_setup.argtypes = [C.POINTER(vp), C.c_int64, C.c_int64, C.c_int64, ip, ip, dp, dp, ip, ip, dp,
                                          dp, dp, C.POINTER(Settings), C.c_int64]
        L.mi_osqp_batch_update_A.argtypes = [vp, ip, ip, dp]
        L.mi_osqp_batch_update_A_bounds.argtypes = [vp, ip, ip, dp, dp, dp]
        L.mi_osqp_batch_update_bounds.argtypes = [vp, dp, dp]
        L.mi_osqp_batch_warm_start_x.argtypes = [vp, dp]
        L.mi_osqp_batch_update_q.argtypes = [vp, dp]
        L.mi_osqp_batch_update_q_device.argtypes = [vp, vp, vp]
        L.mi_osqp_batch_update_P.argtypes = [vp, ip, ip, dp]
        L.mi_osqp_batch_update_P_A.argtypes = [vp, ip, ip, dp, ip, ip, dp]
        L.mi_osqp_batch_warm_start_y.argtypes = [vp, dp]
        L.mi_osqp_batch_get_P_upper_pattern.argtypes = [vp, ip, ip, ip]
        L.mi_osqp_batch_update_P_device.argtypes = [vp, vp, vp]
        L.mi_osqp_batch_update_P_A_bounds_device.argtypes = [vp, vp, vp, vp, vp, vp]
        L.mi_osqp_batch_update_P_some.argtypes = [vp, C.c_int64, ip, dp]
        L.mi_osqp_batch_update_P_A_bounds_some.argtypes = [vp, C.c_int64, ip, dp, dp, dp, dp]
        L.mi_osqp_batch_update_q_some.argtypes = [vp, C.c_int64, ip, dp]
        L.mi_osqp_batch_warm_start_y_some.argtypes = [vp, C.c_int64, ip, dp]
        L.mi_osqp_settings_update_check.argtypes = [C.POINTER(Settings), C.POINTER(Settings)]
        L.mi_osqp_batch_get_settings.argtypes = [vp, C.POINTER(Settings)]
        L.mi_osqp_batch_update_settings.argtypes = [vp, C.POINTER(Settings)]
        L.mi_osqp_batch_update_rho_each.argtypes = [vp, dp]
        L.mi_osqp_batch_update_rho_some.argtypes = [vp, C.c_int64, ip, dp]
        L.mi_osqp_get_settings.argtypes = [vp, C.POINTER(Settings)]
        L.mi_osqp_update_settings.argtypes = [vp, C.POINTER(Settings)]
        L.mi_osqp_multi_batch_get_settings.argtypes = [vp, C.POINTER(Settings)]
        L.mi_osqp_multi_batch_update_settings.argtypes = [vp, C.POINTER(Settings)]
        L.mi_osqp_multi_batch_update_rho_each.argtypes = [vp, dp]
        L.mi_osqp_batch_solve.argtypes = [vp]
        L.mi_osqp_batch_get_primal.argtypes = [vp, dp]
        L.mi_osqp_batch_get_dual.argtypes = [vp, dp]
        L.mi_osqp_batch_get_info.argtypes = [vp, C.POINTER(Info)]
        for f in ("mi_osqp_get_prim_inf_cert", "mi_osqp_get_dual_inf_cert", "mi_osqp_batch_get_prim_inf_cert",
                  "mi_osqp_batch_get_dual_inf_cert", "mi_osqp_multi_batch_get_prim_inf_cert", "mi_osqp_multi_batch_get_dual_inf_cert"):
            getattr(L, f).argtypes = [vp, dp]
        L.mi_osqp_batch_get_prim_inf_cert_some.argtypes = [vp, C.c_int64, ip, dp]
        L.mi_osqp_batch_get_dual_inf_cert_some.argtypes = [vp, C.c_int64, ip, dp]
        L.mi_osqp_batch_get_stats.argtypes = [vp, C.POINTER(Stats)]
        L.mi_osqp_batch_get_ordering.argtypes = [vp, ip]
        L.mi_osqp_batch_free.argtypes = [vp]; L.mi_osqp_batch_free.restype = None
        L.mi_osqp_batch_update_bounds_device.argtypes = [vp, vp, vp, vp]
        L.mi_osqp_batch_update_A_bounds_device.argtypes = [vp, vp, vp, vp, vp]
        L.mi_osqp_batch_solve_device.argtypes = [vp, vp, vp, vp, vp]
        L.mi_osqp_batch_reset.argtypes = [vp]
        L.mi_osqp_batch_refactor_device.argtypes = [vp]
        L.mi_osqp_batch_last_solve_stats.argtypes = [vp, ip, ip, dp, dp, ip, dp]
        L.mi_osqp_batch_last_polish_stats.argtypes = [vp, ip, ip, dp]
        L.mi_osqp_batch_get_polish_active.argtypes = [vp, C.POINTER(C.c_int8)]
        L.mi_osqp_batch_adjoint.argtypes = [vp, dp, dp, dp, dp, dp, dp, dp, C.POINTER(C.c_int32)]
        L.mi_osqp_adjoint.argtypes = [vp, dp, dp, dp, dp, dp, dp, dp, C.POINTER(C.c_int32)]
        L.mi_osqp_batch_adjoint_device.argtypes = [vp] * 10
        L.mi_osqp_batch_get_scaling.argtypes = [vp, dp, dp, dp]
        L.mi_osqp_batch_spmv.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.mi_osqp_batch_kkt_solve.argtypes = [vp, vp, vp, vp]
        L.mi_osqp_batch_kernel_time.argtypes = [vp, dp, ip]
        L.mi_osqp_batch_refactor_time.argtypes = [vp, dp, dp, ip, ip]
        L.mi_osqp_batch_refactor_peak.argtypes = [vp, ip, dp, dp]
        L.mi_osqp_batch_reinit_some.argtypes = [vp, C.c_int64, ip, dp, dp, dp]
        L.mi_osqp_batch_update_A_bounds_some.argtypes = [vp, C.c_int64, ip, dp, dp, dp]
        L.mi_osqp_batch_warm_start_x_some.argtypes = [vp, C.c_int64, ip, dp]
        L.mi_osqp_batch_solve_begin_some.argtypes = [vp, C.c_int64, ip]
        L.mi_osqp_batch_polish_some.argtypes = [vp, C.c_int64, ip]
        L.mi_osqp_batch_advance.argtypes = [vp, C.c_int64]
        L.mi_osqp_batch_poll.argtypes = [vp, C.c_int64, ip, ip, C.c_int64]
        L.mi_osqp_batch_get_primal_some.argtypes = [vp, C.c_int64, ip, dp]
        L.mi_osqp_batch_get_dual_some.argtypes = [vp, C.c_int64, ip, dp]
        L.mi_osqp_batch_get_info_some.argtypes = [vp, C.c_int64, ip, C.POINTER(Info)]
        L.mi_osqp_batch_running.argtypes = [vp]; L.mi_osqp_batch_running.restype = C.c_int64
        L.mi_osqp_batch_ring_wraps.argtypes = [vp]; L.mi_osqp_batch_ring_wraps.restype = C.c_int64
        L.mi_osqp_release_device_cache.argtypes = []; L.mi_osqp_release_device_cache.restype = None
        L.mi_osqp_setup.argtypes = [C.POINTER(vp), C.c_int64, C.c_int64, ip, ip, dp, dp, ip, ip, dp, dp, dp, C.POINTER(Settings)]
        L.mi_osqp_update_A.argtypes = [vp, ip, ip, dp]
        L.mi_osqp_update_bounds.argtypes = [vp, dp, dp]
        L.mi_osqp_warm_start_x.argtypes = [vp, dp]
        L.mi_osqp_update_q.argtypes = [vp, dp]
        L.mi_osqp_update_P.argtypes = [vp, ip, ip, dp]
        L.mi_osqp_update_P_A.argtypes = [vp, ip, ip, dp, ip, ip, dp]
        L.mi_osqp_warm_start_y.argtypes = [vp, dp]
        L.mi_osqp_solve.argtypes = [vp, C.POINTER(Info)]
        L.mi_osqp_get_primal.argtypes = [vp, dp]
        L.mi_osqp_get_dual.argtypes = [vp, dp]
        L.mi_osqp_get_stats.argtypes = [vp, C.POINTER(Stats)]
        L.mi_osqp_free.argtypes = [vp]; L.mi_osqp_free.restype = None
        L.mi_osqp_multi_batch_setup.argtypes = [C.POINTER(vp), C.c_int64, ip, C.c_int64, C.c_int64, C.c_int64, ip, ip, dp, dp,
                                                ip, ip, dp, dp, dp, C.POINTER(Settings)]
        L.mi_osqp_multi_batch_update_A.argtypes = [vp, ip, ip, dp]
        L.mi_osqp_multi_batch_update_bounds.argtypes = [vp, dp, dp]
        L.mi_osqp_multi_batch_update_A_bounds.argtypes = [vp, ip, ip, dp, dp, dp]
        L.mi_osqp_multi_batch_warm_start_x.argtypes = [vp, dp]
        L.mi_osqp_multi_batch_update_q.argtypes = [vp, dp]
        L.mi_osqp_multi_batch_update_P.argtypes = [vp, ip, ip, dp]
        L.mi_osqp_multi_batch_update_P_A.argtypes = [vp, ip, ip, dp, ip, ip, dp]
        L.mi_osqp_multi_batch_warm_start_y.argtypes = [vp, dp]
        L.mi_osqp_multi_batch_solve.argtypes = [vp]
        L.mi_osqp_multi_batch_solve_async.argtypes = [vp]
        L.mi_osqp_multi_batch_wait.argtypes = [vp]
        L.mi_osqp_multi_batch_get_primal.argtypes = [vp, dp]
        L.mi_osqp_multi_batch_get_dual.argtypes = [vp, dp]
        L.mi_osqp_multi_batch_get_info.argtypes = [vp, C.POINTER(Info)]
        L.mi_osqp_multi_batch_shards.argtypes = [vp]; L.mi_osqp_multi_batch_shards.restype = C.c_int64
        L.mi_osqp_multi_batch_shard.argtypes = [vp, C.c_int64, ip, ip, ip, C.POINTER(vp)]
        L.mi_osqp_multi_batch_free.argtypes = [vp]; L.mi_osqp_multi_batch_free.restype = None
        L.mi_osqp_debug_host_kkt_solve.argtypes = [C.c_int64, C.c_int64, ip, ip, dp, ip, ip, dp, dp, dp,
                                                   C.POINTER(Settings), C.c_int64, dp, dp, dp, C.POINTER(Stats)]
        L.mi_osqp_debug_refactor_chunks.argtypes = [C.c_int64, ip, C.c_int64, ip, C.c_int64, C.c_int64, C.c_int64, ip, ip, ip, ip]
        L.mi_osqp_debug_refactor_lanes.argtypes = [C.c_int64, ip, C.c_int64, ip] + [C.c_int64] * 7 + [ip] * 8
        L.mi_osqp_debug_runahead_group.argtypes = [C.c_int64, ip, dp, dp, C.c_int64, C.c_int64, ip, ip]
        L.mi_osqp_debug_region_chunks.argtypes = [C.c_int64] * 3 + [ip] * 2
        L.mi_osqp_debug_iterate_form.argtypes = [C.c_int64] * 4 + [ip]
        L.mi_osqp_debug_index_words_fit.argtypes = [C.c_int64] * 6 + [ip] * 3
        L.mi_osqp_prefetch_analysis.argtypes = [C.c_int64, C.c_int64, C.c_int64, ip, ip, ip, ip, C.c_int64]
        L.mi_osqp_debug_host_block_factor.argtypes = [C.c_int64, C.c_int64, ip, ip, dp, ip, ip, dp, dp, dp,
                                                      C.POINTER(Settings), dp, dp, ip]
        _LIB = L
    return _LIB


def host_cores():
    """CPU cores this process may actually use: min(affinity, cgroup quota)."""
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max",):
        try:
            quota, period = open(path).read().split()[:2]
            if quota != "max":
                n = min(n, max(1, int(round(int(quota) / int(period)))))
        except Exception:
            pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0:
            n = min(n, max(1, int(round(q / p))))
    except Exception:
        pass
    return n


def default_settings(**kw):
    s = Settings()
    lib().mi_osqp_default_settings(C.byref(s))
    for k, v in kw.items():
        if not hasattr(s, k):
            raise KeyError(k)
        setattr(s, k, v)
    return s


class HandleSettings(Settings):
    """The `settings` attribute of a solver: the fields hold the settings in force (they follow update_settings), and calling
    it - solver.settings() - reads them from the handle and returns them as a fresh Settings."""

    def bind(self, getter):
        self._getter = getter
        return self

    def __call__(self):
        out = Settings()
        self._getter(out)
        C.memmove(C.byref(self), C.byref(out), C.sizeof(Settings))
        return out


def settings_update_check(in_force, wanted):
    """Host only: the mi_osqp_error update_settings(wanted) would return on a handle whose settings are `in_force`."""
    return int(lib().mi_osqp_settings_update_check(C.byref(in_force), C.byref(wanted)))


def _handle_settings(kw, get_name, owner):
    """default_settings(**kw) as a HandleSettings whose call reads the handle of `owner` (held weakly) through `get_name`."""
    import weakref
    hs = HandleSettings()
    C.memmove(C.byref(hs), C.byref(default_settings(**kw)), C.sizeof(Settings))
    ref = weakref.ref(owner)

    def getter(out):
        _chk(getattr(lib(), get_name)(ref()._h, C.byref(out)), get_name)
    return hs.bind(getter)


def _update_settings(self, fn_name, fields):
    """get, set the given fields, update: the whole struct goes to the C-ABI, which refuses it as a whole."""
    s = self.settings()
    for k, v in fields.items():
        if not hasattr(s, k):
            raise KeyError(k)
        setattr(s, k, v)
    _chk(getattr(lib(), fn_name)(self._h, C.byref(s)), fn_name)
    return self.settings()


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _chk(rc, where):
    if rc != 0:
        raise MiOsqpError(rc, where)


def _csc(M):
    import scipy.sparse as sp
    M = sp.csc_matrix(M)
    M.sort_indices()
    return M


class BatchSolver:
    """B QPs with one shared sparsity pattern (P_pattern / A_pattern are scipy
    sparse matrices carrying the pattern; Px[B,nnzP], Ax[B,nnzA] the per-QP values
    in CSC order of those patterns)."""

    def __init__(self, P_pattern, Px, q, A_pattern, Ax, l, u, device=-1, **settings):
        L = lib()
        P, A = _csc(P_pattern), _csc(A_pattern)
        self.n, self.m = A.shape[1], A.shape[0]
        Px, Ax, l, u = _f64(Px), _f64(Ax), _f64(l), _f64(u)
        if Ax.ndim == 1:
            Px, Ax, l, u = Px[None], Ax[None], l[None], u[None]
            q = None if q is None else _f64(q)[None]
        self.B = Ax.shape[0]
        q = None if q is None else _f64(q)
        self._Pp, self._Pi = _i64(P.indptr), _i64(P.indices)
        self._Ap, self._Ai = _i64(A.indptr), _i64(A.indices)
        self.settings = _handle_settings(settings, "mi_osqp_batch_get_settings", self)
        self._h = C.c_void_p()
        rc = L.mi_osqp_batch_setup(C.byref(self._h), self.B, self.n, self.m, _ip(self._Pp), _ip(self._Pi), _dp(Px),
                                   _dp(q), _ip(self._Ap), _ip(self._Ai), _dp(Ax), _dp(l), _dp(u),
                                   C.byref(self.settings), device)
        _chk(rc, "mi_osqp_batch_setup")

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                lib().mi_osqp_batch_free(self._h)
                self._h = C.c_void_p()
        except Exception:       # interpreter shutdown: module globals may already be gone
            pass

    close = __del__

    def solve(self):
        _chk(lib().mi_osqp_batch_solve(self._h), "mi_osqp_batch_solve")
        return self.info()

    def primal(self):
        x = np.empty((self.B, self.n))
        _chk(lib().mi_osqp_batch_get_primal(self._h, _dp(x)), "get_primal")
        return x

    def dual(self):
        y = np.empty((self.B, self.m))
        _chk(lib().mi_osqp_batch_get_dual(self._h, _dp(y)), "get_dual")
        return y

    def info(self):
        arr = (Info * self.B)()
        _chk(lib().mi_osqp_batch_get_info(self._h, arr), "get_info")
        return list(arr)

    # ---- infeasibility certificates (mi_osqp.h mi_osqp_get_prim_inf_cert): unit infinity norm, NaN rows where there is none
    def prim_inf_cert(self):
        """[B, m]: delta_y of every QP whose last solve ended primal infeasible (status -3 / 3), NaN rows elsewhere."""
        v = np.empty((self.B, self.m))
        _chk(lib().mi_osqp_batch_get_prim_inf_cert(self._h, _dp(v)), "get_prim_inf_cert")
        return v

    def dual_inf_cert(self):
        """[B, n]: delta_x of every QP whose last solve ended dual infeasible (status -4 / 4), NaN rows elsewhere."""
        v = np.empty((self.B, self.n))
        _chk(lib().mi_osqp_batch_get_dual_inf_cert(self._h, _dp(v)), "get_dual_inf_cert")
        return v

    def stats(self):
        s = Stats()
        _chk(lib().mi_osqp_batch_get_stats(self._h, C.byref(s)), "get_stats")
        return s.as_dict()

    def ordering(self):
        """Elimination order of the KKT matrix chosen by the analysis (natural index eliminated k-th)."""
        perm = np.empty(self.n + self.m, dtype=np.int64)
        _chk(lib().mi_osqp_batch_get_ordering(self._h, _ip(perm)), "get_ordering")
        return perm

    def update_A(self, Ax, A_pattern=None):
        Ax = _f64(Ax).reshape(self.B, -1)
        Ap, Ai = self._Ap, self._Ai
        if A_pattern is not None:
            A = _csc(A_pattern)
            Ap, Ai = _i64(A.indptr), _i64(A.indices)
            if len(Ai) != len(self._Ai):
                raise MiOsqpError(3, "update_A")
        _chk(lib().mi_osqp_batch_update_A(self._h, _ip(Ap), _ip(Ai), _dp(Ax)), "update_A")

    def update_A_bounds(self, Ax, l, u):
        """QPSolver::update as one call: new A values and new bounds, one refactorisation."""
        Ax = _f64(Ax).reshape(self.B, -1)
        l, u = _f64(l).reshape(self.B, -1), _f64(u).reshape(self.B, -1)
        _chk(lib().mi_osqp_batch_update_A_bounds(self._h, _ip(self._Ap), _ip(self._Ai), _dp(Ax), _dp(l), _dp(u)), "update_A_bounds")

    def update_bounds(self, l, u):
        l, u = _f64(l).reshape(self.B, -1), _f64(u).reshape(self.B, -1)
        _chk(lib().mi_osqp_batch_update_bounds(self._h, _dp(l), _dp(u)), "update_bounds")

    def warm_start_x(self, x):
        x = _f64(x).reshape(self.B, -1)
        _chk(lib().mi_osqp_batch_warm_start_x(self._h, _dp(x)), "warm_start_x")

    # ---- objective updates (OSQP osqp_update_lin_cost / osqp_update_P / osqp_update_P_A / osqp_warm_start_y)
    def update_q(self, q):
        q = _f64(q).reshape(self.B, -1)
        _chk(lib().mi_osqp_batch_update_q(self._h, _dp(q)), "update_q")

    def update_q_device(self, q, stream=None):
        """update_q from a torch CUDA tensor ([B, n], float64, contiguous)."""
        _chk(lib().mi_osqp_batch_update_q_device(self._h, C.c_void_p(q.data_ptr()), None if stream is None else C.c_void_p(stream)),
             "update_q_device")

    def _P_arrays(self, Px, P_pattern):
        Pp, Pi = self._Pp, self._Pi
        if P_pattern is not None:
            P = _csc(P_pattern)
            Pp, Pi = _i64(P.indptr), _i64(P.indices)
        return Pp, Pi, _f64(Px).reshape(self.B, -1)

    def update_P(self, Px, P_pattern=None):
        """New P values [B, nnz] in the CSC order of P_pattern (default: setup's pattern); both triangles or the upper one."""
        Pp, Pi, Px = self._P_arrays(Px, P_pattern)
        _chk(lib().mi_osqp_batch_update_P(self._h, _ip(Pp), _ip(Pi), _dp(Px)), "update_P")

    def update_P_A(self, Px, Ax, P_pattern=None):
        Pp, Pi, Px = self._P_arrays(Px, P_pattern)
        Ax = _f64(Ax).reshape(self.B, -1)
        _chk(lib().mi_osqp_batch_update_P_A(self._h, _ip(Pp), _ip(Pi), _dp(Px), _ip(self._Ap), _ip(self._Ai), _dp(Ax)),
             "update_P_A")

    def P_upper_pattern(self):
        """(colptr [n + 1], rowidx [nnzPu]) of triu(P) as the analysis keeps it: the order of adjoint()'s dP and of the Px of
        update_P_device / update_P_A_bounds_device / update_P_some / update_P_A_bounds_some, whichever form P had at setup."""
        nnz = C.c_int64()
        _chk(lib().mi_osqp_batch_get_P_upper_pattern(self._h, None, None, C.byref(nnz)), "get_P_upper_pattern")
        Pp, Pi = np.empty(self.n + 1, dtype=np.int64), np.empty(nnz.value, dtype=np.int64)
        _chk(lib().mi_osqp_batch_get_P_upper_pattern(self._h, _ip(Pp), _ip(Pi), C.byref(nnz)), "get_P_upper_pattern")
        return Pp, Pi

    def _check_Pu(self, Px, rows):
        """Px must be [rows, nnzPu]: a P with both triangles, as update_P takes it, is not the form of these calls"""
        if getattr(self, "_nnzPu", None) is None:
            nnz = C.c_int64()
            _chk(lib().mi_osqp_batch_get_P_upper_pattern(self._h, None, None, C.byref(nnz)), "get_P_upper_pattern")
            self._nnzPu = nnz.value
        if tuple(Px.shape) != (rows, self._nnzPu):
            raise ValueError(f"Px must have shape ({rows}, {self._nnzPu}): triu(P) in the order of P_upper_pattern(); got {tuple(Px.shape)}")

    def update_P_device(self, Px, stream=None):
        """update_P from a torch CUDA tensor ([B, nnzPu], float64, contiguous): triu(P) in the order of P_upper_pattern()."""
        self._check_Pu(Px, self.B)
        _chk(lib().mi_osqp_batch_update_P_device(self._h, C.c_void_p(Px.data_ptr()), None if stream is None else C.c_void_p(stream)),
             "update_P_device")

    def update_P_A_bounds_device(self, Px, Ax, l, u, stream=None):
        """New triu(P) values, A values and bounds from torch CUDA tensors with one equilibration and one refactorisation.
        Px None: update_A_bounds_device; Ax, l and u all None: update_P_device."""
        if Px is not None:
            self._check_Pu(Px, self.B)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        _chk(lib().mi_osqp_batch_update_P_A_bounds_device(self._h, p(Px), p(Ax), p(l), p(u), None if stream is None else C.c_void_p(stream)),
             "update_P_A_bounds_device")

    def warm_start_y(self, y):
        y = _f64(y).reshape(self.B, -1)
        _chk(lib().mi_osqp_batch_warm_start_y(self._h, _dp(y)), "warm_start_y")

    # ---- settings updates (OSQP osqp_update_*; mi_osqp.h "settings updates").  self.settings() returns the settings in force.
    def update_settings(self, **fields):
        """Change the given settings (rho, max_iter, eps_*, alpha, scaled_termination, check_termination, warm_start, polish,
        polish_refine_iter, delta, verbose); a new rho refactors every QP.  Returns the settings in force."""
        return _update_settings(self, "mi_osqp_batch_update_settings", fields)

    def update_rho_each(self, rho):
        """One rho per QP ([B]); every QP is refactored.  settings.rho is not touched."""
        rho = _f64(rho).reshape(self.B)
        _chk(lib().mi_osqp_batch_update_rho_each(self._h, _dp(rho)), "update_rho_each")

    def update_rho_some(self, ids, rho):
        """Continuous mode: a new rho for the listed idle QPs, enqueued without waiting."""
        ids = _i64(ids); rho = _f64(rho).reshape(len(ids))
        _chk(lib().mi_osqp_batch_update_rho_some(self._h, len(ids), _ip(ids), _dp(rho)), "update_rho_some")

    def reset(self):
        _chk(lib().mi_osqp_batch_reset(self._h), "reset")

    def refactor_device(self):
        _chk(lib().mi_osqp_batch_refactor_device(self._h), "refactor_device")

    def last_solve_stats(self):
        it, ln, rc = C.c_int64(), C.c_int64(), C.c_int64()
        ds, rs, cs = C.c_double(), C.c_double(), C.c_double()
        _chk(lib().mi_osqp_batch_last_solve_stats(self._h, C.byref(it), C.byref(ln), C.byref(ds), C.byref(rs), C.byref(rc),
                                                  C.byref(cs)), "stats")
        return dict(total_iters=it.value, launches=ln.value, device_s=ds.value, refactor_s=rs.value, refactors=rc.value,
                    compact_s=cs.value)

    def last_polish_stats(self):
        """Polishing of the last solve: QPs polished, QPs whose polished solution was accepted, device seconds."""
        pol, acc, sec = C.c_int64(), C.c_int64(), C.c_double()
        _chk(lib().mi_osqp_batch_last_polish_stats(self._h, C.byref(pol), C.byref(acc), C.byref(sec)), "last_polish_stats")
        return dict(polished=pol.value, accepted=acc.value, seconds=sec.value)

    def polish_active(self):
        """Active set of the last polish, int8 [B, m]: -1 lower-active, +1 upper-active, 0 inactive / not polished."""
        act = np.zeros((self.B, self.m), dtype=np.int8)
        _chk(lib().mi_osqp_batch_get_polish_active(self._h, act.ctypes.data_as(C.POINTER(C.c_int8))), "get_polish_active")
        return act

    # ---- adjoint derivative (OSQP 1.0 osqp_adjoint_derivative_compute / _get_mat / _get_vec; mi_osqp.h "adjoint derivative")
    def adjoint(self, dx, dy=None):
        """Gradient of a loss with respect to the problem data from its gradient dx [B, n] (and dy [B, m], None = 0) with
        respect to the solutions of the last solve: dict(dq [B, n], dP [B, nnz triu(P)] (upper triangle, CSC order), dA
        [B, nnzA], dl, du [B, m], status int32 [B]: 1 computed, 0 not kOptimal, -1 factor failed; NaN rows where not 1)."""
        dx = _f64(dx).reshape(self.B, self.n)
        dy = None if dy is None else _f64(dy).reshape(self.B, self.m)
        st = self.stats()
        out = dict(dq=np.empty((self.B, self.n)), dP=np.empty((self.B, st["nnz_P_triu"])), dA=np.empty((self.B, st["nnz_A"])),
                   dl=np.empty((self.B, self.m)), du=np.empty((self.B, self.m)), status=np.zeros(self.B, dtype=np.int32))
        _chk(lib().mi_osqp_batch_adjoint(self._h, _dp(dx), _dp(dy), _dp(out["dq"]), _dp(out["dP"]), _dp(out["dA"]), _dp(out["dl"]),
                                         _dp(out["du"]), out["status"].ctypes.data_as(C.POINTER(C.c_int32))), "adjoint")
        return out

    def adjoint_device(self, dx, dy, dq=None, dP=None, dA=None, dl=None, du=None, status=None, stream=None):
        """adjoint() on torch CUDA tensors (float64, contiguous; status int32 [B]); dy and every output may be None."""
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        _chk(lib().mi_osqp_batch_adjoint_device(self._h, p(dx), p(dy), p(dq), p(dP), p(dA), p(dl), p(du), p(status),
                                                None if stream is None else C.c_void_p(stream)), "adjoint_device")

    def scaling(self):
        """Ruiz scaling in force, read from the device: (D [B, n], E [B, m], c [B]); all ones with scaling = 0."""
        D, E, c = np.empty((self.B, self.n)), np.empty((self.B, self.m)), np.empty(self.B)
        _chk(lib().mi_osqp_batch_get_scaling(self._h, _dp(D), _dp(E), _dp(c)), "get_scaling")
        return D, E, c

    def kernel_time(self):
        ms, cnt = C.c_double(), C.c_int64()
        _chk(lib().mi_osqp_batch_kernel_time(self._h, C.byref(ms), C.byref(cnt)), "kernel_time")
        return ms.value, cnt.value

    def refactor_time(self):
        """(factor_kernel ms, dense_inverse_kernel ms, launches, QPs refactored) since the last call."""
        f, d, ln, nq = C.c_double(), C.c_double(), C.c_int64(), C.c_int64()
        _chk(lib().mi_osqp_batch_refactor_time(self._h, C.byref(f), C.byref(d), C.byref(ln), C.byref(nq)), "refactor_time")
        return f.value, d.value, ln.value, nq.value

    def refactor_peak(self):
        """(QPs, factor_kernel ms, dense-tail kernels ms) of the largest refactorisation since the last refactor_time()."""
        nq, f, d = C.c_int64(), C.c_double(), C.c_double()
        _chk(lib().mi_osqp_batch_refactor_peak(self._h, C.byref(nq), C.byref(f), C.byref(d)), "refactor_peak")
        return nq.value, f.value, d.value

    # ---- continuous batching: per-QP entry points + non-blocking advance / poll (mi_osqp.h "continuous batching")
    def reinit_some(self, ids, Ax, l, u):
        ids = _i64(ids); k = len(ids)
        Ax, l, u = _f64(Ax).reshape(k, -1), _f64(l).reshape(k, -1), _f64(u).reshape(k, -1)
        _chk(lib().mi_osqp_batch_reinit_some(self._h, k, _ip(ids), _dp(Ax), _dp(l), _dp(u)), "reinit_some")

    def update_A_bounds_some(self, ids, Ax, l, u):
        ids = _i64(ids); k = len(ids)
        Ax, l, u = _f64(Ax).reshape(k, -1), _f64(l).reshape(k, -1), _f64(u).reshape(k, -1)
        _chk(lib().mi_osqp_batch_update_A_bounds_some(self._h, k, _ip(ids), _dp(Ax), _dp(l), _dp(u)), "update_A_bounds_some")

    def update_P_some(self, ids, Px):
        """New triu(P) values [len(ids), nnzPu] (order of P_upper_pattern()) for the listed idle QPs; nothing waits."""
        ids = _i64(ids); Px = _f64(Px).reshape(len(ids), -1)
        self._check_Pu(Px, len(ids))
        _chk(lib().mi_osqp_batch_update_P_some(self._h, len(ids), _ip(ids), _dp(Px)), "update_P_some")

    def update_P_A_bounds_some(self, ids, Px, Ax, l, u):
        ids = _i64(ids); k = len(ids)
        Px, Ax, l, u = _f64(Px).reshape(k, -1), _f64(Ax).reshape(k, -1), _f64(l).reshape(k, -1), _f64(u).reshape(k, -1)
        self._check_Pu(Px, k)
        _chk(lib().mi_osqp_batch_update_P_A_bounds_some(self._h, k, _ip(ids), _dp(Px), _dp(Ax), _dp(l), _dp(u)),
             "update_P_A_bounds_some")

    def warm_start_x_some(self, ids, x):
        ids = _i64(ids); x = _f64(x).reshape(len(ids), -1)
        _chk(lib().mi_osqp_batch_warm_start_x_some(self._h, len(ids), _ip(ids), _dp(x)), "warm_start_x_some")

    def update_q_some(self, ids, q):
        ids = _i64(ids); q = _f64(q).reshape(len(ids), -1)
        _chk(lib().mi_osqp_batch_update_q_some(self._h, len(ids), _ip(ids), _dp(q)), "update_q_some")

    def warm_start_y_some(self, ids, y):
        ids = _i64(ids); y = _f64(y).reshape(len(ids), -1)
        _chk(lib().mi_osqp_batch_warm_start_y_some(self._h, len(ids), _ip(ids), _dp(y)), "warm_start_y_some")

    def solve_begin_some(self, ids):
        ids = _i64(ids)
        _chk(lib().mi_osqp_batch_solve_begin_some(self._h, len(ids), _ip(ids)), "solve_begin_some")

    def polish_some(self, ids):
        """Polish the listed QPs (finished kOptimal, untouched since) without waiting; they count as running and are reported
        once more by the poll() of the next advance().  Refused as a whole (MiOsqpError, code 1) if any id does not qualify."""
        ids = _i64(ids)
        _chk(lib().mi_osqp_batch_polish_some(self._h, len(ids), _ip(ids)), "polish_some")

    def advance(self, n_segments=1):
        _chk(lib().mi_osqp_batch_advance(self._h, n_segments), "advance")

    def poll(self, wait=True):
        """QP ids that finished in the oldest advance not polled yet (None: wait=False and it has not run yet)."""
        out = np.empty(self.B, dtype=np.int64)
        nf = C.c_int64()
        _chk(lib().mi_osqp_batch_poll(self._h, 1 if wait else 0, C.byref(nf), _ip(out), self.B), "poll")
        return None if nf.value < 0 else out[:nf.value].copy()

    def running(self):
        return int(lib().mi_osqp_batch_running(self._h))

    def ring_wraps(self):
        """(tests) times the staging ring of the per-QP calls has wrapped since setup"""
        return int(lib().mi_osqp_batch_ring_wraps(self._h))

    def primal_some(self, ids):
        ids = _i64(ids); x = np.empty((len(ids), self.n))
        _chk(lib().mi_osqp_batch_get_primal_some(self._h, len(ids), _ip(ids), _dp(x)), "get_primal_some")
        return x

    def dual_some(self, ids):
        ids = _i64(ids); y = np.empty((len(ids), self.m))
        _chk(lib().mi_osqp_batch_get_dual_some(self._h, len(ids), _ip(ids), _dp(y)), "get_dual_some")
        return y

    def info_some(self, ids):
        ids = _i64(ids); arr = (Info * len(ids))()
        _chk(lib().mi_osqp_batch_get_info_some(self._h, len(ids), _ip(ids), arr), "get_info_some")
        return list(arr)

    def prim_inf_cert_some(self, ids):
        ids = _i64(ids); v = np.empty((len(ids), self.m))
        _chk(lib().mi_osqp_batch_get_prim_inf_cert_some(self._h, len(ids), _ip(ids), _dp(v)), "get_prim_inf_cert_some")
        return v

    def dual_inf_cert_some(self, ids):
        ids = _i64(ids); v = np.empty((len(ids), self.n))
        _chk(lib().mi_osqp_batch_get_dual_inf_cert_some(self._h, len(ids), _ip(ids), _dp(v)), "get_dual_inf_cert_some")
        return v

    # ---- device-resident variants (torch tensors on the solver's GPU)
    def solve_device(self, x_out=None, status=None, iters=None, stream=None):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        _chk(lib().mi_osqp_batch_solve_device(self._h, p(x_out), p(status), p(iters),
                                              None if stream is None else C.c_void_p(stream)), "solve_device")

    def update_A_bounds_device(self, Ax, l, u, stream=None):
        """QPSolver::update from torch CUDA tensors ([B, nnzA], [B, m], [B, m], float64, contiguous)."""
        _chk(lib().mi_osqp_batch_update_A_bounds_device(self._h, C.c_void_p(Ax.data_ptr()), C.c_void_p(l.data_ptr()), C.c_void_p(u.data_ptr()),
                                                        None if stream is None else C.c_void_p(stream)), "update_A_bounds_device")

    def update_bounds_device(self, l, u, stream=None):
        _chk(lib().mi_osqp_batch_update_bounds_device(self._h, C.c_void_p(l.data_ptr()), C.c_void_p(u.data_ptr()),
                                                      None if stream is None else C.c_void_p(stream)), "update_bounds_device")

    def spmv_device(self, x, y, Px, Aty, Ax, stream=None):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        _chk(lib().mi_osqp_batch_spmv(self._h, p(x), p(y), p(Px), p(Aty), p(Ax),
                                      None if stream is None else C.c_void_p(stream)), "spmv")

    def debug_trace_kkt_solve(self, rhs, sol):
        """Diagnostics (tile 2 only): returns (stamps[2 tiles], fwd phase table, bwd phase table, dims)."""
        import numpy as np
        L = lib()
        L.mi_osqp_debug_trace_kkt_solve.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                    C.POINTER(C.c_int64)]
        dims = (C.c_int64 * 4)()
        _chk(L.mi_osqp_debug_trace_kkt_solve(self._h, 0, None, None, None, 0, dims), "trace dims")
        fp, bp, nw, words = (int(v) for v in dims)
        tr = np.zeros(2 * words, dtype=np.uint32)
        _chk(L.mi_osqp_debug_trace_kkt_solve(self._h, 0, C.c_void_p(rhs.data_ptr()), C.c_void_p(sol.data_ptr()),
                                             tr.ctypes.data_as(C.c_void_p), tr.size, dims), "trace")
        tabs = []
        for which, rows in ((1, fp), (2, bp)):
            t = np.zeros(rows * (4 * nw + 1), dtype=np.uint32)
            _chk(L.mi_osqp_debug_trace_kkt_solve(self._h, which, None, None, t.ctypes.data_as(C.c_void_p), t.size, dims), "trace table")
            tabs.append(t.reshape(rows, 4 * nw + 1))
        return tr.reshape(2, words), tabs[0], tabs[1], (fp, bp, nw, words)

    def kkt_solve_device(self, rhs, sol, stream=None):
        _chk(lib().mi_osqp_batch_kkt_solve(self._h, C.c_void_p(rhs.data_ptr()), C.c_void_p(sol.data_ptr()),
                                           None if stream is None else C.c_void_p(stream)), "kkt_solve")


class MultiBatchSolver:
    """The batch sharded over several HIP devices inside ONE process (mi_osqp_multi_batch_*: block partition, one host
    thread per shard, no data-path collective).  `devices` may list a device more than once."""

    def __init__(self, P_pattern, Px, q, A_pattern, Ax, l, u, devices=(0,), **settings):
        L = lib()
        P, A = _csc(P_pattern), _csc(A_pattern)
        self.n, self.m = A.shape[1], A.shape[0]
        Px, Ax, l, u = _f64(Px), _f64(Ax), _f64(l), _f64(u)
        self.B = Ax.shape[0]
        q = None if q is None else _f64(q)
        self._Pp, self._Pi = _i64(P.indptr), _i64(P.indices)
        self._Ap, self._Ai = _i64(A.indptr), _i64(A.indices)
        self.settings = _handle_settings(settings, "mi_osqp_multi_batch_get_settings", self)
        devs = _i64(list(devices))
        self._h = C.c_void_p()
        _chk(L.mi_osqp_multi_batch_setup(C.byref(self._h), len(devs), _ip(devs), self.B, self.n, self.m, _ip(self._Pp),
                                         _ip(self._Pi), _dp(Px), _dp(q), _ip(self._Ap), _ip(self._Ai), _dp(Ax), _dp(l), _dp(u),
                                         C.byref(self.settings)), "mi_osqp_multi_batch_setup")

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                lib().mi_osqp_multi_batch_free(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    close = __del__

    def shards(self):
        out = []
        for k in range(lib().mi_osqp_multi_batch_shards(self._h)):
            d, b, e = C.c_int64(), C.c_int64(), C.c_int64()
            _chk(lib().mi_osqp_multi_batch_shard(self._h, k, C.byref(d), C.byref(b), C.byref(e), None), "shard")
            out.append((d.value, b.value, e.value))
        return out

    def solve(self):
        _chk(lib().mi_osqp_multi_batch_solve(self._h), "mi_osqp_multi_batch_solve")
        return self.info()

    def solve_async(self):
        _chk(lib().mi_osqp_multi_batch_solve_async(self._h), "mi_osqp_multi_batch_solve_async")

    def wait(self):
        _chk(lib().mi_osqp_multi_batch_wait(self._h), "mi_osqp_multi_batch_wait")
        return self.info()

    def info(self):
        arr = (Info * self.B)()
        _chk(lib().mi_osqp_multi_batch_get_info(self._h, arr), "multi get_info")
        return list(arr)

    def primal(self):
        x = np.empty((self.B, self.n))
        _chk(lib().mi_osqp_multi_batch_get_primal(self._h, _dp(x)), "multi get_primal")
        return x

    def dual(self):
        y = np.empty((self.B, self.m))
        _chk(lib().mi_osqp_multi_batch_get_dual(self._h, _dp(y)), "multi get_dual")
        return y

    def prim_inf_cert(self):
        v = np.empty((self.B, self.m))
        _chk(lib().mi_osqp_multi_batch_get_prim_inf_cert(self._h, _dp(v)), "multi get_prim_inf_cert")
        return v

    def dual_inf_cert(self):
        v = np.empty((self.B, self.n))
        _chk(lib().mi_osqp_multi_batch_get_dual_inf_cert(self._h, _dp(v)), "multi get_dual_inf_cert")
        return v

    def update_A(self, Ax):
        Ax = _f64(Ax).reshape(self.B, -1)
        _chk(lib().mi_osqp_multi_batch_update_A(self._h, _ip(self._Ap), _ip(self._Ai), _dp(Ax)), "multi update_A")

    def update_bounds(self, l, u):
        l, u = _f64(l).reshape(self.B, -1), _f64(u).reshape(self.B, -1)
        _chk(lib().mi_osqp_multi_batch_update_bounds(self._h, _dp(l), _dp(u)), "multi update_bounds")

    def update_A_bounds(self, Ax, l, u):
        Ax = _f64(Ax).reshape(self.B, -1)
        l, u = _f64(l).reshape(self.B, -1), _f64(u).reshape(self.B, -1)
        _chk(lib().mi_osqp_multi_batch_update_A_bounds(self._h, _ip(self._Ap), _ip(self._Ai), _dp(Ax), _dp(l), _dp(u)), "multi update_A_bounds")

    def warm_start_x(self, x):
        x = _f64(x).reshape(self.B, -1)
        _chk(lib().mi_osqp_multi_batch_warm_start_x(self._h, _dp(x)), "multi warm_start_x")

    def update_q(self, q):
        q = _f64(q).reshape(self.B, -1)
        _chk(lib().mi_osqp_multi_batch_update_q(self._h, _dp(q)), "multi update_q")

    def update_P(self, Px):
        Px = _f64(Px).reshape(self.B, -1)
        _chk(lib().mi_osqp_multi_batch_update_P(self._h, _ip(self._Pp), _ip(self._Pi), _dp(Px)), "multi update_P")

    def update_P_A(self, Px, Ax):
        Px, Ax = _f64(Px).reshape(self.B, -1), _f64(Ax).reshape(self.B, -1)
        _chk(lib().mi_osqp_multi_batch_update_P_A(self._h, _ip(self._Pp), _ip(self._Pi), _dp(Px), _ip(self._Ap), _ip(self._Ai),
                                                  _dp(Ax)), "multi update_P_A")

    def warm_start_y(self, y):
        y = _f64(y).reshape(self.B, -1)
        _chk(lib().mi_osqp_multi_batch_warm_start_y(self._h, _dp(y)), "multi warm_start_y")

    def update_settings(self, **fields):
        return _update_settings(self, "mi_osqp_multi_batch_update_settings", fields)

    def update_rho_each(self, rho):
        rho = _f64(rho).reshape(self.B)
        _chk(lib().mi_osqp_multi_batch_update_rho_each(self._h, _dp(rho)), "multi update_rho_each")


class QPSolver:
    """Python twin of the reference class QPSolver
    ([REF] /root/reference/src/osqp-wrapper.h:12-60): ctor(constraints, P),
    update(constraints), setWarmStart(x), solve() -> (exit_code, x).
    `constraints` = (l, A, u) like the reference's QPConstraints tuple."""

    def __init__(self, constraints, P, q=None, **settings):
        l, A, u = constraints
        self._b = BatchSolver(P, _csc(P).data, q, A, _csc(A).data, l, u, **settings)

    def update(self, constraints):
        l, A, u = constraints
        A = _csc(A)
        try:
            self._b.update_A(A.data, A_pattern=A)
            self._b.update_bounds(l, u)
        except MiOsqpError as e:           # the reference throws std::invalid_argument here
            raise ValueError(str(e)) from e

    def setWarmStart(self, x):
        self._b.warm_start_x(x)

    def update_settings(self, **fields):
        """osqp-cpp's Update* methods in one call (BatchSolver.update_settings); returns the settings in force."""
        return self._b.update_settings(**fields)

    def solve(self):
        info = self._b.solve()[0]
        return int(info.exit_code), self._b.primal()[0]

    def info(self):
        return self._b.info()[0]

    def dual(self):
        return self._b.dual()[0]

    def prim_inf_cert(self):
        """osqp-cpp primal_infeasibility_certificate(): [m], NaN unless the last solve ended primal infeasible."""
        return self._b.prim_inf_cert()[0]

    def dual_inf_cert(self):
        """osqp-cpp dual_infeasibility_certificate(): [n], NaN unless the last solve ended dual infeasible."""
        return self._b.dual_inf_cert()[0]

    def adjoint(self, dx, dy=None):
        """OSQP 1.0 adjoint derivative of the last solve (BatchSolver.adjoint without the batch axis; status is an int)."""
        out = self._b.adjoint(dx, dy)
        return {k: (int(v[0]) if k == "status" else v[0]) for k, v in out.items()}

    def stats(self):
        return self._b.stats()


def debug_host_kkt_solve(P, A, l, u, rhs, tri_waves=0, **settings):
    """Host-only: factor one QP's KKT and solve K sol = rhs twice -- by replaying
    the DEVICE schedules sequentially and by a plain CSC solve.  (No GPU.)
    tri_waves > 0: the dataflow form of the sweeps for that many waves (large single QPs)."""
    L = lib()
    P, A = _csc(P), _csc(A)
    n, m = A.shape[1], A.shape[0]
    s = default_settings(**settings)
    rhs = _f64(rhs)
    sol_s, sol_d = np.empty(n + m), np.empty(n + m)
    st = Stats()
    Pp, Pi, Px = _i64(P.indptr), _i64(P.indices), _f64(P.data)
    Ap, Ai, Ax = _i64(A.indptr), _i64(A.indices), _f64(A.data)
    l, u = _f64(l), _f64(u)
    rc = L.mi_osqp_debug_host_kkt_solve(n, m, _ip(Pp), _ip(Pi), _dp(Px), _ip(Ap), _ip(Ai), _dp(Ax), _dp(l), _dp(u),
                                        C.byref(s), 1 + int(tri_waves), _dp(rhs), _dp(sol_s), _dp(sol_d), C.byref(st))
    _chk(rc, "debug_host_kkt_solve")
    return sol_s, sol_d, st.as_dict()


def prefetch_analysis(P, A, B=1, device=-1, check=True):
    """Pattern analysis of a later setup of B QPs with the patterns of (P, A), computed now into the process-wide cache
    (host work only; blocking - call it from a spare thread).  Returns the C-ABI status."""
    L = lib()
    P, A = _csc(P), _csc(A)
    n, m = A.shape[1], A.shape[0]
    Pp, Pi, Ap, Ai = _i64(P.indptr), _i64(P.indices), _i64(A.indptr), _i64(A.indices)
    rc = L.mi_osqp_prefetch_analysis(B, n, m, _ip(Pp), _ip(Pi), _ip(Ap), _ip(Ai), device)
    if check:
        _chk(rc, "prefetch_analysis")
    return rc


def debug_refactor_chunks(flagged, active, tile, chunk_qps, max_chunks=8):
    """Host-only: the chunks of a pipelined refactorisation.  flagged / active: ascending slots (tile * `tile` + b) that get a new
    factor / iterate on.  Returns (work, tiles): per chunk the flagged slots it refactors and the tiles it iterates; chunk 0
    refactors nothing."""
    f, a = _i64(flagged), _i64(active)
    nch = C.c_int64()
    wb = np.zeros(max_chunks + 2, dtype=np.int64); tb = np.zeros(max_chunks + 2, dtype=np.int64)
    tl = np.zeros(max(1, len(a)), dtype=np.int64)
    _chk(lib().mi_osqp_debug_refactor_chunks(len(f), _ip(f), len(a), _ip(a), tile, chunk_qps, max_chunks, C.byref(nch), _ip(wb), _ip(tl),
                                             _ip(tb)), "debug_refactor_chunks")
    k = int(nch.value)
    return ([f[wb[c]:wb[c + 1]].tolist() for c in range(k)], [tl[tb[c]:tb[c + 1]].tolist() for c in range(k)])


def debug_refactor_lanes(flagged, active, tile, chunk_qps, lanes, kbt=None, chunk0_first=False, scratch_slots=None, max_chunks=8):
    """Host-only: the chunk lanes of a pipelined refactorisation (the chunks are those of debug_refactor_chunks).  kbt: slots
    per workgroup of the refactorisation kernels (default: tile); scratch_slots: what the scratch buffers hold (default: no
    limit).  Returns a dict: n_lanes, lane_of (per chunk), order (per lane, its chunks in launch order), scratch (per chunk:
    (first slot, slots) of its scratch), waits (pairs (c, d): the iterate of chunk c waits for the tail of chunk d, another lane)."""
    f, a = _i64(flagged), _i64(active)
    kbt = tile if kbt is None else kbt
    work, _ = debug_refactor_chunks(flagged, active, tile, chunk_qps, max_chunks)
    k = len(work)
    nl, nw = C.c_int64(), C.c_int64()
    lane_of = np.zeros(max_chunks + 2, dtype=np.int64); order = np.zeros(max_chunks + 2, dtype=np.int64)
    ob = np.zeros(4, dtype=np.int64); sb = np.zeros(max_chunks + 2, dtype=np.int64)
    wc = np.zeros((max_chunks + 1) ** 2, dtype=np.int64); wf = np.zeros((max_chunks + 1) ** 2, dtype=np.int64)
    _chk(lib().mi_osqp_debug_refactor_lanes(len(f), _ip(f), len(a), _ip(a), tile, chunk_qps, max_chunks, kbt, lanes, int(bool(chunk0_first)),
                                            2 ** 31 - 1 if scratch_slots is None else scratch_slots, C.byref(nl), _ip(lane_of), _ip(order),
                                            _ip(ob), _ip(sb), C.byref(nw), _ip(wc), _ip(wf)), "debug_refactor_lanes")
    L = int(nl.value)
    return dict(n_lanes=L, lane_of=lane_of[:k].tolist(), order=[order[ob[l]:ob[l + 1]].tolist() for l in range(L)],
                scratch=[(int(sb[c]), (len(work[c]) + kbt - 1) // kbt * kbt) for c in range(k)],
                waits=list(zip(wc[:nw.value].tolist(), wf[:nw.value].tolist())))


def debug_region_chunks(nq, gw, n_cus):
    """Host-only: the default chunks of a pipelined region of nq flagged QPs beside a run-ahead chain of gw flagged QPs (0:
    no chain) on n_cus CUs.  Returns (QPs per chunk, refactorisation chunks)."""
    q, k = C.c_int64(), C.c_int64()
    _chk(lib().mi_osqp_debug_region_chunks(nq, gw, n_cus, C.byref(q), C.byref(k)), "debug_region_chunks")
    return int(q.value), int(k.value)


def debug_runahead_group(tiles, pri_res, dua_res, size, min_active):
    """Host-only: the run-ahead group of a rho-update point (MI_OSQP_RUNAHEAD).  tiles: the active tiles; pri_res / dua_res:
    their residuals of the check that has just run; size: tiles of the group; min_active: no group when fewer tiles are
    active.  Returns the group's tiles in descending score pri / median(pri) + dua / median(dua), ties by ascending tile."""
    t, p, d = _i64(tiles), _f64(pri_res), _f64(dua_res)
    if not (len(t) == len(p) == len(d)):
        raise ValueError("tiles, pri_res and dua_res differ in length")
    ng = C.c_int64()
    out = np.zeros(max(1, len(t)), dtype=np.int64)
    _chk(lib().mi_osqp_debug_runahead_group(len(t), _ip(t), _dp(p), _dp(d), size, min_active, C.byref(ng), _ip(out)), "debug_runahead_group")
    return out[:ng.value].tolist()


def debug_iterate_form(tiles, has_head=True, forced_form=0, long_min=-1):
    """Host-only: the form of the resident head of S^-1 an iterate launch of `tiles` iterating tiles takes: 0 streamed (a
    handle without a head), 1 deep ring, 2 long head.  forced_form: MI_OSQP_RF_FORM; long_min: MI_OSQP_RF_LONG_MIN (-1 = the
    default)."""
    form = C.c_int64()
    _chk(lib().mi_osqp_debug_iterate_form(tiles, int(bool(has_head)), forced_form, long_min, C.byref(form)), "debug_iterate_form")
    return int(form.value)


def debug_index_words_fit(n, m, tile=1, threads=1024, resident_state=True, lds_vector=True):
    """Host-only: whether the resident iterate of a handle keeps its index words (each thread's entries of pinv and xloc) in
    registers (host_core.hpp index_words_fit; stats()["resident_index_words"]).  Returns (fit, xloc trips a thread may
    have, pinv trips per row kind a thread may have)."""
    fit, xt, pt = C.c_int64(), C.c_int64(), C.c_int64()
    _chk(lib().mi_osqp_debug_index_words_fit(int(bool(resident_state)), int(bool(lds_vector)), tile, threads, n, m,
                                             C.byref(fit), C.byref(xt), C.byref(pt)), "debug_index_words_fit")
    return bool(fit.value), int(xt.value), int(pt.value)


def debug_host_block_factor(P, A, l, u, **settings):
    """Host-only: replay the device block refactorisation and compare with the host
    left-looking factor.  Returns (max rel diff L, max rel diff Dinv, counts dict)."""
    L = lib()
    P, A = _csc(P), _csc(A)
    n, m = A.shape[1], A.shape[0]
    s = default_settings(**settings)
    Pp, Pi, Px = _i64(P.indptr), _i64(P.indices), _f64(P.data)
    Ap, Ai, Ax = _i64(A.indptr), _i64(A.indices), _f64(A.data)
    l, u = _f64(l), _f64(u)
    dL, dD = C.c_double(), C.c_double()
    cnt = (C.c_int64 * 4)()
    rc = L.mi_osqp_debug_host_block_factor(n, m, _ip(Pp), _ip(Pi), _dp(Px), _ip(Ap), _ip(Ai), _dp(Ax), _dp(l), _dp(u),
                                           C.byref(s), C.byref(dL), C.byref(dD), cnt)
    _chk(rc, "debug_host_block_factor")
    return dL.value, dD.value, dict(blocks=cnt[0], triples=cnt[1], storage=cnt[2], levels=cnt[3])
