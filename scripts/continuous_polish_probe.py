"""Cost of polishing on demand in the continuous mode: wall time from polish_some of 16 kOptimal QPs to
the poll() that reports them, nothing else running on the handle, next to last_polish_stats()["seconds"] of the blocking
polish of the same QPs.  Single measurements.  (Run from the repository root; a library without polish_some gives the blocking
figures only.)"""
import json, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import osqp_solver_amd as M
from osqp_solver_amd import problems as PR

pr = PR.random_box_qp(16, n=96, mg=64, nnz_per_row=6)
mk = lambda **kw: M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **kw)
out = {}
b = mk(polish=1)
info = b.solve()
out["blocking_first"] = b.last_polish_stats()
b.solve()
out["blocking_second"] = b.last_polish_stats()
if hasattr(M.BatchSolver, "polish_some"):
    s = mk()
    def drain():
        while s.running():
            s.advance(1); s.poll(True)
    for rnd in ("first_with_allocation", "second"):
        s.solve_begin_some(range(16)); drain()
        opt = [q for q, i in enumerate(s.info_some(range(16))) if i.status_val == 1]
        t0 = time.perf_counter()
        s.polish_some(opt)
        t1 = time.perf_counter()
        s.advance(1)
        got = s.poll(True)
        t2 = time.perf_counter()
        assert sorted(got) == opt
        out["continuous_" + rnd] = dict(qps=len(opt), call_s=t1 - t0, to_report_s=t2 - t0, stats=s.last_polish_stats())
print(json.dumps(out))
