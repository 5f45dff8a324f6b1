"""Polish cost on the headline batch and the accuracy table (configs 2, 3, 4)."""
import os, sys, time, json
import numpy as np
sys.path.insert(0, os.getcwd())
import torch
import osqp_solver_amd as M
from osqp_solver_amd import problems as PR
from oracle.kkt_check import kkt_residuals

out = {}
timing_only = "--timing-only" in sys.argv
torch.cuda.init()
pr = PR.random_box_qp(1024)
def mk(**kw):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], device=0, **kw)
free0 = torch.cuda.mem_get_info()[0]
s1 = mk(polish=1)
free1 = torch.cuda.mem_get_info()[0]
s1.reset(); s1.solve()
free2 = torch.cuda.mem_get_info()[0]
out["polish_buffer_bytes_per_qp"] = (free1 - free2) / 1024
rows = []
for step in range(6):
    s1.reset()
    t = time.perf_counter(); s1.solve(); wall = time.perf_counter() - t
    rows.append(dict(wall_ms=wall * 1e3, **s1.last_polish_stats()))
out["headline_polish"] = rows
if not timing_only:
    s0 = mk()
    w0 = []
    for step in range(6):
        s0.reset(); t = time.perf_counter(); s0.solve(); w0.append((time.perf_counter() - t) * 1e3)
    out["headline_wall_ms_polish0"] = w0
    del s0
del s1
print(json.dumps(out), flush=True)
if timing_only:
    sys.exit(0)
table = {}
for name, p in (("config 2", PR.gomp_batch(1, 6, 50)), ("config 3", PR.random_box_qp(256)), ("config 4", PR.gomp_batch(256, 7, 100))):
    for pol in (0, 1):
        s = M.BatchSolver(p["P"], p["Px"], p["q"], p["A"], p["Ax"], p["l"], p["u"], device=0, polish=pol)
        info = s.solve(); x, y = s.primal(), s.dual()
        res = []
        for b in range(s.B):
            P, A = PR.qp_matrices(p, b)
            r = kkt_residuals(P, None if p["q"] is None else p["q"][b], A, p["l"][b], p["u"][b], x[b], y[b])
            res.append(max(r["prim"], r["stat"], r["comp"]))
        res = np.array(res)
        st = s.last_polish_stats()
        table[f"{name} polish={pol}"] = dict(B=s.B, optimal=int(sum(i.status_val == 1 for i in info)), polished=st["polished"],
                                             accepted=st["accepted"], polish_ms=st["seconds"] * 1e3,
                                             kkt_median=float(np.median(res)), kkt_max=float(res.max()))
        print(name, pol, table[f"{name} polish={pol}"], flush=True)
        s.close()
print(json.dumps({"accuracy": table}), flush=True)
