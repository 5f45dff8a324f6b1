"""Adjoint derivative cost on the headline batch (config 3, B = 1024) against the polish of the same handle in the same
process: HIP events around adjoint_device, last_polish_stats() of the solves in between.  The record goes to
profiles/adjoint/adjoint_probe.json (or to the path behind --out)."""
import os, sys, json
import numpy as np
sys.path.insert(0, os.getcwd())
import torch
import osqp_solver_amd as M
from osqp_solver_amd import problems as PR

torch.cuda.init()
B = 1024
pr = PR.random_box_qp(B)
s = M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], device=0, polish=1)
st = s.stats()
rng = np.random.default_rng(0)
gx = torch.tensor(rng.standard_normal((B, s.n)), device="cuda")
gy = torch.tensor(rng.standard_normal((B, s.m)), device="cuda")
outs = dict(dq=torch.empty((B, s.n), dtype=torch.float64, device="cuda"), dP=torch.empty((B, st["nnz_P_triu"]), dtype=torch.float64, device="cuda"),
            dA=torch.empty((B, st["nnz_A"]), dtype=torch.float64, device="cuda"), dl=torch.empty((B, s.m), dtype=torch.float64, device="cuda"),
            du=torch.empty((B, s.m), dtype=torch.float64, device="cuda"), status=torch.empty(B, dtype=torch.int32, device="cuda"))
rows = []
for step in range(7):
    s.reset(); s.solve()
    pol = s.last_polish_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.current_stream()
    e0.record(stream)
    s.adjoint_device(gx, gy, stream=stream.cuda_stream, **outs)
    e1.record(stream)
    torch.cuda.synchronize()
    rows.append(dict(adjoint_ms=e0.elapsed_time(e1), polish_ms=pol["seconds"] * 1e3, polished=pol["polished"], accepted=pol["accepted"],
                     computed=int((outs["status"] == 1).sum())))
warm = rows[1:]                                    # (the first round allocates the adjoint's marks and sets the LDS attribute)
out = dict(B=B, n=s.n, m=s.m, gradient_bytes_per_qp=8 * (2 * s.n + 2 * s.m + st["nnz_P_triu"] + st["nnz_A"]), rounds=rows,
           adjoint_ms_median=float(np.median([r["adjoint_ms"] for r in warm])), polish_ms_median=float(np.median([r["polish_ms"] for r in warm])))
out["ratio"] = out["adjoint_ms_median"] / out["polish_ms_median"]
path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "adjoint", "adjoint_probe.json")
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out), flush=True)
