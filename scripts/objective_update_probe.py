"""Cost of a new objective vector on the BASELINE config-4 batch (256 GOMP 7-DOF trajectories, 100 waypoints): update_q_device
(q already in HBM), update_q (host q), update_P, against what was needed before - a new setup of the batch with that q.
Times are HIP events on the current stream around each call (the calls block), best and median of the repetitions."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import torch
import osqp_solver_amd as M
from osqp_solver_amd import problems as PR

REPS = 20
torch.cuda.init()
pr = PR.gomp_batch(256, 7, 100)
B, n = pr["l"].shape[0], pr["n"]
q0 = np.zeros((B, n))


def mk(q):
    return M.BatchSolver(pr["P"], pr["Px"], q, pr["A"], pr["Ax"], pr["l"], pr["u"], device=0)


def timed(fn, reps=REPS):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms, wall = [], []
    for r in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        ev0.record()
        fn(r)
        ev1.record()
        ev1.synchronize()
        wall.append(1e3 * (time.perf_counter() - t))
        ms.append(ev0.elapsed_time(ev1))
    return dict(best_ms=min(ms), median_ms=float(np.median(ms)), median_wall_ms=float(np.median(wall)))


rng = np.random.default_rng(5)
qs = [0.1 * rng.standard_normal((B, n)) for _ in range(4)]
dqs = [torch.tensor(q, dtype=torch.float64, device="cuda:0") for q in qs]
s = mk(q0)
s.solve()
out = {"config": "config 4: batch of 256 GOMP 7-DOF trajectories, 100 waypoints", "B": B, "n": n, "m": pr["m"], "reps": REPS}
out["update_q_device"] = timed(lambda r: s.update_q_device(dqs[r % 4]))
out["update_q"] = timed(lambda r: s.update_q(qs[r % 4]))
out["update_P"] = timed(lambda r: s.update_P(pr["Px"] * (1.0 + 0.01 * (r % 4))))
keep = []
out["re_setup"] = timed(lambda r: keep.append(mk(qs[r % 4])) or (len(keep) > 2 and keep.pop(0).close()))
out["speedup_vs_re_setup"] = out["re_setup"]["median_ms"] / out["update_q_device"]["median_ms"]
s.update_q(qs[0]); info = s.solve()
out["solve_after_update_q"] = dict(optimal=sum(i.exit_code == 0 for i in info), iters=int(sum(i.iter for i in info)))
print(json.dumps(out))
if len(sys.argv) > 2 and sys.argv[1] == "--out":
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
