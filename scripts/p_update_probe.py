"""Cost of new P values on the BASELINE config-4 batch (256 GOMP 7-DOF trajectories, 100 waypoints), beside
objective_update_probe.py: update_P_device (triu(P) already in HBM) against update_P from the host on the same handle in the
same process - the host form is measured twice, before and after, and the distance between its two medians is the spread the
device form is judged against - and update_P_some of 1, 16 and 256 ids in the continuous mode (the call, which only enqueues,
and until the device is idle again).  The blocking calls are timed with HIP events on the current stream around each call,
the per-QP calls by the host clock; best and median of the repetitions."""
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


Ps = [pr["Px"] * (1.0 + 0.01 * k) for k in range(4)]          # the form of setup (the GOMP P holds both triangles): update_P
Pc = pr["P"].tocsc()
upper = Pc.indices <= np.repeat(np.arange(n), np.diff(Pc.indptr))
Pus = [np.ascontiguousarray(P[:, upper]) for P in Ps]         # triu(P), CSC order: the device and per-QP forms
dPs = [torch.tensor(P, dtype=torch.float64, device="cuda:0") for P in Pus]
s = M.BatchSolver(pr["P"], pr["Px"], None, pr["A"], pr["Ax"], pr["l"], pr["u"], device=0)
s.solve()
out = {"config": "config 4: batch of 256 GOMP 7-DOF trajectories, 100 waypoints", "B": B, "n": n, "m": pr["m"], "reps": REPS,
       "nnz_P_triu": int(s.stats()["nnz_P_triu"])}
s.update_P(Ps[0]); s.update_P_device(dPs[0])                  # (first calls: staging buffers)
out["update_P_host_first"] = timed(lambda r: s.update_P(Ps[r % 4]))
out["update_P_device"] = timed(lambda r: s.update_P_device(dPs[r % 4]))
out["update_P_host_second"] = timed(lambda r: s.update_P(Ps[r % 4]))
h1, h2, d = (out[k]["median_ms"] for k in ("update_P_host_first", "update_P_host_second", "update_P_device"))
out["host_spread_ms"] = abs(h1 - h2)
out["device_minus_host_ms"] = d - 0.5 * (h1 + h2)
out["device_not_slower_than_host_by_more_than_its_spread"] = bool(d <= max(h1, h2) + abs(h1 - h2))
# the per-QP form enqueues on the handle's own stream and returns: events on the caller's stream would time the call alone.
# So: wall time of the call (what the host pays), and wall time until the device is idle again (what the listed QPs wait
# for their equilibration, refactorisation and snapshot)
s.solve_begin_some(np.arange(B))
while s.running():
    s.advance(4); s.poll(True)
for k in (1, 16, 256):
    ids = np.arange(k) * (B // k)
    call, done = [], []
    for r in range(REPS):
        rows = Pus[r % 4][ids]
        torch.cuda.synchronize()
        t = time.perf_counter()
        s.update_P_some(ids, rows)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        call.append(1e3 * (t1 - t)); done.append(1e3 * (t2 - t))
    out[f"update_P_some_{k}"] = dict(median_call_ms=float(np.median(call)), best_call_ms=min(call),
                                     median_until_idle_ms=float(np.median(done)), best_until_idle_ms=min(done))
s.solve_begin_some(np.arange(B))
while s.running():
    s.advance(4); s.poll(True)
info = s.info_some(np.arange(B))
out["solve_after_update_P_some"] = dict(optimal=sum(i.exit_code == 0 for i in info), iters=int(sum(i.iter for i in info)))
print(json.dumps(out))
if len(sys.argv) > 2 and sys.argv[1] == "--out":
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
