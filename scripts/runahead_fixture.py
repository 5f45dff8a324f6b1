"""Writes tests/golden/runahead_residuals.json, the fixture of tests/test_runahead_group.py: what the oracle records for a fixed
sample of the headline batch (problems.random_box_qp(1024, value_seed=1000), every STEP-th QP) - pri_res / dua_res after 100
iterations of the QPs that have not finished by then, and the iteration count of their full solve.  CPU only.

usage: python scripts/runahead_fixture.py [STEP]        (default 4: 256 QPs)"""
import json
import os
import sys
from multiprocessing.pool import ThreadPool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O                       # noqa: E402
from osqp_solver_amd import problems as PR           # noqa: E402

KW = dict(adaptive_rho_interval=100)                 # the interval the device derives for this batch


def main():
    step = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    pr = PR.random_box_qp(1024, value_seed=1000)
    O.lib()

    def one(b):
        P, A = PR.qp_matrices(pr, b)
        o = O.OracleQPSolver(P, pr["q"][b], A, pr["l"][b], pr["u"][b], max_iter=100, **KW)
        st, _ = o.solve()
        i100 = o.info()
        if st not in (-2, 2):                        # finished within 100 iterations (at max_iter the oracle reports -2, or 2 where
            return None                              # the tenfold tolerances hold: both go on in a longer solve)
        full = O.OracleQPSolver(P, pr["q"][b], A, pr["l"][b], pr["u"][b], **KW)
        full.solve()
        return b, float(i100.pri_res), float(i100.dua_res), int(full.info().iter)

    with ThreadPool(min(16, os.cpu_count() or 1)) as pool:
        rows = [r for r in pool.map(one, range(0, 1024, step)) if r is not None]
    out = {"batch": "problems.random_box_qp(1024, value_seed=1000)", "sample": f"range(0, 1024, {step})", "settings": KW,
           "at_iteration": 100, "qp": [r[0] for r in rows], "pri_res": [r[1] for r in rows], "dua_res": [r[2] for r in rows],
           "iterations": [r[3] for r in rows]}
    path = os.path.join(ROOT, "tests", "golden", "runahead_residuals.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    hist = {}
    for r in rows:
        hist[r[3]] = hist.get(r[3], 0) + 1
    print(f"{len(rows)} active after 100 iterations of {len(range(0, 1024, step))}; iterations of the full solve: {sorted(hist.items())}")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
