"""Timeline of the rho-update region of the last benchmark step, from a rocprofv3 kernel trace.

usage: python scripts/region_timeline.py TRACE_DIR [LABEL]
TRACE_DIR: what `rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -- python bench.py --steps 3 --warmup 1` wrote.
Prints every kernel between the last two check_kernel launches of the solve loop (more than half the largest check grid: the
checks of a run-ahead group's chain lie inside the region) that have a long refactorisation between them (more than 500
factor_kernel workgroups: the check at iteration 100 and the one at 125 of the headline batch) with its stream or queue,
workgroups, start, end and duration in us from the end of the first check, then the per-kernel totals of the whole run."""
import csv
import glob
import os
import sys
from collections import defaultdict


def short(name):
    name = name.split("(")[0].split("<")[0]
    return name.split("::")[-1].replace("void ", "").strip()


def main():
    d, label = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "")
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {d}")
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            wg = max(1, int(r.get("Workgroup_Size_X", r.get("Workgroup_Size", 1)) or 1))
            grid = int(r.get("Grid_Size_X", r.get("Grid_Size", wg)) or wg)
            stream = r.get("Stream_Id") or r.get("Queue_Id") or "?"
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), stream, grid // wg))
    rows.sort()
    # the checks of the solve loop: the full grid, or everyone but a run-ahead group (whose own checks, over the group's tiles
    # only, sit inside the region)
    full = max((r[4] for r in rows if r[2] == "check_kernel"), default=0)
    checks = [i for i, r in enumerate(rows) if r[2] == "check_kernel" and 2 * r[4] > full]
    region = None
    for a, b in zip(checks, checks[1:]):
        if sum(r[4] for r in rows[a + 1:b] if r[2] == "factor_kernel") > 500:
            region = (a, b)
    print(f"== {label} region after the check at iteration 100 of the last step (us from the end of that check)")
    if region:
        a, b = region
        t0 = rows[a][1]
        ids = {}
        for s, e, name, stream, wgs in rows[a + 1:b + 1]:
            sid = ids.setdefault(stream, len(ids) + 1)
            print(f"  {name:<24} stream {sid}  wgs {wgs:4d}  start {(s - t0) / 1e3:8.1f}  end {(e - t0) / 1e3:8.1f}  dur {(e - s) / 1e3:8.1f}")
        print(f"  region: end of check(100) -> start of check(125): {(rows[b][0] - t0) / 1e6:.3f} ms")
    else:
        print("  (no such region found)")
    tot = defaultdict(lambda: [0, 0])
    for s, e, name, _, _ in rows:
        tot[name][0] += 1; tot[name][1] += e - s
    for name, (n, ns) in sorted(tot.items(), key=lambda kv: -kv[1][1])[:8]:
        print(f"  {name:<24} calls {n:4d} total {ns / 1e6:8.2f} ms avg {ns / 1e6 / n:.3f} ms")


if __name__ == "__main__":
    main()
