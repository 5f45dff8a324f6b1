"""Timeline of the rho-update region of the last benchmark step, from a rocprofv3 kernel trace.

usage: python scripts/region_timeline.py [--step] TRACE_DIR [LABEL]      (--step: the whole last step instead, see last_step)
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


def last_step(rows, label):
    """--step: every kernel of the last benchmark step (from the first iterate behind the last but one gather_status_kernel to
    the last one), and two spans from the end of the last full-grid check in front of the refactorisation: (a) to the end of
    the last kernel of a chunk lane, (b) to the end of the run-ahead chain's last check.  The chain's stream is the one with
    the most checks of less than half the grid; the lanes are the streams that are neither it nor the stream of the full launches."""
    g = [i for i, r in enumerate(rows) if r[2] == "gather_status_kernel"]
    if len(g) < 2:
        sys.exit("fewer than two steps in the trace")
    lo = next(i for i in range(g[-2], g[-1]) if rows[i][2] == "iterate_kernel")
    step = rows[lo:g[-1] + 1]
    full = max(r[4] for r in step if r[2] == "check_kernel")
    first_factor = next((i for i, r in enumerate(step) if r[2] == "factor_kernel"), None)
    ids, t00, prev_end = {}, step[0][0], step[0][0]
    print(f"== {label} last step (us from its first launch)")
    for s, e, name, stream, wgs in step:
        sid = ids.setdefault(stream, len(ids) + 1)
        print(f"{name:<26} st {sid} wgs {wgs:5d} start {(s - t00) / 1e3:9.1f} end {(e - t00) / 1e3:9.1f} dur {(e - s) / 1e3:8.1f} gap {(s - prev_end) / 1e3:8.1f}")
        prev_end = e
    if first_factor is None:
        return
    t0 = max(r[1] for r in step[:first_factor] if r[2] == "check_kernel" and 2 * r[4] > full)
    after = [r for r in step if r[0] >= t0]
    small = defaultdict(int)
    for r in after:
        if r[2] == "check_kernel" and 2 * r[4] <= full:
            small[r[3]] += 1
    main_stream = step[0][3]
    chain = max(small, key=small.get) if small else main_stream
    lanes = [r for r in after if r[3] not in (chain, main_stream)]
    chain_end = max((r[1] for r in after if r[3] == chain and r[2] == "check_kernel" and 2 * r[4] <= full), default=t0)
    if lanes:
        print(f"(a) end of the check in front of the region -> end of the last lane kernel: {(max(r[1] for r in lanes) - t0) / 1e6:.3f} ms")
    print(f"(b) end of the check in front of the region -> end of the chain's last check (stream {ids[chain]}): {(chain_end - t0) / 1e6:.3f} ms")
    print(f"    step: first launch -> gather_status_kernel: {(step[-1][1] - t00) / 1e6:.3f} ms")


def main():
    want_step = "--step" in sys.argv
    if want_step:
        sys.argv.remove("--step")
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
    if want_step:
        return last_step(rows, label)
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
