"""List-scheduling model of the rho-update region ("Measurements (chunk lanes)"): try a schedule on the CPU
before building it.

usage: python scripts/refactor_schedule_model.py [--cus 256] [--flagged 605] [--active 634] [--f 0.54 --a 0.21 --t 0.75 --i 0.95]

Every kernel is a set of workgroups that each take one CU for a constant time (--f factor_kernel, --a tail_assemble_kernel,
--t tail_kernel, --i a chunk iterate: ms of a chunk of ~200 QPs run alone); a free CU takes the next ready workgroup; a
stream starts its next kernel when the previous one has drained and the kernels it waits for have ended.  What the model does
NOT know: a kernel runs slower beside another one (factor_kernel 0.54 -> 1.3 ms beside a chunk iterate), and streams that
share a hardware queue serialise (the third lane did, profiles/r08/region_lanes3.txt).  It ranks schedules; the trace decides."""
import argparse
import heapq


def simulate(streams, cus):
    """streams: list of lists of kernels (name, workgroups, ms per workgroup, names it waits for); returns (makespan, ends)."""
    ends, pos = {}, [0] * len(streams)
    free_at = [0.0] * cus                      # a heap of the times at which the CUs fall free
    heapq.heapify(free_at)
    drained = [0.0] * len(streams)
    todo = sum(len(s) for s in streams)
    while todo:
        # the stream whose next kernel becomes ready first
        best = None
        for k, s in enumerate(streams):
            if pos[k] == len(s):
                continue
            name, wgs, dur, waits = s[pos[k]]
            if any(w not in ends for w in waits):
                continue
            ready = max([drained[k]] + [ends[w] for w in waits])
            if best is None or ready < best[0]:
                best = (ready, k)
        ready, k = best
        name, wgs, dur, _ = streams[k][pos[k]]
        end = ready
        for _ in range(wgs):
            t = max(heapq.heappop(free_at), ready) + dur
            heapq.heappush(free_at, t)
            end = max(end, t)
        ends[name] = drained[k] = end
        pos[k] += 1
        todo -= 1
    return max(ends.values()), ends


def chain(c, n, d):
    return [(f"F{c}", n, d["f"], []), (f"A{c}", n, d["a"], []), (f"T{c}", n, d["t"], [])]


def schedules(chunks, rest, d):
    n = len(chunks)
    out = {}
    tot = sum(chunks)
    out["serial"] = [[("F", tot, d["f"], []), ("A", tot, d["a"], []), ("T", tot, d["t"], []), ("I", tot + rest, d["i"], [])]]
    r = [k for c, q in enumerate(chunks, 1) for k in chain(c, q, d)]
    i = [("I0", rest, d["i"], [])] + [(f"I{c}", q, d["i"], [f"T{c}"]) for c, q in enumerate(chunks, 1)]
    out["one lane (two streams)"] = [r, i]
    for lanes in (2, 3):
        for first in (False, True):
            ls = [[] for _ in range(lanes)]
            for c, q in enumerate(chunks, 1):
                ls[(c - 1) % lanes] += chain(c, q, d) + [(f"I{c}", q, d["i"], [])]
            if first:
                ls[-1].insert(0, ("I0", rest, d["i"], []))
            else:
                at = max(range(lanes), key=lambda a: (-len(ls[a]), a))
                ls[at].append(("I0", rest, d["i"], []))
            out[f"{lanes} lanes x {n} chunks, chunk 0 {'first' if first else 'last'}"] = ls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--flagged", type=int, default=605)
    ap.add_argument("--active", type=int, default=634)
    for k, v in (("f", 0.54), ("a", 0.21), ("t", 0.75), ("i", 0.95)):
        ap.add_argument("--" + k, type=float, default=v)
    a = ap.parse_args()
    d = {k: getattr(a, k) for k in "fati"}
    for n in (3, 4, 6):
        q = (a.flagged + n - 1) // n
        chunks = [min(q, a.flagged - c * q) for c in range(n)]
        for name, s in schedules(chunks, a.active - a.flagged, d).items():
            if n > 3 and not name[0].isdigit():
                continue
            print(f"{name:<42} {simulate(s, a.cus)[0]:.2f} ms")


if __name__ == "__main__":
    main()
