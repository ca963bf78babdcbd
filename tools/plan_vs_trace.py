#!/usr/bin/env python3
"""Compare the launches tests/launch_plan.py plans with what a rocprofv3 kernel trace shows, call by call.

usage: plan_vs_trace.py <rocprofv3 output dir> <plan log> [--calls]

The plan log is what tests/test_gpu_selection_boundaries.py appends under HE355_PLAN_LOG=<file> (one JSON line per call: the planned
kernel families, grids in blocks and block sizes, and the outcome of every selection decision); the trace is the *kernel_trace.csv of
    HE355_PLAN_LOG=<file> KTRACE_DIR=<dir> tools/ktrace.sh <out> 1 -m pytest tests/test_gpu_selection_boundaries.py -m gpu -q
(kernel trace and stats only: no counters in that run).  The trace is put into dispatch order and cut down to the kernel families a
plan can name; each call then consumes as many dispatches as it planned, and family, grid and block size must agree one by one.
Calls without planned launches (a BFV context's coefficient-form key switch) must come last: what they dispatch is left over.
Prints one line per (chain, op), the decisions table -- how many calls took each outcome, planned and confirmed by the trace -- and
the first disagreements in full.  Exit status 1 on any disagreement."""
import csv
import glob
import json
import os
import re
import sys

FAMILIES = {"k_k1", "k_k1_dual", "k_k2n", "k_k2n_dual", "k_k3", "k_k3_dual", "k_k3_dual8", "k_k3_combine", "k_floor_colsn", "k_floor_rows",
            "k_floor_rows_dual", "k_rows_inv_select", "k_lds_digits", "k_lds_floor"}


def family(name):
    m = re.search(r"\b(k_[a-z0-9_]+)\s*(<|\(|$)", name)
    return m.group(1) if m else None


def read_trace(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {d}")
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            col = {k.lower(): v for k, v in r.items()}
            fam = family(col.get("kernel_name", ""))
            if fam not in FAMILIES:
                continue
            wg = [int(col[f"workgroup_size_{a}"]) for a in "xy"]
            gr = [int(col[f"grid_size_{a}"]) for a in "xy"]
            order = int(col.get("dispatch_id") or col.get("start_timestamp"))
            rows.append((order, fam, gr, wg))
    rows.sort(key=lambda x: x[0])
    return rows


def main():
    d, log = sys.argv[1], sys.argv[2]
    show_calls = "--calls" in sys.argv
    calls = [json.loads(l) for l in open(log) if l.strip()]
    trace = read_trace(d)
    # rocprofv3 reports the grid in work-items: blocks = grid / workgroup size (checked on the first planned dispatch)
    pos, bad, per_case, decided = 0, [], {}, {}
    in_items = None
    for c in calls:
        want = c["launches"]
        got = trace[pos:pos + len(want)]
        pos += len(want)
        ok = len(got) == len(want)
        for w, t in zip(want, got):
            _, fam, gr, wg = t
            if in_items is None:
                in_items = not (gr[0] == w[1] and wg[0] * w[1] != gr[0])
            blocks = [gr[0] // wg[0], gr[1] // max(1, wg[1])] if in_items else gr
            if (fam, blocks[0], blocks[1], wg[0]) != (w[0], w[1], w[2], w[3]):
                ok = False
        key = (c["chain"], c["op"], c["L"])
        e = per_case.setdefault(key, [0, 0, set()])
        e[0] += 1
        e[1] += ok
        e[2].add(c["n"])
        for dname, o in c["outcomes"]:
            x = decided.setdefault((dname, o), [0, 0])
            x[0] += 1
            x[1] += ok
        if not ok:
            bad.append((c, [(t[1], t[2], t[3]) for t in got]))
        if show_calls:
            print(f"{'ok ' if ok else 'BAD'} {c['chain']} {c['op']} L={c['L']} n={c['n']} chunk={c['chunk']}: {len(want)} launches")
    print(f"{len(calls)} calls, {sum(len(c['launches']) for c in calls)} planned launches, {len(trace)} traced dispatches of the planned families"
          f" ({len(trace) - pos} left over after the last planned call)")
    print("\ncase table: calls, calls whose trace agrees with the plan, batch sizes")
    for (ch, op, L), (n, ok, ns) in per_case.items():
        print(f"  {ch:32s} {op:30s} L={L:<2d} {n:3d} {ok:3d}  {sorted(ns)}")
    print("\ndecision, outcome: calls that planned it, calls of those whose trace agrees")
    for (dname, o), (n, ok) in sorted(decided.items()):
        print(f"  {dname:13s} {o:15s} {n:4d} {ok:4d}")
    for c, got in bad[:5]:
        print(f"\nDISAGREES: {c['chain']} {c['op']} L={c['L']} n={c['n']} chunk={c['chunk']}")
        print("  planned:", c["launches"])
        print("  traced: ", got)
    print(f"\n{len(bad)} calls disagree")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
