#!/usr/bin/env python3
"""Per-kernel averages of every counter in rocprofv3 --pmc csv runs.

usage: python tools/pmc_sq_summary.py OUT_CSV NAME=run_counter_collection.csv [NAME=...]

One row per (run, kernel): dispatches, average duration (the profiled
duration: counters slow a kernel down) and the per-dispatch average of each
counter; kernels are shortened to their function name with template
arguments.
"""
import csv
import re
import sys
from collections import defaultdict


def short(name):
    m = re.match(r"(?:void )?([\w:]+(?:<[^()]*>)?)\(", name)
    return m.group(1) if m else name


def load(path):
    val = defaultdict(lambda: defaultdict(dict))  # kernel -> counter -> dispatch -> value
    dur = defaultdict(dict)
    for r in csv.DictReader(open(path)):
        k, d = short(r["Kernel_Name"]), int(r["Dispatch_Id"])
        val[k][r["Counter_Name"]][d] = float(r["Counter_Value"])
        dur[k][d] = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    return val, dur


def main(out, specs):
    rows, counters = [], []
    for spec in specs:
        run, path = spec.split("=", 1)
        val, dur = load(path)
        for k in sorted(val, key=lambda k: -sum(dur[k].values())):
            row = {"run": run, "kernel": k, "dispatches": len(dur[k]),
                   "avg_duration_us": round(sum(dur[k].values()) / len(dur[k]) / 1e3, 2)}
            for c, per in sorted(val[k].items()):
                row[c] = round(sum(per.values()) / len(per), 1)
                if c not in counters:
                    counters.append(c)
            rows.append(row)
    with open(out, "w", newline="") as fh:
        w = csv.DictWriter(fh, fieldnames=["run", "kernel", "dispatches", "avg_duration_us"] + counters)
        w.writeheader()
        w.writerows(rows)
    for r in rows:
        if r["dispatches"] and r["avg_duration_us"] > 1000:
            print(r)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
