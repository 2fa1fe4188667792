#!/usr/bin/env python3
"""Per-box-tier HBM bytes and bandwidth of the one-GPU 2^32 solve: the per-dispatch FETCH_SIZE
(x 2, tools/pmc_summary.py) and WRITE_SIZE counters of one solve over the per-tier times of
tools/box_tier_trace.py --json.

    python tools/box_tier_traffic.py FETCH.csv WRITE.csv TRACE.json

A trace of the hybrid schedule (box_tier_trace.py --hybrid) has one row per launch: a dataflow
launch (box_flow_kernel<false, true>) is one row covering its tier range.
"""
import csv
import json
import sys


def per_tier(path, name):
    d = {}
    for r in csv.DictReader(open(path)):
        if (("box_tier_kernel" in r["Kernel_Name"] or "box_flow_kernel<false, true>" in r["Kernel_Name"])
                and r["Counter_Name"] == name):
            d[int(r["Dispatch_Id"])] = d.get(int(r["Dispatch_Id"]), 0.0) + float(r["Counter_Value"])
    return [d[i] * 1024 for i in sorted(d)]   # KiB -> bytes


def main():
    tr = json.load(open(sys.argv[3]))["tiers"]
    nl = len(tr)   # launches per solve: 41, fewer with the hybrid schedule
    f, w = per_tier(sys.argv[1], "FETCH_SIZE")[-nl:], per_tier(sys.argv[2], "WRITE_SIZE")[-nl:]   # the last solve
    print("tier   groups  read MB  write MB       us   TB/s  read/write")
    for t in range(nl):
        b = 2 * f[t] + w[t]
        last = tr[t].get("last_tier", tr[t]["tier"])
        name = "%d-%d" % (tr[t]["tier"], last) if last > tr[t]["tier"] else "%d" % tr[t]["tier"]
        print("%-5s %7d %8.1f %9.1f %8.2f %6.2f %8.3f" % (name, tr[t]["groups"], 2 * f[t] / 1e6, w[t] / 1e6, tr[t]["us"],
                                                         b / tr[t]["us"] / 1e6, 2 * f[t] / w[t]))
    thick = [t for t in range(nl) if tr[t]["groups"] >= 4096 and not tr[t].get("flow")]
    B, T = sum(2 * f[t] + w[t] for t in thick), sum(tr[t]["us"] for t in thick)
    print("thick tiers (%d, >= 4096 groups): %.2f GB in %.1f us = %.2f TB/s" % (len(thick), B / 1e9, T, B / T / 1e6))
    B, T = sum(2 * f[t] + w[t] for t in range(nl)), sum(tr[t]["us"] for t in range(nl))
    print("all launches: %.2f GB in %.1f us = %.2f TB/s" % (B / 1e9, T, B / T / 1e6))


if __name__ == "__main__":
    main()
