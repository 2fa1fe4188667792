#!/usr/bin/env python3
"""Per-box-tier times of the one-GPU 2^32 solve from a rocprofv3 kernel trace.

    python tools/box_tier_trace.py <trace dir> [--json out.json] [--mirror [SET]] [--last N] [--hybrid LO,HI]

--mirror: the groups of the compute list (GM_OPT_SYMMETRY 1), SET as GM_BOX_MIRROR_SET: 1 (the
default of the flag alone) = of the boxes that differ by the exchange of heaps 6 and 7 only the
one with c6 >= c7 is computed, 3 = also only c4 >= c5 of heaps 4 and 5, 7 (with --hybrid) = also
only c2 >= c3 of heaps 2 and 3 in the dataflow launches' tiers; --last N: the last N
solves of the trace only (the bench's timed solves, without its warm-up); --hybrid LO,HI: the
trace is of the hybrid schedule (GM_BOX_HYBRID): box-tiers [0, LO) and (HI, 40] are one launch of
box_flow_kernel<false, true> each, shown as one row covering its tier range (groups, time and
time at throughput summed over the range).

The trace is of `bench.py` (one GPU, box engine): every solve is 41 launches of
box_tier_kernel<false>, box-tier 0 first.  Per box-tier: its groups (two boxes each: the boxes
of the 4x4x4x4x2x2x2x2 lattice whose coordinates sum to the tier), the median launch duration
over the traced solves, and what the tier would take at the throughput of the thick tiers
(groups / (groups per us of the tiers with >= 2 resident rounds)).  A thin tier (fewer groups
than one resident round of 2,048) pays for its latency chain; the sum of (duration - time at
throughput) over them is all that any thin-tier scheme could save at N = 1.
"""
import argparse
import csv
import glob
import json

import numpy as np


def tier_groups(mirror=0):
    b = np.arange(1 << 20)
    t = sum((b >> (2 * i)) & 3 for i in range(4)) + sum((b >> (8 + 3 * j)) & 7 for j in range(4))
    keep = np.ones(1 << 20, bool)
    if mirror & 1:
        keep &= ((b >> 14) & 7) >= ((b >> 17) & 7)
    if mirror & 2:
        keep &= ((b >> 8) & 7) >= ((b >> 11) & 7)
    if mirror & 4:
        keep &= ((b >> 4) & 3) >= ((b >> 6) & 3)
    t = t[keep]
    n = np.bincount(t, minlength=41)
    return (n + 1) // 2


def hybrid_report(a, segs, n, dur, span, med, g):
    """One row per launch; the thick-tier rate from the tier launches of >= 2 resident rounds."""
    single = [(i, s[0]) for i, s in enumerate(segs) if s[0] == s[1] and g[s[0]] >= 2 * a.round]
    if not single:
        raise SystemExit("no thick tier launch in the range")
    rate = sum(g[t] for _, t in single) / sum(med[i] for i, _ in single)
    out = {"solves": int(n), "hybrid": a.hybrid, "solve_span_us_median": float(np.median(span)),
           "launch_sum_us_median": float(np.median(dur.sum(axis=1))),
           "thick_tier_rate_groups_per_us": float(rate), "tiers": []}
    print("tiers   groups      us   at-throughput")
    for i, (t0, t1) in enumerate(segs):
        gr = int(g[t0:t1 + 1].sum())
        out["tiers"].append({"tier": t0, "last_tier": t1, "groups": gr, "us": round(float(med[i]), 2),
                             "us_at_throughput": round(gr / rate, 2), "flow": t1 > t0 or t0 < int(a.hybrid.split(",")[0])
                             or t0 > int(a.hybrid.split(",")[1])})
        print("%-6s %7d %8.2f %8.2f%s" % ("%d-%d" % (t0, t1) if t1 > t0 else "%d" % t0, gr, med[i], gr / rate,
                                          "  flow" if out["tiers"][-1]["flow"] else ""))
    fl = [r for r in out["tiers"] if r["flow"]]
    print("solves %d: span %.1f us (median), launch sum %.1f us; thick-tier rate %.1f groups/us" %
          (n, out["solve_span_us_median"], out["launch_sum_us_median"], rate))
    print("flow launches (%d): %.1f us, %.1f us at throughput" %
          (len(fl), sum(r["us"] for r in fl), sum(r["us_at_throughput"] for r in fl)))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--json", default=None)
    ap.add_argument("--round", type=int, default=2048, help="groups per resident round")
    ap.add_argument("--mirror", type=int, nargs="?", const=1, default=0,
                    help="groups of the mirrors' compute list (GM_BOX_MIRROR_SET; alone: 1, heaps 6/7)")
    ap.add_argument("--last", type=int, default=0, help="use only the last N solves (0: all)")
    ap.add_argument("--hybrid", default=None, metavar="LO,HI", help="the hybrid schedule's tier range (GM_BOX_HYBRID)")
    a = ap.parse_args()
    # the launches of a solve, each covering box-tiers [first, last]
    lo, hi = (int(x) for x in a.hybrid.split(",")) if a.hybrid else (0, 40)
    lo = min(lo, 41)
    segs = ([(0, lo - 1)] if lo > 0 else []) + [(t, t) for t in range(lo, hi + 1)]
    if max(hi + 1, lo) < 41:
        segs.append((max(hi + 1, lo), 40))
    per = len(segs)
    rows = []
    for f in glob.glob(a.trace + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if ("box_tier_kernel<false" in r["Kernel_Name"] or "box_tier4_kernel<false" in r["Kernel_Name"] or
                    (a.hybrid and "box_flow_kernel<false, true>" in r["Kernel_Name"])):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    n = len(rows) // per
    if n == 0:
        raise SystemExit("no complete solve in the trace")
    if a.last:
        n = min(n, a.last)
    rows = rows[-per * n:]
    dur = np.array([(e - s) / 1e3 for s, e in rows]).reshape(n, per)        # us
    span = np.array([(rows[per * i + per - 1][1] - rows[per * i][0]) / 1e3 for i in range(n)])
    med = np.median(dur, axis=0)
    g = tier_groups(a.mirror & 3)
    if a.mirror & 4 and a.hybrid:   # the heap-2/3 mirror: the dataflow launches' tiers only
        flow = np.array([t < lo or t > hi for t in range(41)])
        g = np.where(flow, tier_groups(a.mirror), g)
    if a.hybrid:
        return hybrid_report(a, segs, n, dur, span, med, g)
    thick = g >= 2 * a.round
    rate = g[thick].sum() / med[thick].sum()                                # groups per us
    ideal = g / rate
    thin = g < a.round
    excess = np.maximum(0.0, med - ideal)
    out = {"solves": int(n), "solve_span_us_median": float(np.median(span)),
           "launch_sum_us_median": float(np.median(dur.sum(axis=1))),
           "thick_tier_rate_groups_per_us": float(rate),
           "thin_tiers": [int(t) for t in np.nonzero(thin)[0]],
           "thin_tier_us": float(med[thin].sum()), "thin_tier_us_at_throughput": float(ideal[thin].sum()),
           "thin_tier_excess_us": float(excess[thin].sum()),
           "tiers": [{"tier": t, "groups": int(g[t]), "us": round(float(med[t]), 2),
                      "us_at_throughput": round(float(ideal[t]), 2)} for t in range(41)]}
    print("tier  groups      us   at-throughput")
    for t in range(41):
        print("%4d %7d %8.2f %8.2f%s" % (t, g[t], med[t], ideal[t], "  thin" if thin[t] else ""))
    print("solves %d: span %.1f us (median), launch sum %.1f us; thick-tier rate %.1f groups/us" %
          (n, out["solve_span_us_median"], out["launch_sum_us_median"], rate))
    print("thin tiers (%d): %.1f us, %.1f us at throughput, excess %.1f us = %.1f %% of the span" %
          (thin.sum(), out["thin_tier_us"], out["thin_tier_us_at_throughput"], out["thin_tier_excess_us"],
           100 * out["thin_tier_excess_us"] / out["solve_span_us_median"]))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
