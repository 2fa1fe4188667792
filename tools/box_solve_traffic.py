#!/usr/bin/env python3
"""HBM bytes per solve of the one-GPU box solve under the hybrid schedule, from two rocprofv3
counter runs of `bench.py` (FETCH_SIZE and WRITE_SIZE, each a run of its own, not combined with
tracing), summed over the launches of box_tier_kernel<false> and box_flow_kernel<false, true>.

    python tools/box_solve_traffic.py FETCH_DIR WRITE_DIR SOLVES --tag mirror23_new \\
        [--traffic-json profiles/traffic_subtract8.json]

SOLVES: the solves the traced run made; 0 = half the launches of box_flow_kernel<false, true> (a
head and a tail launch per solve).  A solve counts as 41 box-tiers whatever the schedule, so
bytes per launch = bytes per solve / 41.  FETCH_SIZE is doubled
(tools/pmc_summary.py: gfx950 reports half the bytes of 16-B-per-lane streaming reads).
"""
import argparse
import csv
import glob
import json

NAMES = ("box_tier_kernel<false", "box_flow_kernel<false, true>")


def total(d, name):
    v = []
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if any(n in r["Kernel_Name"] for n in NAMES) and r["Counter_Name"] == name:
                v.append((int(r["Dispatch_Id"]), float(r["Counter_Value"])))
    return len(set(i for i, _ in v)), sum(x for _, x in v) * 1024.0   # KiB -> bytes


def flow_launches(d):
    ids = set()
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if NAMES[1] in r["Kernel_Name"]:
                ids.add(int(r["Dispatch_Id"]))
    return len(ids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("fetch")
    ap.add_argument("write")
    ap.add_argument("solves", type=int)
    ap.add_argument("--tag", required=True)
    ap.add_argument("--traffic-json")
    a = ap.parse_args()
    if not a.solves:
        a.solves = flow_launches(a.fetch) // 2
        assert a.solves and flow_launches(a.write) == 2 * a.solves
    nf, fb = total(a.fetch, "FETCH_SIZE")
    nw, wb = total(a.write, "WRITE_SIZE")
    out = {"kernels": list(NAMES), "solves": a.solves, "dispatches": {"FETCH_SIZE": nf, "WRITE_SIZE": nw},
           "hbm_read_bytes_per_solve": 2 * fb / a.solves, "hbm_write_bytes_per_solve": wb / a.solves,
           "correction": "FETCH_SIZE x2 (gfx950, 16-B/lane streaming reads), KiB -> bytes"}
    out["hbm_bytes_per_solve"] = out["hbm_read_bytes_per_solve"] + out["hbm_write_bytes_per_solve"]
    out["hbm_bytes_per_launch"] = out["hbm_bytes_per_solve"] / 41
    json.dump(out, open("profiles/%s_summary.json" % a.tag, "w"), indent=1)
    if a.traffic_json:
        json.dump({"hbm_bytes_per_launch": out["hbm_bytes_per_launch"], "hbm_bytes_per_solve": out["hbm_bytes_per_solve"],
                   "source": "profiles/%s_summary.json" % a.tag}, open(a.traffic_json, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
