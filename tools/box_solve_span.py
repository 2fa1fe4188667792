#!/usr/bin/env python3
"""What stands in front of and behind the box kernels of each one-GPU solve, from a rocprofv3
kernel trace of `bench.py --gpus 1` (hybrid schedule: a head and a tail box_flow_kernel per solve).

    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d <trace dir> -- python bench.py ...
    python tools/box_solve_span.py <trace dir> [--last N]

Per solve: the nodes before the head launch (a fill kernel for the memset node, box_epoch_kernel)
and after the tail launch (the runtime's copy kernels for device-to-host copies into pinned memory
-- they show in the kernel trace, not in the copy trace -- or box_result_kernel), the time from the
first of them to the head launch's start (front), from the tail launch's end to the last one's end
(back), the box kernels' own span, and all of it (total).  Medians over the last N solves.
"""
import argparse
import csv
import glob

import numpy as np

FRONT = ("box_epoch_kernel", "fillBuffer")
BACK = ("copyBuffer", "box_result_kernel")


def short(name):
    for s in ("box_tier_kernel", "box_tier4_kernel", "box_flow_kernel") + FRONT + BACK:
        if s in name:
            return s
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--last", type=int, default=8, help="use only the last N solves")
    ap.add_argument("--near", type=float, default=100.0, help="us: a node further from the solve is not its own")
    a = ap.parse_args()
    r = []
    for f in glob.glob(a.trace + "/**/*kernel_trace.csv", recursive=True):
        r += [(int(x["Start_Timestamp"]), int(x["End_Timestamp"]), short(x["Kernel_Name"])) for x in csv.DictReader(open(f))]
    r.sort()
    flow = [i for i, x in enumerate(r) if x[2] == "box_flow_kernel"]
    rows = []
    for h, t in list(zip(flow[0::2], flow[1::2]))[-a.last:]:
        i, j = h, t
        while i > 0 and r[i - 1][2] in FRONT and r[h][0] - r[i - 1][0] < a.near * 1e3:
            i -= 1
        while j + 1 < len(r) and r[j + 1][2] in BACK and r[j + 1][0] - r[t][1] < a.near * 1e3:
            j += 1
        rows.append({"nodes": [x[2] for x in r[i:h]] + ["<box kernels>"] + [x[2] for x in r[t + 1:j + 1]],
                     "front": (r[h][0] - r[i][0]) / 1e3, "box kernels": (r[t][1] - r[h][0]) / 1e3,
                     "back": (r[j][1] - r[t][1]) / 1e3, "total": (r[j][1] - r[i][0]) / 1e3,
                     "front nodes' own time": sum(x[1] - x[0] for x in r[i:h]) / 1e3,
                     "back nodes' own time": sum(x[1] - x[0] for x in r[t + 1:j + 1]) / 1e3})
    if not rows:
        raise SystemExit("no solve with a head and a tail launch in the trace")
    print("%d solves; nodes of the last: %s" % (len(rows), ", ".join(rows[-1]["nodes"])))
    for key in ("front", "box kernels", "back", "total", "front nodes' own time", "back nodes' own time"):
        v = np.array([x[key] for x in rows])
        print("  %-22s median %8.2f us   min %8.2f   max %8.2f" % (key, np.median(v), v.min(), v.max()))


if __name__ == "__main__":
    main()
