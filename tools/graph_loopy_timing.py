#!/usr/bin/env python3
"""Time the loopy graph solve (GM_OPT_LOOPY, csrc/graph_loopy.hip) beside the default one.

    python tools/graph_loopy_timing.py [--n 2097409] [--reps 5] [--out FILE]

Three graphs of --n nodes from tests/graph_ref.py and tests/loopy_ref.py: a shallow random DAG
(6 levels), a deep one (257 levels) and the shallow one with half its edges rewired to random
nodes and a quarter of its leaves DRAW (cyclic: the loopy mode only).  Per graph and mode one
context solves once to warm up, then --reps times; the median of gm_stats_t.solve_ms is
reported (upload included, in both modes), for the loopy mode also the medians of forward_ms --
the reverse graph: count, scan, fill -- and backward_ms -- the levels -- and the levels run.
On the DAGs the two modes' digests must agree.  The default mode's round kernel is the
baseline: it rescans all n nodes once per level of the graph, the loopy mode pays the
transpose once and then touches each edge once.  A finding, not a gate.
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import graph_ref  # noqa: E402
import loopy_ref  # noqa: E402
from gamesmanmpi_amd import Context, _lib  # noqa: E402


def measure(graph, loopy, reps):
    ctx = Context(_lib.GAME_GRAPH, (), device=0)
    ctx.set_option(_lib.OPT_LOOPY, int(loopy))
    ctx.solve_graph(*graph)   # warm-up: the context's buffers, the kernels' code objects
    runs = []
    for _ in range(reps):
        ctx.solve_graph(*graph)
        runs.append(ctx.stats())
    out = {"solve_ms_median": round(statistics.median(r["solve_ms"] for r in runs), 3),
           "solve_ms_min": round(min(r["solve_ms"] for r in runs), 3),
           "levels": runs[0]["n_tiers"], "digest": "%016x" % ctx.digest()[0]}
    if loopy:
        out["transpose_ms_median"] = round(statistics.median(r["forward_ms"] for r in runs), 3)
        out["levels_ms_median"] = round(statistics.median(r["backward_ms"] for r in runs), 3)
        out["draw"] = ctx.draw_count()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_097_409)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    reps = max(5, a.reps)
    shallow = graph_ref.random_dag(a.n, 6, 3, True, (1, 1, 1), 99)
    graphs = {"shallow_dag": shallow,
              "deep_dag": graph_ref.random_dag(a.n, 257, 3, True, (1, 1, 1), 99),
              "rewired_cyclic": loopy_ref.rewire(shallow, 0.5, 5, True)}
    res = {"n": a.n, "reps": reps}
    for name, g in graphs.items():
        row = {"edges": int(g[1][-1]), "loopy": measure(g, True, reps)}
        if name != "rewired_cyclic":
            row["default"] = measure(g, False, reps)
            assert row["default"]["digest"] == row["loopy"]["digest"], name
            row["loopy_over_default"] = round(row["loopy"]["solve_ms_median"] / row["default"]["solve_ms_median"], 3)
        res[name] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
