#!/usr/bin/env python3
"""Time gm_reach beside gm_histogram, the solve and the host route.

    python tools/reach_timing.py [--reps N] [--skip-toot] [--out FILE]

Per workload (Othello 4x4, Toot 6x4, each from its root on device 0): the wall time of a
replayed solve, of gm_histogram, and of gm_reach with ALL / ALL and with BEST / ALL -- host
clock around calls that end synchronised, one warm-up call, the median of N -- with the
positions first reached per ply and, on Othello 4x4, the moves followed per level (the
difference of `edges` between searches bounded one ply apart).  On Othello 4x4 also the host
route: a breadth-first search in Python with one Solver.annotate call (gm_moves) and a set per
ply.  A line is printed after every step; --out writes the figures as JSON.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from gamesmanmpi_amd import Context, Solver, _lib, moves  # noqa: E402


def timed(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def workload(name, game, params, reps, per_level, say):
    ctx = Context(game, params, device=0)
    root = ctx.initial()
    n, _ = ctx.solve(root)
    say(name, "n_positions", n)
    say(name, "n_stored", ctx.stats()["n_stored"])
    say(name, "solve", timed(lambda: ctx.solve(root), reps))
    say(name, "histogram", timed(ctx.histogram, reps))
    for tag, m, o in (("all_all", _lib.REACH_ALL, _lib.REACH_ALL), ("best_all", _lib.REACH_BEST, _lib.REACH_ALL)):
        out, pcs, _, _, _ = ctx.reach([root], m, o)
        r = dict(timed(lambda: ctx.reach([root], m, o), reps), out=out, ply_counts=pcs.tolist())
        if per_level:
            edges, prev = [], 0
            for d in range(1, out["plies"]):
                e = ctx.reach([root], m, o, d, plies=False)[0]["edges"]
                edges.append(e - prev)
                prev = e
            r["edges_per_level"] = edges
        say(name, "reach_" + tag, r)
    ctx.close()


def host_route(s, best):
    """The positions below the root, the mover following every move (or its optimal ones) and
    the opponent every move: one annotate call per ply."""
    seen, cur, ply = {(s.codec.key(s.root), 0)}, [s.root], 0
    while cur:
        nxt = []
        for rows, _ in s.annotate(cur):
            if rows and best and ply % 2 == 0:
                r = moves.rank([moves.record_of(v, rem) for _, _, v, rem in rows])
                rows = [row for row, x in zip(rows, r) if x == r.max()]
            for _, p, _, _ in rows:
                k = (s.codec.key(p), (ply + 1) & 1)
                if k not in seen:
                    seen.add(k)
                    nxt.append(p)
        cur, ply = nxt, ply + 1
    return len({k for k, _ in seen})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-toot", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {}

    def say(name, key, value):
        res.setdefault(name, {})[key] = value
        print(name, key, json.dumps(value), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    workload("othello_4x4", _lib.GAME_OTHELLO, (4, 4), a.reps, True, say)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from conftest import load_plugin
    s = Solver(load_plugin("test_games/othello_bit_new.py", length=4, height=4, area=16), device=0)
    s.solve()
    for tag, best in (("all_all", False), ("best_all", True)):
        t = time.perf_counter()
        n = host_route(s, best)
        say("othello_4x4", "host_route_" + tag, {"n": n, "ms": (time.perf_counter() - t) * 1e3})
    s.close()
    if not a.skip_toot:
        workload("toot_6x4", _lib.GAME_TOOT, (6, 4), min(a.reps, 3), False, say)


if __name__ == "__main__":
    main()
