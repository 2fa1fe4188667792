#!/usr/bin/env python3
"""Time gm_moves over every position of a solved table, beside the two routes it stands between.

    python tools/moves_timing.py [--reps 5] [--toot 5x4] [--othello 12] [--out profiles/moves_timing.json]

For each workload -- Toot-and-Otto --toot and the Othello 8x8 playout root with --othello empty
squares (tools/othello8_scale.py playout_roots) -- one context solves once and exports its keys.
On that context the median host wall time of --reps calls, each of which synchronises, of
    gm_moves over every exported key, with children     (buffers allocated before the clock starts)
    gm_moves over every exported key, heads only
    gm_query over the children gm_moves returned        the lookups alone: the floor of the pass
and the wall time of the parent route, a Context.moves loop (gm_expand_host + gm_query per key),
over 4,096 evenly spaced keys, scaled per key.  Written down, not gated.
Prints one JSON line and writes it to --out.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from gamesmanmpi_amd import Context, Solver, _lib  # noqa: E402

LOOP_KEYS = 4096


def _median_ms(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 4), round(min(times), 4)


def measure(ctx, reps):
    keys, _ = ctx.export()
    n = len(keys)
    heads, ck, cr = ctx.moves_batch(keys)
    total = len(cr)
    ck = np.ascontiguousarray(ck)
    got = ctypes.c_uint64()

    def with_children():
        _lib.check(ctx.L.gm_moves(ctx.h, keys.ctypes.data, n, heads.ctypes.data, ck.ctypes.data, cr.ctypes.data, total,
                                  ctypes.byref(got)))

    def heads_only():
        _lib.check(ctx.L.gm_moves(ctx.h, keys.ctypes.data, n, heads.ctypes.data, None, None, 0, ctypes.byref(got)))

    with_children()
    heads_only()
    assert got.value == total
    res = {"positions": n, "children": total, "reps": reps}
    res["moves_ms_median"], res["moves_ms_min"] = _median_ms(with_children, reps)
    res["heads_ms_median"], res["heads_ms_min"] = _median_ms(heads_only, reps)
    ctx.query(ck)
    res["query_children_ms_median"], res["query_children_ms_min"] = _median_ms(lambda: ctx.query(ck), reps)
    pick = np.unique(np.linspace(0, n - 1, LOOP_KEYS).astype(np.int64))
    loop_keys = [int(k) for k in keys[pick]] if ctx.words == 1 else [_lib.words_to_int(w) for w in keys[pick]]
    t0 = time.perf_counter()
    for k in loop_keys:
        ctx.moves(k)
    loop_ms = (time.perf_counter() - t0) * 1e3
    sub = np.ascontiguousarray(keys[pick])
    small = lambda: ctx.moves_batch(sub)   # noqa: E731
    small()
    res["loop_keys"] = len(loop_keys)
    res["loop_ms"] = round(loop_ms, 3)
    res["batch_same_keys_ms_median"], _ = _median_ms(small, reps)
    res["loop_us_per_key"] = round(loop_ms / len(loop_keys) * 1e3, 3)
    res["moves_us_per_key"] = round(res["moves_ms_median"] / n * 1e3, 5)
    res["heads_us_per_key"] = round(res["heads_ms_median"] / n * 1e3, 5)
    res["loop_over_moves_per_key"] = round(res["loop_us_per_key"] / res["moves_us_per_key"], 1)
    res["loop_over_batch_same_keys"] = round(loop_ms / res["batch_same_keys_ms_median"], 1)
    res["moves_over_query_children"] = round(res["moves_ms_median"] / res["query_children_ms_median"], 3)
    res["children_per_s"] = round(total / res["moves_ms_median"] * 1e3, 1)
    return res


def _othello8(empties):
    import importlib.util
    import src.utils
    import othello8_scale
    spec = importlib.util.spec_from_file_location("game_module", os.path.join(REPO, "test_games/othello_bit_new.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    src.utils.game_module = mod
    return Solver(mod, othello8_scale.playout_roots()[empties], device=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--toot", default="5x4", help="LxH of the Toot-and-Otto workload, or none")
    ap.add_argument("--othello", default="12", help="empty squares of the Othello 8x8 root, or none")
    ap.add_argument("--out")
    a = ap.parse_args()
    reps = max(3, a.reps)
    res = {}
    if a.toot != "none":
        L, H = (int(x) for x in a.toot.lower().split("x"))
        ctx = Context(_lib.GAME_TOOT, (L, H), device=0)
        ctx.solve(ctx.initial())
        res["toot_%dx%d" % (L, H)] = measure(ctx, reps)
        ctx.close()
    if a.othello != "none":
        s = _othello8(int(a.othello))
        s.solve()
        res["othello_8x8_e%s" % a.othello] = measure(s.ctx, reps)
        s.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
