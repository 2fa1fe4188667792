#!/usr/bin/env python3
"""Time gm_import beside the solve that produced the table.

    python tools/import_timing.py [--reps 5] [--tables toot_4x4,othello_8x8_e12[,toot_5x4]]
                                  [--limit-s 420] [--out profiles/import_timing.json]

For each table a child process solves the game, exports the table (gm_export: the host sort
included), opens a fresh context and imports the table --reps times after one warm-up: the
median wall time of the import (gm_stats_t.solve_ms after gm_import) is set beside the solve's
solve_ms.  A second child does the same under GM_TRACE=1, where the library times the import's
phases with events (upload, scan, insert, score, census; each phase synchronises there, so
their sum is above the untraced wall time); the medians of those are recorded too.  A child
that is not done after --limit-s seconds is stopped and the table recorded as not finished.
Loading is not meant to beat solving: the figures say what a stored table costs to bring back
(DESIGN.md §4.8).  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# the seed-5 playout of tests/plugins/othello8_endgame.py, stopped with E squares empty
OTHELLO8_ROOTS = {10: "303800204018057a4646bfdebfe6fa800200", 12: "30380028503841784646bfd6afc6be000200",
                  14: "30300c2c503841784646b1d2afc6be000200"}
PHASES = ("upload", "scan", "insert", "score", "census")
TRACE_LINE = re.compile(r"\[gm\] import of (\d+) keys: " + " ".join(p + r" ([0-9.]+)" for p in PHASES) + " ms")


def _solver(table):
    from gamesmanmpi_amd import Context, Solver, _lib
    if table.startswith("toot_"):
        L, H = (int(x) for x in table[5:].split("x"))
        ctx = Context(_lib.GAME_TOOT, (L, H), device=0)
        return ctx, ctx.initial(), (_lib.GAME_TOOT, (L, H))
    empties = int(table.rsplit("_e", 1)[1])
    import importlib.util
    import src.utils
    spec = importlib.util.spec_from_file_location("game_module", os.path.join(REPO, "test_games/othello_bit_new.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    src.utils.game_module = mod
    s = Solver(mod, bytes.fromhex(OTHELLO8_ROOTS[empties]).decode("latin-1"), device=0)
    return s.ctx, s.root_key, (s.codec.game_id, s.codec.params)


def child(table, reps):
    from gamesmanmpi_amd import Context
    ctx, root, (game, params) = _solver(table)
    n, rec = ctx.solve(root)
    st = ctx.stats()
    t0 = time.perf_counter()
    keys, recs = ctx.export()
    export_s = time.perf_counter() - t0
    want = ctx.digest()
    ctx.close()
    b = Context(game, params, device=0)
    times = []
    for i in range(reps + 1):
        assert b.import_table(keys, recs, root) == (n, rec)
        if i:
            times.append(b.stats()["solve_ms"])
    assert b.digest() == want
    out = {"positions": n, "stored": st["n_stored"], "key_words": b.words, "input_bytes": int(keys.nbytes + recs.nbytes),
           "solve_ms": round(st["solve_ms"], 3), "export_s": round(export_s, 3),
           "import_ms_median": round(statistics.median(times), 3), "import_ms_min": round(min(times), 3)}
    b.close()
    print(json.dumps(out))
    return 0


def run_child(table, reps, limit_s, trace):
    env = dict(os.environ)
    env.pop("GM_TRACE", None)
    if trace:
        env["GM_TRACE"] = "1"
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", table, "--reps", str(reps)],
                           capture_output=True, text=True, timeout=limit_s, env=env, cwd=REPO)
    except subprocess.TimeoutExpired:
        return None, "not finished within %d s" % limit_s
    if r.returncode:
        return None, "exit status %d: %s" % (r.returncode, r.stderr[-400:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    if trace:
        rows = [[float(x) for x in m.groups()[1:]] for m in TRACE_LINE.finditer(r.stderr)][1:]   # warm-up dropped
        res = {p + "_ms": round(statistics.median(row[i] for row in rows), 3) for i, p in enumerate(PHASES)} if rows else {}
    return res, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tables", default="toot_4x4,othello_8x8_e12")
    ap.add_argument("--limit-s", type=int, default=420)
    ap.add_argument("--out")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    res = {"reps": a.reps, "limit_s": a.limit_s}
    for table in a.tables.split(","):
        t0 = time.perf_counter()
        wall, err = run_child(table, a.reps, a.limit_s, trace=False)
        if err:
            res[table] = {"finished": False, "why": err}
            continue
        left = max(30, a.limit_s - int(time.perf_counter() - t0))
        phases, err = run_child(table, a.reps, left, trace=True)
        res[table] = dict(wall, finished=True, phases_traced=phases if not err else {"why": err})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
