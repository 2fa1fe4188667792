#!/usr/bin/env python3
"""How large a Connect board one GPU holds: solve test_games/connect4.py's game
from the empty board on growing boards, each board in a process of its own under its own time
limit, and stop at the first board that does not fit (GM_E_NOMEM), fails or runs out of time.
Toot-and-Otto 6x4 is solved first, the same way, as the rate to compare with.

    python tools/connect_scale.py [--boards 5x4 6x4 5x5 5x6 7x4 6x5] [--connect 4] [--limit 300]
                                  [--repeats 2] [--out FILE]

One JSON line per board on stdout (and all of them as a list in FILE): positions, stored
positions (one per mirror pair), root record, wall seconds per solve, the engine's own solve /
forward / backward milliseconds, table bytes, positions per second of the fastest solve, digest.
`--one LxH` is the child's entry: one board, one line.

The default list ends at 6x5 (2.8 G positions).  The next boards up, 6x6 (69 G) and 7x5 (113 G),
have single tiers of more than 2^31 positions.  Such a tier is no longer sorted with a truncated
count (sparse.hip sort_max: it skips the batch sort), but nothing else about tiers of that size
has been tried (32-bit slot indices, table sizes), so they stay off the default list."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BOARDS = ["5x4", "6x4", "5x5", "5x6", "7x4", "6x5"]


def one(game, dims, repeats):
    from gamesmanmpi_amd import Context, GMError, _lib
    out = {"game": game, "dims": list(dims)}
    ctx = Context(_lib.GAME_TOOT if game == "toot" else _lib.GAME_CONNECT, dims, device=0)
    try:
        wall, ms = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            n, rec = ctx.solve(ctx.initial())
            wall.append(round(time.perf_counter() - t0, 4))
            ms.append(round(ctx.stats()["solve_ms"], 3))
        st = ctx.stats()
        d, m = ctx.digest()
        out.update({"positions": n, "stored": st["n_stored"], "root_record": rec, "wall_s": wall, "solve_ms": ms,
                    "forward_ms": round(st["forward_ms"], 3), "backward_ms": round(st["backward_ms"], 3),
                    "table_bytes": st["table_bytes"], "edges": st["n_edges"], "tiers": st["n_tiers"],
                    "positions_per_s": n / (min(ms) / 1e3), "digest": "%#018x" % d, "digest_positions": m})
    except GMError as e:
        out["error"] = _lib.ERRORS.get(e.code, str(e.code))
        out["message"] = str(e)
    finally:
        ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", nargs="+", default=BOARDS, metavar="LxH")
    ap.add_argument("--connect", type=int, default=4)
    ap.add_argument("--limit", type=float, default=300, help="seconds per board")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--no-toot", action="store_true", help="leave out the Toot-and-Otto 6x4 solve")
    ap.add_argument("--out", help="also write the lines as a JSON list to this file")
    ap.add_argument("--one", metavar="LxH", help=argparse.SUPPRESS)
    ap.add_argument("--game", default="connect", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        L, H = (int(v) for v in a.one.lower().split("x"))
        return one(a.game, (L, H) if a.game == "toot" else (L, H, a.connect), a.repeats)
    jobs = ([] if a.no_toot else [("toot", "6x4")]) + [("connect", b) for b in a.boards]
    rows = []
    for game, board in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", board, "--game", game, "--connect", str(a.connect),
               "--repeats", str(a.repeats)]
        t0 = time.time()
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            row = json.loads(lines[-1]) if lines else {"game": game, "board": board, "error": "exit %d" % r.returncode,
                                                        "message": r.stderr[-400:]}
        except subprocess.TimeoutExpired:
            row = {"game": game, "board": board, "error": "time limit of %g s" % a.limit}
        row["process_s"] = round(time.time() - t0, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
                f.write("\n")
        if "error" in row:   # the first board that does not fit ends the run: nothing more is started
            break


if __name__ == "__main__":
    main()
