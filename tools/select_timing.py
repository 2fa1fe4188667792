#!/usr/bin/env python3
"""Time gm_select against gm_digest and gm_histogram on the same solved table.

    python tools/select_timing.py [--reps 15] [--out profiles/select_timing.json] [--design DESIGN.md]

Solves the 2^32-position 8-heap game once, warms every call up, then takes the median host wall
time of `--reps` calls each, all of which synchronise, of
    ctx.digest()                                   the yardstick: the same 2^32 bytes, more arithmetic per byte
    ctx.histogram()                                for information
    ctx.select(LOSS, 78, 80)                       a narrow filter: 2,048 matches
    ctx.select(WIN | LOSS, cap = 65536)            every position matches; the list fills and the pass only counts
Neither selection's median should exceed the digest's.  Prints one JSON line,
writes it to --out, and with --design rewrites the table between the select_timing markers
of that file.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from gamesmanmpi_amd import Context, _lib  # noqa: E402

BEGIN, END = "<!-- select_timing:begin -->", "<!-- select_timing:end -->"


def _median_ms(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 4), round(min(times), 4)


def table(res):
    rows = [("gm_digest", "digest", "the yardstick"),
            ("gm_histogram", "histogram", "for information"),
            ("gm_select LOSS 78-80, cap 4096", "narrow", "%d matches" % res["narrow_matches"]),
            ("gm_select WIN\\|LOSS, cap 65536", "all", "%d matches, 65,536 written" % res["all_matches"])]
    out = ["| call | median ms | min ms | GB/s | |", "|---|---|---|---|---|"]
    for name, key, note in rows:
        med = res[key + "_ms_median"]
        out.append("| %s | %.2f | %.2f | %.0f | %s |" % (name, med, res[key + "_ms_min"], (1 << 32) / med / 1e6, note))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out")
    ap.add_argument("--design", help="a file whose table between the select_timing markers is rewritten")
    a = ap.parse_args()
    reps = max(10, a.reps)
    ctx = Context(_lib.GAME_SUBTRACT, (8,), device=0)
    n, _ = ctx.solve(ctx.initial())
    win_loss = _lib.SEL_WIN | _lib.SEL_LOSS
    calls = {
        "digest": ctx.digest,
        "histogram": ctx.histogram,
        "narrow": lambda: ctx.select(_lib.SEL_LOSS, 78, 80, 4096, as_array=True),
        "all": lambda: ctx.select(win_loss, 0, _lib.SEL_ANY_REM, 65536, as_array=True),
    }
    for _ in range(3):
        got = {name: call() for name, call in calls.items()}
    assert got["digest"][1] == n == int(got["histogram"].sum()) == got["all"][0] and len(got["all"][1]) == 65536
    assert got["narrow"][0] == 2048 == len(got["narrow"][1])
    res = {"positions": n, "bytes_read": 1 << 32, "reps": reps, "narrow_matches": got["narrow"][0],
           "all_matches": got["all"][0]}
    for name, call in calls.items():
        res[name + "_ms_median"], res[name + "_ms_min"] = _median_ms(call, reps)
    ctx.close()
    res["narrow_not_slower_than_digest"] = res["narrow_ms_median"] <= res["digest_ms_median"]
    res["all_not_slower_than_digest"] = res["all_ms_median"] <= res["digest_ms_median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.design:
        text = open(a.design).read()
        head, rest = text.split(BEGIN, 1)
        _, tail = rest.split(END, 1)
        with open(a.design, "w") as f:
            f.write(head + BEGIN + "\n" + "\n".join(table(res)) + "\n" + END + tail)
    return 0


if __name__ == "__main__":
    sys.exit(main())
