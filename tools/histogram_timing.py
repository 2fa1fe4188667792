#!/usr/bin/env python3
"""Time gm_histogram against gm_digest on the same solved table.

    python tools/histogram_timing.py [--reps 15] [--toot 5x4] [--out FILE]

Solves the 2^32-position 8-heap game once, warms both calls up, then takes the median host
wall time of `--reps` ctx.digest() calls and `--reps` ctx.histogram() calls on that context.
Both calls synchronise and copy a few bytes back, so they carry the same overhead; the digest
reads the same 2^32 bytes and does more arithmetic per byte, which makes it the yardstick:
the histogram's median should not exceed the digest's.  Prints one JSON line
(both medians, bytes read, GB/s; for information the same pair for Toot-and-Otto --toot,
skipped with --toot none) and writes it to --out when given.
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

DEVICE_COPY_TBS = 4.88   # device-copy bandwidth measured on the same part


def _median_ms(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times)


def measure(game, params, reps, warmup=3):
    ctx = Context(game, params, device=0)
    n, _ = ctx.solve(ctx.initial())
    for _ in range(warmup):
        ctx.digest()
        hist = ctx.histogram()
    assert int(hist.sum()) == n == ctx.digest()[1]
    d_med, d_min = _median_ms(ctx.digest, reps)
    h_med, h_min = _median_ms(ctx.histogram, reps)
    ctx.close()
    return {"positions": n, "n_rem": int(hist.shape[1]), "digest_ms_median": round(d_med, 4),
            "digest_ms_min": round(d_min, 4), "histogram_ms_median": round(h_med, 4),
            "histogram_ms_min": round(h_min, 4), "histogram_not_slower": h_med <= d_med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--toot", default="5x4", help="LxH of the Toot-and-Otto pair, or none")
    ap.add_argument("--out")
    a = ap.parse_args()
    reps = max(10, a.reps)
    res = measure(_lib.GAME_SUBTRACT, (8,), reps)
    res["bytes_read"] = 1 << 32
    res["histogram_gbs"] = round((1 << 32) / res["histogram_ms_median"] / 1e6, 1)
    res["digest_gbs"] = round((1 << 32) / res["digest_ms_median"] / 1e6, 1)
    res["device_copy_gbs"] = DEVICE_COPY_TBS * 1e3
    res["reps"] = reps
    if a.toot != "none":
        L, H = (int(x) for x in a.toot.lower().split("x"))
        res["toot_%dx%d" % (L, H)] = measure(_lib.GAME_TOOT, (L, H), reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
