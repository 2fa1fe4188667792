#!/usr/bin/env python3
"""Time gm_verify beside the solve it checks.

    python tools/verify_timing.py [--reps 7] [--toot 5x4] [--othello 14] [--launcher 16] [--out FILE]

For each workload -- the 2^32-position 8-heap subtraction game, Toot-and-Otto --toot, and the
Othello 8x8 endgame root with --othello empty squares (tools/othello8_roots.py) -- one context
solves once, warms ctx.verify() and ctx.digest() up, and the median host wall time of --reps
calls of each is set beside the same context's solve_ms and backward_ms (gm_stats_t).  The
yardstick is the workload's own backward pass: verification makes the same child lookups,
without the sorted interior lists and without the shortcut for a LOSS-in-0 child, so the ratio
verify / backward is reported -- a finding, not a gate.

--launcher E runs ``solver_launcher.py test_games/othello_bit_new.py --custom
tools/othello8_roots.py --init_pos endgame_E --verify`` once in this process and records its
output, exit status and wall time (none: skip).  Prints one JSON line and writes it to --out.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from gamesmanmpi_amd import Context, Solver, _lib  # noqa: E402


def _median_ms(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 4), round(min(times), 4)


def measure(ctx, n, reps, warmup=2):
    st = ctx.stats()
    for _ in range(warmup):
        res, keys = ctx.verify(cap=0)
        ctx.digest()
    assert res["n_bad"] == 0 and res["root_ok"] == 1 and res["checked"] == (st["n_stored"] or n), res
    v_med, v_min = _median_ms(lambda: ctx.verify(cap=0), reps)
    d_med, d_min = _median_ms(ctx.digest, reps)
    back = st["backward_ms"]
    return {"positions": n, "checked": res["checked"], "child_lookups": res["child_lookups"], "consistent": True,
            "solve_ms": round(st["solve_ms"], 4), "backward_ms": round(back, 4),
            "verify_ms_median": v_med, "verify_ms_min": v_min, "digest_ms_median": d_med, "digest_ms_min": d_min,
            "verify_over_backward": round(v_med / back, 3) if back else None,
            "lookups_per_s": round(res["child_lookups"] / v_med * 1e3, 1)}


def _othello8(empties):
    import importlib.util
    import src.utils
    spec = importlib.util.spec_from_file_location("game_module", os.path.join(REPO, "test_games/othello_bit_new.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    src.utils.game_module = mod
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import othello8_roots
    return Solver(mod, getattr(othello8_roots, "endgame_%d" % empties)(), device=0)


def launcher_verify(empties):
    import solver_launcher
    args = solver_launcher.build_parser().parse_args(
        [os.path.join(REPO, "test_games/othello_bit_new.py"), "--custom", os.path.join(REPO, "tools/othello8_roots.py"),
         "--init_pos", "endgame_%d" % empties, "--verify"])
    out = io.StringIO()
    t0 = time.perf_counter()
    status = solver_launcher.run(args, out=out)
    return {"exit_status": status, "wall_s": round(time.perf_counter() - t0, 3), "output": out.getvalue().splitlines()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--toot", default="5x4", help="LxH of the Toot-and-Otto workload, or none")
    ap.add_argument("--othello", default="14", help="empty squares of the Othello 8x8 root, or none")
    ap.add_argument("--launcher", default="16", help="empty squares of the root run through --verify, or none")
    ap.add_argument("--out")
    a = ap.parse_args()
    reps = max(3, a.reps)
    res = {"reps": reps}
    ctx = Context(_lib.GAME_SUBTRACT, (8,), device=0)
    n, _ = ctx.solve(ctx.initial())
    res["subtract_8"] = measure(ctx, n, reps)
    ctx.close()
    if a.toot != "none":
        L, H = (int(x) for x in a.toot.lower().split("x"))
        ctx = Context(_lib.GAME_TOOT, (L, H), device=0)
        n, _ = ctx.solve(ctx.initial())
        res["toot_%dx%d" % (L, H)] = measure(ctx, n, reps)
        ctx.close()
    if a.othello != "none":
        s = _othello8(int(a.othello))
        n, _ = s.solve()
        res["othello_8x8_e%s" % a.othello] = measure(s.ctx, n, reps)
        s.close()
    if a.launcher != "none":
        res["launcher_othello_8x8_e%s" % a.launcher] = launcher_verify(int(a.launcher))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
