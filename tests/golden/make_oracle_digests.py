"""Digest fixtures for tables too large to commit.

    python tests/golden/make_oracle_digests.py [board ...]

Runs the C oracle (oracle/gm_oracle.c, itself pinned to the reference plugins'
golden tables by tests/test_oracle_golden.py) and writes, per case, the position
count, the per-tier counts, the root record and the order-independent digest of
the full (key, record) table (the gm_digest formula, include/gmsolve.h) into
tests/golden/oracle_digests.json:

  toot_4x4, toot_5x4, toot_6x4   Toot-and-Otto (config 3 is 6x4: 1,187,212,827
                                 positions) by oracle_solve_layered, the sorted-layer
                                 OpenMP solver (6x4 needs ~25 GB of host memory);
                                 4x4 / 5x4 were first produced by the hash-map
                                 oracle_solve and both solvers agree on them;
  othello_4x4                    config 4 (54,089 positions; also a golden table);
  subtract_8                     the 2^32-position synthetic game (config 5) by
                                 oracle_subtract_dense_mt + oracle_dense_digest.

  othello_8x8_e12, othello_8x8_e14
                                 the reference plugin's default 8x8 board from the 12- and
                                 14-empty roots of the seed-5 playout (1,175,730 and 53.7 M
                                 positions; 14 empties needs ~10 GB) by oracle/othello8.c,
                                 which tests/test_oracle_othello8.py pins to the plugin's
                                 own results (othello_8x8_playouts.npz, the 10-empty table,
                                 othello_8x8_reference.json).  digest is the gm_digest form,
                                 word_digest the layout-independent one of othello8_words.py.
                                 e14 also writes othello_8x8_e14_sample.npz: 4,096 evenly
                                 spaced entries of its table in key order.

Existing entries are kept unless named on the command line.
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from conftest import Oracle  # noqa: E402
import othello8  # noqa: E402  (oracle/, on the path through conftest)
import othello8_words as ow  # noqa: E402

TOOT, SUB = 3, 5
OUT = os.path.join(HERE, "oracle_digests.json")


def layered(o, game, params):
    n, dg, root, tiers = o.solve_layered(game, params)
    return {"positions": n, "per_tier": tiers, "digest": dg, "root_record": root}


def toot(o, L, H):
    n, dg, root, tiers = o.solve_layered(TOOT, (L, H))
    return {"positions": n, "per_ply": tiers, "digest": dg, "root_record": root}


def subtract(o, heaps):
    recs = o.subtract_dense_mt(heaps)
    dg = o.dense_digest(recs)
    root = int(recs[(1 << (4 * heaps)) - 1])
    del recs
    return {"positions": 1 << (4 * heaps), "digest": dg, "root_record": root}


OTHELLO8_ROOTS = {"othello_8x8_e12": "30380028503841784646bfd6afc6be000200",    # tests/test_gpu_othello8.py ROOT12
                  "othello_8x8_e14": "30300c2c503841784646b1d2afc6be000200"}    # tools/othello8_roots.py endgame_14
OTHELLO8_SAMPLE = 4096


def othello8_case(name):
    root_hex = OTHELLO8_ROOTS[name]
    sample = name == "othello_8x8_e14"
    t = time.time()
    r = othello8.Othello8Oracle().solve(ow.words_of(bytes.fromhex(root_hex).decode("latin-1")),
                                        want=OTHELLO8_SAMPLE if sample else 0)
    out = {"root_hex": root_hex, "positions": r["positions"], "per_tier": r["per_tier"],
           "root_record": r["root_record"], "digest": r["digest"], "word_digest": r["word_digest"],
           "seconds": round(time.time() - t, 1)}
    if sample:
        assert len(r["words"]) == OTHELLO8_SAMPLE
        np.savez_compressed(os.path.join(HERE, name + "_sample.npz"), words=r["words"], records=r["records"],
                            meta=json.dumps({"root_hex": root_hex, "positions": r["positions"],
                                             "entries": "floor(i * positions / 4096) of the table in key order"}))
    return out


CASES = {
    "othello_8x8_e12": lambda o: othello8_case("othello_8x8_e12"),
    "othello_8x8_e14": lambda o: othello8_case("othello_8x8_e14"),
    "othello_4x4": lambda o: layered(o, 4, (4, 4)),
    "toot_4x4": lambda o: toot(o, 4, 4),
    "toot_5x4": lambda o: toot(o, 5, 4),
    "toot_6x4": lambda o: toot(o, 6, 4),
    "subtract_8": lambda o: subtract(o, 8),
}


def main():
    names = sys.argv[1:] or list(CASES)
    out = json.load(open(OUT)) if os.path.exists(OUT) else {}
    o = Oracle()
    for name in names:
        t = time.time()
        out[name] = CASES[name](o)
        print("%s: %d positions, root %#x, %.1f s" % (name, out[name]["positions"], out[name]["root_record"],
                                                     time.time() - t), flush=True)
        with open(OUT, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
