#!/usr/bin/env python3
"""Generate the Connect fixtures in ``tests/golden/`` from ``test_games/connect4.py``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_connect_golden.py [--skip-big]

Runs on the CPU only: the plugin is strong-solved by the canonical fixed point of
``oracle/canonical.py``.  A position of this plugin is its u64 key, so no
codec is involved.  It writes

* ``connect_<L>x<H>_<K>.npz`` for the small boards: the sorted ``(keys u64, records u16)``
  table (record = value << 14 | remoteness).  The 4x4 table stores ``key_deltas`` (the first
  key, then the differences of the sorted keys) in place of ``keys`` to stay small;
  ``load_table`` undoes that;
* ``connect.json``: per solve the board, the root key, whether the root is its own mirror
  image, the position count, the primitive count, the root record, the per-tier counts (index
  = discs - the root's discs), the value x remoteness histogram (rows WIN, LOSS, TIE) and the
  ``gm_digest`` sum -- for the tables above, for 4x5 and 5x4 from the empty board, and for
  custom roots on 7x6 and 9x6 (the 63-bit boundary).

A custom root is a position of a seeded random game, found by walking the game back from its
end until the subgame below holds at least 1,000 positions (at most 300,000, else the next
seed); ``sym`` roots come from games played in mirrored pairs of moves, so that the root is its
own mirror image.  The helpers below (``load_table``, ``discs``, ``mirror``, ``histogram``) are
what the tests read the fixtures with.
"""
import argparse
import importlib.util
import json
import os
import random
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
JSON = os.path.join(HERE, "connect.json")
sys.dont_write_bytecode = True

TABLES = [(3, 3, 3), (4, 3, 3), (2, 5, 4), (5, 2, 4), (4, 4, 4)]   # full tables (.npz)
SUMMARIES = [(4, 5, 4), (5, 4, 4)]                                  # from the empty board, summary only
# name -> (L, H, K, first seed tried, played in mirrored pairs)
CUSTOM = {"c7x6_a": (7, 6, 4, 1, False), "c7x6_b": (7, 6, 4, 2, False), "c7x6_sym": (7, 6, 4, 3, True),
          "c9x6_a": (9, 6, 4, 4, False)}
SUB_MIN, SUB_MAX = 1000, 300000
MAX_FILE = 525568   # the largest fixture committed before these (toot_4x3.npz)


def name_of(L, H, K):
    return "connect_%dx%d_%d" % (L, H, K)


# ---------------------------------------------------------------- what the tests share
def load_table(name):
    """(keys, records) of a connect_*.npz fixture, keys ascending."""
    d = np.load(os.path.join(HERE, name + ".npz"))
    keys = d["keys"] if "keys" in d.files else np.cumsum(d["key_deltas"], dtype=np.uint64)
    return keys.astype(np.uint64), d["records"]


def load_json():
    with open(JSON) as f:
        return json.load(f)


def discs(keys, L, H):
    """Disc count (the descriptor's tier) of every key of an array."""
    keys = np.asarray(keys, dtype=np.uint64)
    w = H + 1
    n = np.zeros(len(keys), dtype=np.int64)
    for x in range(L):
        f = (keys >> np.uint64(x * w)) & np.uint64((1 << w) - 1)
        for j in range(1, w):
            n += (f >> np.uint64(j)) != 0
    return n


def mirror(key, L, H):
    """The position with the order of its column fields reversed."""
    w = H + 1
    return sum(((key >> (x * w)) & ((1 << w) - 1)) << ((L - 1 - x) * w) for x in range(L))


def histogram(records):
    """(3, n_rem) counts by value (rows WIN, LOSS, TIE) and remoteness."""
    records = np.asarray(records, dtype=np.uint16)
    v, r = (records >> 14).astype(np.int64), (records & 0x3FFF).astype(np.int64)
    n_rem = int(r.max()) + 1
    return np.bincount(v * n_rem + r, minlength=3 * n_rem).reshape(3, n_rem)


def digest(keys, recs):
    """gm_digest (include/gmsolve.h): the sum of mix64(key * phi + record)."""
    k = np.asarray(keys, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = k * np.uint64(0x9E3779B97F4A7C15) + np.asarray(recs).astype(np.uint64)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
        return int(x.sum(dtype=np.uint64))


def summary(keys, recs, root, L, H, K):
    keys = np.asarray(keys, dtype=np.uint64)
    t = discs(keys, L, H)
    t0 = int(discs([root], L, H)[0])
    i = int(np.searchsorted(keys, np.uint64(root)))
    assert int(keys[i]) == root
    return {"dims": [L, H, K], "root": int(root), "root_symmetric": mirror(root, L, H) == root,
            "positions": int(len(keys)), "primitive": int(((recs & 0x3FFF) == 0).sum()),
            "root_record": int(recs[i]), "root_discs": t0,
            "per_tier": [int(c) for c in np.bincount(t - t0)],
            "histogram": [[int(c) for c in row] for row in histogram(recs)],
            "digest": digest(keys, recs)}


# ---------------------------------------------------------------- the generator
def load_plugin(L, H, K):
    sys.path.insert(0, REPO)
    import src.utils
    spec = importlib.util.spec_from_file_location("game_module", os.path.join(REPO, "test_games/connect4.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.length, mod.height, mod.connect = L, H, K
    src.utils.game_module = mod
    return mod


def solve(mod, root):
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import canonical
    table, _ = canonical.solve(mod, root)
    keys = np.fromiter(table.keys(), dtype=np.uint64, count=len(table))
    recs = np.fromiter(((v << 14) | r for v, r in table.values()), dtype=np.uint16, count=len(table))
    order = np.argsort(keys, kind="stable")
    return keys[order], recs[order]


def count_below(mod, root, limit):
    """Positions reachable from root, or limit + 1 once there are more."""
    seen = {root}
    frontier = [root]
    while frontier:
        nxt = []
        for p in frontier:
            if mod.primitive(p) != 4:
                continue
            for m in mod.gen_moves(p):
                c = mod.do_move(p, m)
                if c not in seen:
                    seen.add(c)
                    nxt.append(c)
            if len(seen) > limit:
                return limit + 1
        frontier = nxt
    return len(seen)


def playout(mod, seed, paired):
    """The positions of one seeded random game; paired: only those after each mirrored group of
    four moves (x, y, L-1-x, L-1-y) that left the position its own mirror image."""
    rng = random.Random(seed)
    L, H = mod.length, mod.height
    p = mod.initial_position()
    line = [p]
    while mod.primitive(p) == 4:
        ms = mod.gen_moves(p)
        if not paired:
            p = mod.do_move(p, ms[rng.randrange(len(ms))])
            line.append(p)
            continue
        x, y = ms[rng.randrange(len(ms))], ms[rng.randrange(len(ms))]
        q = p
        for m in (x, y, L - 1 - x, L - 1 - y):
            if mod.primitive(q) != 4 or m not in mod.gen_moves(q):
                q = None
                break
            q = mod.do_move(q, m)
        if q is None or mirror(q, L, H) != q:
            if rng.random() < 0.02:   # a board where no group fits any more
                break
            continue
        p = q
        line.append(p)
    return line


def custom_root(L, H, K, seed, paired):
    mod = load_plugin(L, H, K)
    while True:
        for p in reversed(playout(mod, seed, paired)):
            if mod.primitive(p) != 4:
                continue
            n = count_below(mod, p, SUB_MAX)
            if n >= SUB_MIN:
                break
        else:
            n = 0
        if SUB_MIN <= n <= SUB_MAX:
            return mod, p, seed
        seed += 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-big", action="store_true", help="leave the 4x5 and 5x4 summaries as they are")
    args = ap.parse_args()
    out = load_json() if os.path.exists(JSON) else {}

    def put(name, entry, t0):
        entry["seconds"] = round(time.time() - t0, 1)
        out[name] = entry
        print(name, json.dumps({k: v for k, v in entry.items() if k not in ("histogram", "per_tier")}), flush=True)
        with open(JSON, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")

    for L, H, K in TABLES:
        t0 = time.time()
        mod = load_plugin(L, H, K)
        root = mod.initial_position()
        keys, recs = solve(mod, root)
        path = os.path.join(HERE, name_of(L, H, K) + ".npz")
        meta = json.dumps({"game": "connect4", "dims": [L, H, K], "root": root})
        if len(keys) > 50000:
            np.savez_compressed(path, key_deltas=np.diff(keys, prepend=np.uint64(0)), records=recs, meta=meta)
        else:
            np.savez_compressed(path, keys=keys, records=recs, meta=meta)
        k2, r2 = load_table(name_of(L, H, K))
        assert np.array_equal(k2, keys) and np.array_equal(r2, recs)
        assert os.path.getsize(path) < MAX_FILE, os.path.getsize(path)
        put(name_of(L, H, K), summary(keys, recs, root, L, H, K), t0)

    for name, (L, H, K, seed, paired) in CUSTOM.items():
        t0 = time.time()
        mod, root, used = custom_root(L, H, K, seed, paired)
        keys, recs = solve(mod, root)
        e = summary(keys, recs, root, L, H, K)
        e["playout_seed"], e["mirrored_pairs"] = used, paired
        assert e["root_symmetric"] == paired, name
        put(name, e, t0)
    assert any(not out[n]["root_symmetric"] for n in CUSTOM if n.startswith("c7x6"))

    if not args.skip_big:
        for L, H, K in SUMMARIES:
            t0 = time.time()
            mod = load_plugin(L, H, K)
            root = mod.initial_position()
            keys, recs = solve(mod, root)
            put(name_of(L, H, K), summary(keys, recs, root, L, H, K), t0)


if __name__ == "__main__":
    main()
