#!/usr/bin/env python3
"""Draw the mid-game Connect roots of tests/connect_roots.py (DRAWN) and print them as literals.

    PYTHONDONTWRITEBYTECODE=1 python tools/draw_connect_roots.py

Runs on the CPU only, over the C oracle (oracle/gm_oracle.c) and the cell helpers of
tests/connect_roots.py.  No test calls it: the literals are the record, and
tests/test_connect_roots.py checks the conditions they were drawn to meet.

A root is a position of a seeded game, found by walking the game back from its end until the
oracle's subtree holds at least 1,000 positions; with more than 100,000 the next seed (+ 100) is
tried.  The games:

* "random": every move drawn uniformly;
* "paired": groups of four moves x, y, L-1-x, L-1-y that leave the position its own mirror
  image (as tests/golden/make_connect_golden.py plays them); only the positions between groups
  count;
* a direction: a K-line of that direction ending in the top row is chosen (its place by the
  seed), one player takes its cells whenever one can be played, the other never does, and the
  line's highest cell is kept for last until few cells are empty, so that the subtree below a
  position shortly before the end is small and holds the finished line;
* "built": 16 columns, K = 2, one alternating row of 10 discs: every move into those columns ends
  the game at once, so the root keeps all 16 columns open over a subtree of a few thousand.

It also prints EDGE, positions put together cell by cell that hold a column of 8, 16, 30 and 31
second-player stones (edge_positions()).
"""
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

import connect_roots as R  # noqa: E402
from conftest import Oracle  # noqa: E402

# board -> the games to draw from: (kind, first seed)
PLAN = [
    ((7, 8, 4), [("random", 1), ("random", 2), ("paired", 3)]),
    ((3, 20, 4), [("random", 1), ("random", 2), ("paired", 3)]),
    ((2, 30, 4), [("random", 1), ("random", 2), ("paired", 3)]),
    ((16, 2, 4), [("random", 1), ("horizontal", 2), ("paired", 3)]),
    ((16, 2, 8), [("random", 1), ("horizontal", 2)]),
    ((15, 3, 4), [("random", 1), ("paired", 3)]),
    ((12, 4, 5), [("random", 1), ("horizontal", 2), ("paired", 3)]),
    ((8, 6, 6), [("vertical", 1), ("horizontal", 2), ("diagonal", 3), ("antidiagonal", 4)]),
    ((7, 7, 7), [("vertical", 1), ("horizontal", 2), ("diagonal", 3), ("antidiagonal", 4)]),
    ((9, 6, 8), [("random", 1), ("horizontal", 2)]),
]
KEEP_LAST_UNTIL = 7     # a steered game takes its line's last cell once this few cells are empty
o = Oracle()


def expand(dims, key):
    """(primitive, children in column order) straight from the oracle."""
    import ctypes
    p, n = o._params(dims)
    kids = (ctypes.c_uint64 * 64)()
    nk, pr, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    assert o.L.oracle_expand(R.CONNECT, p, n, key, kids, ctypes.byref(nk), ctypes.byref(pr), ctypes.byref(t)) == 0
    return pr.value, list(kids[:nk.value])


def count_below(dims, root, limit):
    seen = {root}
    frontier = [root]
    while frontier:
        nxt = []
        for p in frontier:
            for c in expand(dims, p)[1]:
                if c not in seen:
                    seen.add(c)
                    nxt.append(c)
            if len(seen) > limit:
                return limit + 1
        frontier = nxt
    return len(seen)


def open_columns(dims, key):
    """[(column, row its next disc lands in)], ascending: the order of the oracle's children."""
    L, H, _ = dims
    _, heights = R.cells_of([key], L, H)
    return [(x, int(heights[0, x])) for x in range(L) if heights[0, x] < H]


def play_random(dims, rng):
    p = o.initial(R.CONNECT, dims)
    line = [p]
    while True:
        prim, kids = expand(dims, p)
        if prim != R.UNDECIDED:
            return line
        p = kids[rng.randrange(len(kids))]
        line.append(p)


def play_paired(dims, rng):
    L, H, _ = dims
    p = o.initial(R.CONNECT, dims)
    line = [p]
    misses = 0
    while expand(dims, p)[0] == R.UNDECIDED and misses < 200:
        cols = [x for x, _ in open_columns(dims, p)]
        x, y = cols[rng.randrange(len(cols))], cols[rng.randrange(len(cols))]
        q = p
        for m in (x, y, L - 1 - x, L - 1 - y):
            prim, kids = expand(dims, q)
            now = [c for c, _ in open_columns(dims, q)]
            if prim != R.UNDECIDED or m not in now:
                q = None
                break
            q = kids[now.index(m)]
        if q is None or R.mirror(q, L, H) != q:
            misses += 1
            continue
        p = q
        line.append(p)
    return line


def play_steered(dims, rng, direction):
    """A game that ends in a K-line of `direction` through the top row, or None."""
    L, H, K = dims
    dx, dy = R.DIRS[direction]
    x0 = rng.randrange(L - (K - 1) * dx)
    target = [(x0 + j * dx, (H - K + j) if dy >= 0 else (H - 1 - j)) for j in range(K)]
    if direction == "horizontal":
        target = [(x0 + j, H - 1) for j in range(K)]
    last = max(target, key=lambda c: (c[1], rng.random()))
    winner = rng.choice((R.FIRST, R.SECOND))
    p = o.initial(R.CONNECT, dims)
    line = [p]
    discs = 0
    while True:
        prim, kids = expand(dims, p)
        if prim != R.UNDECIDED:
            break
        cols = open_columns(dims, p)
        mover = R.FIRST if discs % 2 == 0 else R.SECOND
        empty = L * H - discs
        if mover == winner:
            mine = [i for i, c in enumerate(cols) if c in target and (c != last or empty <= KEEP_LAST_UNTIL)]
            rest = [i for i, c in enumerate(cols) if c not in target]
            pick = mine or rest or list(range(len(cols)))
        else:
            pick = [i for i, c in enumerate(cols) if c not in target]
            if not pick:
                return None
        p = kids[pick[rng.randrange(len(pick))]]
        line.append(p)
        discs += 1
    cells, heights = R.cells_of([p], L, H)
    mine = cells == R.last_mover(heights)[:, None, None]
    s = R.line_starts(mine, K, direction)
    if not (s.size and R.touches(s, K, direction, "top", L, H)[0]):
        return None
    return line


def draw(dims, kind, seed):
    tries = 0
    while True:
        tries += 1
        assert tries < 3000, (dims, kind)
        rng = random.Random(seed)
        line = play_random(dims, rng) if kind == "random" else play_paired(dims, rng) if kind == "paired" \
            else play_steered(dims, rng, kind)
        n = 0
        if line:
            for p in reversed(line):
                if expand(dims, p)[0] != R.UNDECIDED:
                    continue
                n = count_below(dims, p, R.DRAWN_MAX)
                if n >= R.DRAWN_MIN:
                    break
        if line and R.DRAWN_MIN <= n <= R.DRAWN_MAX:
            return p, seed, n
        seed += 100


def built_16x2():
    """16x2, K = 2: columns 0..9 hold one disc each, first and second player in turn."""
    return R.key_of([[R.FIRST if x % 2 == 0 else R.SECOND] if x < 10 else [] for x in range(16)], 2)


def edge_positions():
    """[(dims, key)]: long runs of second-player stones, each position valid by the key's rules."""
    F, S = R.FIRST, R.SECOND
    out = []
    rng = random.Random(1)
    while True:     # 7x8: one column of 8 second-player stones, 10 first-player stones and 1 more elsewhere
        cols = [[] for _ in range(7)]
        cols[rng.randrange(7)] = [S] * 8
        free = [x for x in range(7) if not cols[x]]
        stones = [F] * 10 + [S]
        rng.shuffle(stones)
        for s in stones:
            cols[rng.choice(free)].append(s)
        k = R.key_of(cols, 8)
        if R.valid(k, 7, 8) and R.primitive([k], 7, 8, 4)[0] == R.UNDECIDED:
            out.append(((7, 8, 4), k))
            break
    # 3x20: 16 second-player stones; the first player's 26 in runs of three, and it has just moved
    out.append(((3, 20, 4), R.key_of([[S] * 16, [F, F, F, S] * 4 + [F, F], [F, F, F, S] * 4 + [S]], 20)))
    out.append(((2, 30, 4), R.key_of([[S] * 30, [F] * 30], 30)))
    out.append(((1, 62, 4), R.key_of([[S] * 31 + [F] * 31], 62)))
    return out


def main():
    print("EDGE = (")
    for dims, k in edge_positions():
        assert R.valid(k, dims[0], dims[1])
        print("    (%r, 0x%016X, %d)," % (dims, k, count_below(dims, k, R.DRAWN_MAX)))
    print(")")
    print("DRAWN = (")
    for dims, games in PLAN:
        L, H, K = dims
        for kind, seed in games:
            root, used, n = draw(dims, kind, seed)
            sym = R.mirror(root, L, H) == root
            assert sym == (kind == "paired") or kind != "paired"
            assert R.valid(root, L, H)
            print("    (%r, 0x%016X, %r, %r),   # seed %d, %d positions" % (dims, root, sym, kind, used, n), flush=True)
    dims = (16, 2, 2)
    root = built_16x2()
    print("    (%r, 0x%016X, %r, 'built'),   # %d positions" % (dims, root, R.mirror(root, 16, 2) == root,
                                                           count_below(dims, root, R.DRAWN_MAX)))
    print(")")


if __name__ == "__main__":
    main()
