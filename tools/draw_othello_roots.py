#!/usr/bin/env python3
"""Draws the literal root sets of tests/othello_roots.py (OTH8_ROOTS, OTH8_EDGE, OTH4_ROOTS).

    python tools/draw_othello_roots.py            # prints the block
    python tools/draw_othello_roots.py --write    # replaces the block in tests/othello_roots.py

No test calls this: the sets are literals, and tests/test_othello_roots.py checks the conditions
they were drawn to meet.  The generator walked here is the reference one of tests/othello_roots.py;
position counts of 8x8 candidates come from the C oracle (oracle/othello8.c) first, which is quick
at refusing the large ones.

8x8: random boards first, then constructed ones -- all of the mover's colour but for a few empty
squares that each start a ray of opponent discs closed by a mover's disc, the rays taken from the
flip cases no accepted root covers yet, the best of a batch of candidates at a time -- until every
feasible case is covered, then random boards again up to N8.  A root has 1 to 7 empties and at most
CAP8 positions below it; about a quarter carry pass byte 1.
4x4: random boards of 1 to 12 empties and arbitrary contents, boards of one colour, boards
symmetrised under every non-trivial subgroup of D4 whose subtrees the subgroup shrinks by a fifth
or more, at most CAP4 positions each.
"""
import argparse
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

import othello_roots as R  # noqa: E402

CAP8, CAP4 = 3000, 4000
N8, N4 = 120, 96          # roots at least / exactly
N8_RANDOM, BATCH8 = 45, 24   # random roots drawn first; constructed candidates per greedy pick
MARK = "# ---------------------------------------------------------------- the drawn sets\n"


# ---------------------------------------------------------------- 8x8
def random8(rng):
    e = rng.randint(1, 7)
    free = [j for j in range(64) if (j % 8, j // 8) not in R.CENTRE8]
    holes = set(rng.sample(free, e))
    p = rng.random()
    cells = [0 if j in holes else (R.WHITE if rng.random() < p else R.BLACK) for j in range(64)]
    return R.key_from_cells(8, cells, rng.randint(1, 2), 1 if rng.random() < 0.25 else 0)


def constructed8(rng, wanted):
    """A board for up to seven of the wanted flip cases of one colour, or None."""
    me = rng.choice((R.BLACK, R.WHITE))
    mine = [c for c in wanted if c[0] == me]
    if not mine:
        return None
    rng.shuffle(mine)
    cells = [me] * 64
    holes, closers, runs = set(), set(), set()
    want = rng.randint(4, 7)
    for _, x, y, d, n in mine:
        j = 8 * y + x
        line = dict(R.rays(8)[j])[d]
        run, closer = set(line[:n]), line[n]
        if j in holes or j in closers or j in runs or run & holes or closer in holes or closer in runs or run & closers:
            continue
        holes.add(j)
        runs |= run
        closers.add(closer)
        if len(holes) == want:
            break
    for j in runs:
        cells[j] = 3 - me
    for j in holes:
        cells[j] = 0
    for _ in range(rng.randint(0, 3)):      # a few more opponent discs, off the rays' ends
        j = rng.randrange(64)
        if j not in holes and j not in closers:
            cells[j] = 3 - me
    if not all(cells[8 * y + x] for x, y in R.CENTRE8):
        return None
    return R.key_from_cells(8, cells, me, 1 if rng.random() < 0.25 else 0)


def draw8(rng):
    from othello8 import Othello8Oracle
    o8 = Othello8Oracle()

    def small(key):
        return R.valid(8, key) and o8.solve(R.words_of(key))["positions"] <= CAP8

    wanted = R.feasible(8)
    roots, walks = [], []

    def random_roots(upto, least):
        while len(roots) < upto:
            key = random8(rng)
            if key in roots or not small(key):
                continue
            w = R.Walk(8, key)
            if len(w) < least and rng.random() < 0.9:   # mostly subtrees worth a solve
                continue
            roots.append(key)
            walks.append(w)
            wanted.difference_update(w.cases)

    random_roots(N8_RANDOM, 200)
    while wanted:                                # greedy: the best of a batch of constructed boards
        best = None
        for _ in range(BATCH8):
            key = constructed8(rng, wanted)
            if key is None or key in roots or not small(key):
                continue
            w = R.Walk(8, key)
            if best is None or len(w.cases & wanted) > len(best[1].cases & wanted):
                best = (key, w)
        assert best is not None and best[1].cases & wanted, "%d flip cases left uncovered" % len(wanted)
        roots.append(best[0])
        walks.append(best[1])
        wanted -= best[1].cases
    n_constructed = len(roots) - N8_RANDOM
    random_roots(N8, 50)
    order = list(range(len(roots)))
    rng.shuffle(order)                           # consecutive solves of a context differ in kind
    print("8x8: %d constructed + %d random roots, %d positions, %d passes, %d double-pass ends, most directions %d"
          % (n_constructed, len(roots) - n_constructed, sum(len(w) for w in walks), sum(w.passes for w in walks),
             sum(w.double_pass_ends for w in walks), max(w.most_dirs for w in walks)), file=sys.stderr)
    return [roots[i] for i in order]


def board8(rows, turn, npass):
    """Rows of 'X' black, 'O' white, '.' empty, top row y = 0."""
    cells = [{"X": R.BLACK, "O": R.WHITE, ".": 0}[c] for row in rows for c in row]
    assert len(cells) == 64
    return R.key_from_cells(8, cells, turn, npass)


def edge8(rng):
    mixed = ["".join(rng.choice("XO") for _ in range(8)) for _ in range(8)]
    tie = ["XOXOXOXO", "OXOXOXOX"] * 4
    black = ["XXXXXXXX"] * 8
    out = {}
    for turn, who in ((R.BLACK, "black"), (R.WHITE, "white")):
        for npass in (0, 1, 2):
            rows = tie if (who, npass) == ("black", 1) else black if (who, npass) == ("white", 2) else mixed
            out["full_%s_pass%d" % (who, npass)] = board8(rows, turn, npass)
    # the second pass made with empty squares left: primitive, one position
    out["pass2_with_empties"] = board8(["XXXXXXXX", "XOOOOOX.", "XXXXXXXX", "XXXOOXXX", "XXXOXXXX", "XXXXXXXX",
                                        ".OXXXXXX", "XXXXXXX."], R.BLACK, 2)
    # pass byte 1 and the mover (white, without a disc to close a run) passes again: two positions
    out["pass1_passes_again"] = board8(["XXXXXXX.", "XXXXXXXX", "XXXXXXXX", "XXXXXXXX", "XXXXXXXX", "XXXXXXXX",
                                        "XXXXXXXX", ".XXXXXX."], R.WHITE, 1)
    # pass byte 1 and the mover has a move: the first tier step is 2, not 3
    out["pass1_has_a_move"] = board8([".OOOOOOX", "XXXXXXXX", "XOXXXXXX", ".XOXXXXX", "XXXOOXXX", "XXXOXOXX",
                                      "XXXXXXOX", "XXX.OOOX"], R.BLACK, 1)
    # one empty square that neither side can play: root, pass, second pass
    out["one_empty_unplayable"] = board8([".XXXXXXX", "XXXXXXXX", "XXXXXXXX", "XXXXOXXX", "XXXOXXXX", "XXXXXXXX",
                                          "XXXXXXXX", "XXXXXXXX"], R.WHITE, 0)
    return out


# ---------------------------------------------------------------- 4x4
def d4_cell(g, x, y, L=4):
    return {0: (x, y), 1: (L - 1 - y, x), 2: (L - 1 - x, L - 1 - y), 3: (y, L - 1 - x), 4: (y, x),
            5: (L - 1 - y, L - 1 - x), 6: (L - 1 - x, y), 7: (x, L - 1 - y)}[g]


def symmetrised4(cells, mask):
    """White the union of the white cells' images under the subgroup, black the union of the black
    cells' images off white."""
    out = [0] * 16
    for colour in (R.BLACK, R.WHITE):
        for j in range(16):
            if cells[j] != colour:
                continue
            for g in range(8):
                if (mask >> g) & 1:
                    x, y = d4_cell(g, j % 4, j // 4)
                    out[4 * y + x] = colour
    return out


def random_cells4(rng, e=None):
    e = rng.randint(1, 12) if e is None else e
    holes = set(rng.sample(range(16), e))
    p = rng.random()
    return [0 if j in holes else (R.WHITE if rng.random() < p else R.BLACK) for j in range(16)]


def draw4(rng):
    import numpy as np
    from test_symmetry_algebra import SUBGROUPS, ref_canon, ref_images
    roots, walks = [], []

    def take(key):
        if key in roots or not 1 <= R.empties(4, key) <= 12:
            return False
        w = R.Walk(4, key)
        if len(w) > CAP4:
            return False
        roots.append(key)
        walks.append(w)
        return True

    for colour in (R.BLACK, R.WHITE):            # one colour only, either side to move
        for turn in (R.BLACK, R.WHITE):
            cells = [0 if c == 0 else colour for c in random_cells4(rng, rng.randint(2, 6))]
            assert take(R.key_from_cells(4, cells, turn, 0))
    for mask in SUBGROUPS[1:]:                   # fixed by a subgroup, which merges positions below
        done = tries = 0
        while done < 3:
            tries += 1
            cells = symmetrised4(random_cells4(rng, rng.randint(6, 13)), mask)
            key = R.key_from_cells(4, cells, rng.randint(1, 2), 0)
            keys = np.array(sorted(R.Walk(4, key).kids), dtype=np.uint64)
            shrunk = len(keys) >= 30 and len(np.unique(ref_canon(ref_images(keys, 4), mask))) <= 0.8 * len(keys)
            if shrunk or tries > 200:            # (the larger subgroups leave few boards with room to play)
                done += take(key)
    while len(roots) < N4:
        cells = random_cells4(rng)
        key = R.key_from_cells(4, cells, rng.randint(1, 2), 1 if rng.random() < 0.15 else 0)
        if len(R.Walk(4, key)) < 10 and rng.random() < 0.8:
            continue
        take(key)
    cases = set().union(*(w.cases for w in walks))
    assert cases == R.feasible(4), "%d 4x4 flip cases left uncovered" % len(R.feasible(4) - cases)
    order = list(range(len(roots)))
    rng.shuffle(order)
    print("4x4: %d roots, %d positions, largest %d" % (len(roots), sum(len(w) for w in walks), max(len(w) for w in walks)),
          file=sys.stderr)
    return [roots[i] for i in order]


def block(seed):
    rng = random.Random(seed)
    r8, e8, r4 = draw8(rng), edge8(rng), draw4(rng)
    out = [MARK,
           "# 8x8 roots as (w0, w1, w2): 1 to 7 empties, at most %d positions below each; constructed boards\n" % CAP8,
           "# (mostly the mover's colour, a few empty squares that each start a closed ray of opponent discs)\n",
           "# and random ones, about a quarter with pass byte 1\n",
           "OTH8_ROOTS = (\n"]
    out += ["    (0x%016X, 0x%016X, 0x%04X),\n" % R.words_of(k) for k in r8]
    out += [")\n\n",
            "# named 8x8 roots, added by hand: full boards for either side at every pass byte (a full white-to-move\n",
            "# board is one bit away from the table's empty mark), roots that start with pass byte 1 or 2, and a\n",
            "# square that nobody can play\n",
            "OTH8_EDGE = {\n"]
    out += ['    "%s": (0x%016X, 0x%016X, 0x%04X),\n' % ((name,) + R.words_of(k)) for name, k in e8.items()]
    out += ["}\n\n",
            "# 4x4 keys: 1 to 12 empties and arbitrary contents (empty centres, one colour only, boards fixed by\n",
            "# every non-trivial subgroup of D4), at most %d positions below each\n" % CAP4,
            "OTH4_ROOTS = (\n"]
    out += ["    " + " ".join("0x%012X," % k for k in r4[i:i + 6]) + "\n" for i in range(0, len(r4), 6)]
    out += [")\n"]
    return "".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    text = block(a.seed)
    if not a.write:
        sys.stdout.write(text)
        return
    path = os.path.join(REPO, "tests", "othello_roots.py")
    src = open(path).read()
    open(path, "w").write(src[:src.index(MARK)] + text)


if __name__ == "__main__":
    main()
