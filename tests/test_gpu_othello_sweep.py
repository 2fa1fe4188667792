"""Synthetic Othello boards on both descriptors, on the device, against the C oracles.

tests/othello_roots.py holds the roots: 8x8 boards of 1 to 7 empties whose subtrees flip every
(mover colour, square, direction, run length) an 8x8 board admits, named 8x8 edge roots (full
boards, pass bytes 1 and 2 at the root, an unplayable square) and 4x4 boards of arbitrary contents
(tests/test_othello_roots.py states what they cover and pins the oracles to a third generator).

8x8 (csrc/games.hpp DescOthello8: step / run / legal / flips_at; 128-bit keys, 32-byte slots, the
hash-sharded sparse engine) at 1, 3 and 8 virtual ranks, one context per test id solving its roots
one after another, so consecutive solves differ in tier offset, depth and table size on tables the
context reuses.  Every read of the table is compared with oracle/othello8.c: count, root record,
export, digest, per-tier counts, histogram, verify, query inside and outside the table, and gm_moves
over the whole table -- the children in the ORACLE's order (csrc/moves_common.hpp move_slot), their
records, best / n_best by the rank order of include/gmsolve.h.

4x4 (DescOthello: the cell-walk flips, visit_part of the split kernels, the D4 canon) with and
without the symmetry reduction at 1 rank (the single-GPU sparse engine: at its default settings the
split kernels on every tier of these solves) and 4 virtual ranks, against oracle/gm_oracle.c; and
once more in a child process with GM_SPARSE_SPLIT_MAX=1, which puts the same roots through the
sorted-list batch kernels (visit() instead of visit_part()).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import othello8  # noqa: E402  (oracle/)
import othello_roots as R
from conftest import REPO
from othello_roots import OTH4_ROOTS, OTH8_EDGE, OTH8_ROOTS, key_of
from test_gpu_symmetry_roots import Ref, check_solve, open_ctx, othello_orbits
from test_symmetry_algebra import ref_images, ref_stabilizer

pytestmark = pytest.mark.gpu

from gamesmanmpi_amd import Context, _lib  # noqa: E402
from gamesmanmpi_amd._lib import GMError  # noqa: E402

OTH = 4
U64 = np.uint64
NONE = 0xFFFF
GM_E_KEY = -10
CHUNK8, CHUNK4 = 24, 24
CHUNKS8 = [OTH8_ROOTS[i:i + CHUNK8] for i in range(0, len(OTH8_ROOTS), CHUNK8)]
CHUNKS4 = [OTH4_ROOTS[i:i + CHUNK4] for i in range(0, len(OTH4_ROOTS), CHUNK4)]


def rank_of(recs):
    """The mover's preference among child records as include/gmsolve.h (gm_moves) documents it:
    LOSS (shortest) > TIE (shortest) > WIN (longest) > 0xFFFF.  Written from that sentence."""
    rec = np.asarray(recs, dtype=np.uint16).astype(np.int64)
    val, rem = rec >> 14, rec & 0x3FFF
    out = np.where(val == 1, (3 << 16) + (0x3FFF - rem), np.where(val == 2, (2 << 16) + (0x3FFF - rem), (1 << 16) + rem))
    out[rec == NONE] = 0
    return out


def best_of(child_recs, counts):
    """(best, n_best) per key: the first child of maximal rank (-1 without children), the number of
    children of that rank."""
    best, n_best = np.full(len(counts), -1, dtype=np.int64), np.zeros(len(counts), dtype=np.int64)
    r = rank_of(child_recs)
    at = 0
    for i, n in enumerate(counts.tolist()):
        if n:
            seg = r[at:at + n]
            best[i] = int(np.argmax(seg))       # argmax returns the first of equals
            n_best[i] = int((seg == seg.max()).sum())
            at += n
    return best, n_best


def sort144(words, recs):
    order = np.lexsort((words[:, 0], words[:, 1], words[:, 2]))
    return words[order], recs[order]


def lookup144(ref, words):
    """The oracle's record of every row of `words` (all of them positions of the table)."""
    index = ref.index
    return np.array([ref.recs[index[tuple(w)]] for w in words.tolist()], dtype=np.uint16)


class Ref8:
    """The 8x8 oracle's table from one root, with what the tests derive from it (read-only)."""

    def __init__(self, o8, root):
        self.root = tuple(int(x) for x in root)
        r = o8.solve(self.root, want=1 << 62)
        self.n, self.per_tier, self.root_record, self.digest = r["positions"], r["per_tier"], r["root_record"], r["digest"]
        self.words, self.recs = sort144(r["words"], r["records"])
        assert len(self.words) == self.n
        self.index = {tuple(w): i for i, w in enumerate(self.words.tolist())}
        assert self.recs[self.index[self.root]] == self.root_record
        value, rem = (self.recs >> 14).astype(np.int64), (self.recs & 0x3FFF).astype(np.int64)
        depth = int(rem.max()) + 1
        self.hist = np.bincount(value * depth + rem, minlength=3 * depth).reshape(3, depth).astype(U64)
        # gm_moves' answer over the whole table, from the oracle's expand
        counts, kids, outside = [], [], []
        for w in self.words.tolist():
            prim, _, ch = o8.expand(w)
            counts.append(len(ch) if prim == R.UNDECIDED else 0)
            kids.extend(ch)
            # a position whose mover has a move, with the pass byte set: only a pass, from a position
            # without moves, reaches pass byte 1
            if prim == R.UNDECIDED and w[0] & 0xFF == 0 and ch[0][0] & 0xFF == 0 and (w[0] | 1, w[1], w[2]) not in self.index:
                outside.append((w[0] | 1, w[1], w[2]))
        self.counts = np.array(counts, dtype=np.int64)
        self.kids = np.array(kids, dtype=U64).reshape(-1, 3)
        self.kid_recs = lookup144(self, self.kids)
        self.best, self.n_best = best_of(self.kid_recs, self.counts)
        self.outside = np.array(outside, dtype=U64).reshape(-1, 3)
        for a in (self.words, self.recs, self.hist, self.counts, self.kids, self.kid_recs, self.best, self.n_best, self.outside):
            a.setflags(write=False)


_o8 = []
_refs8 = {}


def ref8(root):
    if root not in _refs8:
        if not _o8:
            _o8.append(othello8.Othello8Oracle())
        _refs8[root] = Ref8(_o8[0], root)
    return _refs8[root]


def check_moves(ctx, ask, counts, kids, kid_recs, best, n_best, own):
    heads, ck, cr = ctx.moves_batch(ask)
    assert np.array_equal(heads["record"], own)
    assert np.array_equal(heads["count"], counts)
    assert np.array_equal(heads["first"], np.cumsum(counts) - counts)
    assert np.array_equal(ck, kids)             # the oracle's children in the oracle's order
    assert np.array_equal(cr, kid_recs)
    assert np.array_equal(heads["best"], best) and np.array_equal(heads["n_best"], n_best)


def check_solve8(ctx, ref, ranks):
    """Solve ref's root on ctx; every read of the table against the oracle's."""
    n, rec = ctx.solve(key_of(ref.root))
    assert (n, rec) == (ref.n, ref.root_record)
    st = ctx.stats()
    assert st["engine"] == _lib.ENGINE_DIST_SPARSE and st["world"] == ranks and st["n_positions"] == ref.n
    words, recs = ctx.export()
    assert words.shape == (ref.n, 3)
    words, recs = sort144(words, recs)
    assert np.array_equal(words, ref.words) and np.array_equal(recs, ref.recs)
    assert ctx.digest() == (ref.digest, ref.n)
    tiers = [int(x) for x in ctx.tier_counts()]
    while tiers and tiers[-1] == 0:
        tiers.pop()
    assert tiers == ref.per_tier
    assert np.array_equal(ctx.histogram(), ref.hist)
    res, bad = ctx.verify()
    assert res["n_bad"] == 0 and bad == [] and res["root_ok"] == 1 and res["checked"] == ref.n
    assert np.array_equal(ctx.query(ref.words), ref.recs)
    if len(ref.outside):
        assert (ctx.query(ref.outside) == NONE).all()
    check_moves(ctx, ref.words, ref.counts, ref.kids, ref.kid_recs, ref.best, ref.n_best, ref.recs)


def open8(ranks):
    ctx = Context(OTH, (8, 8), device=0)
    assert ctx.words == 3
    ctx.set_option(_lib.OPT_VIRTUAL_RANKS, ranks)
    return ctx


def name8(root):
    return "0x%04X_%016X_%016X" % (root[2], root[1], root[0])


# ---------------------------------------------------------------- 8x8
@pytest.mark.parametrize("chunk", range(len(CHUNKS8)))
@pytest.mark.parametrize("ranks", [1, 3, 8])
def test_othello8_synthetic_roots_vs_oracle(ranks, chunk):
    ctx = open8(ranks)
    outside = 0
    for root in CHUNKS8[chunk]:
        ref = ref8(root)
        try:
            check_solve8(ctx, ref, ranks)
        except AssertionError as e:
            raise AssertionError("root %s (%d positions)" % (name8(root), ref.n)) from e
        outside += len(ref.outside)
    assert outside >= 100       # the 0xFFFF answers were asked for
    ctx.close()


@pytest.mark.parametrize("ranks", [1, 3, 8])
def test_othello8_edge_roots_vs_oracle(ranks):
    """Full boards for either side at every pass byte (one position each; the device key of a full
    white-to-move board is one bit from the tables' empty mark), roots with pass byte 1 and 2, an
    unplayable last square; between them a drawn root, so a table of one slot follows a large one."""
    ctx = open8(ranks)
    for i, (name, root) in enumerate(OTH8_EDGE.items()):
        for r in (root, OTH8_ROOTS[i]):
            ref = ref8(r)
            try:
                check_solve8(ctx, ref, ranks)
            except AssertionError as e:
                raise AssertionError("root %s %s (%d positions)" % (name if r is root else "after " + name, name8(r), ref.n)) from e
    assert [ref8(r).n for r in OTH8_EDGE.values()] == [1, 1, 1, 1, 1, 1, 1, 2, 14, 3]
    ctx.close()


def test_othello8_root_with_an_empty_centre_square_is_refused():
    """Words that are no position of DescOthello8 (a centre square empty): GM_E_KEY before any
    launch, and the context solves the next root as if nothing had been asked."""
    ctx = open8(3)
    first, second = ref8(OTH8_ROOTS[0]), ref8(OTH8_ROOTS[1])
    check_solve8(ctx, first, 3)
    for cell in (27, 28, 35, 36):
        cells = R.cells_of(8, key_of(second.root))
        cells[cell] = 0
        bad = R.key_from_cells(8, cells, 1, 0)
        assert not R.valid(8, bad)
        with pytest.raises(GMError) as e:
            ctx.solve(bad)
        assert e.value.code == GM_E_KEY
    check_solve8(ctx, second, 3)
    ctx.close()


# ---------------------------------------------------------------- 4x4
_refs4 = {}


class Ref4(Ref):
    """The 4x4 oracle's table with gm_moves' answer from the reference generator's ordered lists."""

    def __init__(self, oracle, root):
        super().__init__(oracle, OTH, (4, 4), root)
        self.stab = int(ref_stabilizer(ref_images(np.array([root], dtype=U64), 4))[0])
        counts, kids = [], []
        for k in self.keys.tolist():
            prim, mv = R.expand(4, k)
            counts.append(len(mv))
            kids.extend(c for c, _, _ in mv)
        self.counts = np.array(counts, dtype=np.int64)
        self.kids = np.array(kids, dtype=U64)
        at = np.searchsorted(self.keys, self.kids)
        assert np.array_equal(self.keys[at], self.kids)
        self.kid_recs = self.recs[at]
        self.best, self.n_best = best_of(self.kid_recs, self.counts)
        for a in (self.counts, self.kids, self.kid_recs, self.best, self.n_best):
            a.setflags(write=False)


def ref4(oracle, root):
    if root not in _refs4:
        _refs4[root] = Ref4(oracle, root)
    return _refs4[root]


@pytest.mark.parametrize("chunk", range(len(CHUNKS4)))
@pytest.mark.parametrize("ranks", [1, 4])
@pytest.mark.parametrize("sym", [1, 0])
def test_othello4_synthetic_roots_vs_oracle(oracle, sym, ranks, chunk):
    ctx = open_ctx(OTH, (4, 4), sym, ranks)
    reduced = 0
    for root in CHUNKS4[chunk]:
        ref = ref4(oracle, root)
        orbits = othello_orbits(ref, ref.stab)
        assert ref.n // bin(ref.stab).count("1") <= orbits <= ref.n
        reduced += orbits < ref.n
        try:
            st = check_solve(ctx, ref, orbits if sym else ref.n)
            assert st["engine"] == (_lib.ENGINE_SPARSE if ranks == 1 else _lib.ENGINE_DIST_SPARSE) and st["world"] == ranks
            res, bad = ctx.verify()
            assert res["n_bad"] == 0 and bad == [] and res["root_ok"] == 1
            assert np.array_equal(ctx.query(ref.keys), ref.recs)
            check_moves(ctx, ref.keys, ref.counts, ref.kids, ref.kid_recs, ref.best, ref.n_best, ref.recs)
        except AssertionError as e:
            raise AssertionError("root 0x%012X (%d positions, stabiliser 0x%02X)" % (root, ref.n, ref.stab)) from e
    assert reduced >= 1         # some root of every chunk has a stabiliser that merges positions
    ctx.close()


_SORTED_LISTS = r'''
import os, sys
import numpy as np
repo = sys.argv[1]
sys.path.insert(0, repo)
sys.path.insert(0, os.path.join(repo, "tests"))
from conftest import Oracle
from othello_roots import OTH4_ROOTS
from gamesmanmpi_amd import Context, _lib
oracle = Oracle()
sym = int(sys.argv[2])
ctx = Context(4, (4, 4), device=0)
ctx.set_option(_lib.OPT_ENGINE, _lib.ENGINE_SPARSE)
ctx.set_option(_lib.OPT_SYMMETRY, sym)
for root in OTH4_ROOTS:
    keys, recs = oracle.solve(4, (4, 4), root=root)
    n, rec = ctx.solve(root)
    k, r = ctx.export()
    assert n == len(keys) and np.array_equal(k, keys) and np.array_equal(r, recs), hex(root)
    assert rec == int(recs[np.searchsorted(keys, np.uint64(root))]), hex(root)
ctx.close()
print("ok")
'''


@pytest.mark.parametrize("sym", [1, 0])
def test_othello4_synthetic_roots_sorted_lists_vs_oracle(sym):
    """GM_SPARSE_SPLIT_MAX=1 (read once: a fresh process) moves every tier of these solves from the
    split kernels (visit_part) to the sorted-list batch kernels (visit): every export equals the
    oracle's table."""
    env = dict(os.environ, GM_SPARSE_SPLIT_MAX="1")
    r = subprocess.run([sys.executable, "-c", _SORTED_LISTS, REPO, str(sym)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
