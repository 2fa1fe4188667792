"""Connect boards and roots on the device against the C oracle (oracle/gm_oracle.c G_CONNECT).

tests/connect_roots.py holds what is swept: full games on boards around the H > 7 branch of
DescConnect::filled (csrc/games.hpp), of one column, with K from 2 to 8, of one row and up to 12
columns, with a K that fits nowhere; and drawn mid-game roots on the 62- and 63-bit boards, on 16 and
15 columns, and with the long lines of K = 5..8 (tests/test_connect_roots.py states what the set
covers).  One context per (board, symmetry, virtual ranks) solves that board's roots one after
another, so consecutive solves differ in root tier, depth and table size on tables the context
reuses.  Every read of the table is compared with the oracle: count, root record, export, digest,
per-tier counts, histogram, n_stored, verify, query inside and outside the table, and gm_moves --
the children in the oracle's column order, their records, best / n_best by the rank order of
include/gmsolve.h.  Then select / reach / import on a tall and a wide board, the keys gm_solve
refuses, and child processes that put the same roots through the sorted-list batch kernels, their
sorted-pair check, the CSR kernels, and the unsorted path of tiers beyond GM_SPARSE_SORT_MAX.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import connect_roots as R
from conftest import GOLDEN, REPO, digest
from connect_roots import CONNECT, FULL
from test_gpu_othello_sweep import best_of, check_moves
from test_gpu_symmetry_roots import check_solve, open_ctx

sys.path.insert(0, GOLDEN)
import make_connect_golden as mcg  # noqa: E402

pytestmark = pytest.mark.gpu

from gamesmanmpi_amd import Context, _lib  # noqa: E402
from gamesmanmpi_amd._lib import GMError  # noqa: E402

U64 = np.uint64
NONE = 0xFFFF
GM_E_KEY = -10
MOVES_WHOLE = 50000      # gm_moves over the whole table up to here, over every 7th position above
BOARDS = R.boards()
IDS = ["%dx%d_%d" % d for d in BOARDS]


def roots_of(dims):
    """The board's roots in solve order: the empty board where the full game is swept, then the drawn."""
    return ([None] if dims in FULL else []) + [r for _, r, _, _ in R.drawn_of(dims)]


SYMMETRIC_BOARDS = [d for d in BOARDS if d in FULL or any(s for _, _, s, _ in R.drawn_of(d))]


def expand_many(oracle, dims, keys):
    """(counts, children in the oracle's column order) of every key, from one call of the library."""
    L = oracle.L
    P = ctypes.POINTER
    L.oracle_expand_many.restype = ctypes.c_int64
    L.oracle_expand_many.argtypes = [ctypes.c_int, P(ctypes.c_int32), ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                     ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    p, n = oracle._params(dims)
    keys = np.ascontiguousarray(keys, dtype=U64)
    kids = np.empty(len(keys) * dims[0] + 1, dtype=U64)
    counts = np.zeros(len(keys), dtype=np.int32)
    prims = np.zeros(len(keys), dtype=np.int32)
    total = L.oracle_expand_many(CONNECT, p, n, keys.ctypes.data, len(keys), kids.ctypes.data, len(kids),
                                 counts.ctypes.data, prims.ctypes.data)
    assert total >= 0
    return counts.astype(np.int64), kids[:total].copy(), prims


class Ref:
    """The oracle's table from one root, with what the tests derive from it (read-only); the fields
    test_gpu_symmetry_roots.check_solve reads, with Connect's tier: the disc count."""

    def __init__(self, oracle, dims, root):
        L, H, K = dims
        self.dims = dims
        self.root = oracle.initial(CONNECT, dims) if root is None else root
        self.keys, self.recs = oracle.solve(CONNECT, dims, root=self.root)
        self.n = len(self.keys)
        assert (self.keys[1:] > self.keys[:-1]).all()
        self.digest = digest(self.keys, self.recs)
        self.hist = mcg.histogram(self.recs).astype(U64)
        at = int(np.searchsorted(self.keys, U64(self.root)))
        assert int(self.keys[at]) == self.root
        self.root_record = int(self.recs[at])
        tier = mcg.discs(self.keys, L, H)
        self.tiers = np.bincount(tier - tier[at]).tolist()
        # the mirror reduction: one stored position per mirror pair, when the root is its own image
        m = R.mirror_keys(self.keys, L, H)
        some = range(0, self.n, max(1, self.n // 50))
        assert [int(m[i]) for i in some] == [mcg.mirror(int(self.keys[i]), L, H) for i in some]
        self.symmetric = mcg.mirror(self.root, L, H) == self.root
        self.reduced = (self.n + int((m == self.keys).sum())) // 2 if self.symmetric else self.n
        # valid positions outside the table: mirror images (of an asymmetric root's subtree) and
        # positions one disc past a finished line
        out = [m[~np.isin(m, self.keys)][:2000], R.after_the_end(self.keys, self.recs, L, H)]
        out = np.unique(np.concatenate(out))
        self.outside = out[~np.isin(out, self.keys)]
        assert all(R.valid(int(k), L, H) for k in self.outside[:: max(1, len(self.outside) // 40)].tolist())
        # gm_moves' answer, from the oracle's children and the oracle's records
        self.ask = self.keys if self.n <= MOVES_WHOLE else self.keys[::7].copy()
        self.ask_recs = self.recs if self.n <= MOVES_WHOLE else self.recs[::7].copy()
        self.counts, self.kids, prims = expand_many(oracle, dims, self.ask)
        assert np.array_equal(prims != R.UNDECIDED, (self.ask_recs & 0x3FFF) == 0)
        assert (self.counts[prims != R.UNDECIDED] == 0).all() and (self.counts[prims == R.UNDECIDED] >= 1).all()
        pos = np.searchsorted(self.keys, self.kids)
        assert np.array_equal(self.keys[pos], self.kids)
        self.kid_recs = self.recs[pos]
        self.best, self.n_best = best_of(self.kid_recs, self.counts)
        for a in (self.keys, self.recs, self.hist, self.outside, self.ask, self.ask_recs, self.counts, self.kids,
                  self.kid_recs, self.best, self.n_best):
            a.setflags(write=False)


_refs = {}


def ref_of(oracle, dims, root):
    if (dims, root) not in _refs:
        _refs[(dims, root)] = Ref(oracle, dims, root)
    return _refs[(dims, root)]


def check_all(ctx, ref, sym, ranks):
    """Solve ref's root on ctx; every read of the table against the oracle's."""
    stored = ref.reduced if sym else ref.n
    st = check_solve(ctx, ref, stored)
    assert st["engine"] == (_lib.ENGINE_SPARSE if ranks == 1 else _lib.ENGINE_DIST_SPARSE) and st["world"] == ranks
    res, bad = ctx.verify()
    assert res["n_bad"] == 0 and bad == [] and res["root_ok"] == 1 and res["checked"] == stored
    assert np.array_equal(ctx.query(ref.keys), ref.recs)
    if len(ref.outside):
        assert (ctx.query(ref.outside) == NONE).all()
    check_moves(ctx, ref.ask, ref.counts, ref.kids, ref.kid_recs, ref.best, ref.n_best, ref.ask_recs)


def sweep(oracle, dims, sym, ranks, roots):
    ctx = open_ctx(CONNECT, dims, sym, ranks)
    outside = 0
    try:
        for root in roots:
            ref = ref_of(oracle, dims, root)
            try:
                check_all(ctx, ref, sym, ranks)
            except AssertionError as e:
                raise AssertionError("%dx%d connect %d, root 0x%016X (%d positions), symmetry %d, %d ranks"
                                     % (dims + (ref.root, ref.n, sym, ranks))) from e
            outside += len(ref.outside)
    finally:
        ctx.close()
    print("swept %d solves, %d positions compared" % (len(roots), sum(ref_of(oracle, dims, r).n for r in roots)))
    return outside


@pytest.mark.parametrize("ranks", [1, 3, 8])
@pytest.mark.parametrize("dims", BOARDS, ids=IDS)
def test_every_root_with_the_reduction_on(oracle, dims, ranks):
    """Symmetry 1: a root that is its own mirror image stores one position per mirror pair, any other
    root every position."""
    roots = roots_of(dims)
    outside = sweep(oracle, dims, 1, ranks, roots)
    for root in roots:
        ref = ref_of(oracle, dims, root)
        assert (ref.reduced < ref.n) == (ref.symmetric and dims[0] > 1), hex(ref.root)
    # the 0xFFFF answers were asked for wherever lines end games
    if sum(int((ref_of(oracle, dims, r).recs == R.LOSS << 14).sum()) for r in roots) >= 5:
        assert outside >= 1


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("dims", SYMMETRIC_BOARDS, ids=["%dx%d_%d" % d for d in SYMMETRIC_BOARDS])
def test_symmetric_roots_with_the_reduction_off(oracle, dims, ranks):
    roots = [r for r in roots_of(dims) if ref_of(oracle, dims, r).symmetric]
    assert roots
    sweep(oracle, dims, 0, ranks, roots)


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("sym", [1, 0])
def test_positions_with_long_runs_of_second_player_stones(oracle, sym, ranks):
    """tests/connect_roots.py EDGE: columns of 8, 16, 30 and 31 second-player stones, which
    DescConnect::filled reaches only through its shifts by 8 and 16 (the root check, classify, every
    reader); between them a drawn root of the same board, so a table of a few slots follows a larger one."""
    for dims, key, positions in R.EDGE:
        after = R.drawn_of(dims)[:1]
        roots = [key] + [r for _, r, _, _ in after] + [key]
        assert ref_of(oracle, dims, key).n == positions
        sweep(oracle, dims, sym, ranks, roots)


# ---------------------------------------------------------------- the readers, tall and wide
@pytest.mark.parametrize("dims", [(2, 9, 4), (10, 1, 3)], ids=["2x9_4", "10x1_3"])
def test_select_reach_and_import_on_a_tall_and_a_wide_board(oracle, dims):
    ref = ref_of(oracle, dims, None)
    ctx = open_ctx(CONNECT, dims, 1, 1)
    other = Context(CONNECT, dims, device=0)
    try:
        assert ctx.solve(ref.root) == (ref.n, ref.root_record)
        # one cell of the histogram per value: the fullest one past remoteness 0
        for sel, value in ((_lib.SEL_WIN, 0), (_lib.SEL_LOSS, 1), (_lib.SEL_TIE, 2)):
            rem = int(np.argmax(ref.hist[value][1:])) + 1 if ref.hist.shape[1] > 1 and ref.hist[value][1:].any() else 0
            want = ref.keys[ref.recs == (value << 14 | rem)]
            assert len(want) == int(ref.hist[value][rem]) > 0, (value, rem)
            n, k, r = ctx.select(sel, rem, rem, cap=ref.n, as_array=True)
            assert n == len(want) and np.array_equal(k, want) and set(r.tolist()) == {value << 14 | rem}
        out, plies, _, _, _ = ctx.reach([ref.root], _lib.REACH_ALL, _lib.REACH_ALL)
        assert out["n"] == ref.n and out["missing"] == 0 and plies.tolist() == ref.tiers
        keys, recs = ctx.export()
        assert other.import_table(keys[::-1].copy(), recs[::-1].copy(), ref.root) == (ref.n, ref.root_record)
        res, bad = other.verify()
        assert res["n_bad"] == 0 and bad == [] and res["root_ok"] == 1
        assert other.stats()["n_stored"] == ctx.stats()["n_stored"] == ref.reduced
        k2, r2 = other.export()
        assert np.array_equal(k2, ref.keys) and np.array_equal(r2, ref.recs)
        assert other.digest() == (ref.digest, ref.n)
    finally:
        ctx.close()
        other.close()


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("dims", [(2, 9, 4), (10, 1, 3), (7, 8, 4)], ids=["tall", "wide", "63_bits"])
def test_keys_that_are_no_position_are_refused(oracle, dims):
    """GM_E_KEY before any launch, and the context solves a good root afterwards."""
    L, H, K = dims
    good = R.drawn_of(dims)[0][1] if R.drawn_of(dims) else oracle.initial(CONNECT, dims)
    cols = R.columns_of(good, L, H)
    field = (1 << (H + 1)) - 1
    lone = next(x for x in range(L) if len(cols[x]) < H)
    more = [c[:] for c in cols]
    more[lone].append(R.FIRST if sum(map(len, cols)) % 2 else R.SECOND)   # a disc of the player NOT to move
    bad = {"a zero column field": good & ~(field << ((L - 1) * (H + 1))),
           "a zero first column field": good & ~field,
           "the bit just above the board": good | 1 << (L * (H + 1)),
           "bit 63": good | 1 << 63,
           "a disc of the wrong colour": R.key_of(more, H)}
    ctx = open_ctx(CONNECT, dims, 1, 1)
    try:
        for why, k in bad.items():
            assert not R.valid(k, L, H), why
            with pytest.raises(GMError) as e:
                ctx.solve(k)
            assert e.value.code == GM_E_KEY, why
        check_all(ctx, ref_of(oracle, dims, good if R.drawn_of(dims) else None), 1, 1)
    finally:
        ctx.close()


# ---------------------------------------------------------------- the other kernel families
_CHILD = r'''
import os, sys
import numpy as np
repo = sys.argv[1]
sys.path.insert(0, repo)
sys.path.insert(0, os.path.join(repo, "tests"))
from conftest import Oracle
import connect_roots as R
from gamesmanmpi_amd import Context, _lib
oracle = Oracle()
boards = [tuple(int(x) for x in b.split("x")) for b in sys.argv[3].split(",")] if sys.argv[3] else R.boards()
repeats = int(sys.argv[2])
solves = 0
for dims in boards:
    roots = ([oracle.initial(R.CONNECT, dims)] if dims in R.FULL else []) + [r for _, r, _, _ in R.drawn_of(dims)][:1] \
        + [k for d, k, _ in R.EDGE if d == dims]
    ctx = Context(R.CONNECT, dims, device=0)
    ctx.set_option(_lib.OPT_ENGINE, _lib.ENGINE_SPARSE)
    for root in roots:
        keys, recs = oracle.solve(R.CONNECT, dims, root=root)
        for _ in range(repeats):
            n, rec = ctx.solve(root)
            k, r = ctx.export()
            assert n == len(keys) and np.array_equal(k, keys) and np.array_equal(r, recs), (dims, hex(root))
            assert rec == int(recs[np.searchsorted(keys, np.uint64(root))]), (dims, hex(root))
            solves += 1
    ctx.close()
print("solves", solves)
print("ok")
'''


def run_child(env, repeats=1, boards=""):
    env = dict(os.environ, **env)
    r = subprocess.run([sys.executable, "-c", _CHILD, REPO, str(repeats), boards], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    return r


@pytest.mark.parametrize("env", [{"GM_SPARSE_SPLIT_MAX": "1"},
                                 {"GM_SPARSE_SPLIT_MAX": "1", "GM_SPARSE_BATCH": "3"},
                                 {"GM_SPARSE_SPLIT_MAX": "1", "GM_SPARSE_CSR": "1"}],
                         ids=["sorted_lists", "sorted_pair_check", "csr"])
def test_every_board_through_the_batch_kernels(env):
    """The variables are read once, so a fresh process: GM_SPARSE_SPLIT_MAX=1 moves every tier from the
    split kernels (visit_part) to the sorted-list batch kernels (visit), GM_SPARSE_BATCH=3 adds the check
    of every sorted pair, GM_SPARSE_CSR=1 selects the CSR kernels (Connect moves one tier deeper; the
    16-column boards fill a parent's child count to its limit).  Every full game and one root per
    drawn board: the export equals the oracle's table."""
    assert any(d[0] == 16 for d in BOARDS)
    run_child(env)


def test_tiers_beyond_the_sort_threshold_are_solved_unsorted(oracle):
    """A tier whose interior count exceeds the batch sort's count is not sorted (csrc/sparse.hip
    sort_max): with GM_SPARSE_SORT_MAX=1000 the 2x9 and 10x1 full games have tiers on both sides of
    1,000 interior positions; each root is solved twice in one context, so the recorded plan, which
    sorts only the tiers that were sorted, replays."""
    for dims in ((2, 9, 4), (10, 1, 3)):
        ref = ref_of(oracle, dims, None)
        interior = np.bincount(mcg.discs(ref.keys, *dims[:2])[(ref.recs & 0x3FFF) != 0])
        assert (interior > 1000).any() and ((interior >= 1) & (interior <= 1000)).any(), dims
    run_child({"GM_SPARSE_SPLIT_MAX": "1", "GM_SPARSE_SORT_MAX": "1000"}, repeats=2, boards="2x9x4,10x1x3")
    # with the sorted-pair check the sorted tiers report themselves and the others stay silent
    r = run_child({"GM_SPARSE_SPLIT_MAX": "1", "GM_SPARSE_SORT_MAX": "1000", "GM_SPARSE_BATCH": "3"}, boards="2x9x4")
    sizes = [int(line.split(":")[1].split()[0]) for line in r.stderr.splitlines() if "batch sort of tier" in line]
    assert sizes and max(sizes) <= 1000
