"""Every tic-tac-toe root and Four-To-One up to the end of the 14-bit remoteness, on the device.

Tic-tac-toe: all 3^9 boards are legal roots (csrc/games.hpp DescTTT::valid), also those no game
reaches -- any piece counts, two lines, full boards -- and only on those does the mover rule
`no >= nx ? X : O` differ from "X on an even piece count".  The one-workgroup LDS engine
(csrc/small_dense.hip), whose kernel takes the root and its tier as arguments, solves every one
of them; the sparse engine and the hash-sharded engine (3 virtual ranks) the 1,873 roots of
tests/small_roots.py TTT_STRATA.  Every table is compared bit for bit with oracle_solve of the
same root (tests/test_small_roots.py compares that with the plugins).

Four-To-One is the one descriptor game of unbounded depth -- one position per tier, the root is
the depth -- so only it drives the tier-table engines (csrc/sparse.hip, csrc/dist_sparse.hip,
csrc/sparse_tables.hpp) to where score_overflows matters, past gm_import's 1,024 tiers, past the
4,096 bins per value that fit the census kernel's LDS, and through a replay of thousands of
tiers.  Its tables are compared with the closed form (tests/small_roots.py f2o_table) and the
oracle.  No Four-To-One root above 24,576 is solved here: the forward pass has no depth bound.

One context per engine walks its roots in a fixed shuffled order, so a 5,478-position solve is
followed by a one-position one: state that survives a re-solve (the replay plan, the LDS engine's
host copy, cached buffers) shows as a wrong table.

Measured on an MI355X: the whole file takes 41 s, the tic-tac-toe ids at most 0.7 s each, root
3,000 with its replay 0.7 s (sparse), 2.7 s and 4.0 s (2 and 3 virtual ranks), root 7,000 1.0 s, 3.6 s
and 6.0 s, the limit test 13 s (see DEEP_ENGINES).
"""
import numpy as np
import pytest

from conftest import digest, golden
from small_roots import (F2O_DEEPEST, F2O_FIRST_REFUSED, F2O_IMPORT_DEEPEST, F2O_SMALL, LOSS, TTT_BY_PIECES, TTT_STRATA,
                         f2o_histogram, f2o_key, f2o_record, f2o_table, histogram_of, shuffled, ttt_outside_key, ttt_pieces)

from gamesmanmpi_amd import Context, GMError, _lib, reach
from gamesmanmpi_amd.solver import best_move

pytestmark = pytest.mark.gpu

F2O, TTT = 1, 2
UNDECIDED = 4
E_STATE, E_CAP, E_KEY = -5, -8, -10
UNSOLVED = _lib.REC_UNSOLVED
SHARDS = 3   # virtual ranks of the sharded tic-tac-toe sweeps

PIECES = np.array([ttt_pieces(k) for k in range(3 ** 9)])


def _chunks(roots, k):
    """`roots` in k nearly equal runs."""
    n = len(roots)
    return [roots[n * i // k:n * (i + 1) // k] for i in range(k)]


# ---------------------------------------------------------------- tic-tac-toe: the references
@pytest.fixture(scope="module")
def ttt_ref(oracle):
    """root -> (keys, records, primitive positions, positions per piece count), from the oracle;
    the tables of the TTT_STRATA roots, which several tests walk, are kept."""
    prim = np.array([oracle.expand(TTT, (), k)[0] != UNDECIDED for k in range(3 ** 9)])
    kept, strata = {}, set(TTT_STRATA)

    def ref(root):
        if root in kept:
            return kept[root]
        keys, recs = oracle.solve(TTT, (), root)
        k = keys.astype(np.int64)
        out = (keys, recs, int(prim[k].sum()), np.bincount(PIECES[k], minlength=10))
        if root in strata:
            kept[root] = out
        return out

    ref.interior = lambda root: not prim[root]
    return ref


class _Contexts:
    """One context per engine name, made on first use and shared by the tests of the module."""
    OPTIONS = {"lds": {}, "sparse": {"ENGINE": _lib.ENGINE_SPARSE}, "sharded": {"VIRTUAL_RANKS": SHARDS},
               "replay": {"ENGINE": _lib.ENGINE_SPARSE}}
    ENGINE = {"lds": _lib.ENGINE_DENSE, "sparse": _lib.ENGINE_SPARSE, "sharded": _lib.ENGINE_DIST_SPARSE,
              "replay": _lib.ENGINE_SPARSE}

    def __init__(self, game):
        self.game, self.ctxs = game, {}

    def __call__(self, name, **options):
        if name not in self.ctxs:
            c = Context(self.game, (), device=0)
            for k, v in dict(self.OPTIONS.get(name, {}), **options).items():
                c.set_option(getattr(_lib, "OPT_" + k), v)
            self.ctxs[name] = c
        return self.ctxs[name]

    def close(self):
        for c in self.ctxs.values():
            c.close()


@pytest.fixture(scope="module")
def ttt_ctx():
    c = _Contexts(TTT)
    yield c
    c.close()


def _ttt_solve_and_check(ctx, ref, engine, root):
    """One solve and what the context then answers about it, against the oracle's table."""
    keys, recs, n_prim, by_pieces = ref(root)
    where = "%s root %d" % (engine, root)
    root_rec = int(recs[np.searchsorted(keys, root)])
    n, rec = ctx.solve(root)
    assert (n, rec) == (len(keys), root_rec), where
    k, r = ctx.export()
    assert np.array_equal(k, keys), where
    if not np.array_equal(r, recs):
        i = int(np.nonzero(r != recs)[0][0])
        pytest.fail("%s: %d records differ, the first at key %d: expected 0x%04X, got 0x%04X"
                    % (where, int((r != recs).sum()), int(keys[i]), int(recs[i]), int(r[i])))
    st = ctx.stats()
    assert st["engine"] == _Contexts.ENGINE[engine], where
    assert (st["n_positions"], st["n_primitive"]) == (len(keys), n_prim), where
    assert ctx.query([root, ttt_outside_key(root)]).tolist() == [root_rec, UNSOLVED], where
    # gm_tier_counts (include/gmsolve.h): the LDS engine by absolute piece count, the tier engines
    # from the root's tier to the last one reached
    tiers = ctx.tier_counts().tolist()
    if engine == "lds":
        assert tiers == by_pieces.tolist(), where
    else:
        t0 = int(PIECES[root])
        assert tiers == by_pieces[t0:int(np.nonzero(by_pieces)[0][-1]) + 1].tolist(), where
        assert ctx.digest() == (digest(keys, recs), len(keys)), where
        if engine == "sharded":
            assert st["world"] == SHARDS, where
    return n, rec


# ---------------------------------------------------------------- tic-tac-toe: the sweeps
@pytest.mark.parametrize("pieces", range(10))
def test_ttt_lds_engine_every_root(ttt_ctx, ttt_ref, pieces):
    """All 19,683 roots on the one-workgroup engine, by piece count: 1, 18, 144, 672, 2,016,
    4,032, 5,376, 4,608, 2,304 and 512 roots."""
    ctx = ttt_ctx("lds")
    for root in shuffled(TTT_BY_PIECES[pieces]):
        _ttt_solve_and_check(ctx, ttt_ref, "lds", root)


STRATA_ORDER = shuffled(TTT_STRATA)
N_CHUNKS = 8


@pytest.mark.parametrize("chunk", range(N_CHUNKS))
@pytest.mark.parametrize("engine", ["sparse", "sharded"])
def test_ttt_tier_engines_every_strata_root(ttt_ctx, ttt_ref, engine, chunk):
    """The 1,873 roots of TTT_STRATA on the sparse engine and on the hash-sharded engine with 3
    virtual ranks, one context each over all chunks."""
    ctx = ttt_ctx(engine)
    for root in _chunks(STRATA_ORDER, N_CHUNKS)[chunk]:
        _ttt_solve_and_check(ctx, ttt_ref, engine, root)


def _reader_roots(ref):
    return shuffled([k for k in TTT_STRATA if ref.interior(k)][::10])


@pytest.mark.parametrize("engine", ["lds", "sparse", "sharded"])
def test_ttt_readers_on_custom_roots(ttt_ctx, ttt_ref, oracle, engine):
    """gm_verify, gm_histogram, gm_reach, gm_select and gm_moves after a solve from every 10th
    non-primitive root of TTT_STRATA."""
    roots = _reader_roots(ttt_ref)
    assert len(roots) >= 70
    ctx = ttt_ctx(engine)
    for root in roots:
        keys, recs, _, _ = ttt_ref(root)
        where = "%s root %d" % (engine, root)
        n, rec = ctx.solve(root)
        assert n == len(keys), where
        v, bad = ctx.verify()
        assert (v["n_bad"], v["root_ok"], v["checked"]) == (0, 1, n), (where, v, bad[:4])
        h, want = ctx.histogram(), histogram_of(recs)
        assert h.shape == want.shape and np.array_equal(h, want), where
        out, plies, rk, rr, _ = ctx.reach([root], _lib.REACH_ALL, _lib.REACH_ALL, cap=n)
        assert out["n"] == n and out["n_starts"] == 1 and out["missing"] == 0, (where, out)
        assert np.array_equal(np.sort(rk), keys) and np.array_equal(rr[np.argsort(rk)], recs), where
        assert plies.tolist() == np.bincount(PIECES[keys.astype(np.int64)])[int(PIECES[root]):].tolist(), where
        assert ctx.select(_lib.SEL_WIN | _lib.SEL_LOSS | _lib.SEL_TIE, cap=0)[0] == n, where
        heads, ck, cr = ctx.moves_batch([root])
        kids = oracle.expand(TTT, (), root)[1]   # ascending, which is the plugin's move order: cell by cell
        assert (int(heads[0]["first"]), int(heads[0]["count"]), int(heads[0]["record"])) == (0, len(kids), rec), where
        assert ck.tolist() == kids and np.array_equal(cr, recs[np.searchsorted(keys, np.array(kids, np.uint64))]), where
        assert int(heads[0]["best"]) == best_move(cr)[0], where


def test_ttt_sparse_replay_on_custom_roots(ttt_ctx, ttt_ref):
    """Each of 20 non-primitive roots solved twice in a row on one sparse context: the second
    solve replays the first one's recorded tier sequence (csrc/sparse.hip replay_with; it alone
    reports forward_ms 0) and must give the same root record and export; the next root must not
    reuse the record."""
    roots = shuffled([k for k in TTT_STRATA if ttt_ref.interior(k)], seed=1)[:20]
    ctx = ttt_ctx("replay")
    for root in roots:
        keys, recs, _, _ = ttt_ref(root)
        first = _ttt_solve_and_check(ctx, ttt_ref, "replay", root)
        assert ctx.stats()["forward_ms"] > 0, root
        again = _ttt_solve_and_check(ctx, ttt_ref, "replay", root)
        assert again == first and ctx.stats()["forward_ms"] == 0, root


# ---------------------------------------------------------------- Four-To-One
F2O_ENGINES = ["sparse", "sharded2", "sharded3"]


@pytest.fixture(scope="module")
def f2o_ctx():
    c = _Contexts(F2O)
    yield c
    c.close()


def _f2o(f2o_ctx, engine):
    return f2o_ctx(engine, **({"VIRTUAL_RANKS": int(engine[-1])} if engine.startswith("sharded") else {}))


def _f2o_expand(key):
    """Context.expand of a Four-To-One key by the rules: take 1, take 2 (test_games/four_to_one.py)."""
    pile = key - (1 << 64) if key >> 63 else key
    return (LOSS, [], -pile) if pile <= 0 else (UNDECIDED, [f2o_key(pile - 1), f2o_key(pile - 2)], -pile)


def _f2o_check_export(ctx, root, oracle=None):
    keys, recs = f2o_table(root)
    k, r = ctx.export()
    assert np.array_equal(k, keys) and np.array_equal(r, recs), root
    if oracle is not None:
        ok, orec = oracle.solve(F2O, (), f2o_key(root))
        assert np.array_equal(k, ok) and np.array_equal(r, orec), root
    return keys, recs


@pytest.mark.parametrize("engine", F2O_ENGINES)
def test_f2o_small_roots(f2o_ctx, oracle, engine):
    """Roots -3 .. 40: a root of 0 or less is a single primitive position; -1 is the key 2^64 - 1,
    the last of every export."""
    ctx = _f2o(f2o_ctx, engine)
    for root in shuffled(F2O_SMALL):
        n, rec = ctx.solve(f2o_key(root))
        keys, recs = _f2o_check_export(ctx, root, oracle)
        assert (n, rec) == (len(keys), f2o_record(root)), root
        assert ctx.digest() == (digest(keys, recs), n), root
        assert ctx.stats()["n_primitive"] == (1 if root <= 0 else 2), root
        assert ctx.tier_counts().tolist() == [1] * n, root
        assert ctx.query([f2o_key(root), f2o_key(root + 1)]).tolist() == [rec, UNSOLVED], root


@pytest.mark.parametrize("engine", F2O_ENGINES)
def test_f2o_roots_outside_the_game_are_refused(f2o_ctx, engine):
    """|pile| >= 2^60 is no position (DescF2O::valid): GM_E_KEY before any launch."""
    ctx = _f2o(f2o_ctx, engine)
    ctx.solve(6)
    for root in (1 << 60, f2o_key(-(1 << 60))):
        with pytest.raises(GMError) as e:
            ctx.solve(root)
        assert e.value.code == E_KEY and "not a valid position" in str(e.value)
        _f2o_check_export(ctx, 6)   # refused before the context was touched: it still holds root 6
    ctx.solve(f2o_key(-(1 << 60) + 1))   # the last pile inside: a single primitive position
    assert ctx.export()[1].tolist() == [LOSS << 14]


@pytest.fixture
def f2o_own():
    """Contexts of one test alone, closed whatever the test's outcome."""
    c = _Contexts(F2O)
    yield c
    c.close()


def test_f2o_import_depth(f2o_own, oracle):
    """gm_import takes keys up to 1,023 tiers below the root (csrc/sparse_tables.hpp
    IMPORT_MAX_TIERS: tier - t_root < 1,024).  Pile -1 lies root + 1 tiers below the root, so
    the table of root 1,022 imports and the table of root 1,023 is GM_E_CAP.  (One context, no
    virtual ranks: gm_import builds the whole table in one context.)"""
    root = F2O_IMPORT_DEEPEST
    keys, recs = f2o_table(root)
    ctx = f2o_own("solved")
    n, rec = ctx.solve(root)
    assert ctx.stats()["engine"] == _lib.ENGINE_SPARSE and ctx.stats()["n_primitive"] == 2
    solved = (ctx.digest(), ctx.verify()[0], ctx.query(keys[::37]).tolist(), ctx.tier_counts().tolist())
    ctx = f2o_own("imported")
    order = np.random.default_rng(0).permutation(len(keys))
    assert ctx.import_table(keys[order], recs[order], root) == (n, rec) == (root + 2, f2o_record(root))
    st = ctx.stats()
    assert st["engine"] == _lib.ENGINE_SPARSE and (st["n_positions"], st["n_stored"], st["n_tiers"]) == (n, n, n)
    assert st["n_primitive"] == 0   # an import classifies nothing (include/gmsolve.h gm_stats_t)
    _f2o_check_export(ctx, root, oracle)
    v = ctx.verify()[0]
    assert (v["n_bad"], v["root_ok"], v["checked"]) == (0, 1, n)
    assert (ctx.digest(), v, ctx.query(keys[::37]).tolist(), ctx.tier_counts().tolist()) == solved
    assert ctx.digest() == (digest(keys, recs), n)
    keys, recs = f2o_table(root + 1)
    with pytest.raises(GMError) as e:
        ctx.import_table(keys, recs, root + 1)
    assert e.value.code == E_CAP and "1024 or more tiers below the root" in str(e.value)
    with pytest.raises(GMError) as e:
        ctx.export()
    assert e.value.code == E_STATE
    # without pile -1 the same root's keys end 1,023 tiers below it: they import
    assert ctx.import_table(keys[:-1], recs[:-1], root + 1) == (len(keys) - 1, f2o_record(root + 1))


@pytest.mark.parametrize("engine", F2O_ENGINES)
def test_f2o_root_3000_and_its_replay(f2o_ctx, oracle, engine):
    """3,002 tiers; on the sparse engine the second solve is a replay of all of them as one graph."""
    root = 3000
    ctx = _f2o(f2o_ctx, engine)
    for i in range(2):
        n, rec = ctx.solve(root)
        assert (n, rec) == (root + 2, f2o_record(root)), i
        _f2o_check_export(ctx, root, oracle if i == 0 else None)
        if engine == "sparse":
            assert (ctx.stats()["forward_ms"] == 0) == (i == 1), i
    v = ctx.verify()[0]
    assert (v["n_bad"], v["root_ok"], v["checked"]) == (0, 1, n)
    assert ctx.tier_counts().tolist() == [1] * n
    # LOSS in 1000 is pile 1500; no LOSS has an odd remoteness
    cnt, keys, recs = ctx.select(_lib.SEL_LOSS, 1000, 1001)
    assert (cnt, keys, recs.tolist()) == (1, [1500], [LOSS << 14 | 1000])
    # gm_reach over more plies than the 1,024 the first call has room for.  Both sides playing the
    # first of their best moves walk the principal variation: LOSS in 2,000, so 2,001 plies of
    # one position.  Every move: ply d first reaches the piles root - 2d .. root - d on side
    # d & 1, until every (position, side) is marked.  Both as the host reference over the closed
    # form says.
    keys, recs = f2o_table(root)
    table = dict(zip(keys.tolist(), recs.tolist()))
    want, want_plies, _ = reach.reference([root], table, _f2o_expand, "first", "first")
    out, plies, _, _, _ = ctx.reach([root], _lib.REACH_FIRST, _lib.REACH_FIRST)
    assert out == want and (out["n"], out["plies"], out["missing"]) == (2001, 2001, 0)
    assert plies.tolist() == want_plies == [1] * 2001
    want, want_plies, marks = reach.reference([root], table, _f2o_expand)
    out, plies, rk, rr, sides = ctx.reach([root], cap=n)
    assert out == want and out["n"] == n and out["plies"] > 1024
    assert plies.tolist() == want_plies and plies[:3].tolist() == [1, 2, 3]
    assert np.array_equal(rk, keys) and np.array_equal(rr, recs) and sides.tolist() == [marks[k] for k in keys.tolist()]


@pytest.mark.parametrize("engine", F2O_ENGINES)
def test_f2o_root_7000_census_past_the_lds_bins(f2o_ctx, engine):
    """7,002 tiers, so 7,003 bins per value: more than the 4,096 that fit the census kernel's
    LDS, which takes res_hist_kernel to its global bins (csrc/hist_common.hpp score_bin_add).
    A LOSS at every even remoteness (two at 0), two WINs at every odd one (the root alone at the
    last)."""
    root = 7000
    ctx = _f2o(f2o_ctx, engine)
    n, rec = ctx.solve(root)
    assert (n, rec) == (root + 2, f2o_record(root))
    h, want = ctx.histogram(), f2o_histogram(root)
    assert want.shape == (3, 4668) and want[0, 1::2].tolist() == [2] * 2333 + [1] and want[1, 0] == 2
    assert want[1, 2::2].tolist() == [1] * 2333 and not want[2].any() and not want[0, ::2].any()
    assert h.shape == want.shape and np.array_equal(h, want)
    _f2o_check_export(ctx, root)


def _refused(call):
    with pytest.raises(GMError) as e:
        call()
    return e.value.code, str(e.value)


# The deep solve was measured on an MI355X at 4.0 s on the sparse engine (7.9 s more for the
# refused root, which is found out only after the whole backward pass) and, with 2 virtual ranks,
# at 22.1 s on the sharded engine (59.3 s for the refused root): over the 20 s above which the
# sharded engine is to stop at root 7,000.  So the limit is pinned on the one-GPU sparse engine
# alone, as a slow test (13 s), and the score_overflows checks of csrc/dist_sparse.hip's retro
# kernels and the sharded solve's GM_E_CAP path stay unexercised at 0x3FFE / 0x3FFF.
DEEP_ENGINES = [pytest.param("sparse", marks=pytest.mark.slow)]


@pytest.mark.parametrize("engine", DEEP_ENGINES)
def test_f2o_the_14_bit_limit(f2o_own, oracle, engine):
    """Root 24,575 is WIN in 0x3FFF, the deepest that solves (24,573 below it is LOSS in 0x3FFE).
    Root 24,576 would be LOSS in 0x4000: its children are both WIN in 0x3FFF, which
    score_overflows flags -- GM_E_CAP, and the context then holds no table.  The next solve on
    the context works as ever.  (No second solve of a deep root: a replay graph of some 74,000
    kernel nodes is not what this test is for.)"""
    ctx = _f2o(f2o_own, engine)
    n, rec = ctx.solve(F2O_DEEPEST)
    assert (n, rec) == (24577, 0x3FFF) and ctx.stats()["engine"] == _lib.ENGINE_SPARSE
    keys, recs = _f2o_check_export(ctx, F2O_DEEPEST, oracle)
    assert ctx.query([24573, 24574, 24575, 24576]).tolist() == [LOSS << 14 | 0x3FFE, 0x3FFF, 0x3FFF, UNSOLVED]
    assert ctx.digest() == (digest(keys, recs), n)
    code, msg = _refused(lambda: ctx.solve(F2O_FIRST_REFUSED))
    assert code == E_CAP and "remoteness exceeds 14 bits" in msg
    for call in (ctx.export, lambda: ctx.query([0]), ctx.histogram):
        assert _refused(call)[0] == E_STATE
    gk, gr = golden("four_to_one_six")
    assert ctx.solve(6) == (len(gk), int(gr[np.searchsorted(gk, 6)]))
    k, r = ctx.export()
    assert np.array_equal(k, gk) and np.array_equal(r, gr)
