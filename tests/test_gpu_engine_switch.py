"""One context solved by one engine after another: every read after a solve (export, query,
digest, histogram, dense table, rank stats) is answered by the engine of the newest solve,
never from the table an earlier solve left in the context."""
import ctypes

import numpy as np
import pytest

from conftest import digest, golden

from gamesmanmpi_amd import Context, _lib

pytestmark = pytest.mark.gpu

TTT, TOOT, SUB = 2, 3, 5


def _has_dense_table(ctx):
    try:
        ctx.dense_table()
    except _lib.GMError as e:
        assert e.code == -5 and "only the SUBTRACT dense path has a dense table" in str(e)   # GM_E_STATE
        return False
    return True


def test_subtract_box_split_block_sharded_box(oracle):
    """8 heaps, root 0x33557777: the box engine, the box engine split over 2 virtual ranks, the
    block engine, the block engine sharded over 2, the box engine again.  A rank of the split box
    engine has a dense table too (include/gmsolve.h gm_dense_table, "At N > 1"); the sharded
    block engine has none."""
    root = 0x33557777
    ok, orec = oracle.solve(SUB, (8,), root=root)
    want = (digest(ok, orec), len(ok))
    ctx = Context(SUB, (8,), device=0)
    steps = [  # options set before the solve, stats()["engine"], stats()["world"], dense table, ranks reported
        ((), _lib.ENGINE_DENSE, 1, True, 0),
        (((_lib.OPT_VIRTUAL_RANKS, 2),), _lib.ENGINE_DIST_DENSE, 2, True, 2),
        (((_lib.OPT_VIRTUAL_RANKS, 1), (_lib.OPT_SUB_INTERLEAVE, 10)), _lib.ENGINE_DENSE, 1, True, 0),
        (((_lib.OPT_VIRTUAL_RANKS, 2),), _lib.ENGINE_DIST_DENSE, 2, False, 0),
        (((_lib.OPT_VIRTUAL_RANKS, 1), (_lib.OPT_SUB_INTERLEAVE, 20)), _lib.ENGINE_DENSE, 1, True, 0),
    ]
    for opts, engine, world, table, nranks in steps:
        for o, v in opts:
            ctx.set_option(o, v)
        n, rec = ctx.solve(root)
        assert n == len(ok)
        assert ctx.digest() == want
        assert ctx.query([root]).tolist() == [rec]
        assert int(ctx.histogram().sum()) == n
        st = ctx.stats()
        assert (st["engine"], st["world"]) == (engine, world)
        assert _has_dense_table(ctx) == table
        assert len(ctx.rank_stats()) == nranks
    ctx.close()


def test_toot_sparse_sharded_replay_forced():
    """Toot 4x3: the sparse engine, 4 virtual ranks of the sharded one, the sparse engine again
    (a replay of its first solve), the sharded engine forced at one rank."""
    keys, recs = golden("toot_4x3")
    ctx = Context(TOOT, (4, 3), device=0)
    uid = ctypes.create_string_buffer(128)
    _lib.check(_lib.lib().gm_comm_unique_id(uid, 128))
    digests = []
    for step in range(4):
        if step == 1:
            ctx.set_option(_lib.OPT_VIRTUAL_RANKS, 4)
        if step == 2:
            ctx.set_option(_lib.OPT_VIRTUAL_RANKS, 1)
        if step == 3:
            ctx.set_comm(0, 1, uid.raw)
            ctx.set_option(_lib.OPT_ENGINE, _lib.ENGINE_DIST_SPARSE)
        n, rec = ctx.solve(ctx.initial())
        assert n == len(keys)
        k, r = ctx.export()
        assert np.array_equal(k, keys) and np.array_equal(r, recs)
        digests.append(ctx.digest())
        assert int(ctx.histogram().sum()) == n
        assert ctx.stats()["engine"] == (_lib.ENGINE_DIST_SPARSE if step in (1, 3) else _lib.ENGINE_SPARSE)
    assert digests == [(digest(keys, recs), len(keys))] * 4
    ctx.close()


def test_ttt_dense_sparse_dense(oracle):
    """Tic-tac-toe: dense from the empty board, sparse from one of its children, dense again."""
    keys, recs = golden("ttt")
    ctx = Context(TTT, (), device=0)
    child = oracle.expand(TTT, (), ctx.initial())[1][0]
    ck, cr = oracle.solve(TTT, (), root=child)
    assert 0 < len(ck) < len(keys)
    for engine, root, wk, wr in [(_lib.ENGINE_DENSE, ctx.initial(), keys, recs), (_lib.ENGINE_SPARSE, child, ck, cr),
                                 (_lib.ENGINE_DENSE, ctx.initial(), keys, recs)]:
        ctx.set_option(_lib.OPT_ENGINE, engine)
        n, rec = ctx.solve(root)
        assert ctx.stats()["engine"] == engine
        k, r = ctx.export()
        assert n == len(wk)
        assert np.array_equal(k, wk) and np.array_equal(r, wr)
    ctx.close()
