"""gm_moves on the device: every move of a batch of positions valued in one call
(csrc/moves_common.hpp), for every engine and every way a context holds a solve, and what is
built on it: Context.moves_batch, Solver.annotate and --moves.

Expected values come from golden / C-oracle tables, from tests/loopy_ref.py and from the host
twin of the parent commit (Context.expand, Context.moves, Context.query), never from gm_moves
itself.
"""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden, load_plugin

pytestmark = pytest.mark.gpu

from gamesmanmpi_amd import Context, Solver, _lib, moves  # noqa: E402
from gamesmanmpi_amd.solver import best_move  # noqa: E402

F2O, TTT, TOOT, OTH, SUB = 1, 2, 3, 4, 5
NONE = 0xFFFF


def _solve(game, params=(), root=None, engine=None, **opts):
    ctx = Context(game, params, device=0)
    if engine is not None:
        ctx.set_option(_lib.OPT_ENGINE, engine)
    for k, v in opts.items():
        ctx.set_option(getattr(_lib, "OPT_" + k.upper()), v)
    ctx.solve(ctx.initial() if root is None else root)
    return ctx


def _lookup(keys, recs, ask):
    """The table's record of every asked key (0xFFFF where the table does not hold it)."""
    keys, ask = np.asarray(keys, dtype=np.uint64), np.asarray(ask, dtype=np.uint64)
    order = np.argsort(keys, kind="stable")
    keys, recs = keys[order], np.asarray(recs, dtype=np.uint16)[order]
    at = np.minimum(np.searchsorted(keys, ask), len(keys) - 1)
    return np.where(keys[at] == ask, recs[at], np.uint16(NONE)).astype(np.uint16)


def _sample(n, small):
    return np.arange(n) if small else np.unique(np.linspace(0, n - 1, 512).astype(np.int64))


def _check_structure(heads, ck, cr):
    """first is the running sum of count; best / n_best are the argmax / count of moves.rank per
    segment, first of equals."""
    counts = heads["count"].astype(np.uint64)
    assert np.array_equal(heads["first"], np.cumsum(counts) - counts)
    assert len(ck) == len(cr) == int(counts.sum())
    best, n_best = moves.best_of(cr, counts)
    assert np.array_equal(heads["best"], best) and np.array_equal(heads["n_best"], n_best)


def _check(ctx, keys, recs, ask=None):
    """The shared checker: gm_moves of `ask` (default: every key of the table) against the
    expected (keys, records) table and, on a sample, against the host twin."""
    ask = np.asarray(keys if ask is None else ask, dtype=np.uint64)
    heads, ck, cr = ctx.moves_batch(ask)
    print("keys %d children %d" % (len(ask), len(ck)))
    want = _lookup(keys, recs, ask)
    assert np.array_equal(heads["record"], want)
    assert (heads["count"][want == NONE] == 0).all() and (heads["best"][heads["count"] == 0] == -1).all()
    _check_structure(heads, ck, cr)
    assert np.array_equal(cr, _lookup(keys, recs, ck))
    for i in _sample(len(ask), len(keys) < 10000):
        h, k = heads[i], int(ask[i])
        a, n = int(h["first"]), int(h["count"])
        if int(h["record"]) == NONE:
            continue
        prim, kids, _ = ctx.expand(k)
        assert ck[a:a + n].tolist() == (kids if prim == 4 else []), hex(k)
        mk, mr, mb = ctx.moves(k)
        assert (ck[a:a + n].tolist(), cr[a:a + n].tolist(), int(h["best"]) if n else None) == (mk, mr.tolist(), mb), hex(k)
    return heads, ck, cr


# ---------------------------------------------------------------- small games
@pytest.mark.parametrize("engine", [_lib.ENGINE_DENSE, _lib.ENGINE_SPARSE])
def test_ttt(engine):
    keys, recs = golden("ttt")
    ctx = _solve(TTT, engine=engine)
    heads, ck, cr = _check(ctx, keys, recs)
    root = int(np.flatnonzero(keys == ctx.initial())[0])
    assert [int(heads[root][f]) for f in ("count", "best", "record", "n_best")] == [9, 0, 0x8009, 9]
    # an invalid key, a valid key no solve reaches (two X, no O), one key twice
    assert int(ctx.query([4])[0]) == NONE and ctx.expand(4)[0] == 4
    ask = np.array([19683, 4, ctx.initial(), 1 << 40, ctx.initial()], dtype=np.uint64)
    h, k, r = _check(ctx, keys, recs, ask)
    assert h["record"].tolist() == [NONE, NONE, 0x8009, NONE, 0x8009] and h["count"].tolist() == [0, 0, 9, 0, 9]
    assert h["first"].tolist() == [0, 0, 0, 9, 9] and k[:9].tolist() == k[9:].tolist() == ctx.expand(ctx.initial())[1]
    ctx.close()


def test_four_to_one_root_6():
    ctx = _solve(F2O, root=6)
    _check(ctx, *golden("four_to_one_six"))
    ctx.close()


# ---------------------------------------------------------------- reordered moves, passes, orbits, virtual ranks
@pytest.mark.parametrize("ranks", [1, 4])
@pytest.mark.parametrize("sym", [1, 0])
def test_othello_4x4(sym, ranks):
    keys, recs = golden("othello_4x4")
    ctx = _solve(OTH, (4, 4), symmetry=sym, virtual_ranks=ranks)
    heads, ck, cr = _check(ctx, keys, recs)
    # pass children (key + 1) are among them, and children that are not their orbit's representative
    one = heads["count"] == 1
    assert (ck[heads["first"][one].astype(np.int64)] == keys[one] + np.uint64(1)).any()
    ctx.close()


def test_othello_4x4_across_chunks(monkeypatch):
    keys, recs = golden("othello_4x4")
    ctx = _solve(OTH, (4, 4))
    whole = ctx.moves_batch(keys)
    monkeypatch.setenv("GM_MOVES_CHUNK", "1000")
    heads, ck, cr = _check(ctx, keys, recs)
    for a, b in zip(whole, (heads, ck, cr)):
        assert np.array_equal(a, b)
    # too small by one over 55 chunks: GM_E_CAP, heads and the total set, the child arrays untouched
    total = ctypes.c_uint64()
    kb, rb = np.full(len(ck), 7, dtype=np.uint64), np.full(len(ck), 7, dtype=np.uint16)
    h2 = np.zeros(len(keys), dtype=_lib.moves_dtype())
    rc = ctx.L.gm_moves(ctx.h, keys.ctypes.data, len(keys), h2.ctypes.data, kb.ctypes.data, rb.ctypes.data, len(ck) - 1,
                        ctypes.byref(total))
    assert rc == -8 and total.value == len(ck) and (kb == 7).all() and (rb == 7).all() and np.array_equal(h2, heads)
    ctx.close()


@pytest.mark.parametrize("sym", [1, 0])
def test_toot_4x3(sym):
    ctx = _solve(TOOT, (4, 3), symmetry=sym)
    _check(ctx, *golden("toot_4x3"))
    ctx.close()


def test_toot_4x4_vs_oracle(oracle):
    ctx = _solve(TOOT, (4, 4), symmetry=1)
    _check(ctx, *oracle.solve(TOOT, (4, 4)))
    ctx.close()


# ---------------------------------------------------------------- 128-bit keys
@pytest.mark.parametrize("ranks", [1, 8])
def test_othello_8x8_endgame_10(ranks):
    """The golden keys of this table are hashes, not ABI keys: the keys come from export(), the
    records from query(), the children from expand()."""
    s = Solver(load_plugin("tests/plugins/othello8_endgame.py"), device=0)
    assert s.ctx.words == 3
    if ranks > 1:
        s.ctx.set_option(_lib.OPT_VIRTUAL_RANKS, ranks)
    s.solve()
    keys, _ = s.ctx.export()
    assert keys.shape == (56552, 3)
    heads, ck, cr = s.ctx.moves_batch(keys)
    assert ck.shape == (len(cr), 3)
    assert np.array_equal(heads["record"], s.ctx.query(keys))
    _check_structure(heads, ck, cr)
    assert np.array_equal(cr, s.ctx.query(ck))
    for i in _sample(len(keys), False):
        k, h = _lib.words_to_int(keys[i]), heads[i]
        a, n = int(h["first"]), int(h["count"])
        prim, kids, _ = s.ctx.expand(k)
        assert [_lib.words_to_int(w) for w in ck[a:a + n]] == (kids if prim == 4 else [])
    root = _lib.int_to_words(s.root_key, 3)
    at = int(np.flatnonzero((keys == np.array(root, dtype=np.uint64)).all(axis=1))[0])
    assert int(heads[at]["record"]) == (1 << 14 | 11) and int(heads[at]["count"]) == len(s.ctx.expand(s.root_key)[1])
    # a key that is no position (a centre square empty) among valid ones
    bad = np.zeros((1, 3), dtype=np.uint64)
    h, k, r = s.ctx.moves_batch(np.concatenate([keys[at:at + 1], bad, keys[at:at + 1]]))
    assert h["record"].tolist() == [0x400B, NONE, 0x400B] and h["count"][1] == 0 and h["best"][1] == -1
    assert np.array_equal(k[:len(k) // 2], k[len(k) // 2:])
    s.close()


# ---------------------------------------------------------------- block engine
@pytest.mark.parametrize("interleave", [1, 6, 10])
@pytest.mark.parametrize("heaps", [3, 5])
def test_subtract_block_engine(oracle, heaps, interleave):
    recs = oracle.subtract_dense(heaps)
    ctx = _solve(SUB, (heaps,), sub_interleave=interleave)
    keys = np.arange(len(recs), dtype=np.uint64)
    _check(ctx, keys, recs)
    h, k, r = ctx.moves_batch([len(recs), 0, 1 << 63])                   # past the table: no record
    assert h["record"].tolist() == [NONE, 0x4000, NONE] and h["count"].tolist() == [0, 0, 0] and len(k) == 0
    ctx.close()


# ---------------------------------------------------------------- box engine, 8 heaps
def _region(table, root, heaps):
    dims = [((root >> (4 * j)) & 15) + 1 for j in range(heaps)]
    part = table[tuple(slice(0, d) for d in reversed(dims))]
    idx = np.indices(part.shape)
    keys = sum(idx[a].astype(np.uint64) << np.uint64(4 * (heaps - 1 - a)) for a in range(heaps))
    return keys.ravel(), part.ravel()


def _outside(root):
    """Keys outside the root's region: one heap above the root's, and past 32 bits."""
    out = [1 << 32, (1 << 32) | 1]
    for j in range(8):
        if (root >> (4 * j)) & 15 < 15:
            out.append((root & ~(15 << (4 * j))) | ((((root >> (4 * j)) & 15) + 1) << (4 * j)))
    return out


def _check_box(ctx, keys, recs, root, step=1):
    order = np.argsort(keys)
    keys, recs = keys[order], recs[order]
    ask = np.concatenate([keys[::step], np.array(_outside(root), dtype=np.uint64), keys[:3]])
    heads, ck, cr = _check(ctx, keys, recs, ask)
    n_out = len(_outside(root))
    tail = heads[len(keys[::step]):len(keys[::step]) + n_out]
    assert (tail["record"] == NONE).all() and (tail["count"] == 0).all() and (tail["best"] == -1).all()


@pytest.mark.parametrize("root", [0x00000003, 0x000F0FFF, 0x12345678])
def test_box_engine_custom_roots(oracle, root):
    ctx = _solve(SUB, (8,), root=root)
    assert ctx.stats()["engine"] == _lib.ENGINE_DENSE
    if root < 16 ** 5:
        keys, recs = _region(oracle.subtract_dense(5).reshape((16,) * 5), root, 5)
    else:
        keys, recs = oracle.solve(SUB, (8,), root)
    _check_box(ctx, keys, recs, root)
    ctx.close()


@pytest.fixture(scope="module")
def root_3355(oracle):
    return oracle.solve(SUB, (8,), root=0x33557777)


@pytest.mark.parametrize("opts", [{}, {"virtual_ranks": 2}, {"virtual_ranks": 8},
                                  {"sub_interleave": 10, "virtual_ranks": 4}],
                         ids=["one", "split2", "split8", "dist_sub4"])
def test_box_engine_split_and_dist_sub(root_3355, opts):
    """2.36 M positions with 14 children each: every fifth key is asked (a stride that is odd,
    so every box and every owner is met), all their children are checked."""
    ctx = _solve(SUB, (8,), root=0x33557777, **opts)
    assert ctx.stats()["engine"] == (_lib.ENGINE_DIST_DENSE if opts else _lib.ENGINE_DENSE)
    _check_box(ctx, *root_3355, 0x33557777, step=5)
    ctx.close()


def test_full_2_32():
    ctx = _solve(SUB, (8,))
    rng = np.random.default_rng(20261020)
    ask = np.concatenate([rng.integers(0, 1 << 32, 65536, dtype=np.uint64), np.array([0, 0xFFFFFFFF], dtype=np.uint64)])
    heads, ck, cr = ctx.moves_batch(ask)
    assert np.array_equal(heads["record"], ctx.query(ask)) and (heads["record"] != NONE).all()
    _check_structure(heads, ck, cr)
    assert np.array_equal(cr, ctx.query(ck))
    nib = (ask[:, None] >> (np.arange(8, dtype=np.uint64) * np.uint64(4))) & np.uint64(15)
    assert np.array_equal(heads["count"], ((nib >= 1).sum(axis=1) + (nib >= 2).sum(axis=1)))
    assert heads[-2]["count"] == 0 and heads[-2]["record"] == 0x4000 and heads[-1]["count"] == 16
    # the parent-of-best rule: a position's record is the one its best child implies
    has = heads["count"] > 0
    b = cr[(heads["first"][has] + heads["best"][has].astype(np.uint64)).astype(np.int64)].astype(np.uint32)
    implied = np.where(b >> 14 == 1, (b & 0x3FFF) + 1, (1 << 14) | ((b & 0x3FFF) + 1))
    assert np.array_equal(heads["record"][has], implied.astype(np.uint16))
    for i in (0, 1, 65535, 65537):
        a, n = int(heads[i]["first"]), int(heads[i]["count"])
        assert ck[a:a + n].tolist() == ctx.expand(int(ask[i]))[1]
    ctx.close()


# ---------------------------------------------------------------- graph engine
def _check_graph(ctx, prim, off, kids, recs, extra=()):
    n = len(prim)
    ask = np.concatenate([np.arange(n, dtype=np.uint64), np.array(list(extra), dtype=np.uint64)])
    heads, ck, cr = ctx.moves_batch(ask)
    want = np.concatenate([np.asarray(recs, dtype=np.uint16), np.full(len(extra), NONE, dtype=np.uint16)])
    assert np.array_equal(heads["record"], want)
    deg = (off[1:] - off[:-1]).astype(np.uint64)
    deg[np.asarray(prim) != 4] = 0
    assert np.array_equal(heads["count"], np.concatenate([deg, np.zeros(len(extra), dtype=np.uint64)]))
    _check_structure(heads, ck, cr)
    seg = moves.segments(heads)
    edge = off[:-1].astype(np.int64)[seg] + (np.arange(len(ck)) - heads["first"].astype(np.int64)[seg])
    assert np.array_equal(ck, np.asarray(kids, dtype=np.uint64)[edge])
    assert np.array_equal(cr, np.asarray(recs, dtype=np.uint16)[ck.astype(np.int64)])
    return heads, ck, cr


def test_graph_chain():
    n = 5000
    prim = np.full(n, 4, dtype=np.uint8)
    prim[-1] = 1
    off = np.minimum(np.arange(n + 1), n - 1).astype(np.uint64)
    kids = np.arange(1, n, dtype=np.uint32)
    ctx = Context(_lib.GAME_GRAPH, (), device=0)
    ctx.solve_graph(prim, off, kids)
    rem = (n - 1 - np.arange(n)).astype(np.uint16)
    recs = np.where(np.arange(n) % 2 == 1, (1 << 14) | rem, rem).astype(np.uint16)
    heads, ck, cr = _check_graph(ctx, prim, off, kids, recs, extra=(n, n + 7, 1 << 40))
    assert heads["count"].max() == 1 and np.array_equal(ck, np.arange(1, n, dtype=np.uint64))
    ctx.close()


def test_graph_plugin_nim3():
    """No golden table for this plugin: the graph engine's export is pinned to the canonical
    oracle by tests/test_graph.py; the children are the CSR's of the host walk."""
    from gamesmanmpi_amd.graph import enumerate_graph
    mod = load_plugin("tests/plugins/nim3.py")
    positions, prim, off, kids = enumerate_graph(mod, mod.initial_position(), workers=1)
    ctx = Context(_lib.GAME_GRAPH, (), device=0)
    ctx.solve_graph(prim, off, kids)
    keys, recs = ctx.export()
    assert np.array_equal(keys, np.arange(len(positions), dtype=np.uint64))
    heads, ck, cr = _check_graph(ctx, prim, off, kids, recs, extra=(len(positions),))
    assert heads["count"].max() > 1
    for i in _sample(len(positions), False):                             # the choice is the one Context.query implies
        a, n = int(heads[i]["first"]), int(heads[i]["count"])
        if n:
            assert int(heads[i]["best"]) == best_move(ctx.query(kids[int(off[i]):int(off[i + 1])]))[0]
    ctx.close()


def test_graph_loopy_shuttle():
    import loopy_ref
    from gamesmanmpi_amd.graph import enumerate_graph
    mod = load_plugin("tests/plugins/shuttle.py")
    positions, prim, off, kids = enumerate_graph(mod, mod.initial_position(), workers=1)
    recs = loopy_ref.solve_loopy(prim, off, kids)
    ctx = Context(_lib.GAME_GRAPH, (), device=0)
    ctx.set_option(_lib.OPT_LOOPY, 1)
    ctx.solve_graph(prim, off, kids)
    heads, ck, cr = _check_graph(ctx, prim, off, kids, recs)
    draws = loss_child = 0
    for h in heads:
        a, n = int(h["first"]), int(h["count"])
        if not n:
            continue
        best = int(cr[a + int(h["best"])])
        if int(h["record"]) == 0xC000:                                   # a DRAW parent's best child is DRAW
            assert best == 0xC000
            draws += 1
        if ((cr[a:a + n] >> 14) == 1).any():                             # a LOSS child is never passed over for a DRAW
            assert best >> 14 == 1 and best != 0xC000
            loss_child += (cr[a:a + n] == 0xC000).any()
    assert draws > 0 and loss_child > 0
    ctx.close()


# ---------------------------------------------------------------- the call's contract
def _raw(ctx, keys, cap, with_words=True, with_recs=True, fill=7):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    heads = np.zeros(len(keys), dtype=_lib.moves_dtype())
    kb, rb = np.full(max(cap, 1), fill, dtype=np.uint64), np.full(max(cap, 1), fill, dtype=np.uint16)
    total = ctypes.c_uint64(77)
    rc = ctx.L.gm_moves(ctx.h, keys.ctypes.data if len(keys) else None, len(keys), heads.ctypes.data if len(keys) else None,
                        kb.ctypes.data if with_words else None, rb.ctypes.data if with_recs else None, cap,
                        ctypes.byref(total))
    return rc, total.value, heads, kb, rb


@pytest.mark.parametrize("engine", [_lib.ENGINE_DENSE, _lib.ENGINE_SPARSE])
def test_call_contract(engine):
    keys, recs = golden("ttt")
    ctx = _solve(TTT, engine=engine)
    heads, ck, cr = ctx.moves_batch(keys)
    total = len(ck)
    assert total == sum(len(ctx.expand(int(k))[1]) for k in keys if ctx.expand(int(k))[0] == 4)
    rc, n, h, kb, rb = _raw(ctx, keys, total - 1)                        # too small by one
    assert rc == -8 and n == total and (kb == 7).all() and (rb == 7).all() and np.array_equal(h, heads)
    assert b"gm_moves" in ctx.L.gm_last_error()
    rc, n, h, kb, rb = _raw(ctx, keys, total)
    assert rc == 0 and n == total and np.array_equal(kb, ck) and np.array_equal(rb, cr) and np.array_equal(h, heads)
    rc, n, h, kb, rb = _raw(ctx, keys, total, with_words=False)          # heads only
    assert rc == 0 and n == total and (rb == 7).all() and np.array_equal(h, heads)
    rc, n, h, kb, rb = _raw(ctx, keys, 0)                                # cap 0: heads only
    assert rc == 0 and n == total and (kb == 7).all() and (rb == 7).all() and np.array_equal(h, heads)
    h2, k2, r2 = ctx.moves_batch(keys, children=False)
    assert np.array_equal(h2, heads) and k2 is None and r2 is None
    rc, n, h, kb, rb = _raw(ctx, keys, total + 5, with_recs=False)       # child_records may be NULL
    assert rc == 0 and n == total and np.array_equal(kb[:total], ck) and (kb[total:] == 7).all()
    rc, n, h, kb, rb = _raw(ctx, keys[:0], 4)                            # n == 0
    assert (rc, n) == (0, 0) and (kb == 7).all()
    assert ctx.L.gm_moves(ctx.h, keys.ctypes.data, 3, None, None, None, 0, ctypes.byref(ctypes.c_uint64())) == -1
    assert ctx.L.gm_moves(ctx.h, keys.ctypes.data, 3, heads.ctypes.data, None, None, 0, None) == -1
    h0, k0, r0 = ctx.moves_batch([])
    assert len(h0) == len(k0) == len(r0) == 0
    ctx.close()


def test_second_solve_replaces_the_answer():
    ctx = Context(F2O, (), device=0)
    for root, name in ((6, "four_to_one_six"), (4, "four_to_one_four"), (6, "four_to_one_six")):
        ctx.solve(root)
        keys, recs = golden(name)
        _check(ctx, keys, recs, np.concatenate([keys, np.array([5, 6, 7], dtype=np.uint64)]))
    ctx.close()


@pytest.mark.parametrize("engine", [_lib.ENGINE_DENSE, _lib.ENGINE_SPARSE])
def test_poke_changes_the_children_and_the_choice(engine):
    ctx = _solve(TTT, engine=engine)
    root = ctx.initial()
    kids = ctx.expand(root)[1]
    h, k, r = ctx.moves_batch([root])
    assert (int(h[0]["best"]), int(h[0]["n_best"])) == (0, 9) and r.tolist() == [0x8008] * 9
    ctx.poke(kids[4], 0x4000 | 2)                                        # a LOSS child: the one best move
    h, k, r = ctx.moves_batch([root])
    assert (int(h[0]["best"]), int(h[0]["n_best"])) == (4, 1) and r.tolist() == [0x8008] * 4 + [0x4002] + [0x8008] * 4
    assert h[0]["record"] == 0x8009                                      # the key's own record is what the table holds
    ctx.poke(kids[4], 3)                                                 # WIN in 3: the worst of nine
    h, k, r = ctx.moves_batch([root])
    assert (int(h[0]["best"]), int(h[0]["n_best"])) == (0, 8) and int(r[4]) == 3
    ctx.poke(kids[0], NONE)                                              # removed: listed, 0xFFFF, ranks lowest
    h, k, r = ctx.moves_batch([root, kids[0]])
    assert k[:9].tolist() == kids and int(r[0]) == NONE and (int(h[0]["best"]), int(h[0]["n_best"])) == (1, 7)
    assert (int(h[1]["record"]), int(h[1]["count"]), int(h[1]["best"])) == (NONE, 0, -1)
    assert ctx.moves(root)[2] == 1 and ctx.moves(root)[1].tolist() == r[:9].tolist()
    ctx.close()


def test_poke_in_a_byte_table():
    ctx = _solve(SUB, (8,), root=0x00000333)
    key = 0x123
    kids = ctx.expand(key)[1]
    h, k, r = ctx.moves_batch([key])
    assert k.tolist() == kids and np.array_equal(r, ctx.query(kids))
    ctx.poke(kids[1], 0x4000 | 1)                                        # LOSS in 1: nothing is shorter
    h2, k2, r2 = ctx.moves_batch([key])
    assert int(r2[1]) == 0x4001 and (int(h2[0]["best"]), int(h2[0]["n_best"])) == best_of_list(r2.tolist())
    ctx.poke(kids[1], NONE)
    h3, k3, r3 = ctx.moves_batch([key])
    assert int(r3[1]) == NONE and k3.tolist() == kids and int(h3[0]["best"]) == best_move(r3)[0] != 1
    ctx.close()


def best_of_list(recs):
    b = best_move(recs)[0]
    return b, sum(moves.rank([x])[0] == moves.rank([recs[b]])[0] for x in recs)


def test_import_then_moves():
    keys, recs = golden("othello_4x4")
    ctx = Context(OTH, (4, 4), device=0)
    ctx.import_table(keys, recs, ctx.initial())
    _check(ctx, keys, recs)
    ctx.close()


# ---------------------------------------------------------------- processes
def test_two_processes_are_refused():
    import socket
    from moves_ranks import rank_main
    from mp_ranks import run_ranks
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    res = run_ranks(rank_main, 2, (OTH, (4, 4), {"sparse_transport": 1}), timeout=240)
    assert sum(r["m"] for r in res) == 54089
    for r in res:
        assert r["rc"] == -5 and "gm_moves needs the whole table in one context" in r["message"]


# ---------------------------------------------------------------- Solver.annotate
def _same(a, b):
    """Rows of moves() / annotate(), compared through repr (positions may be numpy boards)."""
    return repr(a) == repr(b)


def test_annotate_mttt_principal_variation():
    s = Solver(load_plugin("test_games/mttt.py"), device=0)
    s.solve()
    positions = [p for _, p, _, _ in s.line()]
    assert len(positions) == 10
    got = s.annotate(positions)
    assert _same(got, [s.moves(p) for p in positions])
    assert got[-1] == ([], None) and len(got[0][0]) == 9 and got[0][1] == got[0][0][0]
    s.close()


def test_annotate_othello_4x4_found_rows():
    s = Solver(load_plugin("test_games/othello_bit_new.py", length=4, height=4, area=16), device=0)
    s.solve()
    n, rows = s.find("win:3", cap=64)
    positions = [p for p, _, _ in rows]
    assert len(positions) == min(n, 64) > 8
    got = s.annotate(positions)
    assert _same(got, [s.moves(p) for p in positions])
    assert all(best is not None and best[2:] == (1, 2) for _, best in got)   # WIN in 3: the choice is a LOSS in 2
    s.close()


def test_annotate_graph_contexts():
    s = Solver(load_plugin("tests/plugins/ttt_symmetric.py"), device=0, graph=True)
    s.solve()
    positions = [p for _, p, _, _ in s.line()]
    assert _same(s.annotate(positions), [s.moves(p) for p in positions])
    s.close()


# ---------------------------------------------------------------- command lines
TTT_NP = os.path.join(REPO, "test_games/tic_tac_toe_np.py")


def _check_find_with_moves(text, head):
    assert text.startswith(head + "Found 122 positions: win:5\n  array(")
    lines = text[len(head):].splitlines()[1:]
    starts = [i for i, ln in enumerate(lines) if re.match(r"  array\(", ln)]
    assert len(starts) == 3
    for a, b in zip(starts, starts[1:] + [len(lines)]):
        block = lines[a:b]
        row_end = next(i for i, ln in enumerate(block) if ln.endswith(": WIN in 5"))
        mv = block[row_end + 1:]
        assert mv and all(ln.startswith("    ") for ln in mv)
        ends = [ln for ln in mv if re.search(r": (WIN|LOSS|TIE) in \d+( \*)?$", ln)]
        assert len(ends) == len([ln for ln in mv if re.match(r"    \S.* -> array\(", ln)]) >= 1
        stars = [ln for ln in ends if ln.endswith(" *")]
        assert stars and all(re.search(r": LOSS in 4 \*$", ln) for ln in stars)   # WIN in 5: a LOSS in 4 child


def test_launcher_moves():
    import solver_launcher
    parse = solver_launcher.build_parser().parse_args
    plain = io.StringIO()
    assert solver_launcher.run(parse([TTT_NP]), out=plain) == 0
    assert plain.getvalue() == "TIE in 9 moves\n"                        # without the flag: as before
    out = io.StringIO()
    assert solver_launcher.run(parse([TTT_NP, "--moves"]), out=out) == 0
    text = out.getvalue()
    assert text.startswith("TIE in 9 moves\nMoves:\n  ")
    assert len(re.findall(r": TIE in 8 \*$", text, flags=re.M)) == 9 and len(re.findall(r"^  \S.* -> array\(", text, flags=re.M)) == 9
    out = io.StringIO()
    assert solver_launcher.run(parse([TTT_NP, "--analysis", "--verify", "--moves"]), out=out) == 0
    tail = out.getvalue()
    assert tail.index("Verified 5478 positions: consistent\n") < tail.index("Moves:\n") and tail.endswith(": TIE in 8 *\n")
    out = io.StringIO()
    assert solver_launcher.run(parse([TTT_NP, "--find", "win:5", "--find-cap", "3", "--moves"]), out=out) == 0
    assert "Moves:" not in out.getvalue()
    _check_find_with_moves(out.getvalue(), "TIE in 9 moves\n")


def test_solve_local_moves(capsys):
    import solve_local
    solve_local.main([TTT_NP])
    assert capsys.readouterr().out == "Tie\n"
    assert solve_local.main([TTT_NP, "--moves"]) == 0
    text = capsys.readouterr().out
    assert text.startswith("Tie\nMoves:\n  ") and len(re.findall(r": TIE in 8 \*$", text, flags=re.M)) == 9
    assert solve_local.main([TTT_NP, "--find", "win:5", "--find-cap", "3", "--moves"]) == 0
    _check_find_with_moves(capsys.readouterr().out, "Tie\n")
