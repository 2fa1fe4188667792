"""The two forms of the key-carrying calls of include/gmsolve.h against each other.

* On a one-word game the *_key forms equal the one-word forms (the header's promise): solve,
  export -- the cap-too-small answer included -- and query, called through the C functions on one
  context, on the sparse engine (tic-tac-toe, the golden table's 5,478 positions) and on the
  block engine (SUBTRACT with 3 heaps, 4,096 positions).
* On a multi-word game the one-word reads refuse a solved context (GM_E_ARG) and leave it as it
  was: the 10-empties 8x8 Othello endgame (tests/plugins/othello8_endgame.py, 56,552 positions)
  still answers gm_query_key for its root, and gm_poke finds the root by its three words.
"""
import ctypes

import numpy as np
import pytest

from conftest import golden, load_plugin
from gamesmanmpi_amd import Context, GMError, Solver, _lib

pytestmark = pytest.mark.gpu

E_ARG, E_CAP, E_KEY = -1, -8, -10


def _solve(fn, h, root):
    n, r = ctypes.c_uint64(), ctypes.c_uint16()
    _lib.check(fn(h, root, ctypes.byref(n), ctypes.byref(r)))
    return n.value, r.value


def _export(fn, h):
    n = ctypes.c_uint64()
    _lib.check(fn(h, None, None, 0, ctypes.byref(n)))
    keys, recs = np.zeros(n.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint16)
    m = ctypes.c_uint64()
    _lib.check(fn(h, keys.ctypes.data, recs.ctypes.data, n.value, ctypes.byref(m)))
    assert m.value == n.value
    # one entry short: GM_E_CAP, the count still set, the arrays untouched
    k2, r2 = np.full(n.value, 7, dtype=np.uint64), np.full(n.value, 7, dtype=np.uint16)
    m = ctypes.c_uint64()
    assert fn(h, k2.ctypes.data, r2.ctypes.data, n.value - 1, ctypes.byref(m)) == E_CAP
    assert m.value == n.value and (k2 == 7).all() and (r2 == 7).all()
    return keys, recs


def _query(fn, h, keys):
    out = np.zeros(len(keys), dtype=np.uint16)
    _lib.check(fn(h, keys.ctypes.data, out.ctypes.data, len(keys)))
    return out


@pytest.mark.parametrize("game,params,option,engine,size", [
    (_lib.GAME_TTT, (), (_lib.OPT_ENGINE, _lib.ENGINE_SPARSE), _lib.ENGINE_SPARSE, 5478),
    (_lib.GAME_SUBTRACT, (3,), (_lib.OPT_SUB_INTERLEAVE, 10), _lib.ENGINE_DENSE, 4096),
])
def test_key_forms_equal_the_one_word_forms(game, params, option, engine, size):
    ctx = Context(game, params, device=0)
    ctx.set_option(*option)
    L, h = ctx.L, ctx.h
    root = ctypes.c_uint64()
    _lib.check(L.gm_pack_initial(h, ctypes.byref(root)))
    word = ctypes.c_uint64()
    _lib.check(L.gm_pack_initial_key(h, ctypes.byref(word)))
    assert word.value == root.value and L.gm_key_words(h) == 1

    one = _solve(L.gm_solve, h, root.value)
    assert one[0] == size and ctx.stats()["engine"] == engine
    k1, r1 = _export(L.gm_export, h)
    assert len(k1) == size and (np.diff(k1.astype(np.int64)) > 0).all()
    if game == _lib.GAME_TTT:
        gk, gr = golden("ttt")
        assert np.array_equal(k1, gk) and np.array_equal(r1, gr)
    # every stored key, and keys the table does not hold
    probe = np.concatenate([k1, np.setdiff1d(np.arange(int(k1.max()) + 40, dtype=np.uint64), k1)[:64],
                            np.array([int(k1.max()) + 1, 1 << 40, (1 << 64) - 1], dtype=np.uint64)])
    q1 = _query(L.gm_query, h, probe)
    assert np.array_equal(q1[:size], r1) and (q1[size:] == _lib.REC_UNSOLVED).all()

    assert _solve(L.gm_solve_key, h, ctypes.byref(word)) == one
    k2, r2 = _export(L.gm_export_key, h)
    assert np.array_equal(k2, k1) and np.array_equal(r2, r1)
    assert np.array_equal(_query(L.gm_query_key, h, probe), q1)
    # and crosswise on the table the *_key solve left
    k3, r3 = _export(L.gm_export, h)
    assert np.array_equal(k3, k1) and np.array_equal(r3, r1)
    assert np.array_equal(_query(L.gm_query, h, probe), q1)
    ctx.close()


def test_solved_wide_context_refuses_the_one_word_reads():
    s = Solver(load_plugin("tests/plugins/othello8_endgame.py"), device=0)
    n, rec = s.solve()
    assert s.ctx.words == 3 and n == 56552 and rec != _lib.REC_UNSOLVED
    L, h = s.ctx.L, s.ctx.h
    m = ctypes.c_uint64(123)
    keys, recs = np.zeros(4, dtype=np.uint64), np.full(4, 7, dtype=np.uint16)
    assert L.gm_export(h, None, None, 0, ctypes.byref(m)) == E_ARG
    assert b"gm_export_key" in L.gm_last_error()
    assert L.gm_export(h, keys.ctypes.data, recs.ctypes.data, 4, ctypes.byref(m)) == E_ARG
    assert L.gm_query(h, keys.ctypes.data, recs.ctypes.data, 1) == E_ARG
    assert b"gm_query_key" in L.gm_last_error()
    assert m.value == 123 and (recs == 7).all()
    # the context is as the solve left it
    root = s.root_key
    assert s.ctx.query([root])[0] == rec
    assert s.ctx.digest()[1] == n
    # gm_poke finds a position by its three words ...
    other = rec ^ 1   # the same value, another remoteness
    s.ctx.poke(root, other)
    assert s.ctx.query([root])[0] == other
    s.ctx.poke(root, rec)
    assert s.ctx.query([root])[0] == rec
    # ... and words that are no position (turn byte 3), or a position the table does not hold, are GM_E_KEY
    for bad in ((root & ~(0xFF << 8)) | (3 << 8), s.ctx.initial()):
        with pytest.raises(GMError) as e:
            s.ctx.poke(bad, rec)
        assert e.value.code == E_KEY
    s.close()
