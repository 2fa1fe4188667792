"""gm_reach on the device: the positions reachable under a move policy (csrc/reach_common.hpp),
for every engine and every way a context holds a solve, and what is built on it: Context.reach,
Solver.strategy and --strategy.

Expected values come from golden / C-oracle tables, from tests/loopy_ref.py and from the host
twins Context.expand / gm_expand_host_key through reach.reference, never from gm_reach itself.
"""
import ctypes
import functools
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, golden, load_plugin

pytestmark = pytest.mark.gpu

from gamesmanmpi_amd import Context, Solver, _lib, reach  # noqa: E402

F2O, TTT, TOOT, OTH, SUB = 1, 2, 3, 4, 5
NONE = 0xFFFF
POLICIES = ("all", "best", "first")
ALL9 = list(itertools.product(POLICIES, POLICIES))
NO_FIRST = [p for p in ALL9 if "first" not in p]
TTT_PLIES = [1, 9, 72, 252, 756, 1260, 1520, 1140, 390, 78]


def _solve(game, params=(), root=None, engine=None, **opts):
    ctx = Context(game, params, device=0)
    if engine is not None:
        ctx.set_option(_lib.OPT_ENGINE, engine)
    for k, v in opts.items():
        ctx.set_option(getattr(_lib, "OPT_" + k.upper()), v)
    ctx.solve(ctx.initial() if root is None else root)
    return ctx


def _ints(keys):
    keys = np.asarray(keys)
    return [_lib.words_to_int(w) for w in keys] if keys.ndim == 2 else [int(k) for k in keys]


class Model:
    """An expected table and the host twin that expands its positions: what reach.reference
    runs over.  Expansions and selections are kept, so every policy pair after the first costs
    one breadth-first search."""

    def __init__(self, keys, recs, expand):
        self.table = dict(zip(_ints(keys), [int(r) for r in recs]))
        self._expand, self._kept, self.memo, self._want = expand, {}, {}, {}

    def expand(self, k):
        if k not in self._kept:
            self._kept[k] = self._expand(k)
        return self._kept[k]

    def want(self, starts, mover, other, max_plies=0, symmetries=None):
        at = (tuple(starts), mover, other, max_plies, symmetries is not None)
        if at not in self._want:
            self._want[at] = reach.reference(starts, self.table, self.expand, mover, other, max_plies, symmetries,
                                             memo=self.memo)
        return self._want[at]


MODELS = {}


def _model(name, make):
    if name not in MODELS:
        MODELS[name] = make()
    return MODELS[name]


def _check(ctx, model, starts, pairs=ALL9, max_plies=0, symmetries=None):
    """The shared checker: out, ply_counts and the full key / record / side list of gm_reach
    against reach.reference, for every policy pair asked."""
    for mover, other in pairs:
        want, plies, marks = model.want(starts, mover, other, max_plies, symmetries)
        out, pcs, keys, recs, sides = ctx.reach(starts, reach.policy(mover), reach.policy(other), max_plies,
                                                cap=len(model.table) + 8)
        print(mover, other, out, pcs.tolist())
        assert out == want, (mover, other)
        assert pcs.tolist() == plies, (mover, other)
        order = sorted(marks)
        assert _ints(keys) == order, (mover, other)
        assert recs.tolist() == [model.table[k] for k in order]
        assert sides.tolist() == [marks[k] for k in order]
    return want, plies, marks


# ---------------------------------------------------------------- small games
@pytest.mark.parametrize("engine", [_lib.ENGINE_DENSE, _lib.ENGINE_SPARSE])
def test_ttt(engine):
    ctx = _solve(TTT, engine=engine)
    assert ctx.stats()["engine"] == engine
    m = _model("ttt", lambda: Model(*golden("ttt"), Context(TTT, ()).expand))
    _check(ctx, m, [ctx.initial()])
    out, pcs, _, _, _ = ctx.reach([ctx.initial()])
    assert out["n"] == 5478 and pcs.tolist() == TTT_PLIES and out["n_mover"] + out["n_other"] == out["n"]
    ctx.close()


def test_four_to_one_root_6():
    ctx = _solve(F2O, root=6)
    m = Model(*golden("four_to_one_six"), ctx.expand)
    want, plies, marks = _check(ctx, m, [6])
    ctx.close()


@pytest.mark.parametrize("engine", [_lib.ENGINE_DENSE, _lib.ENGINE_SPARSE])
def test_starts_of_every_kind_in_one_call(engine):
    """Non-root, repeated, invalid and unheld start keys: n_starts counts the held ones with
    their repeats, the others are skipped."""
    ctx = _solve(TTT, engine=engine)
    m = _model("ttt", lambda: Model(*golden("ttt"), Context(TTT, ()).expand))
    kids = ctx.expand(ctx.initial())[1]
    assert int(ctx.query([4])[0]) == NONE                                # a valid key no solve reaches
    starts = [kids[0], 19683, kids[0], 4, kids[3], 1 << 40]
    want, plies, marks = _check(ctx, m, starts, pairs=[("all", "all"), ("best", "all"), ("first", "best")])
    assert want["n_starts"] == 3 and plies[0] == 2
    out, pcs, keys, _, _ = ctx.reach([19683, 4], cap=4)                  # nothing held: zero counts, no plies
    assert out == dict(n=0, n_mover=0, n_other=0, n_starts=0, edges=0, missing=0, plies=0) and len(pcs) == 0 == len(keys)
    out, pcs, keys, _, _ = ctx.reach([], cap=4)
    assert out["n"] == 0 and out["plies"] == 0 and len(pcs) == 0 == len(keys)
    ctx.close()


# ---------------------------------------------------------------- reordered moves, passes, orbits, virtual ranks
@pytest.mark.parametrize("ranks", [1, 4])
@pytest.mark.parametrize("sym", [1, 0])
def test_othello_4x4(sym, ranks):
    keys, recs = golden("othello_4x4")
    ctx = _solve(OTH, (4, 4), symmetry=sym, virtual_ranks=ranks)
    m = _model("oth4", lambda: Model(keys, recs, Context(OTH, (4, 4)).expand))
    root = ctx.initial()
    # the root is its own image under the group the table is reduced by: ALL and BEST equal
    # the unreduced answer (but for the lookups, made from one member of every orbit); FIRST
    # follows one move, which the reduction does not preserve
    group = _othello_group(4, root)
    assert len(group) == 4
    _check(ctx, m, [root], pairs=ALL9 if not sym else NO_FIRST, symmetries=group if sym else None)
    for pair in NO_FIRST:
        a, b = m.want([root], *pair), m.want([root], *pair, symmetries=group)
        assert a[1:] == b[1:] and dict(a[0], edges=0) == dict(b[0], edges=0) and b[0]["edges"] < a[0]["edges"]
    full = m.want([root], "all", "all")
    assert full[0]["n"] == 54089 == len(keys) and sorted(full[2]) == keys.tolist()
    if sym:
        out = _lib.ReachOut()
        k = np.array([root], dtype=np.uint64)
        for how in (_lib.Reach(2, 0, 0, 0), _lib.Reach(0, 2, 0, 0)):
            rc = ctx.L.gm_reach(ctx.h, ctypes.byref(how), k.ctypes.data, 1, ctypes.byref(out), None, 0, None, None, None, 0)
            assert rc == -1 and b"GM_OPT_SYMMETRY 0" in ctx.L.gm_last_error()
    else:
        # FIRST pins the reordered move walk (the plugin's first best move need not be the first
        # best child in the descriptor's plane order), and pass children (key + 1) are followed
        first = m.want([root], "first", "all")[2]
        assert any(k + 1 in first and m.expand(k)[1] == [k + 1] for k in first)
        # the order matters: some followed position has several best moves
        assert any(len(reach.selected(m.expand(k)[1], [m.table[c] for c in m.expand(k)[1]], 1)) > 1
                   for k in first if m.expand(k)[0] == 4)
    ctx.close()


def _othello_group(L, root):
    """The maps of Othello keys (both planes turned alike, the low 16 bits kept) under the
    elements of the square's symmetry group that fix `root`."""
    A = L * L
    turns = [lambda x, y: (x, y), lambda x, y: (L - 1 - y, x), lambda x, y: (L - 1 - x, L - 1 - y),
             lambda x, y: (y, L - 1 - x), lambda x, y: (y, x), lambda x, y: (L - 1 - y, L - 1 - x),
             lambda x, y: (L - 1 - x, y), lambda x, y: (x, L - 1 - y)]

    def key_map(t):
        perm = [L * t(i % L, i // L)[1] + t(i % L, i // L)[0] for i in range(A)]

        lut = [[sum(((b >> i) & 1) << perm[8 * j + i] for i in range(8) if 8 * j + i < A) for b in range(256)]
               for j in range((A + 7) // 8)]

        def plane(p):
            return sum(lut[j][(p >> (8 * j)) & 255] for j in range(len(lut)))

        @functools.lru_cache(maxsize=None)
        def apply(k):
            m = (1 << A) - 1
            return (k & 0xFFFF) | plane((k >> 16) & m) << 16 | plane((k >> (A + 16)) & m) << (A + 16)
        return apply
    return [f for f in map(key_map, turns) if f(root) == root]


def _toot_mirror(L, H):
    A = L * H

    def plane(p):
        return sum(int(bin((p >> (L * y)) & ((1 << L) - 1))[2:].zfill(L)[::-1], 2) << (L * y) for y in range(H))

    @functools.lru_cache(maxsize=None)
    def mirror(k):
        m = (1 << A) - 1
        return (k & 0xFFFF) | plane((k >> 16) & m) << 16 | plane((k >> (A + 16)) & m) << (A + 16)
    return mirror


@pytest.mark.parametrize("sym", [1, 0])
def test_toot_4x3_across_chunks(sym, monkeypatch):
    """200,127 positions; a chunk of 1,000 entries makes every level of 2,001 entries or more
    cross at least three launches, each of several workgroups."""
    keys, recs = golden("toot_4x3")
    assert len(keys) == 200127
    ctx = _solve(TOOT, (4, 3), symmetry=sym)
    m = _model("toot43", lambda: Model(keys, recs, Context(TOOT, (4, 3)).expand))
    root = ctx.initial()
    whole = ctx.reach([root], 1, 0, cap=len(keys))
    monkeypatch.setenv("GM_REACH_CHUNK", "1000")
    mirror = _toot_mirror(4, 3)
    assert mirror(root) == root
    want, plies, marks = _check(ctx, m, [root], pairs=NO_FIRST if sym else ALL9, symmetries=[mirror] if sym else None)
    assert max(m.want([root], "all", "all")[1]) > 3000
    for pair in NO_FIRST:                                                # the reduced answer is the unreduced one
        a, b = m.want([root], *pair), m.want([root], *pair, symmetries=[mirror])
        assert a[1:] == b[1:] and dict(a[0], edges=0) == dict(b[0], edges=0)
    chunked = ctx.reach([root], 1, 0, cap=len(keys))
    assert whole[0] == chunked[0] and all(np.array_equal(a, b) for a, b in zip(whole[1:], chunked[1:]))
    # a start that is not its own mirror image: with the reduction on the result is closed under the mirror
    start = next(k for k in ctx.expand(root)[1] if mirror(k) != k)
    assert mirror(mirror(start)) == start and mirror(start) in m.table
    _check(ctx, m, [start], pairs=[("all", "all"), ("best", "all")], symmetries=[mirror] if sym else None)
    ctx.close()


def test_after_import_equals_after_solve():
    keys, recs = golden("toot_3x3")
    solved = _solve(TOOT, (3, 3))
    loaded = Context(TOOT, (3, 3), device=0)
    loaded.import_table(keys, recs, loaded.initial())
    m = Model(keys, recs, solved.expand)
    root = solved.initial()
    _check(loaded, m, [root], pairs=NO_FIRST, symmetries=[_toot_mirror(3, 3)])
    for mover, other in NO_FIRST:
        a = solved.reach([root], reach.policy(mover), reach.policy(other), cap=len(keys))
        b = loaded.reach([root], reach.policy(mover), reach.policy(other), cap=len(keys))
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    solved.close()
    loaded.close()


# ---------------------------------------------------------------- 128-bit keys
@pytest.mark.parametrize("ranks", [1, 3])
def test_othello_8x8_endgame_10(ranks):
    """The golden keys of this table are hashes, not ABI keys: the keys come from export(), the
    records from query(), the children from expand()."""
    s = Solver(load_plugin("tests/plugins/othello8_endgame.py"), device=0)
    assert s.ctx.words == 3
    if ranks > 1:
        s.ctx.set_option(_lib.OPT_VIRTUAL_RANKS, ranks)
    s.solve()
    keys, recs = s.ctx.export()
    assert keys.shape == (56552, 3)
    twin = Context(OTH, (8, 8))
    m = _model("oth8", lambda: Model(keys, recs, twin.expand))
    assert m.table == dict(zip(_ints(keys), recs.tolist()))
    want, plies, marks = _check(s.ctx, m, [s.root_key])
    assert m.want([s.root_key], "all", "all")[0]["n"] == 56552
    # a key that is no position (a centre square empty) among the starts
    out, _, _, _, _ = s.ctx.reach(np.concatenate([np.zeros((1, 3), dtype=np.uint64), keys[:1]]), cap=0)
    assert out["n_starts"] == 1
    s.close()


# ---------------------------------------------------------------- byte tables
def _sub_model(oracle, heaps):
    recs = oracle.subtract_dense(heaps)
    return Model(np.arange(len(recs), dtype=np.uint64), recs, Context(SUB, (heaps,)).expand)


@pytest.mark.parametrize("interleave", [1, 6, 10])
@pytest.mark.parametrize("heaps", [3, 4])
def test_subtract_block_engine(oracle, heaps, interleave):
    """Root 0xFFFF: 65,536 positions, 16 to a mark word, written concurrently.  The keys carry
    no turn, so positions are reached at both parities."""
    ctx = _solve(SUB, (heaps,), sub_interleave=interleave)
    m = _model("sub%d" % heaps, lambda: _sub_model(oracle, heaps))
    root = (1 << (4 * heaps)) - 1
    want, plies, marks = _check(ctx, m, [root])
    full = m.want([root], "all", "all")[0]
    assert full["n"] == 16 ** heaps and full["n_mover"] + full["n_other"] - full["n"] > 0
    out, _, _, _, _ = ctx.reach([root, 1 << (4 * heaps), 1 << 63])      # past the table: skipped
    assert out == full
    ctx.close()


@pytest.mark.parametrize("opts", [{}, {"virtual_ranks": 2}, {"sub_interleave": 10, "virtual_ranks": 2}],
                         ids=["box", "split_box2", "dist_sub2"])
def test_box_engine_and_the_split_engines(oracle, opts):
    root = 0x11113333
    ctx = _solve(SUB, (8,), root=root, **opts)
    assert ctx.stats()["engine"] == (_lib.ENGINE_DIST_DENSE if opts else _lib.ENGINE_DENSE)
    m = _model("box", lambda: Model(*oracle.solve(SUB, (8,), root), Context(SUB, (8,)).expand))
    assert len(m.table) == 4096
    want, plies, marks = _check(ctx, m, [root])
    full = m.want([root], "all", "all")[0]
    assert full["n"] == 4096 and full["n_mover"] + full["n_other"] - full["n"] > 0
    # keys outside the root's region are no starts
    out, _, _, _, _ = ctx.reach([root, 0x21113333, 1 << 32])
    assert out == full
    ctx.close()


# ---------------------------------------------------------------- graph engine
def _graph_model(prim, off, kids, recs):
    def expand(i):
        return int(prim[i]), [int(c) for c in kids[int(off[i]):int(off[i + 1])]], 0
    return Model(np.arange(len(prim), dtype=np.uint64), recs, expand)


def test_graph_plugin_nim3():
    """No golden table for this plugin: the graph engine's export is pinned to the canonical
    oracle by tests/test_graph.py; the children are the CSR's of the host walk."""
    from gamesmanmpi_amd.graph import enumerate_graph
    mod = load_plugin("tests/plugins/nim3.py")
    positions, prim, off, kids = enumerate_graph(mod, mod.initial_position(), workers=1)
    ctx = Context(_lib.GAME_GRAPH, (), device=0)
    ctx.solve_graph(prim, off, kids)
    keys, recs = ctx.export()
    m = _graph_model(prim, off, kids, recs)
    want, plies, marks = _check(ctx, m, [0])
    assert m.want([0], "all", "all")[0]["n"] == len(positions)
    _check(ctx, m, [len(positions), 3, 3, 1 << 40], pairs=[("all", "all"), ("best", "first")])
    ctx.close()


def test_graph_loopy_shuttle():
    import loopy_ref
    from gamesmanmpi_amd.graph import enumerate_graph
    mod = load_plugin("tests/plugins/shuttle.py")
    positions, prim, off, kids = enumerate_graph(mod, mod.initial_position(), workers=1)
    recs = loopy_ref.solve_loopy(prim, off, kids)
    assert (np.asarray(recs) == 0xC000).any()
    ctx = Context(_lib.GAME_GRAPH, (), device=0)
    ctx.set_option(_lib.OPT_LOOPY, 1)
    ctx.solve_graph(prim, off, kids)
    m = _graph_model(prim, off, kids, recs)
    _check(ctx, m, [0])                                                  # cycles end at the marks
    full = m.want([0], "all", "all")
    assert full[0]["n"] == len(positions) and full[0]["plies"] <= 2 * len(positions)
    # DRAW ranks between TIE and WIN: a position with DRAW and WIN children and nothing
    # better follows the DRAW ones only, one with a TIE or LOSS child never a DRAW one
    seen = 0
    for i in range(len(prim)):
        if prim[i] != 4:
            continue
        ks = [int(c) for c in kids[int(off[i]):int(off[i + 1])]]
        vals = {int(recs[c]) >> 14 for c in ks}
        if 3 in vals and 0 in vals and not vals & {1, 2}:
            want, plies, marks = _check(ctx, m, [i], pairs=[("best", "all")], max_plies=1)
            assert {k for k in marks if k != i or marks[k] & 2} == {c for c in ks if int(recs[c]) == 0xC000}
            seen += 1
            if seen == 3:
                break
    assert seen
    ctx.close()


# ---------------------------------------------------------------- the call's contract
@pytest.mark.parametrize("engine", [_lib.ENGINE_DENSE, _lib.ENGINE_SPARSE])
def test_poke_removes_a_subtree(engine):
    keys, recs = golden("ttt")
    ctx = _solve(TTT, engine=engine)
    twin = Context(TTT, ())
    root = ctx.initial()
    victim = ctx.expand(ctx.expand(root)[1][4])[1][0]                    # an interior position two plies down
    assert ctx.expand(victim)[0] == 4
    ctx.poke(victim, NONE)
    keep = keys != np.uint64(victim)
    m = Model(keys[keep], recs[keep], twin.expand)
    _check(ctx, m, [root])
    want, plies, marks = m.want([root], "all", "all")
    assert want["missing"] >= 1 and victim not in marks and want["n"] < 5478
    # below its parent the victim's children are reached through the victim alone: not expanded
    parent = ctx.expand(root)[1][4]
    want, plies, marks = _check(ctx, m, [parent], pairs=[("all", "all")])
    assert want["missing"] == 1 and not set(twin.expand(victim)[1]) & set(marks)
    assert ctx.reach([victim])[0]["n"] == 0                              # and it is no start
    ctx.close()


def test_poke_in_a_byte_table(oracle):
    recs = oracle.subtract_dense(3).copy()
    ctx = _solve(SUB, (3,))
    victim = 0x765
    ctx.poke(victim, NONE)
    keep = np.arange(len(recs)) != victim
    m = Model(np.arange(len(recs), dtype=np.uint64)[keep], recs[keep], Context(SUB, (3,)).expand)
    _check(ctx, m, [0xFFF], pairs=[("all", "all"), ("best", "all"), ("first", "first")])
    want, plies, marks = m.want([0xFFF], "all", "all")
    assert want["missing"] >= 1 and victim not in marks
    ctx.close()


@pytest.mark.parametrize("game", ["ttt", "sub3"])
def test_max_plies_3(oracle, game):
    if game == "ttt":
        ctx, root = _solve(TTT, engine=_lib.ENGINE_SPARSE), 0
        m = _model("ttt", lambda: Model(*golden("ttt"), Context(TTT, ()).expand))
        root = ctx.initial()
    else:
        ctx, root = _solve(SUB, (3,)), 0xFFF
        m = _model("sub3", lambda: _sub_model(oracle, 3))
    for pair in (("all", "all"), ("best", "all")):
        whole = m.want([root], *pair)
        want, plies, marks = _check(ctx, m, [root], pairs=[pair], max_plies=3)
        assert plies == whole[1][:4] and want["plies"] == 4
    ctx.close()


def test_cap_and_ply_cap():
    ctx = _solve(TTT, engine=_lib.ENGINE_SPARSE)
    m = _model("ttt", lambda: Model(*golden("ttt"), Context(TTT, ()).expand))
    root = ctx.initial()
    want, plies, marks = m.want([root], "best", "all")
    out, pcs, keys, recs, sides = ctx.reach([root], 1, 0, cap=0)         # counts only
    assert out == want and pcs.tolist() == plies and keys is None and recs is None and sides is None
    out, pcs, keys, recs, sides = ctx.reach([root], 1, 0, cap=0, plies=False)
    assert out == want and pcs is None
    cap = 100
    assert cap < want["n"]
    out, pcs, keys, recs, sides = ctx.reach([root], 1, 0, cap=cap)
    ks = keys.tolist()
    assert out == want and len(ks) == cap == len(set(ks)) and ks == sorted(ks) and set(ks) <= set(marks)
    assert recs.tolist() == [m.table[k] for k in ks] and sides.tolist() == [marks[k] for k in ks]
    # records and sides may each be NULL; a ply buffer too small is GM_E_CAP with out filled
    how, o = _lib.Reach(1, 0, 0, 0), _lib.ReachOut()
    start = np.array([root], dtype=np.uint64)
    kb = np.full(want["n"] + 4, 7, dtype=np.uint64)
    pb = np.full(16, 7, dtype=np.uint64)
    rc = ctx.L.gm_reach(ctx.h, ctypes.byref(how), start.ctypes.data, 1, ctypes.byref(o), pb.ctypes.data, 16,
                        kb.ctypes.data, None, None, len(kb))
    assert rc == 0 and o.as_dict() == want and kb[:want["n"]].tolist() == sorted(marks) and (kb[want["n"]:] == 7).all()
    assert pb.tolist() == plies + [0] * (16 - len(plies))
    o2 = _lib.ReachOut()
    pb = np.full(16, 7, dtype=np.uint64)
    rc = ctx.L.gm_reach(ctx.h, ctypes.byref(how), start.ctypes.data, 1, ctypes.byref(o2), pb.ctypes.data, len(plies) - 1,
                        None, None, None, 0)
    assert rc == -8 and o2.as_dict() == want and b"gm_reach" in ctx.L.gm_last_error()
    # a kept histogram stays kept, and the table is unchanged
    before = ctx.digest()
    hist = ctx.histogram()
    ctx.reach([root], 2, 2)
    assert ctx.digest() == before and np.array_equal(ctx.histogram(), hist)
    ctx.close()


# ---------------------------------------------------------------- processes
def test_two_processes_are_refused():
    import socket
    from mp_ranks import run_ranks
    from reach_ranks import rank_main
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    res = run_ranks(rank_main, 2, (OTH, (4, 4), {"sparse_transport": 1}), timeout=240)
    assert sum(r["m"] for r in res) == 54089
    for r in res:
        assert r["rc"] == -5 and "gm_reach needs the whole table in one context" in r["message"]


# ---------------------------------------------------------------- Solver.strategy and --strategy
TTT_NP = os.path.join(REPO, "test_games/tic_tac_toe_np.py")


def test_strategy_on_tic_tac_toe():
    m = _model("ttt", lambda: Model(*golden("ttt"), Context(TTT, ()).expand))
    s = Solver(load_plugin("test_games/tic_tac_toe_np.py"), device=0)
    s.solve()
    for first in (False, True):
        want, plies, marks = m.want([s.root_key], "first" if first else "best", "all")
        got = s.strategy(first=first)
        assert got["side"] == "mover" and got["value"] == 2                # a tied root: the mover does not lose
        assert got["n"] == want["n"] and got["ply_counts"] == plies and got["share"] == want["n"] / 5478
    other = s.strategy(side="other")
    assert other["n"] == m.want([s.root_key], "all", "best")[0]["n"]
    rows = s.reach(mover="best", cap=20)["positions"]
    assert len(rows) == 20 and all(v is not None and b in (1, 2) for _, v, _, b in rows)
    s.close()
    want, plies, _ = m.want([s.root_key], "best", "all")
    for tool, head in (("solver_launcher.py", "TIE in 9 moves\n"), ("solve_local.py", "Tie\n")):
        plain = subprocess.run([sys.executable, os.path.join(REPO, tool), TTT_NP], capture_output=True, text=True,
                               cwd=REPO, timeout=240)
        assert plain.returncode == 0 and plain.stdout == head               # without the flag: as before
        run = subprocess.run([sys.executable, os.path.join(REPO, tool), TTT_NP, "--strategy"], capture_output=True,
                             text=True, cwd=REPO, timeout=240)
        assert run.returncode == 0, run.stderr
        lines = run.stdout.splitlines()
        assert lines[0] + "\n" == head
        hit = re.fullmatch(r"Strategy for the player to move \(root TIE in 9 moves\): (\d+) of 5478 positions "
                           r"\((\d+\.\d\d)%\), deepest ply (\d+)", lines[1])
        assert hit and int(hit.group(1)) == want["n"] and int(hit.group(3)) == len(plies) - 1
        assert float(hit.group(2)) == round(100.0 * want["n"] / 5478, 2)
        assert lines[2:] == ["  ply %d: %d" % (d, c) for d, c in enumerate(plies)]


def test_strategy_first_on_a_reduced_solve_exits_1():
    oth = os.path.join(REPO, "test_games/othello_bit_new.py")
    run = subprocess.run([sys.executable, os.path.join(REPO, "solve_local.py"), oth, "--dims", "4x4", "--strategy", "first"],
                         capture_output=True, text=True, cwd=REPO, timeout=240)
    assert run.returncode == 1 and "rerun with the reduction off" in run.stderr
