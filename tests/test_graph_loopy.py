"""The loopy solve of gm_solve_graph (GM_OPT_LOOPY, csrc/graph_loopy.hip) against tests/loopy_ref.py.

Cycles and DRAW primitives are solved, not refused: the table is the least fixed point by
levels, what no level decides is DRAW (record 0xC000).  The unmarked tests pin the reference
itself -- to graph_ref on acyclic graphs, to its own local rule on cyclic ones -- and show that
the inputs are not degenerate; the `gpu` tests compare export, root, digest, histogram,
draw count, stats and gm_verify of a device solve with it, each on a context of its own.
"""
import ctypes
import functools
import io
import json
import os

import numpy as np
import pytest

import conftest
import graph_ref
import loopy_ref
import test_graph_random as tgr
from graph_ref import DRAW, LOSS, TIE, UNDECIDED, WIN

from gamesmanmpi_amd import _lib, analysis
from gamesmanmpi_amd.graph import enumerate_graph

gpu = pytest.mark.gpu

SIZES = (2, 63, 64, 65, 255, 256, 257, 4097)
MIXES, SEEDS, LEVELS = tgr.MIXES, tgr.SEEDS, tgr.LEVELS
FRACS = (0.05, 0.5)
REC_DRAW = 0xC000
E_ARG, E_STATE, E_NOMOVES, E_CAP = -1, -5, -7, -8


def rec(value, rem):
    return value << 14 | rem


@functools.lru_cache(maxsize=None)
def rewired(n, mix, seed, frac, draw_leaves):
    g = loopy_ref.rewire(tgr.dag(n, mix, seed), frac, 7000 * n + 10 * seed + draw_leaves, draw_leaves)
    for a in g:
        a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def solved(*key):
    """(records, levels) of rewired(*key) by the reference, computed once."""
    value, rem, levels = loopy_ref.solve_levels(*rewired(*key))
    ref = graph_ref.pack(value, rem)
    ref.setflags(write=False)
    return ref, levels


def cyclic_keys():
    for n in SIZES:
        for mix in MIXES:
            for seed in SEEDS:
                for frac in FRACS:
                    for draw_leaves in (False, True):
                        yield n, mix, seed, frac, draw_leaves


# fixed shapes: name -> (graph, expected records)
_ring = tgr.CYCLES["1000-cycle"]
FIXED = {
    # the root can leave the loop at once: 0 -> {0, 1}, 1 a LOSS leaf
    "self-loop": (tgr.CYCLES["self-loop"], [rec(WIN, 1), rec(LOSS, 0)]),
    "2-cycle": (tgr.CYCLES["2-cycle"], [REC_DRAW, REC_DRAW]),
    # every tenth node of the ring has the LOSS leaf: WIN in 1; the node before it has that WIN
    # node as its only child: LOSS in 2; and so on round the ring, nine nodes back from each exit
    "1000-cycle": (_ring, [rec(WIN, 1) if i % 10 == 0 else rec((10 - i % 10) % 2, 1 + (10 - i % 10))
                           for i in range(1000)] + [rec(LOSS, 0)]),
    "unreachable-cycle": (tgr.CYCLES["unreachable-cycle"], [rec(LOSS, 1), rec(WIN, 0), REC_DRAW, REC_DRAW, REC_DRAW]),
    "draw": (tgr.BAD_NODES["draw"][:3], [REC_DRAW, REC_DRAW]),
    "draw-alone": (tgr.BAD_NODES["draw-alone"][:3], [REC_DRAW]),
    "draw-unreachable": (tgr.BAD_NODES["draw-unreachable"][:3], [rec(WIN, 1), rec(LOSS, 0), REC_DRAW]),
}


def star_with_a_2_cycle():
    """graph_ref.star(100_000) with the first top turned into a 2-cycle with a new node."""
    prim, off, kids = graph_ref.star(100_000)
    top = int(next(k for k in kids[:100_000] if prim[k] == UNDECIDED))
    n, m = len(prim), len(kids)
    lo, hi = int(off[top]), int(off[top + 1])
    assert prim[top] == UNDECIDED and hi - lo == 1   # a chain node: its one edge now goes to the new node
    prim2 = np.concatenate([prim, [UNDECIDED]]).astype(np.uint8)
    kids2 = np.concatenate([kids, [top]]).astype(np.uint32)
    kids2[lo] = n
    off2 = np.concatenate([off, [m + 1]]).astype(np.uint64)
    return prim2, off2, kids2


# ---------------------------------------------------------------- the reference (CPU)
@pytest.mark.parametrize("graph", tgr.SMALL_GRAPHS, ids=tgr.SMALL_IDS)
def test_reference_equals_the_acyclic_one_on_dags(graph):
    assert np.array_equal(loopy_ref.solve_loopy(*graph), graph_ref.solve_reference(*graph))


@pytest.mark.parametrize("n", SIZES)
def test_reference_satisfies_the_local_rule_on_cyclic_graphs(n):
    for key in cyclic_keys():
        if key[0] == n:
            assert loopy_ref.check_rules(*rewired(*key), solved(*key)[0]) == [], key


@pytest.mark.parametrize("name", FIXED)
def test_reference_on_the_fixed_shapes(name):
    graph, want = FIXED[name]
    got = loopy_ref.solve_loopy(*graph)
    assert got.tolist() == want
    assert loopy_ref.check_rules(*graph, got) == []


def test_reference_still_refuses_what_has_no_solution():
    for name in ("no-moves", "code-5"):
        with pytest.raises(graph_ref.GraphError):
            loopy_ref.solve_loopy(*tgr.BAD_NODES[name][:3])


def test_local_rule_flags_a_planted_record_of_each_kind():
    graph = rewired(257, "even", 1, 0.5, True)
    prim, off, kids = graph
    good = solved(257, "even", 1, 0.5, True)[0]
    parents = {int(k): [] for k in range(len(prim))}
    for i in np.flatnonzero(prim == UNDECIDED):
        for k in kids[int(off[i]):int(off[i + 1])]:
            parents[int(k)].append(int(i))

    def planted(node, record):
        bad = good.copy()
        bad[node] = record
        return dict(loopy_ref.check_rules(*graph, bad))
    leaf = int(np.flatnonzero(prim == DRAW)[0])
    assert planted(leaf, rec(LOSS, 0))[leaf] == "bad_primitive"
    draw = int(np.flatnonzero((prim == UNDECIDED) & (good == REC_DRAW))[0])
    assert planted(draw, rec(WIN, 1))[draw] == "bad_value"
    tie = int(np.flatnonzero((prim == UNDECIDED) & (good >> 14 == TIE))[0])
    assert planted(tie, REC_DRAW)[tie] == "bad_value"
    win = int(np.flatnonzero((prim == UNDECIDED) & (good >> 14 == WIN))[0])
    assert planted(win, good[win] + 1)[win] == "bad_value"
    child = next(k for k in range(len(prim)) if parents[k])
    found = planted(child, 0xFFFF)
    assert all(found[p] == "missing_child" for p in parents[child])


def test_inputs_are_not_degenerate():
    """Conditions on the inputs, from the reference alone: all four values on interior nodes
    of one graph, more than 10 % interior DRAW in one, a TIE node with a DRAW child in one, a
    remoteness of 30 or more somewhere."""
    four = tenth = tie_over_draw = False
    deepest = 0
    for key in cyclic_keys():
        prim, off, kids = rewired(*key)
        ref = solved(*key)[0]
        inner = prim == UNDECIDED
        val = ref >> 14
        four |= set(val[inner].tolist()) == {WIN, LOSS, TIE, DRAW}
        tenth |= np.count_nonzero(val[inner] == DRAW) > 0.1 * np.count_nonzero(inner)
        src, dst = graph_ref._interior_edges(*graph_ref._arrays(prim, off, kids))
        tie_over_draw |= bool(np.any((val[src] == TIE) & (val[dst] == DRAW)))
        deepest = max(deepest, int((ref & 0x3FFF).max()))   # a DRAW record's is 0
    assert four and tenth and tie_over_draw and deepest >= 30, (four, tenth, tie_over_draw, deepest)
    # the n = 4097 all-WIN-leaf DAG, half rewired: a long win/loss phase with draws
    ref = solved(4097, "win", 1, 0.5, False)[0]
    assert np.count_nonzero(ref == REC_DRAW) > 100 and int((ref & 0x3FFF).max()) >= 30


def shuttle():
    return conftest.load_plugin("tests/plugins/shuttle.py")


def test_enumerate_graph_returns_the_whole_cyclic_graph(monkeypatch):
    """Serial, and sharded over two worker processes (forced on for so small a graph, as in
    tests/test_graph.py): the walk deduplicates by fingerprint, so a position met again --
    at its own level or above -- is an edge to the node it already is."""
    from gamesmanmpi_amd import graph
    mod = shuttle()
    serial = enumerate_graph(mod, mod.initial_position(), workers=1)
    assert len(serial[0]) == 64 and len(set(serial[0])) == 64 and serial[0][0] == (0, 0)
    monkeypatch.setattr(graph, "PAR_MIN", 4)
    monkeypatch.setattr(graph, "PAR_START", 4)
    pairs = enumerate_graph(mod, mod.initial_position(), workers=2)
    assert pairs[0] == serial[0] and all(np.array_equal(a, b) for a, b in zip(pairs[1:], serial[1:]))
    positions, prim, off, kids = serial
    for i, pos in enumerate(positions):   # every move of every position is an edge, in order
        want = [] if mod.primitive(pos) != UNDECIDED else [mod.do_move(pos, m) for m in mod.gen_moves(pos)]
        assert [positions[k] for k in kids[int(off[i]):int(off[i + 1])]] == want
    with pytest.raises(graph_ref.CycleError):
        graph_ref.solve_reference(prim, off, kids)
    ref = loopy_ref.solve_loopy(prim, off, kids)
    assert ref[0] == REC_DRAW and ref[positions.index((0, 1))] == rec(WIN, 9)
    assert np.count_nonzero(ref == REC_DRAW) == 19 and loopy_ref.check_rules(prim, off, kids, ref) == []


def test_draw_records_round_trip_through_both_table_formats(tmp_path):
    from gamesmanmpi_amd.persist import read_reference_tables, write_reference_tables
    from gamesmanmpi_amd.solver import dump_table

    class Codec:
        def pos(self, key):
            return "p%d" % key
    keys = np.arange(4, dtype=np.uint64)
    recs = np.array([REC_DRAW, rec(WIN, 3), rec(TIE, 2), REC_DRAW], dtype=np.uint16)
    dump_table(str(tmp_path / "table.npz"), keys, recs)
    back = np.load(tmp_path / "table.npz")
    assert np.array_equal(back["keys"], keys) and np.array_equal(back["records"], recs)
    assert sum(write_reference_tables(str(tmp_path), Codec(), keys, recs, 2)) == 4
    assert read_reference_tables(str(tmp_path), 2) == {"p0": (DRAW, 0), "p1": (WIN, 3), "p2": (TIE, 2), "p3": (DRAW, 0)}


def test_moves_rank_a_draw_child_between_tie_and_win():
    from gamesmanmpi_amd.solver import best_move
    assert best_move([rec(WIN, 1), REC_DRAW, rec(WIN, 9)]) == (1, (DRAW, 0))
    assert best_move([REC_DRAW, rec(TIE, 7), rec(WIN, 2)]) == (1, (TIE, 8))
    assert best_move([REC_DRAW, rec(TIE, 7), rec(LOSS, 30)]) == (2, (WIN, 31))
    assert best_move([rec(WIN, 2), rec(WIN, 5)]) == (1, (LOSS, 6))   # as ever without a DRAW


# ---------------------------------------------------------------- the device
def context(loopy=True):
    from gamesmanmpi_amd import Context
    c = Context(_lib.GAME_GRAPH, (), device=0)
    if loopy:
        c.set_option(_lib.OPT_LOOPY, 1)
    return c


@pytest.fixture
def ctx():
    c = context()
    yield c
    c.close()


def positions_counted(c):
    """*n of gm_histogram: every stored position."""
    n_rem, n = ctypes.c_int(), ctypes.c_uint64()
    _lib.check(c.L.gm_histogram(c.h, None, 0, ctypes.byref(n_rem), ctypes.byref(n)))
    return n.value


def check_table(c, graph, ref, levels, got):
    """Export, root, digest, histogram, draw count, stats and gm_verify of the table c holds."""
    prim, off, kids = graph
    n = len(prim)
    ref = np.asarray(ref, dtype=np.uint16)
    assert got == (n, ref[0])
    keys, recs = c.export()
    assert np.array_equal(keys, np.arange(n, dtype=np.uint64))
    bad = np.flatnonzero(recs != ref)
    assert not len(bad), (len(bad), [(int(i), hex(recs[i]), hex(ref[i])) for i in bad[:5]])
    assert c.digest() == (conftest.digest(np.arange(n, dtype=np.uint64), ref), n)
    draws = int(np.count_nonzero(ref == REC_DRAW))
    hist = c.histogram()
    want = analysis.from_records(ref[ref != REC_DRAW])
    assert hist.shape == want.shape and np.array_equal(hist, want)
    assert c.draw_count() == draws
    assert positions_counted(c) == n and positions_counted(c) - int(hist.sum()) == draws
    st = c.stats()
    interior = int(np.count_nonzero(np.asarray(prim) == UNDECIDED))
    assert (st["n_positions"], st["n_primitive"], st["n_edges"], st["engine"]) == (n, n - interior, int(off[n]), 5)
    assert st["n_tiers"] == levels
    res, offenders = c.verify()
    assert res["n_bad"] == 0 and res["root_ok"] == 1 and res["checked"] == n and offenders == []


def check_solve(c, graph):
    value, rem, levels = loopy_ref.solve_levels(*graph)
    check_table(c, graph, graph_ref.pack(value, rem), levels, c.solve_graph(*graph))


def check_no_table(c):
    for call in (c.export, c.digest, c.histogram, c.draw_count, c.verify):
        with pytest.raises(_lib.GMError) as e:
            call()
        assert e.value.code == E_STATE, (call.__name__, str(e.value))


@gpu
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("n", SIZES)
def test_loopy_mode_on_dags_equals_the_default_mode(n, mix):
    plain, loopy = context(loopy=False), context()
    for seed in SEEDS:
        graph = tgr.dag(n, mix, seed)
        plain.solve_graph(*graph)
        want = plain.export()[1]
        assert np.array_equal(want, tgr.dag_ref(n, mix, seed)) and plain.draw_count() == 0
        value, rem, levels = loopy_ref.solve_levels(*graph)
        assert np.array_equal(graph_ref.pack(value, rem), want)
        check_table(loopy, graph, want, levels, loopy.solve_graph(*graph))
        assert loopy.digest() == plain.digest()
    plain.close()
    loopy.close()


@gpu
@pytest.mark.parametrize("draw_leaves", [False, True], ids=["", "draw-leaves"])
@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("n", SIZES)
def test_rewired_graphs(ctx, n, frac, draw_leaves):
    for mix in MIXES:
        for seed in SEEDS:
            key = (n, mix, seed, frac, draw_leaves)
            ref, levels = solved(*key)
            check_table(ctx, rewired(*key), ref, levels, ctx.solve_graph(*rewired(*key)))


@gpu
def test_one_cyclic_graph_past_the_grid_cap(ctx):
    """8192 * 256 + 257 nodes: every grid-stride loop of the loopy kernels goes round again."""
    graph = loopy_ref.rewire(graph_ref.random_dag(tgr.BIG_N, 6, 3, True, MIXES["even"], 99), 0.05, 5, True)
    value, rem, levels = loopy_ref.solve_levels(*graph)
    ref = graph_ref.pack(value, rem)
    assert set(value.tolist()) == {WIN, LOSS, TIE, DRAW} and np.any(value[tgr.GRID_CAP:] == DRAW)
    check_table(ctx, graph, ref, levels, ctx.solve_graph(*graph))
    idx = np.random.default_rng(5).integers(0, tgr.BIG_N, size=10_000).astype(np.uint64)
    assert np.array_equal(ctx.query(idx), ref[idx.astype(np.int64)])


@gpu
@pytest.mark.parametrize("name", FIXED)
def test_fixed_shapes(ctx, name):
    graph, want = FIXED[name]
    ctx.solve_graph(*graph)
    assert ctx.export()[1].tolist() == want
    check_solve(ctx, graph)


@gpu
@pytest.mark.parametrize("name,code", [("no-moves", E_NOMOVES), ("code-5", None)])
def test_unsolvable_nodes_are_still_refused(ctx, name, code):
    check_solve(ctx, FIXED["2-cycle"][0])
    with pytest.raises(_lib.GMError) as e:
        ctx.solve_graph(*tgr.BAD_NODES[name][:3])
    assert code is None or e.value.code == code, str(e.value)
    check_no_table(ctx)
    check_solve(ctx, FIXED["2-cycle"][0])


@gpu
@pytest.mark.parametrize("shape", ["alone", "under-chain", "with-2-cycle"])
def test_fan_in_and_multiplicity(ctx, shape):
    """The root's counter is 100,000 over 64 distinct children; each of them has about 1,500
    parent entries, all the root."""
    graph = {"alone": lambda: graph_ref.star(100_000),
             "under-chain": lambda: graph_ref.hang_under_chain(graph_ref.star(100_000), 3),
             "with-2-cycle": star_with_a_2_cycle}[shape]()
    check_solve(ctx, graph)
    if shape != "with-2-cycle":
        assert np.array_equal(ctx.export()[1], graph_ref.solve_reference(*graph))
    else:
        assert ctx.draw_count() == 2


@gpu
@pytest.mark.parametrize("top", [0x3FFE, 0x4000])
@pytest.mark.parametrize("leaf", [LOSS, TIE], ids=["loss", "tie"])
def test_remoteness_boundary(ctx, leaf, top):
    """A chain whose root has remoteness `top`: about 16 k host-synchronised levels, of the
    win/loss phase under a LOSS leaf and of the tie phase under a TIE leaf.  0x3FFE solves; one
    past 0x3FFF is GM_E_CAP and leaves no table.  The expected table is graph_ref's (the chain
    is acyclic; the pull-style reference would take a numpy pass per level)."""
    graph = graph_ref.chain(top + 1, leaf)
    value, rem = graph_ref.solve_values(*graph)
    assert rem[0] == top == rem.max()
    if top > 0x3FFF:
        with pytest.raises(_lib.GMError) as e:
            ctx.solve_graph(*graph)
        assert e.value.code == E_CAP, str(e.value)
        check_no_table(ctx)
        check_solve(ctx, FIXED["1000-cycle"][0])
        return
    check_table(ctx, graph, graph_ref.pack(value, rem), top, ctx.solve_graph(*graph))


@gpu
def test_one_context_solves_loopy_default_and_loopy_again():
    c = context()
    cyc, dag = rewired(257, "even", 1, 0.5, True), tgr.dag(257, "even", 0)
    check_table(c, cyc, *solved(257, "even", 1, 0.5, True), c.solve_graph(*cyc))
    c.set_option(_lib.OPT_LOOPY, 0)
    tgr.check_solve(c, dag, tgr.dag_ref(257, "even", 0), LEVELS[0] - 1)
    assert c.draw_count() == 0
    with pytest.raises(_lib.GMError) as e:
        c.poke(0, REC_DRAW)     # not a record of the default mode's table
    assert e.value.code == E_ARG
    with pytest.raises(_lib.GMError, match="cycle") as e:
        c.solve_graph(*rewired(257, "even", 1, 0.5, False))   # cycles, no DRAW leaf
    assert e.value.code == E_STATE
    check_no_table(c)
    with pytest.raises(_lib.GMError) as e:
        c.solve_graph(*FIXED["draw"][0])
    assert e.value.code == -6   # GM_E_DRAW, as ever
    c.set_option(_lib.OPT_LOOPY, 1)
    check_table(c, cyc, *solved(257, "even", 1, 0.5, True), c.solve_graph(*cyc))
    c.close()


@gpu
def test_the_option_is_the_graph_engines():
    from gamesmanmpi_amd import Context
    c = context(loopy=False)
    for value in (-1, 2):
        with pytest.raises(_lib.GMError) as e:
            c.set_option(_lib.OPT_LOOPY, value)
        assert e.value.code == E_ARG
    with pytest.raises(_lib.GMError) as e:
        c.draw_count()
    assert e.value.code == E_STATE      # before a solve
    c.close()
    t = Context(_lib.GAME_TTT, (), device=0)
    with pytest.raises(_lib.GMError) as e:
        t.set_option(_lib.OPT_LOOPY, 1)
    assert e.value.code == E_ARG
    with pytest.raises(_lib.GMError) as e:
        t.draw_count()
    assert e.value.code == E_STATE
    t.solve(t.initial())
    assert t.draw_count() == 0
    with pytest.raises(_lib.GMError) as e:
        t.poke(0, REC_DRAW)
    assert e.value.code == E_ARG
    t.close()


# gm_poke + gm_verify: name -> (graph, node, planted record, the class it must be reported as)
POKES = {
    # 0 <-> 1 and 2 <-> 3, 1 -> 2 as well: all DRAW, and node 1 stays DRAW by its child 2
    "draw-to-win-on-a-2-cycle": (([4, 4, 4, 4], [0, 1, 3, 4, 5], [1, 0, 2, 3, 2]), 0, rec(WIN, 1), "bad_value"),
    # the root has two TIE-in-1 children: it stays TIE in 2 by the other
    "tie-to-draw": (([4, 4, 4, 2], [0, 2, 3, 4, 4], [1, 2, 3, 3]), 1, REC_DRAW, "bad_value"),
    # 0 -> {0, 1}, 1 a LOSS leaf: WIN in 1 whatever its own record says
    "win-with-the-wrong-remoteness": (tgr.CYCLES["self-loop"], 0, rec(WIN, 5), "bad_value"),
    # the root has a LOSS leaf besides: WIN in 1 either way
    "draw-primitive-to-loss": (([4, 3, 1], [0, 2, 2, 2], [1, 2]), 1, rec(LOSS, 0), "bad_primitive"),
}


@gpu
@pytest.mark.parametrize("name", POKES)
def test_verify_names_a_planted_record(ctx, name):
    graph, node, planted, cls = POKES[name]
    check_solve(ctx, graph)
    good = int(ctx.query([node])[0])
    assert good != planted
    ctx.poke(node, planted)
    assert ctx.query([node])[0] == planted
    res, offenders = ctx.verify()
    assert offenders == [node] and res["n_bad"] == 1 and res[cls] == 1, (res, offenders)
    bad = ctx.export()[1]
    assert dict(loopy_ref.check_rules(*graph, bad)) == {node: cls}
    ctx.poke(node, good)
    res, offenders = ctx.verify()
    assert res["n_bad"] == 0 and res["root_ok"] == 1 and offenders == []


@gpu
def test_verify_counts_a_missing_child(ctx):
    graph = POKES["tie-to-draw"][0]
    check_solve(ctx, graph)
    ctx.poke(3, 0xFFFF)   # the TIE leaf: both its parents lose a child, the leaf its primitive record
    res, offenders = ctx.verify()
    assert (res["missing_child"], res["bad_primitive"], res["n_bad"]) == (2, 1, 3) and offenders == [1, 2, 3]


@gpu
def test_five_solves_give_one_digest(ctx):
    key = (4097, "even", 2, 0.5, True)
    digests = set()
    for _ in range(5):
        ctx.solve_graph(*rewired(*key))
        digests.add(ctx.digest())
    assert digests == {(conftest.digest(np.arange(4097, dtype=np.uint64), solved(*key)[0]), 4097)}


@gpu
def test_solver_on_a_plugin_with_cycles():
    from gamesmanmpi_amd import Solver
    mod = shuttle()
    s = Solver(mod, loopy=True)
    assert s.codec.game_id == _lib.GAME_GRAPH
    assert s.solve() == (64, REC_DRAW) and s.value == DRAW
    assert s.root_line() == "DRAW"
    assert s.draw_count() == 19 and s.ctx.draw_count() == 19
    # the advances by one give the opponent a WIN; the first advance by two keeps the draw
    rows, best = s.moves((0, 0))
    assert rows == [((0, 1), (1, 0), WIN, 9), ((1, 1), (0, 1), WIN, 9), ((0, 2), (2, 0), DRAW, 0),
                    ((1, 2), (0, 2), DRAW, 0)]
    assert best == rows[2]
    assert s.lookup((0, 1)) == (WIN, 9) and s.lookup((7, 7)) == (LOSS, 0)
    res, offenders = s.verify()
    assert res["n_bad"] == 0 and res["root_ok"] == 1 and res["checked"] == 64
    assert int(s.analysis().sum()) == 64 - 19
    s.close()
    won = Solver(mod, root=(0, 1), loopy=True)
    won.solve()
    assert won.root_line() == "WIN in 9 moves" and won.value == WIN
    won.close()
    refused = Solver(mod)     # the default mode still refuses the cycle
    with pytest.raises(_lib.GMError, match="cycle"):
        refused.solve()
    refused.close()


@gpu
def test_launcher_loopy_analysis_verify(tmp_path):
    import solver_launcher
    args = solver_launcher.build_parser().parse_args(
        [os.path.join(conftest.REPO, "tests", "plugins", "shuttle.py"), "--loopy", "--analysis", "--verify",
         "-sd", str(tmp_path), "--sd-format", "both"])
    out = io.StringIO()
    assert solver_launcher.run(args, out=out) == 0
    lines = out.getvalue().splitlines()
    assert lines[0] == "DRAW" and lines[-2] == "Draw  19" and lines[-1] == "Verified 64 positions: consistent"
    hist = analysis.parse_table("\n".join(lines[1:-2]))
    assert int(hist.sum()) == 64 - 19
    stats = tmp_path / "stats"
    saved = json.load(open(stats / "analysis.json"))
    assert saved["draw"] == 19 and saved["positions"] == 45
    table = np.load(stats / "0" / "table.npz")
    assert int(np.count_nonzero(table["records"] == REC_DRAW)) == 19 and table["records"][0] == REC_DRAW
    from gamesmanmpi_amd.persist import read_reference_tables
    shelves = read_reference_tables(str(tmp_path), 1)
    assert shelves["(0, 0)"] == (DRAW, 0) and shelves["(0, 1)"] == (WIN, 9) and len(shelves) == 64
    assert sum(v == (DRAW, 0) for v in shelves.values()) == 19
