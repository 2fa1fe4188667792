"""gm_solve_graph (csrc/graph.hip) on arbitrary graphs against tests/graph_ref.py.

The explicit-graph engine is the one engine that takes arbitrary input, so this is where the
win/loss/tie reduction every engine shares meets value and remoteness mixes no game produces:
random DAGs whose children resolve in different rounds, huge fan-out, the ends of the 14-bit
remoteness range, a graph larger than the launch grid, and the engine's error contract.

The unmarked tests pin the reference itself to the project's oracle (canonical.solve) and to
enumerate_graph on the CPU; the `gpu` tests compare export, root, digest, histogram and stats
of a device solve with it.
"""
import functools
import re

import numpy as np
import pytest

import conftest
import graph_ref
from graph_ref import LOSS, TIE, UNDECIDED, WIN

import canonical
from gamesmanmpi_amd import _lib, analysis
from gamesmanmpi_amd.graph import enumerate_graph

gpu = pytest.mark.gpu

MIXES = {"win": (1, 0, 0), "loss": (0, 1, 0), "tie": (0, 0, 1), "even": (1, 1, 1)}
SIZES = (2, 63, 64, 65, 255, 256, 257, 4097, 50_000)
SEEDS = (0, 1, 2)
LEVELS = (5, 9, 17)              # by seed
GRID_CAP = 8192 * 256            # threads of the largest grid graph.hip launches
BIG_N = GRID_CAP + 257


@functools.lru_cache(maxsize=None)
def dag(n, mix, seed, levels=None, max_deg=6):
    g = graph_ref.random_dag(n, levels or LEVELS[seed], max_deg, True, MIXES[mix], 1000 * n + seed)
    for a in g:
        a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def dag_ref(n, mix, seed):
    ref = graph_ref.solve_reference(*dag(n, mix, seed))
    ref.setflags(write=False)
    return ref


def with_primitive_parents(graph, seed):
    """`graph` with a third of its interior nodes below the root declared primitive, their
    children still listed -- one of them also lists the root, which would close a cycle if a
    primitive's children counted."""
    prim, off, kids = (a.copy() for a in graph)
    rng = np.random.default_rng(seed)
    inner = np.flatnonzero(prim == UNDECIDED)[1:]
    chosen = inner[rng.random(len(inner)) < 1 / 3]
    prim[chosen] = rng.choice([WIN, LOSS, TIE], size=len(chosen))
    kids[off[chosen[0]]] = 0
    return prim, off, kids


def small_graphs():
    """(name, graph) of every small shape of the GPU tests."""
    for n in SIZES[:-1]:
        for mix in MIXES:
            for seed in SEEDS:
                yield "dag-%d-%s-%d" % (n, mix, seed), dag(n, mix, seed)
    for leaf, name in ((WIN, "win"), (LOSS, "loss"), (TIE, "tie")):
        for n in (1, 2, 3, 700):
            yield "chain-%d-%s" % (n, name), graph_ref.chain(n, leaf)
    yield "star-500", graph_ref.star(500)
    yield "star-500-under-chain", graph_ref.hang_under_chain(graph_ref.star(500), 3)
    for seed in SEEDS:
        yield "primitive-parents-%d" % seed, with_primitive_parents(dag(257, "even", seed), seed)


SMALL = list(small_graphs())
SMALL_IDS = [name for name, _ in SMALL]
SMALL_GRAPHS = [g for _, g in SMALL]

# what the engine must refuse: name -> (prim, off, kids, the reference's exception)
BAD_NODES = {
    "draw": ([4, 3], [0, 1, 1], [1], "DRAW"),
    "draw-alone": ([3], [0, 0], [], "DRAW"),
    "draw-unreachable": ([4, 1, 3], [0, 1, 1, 1], [1], "DRAW"),
    "no-moves": ([4, 4, 1], [0, 2, 2, 2], [1, 2], "without moves"),
    "code-5": ([4, 5], [0, 1, 1], [1], "code"),
}
_ring = [[(i + 1) % 1000] + [1000] * (i % 10 == 0) for i in range(1000)]
CYCLES = {
    "self-loop": ([4, 1], [0, 2, 2], [0, 1]),
    "2-cycle": ([4, 4], [0, 1, 2], [1, 0]),
    # a ring of 1,000; every tenth node also has a LOSS leaf, which must not decide it
    "1000-cycle": ([4] * 1000 + [1], np.r_[0, np.cumsum([len(x) for x in _ring]), 1100], sum(_ring, [])),
    # 0 -> 1 is solvable; 2 <-> 3 and 4 -> 2 are not reachable from the root
    "unreachable-cycle": ([4, 0, 4, 4, 4], [0, 1, 1, 2, 3, 4], [1, 3, 2, 2]),
}
BAD_ARGS = {
    "child-is-n": ([4, 1], [0, 1, 1], [2]),
    "child-is-2^32-1": ([4, 1, 1], [0, 2, 2, 2], [1, 0xFFFFFFFF]),
    "child-of-a-primitive-is-n": ([4, 1], [0, 1, 2], [1, 2]),
    "off-not-monotone": ([4, 4, 1], [0, 2, 1, 2], [1, 2]),
    "empty": ([], [0], []),
}


# ---------------------------------------------------------------- the reference (CPU)
@pytest.mark.parametrize("graph", SMALL_GRAPHS, ids=SMALL_IDS)
def test_reference_equals_canonical_solve(graph):
    ref = graph_ref.solve_reference(*graph)
    table, _ = canonical.solve(graph_ref.as_plugin(*graph))
    assert sorted(table) == graph_ref.reachable(*graph).tolist()
    assert all(canonical_rec == (ref[i] >> 14, ref[i] & 0x3FFF) for i, canonical_rec in table.items())


@pytest.mark.parametrize("graph", SMALL_GRAPHS, ids=SMALL_IDS)
def test_reference_on_the_enumerated_graph(graph):
    ref = graph_ref.solve_reference(*graph)
    positions, prim, off, kids = enumerate_graph(graph_ref.as_plugin(*graph), 0, workers=1)
    assert positions[0] == 0 and sorted(positions) == graph_ref.reachable(*graph).tolist()
    assert np.array_equal(graph_ref.solve_reference(prim, off, kids), ref[positions])


@pytest.mark.parametrize("graph", SMALL_GRAPHS, ids=SMALL_IDS)
def test_layered_reference_equals_the_plain_one(graph):
    assert np.array_equal(graph_ref.solve_reference_layered(*graph), graph_ref.solve_reference(*graph))


@pytest.mark.parametrize("mix", MIXES)
def test_layered_reference_equals_the_plain_one_at_50000(mix):
    assert np.array_equal(graph_ref.solve_reference_layered(*dag(50_000, mix, 0)), dag_ref(50_000, mix, 0))


def test_generated_graphs_have_the_shape_asked_for():
    for seed in SEEDS:
        prim, off, kids = dag(4097, "even", seed)
        assert graph_ref.height(prim, off, kids) == LEVELS[seed] - 1
        deg = np.diff(off.astype(np.int64))
        assert deg[prim == UNDECIDED].min() >= 1 and deg.max() == 6 and not deg[prim != UNDECIDED].any()
        assert set(prim.tolist()) == {WIN, LOSS, TIE, UNDECIDED}
        level = np.where(np.arange(4097) == 0, 0, 1 + (np.arange(4097) - 1) % (LEVELS[seed] - 1))
        src = np.repeat(np.arange(4097), deg)
        span = level[kids] - level[src]
        assert span.min() == 1 and span.max() > 1          # skip edges
        pairs = src.astype(np.int64) << 32 | kids
        assert len(np.unique(pairs)) < len(pairs)            # duplicate children
        ref = dag_ref(4097, "even", seed)
        assert set((ref >> 14).tolist()) == {WIN, LOSS, TIE}
    prim, off, kids = graph_ref.star(100_000)
    assert off[1] == 100_000 and len(np.unique(kids[:100_000])) <= 64
    vals = graph_ref.solve_reference(prim, off, kids)[kids[:100_000]] >> 14
    assert set(vals.tolist()) == {WIN, LOSS, TIE}


@pytest.mark.parametrize("name", BAD_NODES)
def test_reference_refuses_unsolvable_nodes(name):
    prim, off, kids, message = BAD_NODES[name]
    for solve in (graph_ref.solve_reference, graph_ref.solve_reference_layered):
        with pytest.raises(graph_ref.GraphError, match=message):
            solve(prim, off, kids)
    if name != "draw-unreachable":   # canonical.solve only sees what the root reaches
        with pytest.raises(canonical.OracleError):
            canonical.solve(graph_ref.as_plugin(prim, off, kids))


@pytest.mark.parametrize("name,unresolved", [("self-loop", 1), ("2-cycle", 2), ("1000-cycle", 1000),
                                             ("unreachable-cycle", 3)])
def test_reference_counts_the_nodes_of_a_cycle(name, unresolved):
    for solve in (graph_ref.solve_reference, graph_ref.solve_reference_layered):
        with pytest.raises(graph_ref.CycleError) as e:
            solve(*CYCLES[name])
        assert e.value.unresolved == unresolved


def test_reference_reports_a_remoteness_past_the_record():
    value, rem = graph_ref.solve_values(*graph_ref.chain(0x4001, LOSS))
    assert rem[0] == 0x4000 and value[0] == LOSS
    with pytest.raises(graph_ref.RemotenessOverflow):
        graph_ref.solve_reference(*graph_ref.chain(0x4001, LOSS))
    assert graph_ref.solve_reference(*graph_ref.chain(0x4000, LOSS))[0] == (WIN << 14 | 0x3FFF)


# ---------------------------------------------------------------- the device
@pytest.fixture(scope="module")
def ctx():
    from gamesmanmpi_amd import Context
    c = Context(_lib.GAME_GRAPH, (), device=0)
    yield c
    c.close()


def check_solve(ctx, graph, ref, height):
    """Solve `graph` on ctx: export, root, digest, histogram and stats equal the reference's."""
    check_table(ctx, graph, ref, height, ctx.solve_graph(*graph))


def check_table(ctx, graph, ref, height, solved):
    prim, off, kids = graph
    n = len(prim)
    assert solved == (n, ref[0])
    keys, recs = ctx.export()
    assert np.array_equal(keys, np.arange(n, dtype=np.uint64))
    bad = np.flatnonzero(recs != ref)
    assert not len(bad), (len(bad), [(int(i), hex(recs[i]), hex(ref[i])) for i in bad[:5]])
    assert ctx.digest() == (conftest.digest(np.arange(n, dtype=np.uint64), ref), n)
    hist = ctx.histogram()
    want = analysis.from_records(ref)
    assert hist.shape == want.shape and np.array_equal(hist, want)
    st = ctx.stats()
    interior = int(np.count_nonzero(np.asarray(prim) == UNDECIDED))
    assert (st["n_positions"], st["n_primitive"], st["n_edges"], st["engine"]) == (n, n - interior, int(off[n]), 5)
    if interior:
        assert 1 <= st["n_tiers"] <= height, (st["n_tiers"], height)
    else:
        assert st["n_tiers"] == 0


def check_after_failure(ctx):
    """After a failed solve the context holds no table -- not the failed one's, not the one
    before -- and solves the next graph as a fresh one would."""
    for call in (ctx.export, ctx.digest, ctx.histogram):
        with pytest.raises(_lib.GMError) as e:
            call()
        assert e.value.code == -5, (call.__name__, str(e.value))   # GM_E_STATE
    check_solve(ctx, dag(65, "even", 1), dag_ref(65, "even", 1), LEVELS[1] - 1)


@gpu
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("n", SIZES)
def test_random_dags_with_skip_edges(ctx, n, mix):
    for seed in SEEDS:
        check_solve(ctx, dag(n, mix, seed), dag_ref(n, mix, seed), min(n, LEVELS[seed]) - 1)


@gpu
def test_consecutive_solves_on_one_context_do_not_leak():
    from gamesmanmpi_amd import Context
    c = Context(_lib.GAME_GRAPH, (), device=0)
    for n, mix, seed in ((50_000, "even", 1), (65, "loss", 2), (4097, "tie", 0), (4097, "even", 2)):
        check_solve(c, dag(n, mix, seed), dag_ref(n, mix, seed), min(n, LEVELS[seed]) - 1)
    c.close()


@gpu
def test_one_solve_past_the_grid_cap(ctx):
    """2,097,409 nodes: the grid-stride loops of the init, round, digest (8,192 blocks) and
    histogram (2,048 blocks) kernels go round more than once."""
    graph = graph_ref.random_dag(BIG_N, 6, 3, True, MIXES["even"], 99)
    ref = graph_ref.solve_reference_layered(*graph)
    assert set((ref >> 14).tolist()) == {WIN, LOSS, TIE} and ref[GRID_CAP:].max() >> 14 == TIE
    check_solve(ctx, graph, ref, 5)
    idx = np.random.default_rng(5).integers(0, BIG_N, size=10_000).astype(np.uint64)
    assert (idx >= GRID_CAP).any()
    assert np.array_equal(ctx.query(idx), ref[idx.astype(np.int64)])


@gpu
@pytest.mark.parametrize("under_chain", [False, True])
def test_fan_out(ctx, under_chain):
    graph = graph_ref.star(100_000)
    if under_chain:
        graph = graph_ref.hang_under_chain(graph, 3)
    check_solve(ctx, graph, graph_ref.solve_reference(*graph), graph_ref.height(*graph))


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_listed_children_of_a_primitive_are_ignored(ctx, seed):
    graph = with_primitive_parents(dag(4097, "even", seed), seed)
    ref = graph_ref.solve_reference(*graph)
    assert not np.array_equal(ref, dag_ref(4097, "even", seed))
    check_solve(ctx, graph, ref, graph_ref.height(*graph))


@gpu
@pytest.mark.parametrize("top", [0x3FFE, 0x3FFF, 0x4000])
@pytest.mark.parametrize("leaf", [LOSS, WIN, TIE], ids=["loss", "win", "tie"])
def test_remoteness_boundary(ctx, leaf, top):
    """A chain whose root has remoteness `top` (about 16 k host-synchronised rounds).  Up to
    0x3FFE (MAX_REMOTENESS) it solves; from 0x4000 it is GM_E_CAP; at 0x3FFF, the last value a
    record can hold, either -- but never a wrapped record.  Today at 0x3FFF: the chains ending
    in a LOSS leaf (root WIN in 0x3FFF) and in a TIE leaf (root TIE in 0x3FFF) solve; the chain
    ending in a WIN leaf (root LOSS in 0x3FFF) is GM_E_CAP, since score_overflows refuses every
    WIN child from remoteness 0x3FFE on."""
    graph = graph_ref.chain(top + 1, leaf)
    value, rem = graph_ref.solve_values(*graph)
    assert rem[0] == top == rem.max()
    if top > 0x3FFF:
        with pytest.raises(_lib.GMError) as e:
            ctx.solve_graph(*graph)
        assert e.value.code == -8, str(e.value)   # GM_E_CAP
        check_after_failure(ctx)
        return
    try:
        solved = ctx.solve_graph(*graph)
    except _lib.GMError as e:
        assert top == 0x3FFF and e.code == -8, str(e)
        check_after_failure(ctx)
        return
    check_table(ctx, graph, graph_ref.pack(value, rem), top, solved)


def fails(ctx, graph, code=None, match=None):
    """A valid solve, then `graph` fails as asked and leaves no table, then a valid solve."""
    check_solve(ctx, dag(257, "even", 0), dag_ref(257, "even", 0), LEVELS[0] - 1)
    with pytest.raises(_lib.GMError, match=match) as e:
        ctx.solve_graph(*graph)
    assert code is None or e.value.code == code, str(e.value)
    check_after_failure(ctx)
    return str(e.value)


@gpu
@pytest.mark.parametrize("name", BAD_NODES)
def test_unsolvable_nodes_are_refused(ctx, name):
    prim, off, kids, _ = BAD_NODES[name]
    fails(ctx, (prim, off, kids), {"draw": -6, "draw-alone": -6, "draw-unreachable": -6, "no-moves": -7}.get(name))


@gpu
@pytest.mark.parametrize("name", BAD_ARGS)
def test_bad_arguments_are_refused_on_the_host(ctx, name):
    fails(ctx, BAD_ARGS[name], -1)   # GM_E_ARG


@gpu
@pytest.mark.parametrize("name", CYCLES)
def test_cycles_are_refused_with_their_node_count(ctx, name):
    with pytest.raises(graph_ref.CycleError) as ref:
        graph_ref.solve_reference(*CYCLES[name])
    message = fails(ctx, CYCLES[name], -5, "cycle")   # GM_E_STATE
    assert int(re.search(r"(\d+) positions never resolve", message).group(1)) == ref.value.unresolved


@gpu
def test_query(ctx):
    n = 4097
    ref = dag_ref(n, "even", 1)
    ctx.solve_graph(*dag(n, "even", 1))
    got = ctx.query(np.array([0, n - 1, n, 1 << 32, (1 << 64) - 1], dtype=np.uint64))
    assert got.tolist() == [ref[0], ref[n - 1], 0xFFFF, 0xFFFF, 0xFFFF]
    idx = np.random.default_rng(3).permutation(n).astype(np.uint64)
    assert np.array_equal(ctx.query(idx), ref[idx.astype(np.int64)])
    assert len(ctx.query(np.zeros(0, dtype=np.uint64))) == 0
