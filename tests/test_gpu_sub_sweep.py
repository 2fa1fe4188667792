"""Custom roots of the SUBTRACT game on the three byte-table engines -- the one-GPU box engine
(csrc/dense_box.hip), its split over virtual ranks (csrc/dist_box.hip) and the block engine
(csrc/dense_sub.hip, csrc/dist_sub.hip) -- swept against the C oracle.

What an engine does on the host follows from the root: the box lists and their order, which box
of a mirror pair is computed and whether its twin lies outside the region, how the hybrid range
is clipped to the root's box-tiers, the dataflow queues, the split axes and owner maps, the block
lists.  tests/sub_roots.py holds roots drawn over those shapes (tests/test_sub_roots.py says which);
here every one of them is solved on every configuration and compared, bit for bit, with
oracle_solve of the same root: position count, root record, export, digest, histogram, gm_verify,
and keys outside the region.

The one-GPU engines solve into a table the test owns and fills with 0x80 before every solve
(tests/box_table.py): LOSS in 127, which no position of the game has, so a box, a row or a byte
that a solve does not store cannot pass for a solved one -- whatever an earlier solve or the
allocator left there.  One context per configuration solves its roots in sequence: every solve
after the first is a root change, which rebuilds the context's lists, flags and captured graph
when the root's top box changes and keeps them when it does not (PAIRS8).

Option values the library refuses (GM_E_ARG): GM_OPT_SUB_LOW 4 -- the block engine has kernels for
1..3 low heaps -- asserted in test_block_sub_low_4_is_refused.
"""
import os

import numpy as np
import pytest

from box_table import POISON, _Table
from conftest import digest
from sub_roots import IDLE8, PAIRS8, ROOTS8, ROOTS_H, box_tiers, every, outside_keys, positions, split_axes

from gamesmanmpi_amd import Context, GMError, _lib

pytestmark = pytest.mark.gpu

SUB = 5
GM_E_ARG = -1
ALL_FLOW = "41,40"
TIERS_ONLY = "0,40"

_REF = {}


def _ref(oracle, heaps, root):
    """The oracle's table of the root, its digest and its histogram; solved once."""
    if (heaps, root) not in _REF:
        keys, recs = oracle.solve(SUB, (heaps,), root)
        val, rem = recs >> 14, recs & 0x3FFF
        hist = np.zeros((3, int(rem.max()) + 1), dtype=np.uint64)
        for v in range(3):
            hist[v] = np.bincount(rem[val == v], minlength=hist.shape[1])
        _REF[(heaps, root)] = (keys, recs, digest(keys, recs), hist)
    return _REF[(heaps, root)]


def _check(ctx, oracle, heaps, root, n, rec, what, one_gpu=False, launches=None):
    """Everything the context answers about its last solve against the oracle's table."""
    keys, recs, dig, hist = _ref(oracle, heaps, root)
    where = "%s root 0x%0*X" % (what, heaps, root)
    assert n == positions(root, heaps) == len(keys), where
    k, r = ctx.export()
    assert np.array_equal(k, keys), where
    if not np.array_equal(r, recs):
        i = int(np.nonzero(r != recs)[0][0])
        pytest.fail("%s: %d records differ, the first at key 0x%X: expected 0x%04X, got 0x%04X"
                    % (where, int((r != recs).sum()), int(keys[i]), int(recs[i]), int(r[i])))
    assert rec == int(recs[-1]), where
    assert ctx.digest() == (dig, n), where
    assert ctx.query(outside_keys(root, heaps)).tolist() == [_lib.REC_UNSOLVED] * 3, where
    v, bad = ctx.verify()
    assert (v["n_bad"], v["root_ok"], v["checked"]) == (0, 1, n), (where, v, [hex(b) for b in bad[:4]])
    st = ctx.stats()
    assert st["flow_fallbacks"] == 0, where   # a dataflow wait that timed out is a failure here
    if one_gpu:
        h = ctx.histogram()
        assert h.shape == hist.shape and np.array_equal(h, hist), where
    if launches is not None:
        assert st["kernel_launches"] == launches, where


def _chunks(roots, size):
    return [tuple(roots[i:i + size]) for i in range(0, len(roots), size)]


def _solve_env(ctx, root, env):
    """ctx.solve with the engine's environment knobs set around it (both kinds are read per solve
    or per launch: csrc/dense_box.hip box_hybrid_wanted, box_thin_groups)."""
    os.environ.update(env)
    try:
        return ctx.solve(root)
    finally:
        for k in env:
            del os.environ[k]


# ------------------------------------------------------------------ the one-GPU box engine
def _tail_is_last_tier(root):
    """The range of tests/test_gpu_box_hybrid.py _ranges whose tail launch is the last tier alone."""
    t = box_tiers(root)
    return "%d,%d" % (max(0, min(7, t - 3)), t - 2)


# name: (options, environment or a function of the root giving it, roots)
BOX_CONFIGS = {
    "default": ({}, {}, ROOTS8),
    "sym0": ({"SYMMETRY": 0}, {}, ROOTS8),
    "allflow": ({}, {"GM_BOX_HYBRID": ALL_FLOW}, ROOTS8),
    "tiers": ({}, {"GM_BOX_HYBRID": TIERS_ONLY}, every(3)),
    "tail1": ({}, lambda root: {"GM_BOX_HYBRID": _tail_is_last_tier(root)}, every(3)),
    "flow1": ({"BOX_FLOW": 1}, {}, every(3)),
    "eager": ({"GRAPH": 0}, {}, every(3)),
    # the four-wave kernel on box-tiers of at most 4 groups: under the default schedule the few
    # thin tiers left to tier launches, with tier launches only every thin tier
    "thin4": ({}, {"GM_BOX_THIN_GROUPS": "4"}, every(3)),
    "thin4-tiers": ({}, {"GM_BOX_THIN_GROUPS": "4", "GM_BOX_HYBRID": TIERS_ONLY}, every(3)),
}
BOX_CASES = [(name, i) for name, (_, _, roots) in BOX_CONFIGS.items() for i in range(len(_chunks(roots, 16)))]


class _OneGpu:
    """The 4 GiB table the one-GPU contexts adopt, and one context per configuration name."""

    def __init__(self):
        self.table = _Table()
        self.ctxs = {}

    def ctx(self, name, opts, heaps=8, table=None):
        if name not in self.ctxs:
            c = Context(SUB, (heaps,), device=0)
            for k, v in opts.items():
                c.set_option(getattr(_lib, "OPT_" + k), v)
            c.set_option(_lib.OPT_TIMING, 1)
            t = table or self.table
            c.adopt_dense_table(t.data_ptr(), t.numel())
            self.ctxs[name] = c
        return self.ctxs[name]

    def drop(self, name):
        self.ctxs.pop(name).close()

    def close(self):
        for c in self.ctxs.values():
            c.close()
        self.table.free()


@pytest.fixture(scope="module")
def one_gpu():
    g = _OneGpu()
    yield g
    g.close()


def _box_solve(one_gpu, ctx, oracle, root, env, what, launches):
    one_gpu.table.fill(POISON)
    n, rec = _solve_env(ctx, root, env)
    assert ctx.stats()["engine"] == _lib.ENGINE_DENSE
    _check(ctx, oracle, 8, root, n, rec, what, one_gpu=True, launches=launches)


@pytest.mark.parametrize("name,chunk", BOX_CASES, ids=["%s-%d" % c for c in BOX_CASES])
def test_box_engine_roots(one_gpu, oracle, name, chunk):
    """One context per configuration over its roots, every solve into the poisoned table.  The
    launch count (GM_OPT_TIMING) is the root's box-tiers, all of which hold boxes; 1 for the
    whole-solve dataflow."""
    opts, env, roots = BOX_CONFIGS[name]
    ctx = one_gpu.ctx("box-" + name, opts)
    for root in _chunks(roots, 16)[chunk]:
        e = env(root) if callable(env) else env
        _box_solve(one_gpu, ctx, oracle, root, e, name, 1 if opts.get("BOX_FLOW") == 1 else box_tiers(root))


@pytest.mark.parametrize("chunk", range(len(_chunks(PAIRS8, 5))))
def test_box_engine_root_change_inside_one_top_box(one_gpu, oracle, chunk):
    """r, r', r with equal box limits: the second and third solve keep the first one's lists, flags,
    epoch counter and captured graph (csrc/dense_box.hip dense_box_solve), and only the root
    differs -- what is counted, exported, digested and verified must follow it."""
    ctx = one_gpu.ctx("box-pairs", {})
    for r, q in _chunks(PAIRS8, 5)[chunk]:
        for root in (r, q, r):
            _box_solve(one_gpu, ctx, oracle, root, {}, "pair", box_tiers(root))


FLIP_ROOTS = tuple(x for p in zip(ROOTS8[5::24], ROOTS8[2::24]) for x in p)[:12]


@pytest.mark.parametrize("option,values", [("SYMMETRY", (1, 0)), ("BOX_FLOW", (-1, 1))])
def test_box_engine_option_flips_between_roots(one_gpu, oracle, option, values):
    """12 roots on one context, the option changed before every solve: lists and graph are rebuilt
    for the option as well as for the root."""
    assert len(FLIP_ROOTS) == 12
    ctx = one_gpu.ctx("box-flip-" + option, {})
    for i, root in enumerate(FLIP_ROOTS):
        v = values[i % 2]
        ctx.set_option(getattr(_lib, "OPT_" + option), v)
        flow = option == "BOX_FLOW" and v == 1
        _box_solve(one_gpu, ctx, oracle, root, {}, "%s %d" % (option, v), 1 if flow else box_tiers(root))


# ------------------------------------------------------------------ the split box engine
# every fourth root and the deep ones, and of the roots whose region has fewer than three axes to
# split along as many as make eight of them (four with one axis only)
def _split_roots():
    roots = list(every(4))
    for r in IDLE8:
        few = [x for x in roots if split_axes(x) < 3]
        if r not in roots and (len(few) < 8 or (split_axes(r) < 2 and sum(split_axes(x) < 2 for x in few) < 4)):
            roots.append(r)
    return tuple(roots)


SPLIT_ROOTS = _split_roots()
SPLIT_CONFIGS = {"%d-split%d" % (g, s): (g, {"BOX_SPLIT": s}) for g in (2, 3, 4, 8) for s in (0, 1)}
SPLIT_CONFIGS["8-flow1"] = (8, {"BOX_FLOW": 1})
SPLIT_CONFIGS["8-distsym0"] = (8, {"DIST_SYMMETRY": 0})
# a prepare allocates and fills 4 GiB per rank that holds boxes: roots per test id by rank count
SPLIT_CHUNK = {2: 8, 3: 8, 4: 6, 8: 3}
SPLIT_CASES = [(name, i) for name, (g, _) in SPLIT_CONFIGS.items()
               for i in range(len(_chunks(SPLIT_ROOTS, SPLIT_CHUNK[g])))]


class _Live:
    """One sharded context at a time: each holds a table per virtual rank."""

    def __init__(self):
        self.name, self.c = None, None

    def ctx(self, name, heaps, opts):
        if self.name != name:
            self.close()
            self.c = Context(SUB, (heaps,), device=0)
            for k, v in opts.items():
                self.c.set_option(getattr(_lib, "OPT_" + k), v)
            self.name = name
        return self.c

    def close(self):
        if self.c is not None:
            self.c.close()
        self.name, self.c = None, None


@pytest.fixture(scope="module")
def sharded():
    s = _Live()
    yield s
    s.close()


def test_split_roots_leave_ranks_idle():
    assert sum(split_axes(r) < 3 for r in SPLIT_ROOTS) >= 8   # 8 ranks: three axes
    assert sum(split_axes(r) < 2 for r in SPLIT_ROOTS) >= 4   # 4 ranks: two


@pytest.mark.parametrize("name,chunk", SPLIT_CASES, ids=["%s-%d" % c for c in SPLIT_CASES])
def test_split_box_engine_roots(sharded, oracle, name, chunk):
    """Virtual ranks on one GPU, each on its own table, which the engine allocates and fills with
    0xFF at every prepare (nothing adopted): split axes, owner maps, halo lists and fills all
    follow the root."""
    ranks, opts = SPLIT_CONFIGS[name]
    ctx = sharded.ctx("split-" + name, 8, dict(opts, VIRTUAL_RANKS=ranks))
    for root in _chunks(SPLIT_ROOTS, SPLIT_CHUNK[ranks])[chunk]:
        n, rec = ctx.solve(root)
        st = ctx.stats()
        assert st["engine"] == _lib.ENGINE_DIST_DENSE and st["world"] == ranks
        _check(ctx, oracle, 8, root, n, rec, name)


# ------------------------------------------------------------------ the block engine
BLOCK_CASES = [(h, x4) for h in sorted(ROOTS_H) for x4 in (1, 6, 10)]


def _block_solve(table, ctx, oracle, heaps, root, what):
    table.fill(POISON)
    n, rec = ctx.solve(root)
    assert ctx.stats()["engine"] == _lib.ENGINE_DENSE
    _check(ctx, oracle, heaps, root, n, rec, what, one_gpu=True)


@pytest.fixture(scope="module")
def small_tables():
    """16^h bytes per heap count h < 8."""
    t = {h: _Table(16 ** h) for h in ROOTS_H}
    yield t
    for x in t.values():
        x.free()


@pytest.mark.parametrize("heaps,x4", BLOCK_CASES, ids=["%d-x%d" % c for c in BLOCK_CASES])
def test_block_engine_roots(one_gpu, small_tables, oracle, heaps, x4):
    """3 to 7 heaps: one block per workgroup (GM_OPT_SUB_INTERLEAVE 1), the four-block kernel (6)
    and the walker (10), one context each over the heap count's roots."""
    name = "block-%d-%d" % (heaps, x4)
    ctx = one_gpu.ctx(name, {"SUB_INTERLEAVE": x4}, heaps, small_tables[heaps])
    for root in ROOTS_H[heaps]:
        _block_solve(small_tables[heaps], ctx, oracle, heaps, root, name)
    one_gpu.drop(name)


BLOCK8_ROOTS = every(4)


@pytest.mark.parametrize("chunk", range(len(_chunks(BLOCK8_ROOTS, 13))))
def test_block_engine_8_heaps_roots(one_gpu, oracle, chunk):
    ctx = one_gpu.ctx("block-8", {"SUB_INTERLEAVE": 10})
    for root in _chunks(BLOCK8_ROOTS, 13)[chunk]:
        _block_solve(one_gpu.table, ctx, oracle, 8, root, "block-8")


BLOCK8_RANK_CASES = [(o, i) for o in (0, 1) for i in range(len(_chunks(BLOCK8_ROOTS, 6)))]


@pytest.mark.parametrize("owner,chunk", BLOCK8_RANK_CASES, ids=["owner%d-%d" % c for c in BLOCK8_RANK_CASES])
def test_block_engine_8_heaps_roots_over_4_ranks(sharded, oracle, owner, chunk):
    """The partitioned block engine (csrc/dist_sub.hip) solves the whole table whatever the root;
    what it reports, exports and verifies is the root's region."""
    name = "block-8-ranks4-owner%d" % owner
    ctx = sharded.ctx(name, 8, {"SUB_INTERLEAVE": 10, "DIST_OWNER": owner, "VIRTUAL_RANKS": 4})
    for root in _chunks(BLOCK8_ROOTS, 6)[chunk]:
        n, rec = ctx.solve(root)
        st = ctx.stats()
        assert st["engine"] == _lib.ENGINE_DIST_DENSE and st["world"] == 4
        _check(ctx, oracle, 8, root, n, rec, name)


KNOB_ROOTS = ROOTS_H[5][4:7]   # more than one block: high nibbles above 0
KNOB_CASES = [("SUB_THREADS", v) for v in (64, 128, 256)] + [("SUB_LOW", v) for v in (1, 2, 3)]


@pytest.mark.parametrize("option,value", KNOB_CASES, ids=["%s-%d" % c for c in KNOB_CASES])
def test_block_engine_threads_and_low_heaps(one_gpu, small_tables, oracle, option, value):
    """The one-block kernel's workgroup size and the number of low heaps (5 heaps, interleave 1)."""
    assert all(r >> 12 for r in KNOB_ROOTS)
    name = "block-5-%s-%d" % (option, value)
    ctx = one_gpu.ctx(name, {"SUB_INTERLEAVE": 1, option: value}, 5, small_tables[5])
    for root in KNOB_ROOTS:
        _block_solve(small_tables[5], ctx, oracle, 5, root, name)
    one_gpu.drop(name)


def test_block_sub_low_4_is_refused():
    """GM_OPT_SUB_LOW is 1..3 (include/gmsolve.h): 4 is refused with GM_E_ARG and the context keeps
    its value."""
    ctx = Context(SUB, (5,), device=0)
    with pytest.raises(GMError) as e:
        ctx.set_option(_lib.OPT_SUB_LOW, 4)
    assert e.value.code == GM_E_ARG and "sub_low" in str(e.value)
    ctx.close()
