"""The result node of the one-GPU box solve (csrc/dense_box.hip box_result_kernel): the last node
of every solve -- hybrid schedule, tier launches only, every tier in dataflow launches, the
whole-solve dataflow launch, captured graph or eager launches.  It stores the root's code and the
two dataflow error words into the pinned buffer the host waits for, then zeroes the error words
and moves the epoch on for the next solve; nothing runs in front of a solve's first launch and no
copy behind its last.  So the first solve of a DenseBox relies on the epoch set at prepare, and
every later one on what the solve before it left.

The reference is the same root with GM_BOX_HYBRID=0,40 and GM_OPT_SYMMETRY 0: tier launches only,
every box computed.  Equal means: the position count and the root's record, gm_digest, 4,096
seeded keys of the region, no dataflow fallback, and the root's class equal to the closed form
(LOSS iff the xor over heaps of h mod 3 is 0).  The solve under test writes into a table filled
with 0xEE beforehand, so a box it fails to store cannot show the reference's bytes, and a root
code delivered from anywhere but the solve's own store is not a code.

The roots are the smallest regions where the node can go wrong (tests/test_gpu_box_hybrid.py has
the full table):
  0x33333333  16 boxes, 5 box-tiers;
  0x37733333  9 box-tiers, twins outside the region;
  0x7777FFFF  25 box-tiers, leaders in other XCD queues (one case);
  0x33333332  the top box of 0x33333333 and another root in it (a WIN): one DenseBox serves both,
              and the node must read the code of the root being solved.
"""
import functools
import os

import numpy as np
import pytest

from box_table import _Table

from gamesmanmpi_amd import Context, _lib

pytestmark = pytest.mark.gpu

SUB = 5
TIERS_ONLY, ALL_FLOW = "0,40", "41,40"
# per root: no dataflow state (the node with a null d_flow), every tier in dataflow launches, a
# split range, and a range whose tail launch is the last tier alone
RANGES = {0x33333333: (TIERS_ONLY, ALL_FLOW, "1,3", "2,3"),
          0x37733333: (TIERS_ONLY, ALL_FLOW, "3,5", "6,7"),
          0x7777FFFF: ("10,14",)}
CASES = [(root, r) for root, rs in RANGES.items() for r in rs]


def _closed_form_class(root):
    g = 0
    for i in range(8):
        g ^= ((root >> (4 * i)) & 15) % 3
    return 1 if g == 0 else 0   # the record's class bits: 1 = LOSS


def _tiers(root):
    """Box-tiers of the root's region: 1 + the sum of its top box's coordinates."""
    return 1 + sum(((root >> (4 * i)) & 15) >> 2 for i in range(4)) + sum(((root >> (4 * i)) & 15) >> 1 for i in range(4, 8))


def test_roots_are_what_they_are_for():
    assert [_tiers(r) for r in RANGES] == [5, 9, 25]
    for root, rs in RANGES.items():
        for r in rs:
            if r in (TIERS_ONLY, ALL_FLOW):
                continue
            lo, hi = (int(x) for x in r.split(","))
            assert 0 < lo <= hi < _tiers(root) - 1   # a head launch, tier launches and a tail launch
    assert [int(r.split(",")[1]) for r in (RANGES[0x33333333][3], RANGES[0x37733333][3])] == [3, 7]   # tail: one tier
    assert _closed_form_class(0x33333333) == 1 and _closed_form_class(0x33333332) == 0
    # the same top box: heaps 0-3 four values, heaps 4-7 two values to a box coordinate
    assert (0x33333333 ^ 0x33333332) == 1


def _keys(root):
    rng = np.random.default_rng(root)
    k = np.zeros(4096, dtype=np.uint64)
    for i in range(8):
        k |= rng.integers(0, ((root >> (4 * i)) & 15) + 1, size=4096).astype(np.uint64) << np.uint64(4 * i)
    return k


def _context(symmetry, table=None, graph=1, box_flow=0):
    ctx = Context(SUB, (8,), device=0)
    ctx.set_option(_lib.OPT_SYMMETRY, symmetry)
    if not graph:
        ctx.set_option(_lib.OPT_GRAPH, 0)
    if box_flow:
        ctx.set_option(_lib.OPT_BOX_FLOW, 1)
    if table is not None:
        ctx.adopt_dense_table(table.data_ptr(), table.numel())
    return ctx


def _solve_on(ctx, root, hybrid):
    os.environ["GM_BOX_HYBRID"] = hybrid
    try:
        return ctx.solve(root)
    finally:
        del os.environ["GM_BOX_HYBRID"]


@functools.lru_cache(maxsize=None)
def _reference(root):
    ctx = _context(0)
    n, rec = _solve_on(ctx, root, TIERS_ONLY)
    ref = (n, rec, ctx.digest(), ctx.query([root]).tolist(), ctx.query(_keys(root)).tobytes())
    assert ctx.stats()["flow_fallbacks"] == 0
    ctx.close()
    return ref


@pytest.fixture(scope="module")
def scratch_table():
    t = _Table()
    yield t
    t.free()


def _same(ctx, n, rec, root):
    rn, rrec, rdig, rroot, rq = _reference(root)
    assert (n, rec) == (rn, rrec)
    assert rec >> 14 == _closed_form_class(root)
    assert ctx.digest() == rdig
    assert ctx.query([root]).tolist() == rroot == [rec]
    assert ctx.query(_keys(root)).tobytes() == rq
    assert ctx.stats()["flow_fallbacks"] == 0


@pytest.mark.parametrize("root,hybrid", CASES, ids=["%08X-%s" % c for c in CASES])
def test_result_node_of_every_schedule(scratch_table, root, hybrid):
    _reference(root)
    scratch_table.fill(0xEE)
    ctx = _context(1, scratch_table)
    n, rec = _solve_on(ctx, root, hybrid)
    _same(ctx, n, rec, root)
    ctx.close()


@pytest.mark.parametrize("root,hybrid", [(0x33333333, "1,3"), (0x37733333, ALL_FLOW), (0x37733333, "6,7")])
def test_three_solves_in_a_row(scratch_table, root, hybrid):
    """The epoch advances at the end of a solve: solves 2 and 3 replay the captured graph, must not
    accept the flags of the solves before them (the table is refilled, so a group that did not
    wait reads 0xEE) and must find the error words zero (a stale one ends every wait: a fallback)."""
    _reference(root)
    ctx = _context(1, scratch_table)
    ctx.set_option(_lib.OPT_TIMING, 1)
    for _ in range(3):
        scratch_table.fill(0xEE)
        n, rec = _solve_on(ctx, root, hybrid)
        _same(ctx, n, rec, root)
    assert ctx.stats()["kernel_launches"] == _tiers(root)   # the box-tier count, the node not counted
    ctx.close()


@pytest.mark.parametrize("hybrid", ["1,3", TIERS_ONLY])
def test_roots_a_b_a_on_one_context(scratch_table, hybrid):
    """Every root change builds a fresh DenseBox, whose first solve relies on the epoch set at
    prepare (its flags are fresh: zero)."""
    ctx = _context(1, scratch_table)
    for root in (0x33333333, 0x37733333, 0x33333333):
        _reference(root)
        scratch_table.fill(0xEE)
        n, rec = _solve_on(ctx, root, hybrid)
        _same(ctx, n, rec, root)
    ctx.close()


@pytest.mark.parametrize("hybrid", ["1,3", TIERS_ONLY])
def test_two_roots_of_one_top_box(scratch_table, hybrid):
    """0x33333333 (LOSS) and 0x33333332 (WIN) share their top box, so one DenseBox and its lists
    serve both; the node's address of the root's code and the tier counts are the root's own."""
    ctx = _context(1, scratch_table)
    for root in (0x33333333, 0x33333332, 0x33333333):
        _reference(root)
        scratch_table.fill(0xEE)
        n, rec = _solve_on(ctx, root, hybrid)
        _same(ctx, n, rec, root)
        counts = ctx.tier_counts()
        assert int(sum(counts)) == n and len(counts) == 1 + sum((root >> (4 * i)) & 15 for i in range(8))
    ctx.close()


def test_eager_launches(scratch_table):
    """GM_OPT_GRAPH 0: the same nodes enqueued on the stream, twice (the second solve's epoch is the
    first solve's result node's)."""
    root = 0x37733333
    _reference(root)
    ctx = _context(1, scratch_table, graph=0)
    for _ in range(2):
        scratch_table.fill(0xEE)
        n, rec = _solve_on(ctx, root, "3,5")
        _same(ctx, n, rec, root)
    ctx.close()


def test_whole_solve_dataflow_launch(scratch_table):
    """GM_OPT_BOX_FLOW 1: one dataflow launch and the result node, three times."""
    root = 0x37733333
    _reference(root)
    ctx = _context(1, scratch_table, box_flow=1)
    ctx.set_option(_lib.OPT_TIMING, 1)
    for _ in range(3):
        scratch_table.fill(0xEE)
        n, rec = ctx.solve(root)
        _same(ctx, n, rec, root)
    assert ctx.stats()["kernel_launches"] == 1
    ctx.close()
