"""The hybrid schedule of the one-GPU box solve (csrc/dense_box.hip, GM_BOX_HYBRID=lo,hi): the
thin box-tiers [0, lo) and (hi, 40] each run as one dataflow launch over the compute list --
mirrored stores, a flag for every box stored, its twins included -- and [lo, hi] as tier launches.

The reference is the same root with GM_BOX_HYBRID=0,40 and GM_OPT_SYMMETRY 0: tier launches only,
every box computed.  Equal means: gm_digest and the position count, the root's record, 4,096
random keys of the region, and no dataflow fallback.  The hybrid solve writes into a table filled
with 0xEE beforehand, so a box it fails to store cannot show the reference's bytes.

The roots (key nibbles 0-3 are the A heaps, four values to a box coordinate; nibbles 4-7 the B
heaps 4-7, two values to a box coordinate; the mirrors exchange heaps 4/5 and heaps 6/7):
  0x33333333  one box per A coordinate, 2^4 B boxes, 5 box-tiers: twins through both mirrors;
  0x37733333  B limits (heap 4..7) 1, 3, 3, 1 and
  0x73373333  B limits 3, 1, 1, 3: both mirror pairs have unequal limits, so a twin may fall
              outside the region and is then computed directly (9 box-tiers);
  0x7777FFFF  65,536 boxes in 25 box-tiers: mirrored-to boxes whose leader is in another XCD queue;
  0xFFFFFFFF  the full table, also against the committed C-oracle digest.

Ranges per root of T box-tiers: the candidates (7, 33), (10, 30), (12, 28) and the default (14, 26) keep `lo` tiers at
either end, so clipped to T they are (lo, T - 1 - lo), or every tier in the head launch when
2 lo >= T (where that holds for all of them, T // 3 tiers at either end is run as well); plus 41,40 (every tier in dataflow
launches) and one range whose tail is the last tier alone.
"""
import functools
import json
import os

import numpy as np
import pytest

from box_table import _Table
from conftest import GOLDEN

from gamesmanmpi_amd import Context, _lib

pytestmark = pytest.mark.gpu

SUB = 5
CANDIDATES = (7, 10, 12, 14)   # the three the schedule was proposed with, and the default (14, 26)
ALL_FLOW = "41,40"


def _tiers(root):
    """Box-tiers of the root's region: 1 + the sum of its top box's coordinates."""
    return 1 + sum(((root >> (4 * i)) & 15) >> 2 for i in range(4)) + sum(((root >> (4 * i)) & 15) >> 1 for i in range(4, 8))


def _ranges(root):
    t = _tiers(root)
    out = []
    for lo in CANDIDATES:
        r = "%d,%d" % (lo, t - 1 - lo) if 2 * lo < t else ALL_FLOW
        if r not in out:
            out.append(r)
    if out == [ALL_FLOW]:   # too few tiers for any candidate: a third of them at either end
        out.append("%d,%d" % (t // 3, t - 1 - t // 3))
    elif ALL_FLOW not in out:
        out.append(ALL_FLOW)
    out.append("%d,%d" % (min(CANDIDATES[0], t - 3), t - 2))   # the tail launch: the last tier alone
    return out


ROOTS = (0x33333333, 0x37733333, 0x73373333, 0x7777FFFF, 0xFFFFFFFF)
CASES = [(root, r) for root in ROOTS for r in _ranges(root)]


def test_ranges_cover_what_the_roots_are_for():
    assert [_tiers(r) for r in ROOTS] == [5, 9, 9, 25, 41]
    assert _ranges(0xFFFFFFFF) == ["7,33", "10,30", "12,28", "14,26", ALL_FLOW, "7,39"]
    assert _ranges(0x7777FFFF) == ["7,17", "10,14", "12,12", ALL_FLOW, "7,23"]
    assert _ranges(0x33333333) == [ALL_FLOW, "1,3", "2,3"]
    assert _ranges(0x37733333) == [ALL_FLOW, "3,5", "6,7"]
    for root in (0x37733333, 0x73373333):   # unequal limits inside both mirror pairs
        lim = [((root >> (4 * i)) & 15) >> 1 for i in range(4, 8)]
        assert lim[0] != lim[1] and lim[2] != lim[3]


def _keys(root):
    rng = np.random.default_rng(root)
    k = np.zeros(4096, dtype=np.uint64)
    for i in range(8):
        k |= rng.integers(0, ((root >> (4 * i)) & 15) + 1, size=4096).astype(np.uint64) << np.uint64(4 * i)
    return k


def _solve(root, hybrid, symmetry, table=None):
    os.environ["GM_BOX_HYBRID"] = hybrid
    try:
        ctx = Context(SUB, (8,), device=0)
        ctx.set_option(_lib.OPT_SYMMETRY, symmetry)
        if table is not None:
            ctx.adopt_dense_table(table.data_ptr(), table.numel())
        n, rec = ctx.solve(root)
    finally:
        del os.environ["GM_BOX_HYBRID"]
    return ctx, n, rec


@functools.lru_cache(maxsize=None)
def _reference(root):
    ctx, n, rec = _solve(root, "0,40", 0)
    ref = (n, rec, ctx.digest(), ctx.query([root]).tolist(), ctx.query(_keys(root)).tobytes())
    assert ctx.stats()["flow_fallbacks"] == 0
    ctx.close()
    return ref


@pytest.fixture(scope="module")
def scratch_table():
    t = _Table()
    yield t
    t.free()


def _fill(table):
    table.fill(0xEE)


def _same(ctx, n, rec, root):
    rn, rrec, rdig, rroot, rq = _reference(root)
    assert (n, rec) == (rn, rrec)
    assert ctx.digest() == rdig
    assert ctx.query([root]).tolist() == rroot
    assert ctx.query(_keys(root)).tobytes() == rq
    assert ctx.stats()["flow_fallbacks"] == 0


@pytest.mark.parametrize("root,hybrid", CASES, ids=["%08X-%s" % c for c in CASES])
def test_hybrid_equals_tier_launches_of_every_box(scratch_table, root, hybrid):
    _reference(root)
    _fill(scratch_table)
    ctx, n, rec = _solve(root, hybrid, 1, scratch_table)
    _same(ctx, n, rec, root)
    if root == 0xFFFFFFFF:
        ref = json.load(open(os.path.join(GOLDEN, "oracle_digests.json")))["subtract_8"]
        assert ctx.digest() == (ref["digest"], 1 << 32) and rec == ref["root_record"]
    ctx.close()


@pytest.mark.parametrize("root,hybrid", [(0x37733333, "3,5"), (0x7777FFFF, "10,14")])
def test_hybrid_with_full_lists(scratch_table, root, hybrid):
    """GM_OPT_SYMMETRY 0: both kinds of launch run over the full lists (no mirrored store)."""
    _reference(root)
    _fill(scratch_table)
    ctx, n, rec = _solve(root, hybrid, 0, scratch_table)
    _same(ctx, n, rec, root)
    ctx.close()


@pytest.mark.parametrize("root,hybrid", [(0x7777FFFF, "7,17"), (0xFFFFFFFF, "14,26")])
def test_hybrid_twice_on_one_context(scratch_table, root, hybrid):
    """Two solves in a row replay the captured graph: the second solve's epoch must not accept the
    first solve's flags, and the error words are reset.  The table is refilled in between, so the
    second solve's boxes are its own.  The launch count stays the box-tier count."""
    _reference(root)
    _fill(scratch_table)
    ctx, n, rec = _solve(root, hybrid, 1, scratch_table)
    ctx.set_option(_lib.OPT_TIMING, 1)
    _same(ctx, n, rec, root)
    _fill(scratch_table)
    os.environ["GM_BOX_HYBRID"] = hybrid
    try:
        n2, rec2 = ctx.solve(root)
    finally:
        del os.environ["GM_BOX_HYBRID"]
    _same(ctx, n2, rec2, root)
    assert ctx.stats()["kernel_launches"] == _tiers(root)
    ctx.close()


def test_hybrid_range_is_checked():
    os.environ["GM_BOX_HYBRID"] = "7;33"
    try:
        ctx = Context(SUB, (8,), device=0)
        with pytest.raises(_lib.GMError) as e:
            ctx.solve(0x33333333)
        assert e.value.code == -1 and "GM_BOX_HYBRID" in str(e.value)   # GM_E_ARG
        ctx.close()
    finally:
        del os.environ["GM_BOX_HYBRID"]
