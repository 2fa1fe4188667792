"""The heap-2/3 mirror of the hybrid schedule's dataflow launches on the GPU (csrc/dense_box.hip,
box_flow_kernel RANGE, bx_store M23): a computed box stores itself and up to seven twins, the 2/3
twins at moved rows, and publishes a flag for each.

The reference is the same root with GM_BOX_HYBRID=0,40 and GM_OPT_SYMMETRY 0: tier launches only,
every box computed.  Equal means: the position count and the root's record, gm_digest, the records
of a key sample that takes keys from every region box (so from every twin) or 4,096 random keys,
gm_verify without a finding, and no dataflow fallback.  The solve under test writes into a table
filled with 0x80 beforehand (tests/box_table.py POISON: no position's code), and whole boxes
outside the region -- the neighbours of the region's boxes and their images under the three swaps
-- must still read 0x80 afterwards.

Small roots, GM_BOX_HYBRID=41,40 (every box-tier in the one dataflow launch); key nibbles 2 and 3
are heaps 2 and 3, four values to a box coordinate:
  0x0000FF00  16 boxes, only 2/3 pairs, one- and two-box groups
  0x0000B700  limits (1, 2): twins outside the region, computed directly
  0x3355FF33  576 boxes, all eight store variants
  0x0031FF00  equal 2/3 limits, a thin region in heaps 4-7: box-tiers of an odd computed count
Mid-size: 0x7777FFFF with 7,17 -- the tier launches read boxes that only twins' stores produced.
Full: 0xFFFFFFFF at the default range, also against the committed C-oracle digest.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from box_table import POISON, _Table
from conftest import GOLDEN
from test_box_mirror import box_coord, box_index_of_key, box_unit, in_region, region_boxes, swap67
from test_box_mirror23 import _partition, swap23
from test_box_mirror45 import swap45

from gamesmanmpi_amd import Context, _lib

pytestmark = pytest.mark.gpu

SUB = 5
ALL_FLOW = "41,40"
SMALL = (0x0000FF00, 0x0000B700, 0x3355FF33, 0x0031FF00)


def test_roots_cover_what_they_are_for():
    for root in SMALL + (0x7777FFFF,):
        rb, r, computed, per_tier, fold = _partition(root)
        if root == 0x0000B700:
            assert fold == {1: 4, 2: 1}
        if root == 0x3355FF33:
            assert set(fold) == {1, 2, 4, 8}
        if root == 0x0031FF00:
            assert (per_tier[per_tier > 0] % 2 == 1).any() and 2 in fold
        if root == 0x7777FFFF:   # tier 6 is the head's last: twins' stores that tier 7's launch reads
            assert int(computed.sum()) < len(r) and per_tier[6] > 0


def _nboxes(root):
    n = 1
    for i in range(8):
        n *= (((root >> (4 * i)) & 15) >> (2 if i < 4 else 1)) + 1
    return n


@functools.lru_cache(maxsize=None)
def _sample_boxes(root):
    """Every region box of a small region; 64 random region boxes of a large one."""
    if _nboxes(root) <= 1024:
        return region_boxes(root)[1]
    rng = np.random.default_rng(root)
    rb = box_index_of_key(root) >> 12
    return sorted({sum(int(rng.integers(0, box_coord(rb, d) + 1)) * box_unit(d) for d in range(8)) for _ in range(64)})


@functools.lru_cache(maxsize=None)
def _keys(root):
    """Small regions: 8 keys of every region box (a twin's rows included); else 4,096 random keys."""
    rng = np.random.default_rng(root)
    lim = [(root >> (4 * i)) & 15 for i in range(8)]
    if _nboxes(root) > 1024:
        k = np.zeros(4096, dtype=np.uint64)
        for i in range(8):
            k |= rng.integers(0, lim[i] + 1, size=4096).astype(np.uint64) << np.uint64(4 * i)
        return k
    out = []
    for b in _sample_boxes(root):
        for _ in range(8):
            k = 0
            for i in range(8):
                c, w = box_coord(b, i), 4 if i < 4 else 2
                k |= int(rng.integers(c * w, min(lim[i], c * w + w - 1) + 1)) << (4 * i)
            out.append(k)
    k = np.array(out, dtype=np.uint64)
    assert sorted(set((box_index_of_key(k.astype(np.int64)) >> 12).tolist())) == _sample_boxes(root)
    return k


@functools.lru_cache(maxsize=None)
def _outside_boxes(root):
    """Whole boxes outside the region that a wrong twin or a wrong neighbour would hit."""
    rb = box_index_of_key(root) >> 12
    out = set()
    for b in _sample_boxes(root):
        for d in range(8):
            if box_coord(b, d) < (3 if d < 4 else 7):
                out.add(b + box_unit(d))
        for v in range(1, 8):
            t = b
            for bit, sw in ((1, swap67), (2, swap45), (4, swap23)):
                if v & bit:
                    t = sw(t)
            out.add(t)
    return sorted(t for t in out if not in_region(t, rb))[:256]


def _env(**kw):
    class _E:
        def __enter__(self):
            os.environ.update(kw)

        def __exit__(self, *a):
            for k in kw:
                del os.environ[k]
    return _E()


def _solve(root, hybrid, symmetry, table=None, ctx=None, **env):
    with _env(GM_BOX_HYBRID=hybrid, **env):
        if ctx is None:
            ctx = Context(SUB, (8,), device=0)
            ctx.set_option(_lib.OPT_SYMMETRY, symmetry)
            ctx.set_option(_lib.OPT_TIMING, 1)
            if table is not None:
                ctx.adopt_dense_table(table.data_ptr(), table.numel())
        n, rec = ctx.solve(root)
    return ctx, n, rec


@functools.lru_cache(maxsize=None)
def _reference(root):
    ctx, n, rec = _solve(root, "0,40", 0)
    ref = (n, rec, ctx.digest(), ctx.query(_keys(root)).tobytes())
    assert ctx.stats()["flow_fallbacks"] == 0
    ctx.close()
    return ref


@pytest.fixture(scope="module")
def scratch_table():
    t = _Table()
    t.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    t.hip.hipMemcpy.restype = ctypes.c_int
    yield t
    t.free()


def _box_bytes(table, box):
    buf = np.empty(4096, np.uint8)
    assert table.hip.hipMemcpy(buf.ctypes.data, table.data_ptr() + (box << 12), 4096, 2) == 0   # device to host
    return buf


def _same(ctx, n, rec, root, table, fallbacks=0):
    rn, rrec, rdig, rq = _reference(root)
    assert (n, rec) == (rn, rrec)
    st = ctx.stats()
    assert st["n_stored"] == st["n_positions"] == rn
    assert ctx.digest() == rdig
    assert ctx.query(_keys(root)).tobytes() == rq
    res, bad = ctx.verify()
    assert res["n_bad"] == 0 and bad == [] and res["root_ok"] == 1 and res["checked"] == rn
    assert st["flow_fallbacks"] == fallbacks
    for b in _outside_boxes(root):
        assert (_box_bytes(table, b) == POISON).all(), hex(b)


@pytest.mark.parametrize("root", SMALL, ids=["%08X" % r for r in SMALL])
def test_every_tier_in_one_dataflow_launch(scratch_table, root):
    """Solved twice on one context: the second solve's epoch must not accept the first's flags."""
    _reference(root)
    scratch_table.fill(POISON)
    ctx, n, rec = _solve(root, ALL_FLOW, 1, scratch_table)
    _same(ctx, n, rec, root, scratch_table)
    scratch_table.fill(POISON)
    _, n2, rec2 = _solve(root, ALL_FLOW, 1, ctx=ctx)
    _same(ctx, n2, rec2, root, scratch_table)
    ctx.close()


def test_tier_launches_read_boxes_that_twins_stored(scratch_table):
    root = 0x7777FFFF
    _reference(root)
    scratch_table.fill(POISON)
    ctx, n, rec = _solve(root, "7,17", 1, scratch_table)
    _same(ctx, n, rec, root, scratch_table)
    assert ctx.stats()["kernel_launches"] == 25
    ctx.close()


def test_full_table_at_the_default_range(scratch_table):
    root = 0xFFFFFFFF
    _reference(root)
    scratch_table.fill(POISON)
    ctx = Context(SUB, (8,), device=0)
    ctx.set_option(_lib.OPT_TIMING, 1)
    ctx.adopt_dense_table(scratch_table.data_ptr(), scratch_table.numel())
    n, rec = ctx.solve(root)
    _same(ctx, n, rec, root, scratch_table)
    ref = json.load(open(os.path.join(GOLDEN, "oracle_digests.json")))["subtract_8"]
    assert ctx.digest() == (ref["digest"], 1 << 32) and rec == ref["root_record"]
    assert ctx.stats()["kernel_launches"] == 41
    ctx.close()


@pytest.mark.parametrize("root,hybrid", [(0x3355FF33, ALL_FLOW), (0x7777FFFF, "7,17")])
def test_fewer_resident_workgroups(scratch_table, root, hybrid):
    """48 KiB of extra dynamic LDS per workgroup (GM_BOX_FLOW_EXTRA_LDS): the grid shrinks to what
    is resident, a workgroup takes several groups of a tier, and a group's children -- twins among
    them -- must come earlier in the queues, not only carry a flag."""
    _reference(root)
    scratch_table.fill(POISON)
    ctx, n, rec = _solve(root, hybrid, 1, scratch_table, GM_BOX_FLOW_EXTRA_LDS=str(48 << 10))
    _same(ctx, n, rec, root, scratch_table)
    ctx.close()


def test_full_lists_without_symmetry(scratch_table):
    """GM_OPT_SYMMETRY 0: the dataflow launch runs over the full list, no entry carries a flag."""
    root = 0x3355FF33
    _reference(root)
    scratch_table.fill(POISON)
    ctx, n, rec = _solve(root, ALL_FLOW, 0, scratch_table)
    _same(ctx, n, rec, root, scratch_table)
    ctx.close()


def test_fallback_resolves_over_the_tier_launches_list(scratch_table):
    """GM_BOX_FLOW_TEST_STALL makes every wait look for an epoch no flag holds: the launch times
    out (20 ms), and the solve is redone by tier launches over the list without the 2/3 flag."""
    root = 0x3355FF33
    _reference(root)
    scratch_table.fill(POISON)
    ctx, n, rec = _solve(root, ALL_FLOW, 1, scratch_table, GM_BOX_FLOW_TEST_STALL="1", GM_BOX_FLOW_TIMEOUT_MS="20")
    _same(ctx, n, rec, root, scratch_table, fallbacks=1)
    ctx.close()
