"""The box engine's two mirrors on the GPU (csrc/dense_box.hip, GM_OPT_SYMMETRY): the tier kernel
computes one box of each heap-6/7 pair and of each heap-4/5 pair and stores up to four.  Small
roots, each chosen for a way the store can go wrong; every result is compared bit-exactly with
the block engine (GM_OPT_SUB_INTERLEAVE 10, no mirror anywhere) and with the box engine computing
every box (GM_OPT_SYMMETRY 0).

  0x00330000              a single 4/5 pair, one-box groups
  0x00530000, 0x00350000  the twin outside the region, both ways: every box computed directly
  0x33330000              four-fold, two-fold and single stores side by side in one box-tier
  0x35530000              unequal limits on both pairs
  0x00FF0000, 0xFFFF0000  diagonals, odd tier sizes, groups mixing all four flag states
  0x77770011, 0x33FF0033  children along A and B heaps landing in mirrored-to boxes
  0x24640000              even limits

A few seconds per root on an MI355X, nearly all of it the block engine's reference solve."""
import json
import os
import subprocess
import sys

import pytest

from test_box_mirror import region_boxes
from test_box_mirror45 import representative
from test_gpu_box_mirror import _box_tiers, _positions, _result, _same

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu

from gamesmanmpi_amd import Context, _lib  # noqa: E402

SUB = 5
ROOTS = [0x00330000, 0x00530000, 0x00350000, 0x33330000, 0x35530000, 0x00FF0000, 0xFFFF0000, 0x77770011, 0x33FF0033,
         0x24640000]


@pytest.fixture(scope="module")
def block_engine():
    """One block-engine context (no mirror anywhere) for every root's reference."""
    blk = Context(SUB, (8,), device=0)
    blk.set_option(_lib.OPT_SUB_INTERLEAVE, 10)
    yield blk
    blk.close()


@pytest.mark.parametrize("root", ROOTS)
def test_both_mirrors_equal_block_engine_and_every_box_computed(block_engine, root):
    ref = _result(block_engine, root)
    assert ref["n"] == _positions(root)

    ctx = Context(SUB, (8,), device=0)
    ctx.set_option(_lib.OPT_TIMING, 1)
    for sym in (1, 0, 1):   # the default, every box computed, and back: one context, lists rebuilt
        ctx.set_option(_lib.OPT_SYMMETRY, sym)
        got = _result(ctx, root)
        assert _same(got, ref), (hex(root), sym)
        assert got["launches"] == _box_tiers(root), (hex(root), sym)
        st = ctx.stats()
        assert st["engine"] == _lib.ENGINE_DENSE and st["n_stored"] == ref["n"]
        res, bad = ctx.verify()
        assert res["n_bad"] == 0 and bad == [] and res["root_ok"] == 1 and res["checked"] == ref["n"]
    ctx.close()


@pytest.fixture(scope="module")
def adopted():
    """{root: the child's report}: both roots solved into one torch tensor, in a process of its
    own where torch comes first, as in bench.py (torch and the library each bring a HIP runtime)."""
    roots = [0x35530000, 0x53350000]
    r = subprocess.run([sys.executable, os.path.join(HERE, "box_mirror45_adopt.py")] + ["%x" % x for x in roots],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert [d["root"] for d in out] == roots
    return {d["root"]: d for d in out}


@pytest.mark.parametrize("root", [0x35530000, 0x53350000])
def test_adopted_table_nothing_written_outside_the_region(adopted, root):
    """A caller's table (torch.uint8, 2^32 bytes) pre-filled with 0xEE: after the solve only the
    region's boxes hold other bytes, each of them is stored whole, and each box that is not
    computed equals its computed representative under the row permutation of its mirrors (no code
    of these regions is 0xEE: remoteness <= 16)."""
    d = adopted[root]
    rb, region = region_boxes(root)
    assert d["n"] == _positions(root) and d["touched"] == region and d["whole"]
    not_computed = [b for b in region if representative(b, rb)[0] != b]
    # 36 boxes; per pair of heaps 5 of the 6 coordinate pairs are computed (limits 1 and 2: only
    # (0, 1) / (1, 0) has its twin in the region), so 25 boxes are computed and 11 are not
    assert len(region) == 36 and len(not_computed) == 11
    assert d["not_computed"] == not_computed and d["differ"] == []
    assert d["n_bad"] == 0 and d["checked"] == d["n"]
