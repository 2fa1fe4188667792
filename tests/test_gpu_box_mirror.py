"""The box engine's heap-6/7 mirror on the GPU (csrc/dense_box.hip, GM_OPT_SYMMETRY): the tier
kernel computes one box of each mirror pair and stores both.  Small roots, each chosen for a way
the mirrored store can go wrong; every result is compared bit-exactly with the block engine
(GM_OPT_SUB_INTERLEAVE 10, no mirror anywhere) and with the box engine computing every box
(GM_OPT_SYMMETRY 0).

  0x33000000              four boxes, one mirrored, single-box groups
  0x53000000, 0x35000000  unequal limits both ways: twins outside the region are computed
                          directly, nothing outside the region is written
  0xFF000000              64 boxes over 15 box-tiers: diagonal boxes, odd tier sizes, groups
                          mixing flagged and unflagged boxes
  0x77110011, 0xFF330033  children along A and B heaps that land in mirrored boxes
  0x9ABCDEF1              a large uneven region

About 4 s per root on an MI355X, nearly all of it the block engine's reference solve (the box
engine's solves, digests and exports of the small roots take milliseconds); 0x9ABCDEF1 about
10 s with its four exports of 115 M records."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_box_mirror import box_coord, in_region, mirror_class, region_boxes, swap67

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu

from gamesmanmpi_amd import Context, _lib  # noqa: E402

SUB = 5
ROOTS = [0x33000000, 0x53000000, 0x35000000, 0xFF000000, 0x77110011, 0xFF330033, 0x9ABCDEF1]


def _box_tiers(root):
    return sum(((root >> (4 * j)) & 15) >> (2 if j < 4 else 1) for j in range(8)) + 1


def _positions(root):
    n = 1
    for j in range(8):
        n *= ((root >> (4 * j)) & 15) + 1
    return n


def _result(ctx, root):
    """Everything a solve of `root` on `ctx` gives: count, root record, digest, exported records."""
    n, rec = ctx.solve(root)
    launches = ctx.stats()["kernel_launches"]
    dg = ctx.digest()
    keys, recs = ctx.export()
    assert len(keys) == n and (keys[0], keys[-1]) == (0, root)
    return {"n": n, "rec": rec, "digest": dg, "recs": recs, "launches": launches}


def _same(a, b):
    return (a["n"], a["rec"], a["digest"]) == (b["n"], b["rec"], b["digest"]) and np.array_equal(a["recs"], b["recs"])


@pytest.fixture(scope="module")
def block_engine():
    """One block-engine context (no mirror anywhere) for every root's reference."""
    blk = Context(SUB, (8,), device=0)
    blk.set_option(_lib.OPT_SUB_INTERLEAVE, 10)
    yield blk
    blk.close()


@pytest.mark.parametrize("root", ROOTS)
def test_mirror_equals_block_engine_and_every_box_computed(block_engine, root):
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


def test_mirror_is_the_default():
    """A fresh context mirrors without the option being set: same table as with it off."""
    root = 0xFF000000
    a = Context(SUB, (8,), device=0)
    ra = _result(a, root)
    a.close()
    b = Context(SUB, (8,), device=0)
    b.set_option(_lib.OPT_SYMMETRY, 0)
    rb = _result(b, root)
    b.close()
    assert _same(ra, rb)


@pytest.fixture(scope="module")
def adopted():
    """{root: the child's report}: both roots solved into one torch tensor, in a process of its
    own where torch comes first, as in bench.py (torch and the library each bring a HIP runtime)."""
    roots = [0x35000000, 0x53000000]
    r = subprocess.run([sys.executable, os.path.join(HERE, "box_mirror_adopt.py")] + ["%x" % x for x in roots],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert [d["root"] for d in out] == roots
    return {d["root"]: d for d in out}


@pytest.mark.parametrize("root", [0x35000000, 0x53000000])
def test_adopted_table_nothing_written_outside_the_region(adopted, root):
    """A caller's table (torch.uint8, 2^32 bytes) pre-filled with 0xEE: after the solve every byte
    outside the region's boxes is still 0xEE, the region's boxes are stored whole, and each
    mirrored-to box is its twin with dwords 1 and 2 of every row exchanged (no code of these
    regions is 0xEE: remoteness <= 8)."""
    d = adopted[root]
    rb, region = region_boxes(root)
    assert d["n"] == _positions(root) and d["touched"] == region and d["whole"]
    mirrored = [b for b in region if mirror_class(b, rb) == 2]
    assert mirrored and all(in_region(swap67(b), rb) and box_coord(b, 6) < box_coord(b, 7) for b in mirrored)
    assert d["mirrored"] == mirrored and d["differ"] == []
    assert d["n_bad"] == 0 and d["checked"] == d["n"]
