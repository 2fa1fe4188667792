"""The third mirror of the box engine, heaps 2 and 3 (csrc/box_common.hpp bx_swap23 /
bx_mirror_class23, used by the hybrid schedule's dataflow launches), pinned on the host before any
kernel runs.

Heaps 2 and 3 are A heaps: the fields c2 (bits 4-5) and c3 (bits 6-7) of the box id, and the
digits at bits 4-5 and 6-7 of the row index A.  swap23(C) exchanges the two fields; its row
swap_row(m) (m with the two digits exchanged) holds the 16 bytes of row m of C unchanged.  A box
has one class per mirror (0 its own, 1 also stores its twin, 2 mirrored-to); it is computed iff no
class is 2, and stores itself and every composition of its flagged swaps, up to eight boxes."""
import functools

import numpy as np
import pytest

from test_box_mirror import box_coord, box_index_of_key, in_region, mirror_class, oracle_boxes, region_boxes, swap67
from test_box_mirror45 import box_tier, mirror_class45, rows45, rows67, swap45

ROOTS = [0xFFFFFFFF, 0x0000FF00, 0x0000B700, 0x00003F00, 0x3355FF33]


def swap23(box):
    """Python twin of bx_swap23 (ints or numpy arrays)."""
    t = ((box >> 4) ^ (box >> 6)) & 3
    return box ^ (t << 4) ^ (t << 6)


def swap_row(m):
    """bx_swap_row for the transposition of heaps 2 and 3: digits at bits 4-5 and 6-7 of A."""
    t = ((m >> 4) ^ (m >> 6)) & 3
    return m ^ (t << 4) ^ (t << 6)


def mirror_class23(box, root_box):
    """Python twin of bx_mirror_class23."""
    c2, c3 = box_coord(box, 2), box_coord(box, 3)
    if c2 == c3 or not in_region(swap23(box), root_box):
        return 0
    return 1 if c2 > c3 else 2


SWAPS = (swap67, swap45, swap23)            # variant bit 0, 1, 2 (bx_twin_box)
CLASSES = (mirror_class, mirror_class45, mirror_class23)


def stores_of(box, root_box):
    """The boxes a region box stores (empty: not computed): the rule of box_compute_list with all
    three mirrors and of bx_store M23 -- itself and every composition of its flagged swaps."""
    cls = [f(box, root_box) for f in CLASSES]
    if 2 in cls:
        return []
    out = []
    for v in range(8):
        if all(cls[i] == 1 for i in range(3) if v >> i & 1):
            t = box
            for i in range(3):
                if v >> i & 1:
                    t = SWAPS[i](t)
            out.append(t)
    return out


# the same rule over numpy arrays of boxes (the full root has 2^20)
def _coord(b, d):
    return (b >> (2 * d)) & 3 if d < 4 else (b >> (8 + 3 * (d - 4))) & 7


def _in_region(b, rb):
    ok = np.ones(b.shape, bool)
    for d in range(8):
        ok &= _coord(b, d) <= box_coord(rb, d)
    return ok


def _class(b, rb, d0, d1, swap):
    c0, c1 = _coord(b, d0), _coord(b, d1)
    return np.where((c0 == c1) | ~_in_region(swap(b), rb), 0, np.where(c0 > c1, 1, 2))


@functools.lru_cache(maxsize=None)
def _partition(root):
    """(region, computed mask, per-tier computed counts); asserts the partition."""
    rb, region = region_boxes(root)
    r = np.array(region, np.int64)
    cls = [_class(r, rb, 6, 7, swap67), _class(r, rb, 4, 5, swap45), _class(r, rb, 2, 3, swap23)]
    computed = (cls[0] != 2) & (cls[1] != 2) & (cls[2] != 2)
    tier = sum(_coord(r, d) for d in range(8))
    writes = np.zeros(1 << 20, np.int64)
    fold = {}
    nst = np.zeros(r.shape, np.int64)
    for v in range(8):
        on = computed.copy()
        t = r.copy()
        for i in range(3):
            if v >> i & 1:
                on &= cls[i] == 1
                t = SWAPS[i](t)
        assert _in_region(t[on], rb).all(), "a store outside the region"
        assert (sum(_coord(t, d) for d in range(8))[on] == tier[on]).all(), "a twin outside its leader's box-tier"
        np.add.at(writes, t[on], 1)
        nst += on
    inside = np.zeros(1 << 20, bool)
    inside[r] = True
    assert (writes[inside] == 1).all(), "every region box is written exactly once"
    assert (writes[~inside] == 0).all(), "nothing outside the region is written"
    for n in np.unique(nst[computed]).tolist():
        fold[n] = int((nst[computed] == n).sum())
    assert set(fold) <= {1, 2, 4, 8} and sum(k * n for k, n in fold.items()) == len(region)
    return rb, r, computed, np.bincount(tier[computed], minlength=41), fold


@pytest.mark.parametrize("root", ROOTS + [0x9ABCDEF1, 0x12345678, 0x7777FFFF, 0x0031FF00])
def test_three_class_rule_partitions_the_region(root):
    """Computed boxes plus their flagged stores write every region box exactly once and nothing
    outside the region; every twin keeps the box-tier."""
    rb, r, computed, per_tier, fold = _partition(root)
    if root == 0x0000FF00:      # limits (3, 3): 10 of the 16 (c2, c3) pairs computed, 6 flagged
        assert (len(r), int(computed.sum()), fold) == (16, 10, {1: 4, 2: 6})
    if root == 0x0000B700:      # limits (1, 2): only (0, 1) / (1, 0) has its twin in the region
        assert (len(r), int(computed.sum()), fold) == (6, 5, {1: 4, 2: 1})
    if root == 0x00003F00:      # limits (3, 0): no twin in the region, every box computed
        assert (len(r), int(computed.sum()), fold) == (4, 4, {1: 4})
    if root == 0x3355FF33:      # 4 x 4 x 3 x 3 x 2 x 2 boxes, all eight store variants
        assert len(r) == 576 and int(computed.sum()) == 10 * 6 * 3 and fold[8] == 6 * 3 * 1
    if root == 0x0031FF00:      # a thin region in heaps 4-7: a box-tier with an odd computed count
        assert (per_tier[per_tier > 0] % 2 == 1).any()


@pytest.mark.parametrize("root", [0x0000FF00, 0x0000B700, 0x00003F00, 0x3355FF33, 0x12345678])
def test_array_rule_is_the_scalar_rule(root):
    """The numpy form above against the scalar twins of bx_mirror_class67 / 45 / 23, box by box."""
    rb, region = region_boxes(root)
    writes = dict.fromkeys(region, 0)
    n = 0
    for c in region:
        st = stores_of(c, rb)
        assert len(set(st)) == len(st)
        n += bool(st)
        for t in st:
            assert box_tier(t) == box_tier(c)
            writes[t] += 1    # KeyError: a store outside the region
    assert set(writes.values()) == {1}
    assert n == int(_partition(root)[2].sum())


def test_full_game_computes_207360_boxes_and_the_ramp_tiers_groups():
    """With every limit the largest: 10 of the 16 (c2, c3) pairs, 36 x 36 of the (c4, c5, c6, c7)
    tuples, times the 16 boxes of heaps 0 and 1.  The groups (box pairs) of the ramp tiers are what
    the dataflow launches' resident rounds are counted from."""
    rb, r, computed, per_tier, fold = _partition(0xFFFFFFFF)
    assert (len(r), int(computed.sum())) == (1 << 20, 207360) and 207360 == 10 * 1296 * 16
    assert ((per_tier[10:14] + 1) // 2).tolist() == [1447, 2012, 2682, 3437]
    assert (per_tier == per_tier[::-1]).all()                 # the tail tiers 27-30 mirror the head's
    assert int(per_tier[:14].sum()) == int(per_tier[27:].sum()) == 24140
    assert fold[8] == 6 * 28 * 28 * 16


ROW = swap_row(np.arange(256))


def test_swap_row_exchanges_digits_2_and_3():
    assert sorted(ROW.tolist()) == list(range(256)) and (ROW[ROW] == np.arange(256)).all()
    for m in (0x00, 0x1B, 0x6C, 0xE4, 0xFF):
        a = [(m >> (2 * i)) & 3 for i in range(4)]
        assert ROW[m] == a[0] | a[1] << 2 | a[3] << 4 | a[2] << 6
    # 16 consecutive rows (256 B) stay consecutive
    assert (ROW.reshape(16, 16) - ROW.reshape(16, 16)[:, :1] == np.arange(16)).all()


@pytest.mark.parametrize("root", [0x11117733, 0x1111B733, 0x33337733])
def test_swap23_box_is_the_twin_with_its_rows_moved(oracle, root):
    """Row swap_row(m) of swap23(C) equals row m of C, alone and composed with the byte
    permutations of the 4/5 and 6/7 mirrors, on boxes the C oracle solved.  (These roots' A heaps
    end a quarter and their B heaps are odd, so their boxes are whole.)"""
    rb, region = region_boxes(root)
    tab = oracle_boxes(oracle, root)
    assert sorted(tab) == region
    pairs = moved = 0
    for c in region:
        assert (tab[c] != 0xFFFF).all()
        for v in (4, 5, 6, 7):
            t, img = swap23(c), tab[c].reshape(256, 4, 4)
            if v & 1:
                t, img = swap67(t), rows67(img)
            if v & 2:
                t, img = swap45(t), rows45(img)
            if not in_region(t, rb):
                continue
            assert np.array_equal(tab[t].reshape(256, 4, 4)[ROW], img), (hex(c), hex(t), v)
            pairs += 1
            moved += t != c and not np.array_equal(tab[t], tab[c])
    if root == 0x11117733:
        assert pairs == 4 * 4                  # one B box: every variant is the 2/3 twin, all four boxes
    if root == 0x1111B733:
        assert pairs == 4 * 4                  # limits (1, 2): (0,0), (1,1), (0,1), (1,0) of six boxes
    if root == 0x33337733:
        assert pairs == 4 * 64 and moved > 0


def test_box_index_digits():
    """The layout the row rule rests on: heap 2 (3) is bits 4-5 (6-7) of A and of the box id."""
    for h2, h3 in ((5, 14), (15, 0), (9, 6)):
        x = box_index_of_key(h2 << 8 | h3 << 12)
        assert (x >> 4 >> 4) & 3 == h2 & 3 and (x >> 4 >> 6) & 3 == h3 & 3
        assert box_coord(x >> 12, 2) == h2 >> 2 and box_coord(x >> 12, 3) == h3 >> 2
