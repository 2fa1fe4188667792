"""The two mirrors of the box engine together (csrc/box_common.hpp, csrc/dense_box.hip), pinned
on the host before any kernel runs: heaps 6/7 (tests/test_box_mirror.py) and heaps 4/5.

Heaps 4 and 5 are bits 0 and 1 of B and the fields c4 (bits 8-10) and c5 (bits 11-13) of the box
id.  swap45(C) exchanges the two fields; its row m (16 bytes, one A) is row m of C with bytes 1
and 2 of each dword exchanged.  A box has one class per mirror (0 its own, 1 also stores its
twin, 2 mirrored-to); it is computed iff neither class is 2, and stores itself, its 6/7 twin, its
4/5 twin and the twin through both according to its two flags."""
import numpy as np
import pytest

from test_box_mirror import box_coord, in_region, mirror_class, oracle_boxes, region_boxes, swap67


def swap45(box):
    t = ((box >> 8) ^ (box >> 11)) & 7
    return box ^ (t << 8) ^ (t << 11)


def mirror_class45(box, root_box):
    """Python twin of bx_mirror_class45."""
    c4, c5 = box_coord(box, 4), box_coord(box, 5)
    if c4 == c5 or not in_region(swap45(box), root_box):
        return 0
    return 1 if c4 > c5 else 2


def stores_of(box, root_box):
    """The boxes a region box stores (empty: it is not computed), the rule of box_compute_list
    and bx_store: itself, and its twins by its flags."""
    c67, c45 = mirror_class(box, root_box), mirror_class45(box, root_box)
    if c67 == 2 or c45 == 2:
        return []
    out = [box]
    if c67 == 1:
        out.append(swap67(box))
    if c45 == 1:
        out.append(swap45(box))
    if c67 == 1 and c45 == 1:
        out.append(swap45(swap67(box)))
    return out


def representative(box, root_box):
    """(computed box that stores `box`, through 6/7?, through 4/5?)."""
    m67, m45 = mirror_class(box, root_box) == 2, mirror_class45(box, root_box) == 2
    c = swap67(box) if m67 else box
    return (swap45(c) if m45 else c), m67, m45


def box_tier(box):
    return sum(box_coord(box, d) for d in range(8))


def rows45(a):
    """Rows (256 x 4 dwords x 4 bytes) with bytes 1 and 2 of each dword exchanged."""
    return a.reshape(256, 4, 4)[:, :, [0, 2, 1, 3]]


def rows67(a):
    return a.reshape(256, 4, 4)[:, [0, 2, 1, 3], :]


@pytest.mark.parametrize("root", [0x00330000, 0x00FF0000, 0x33330000])
def test_swap45_box_is_the_twin_with_bytes_1_and_2_of_each_dword_exchanged(oracle, root):
    """(These roots' heaps 4 and 5 are odd, so their boxes are whole along both.)"""
    rb, region = region_boxes(root)
    tab = oracle_boxes(oracle, root)
    assert sorted(tab) == region
    pairs = 0
    for c in region:
        t = swap45(c)
        if not in_region(t, rb):
            continue
        assert np.array_equal(tab[t].reshape(256, 4, 4), rows45(tab[c])), (hex(c), hex(t))
        assert (tab[t] != 0xFFFF).any()
        pairs += 1
    assert pairs == len(region)   # equal limits on heaps 4 and 5: every twin is in the region


def test_swap45_of_swap67_is_both_permutations(oracle):
    root = 0x33330000
    rb, region = region_boxes(root)
    tab = oracle_boxes(oracle, root)
    assert len(region) == 16
    for c in region:
        t = swap45(swap67(c))
        assert in_region(t, rb) and t == swap67(swap45(c))
        both = rows45(rows67(tab[c]))
        assert np.array_equal(tab[t].reshape(256, 4, 4), both), (hex(c), hex(t))
        assert np.array_equal(both, rows67(rows45(tab[c])))


def _check_partition(region, rb):
    writes = dict.fromkeys(region, 0)
    computed, fold = 0, {1: 0, 2: 0, 4: 0}
    for c in region:
        st = stores_of(c, rb)
        if not st:
            assert representative(c, rb)[0] != c
            continue
        computed += 1
        fold[len(st)] += 1
        assert len(set(st)) == len(st)
        for t in st:
            assert t in writes, "a store outside the region"
            assert box_tier(t) == box_tier(c)
            assert representative(t, rb)[0] == c
            writes[t] += 1
    assert set(writes.values()) == {1}
    assert fold[1] + 2 * fold[2] + 4 * fold[4] == len(region)
    return computed, fold


@pytest.mark.parametrize("root", [0x00330000, 0x00530000, 0x00350000, 0x33330000, 0x35530000, 0x24640000, 0x9ABCDEF1,
                                  0x12345678])
def test_two_class_rule_partitions_the_region(root):
    """Computed boxes plus their flagged stores write every region box exactly once and nothing
    outside the region; every twin keeps the box-tier."""
    rb, region = region_boxes(root)
    computed, fold = _check_partition(region, rb)
    if root == 0x00330000:
        assert (len(region), computed) == (4, 3)
    if root == 0x33330000:
        assert (len(region), computed, fold[4]) == (16, 9, 1)
    if root in (0x00530000, 0x00350000):   # limits 1 and 2: only (0, 1) / (1, 0) has its twin in the region
        assert (len(region), computed, fold[2]) == (6, 5, 1)


def test_full_game_computes_331776_of_1048576_boxes():
    """With every limit the largest the classes depend on (c4, c5) and (c6, c7) alone: 36 x 36 of
    the 4,096 (c4, c5, c6, c7) tuples are computed, times the 2^8 boxes of the A heaps."""
    rb, region = region_boxes(0xFFFF0000)
    computed, fold = _check_partition(region, rb)
    assert (len(region), computed) == (4096, 1296)
    assert (computed * 256, len(region) * 256) == (331776, 1048576)
