"""The heap-6/7 mirror of the box engine (csrc/box_common.hpp, csrc/dense_box.hip), pinned on
the host before any kernel runs: the layout identity the mirrored store relies on, against the
C oracle's records, and the compute-list rule as a partition of the root's region.

Box layout: index = box << 12 | A << 4 | B; heaps 6 and 7 are bits 2 and 3 of B and the fields
c6 (bits 14-16) and c7 (bits 17-19) of the box id.  swap67(C) exchanges the two fields; its row
m (16 bytes, one A) is row m of C with dwords 1 and 2 exchanged."""
import itertools

import numpy as np
import pytest

SUB = 5
ROOTS = [0x33000000, 0x53000000, 0x35010203, 0x77110011]


def box_index_of_key(k):
    """Python twin of csrc/box_common.hpp box_index_of_key (numpy int64 arrays or ints)."""
    off = box = 0
    for i in range(4):
        h = (k >> (4 * i)) & 15
        off = off | ((h & 3) << (4 + 2 * i))
        box = box | ((h >> 2) << (2 * i))
    for j in range(4):
        h = (k >> (16 + 4 * j)) & 15
        off = off | ((h & 1) << j)
        box = box | ((h >> 1) << (8 + 3 * j))
    return (box << 12) | off


def box_coord(box, d):
    return (box >> (2 * d)) & 3 if d < 4 else (box >> (8 + 3 * (d - 4))) & 7


def box_unit(d):
    return 1 << (2 * d) if d < 4 else 1 << (8 + 3 * (d - 4))


def swap67(box):
    t = ((box >> 14) ^ (box >> 17)) & 7
    return box ^ (t << 14) ^ (t << 17)


def in_region(box, root_box):
    return all(box_coord(box, d) <= box_coord(root_box, d) for d in range(8))


def mirror_class(box, root_box):
    """Python twin of bx_mirror_class: 0 computed and stored once, 1 computed and also stored
    to swap67(box) (the mirror flag), 2 mirrored-to (not computed)."""
    c6, c7 = box_coord(box, 6), box_coord(box, 7)
    if c6 == c7 or not in_region(swap67(box), root_box):
        return 0
    return 1 if c6 > c7 else 2


def region_boxes(root):
    rb = box_index_of_key(root) >> 12
    ranges = [range(box_coord(rb, d) + 1) for d in range(8)]
    return rb, sorted(sum(c * box_unit(d) for d, c in enumerate(cs)) for cs in itertools.product(*ranges))


def oracle_boxes(oracle, root):
    """{box: 4096 uint16 records in box order, 0xFFFF where the position is outside the region}."""
    keys, recs = oracle.solve(SUB, (8,), root=root)
    idx = box_index_of_key(keys.astype(np.int64))
    out = {}
    for b in np.unique(idx >> 12).tolist():
        a = np.full(4096, 0xFFFF, np.uint16)
        sel = (idx >> 12) == b
        a[idx[sel] & 4095] = recs[sel]
        out[b] = a
    return out


@pytest.mark.parametrize("root", ROOTS)
def test_mirrored_box_is_the_twin_with_dwords_1_and_2_exchanged(oracle, root):
    """For every region box C whose swap67(C) is in the region, each 16-byte row of swap67(C)
    is the same row of C with dwords 1 and 2 exchanged.  (These roots' heaps 6 and 7 are odd,
    so their boxes are whole along both and every position of a twin has its image in C.)"""
    rb, region = region_boxes(root)
    tab = oracle_boxes(oracle, root)
    assert sorted(tab) == region
    pairs = 0
    for c in region:
        t = swap67(c)
        if not in_region(t, rb):
            continue
        swapped = tab[c].reshape(256, 4, 4)[:, [0, 2, 1, 3], :]   # row m, dword, byte
        assert np.array_equal(tab[t].reshape(256, 4, 4), swapped), (hex(c), hex(t))
        assert (tab[t] != 0xFFFF).any()
        pairs += 1
    assert pairs >= 4   # 0x33000000: all four boxes (two diagonal ones their own twins)


def _check_partition(region, rb):
    writes = dict.fromkeys(region, 0)
    computed = flagged = 0
    for c in region:
        cls = mirror_class(c, rb)
        if cls == 2:
            continue
        computed += 1
        writes[c] += 1
        if cls == 1:
            flagged += 1
            t = swap67(c)
            assert t in writes, "a store outside the region"
            assert mirror_class(t, rb) == 2 and box_coord(t, 6) + box_coord(t, 7) == box_coord(c, 6) + box_coord(c, 7)
            writes[t] += 1
    assert set(writes.values()) == {1}
    assert computed + flagged == len(region)
    return computed, flagged


@pytest.mark.parametrize("root", ROOTS + [0x35000000, 0xFF000000, 0xFF330033, 0x12345678])
def test_compute_list_rule_partitions_the_region(root):
    """Every region box is computed exactly once or mirrored-to by exactly one flagged box;
    nothing outside the region is written; a twin keeps the box-tier."""
    rb, region = region_boxes(root)
    computed, flagged = _check_partition(region, rb)
    if root == 0x33000000:
        assert (len(region), computed, flagged) == (4, 3, 1)
    if root == 0xFF000000:
        assert (len(region), computed, flagged) == (64, 36, 28)


def test_full_game_computes_589824_of_1048576_boxes():
    """The classes depend on (c6, c7) alone when every limit is the largest: 36 of the 64
    (c6, c7) pairs are computed, 28 of them flagged, times the 2^14 boxes of the other heaps."""
    rb, region = region_boxes(0xFF000000)
    computed, flagged = _check_partition(region, rb)
    others = (1 << 20) // 64
    assert (computed * others, (computed + flagged) * others) == (589824, 1048576)
