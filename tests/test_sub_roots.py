"""The root sets of tests/sub_roots.py cover what tests/test_gpu_sub_sweep.py sweeps them for: the
three shapes of the box engine's hybrid schedule, every way the box limits of a mirror pair
compare, every kind of digit in every heap, root changes that keep and that rebuild a context's
lists -- and the C oracle solves every one of them within the 1-byte codes' range."""
import os
import re

import pytest

import sub_roots as S
from sub_roots import PAIRS8, ROOTS8, ROOTS_H, box_limits, box_tiers, digits, n_boxes, positions

SUB = 5
CAP = 300000
HERE = os.path.dirname(os.path.abspath(__file__))
# the files whose hand-picked roots the sweep adds to
OTHERS = ("test_gpu_parity.py", "test_gpu_box_mirror.py", "test_gpu_box_mirror45.py", "test_gpu_box_hybrid.py",
          "test_gpu_sharded.py", "test_gpu_byte_tables.py")


def test_helpers_on_known_roots():
    assert [box_tiers(r) for r in (0x33333333, 0x37733333, 0x7777FFFF, 0xFFFFFFFF)] == [5, 9, 25, 41]
    assert [(box_tiers(r), positions(r)) for r in (0xEEEE0000, 0xFFFF0003, 0xEFEF0040, 0xFEFE4000, 0xFFEE0300)] == \
        [(29, 50625), (29, 262144), (30, 288000), (30, 288000), (29, 230400)]
    assert box_limits(0x2468BDF3) == (0, 3, 3, 2, 4, 3, 2, 1) and n_boxes(0x2468BDF3) == 4 * 4 * 3 * 5 * 4 * 3 * 2
    assert positions(0xFFF, 3) == 4096 and positions(0) == 1 and n_boxes(0) == 1
    assert S.outside_keys(0xFF3F0A5C) == [0xFF3F0A5D, 1 << 32, 2 ** 64 - 1]
    assert S.outside_keys(0xFFF0A5CF)[0] == 0xFFF0A5DF
    assert S.outside_keys(0xFFF, 3)[0] == 0x1FFF   # every heap full: the nibble above the table
    assert len(S.every(3)) > len(S.every(4)) >= len(ROOTS8) // 4 and set(S.IDLE8) <= set(ROOTS8)


def test_roots8_are_small_new_and_distinct():
    assert len(ROOTS8) >= 120 and len(set(ROOTS8)) == len(ROOTS8)
    used = set()
    for name in OTHERS:
        used |= {int(m, 16) for m in re.findall(r"0[xX][0-9A-Fa-f]+", open(os.path.join(HERE, name)).read())}
    assert len(used) > 25
    for r in ROOTS8 + tuple(q for p in PAIRS8 for q in p):
        assert 0 < r < 1 << 32 and positions(r) <= CAP, hex(r)
        assert n_boxes(r) >= 2, hex(r)
        assert r not in used, hex(r)


def test_roots8_cover_the_hybrid_schedule():
    """csrc/dense_box.hip box_prepare clips the default range (14, 26) to the root's T box-tiers:
    T <= 14 every tier in the head launch, 15..27 a head and tier launches, from 28 a tail too."""
    t = [box_tiers(r) for r in ROOTS8]
    assert sum(x <= 14 for x in t) >= 30
    assert sum(15 <= x <= 27 for x in t) >= 30
    assert sum(x >= 28 for x in t) >= 6
    assert {13, 14, 15, 27, 28} <= set(t)   # either side of both clips


@pytest.mark.parametrize("lo", [4, 6])
def test_roots8_cover_the_mirror_pairs(lo):
    """Heaps lo, lo + 1 are a mirror pair: with unequal limits one box of a pair of twins can lie
    outside the region (computed directly), with equal ones never, with zero ones no box has a twin."""
    lim = [(box_limits(r)[lo], box_limits(r)[lo + 1]) for r in ROOTS8]
    assert sum(a < b for a, b in lim) >= 20
    assert sum(a > b for a, b in lim) >= 20
    assert sum(a == b and a > 0 for a, b in lim) >= 15
    assert sum(a == 0 and b == 0 for a, b in lim) >= 10


def test_roots8_unequal_in_both_pairs_at_once():
    lim = [box_limits(r) for r in ROOTS8]
    assert sum(l[4] != l[5] and l[6] != l[7] for l in lim) >= 30


@pytest.mark.parametrize("heap", range(8))
def test_roots8_digits_of_every_heap(heap):
    """0, a digit that fills the top box (A heaps 3, 7, 11, 15; B heaps odd) and one that leaves it
    partial (not 0), each at least 8 times."""
    d = [digits(r)[heap] for r in ROOTS8]
    full = (lambda x: x & 3 == 3) if heap < 4 else (lambda x: x & 1 == 1)
    assert sum(x == 0 for x in d) >= 8
    assert sum(full(x) for x in d) >= 8
    assert sum(x != 0 and not full(x) for x in d) >= 8


def test_root_changes_that_keep_and_that_rebuild():
    assert len(PAIRS8) >= 12
    for r, q in PAIRS8:
        assert q != r and box_limits(q) == box_limits(r), (hex(r), hex(q))
    assert sum(box_limits(a) != box_limits(b) for a, b in zip(ROOTS8, ROOTS8[1:])) >= 12


def test_roots_h_shapes():
    assert sorted(ROOTS_H) == [3, 4, 5, 6, 7]
    for h, roots in ROOTS_H.items():
        assert 14 <= len(roots) <= 18 and len(set(roots)) == len(roots)
        for r in roots:
            assert 0 < r < 16 ** h and positions(r, h) <= CAP, hex(r)
        for i in range(h):
            d = {digits(r, h)[i] for r in roots}
            assert 0 in d and 15 in d and d - {0, 15}, (h, i)
        if h > 3:
            assert sum(r >> 12 == 0 for r in roots) >= 2      # one block at three low heaps
        if h > 4:
            assert sum(len(set(digits(r, h)[3:])) > 1 for r in roots) >= 4   # uneven high nibbles


def _cases():
    return [(8, r) for r in ROOTS8] + [(8, q) for _, q in PAIRS8] + [(h, r) for h in ROOTS_H for r in ROOTS_H[h]]


def test_oracle_solves_every_root(oracle):
    """n is the region's size and no remoteness reaches 120: every expected record has a 1-byte
    code, and none of them is the sweep's poison byte 0x80 (LOSS in 127)."""
    deepest = 0
    for h, root in _cases():
        keys, recs = oracle.solve(SUB, (h,), root)
        assert len(keys) == positions(root, h), hex(root)
        assert int(keys[-1]) == root and int(keys[0]) == 0
        assert (recs >> 14).max() <= 1   # WIN or LOSS: the game has no ties
        deepest = max(deepest, int((recs & 0x3FFF).max()))
    assert deepest < 120
