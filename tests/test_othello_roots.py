"""The root sets of tests/othello_roots.py are what tests/test_gpu_othello_sweep.py sweeps them for.

Every root's subtree is walked once with the reference generator of tests/othello_roots.py (squares
and directions on a cell array) and compared, position by position, with the C oracles
(oracle/othello8.c for 8x8, oracle/gm_oracle.c for 4x4): three generators written apart from one
another and from the shift-and-mask generator of csrc/games.hpp.  The coverage the sets were drawn
for is asserted as conditions: every (mover colour, square, direction, run length) a board admits
is flipped somewhere below some root, every square is played by either colour, passes and
double-pass endings abound, and the 4x4 roots meet most stabiliser subgroups of D4.  The last test
is the host-twin leg: the CPU build of DescOthello8 (what the kernels run) on every position of
every 8x8 subtree -- where a generator mutant shows first, without a GPU.
"""
import numpy as np
import pytest

import othello8  # noqa: E402  (oracle/)
import othello_roots as R
from othello_roots import OTH4_ROOTS, OTH8_EDGE, OTH8_ROOTS, UNDECIDED, Walk, key_of, words_of
from test_symmetry_algebra import SUBGROUPS, ref_images, ref_stabilizer

OTH = 4
CAP8, CAP4 = 3000, 4000


@pytest.fixture(scope="module")
def o8():
    return othello8.Othello8Oracle()


@pytest.fixture(scope="module")
def walks8():
    """root words -> Walk, the drawn roots then the named ones (read-only)."""
    return {w: Walk(8, key_of(w)) for w in OTH8_ROOTS + tuple(OTH8_EDGE.values())}


@pytest.fixture(scope="module")
def walks4():
    return {k: Walk(4, k) for k in OTH4_ROOTS}


@pytest.fixture(scope="module")
def expanded8(o8, walks8):
    """position -> (primitive, ordered children) by the 8x8 oracle, over every subtree."""
    out = {}
    for w in walks8.values():
        for k in w.kids:
            if k not in out:
                prim, _, kids = o8.expand(words_of(k))
                out[k] = (prim, tuple(key_of(c) for c in kids))
    return out


def test_feasible_flip_cases_are_counted_from_the_board():
    """2 colours x move squares x 8 directions x the run lengths that leave room for the closing disc."""
    for L, n in ((8, 1920), (4, 136)):
        count = 0
        for x in range(L):
            for y in range(L):
                if L == 8 and (x, y) in R.CENTRE8:
                    continue
                for dx, dy in R.DIRS:
                    run = 1
                    while 0 <= x + (run + 1) * dx < L and 0 <= y + (run + 1) * dy < L:
                        count, run = count + 2, run + 1
        assert count == n == len(R.feasible(L))
    assert max(c[4] for c in R.feasible(8)) == 6 and max(c[4] for c in R.feasible(4)) == 2


def test_roots_are_valid_positions_of_their_descriptors():
    assert 100 <= len(OTH8_ROOTS) <= 150 and len(set(OTH8_ROOTS)) == len(OTH8_ROOTS)
    assert not set(OTH8_ROOTS) & set(OTH8_EDGE.values()) and len(set(OTH8_EDGE.values())) == len(OTH8_EDGE)
    for w in OTH8_ROOTS + tuple(OTH8_EDGE.values()):
        assert len(w) == 3 and all(0 <= x < 1 << 64 for x in w) and w[2] < 1 << 16, w
        k = key_of(w)
        white, black, turn, npass = R.split(8, k)
        cells = R.cells_of(8, k)
        assert not white & black and turn in (1, 2) and npass <= 2, w
        assert all(cells[8 * y + x] for x, y in R.CENTRE8), w
        assert R.valid(8, k) and words_of(k) == w
    for w in OTH8_ROOTS:
        assert 1 <= R.empties(8, key_of(w)) <= 7 and w[0] & 0xFF <= 1, w
    n = len(OTH8_ROOTS)
    assert {R.empties(8, key_of(w)) for w in OTH8_ROOTS} == set(range(1, 8))
    assert n // 3 <= sum((w[0] >> 8) & 0xFF == 1 for w in OTH8_ROOTS) <= 2 * n // 3     # the turn is mixed
    assert n // 6 <= sum(w[0] & 0xFF == 1 for w in OTH8_ROOTS) <= n // 3                # about a quarter: pass byte 1
    assert 50 <= len(OTH4_ROOTS) <= 200 and len(set(OTH4_ROOTS)) == len(OTH4_ROOTS)
    for k in OTH4_ROOTS:
        assert R.valid(4, k) and 1 <= R.empties(4, k) <= 12, hex(k)
    centre = [sum(R.cells_of(4, k)[j] == 0 for j in (5, 6, 9, 10)) for k in OTH4_ROOTS]
    assert sum(c >= 1 for c in centre) >= 20 and sum(c == 4 for c in centre) >= 2     # empty centre squares
    one_colour = [k for k in OTH4_ROOTS if not R.split(4, k)[0] or not R.split(4, k)[1]]
    assert len(one_colour) >= 4 and {R.split(4, k)[2] for k in one_colour} == {1, 2}
    assert sum(k & 0xFF == 1 for k in OTH4_ROOTS) >= 5


def test_named_roots_are_what_their_names_say(walks8):
    n = {name: len(walks8[w]) for name, w in OTH8_EDGE.items()}
    full = [name for name in OTH8_EDGE if name.startswith("full_")]
    assert sorted(full) == ["full_%s_pass%d" % (c, p) for c in ("black", "white") for p in (0, 1, 2)]
    for name in full:
        w = OTH8_EDGE[name]
        assert R.empties(8, key_of(w)) == 0 and n[name] == 1
        assert ((w[0] >> 8) & 0xFF, w[0] & 0xFF) == (1 + name.startswith("full_white"), int(name[-1]))
    assert len({walks8[OTH8_EDGE[name]].prim[key_of(OTH8_EDGE[name])] for name in full}) == 3   # WIN, LOSS and TIE
    w = OTH8_EDGE["pass2_with_empties"]
    assert w[0] & 0xFF == 2 and R.empties(8, key_of(w)) >= 1 and n["pass2_with_empties"] == 1
    w = OTH8_EDGE["pass1_passes_again"]
    assert w[0] & 0xFF == 1 and n["pass1_passes_again"] == 2 and walks8[w].kids[key_of(w)] == (key_of(w) + 1,)
    w = OTH8_EDGE["pass1_has_a_move"]
    kids = walks8[w].kids[key_of(w)]
    assert w[0] & 0xFF == 1 and kids and all(c & 0xFF == 0 for c in kids)     # the first tier step is 3 - 1
    w = OTH8_EDGE["one_empty_unplayable"]
    k = key_of(w)
    assert R.empties(8, k) == 1 and sorted(walks8[w].kids) == [k, k + 1, k + 2]


def test_oth8_walks_equal_the_oracle(o8, walks8, expanded8):
    """Position count and position set of every subtree, and per position the primitive value and
    the ORDERED child list, against oracle/othello8.c."""
    total = 0
    for w, walk in walks8.items():
        r = o8.solve(w, want=1 << 62)
        assert r["positions"] == len(walk) <= CAP8, w
        assert {key_of(x) for x in r["words"].tolist()} == set(walk.kids), w
        total += len(walk)
    for walk in walks8.values():
        for k, kids in walk.kids.items():
            prim, okids = expanded8[k]
            assert prim == walk.prim[k], hex(k)
            assert okids == kids, hex(k)
    print("8x8: %d roots, %d positions" % (len(walks8), total))
    assert total >= 50000


def test_oth4_walks_equal_the_oracle(oracle, walks4):
    """As above against oracle/gm_oracle.c; Oracle.expand returns the children sorted, so the child
    sets are compared (the order is the 8x8 generator's, compared above)."""
    total = 0
    for root, walk in walks4.items():
        keys, _ = oracle.solve(OTH, (4, 4), root=root)
        assert len(keys) == len(walk) <= CAP4, hex(root)
        assert keys.tolist() == sorted(walk.kids), hex(root)
        for k, kids in walk.kids.items():
            prim, okids, _ = oracle.expand(OTH, (4, 4), k)
            assert prim == walk.prim[k], hex(k)
            assert okids == sorted(kids) and len(set(kids)) == len(kids), hex(k)
        total += len(walk)
    print("4x4: %d roots, %d positions" % (len(walks4), total))
    assert total >= 10000


def test_oth8_sweep_covers_every_flip_case(walks8):
    cases = set().union(*(w.cases for w in walks8.values()))
    assert cases == R.feasible(8)
    squares = set().union(*(w.squares for w in walks8.values()))
    want = {(c, x, y) for c in (R.BLACK, R.WHITE) for x in range(8) for y in range(8) if (x, y) not in R.CENTRE8}
    assert squares == want and len(want) == 120
    assert max(w.most_dirs for w in walks8.values()) >= 4
    assert sum(w.passes for w in walks8.values()) >= 1000
    assert sum(w.double_pass_ends for w in walks8.values()) >= 100


def test_oth4_sweep_covers_every_flip_case(walks4):
    assert set().union(*(w.cases for w in walks4.values())) == R.feasible(4)
    assert set().union(*(w.squares for w in walks4.values())) == {(c, x, y) for c in (1, 2) for x in range(4)
                                                                  for y in range(4)}
    assert sum(w.passes for w in walks4.values()) >= 100


def test_oth4_roots_meet_the_stabiliser_subgroups():
    stab = ref_stabilizer(ref_images(np.array(OTH4_ROOTS, dtype=np.uint64), 4)).tolist()
    assert set(stab) <= set(SUBGROUPS)
    assert sum(s != 0x01 for s in stab) >= 12
    assert len(set(stab) - {0x01}) >= 5, sorted(set(stab))
    assert stab.count(0x01) >= 50


def test_host_twin_on_every_position_of_every_oth8_subtree(walks8, expanded8):
    """gm_expand_host_key, the CPU build of DescOthello8 (step / run / legal / flips_at, the
    reordering of csrc/moves_common.hpp move_slot's kind in gm_api.hip): the oracle's primitive
    value and the oracle's children in the oracle's order."""
    from gamesmanmpi_amd import games
    hd = games.HostDescriptor(games.OthelloCodec(8, 8))
    try:
        assert hd.words == 3
        for k, (prim, kids) in expanded8.items():
            p, got, tier = hd.expand(k)
            assert p == prim, hex(k)
            assert tuple(got) == (kids if prim == UNDECIDED else ()), hex(k)
            assert tier == 3 * (64 - R.empties(8, k)) + (k & 0xFF), hex(k)
    finally:
        hd.close()
