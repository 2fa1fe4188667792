"""The symmetry reductions on the device, from roots of every stabiliser and on every kind of board.

The sparse engines store one representative per orbit of the subgroup that fixes the root
(csrc/games.hpp DescOthello::canon / orbit / stabilizer, DescToot::mirror / canon / orbit) and
expand the orbits again in every read of the table.  Here: Othello 4x4 from one root per
subgroup of D4, a context whose root's stabiliser changes between solves, and Toot-and-Otto on
boards no other test solves on the device (tall, one or two columns wide, 7 and 8 columns wide).
The expected tables always come from the C oracle (oracle/gm_oracle.c), which knows nothing of
symmetry; the orbit counts from the numpy reference of tests/test_symmetry_algebra.py applied to
the oracle's keys.  GM_OPT_SYMMETRY is set explicitly in every solve.
"""
import numpy as np
import pytest

from conftest import digest

from test_symmetry_algebra import SUBGROUPS, mask_of, popcount, ref_canon, ref_images, ref_mirror, ref_stabilizer

pytestmark = pytest.mark.gpu

from gamesmanmpi_amd import Context, _lib  # noqa: E402

TOOT, OTH = 3, 4
U64 = np.uint64
UNSOLVED = 0xFFFF

# Othello 4x4 roots, one per subgroup of D4 (white plane at bits 32..47, black at 16..31, the
# turn byte at 8..15, pass 0): (the elements that fix the root, root key, reachable positions)
OTH_ROOTS = [
    ((0,), 0x42042000200, 15624),
    ((0, 2), 0x18002400200, 9542),
    ((0, 4), 0x24100200100, 18387),
    ((0, 5), 0x20804600200, 11913),
    ((0, 6), 0x60000600200, 56434),
    ((0, 7), 0x44002200100, 56434),
    ((0, 1, 2, 3), 0x418206600200, 679),
    ((0, 2, 4, 5), 0x24004200200, 54089),       # the standard start
    ((0, 2, 6, 7), 0x66060060100, 480),
    (tuple(range(8)), 0x699600000200, 3),       # root, pass, second pass: the 8-way de-duplication only
]
OTH_IDS = ["".join(str(g) for g in gs) for gs, _, _ in OTH_ROOTS]
OTH_ORBITS = {0x01: 15624, 0x05: 4781, 0x11: 9231, 0x21: 5967, 0x0F: 172, 0xC5: 124, 0xFF: 3}   # where known ahead
MIRROR_X, C4, START = OTH_ROOTS[4], OTH_ROOTS[6], OTH_ROOTS[7]


class Ref:
    """The oracle's table from one root, with what the tests derive from it (read-only)."""

    def __init__(self, oracle, game, params, root):
        self.root = root
        self.keys, self.recs = oracle.solve(game, params, root=root)
        self.n = len(self.keys)
        assert (self.keys[1:] > self.keys[:-1]).all()
        self.digest = digest(self.keys, self.recs)
        value, rem = (self.recs >> 14).astype(np.int64), (self.recs & 0x3FFF).astype(np.int64)
        assert value.max() <= 2
        depth = int(rem.max()) + 1
        self.hist = np.bincount(value * depth + rem, minlength=3 * depth).reshape(3, depth).astype(U64)
        # the descriptors' tiers (games.hpp): discs times 3 plus the pass count / pieces, from the root's
        tier = popcount(self.keys >> U64(16)) * (3 if game == OTH else 1)
        if game == OTH:
            tier += (self.keys & U64(0xFF)).astype(np.int64)
        at = int(np.searchsorted(self.keys, U64(root)))
        assert int(self.keys[at]) == root
        self.root_record = int(self.recs[at])
        self.tiers = np.bincount(tier - tier[at]).tolist()
        for a in (self.keys, self.recs, self.hist):
            a.setflags(write=False)


_refs = {}


def ref_of(oracle, game, params, root):
    key = (game, tuple(params), root)
    if key not in _refs:
        _refs[key] = Ref(oracle, game, params, root)
    return _refs[key]


def othello_orbits(ref, S):
    """Orbits of the oracle's key set under the subgroup S (a mask): distinct least images."""
    if not hasattr(ref, "img"):
        ref.img = ref_images(ref.keys, 4)
        ref.img.setflags(write=False)
    return len(np.unique(ref_canon(ref.img, S)))


def toot_orbits(ref, L, H):
    return len(np.unique(np.minimum(ref.keys, ref_mirror(ref.keys, L, H))))


def open_ctx(game, params, sym, ranks, engine=None):
    ctx = Context(game, params, device=0)
    if engine is not None:
        ctx.set_option(_lib.OPT_ENGINE, engine)
    ctx.set_option(_lib.OPT_SYMMETRY, sym)
    ctx.set_option(_lib.OPT_VIRTUAL_RANKS, ranks)
    return ctx


def check_solve(ctx, ref, stored):
    """Solve ref's root on ctx; every read of the table against the oracle's."""
    n, rec = ctx.solve(ref.root)
    assert n == ref.n and rec == ref.root_record
    k, r = ctx.export()
    assert np.array_equal(k, ref.keys) and np.array_equal(r, ref.recs)
    assert ctx.digest() == (ref.digest, ref.n)
    tiers = [int(x) for x in ctx.tier_counts()]
    assert tiers == ref.tiers and sum(tiers) == ref.n
    assert np.array_equal(ctx.histogram(), ref.hist)
    st = ctx.stats()
    print("n %d stored %d (expected %d) world %d" % (n, st["n_stored"], stored, st["world"]))
    assert st["n_positions"] == ref.n
    assert st["n_stored"] == stored
    return st


def test_othello_root_table_is_what_it_says(oracle):
    """Every root's stabiliser is exactly the stated subgroup, the ten are the ten subgroups,
    and the oracle reaches the stated number of positions, closed under the subgroup."""
    assert sorted(mask_of(gs) for gs, _, _ in OTH_ROOTS) == sorted(SUBGROUPS)
    for gs, root, positions in OTH_ROOTS:
        S = mask_of(gs)
        assert int(ref_stabilizer(ref_images(np.array([root], dtype=U64), 4))[0]) == S, hex(root)
        ref = ref_of(oracle, OTH, (4, 4), root)
        assert ref.n == positions, hex(root)
        othello_orbits(ref, S)
        for g in gs:
            assert np.array_equal(np.sort(ref.img[g]), ref.keys), (hex(root), g)
        if S in OTH_ORBITS:
            assert othello_orbits(ref, S) == OTH_ORBITS[S], hex(root)
        assert othello_orbits(ref, 0x01) == positions


@pytest.mark.parametrize("ranks", [1, 4])
@pytest.mark.parametrize("sym", [1, 0])
@pytest.mark.parametrize("gs,root,positions", OTH_ROOTS, ids=OTH_IDS)
def test_othello_root_per_stabiliser_subgroup(oracle, gs, root, positions, sym, ranks):
    S = mask_of(gs)
    assert int(ref_stabilizer(ref_images(np.array([root], dtype=U64), 4))[0]) == S
    ref = ref_of(oracle, OTH, (4, 4), root)
    assert ref.n == positions
    orbits = othello_orbits(ref, S)
    assert positions // len(gs) <= orbits <= positions
    ctx = open_ctx(OTH, (4, 4), sym, ranks)
    # n_stored counts the stored representatives of all ranks (include/gmsolve.h)
    check_solve(ctx, ref, orbits if sym else positions)
    assert np.array_equal(ctx.query(ref.keys), ref.recs)
    # images under the elements that do not fix the root, where they are no reachable position:
    # a canon() that used such an element would find their representative in the table
    rng = np.random.default_rng(S)
    for g in range(8):
        if g in gs:
            continue
        img = ref.img[g]
        absent = img[~np.isin(img, ref.keys)]
        print("g %d: %d of %d images are no reachable position" % (g, len(absent), len(img)))
        assert len(absent) >= 100, g
        if len(absent) > 2000:
            absent = rng.choice(absent, 2000, replace=False)
        assert (ctx.query(absent) == UNSOLVED).all(), g
    ctx.close()


def test_othello_one_context_changing_stabilisers(oracle):
    """One sparse-engine context, the root's stabiliser changing from solve to solve: a repeated
    solve replays its record (csrc/sparse.hip replay_with, keyed on the subgroup), another root
    or another setting of the reduction must not."""
    mirror = ref_of(oracle, OTH, (4, 4), MIRROR_X[1])
    c4 = ref_of(oracle, OTH, (4, 4), C4[1])
    start = ref_of(oracle, OTH, (4, 4), START[1])
    ctx = open_ctx(OTH, (4, 4), 1, 1, engine=_lib.ENGINE_SPARSE)
    steps = [(mirror, 1, othello_orbits(mirror, 0x41)), (c4, 1, othello_orbits(c4, 0x0F)),
             (mirror, 1, othello_orbits(mirror, 0x41)), (mirror, 1, othello_orbits(mirror, 0x41)),
             (mirror, 0, mirror.n), (start, 1, othello_orbits(start, 0x35))]
    for i, (ref, sym, stored) in enumerate(steps):
        ctx.set_option(_lib.OPT_SYMMETRY, sym)
        st = check_solve(ctx, ref, stored)
        assert st["engine"] == _lib.ENGINE_SPARSE
        # the fourth solve is the replay: one graph launch, no forward pass of its own
        assert (st["forward_ms"] == 0) == (i == 3), i
    ctx.close()


# ---------------------------------------------------------------- Toot-and-Otto
TOOT_FULL = [((1, 1), 3), ((2, 2), 81), ((1, 8), 339), ((2, 6), 45495), ((3, 4), 126559), ((2, 7), 154987),
             ((3, 5), 913817)]

# mid-game roots on the 8- and 7-column boards (their full games are too large): seeded playouts
# of mirrored move pairs (or not), cut at the first depth whose oracle solve has 10,000 to
# 300,000 positions: (board, root key, its own mirror image?)
TOOT_MID = [
    ((8, 3), 0x3C8100813C003333, True),      # 12 pieces, 259,325 positions
    ((8, 3), 0x104A00EA00424342, False),     # 259,408
    ((7, 3), 0x01B2201060803434, True),      # 78,443
    ((7, 3), 0x0350200150025325, False),     # 211,516
]


def check_toot(oracle, dims, root, sym, ranks, symmetric):
    L, H = dims
    ref = ref_of(oracle, TOOT, dims, root)
    assert (int(ref_mirror(np.array([root], dtype=U64), L, H)[0]) == root) == symmetric
    orbits = toot_orbits(ref, L, H) if symmetric else ref.n
    if symmetric:   # the reachable set is closed under the mirror
        assert np.array_equal(np.sort(ref_mirror(ref.keys, L, H)), ref.keys)
        assert (ref.n + 1) // 2 <= orbits <= ref.n
    ctx = open_ctx(TOOT, dims, sym, ranks)
    check_solve(ctx, ref, orbits if sym else ref.n)
    return ctx, ref


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("sym", [1, 0])
@pytest.mark.parametrize("dims,positions", TOOT_FULL, ids=["%dx%d" % d for d, _ in TOOT_FULL])
def test_toot_full_games_on_tall_and_narrow_boards(oracle, dims, positions, sym, ranks):
    ctx, ref = check_toot(oracle, dims, 0x6666, sym, ranks, True)
    assert ref.n == positions
    if dims[0] == 1:   # one column: every position is its own mirror image
        assert ctx.stats()["n_stored"] == ref.n
    ctx.close()


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("sym", [1, 0])
@pytest.mark.parametrize("dims,root,symmetric", TOOT_MID,
                         ids=["%dx%d-%s" % (d + ("symmetric" if s else "asymmetric",)) for d, _, s in TOOT_MID])
def test_toot_mid_game_roots_on_wide_boards(oracle, dims, root, symmetric, sym, ranks):
    ctx, ref = check_toot(oracle, dims, root, sym, ranks, symmetric)
    assert 10000 <= ref.n <= 300000
    st = ctx.stats()
    if symmetric:
        pick = np.random.default_rng(5).choice(ref.n, 2000, replace=False)
        k = ref.keys[pick]
        m = ref_mirror(k, *dims)
        assert (m != k).sum() >= 1000
        got = ctx.query(m)
        assert np.array_equal(got, ctx.query(k)) and np.array_equal(got, ref.recs[pick])
        assert np.array_equal(got, ref.recs[np.searchsorted(ref.keys, m)])
    else:
        assert st["n_stored"] == ref.n
    ctx.close()
