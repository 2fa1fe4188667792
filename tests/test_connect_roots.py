"""What the Connect sweep (tests/test_gpu_connect_sweep.py) covers, stated as conditions over the
union of its subtrees and checked on the CPU: the C oracle (oracle/gm_oracle.c) gives every
subtree's table, the cell arrays of tests/connect_roots.py say what its positions hold.  The set
of tests/connect_roots.py was drawn (tools/draw_connect_roots.py) to meet these conditions; a
condition that fails after a change of the set asks for more roots, not for a weaker condition.
"""
import numpy as np
import pytest

import connect_roots as R
from connect_roots import CONNECT, DRAWN, FULL, LOSS, TIE, UNDECIDED

U64 = np.uint64
# the boards the mid-game roots were asked for
ASKED = [(7, 8, 4), (3, 20, 4), (2, 30, 4), (16, 2, 4), (16, 2, 8), (15, 3, 4), (12, 4, 5), (8, 6, 6), (7, 7, 7), (9, 6, 8)]

_tables = {}
_facts = {}


def table(oracle, dims, root=None):
    """The oracle's (keys, records) below a root (None: the empty board); made once, read-only."""
    if (dims, root) not in _tables:
        keys, recs = oracle.solve(CONNECT, dims, root=root)
        keys.setflags(write=False)
        recs.setflags(write=False)
        _tables[(dims, root)] = (keys, recs)
    return _tables[(dims, root)]


def facts(oracle, dims):
    """Per swept board, over the distinct positions of all its subtrees: what the conditions read."""
    if dims in _facts:
        return _facts[dims]
    L, H, K = dims
    roots = ([None] if dims in FULL else []) + [r for _, r, _, _ in R.drawn_of(dims)]
    keys = np.concatenate([table(oracle, dims, r)[0] for r in roots])
    recs = np.concatenate([table(oracle, dims, r)[1] for r in roots])
    keys, first = np.unique(keys, return_index=True)
    recs = recs[first]
    cells, heights = R.cells_of(keys, L, H)
    assert (heights >= 0).all()
    mine = cells == R.last_mover(heights)[:, None, None]
    f = {"n": len(keys), "keys": keys, "recs": recs, "primitive": R.primitive(keys, L, H, K)}
    lost = f["primitive"] == LOSS
    f["lines"] = {}
    for d in R.DIRS:
        s = R.line_starts(mine, K, d)
        f["lines"][d] = {"any": int(s.reshape(len(keys), -1).any(axis=1).sum()) if s.size else 0,
                         **{w: int(R.touches(s, K, d, w, L, H).sum()) for w in ("top", "left", "right")}}
    f["wraps"] = {d: int((R.wrap_runs(mine, K, s) & ~lost).sum()) for d, s in R.wrap_strides(H).items()}
    f["open"] = set(((heights < H).sum(axis=1)[f["primitive"] == UNDECIDED]).tolist())
    f["bit62"] = int((keys >> U64(62) != 0).sum())
    f["tallest"] = int(heights.max())
    _facts[dims] = f
    return f


def test_full_games_are_within_the_bound(oracle):
    for dims in FULL:
        keys, recs = table(oracle, dims)
        assert 1 <= len(keys) <= R.FULL_MAX, dims
        empty = oracle.initial(CONNECT, dims)
        assert empty == R.key_of([[]] * dims[0], dims[1]) and int(keys[np.searchsorted(keys, U64(empty))]) == empty
    # K fits neither dimension: no position is won or lost
    _, recs = table(oracle, R.NO_LINE)
    assert not R.fits(*R.NO_LINE, "vertical") and not R.fits(*R.NO_LINE, "horizontal")
    assert set((recs >> 14).tolist()) == {TIE}
    # one column of 62: 63 positions, the full one with its cap at bit 62
    keys, recs = table(oracle, (1, 62, 4))
    assert len(keys) == 63 and int(keys[-1]) >> 62 == 1 and set((recs >> 14).tolist()) == {TIE}


def test_drawn_roots_are_positions_within_the_bounds(oracle):
    assert [d for d in ASKED if not R.drawn_of(d)] == []
    assert len(set((d, r) for d, r, _, _ in DRAWN)) == len(DRAWN)
    for dims, root, sym, how in DRAWN:
        L, H, K = dims
        assert R.valid(root, L, H), (dims, hex(root))
        assert R.primitive([root], L, H, K)[0] == UNDECIDED, (dims, hex(root))
        prim, kids, _ = oracle.expand(CONNECT, dims, root)
        assert prim == UNDECIDED and kids, (dims, hex(root))
        assert (R.mirror(root, L, H) == root) == sym == (how == "paired"), (dims, hex(root))
        keys, _ = table(oracle, dims, root)
        assert R.DRAWN_MIN <= len(keys) <= R.DRAWN_MAX, (dims, hex(root), len(keys))
        if sym:   # the subtree of a symmetric root is closed under the mirror
            m = np.array(sorted(R.mirror(int(k), L, H) for k in keys[:: max(1, len(keys) // 500)]), dtype=U64)
            assert np.isin(m, keys).all(), (dims, hex(root))
    symmetric = [d for d, _, s, _ in DRAWN if s]
    assert any(d[0] % 2 == 1 for d in symmetric) and any(d[0] % 2 == 0 for d in symmetric)
    assert any(d[1] > 7 for d in symmetric)
    # at least two games (seeds) behind every asked board
    for d in ASKED:
        assert len(R.drawn_of(d)) >= 2, d


def test_cell_arrays_and_oracle_agree_on_every_swept_position(oracle):
    """The conditions below read the cell arrays; the sweep's expectations come from the oracle.
    Both must call the same positions primitive, with the same value."""
    total = 0
    for dims in R.boards():
        f = facts(oracle, dims)
        ends = (f["recs"] & 0x3FFF) == 0
        assert np.array_equal(ends, f["primitive"] != UNDECIDED), dims
        assert np.array_equal((f["recs"] >> 14)[ends], f["primitive"][ends]), dims
        total += f["n"]
    print("swept positions (distinct per board): %d" % total)


def test_every_k_and_direction_ends_a_game_somewhere(oracle):
    """For every K in 2..8 and every direction that fits some swept board with that K, a LOSS-in-0
    position holds a K-line of that direction; per direction one such line touches the top row,
    one column 0 and one column L - 1."""
    for K in range(2, 9):
        bs = [d for d in R.boards() if d[2] == K]
        assert bs, K
        for direction in R.DIRS:
            fitting = [d for d in bs if R.fits(*d, direction)]
            if fitting:
                assert sum(facts(oracle, d)["lines"][direction]["any"] for d in fitting) >= 1, (K, direction)
    # what fits nowhere among the swept boards: the diagonals of 5 and of 8
    assert [(K, d) for K in range(2, 9) for d in R.DIRS if not any(b[2] == K and R.fits(*b, d) for b in R.boards())] == \
        [(5, "diagonal"), (5, "antidiagonal"), (8, "diagonal"), (8, "antidiagonal")]
    for direction in R.DIRS:
        for where in ("top", "left", "right"):
            assert sum(facts(oracle, d)["lines"][direction][where] for d in R.boards()) >= 1, (direction, where)
        # the steered roots: the long lines through the top row
        for K in (6, 7):
            assert facts(oracle, (8, 6, 6) if K == 6 else (7, 7, 7))["lines"][direction]["top"] >= 1


def test_positions_that_a_board_without_the_guard_row_gets_wrong(oracle):
    """Wrap witnesses: positions that are no primitive LOSS in which the player who just moved has K
    stones at linear cells i, i + s, .., i + (K - 1) s of the unguarded x * H + y numbering -- a run
    that leaves a column through its top row and re-enters the next at row 0.  At least 20 for each
    stride that can wrap: 1 (a column's top continued at the next one's bottom), H - 1 and H + 1
    (the diagonals).  Stride H cannot: i + j H is the same row of the next column and below L * H
    only on the board, so such a run is always a real row and the position a primitive LOSS; the
    count there is zero by construction, and asserted as that."""
    got = {d: sum(facts(oracle, b)["wraps"][d] for b in R.boards()) for d in R.DIRS}
    print("wrap witnesses per stride:", got)
    for d in ("vertical", "antidiagonal", "diagonal"):
        assert got[d] >= 20, (d, got)
    assert got["horizontal"] == 0


def test_open_columns_heights_and_the_top_key_bit(oracle):
    opened = set()
    for d in R.boards():
        opened |= facts(oracle, d)["open"]
    assert 16 in opened and 1 in opened and 0 not in opened
    assert set(range(1, 17)) <= opened
    assert sum(facts(oracle, d)["bit62"] for d in R.boards()) >= 1
    # bit 62 on a board of more than one column as well: the last column of 7x8 or 3x20 full
    assert facts(oracle, (7, 8, 4))["bit62"] >= 1 and facts(oracle, (3, 20, 4))["bit62"] >= 1
    tallest = {d: facts(oracle, d)["tallest"] for d in R.boards()}
    assert max(tallest.values()) >= 32
    assert sum(t >= 16 for t in tallest.values()) >= 2 and sum(t >= 8 for t in tallest.values()) >= 4


def longest_second_player_run(keys, L, H):
    """Per key: the most second-player stones on top of one another in one column."""
    cells, _ = R.cells_of(keys, L, H)
    best = np.zeros(len(cells), dtype=np.int64)
    run = np.zeros((len(cells), L), dtype=np.int64)
    for y in range(H):
        run = np.where(cells[:, :, y] == R.SECOND, run + 1, 0)
        best = np.maximum(best, run.max(axis=1))
    return best


def test_columns_that_need_the_long_shifts_of_filled(oracle):
    """DescConnect::filled smears every set bit of a column field downwards: the shifts by 1, 2 and 4
    reach 7 rows below a set bit, so the `H > 7` branch (the shift by 8, smear[3]) is needed exactly
    where 8 or more second-player stones (clear bits) lie on top of one another, and the shift by 16
    (smear[4]) where 16 or more do.  A game ends at the K-th stone of a column, so from the empty
    board only K = 8 on H >= 8 gets there: 2x9 with K = 8 holds such positions, and the host-twin
    comparison below and the device sweep read them (16 positions, each the end of a game).  Longer runs exist only in positions that no game
    reaches: EDGE.  No valid key holds a run of 32 (1x62 has 31 stones a side), so after the shift by
    16 the shift by 32 (smear[5]) adds no bit to any valid key."""
    f = facts(oracle, (2, 9, 8))
    runs = longest_second_player_run(f["keys"], 2, 9)
    assert int(runs.max()) == 8 and int((runs == 8).sum()) >= 1
    # e.g. 0x3FE01: 8 second-player stones on a first-player one, 7 first-player stones in the other column
    assert 0x3FE01 in f["keys"][runs == 8].tolist()
    assert R.columns_of(0x3FE01, 2, 9) == [[R.FIRST] + [R.SECOND] * 8, [R.FIRST] * 7]
    # (the host-twin comparison below takes every such position, whatever its sample leaves out)
    for dims in R.boards():
        if dims[2] < 8 or dims[1] < 8:
            assert int(longest_second_player_run(facts(oracle, dims)["keys"], dims[0], dims[1]).max()) < 8, dims
    want = {(7, 8, 4): 8, (3, 20, 4): 16, (2, 30, 4): 30, (1, 62, 4): 31}
    assert {d: 0 for d, _, _ in R.EDGE} == {d: 0 for d in want}
    for dims, key, positions in R.EDGE:
        L, H, K = dims
        assert R.valid(key, L, H), (dims, hex(key))
        keys, recs = table(oracle, dims, key)
        assert len(keys) == positions, (dims, hex(key))
        assert int(longest_second_player_run([key], L, H)[0]) == want[dims], (dims, hex(key))
        assert np.array_equal(R.primitive(keys, L, H, K) != UNDECIDED, (recs & 0x3FFF) == 0)


@pytest.mark.parametrize("dims,key,positions", R.EDGE, ids=["%dx%d_%d" % d for d, _, _ in R.EDGE])
def test_host_twin_agrees_with_the_oracle_below_the_edge_positions(oracle, dims, key, positions):
    import ctypes

    from gamesmanmpi_amd import games
    p, n = oracle._params(dims)
    kids = (ctypes.c_uint64 * 64)()
    nk, pr, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    hd = games.HostDescriptor(games.ConnectCodec(*dims))
    try:
        for k in table(oracle, dims, key)[0].tolist():
            assert oracle.L.oracle_expand(CONNECT, p, n, k, kids, ctypes.byref(nk), ctypes.byref(pr), ctypes.byref(t)) == 0
            assert hd.expand(k) == (pr.value, list(kids[:nk.value]), t.value), hex(k)
    finally:
        hd.close()


@pytest.mark.parametrize("dims", R.boards(), ids=["%dx%d_%d" % d for d in R.boards()])
def test_host_twin_agrees_with_the_oracle_on_swept_positions(oracle, dims):
    """The descriptor's host twin (gm_expand_host: DescConnect's filled / line / visit / tier / valid
    compiled for the CPU) against the oracle on the swept positions of every board, up to 6,000 spread
    over the key order and every one with 8 second-player stones on top of one another: the primitive code, the children in column order and the disc count."""
    import ctypes

    from gamesmanmpi_amd import games
    L, H, K = dims
    f = facts(oracle, dims)
    keys = f["keys"][:: max(1, f["n"] // 6000)]
    if H >= 8:      # and every position whose column fields need filled()'s long shifts
        keys = np.union1d(keys, f["keys"][longest_second_player_run(f["keys"], L, H) >= 8])
    p, n = oracle._params(dims)
    kids = (ctypes.c_uint64 * 64)()
    nk, pr, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    hd = games.HostDescriptor(games.ConnectCodec(L, H, K))
    try:
        assert hd.initial() == oracle.initial(CONNECT, dims)
        for k in keys.tolist():
            assert oracle.L.oracle_expand(CONNECT, p, n, k, kids, ctypes.byref(nk), ctypes.byref(pr), ctypes.byref(t)) == 0
            assert hd.expand(k) == (pr.value, list(kids[:nk.value]), t.value), hex(k)
        # positions that no game reaches are positions all the same: one disc past a finished line
        for k in R.after_the_end(f["keys"], f["recs"], L, H, most=20).tolist():
            assert R.valid(k, L, H) and hd.expand(k)[2] == sum(len(c) for c in R.columns_of(k, L, H))
    finally:
        hd.close()
