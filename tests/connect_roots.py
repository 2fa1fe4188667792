"""Connect boards and roots for the sweep of tests/test_gpu_connect_sweep.py: the full games solved
from the empty board, and mid-game roots as literals that a change of a generator cannot move
(tools/draw_connect_roots.py drew them; no test calls it).  tests/test_connect_roots.py holds the
conditions the set was drawn to meet and checks them with the C oracle (oracle/gm_oracle.c).

The helpers below read keys as arrays of cells and import nothing of gamesmanmpi_amd.  A key
(test_games/connect4.py, the DescConnect comment of csrc/games.hpp): column x owns the H + 1 bits
from bit x (H + 1) up; of a column of h discs bit h is set (the cap), nothing above it, and bit
y < h is set iff the disc in row y (0 = bottom) is the first player's.
"""
import numpy as np

CONNECT = 7
WIN, LOSS, TIE, UNDECIDED = 0, 1, 2, 4
FIRST, SECOND = 1, 2
U64 = np.uint64
# (dx, dy): up a column, along a row, the rising and the falling diagonal
DIRS = {"vertical": (0, 1), "horizontal": (1, 0), "diagonal": (1, 1), "antidiagonal": (1, -1)}

# ---------------------------------------------------------------- the swept boards
# full games from the empty board, (L, H, K), each at most 200,000 positions
FULL = (
    (2, 7, 4), (2, 8, 4), (2, 9, 4), (3, 8, 3), (2, 10, 5),     # H on both sides of filled()'s H > 7
    (2, 9, 8),      # the only way to a column of 8 second-player stones, which filled() needs its shift by 8 for
    (1, 62, 4), (1, 8, 2),                                      # one column
    (4, 4, 2), (6, 3, 2), (9, 1, 2), (8, 2, 2),                 # K = 2
    (7, 1, 4), (10, 1, 3), (12, 1, 4), (8, 1, 8),               # H = 1 and many columns
    (3, 5, 5), (4, 4, 5), (5, 3, 5),                            # K = 5
    (3, 4, 5),                                                  # K fits nowhere: every full board a TIE
)
FULL_MAX = 200000
NO_LINE = (3, 4, 5)

# drawn mid-game roots: (L, H, K), root key, its own mirror image?, how it was drawn.  "random": a
# position of a seeded random game; "paired": of a game of mirrored move groups; a direction: of a
# game steered so that it ends in a K-line of that direction that touches the top row; "built": put
# together by hand (tools/draw_connect_roots.py says how).  Each has 1,000 to 100,000 positions below.
DRAWN_MIN, DRAWN_MAX = 1000, 100000
DRAWN = (
    ((7, 8, 4), 0x23462AE079946431, False, "random"),        # seed 801, 72820 positions
    ((7, 8, 4), 0x08DD8B90A07AD06B, False, "random"),        # seed 1402, 2778
    ((7, 8, 4), 0x4943C1B8A06C3D25, True, "paired"),         # seed 203, 1325
    ((3, 20, 4), 0x6C651009D7203A67, False, "random"),       # seed 201, 1882
    ((3, 20, 4), 0x0134ABAC946058ED, False, "random"),       # seed 202, 1327
    ((3, 20, 4), 0x0CAB2C099A832ACB, True, "paired"),        # seed 103, 4162
    ((2, 30, 4), 0x00B36D3581648B49, False, "random"),       # seed 1, 1479
    ((2, 30, 4), 0x029A9556001B2B2D, False, "random"),       # seed 2, 2172
    ((2, 30, 4), 0x00AAAAAA81555555, True, "paired"),        # seed 3, 1479
    ((16, 2, 4), 0x000055759CDD7EA1, False, "random"),       # seed 101, 1214
    ((16, 2, 4), 0x0000D2D6926BFE63, False, "horizontal"),   # seed 102, 1860
    ((16, 2, 4), 0x0000CD3D17EA669E, True, "paired"),        # seed 3, 2003
    ((16, 2, 8), 0x0000E8EE8FB5BD24, False, "random"),       # seed 1, 1263
    ((16, 2, 8), 0x00004B5BB1F96CF1, False, "horizontal"),   # seed 102, 1209
    ((15, 3, 4), 0x095A51CAB427EBCF, False, "random"),       # seed 1, 1508
    ((15, 3, 4), 0x0A7A92E747E29A7A, True, "paired"),        # seed 3, 2547
    ((12, 4, 5), 0x01EF8BD48487CF74, False, "random"),       # seed 1, 1128
    ((12, 4, 5), 0x02FBF8DA0E585474, False, "horizontal"),   # seed 2, 1638
    ((12, 4, 5), 0x01AB177252EBE143, True, "paired"),        # seed 3, 42878
    ((8, 6, 6), 0x005F85A89F680753, False, "vertical"),      # seed 1, 1418
    ((8, 6, 6), 0x00D944B839F52C89, False, "horizontal"),    # seed 102, 1399
    ((8, 6, 6), 0x000FE8361AB2D62C, False, "diagonal"),      # seed 303, 1868
    ((8, 6, 6), 0x00322D29A9FAEA34, False, "antidiagonal"),  # seed 104, 1623
    ((7, 7, 7), 0x00583CD414217FCB, False, "vertical"),      # seed 1, 1588
    ((7, 7, 7), 0x00276221E4CFFB08, False, "horizontal"),    # seed 2, 1219
    ((7, 7, 7), 0x00784EC7A50A2D6C, False, "diagonal"),      # seed 3, 1386
    ((7, 7, 7), 0x00E9728601D4AB1D, False, "antidiagonal"),  # seed 4, 1455
    ((9, 6, 8), 0x049BA8E4F1B15C76, False, "random"),        # seed 1, 2489
    ((9, 6, 8), 0x6721A732EE5BC509, False, "horizontal"),    # seed 2, 1310
    ((16, 2, 2), 0x00002492534D34D3, False, "built"),        # 3714: all 16 columns open at the root
)

# Positions by the key's rules that no game from the empty board reaches, with a run of second-player
# stones (clear bits below the cap) too long for a K of at most 8: filled() needs its shift by 8 for a
# run of 8, by 16 for a run of 16 to 31 (no valid key holds a longer one: 1x62 has 31 stones a side).
# Once the second player has moved such a run is a line, so the subtrees are tiny: (L, H, K), key,
# positions below it.  tools/draw_connect_roots.py builds them.
EDGE = (
    ((7, 8, 4), 0x00C0F000780C1E02, 7),          # 8 second-player stones fill column 4, first player just moved
    ((3, 20, 4), 0x09DDDCEEEEE10000, 4),         # column 0: 16 second-player stones, first player just moved
    ((2, 30, 4), 0x3FFFFFFFC0000000, 1),         # full: 30 second-player stones left, 30 first-player right
    ((1, 62, 4), 0x7FFFFFFF80000000, 1),         # full: 31 second-player stones under 31 first-player ones
)


def boards():
    """Every swept (L, H, K), full games first."""
    out = list(FULL)
    for dims, _, _, _ in DRAWN:
        if dims not in out:
            out.append(dims)
    return out


def drawn_of(dims):
    return [r for r in DRAWN if r[0] == tuple(dims)]


# ---------------------------------------------------------------- keys as arrays of cells
def cells_of(keys, L, H):
    """(cells, heights): cells[n, x, y] = 0 empty, 1 the first player's, 2 the second player's;
    heights[n, x] = discs in column x, -1 where the column's field is zero (no position)."""
    keys = np.asarray(keys, dtype=U64).reshape(-1)
    cells = np.zeros((len(keys), L, H), dtype=np.int8)
    heights = np.zeros((len(keys), L), dtype=np.int64)
    for x in range(L):
        field = (keys >> U64(x * (H + 1))) % U64(1 << (H + 1))
        h = np.full(len(keys), -1, dtype=np.int64)
        for j in range(H + 1):
            h[(field >> U64(j)) % U64(2) == 1] = j      # the highest set bit is the cap
        heights[:, x] = h
        for y in range(H):
            stone = np.where((field >> U64(y)) % U64(2) == 1, FIRST, SECOND)
            cells[:, x, y] = np.where(y < h, stone, 0)
    return cells, heights


def key_of(columns, H):
    """A key from its columns, each a sequence of FIRST / SECOND from the bottom up."""
    key = 0
    for x, col in enumerate(columns):
        assert len(col) <= H
        field = 1 << len(col)
        for y, c in enumerate(col):
            if c == FIRST:
                field += 1 << y
        key += field << (x * (H + 1))
    return key


def columns_of(key, L, H):
    cells, heights = cells_of([key], L, H)
    return [[int(c) for c in cells[0, x, :heights[0, x]]] for x in range(L)]


def mirror(key, L, H):
    return key_of(columns_of(key, L, H)[::-1], H)


def mirror_keys(keys, L, H):
    """mirror() of every key of an array: the column fields in reverse order."""
    keys = np.asarray(keys, dtype=U64)
    out = np.zeros_like(keys)
    for x in range(L):
        field = (keys >> U64(x * (H + 1))) % U64(1 << (H + 1))
        out += field << U64((L - 1 - x) * (H + 1))
    return out


def after_the_end(keys, recs, L, H, most=200):
    """Positions one disc past a finished line: of up to `most` LOSS-in-0 positions with an open
    column, the one with the next disc in the first open column.  Positions by the key's rules
    (valid()), but no game reaches them through their parent."""
    out = []
    for k in np.asarray(keys)[np.asarray(recs) == (LOSS << 14)].tolist():
        cols = columns_of(k, L, H)
        discs = sum(len(c) for c in cols)
        for c in cols:
            if len(c) < H:
                c.append(FIRST if discs % 2 == 0 else SECOND)
                out.append(key_of(cols, H))
                break
        if len(out) >= most:
            break
    return np.array(out, dtype=U64)


def valid(key, L, H):
    """A position by the rules the DescConnect comment states: nothing at or above bit L (H + 1),
    a cap in every column field, and the first player's stones one more than half the discs,
    rounded down (the first player moves on an even count)."""
    if key < 0 or key >> (L * (H + 1)):
        return False
    cells, heights = cells_of([key], L, H)
    if (heights < 0).any():
        return False
    discs = int(heights.sum())
    return int((cells == FIRST).sum()) == (discs + 1) // 2


def last_mover(heights):
    """The colour of the player who just moved: the first player's on an odd disc count."""
    return np.where(heights.sum(axis=1) % 2 == 1, FIRST, SECOND).astype(np.int8)


def line_starts(mine, K, direction):
    """mine[n, x, y] bool -> starts[n, i, j] bool: K cells of `mine` from the start cell on, all on the
    board.  The start cell of starts[:, i, j] is (i, j) for vertical, horizontal and diagonal lines
    and (i, j + K - 1) for antidiagonal ones (which run down from there)."""
    n, L, H = mine.shape
    dx, dy = DIRS[direction]
    nx, ny = L - (K - 1) * dx, H - (K - 1) * abs(dy)
    if nx <= 0 or ny <= 0:
        return np.zeros((n, 0, 0), dtype=bool)
    out = np.ones((n, nx, ny), dtype=bool)
    for j in range(K):
        y0 = j * dy if dy >= 0 else K - 1 - j
        out &= mine[:, j * dx:j * dx + nx, y0:y0 + ny]
    return out


def fits(L, H, K, direction):
    dx, dy = DIRS[direction]
    return L - (K - 1) * dx > 0 and H - (K - 1) * abs(dy) > 0


def touches(starts, K, direction, what, L, H):
    """Per position: some line of `starts` has a cell in the top row / column 0 / column L - 1."""
    if starts.shape[1] == 0:
        return np.zeros(len(starts), dtype=bool)
    if what == "top":       # vertical and rising lines end in the top row, falling ones start there
        s = starts[:, :, -1]
    elif what == "left":
        s = starts[:, 0, :]
    else:                   # the line's last column (its own, if vertical) is L - 1
        s = starts[:, -1, :]
    return s.reshape(len(starts), -1).any(axis=1)


def primitive(keys, L, H, K):
    """The primitive code of every key, from the cells."""
    cells, heights = cells_of(keys, L, H)
    mine = cells == last_mover(heights)[:, None, None]
    lost = np.zeros(len(cells), dtype=bool)
    for d in DIRS:
        lost |= line_starts(mine, K, d).reshape(len(cells), -1).any(axis=1)
    full = heights.sum(axis=1) == L * H
    return np.where(lost, LOSS, np.where(full, TIE, UNDECIDED))


def wrap_strides(H):
    """The four strides of a board numbered x * H + y WITHOUT the guard row above every column."""
    return {"vertical": 1, "horizontal": H, "antidiagonal": H - 1, "diagonal": H + 1}


def wrap_runs(mine, K, stride):
    """Per position: K cells of `mine` at linear indices i, i + stride, .., i + (K - 1) stride of the
    x * H + y numbering, all below L * H.  Where the position holds no real line, such a run is no
    line: it leaves a column through the top row and goes on at the bottom of the next one."""
    flat = mine.reshape(len(mine), -1)
    m = flat.shape[1] - (K - 1) * stride
    if stride < 1 or m <= 0:
        return np.zeros(len(mine), dtype=bool)
    run = np.ones((len(mine), m), dtype=bool)
    for j in range(K):
        run &= flat[:, j * stride:j * stride + m]
    return run.any(axis=1)
