"""Roots of the two smallest descriptor games for the sweeps of tests/test_gpu_small_roots.py, and
the closed form of Four-To-One.  tests/test_small_roots.py holds the coverage conditions of the
tic-tac-toe subset and checks the closed form, and the C oracle on the subset, on the CPU.

Tic-tac-toe (csrc/games.hpp DescTTT): key = sum c_i 3^i, c_i 0 blank, 1 X, 2 O, and every key below
3^9 is a legal root -- also the boards no game reaches (any piece counts, two lines, full boards).
X moves when O has at least as many pieces, which only such boards tell from "X moves on an even
piece count".

Four-To-One (DescF2O): the key is the pile as a two's-complement u64, the moves take 1 or 2, a pile
of 0 or less is LOSS in 0.  From a root n >= 1 the positions are n, n-1, ..., 0 and -1, one per
tier, so the depth of a solve is the root and only this game reaches the end of the 14-bit
remoteness: k = 3m is LOSS in 2m, k = 3m+1 and 3m+2 are WIN in 2m+1.
"""
import numpy as np

WIN, LOSS, TIE = 0, 1, 2
MAX_REM = 0x3FFF
U64 = 1 << 64

# ---------------------------------------------------------------- tic-tac-toe
TTT_SLOTS = 3 ** 9
TTT_ALL = range(TTT_SLOTS)


def ttt_cells(key):
    return [key // 3 ** i % 3 for i in range(9)]


def ttt_counts(key):
    """(number of X, number of O)."""
    c = ttt_cells(key)
    return c.count(1), c.count(2)


def ttt_pieces(key):
    return 9 - ttt_cells(key).count(0)


def _strata(per_pair=40):
    """For every (number of X, number of O) the first `per_pair` keys in numeric order."""
    by_pair = {}
    for k in TTT_ALL:
        by_pair.setdefault(ttt_counts(k), []).append(k)
    return tuple(sorted(k for ks in by_pair.values() for k in ks[:per_pair]))


TTT_STRATA = _strata()
TTT_BY_PIECES = tuple(tuple(k for k in TTT_ALL if ttt_pieces(k) == p) for p in range(10))


def ttt_outside_key(root):
    """A board no solve from `root` holds, with fewer pieces than the root: the root less its
    lowest piece (a move only adds pieces).  The empty board has no such board; for it, a lone O
    (key 2), which play from the empty board never reaches: X moves first."""
    c = ttt_cells(root)
    for i in range(9):
        if c[i]:
            return root - c[i] * 3 ** i
    return 2


def shuffled(roots, seed=0):
    """The fixed order the device sweeps walk a root list in: a large solve is followed by a
    small one, whatever the numeric order would give."""
    roots = list(roots)
    return [roots[i] for i in np.random.default_rng(seed).permutation(len(roots))]


# ---------------------------------------------------------------- Four-To-One
F2O_DEEPEST = 24575         # WIN in 0x3FFF: the deepest root with a table
F2O_FIRST_REFUSED = 24576   # LOSS in 0x4000: no record holds it
F2O_IMPORT_DEEPEST = 1022   # gm_import takes keys up to 1,023 tiers below the root; -1 is root + 1 below
F2O_SMALL = tuple(range(-3, 41))
F2O_CPU = tuple(range(-3, 61)) + (F2O_IMPORT_DEEPEST, F2O_IMPORT_DEEPEST + 1, 3000, 7000, F2O_DEEPEST)


def f2o_key(pile):
    return pile % U64


def f2o_record(pile):
    """The record of a pile, by the closed form; ValueError past the 14 bits."""
    if pile <= 0:
        return LOSS << 14
    m, r = divmod(pile, 3)
    value, rem = (LOSS, 2 * m) if r == 0 else (WIN, 2 * m + 1)
    if rem > MAX_REM:
        raise ValueError("pile %d: remoteness %d exceeds 14 bits" % (pile, rem))
    return value << 14 | rem


def f2o_table(root):
    """(keys, records) of a solve from `root` as gm_export gives them: uint64 keys in unsigned
    order (-1 is 2^64 - 1 and sorts last), uint16 records."""
    piles = [root] if root <= 0 else list(range(root + 1)) + [-1]
    keys = np.array([f2o_key(p) for p in piles], dtype=np.uint64)
    recs = np.array([f2o_record(p) for p in piles], dtype=np.uint16)
    return keys, recs


def histogram_of(recs):
    """The (3, n_rem) census of u16 records as gm_histogram gives it, rows WIN, LOSS, TIE."""
    recs = np.asarray(recs, dtype=np.uint16)
    val, rem = recs >> 14, recs & MAX_REM
    out = np.zeros((3, int(rem.max()) + 1), dtype=np.uint64)
    for v in range(3):
        out[v] = np.bincount(rem[val == v], minlength=out.shape[1])
    return out


def f2o_histogram(root):
    """The census of f2o_table(root)."""
    return histogram_of(f2o_table(root)[1])
