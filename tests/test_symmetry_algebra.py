"""The symmetry reductions of csrc/games.hpp, checked on the host against plain numpy.

The sparse engines store one representative per symmetry orbit: DescOthello::canon / orbit /
stabilizer reduce by the subgroup of the square's dihedral group D4 that fixes the root,
DescToot::mirror / canon / orbit by the left-right mirror.  The functions are compiled from the
header itself (tests/csrc/games_shim.cpp) and compared with a reference that works on the board
as an array, a[y][x] = (plane >> (L*y + x)) & 1, with np.rot90, .T and reversed slices.  Also
asserted here: what the reductions rest on (games.hpp states it in comments) -- Othello's rules
are D4-equivariant with colours kept, Toot's are mirror-equivariant, and visit_part over all
lanes is visit.
"""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

U64 = np.uint64
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)   # no key: bits 0..15 of a key are never all ones here
UNDECIDED = 4
OTH_MAXC, TOOT_MAXC = 24, 16

# the 10 subgroups of D4 as bit masks over g = 0..7 (games.hpp DescOthello::sym)
SUBGROUPS = [0x01, 0x05, 0x11, 0x21, 0x41, 0x81, 0x0F, 0x35, 0xC5, 0xFF]


def mask_of(gs):
    return sum(1 << g for g in gs)


assert SUBGROUPS == [mask_of(s) for s in ([0], [0, 2], [0, 4], [0, 5], [0, 6], [0, 7], [0, 1, 2, 3], [0, 2, 4, 5],
                                           [0, 2, 6, 7], range(8))]


def elements(mask):
    return [g for g in range(8) if (mask >> g) & 1]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("games_shim") / "libgames_shim.so")
    src = os.path.join(REPO, "tests", "csrc", "games_shim.cpp")
    flags = ["-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(REPO, "gamesmanmpi_amd", "csrc"), src, "-o", out]
    # host-only, with ROCm's clang: games.hpp uses __builtin_bitreverse32, which g++ does not have
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    clang = os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    if os.path.exists(clang):
        cmd = [clang] + flags
    else:
        hipcc = shutil.which("hipcc") or os.path.join(rocm, "bin", "hipcc")
        cmd = [hipcc, "-x", "c++"] + flags
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "%s\n%s%s" % (" ".join(cmd), r.stdout, r.stderr)
    return Shim(ctypes.CDLL(out))


class Shim:
    """Array calls into games_shim.cpp: scalars first, then the input array, then the outputs."""

    def __init__(self, lib):
        self.lib = lib

    def _call(self, name, scalars, x, in_dtype, outs):
        x = np.ascontiguousarray(np.atleast_1d(x), dtype=in_dtype)
        n = len(x)
        arrs = [np.full((n, w) if w else n, 0, dtype=dt) for dt, w in outs]
        f = getattr(self.lib, "shim_" + name)
        f.restype = None
        f.argtypes = [ctypes.c_int] * len(scalars) + [ctypes.c_void_p] * (1 + len(arrs)) + [ctypes.c_size_t]
        f(*[int(s) for s in scalars], x.ctypes.data, *[a.ctypes.data for a in arrs], n)
        return arrs[0] if len(arrs) == 1 else arrs

    def make(self, game, L, H):
        f = getattr(self.lib, "shim_%s_make" % game)
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_int, ctypes.c_int]
        return bool(f(L, H))

    def _lists(self, out, cnt, width):
        """(n, width) children / orbit slots and their counts -> slots past the count set to PAD."""
        assert cnt.min() >= 0 and cnt.max() <= width, (cnt.min(), cnt.max())
        out[np.arange(width)[None, :] >= cnt[:, None]] = PAD
        return out, cnt

    # Othello: xform_plane4 is static; the other calls take L, some take sym
    def oth_xform_plane4(self, p, g):
        # g goes between the arrays in the shim's signature
        p = np.ascontiguousarray(p, dtype=np.uint32)
        out = np.empty(len(p), dtype=np.uint32)
        f = self.lib.shim_oth_xform_plane4
        f.restype = None
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
        f(p.ctypes.data, g, out.ctypes.data, len(p))
        return out

    def oth_xform_plane_cells(self, L, p, g):
        p = np.ascontiguousarray(p, dtype=np.uint32)
        out = np.empty(len(p), dtype=np.uint32)
        f = self.lib.shim_oth_xform_plane_cells
        f.restype = None
        f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
        f(L, p.ctypes.data, g, out.ctypes.data, len(p))
        return out

    def oth_xform(self, L, k, g):
        k = np.ascontiguousarray(k, dtype=U64)
        out = np.empty(len(k), dtype=U64)
        f = self.lib.shim_oth_xform
        f.restype = None
        f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
        f(L, k.ctypes.data, g, out.ctypes.data, len(k))
        return out

    def oth_canon(self, L, sym, k):
        return self._call("oth_canon", (L, sym), k, U64, [(U64, 0)])

    def oth_stabilizer(self, L, k):
        return self._call("oth_stabilizer", (L,), k, U64, [(np.uint32, 0)])

    def oth_orbit(self, L, sym, k):
        return self._lists(*self._call("oth_orbit", (L, sym), k, U64, [(U64, 16), (np.int32, 0)]), 16)

    def oth_children(self, L, sym, k):
        return self._lists(*self._call("oth_children", (L, sym), k, U64, [(U64, OTH_MAXC), (np.int32, 0)]), OTH_MAXC)

    def oth_visit_part(self, L, sym, part, nparts, k):
        return self._lists(*self._call("oth_visit_part", (L, sym, part, nparts), k, U64,
                                       [(U64, OTH_MAXC), (np.int32, 0)]), OTH_MAXC)

    def oth_pass_child(self, L, sym, k):
        return self._call("oth_pass_child", (L, sym), k, U64, [(U64, 0)])

    def oth_primitive(self, L, k):
        return self._call("oth_primitive", (L,), k, U64, [(np.int32, 0)])

    def oth_tier(self, L, k):
        return self._call("oth_tier", (L,), k, U64, [(np.int64, 0)])

    def oth_valid(self, L, k):
        return self._call("oth_valid", (L,), k, U64, [(np.uint8, 0)]).astype(bool)

    # Toot-and-Otto
    def toot_mirror_plane(self, L, H, p):
        return self._call("toot_mirror_plane", (L, H), p, np.uint32, [(np.uint32, 0)])

    def toot_mirror(self, L, H, k):
        return self._call("toot_mirror", (L, H), k, U64, [(U64, 0)])

    def toot_canon(self, L, H, sym, k):
        return self._call("toot_canon", (L, H, sym), k, U64, [(U64, 0)])

    def toot_orbit(self, L, H, sym, k):
        return self._lists(*self._call("toot_orbit", (L, H, sym), k, U64, [(U64, 4), (np.int32, 0)]), 4)

    def toot_children(self, L, H, sym, k):
        return self._lists(*self._call("toot_children", (L, H, sym), k, U64, [(U64, TOOT_MAXC), (np.int32, 0)]),
                           TOOT_MAXC)

    def toot_primitive(self, L, H, k):
        return self._call("toot_primitive", (L, H), k, U64, [(np.int32, 0)])

    def toot_tier(self, L, H, k):
        return self._call("toot_tier", (L, H), k, U64, [(np.int64, 0)])

    def toot_valid(self, L, H, k):
        return self._call("toot_valid", (L, H), k, U64, [(np.uint8, 0)]).astype(bool)


# ---------------------------------------------------------------- the numpy reference
def boards(planes, L, H):
    """planes -> (n, H, L) arrays, a[y][x] = (p >> (L*y + x)) & 1."""
    p = np.asarray(planes, dtype=U64)
    return ((p[:, None] >> np.arange(L * H, dtype=U64)[None, :]) & U64(1)).astype(np.uint8).reshape(-1, H, L)


def planes_of(a):
    n, H, L = a.shape
    w = U64(1) << np.arange(L * H, dtype=U64)
    return (a.reshape(n, L * H).astype(U64) * w[None, :]).sum(axis=1, dtype=U64)


def d4(a, g):
    """Element g of D4 on (n, L, L) boards; the numbering is that of xform_plane_cells, whose
    formulas send cell (x, y) to (nx, ny): out[ny][nx] = a[y][x]."""
    if g == 0:
        return a
    if g == 1:   # (L-1-y, x): a quarter turn
        return np.rot90(a, -1, axes=(1, 2))
    if g == 2:   # (L-1-x, L-1-y): a half turn
        return np.rot90(a, 2, axes=(1, 2))
    if g == 3:   # (y, L-1-x): the other quarter turn
        return np.rot90(a, 1, axes=(1, 2))
    if g == 4:   # (y, x)
        return a.transpose(0, 2, 1)
    if g == 5:   # (L-1-y, L-1-x)
        return a[:, ::-1, ::-1].transpose(0, 2, 1)
    if g == 6:   # (L-1-x, y)
        return a[:, :, ::-1]
    if g == 7:   # (x, L-1-y)
        return a[:, ::-1]
    raise ValueError(g)


def ref_plane(planes, g, L):
    return planes_of(d4(boards(planes, L, L), g))


def oth_split(k, L):
    A = L * L
    k = np.asarray(k, dtype=U64)
    m = U64((1 << A) - 1)
    return (k >> U64(A + 16)) & m, (k >> U64(16)) & m, k & U64(0xFFFF)


def oth_join(w, b, low, L):
    return (w.astype(U64) << U64(L * L + 16)) | (b.astype(U64) << U64(16)) | low.astype(U64)


def ref_xform(k, g, L):
    w, b, low = oth_split(k, L)
    return oth_join(ref_plane(w, g, L), ref_plane(b, g, L), low, L)


def ref_images(k, L):
    """(8, n): image of every key under every element."""
    return np.stack([ref_xform(k, g, L) for g in range(8)])


def ref_stabilizer(img):
    s = np.zeros(img.shape[1], dtype=np.uint32)
    for g in range(8):
        s |= (img[g] == img[0]).astype(np.uint32) << np.uint32(g)
    return s


def ref_canon(img, S):
    return img[elements(S)].min(axis=0)


def popcount(x):
    x = np.asarray(x, dtype=U64)
    n = np.zeros(x.shape, dtype=np.int64)
    for i in range(64):
        n += ((x >> U64(i)) & U64(1)).astype(np.int64)
    return n


def sorted_rows(a):
    return np.sort(a, axis=1)


def oth_keys(L, n, seed):
    """Seeded random valid keys: every cell empty / white / black at a density drawn per key,
    turn 1 or 2, pass 0, 1 or 2."""
    rng = np.random.default_rng(seed)
    A = L * L
    fill = rng.random((n, 1))
    u = rng.random((n, A))
    colour = rng.random((n, A)) < rng.random((n, 1))
    occ = u < fill
    w = planes_of((occ & colour).astype(np.uint8).reshape(n, L, L))
    b = planes_of((occ & ~colour).astype(np.uint8).reshape(n, L, L))
    low = (rng.integers(1, 3, n).astype(U64) << U64(8)) | rng.integers(0, 3, n).astype(U64)
    return oth_join(w, b, low, L)


def symmetrised(k, S, L):
    """Keys fixed by every element of S: white is the union of the white plane's images, black
    the union of the black plane's images off white."""
    w, b, low = oth_split(k, L)
    ws, bs = np.zeros_like(w), np.zeros_like(b)
    for g in elements(S):
        ws |= ref_plane(w, g, L)
        bs |= ref_plane(b, g, L)
    return oth_join(ws, bs & ~ws, low, L)


@pytest.fixture(scope="module")
def oth4(shim):
    """The 4x4 sample every Othello test shares: 20,000 random keys and 1,500 symmetrised under
    each subgroup, with their reference images (left unchanged by the tests)."""
    base = oth_keys(4, 20000, 11)
    extra = [symmetrised(oth_keys(4, 1500, 100 + i), S, 4) for i, S in enumerate(SUBGROUPS)]
    k = np.unique(np.concatenate([base] + extra))
    assert len(k) >= 20000 and shim.oth_valid(4, k).all()
    img = ref_images(k, 4)
    k.setflags(write=False)
    img.setflags(write=False)
    return k, img


# ---------------------------------------------------------------- Othello: the plane transforms
def test_xform_plane4_is_the_cell_loop_is_numpy_on_every_plane(shim):
    p = np.arange(1 << 16, dtype=np.uint32)
    for g in range(8):
        ref = ref_plane(p, g, 4).astype(np.uint32)
        assert np.array_equal(shim.oth_xform_plane_cells(4, p, g), ref), g
        assert np.array_equal(shim.oth_xform_plane4(p, g), ref), g


@pytest.mark.parametrize("L", [2, 4])
def test_cell_permutations_form_d4(shim, L):
    """Eight distinct permutations of the cells, closed under composition, each with its inverse
    in the set; closure of every pair of elements gives exactly the 10 subgroups."""
    A = L * L
    bits = (np.uint32(1) << np.arange(A, dtype=np.uint32))
    perm = []
    for g in range(8):
        out = shim.oth_xform_plane_cells(L, bits, g)
        assert (popcount(out) == 1).all()
        perm.append(tuple(int(x).bit_length() - 1 for x in out))
        assert sorted(perm[-1]) == list(range(A))
    assert len(set(perm)) == 8 and perm[0] == tuple(range(A))
    index = {p: g for g, p in enumerate(perm)}
    table = [[index.get(tuple(perm[g][perm[h][c]] for c in range(A))) for h in range(8)] for g in range(8)]
    assert all(x is not None for row in table for x in row)               # closed
    assert all(0 in table[g] for g in range(8))                           # inverses
    # what the descriptor's comments name them: 2 the half turn, 1 and 3 the quarter turns
    assert table[1][1] == 2 and table[3][3] == 2 and table[1][3] == 0 and table[2][2] == 0
    assert all(table[g][g] == 0 for g in (4, 5, 6, 7))

    def closure(gen):
        s = {0} | set(gen)
        while True:
            t = s | {table[a][b] for a in s for b in s}
            if t == s:
                return mask_of(s)
            s = t

    found = {closure(gen) for gen in itertools.product(range(8), repeat=2)}
    assert found == set(SUBGROUPS)
    assert closure(range(8)) == 0xFF


@pytest.mark.parametrize("L", [2, 4])
def test_xform_is_the_reference_and_keeps_the_low_bits(shim, oth4, L):
    k = oth4[0] if L == 4 else oth_keys(2, 2000, 5)
    for g in range(8):
        t = shim.oth_xform(L, k, g)
        assert np.array_equal(t, ref_xform(k, g, L)), g
        assert np.array_equal(t & U64(0xFFFF), k & U64(0xFFFF)), g
        assert np.array_equal(popcount(t), popcount(k)), g
    assert np.array_equal(shim.oth_xform(L, k, 0), k)


# ---------------------------------------------------------------- Othello: canon / orbit / stabilizer
def check_reduction(shim, L, k, img):
    """canon, orbit and stabilizer of the keys k (reference images img) under each subgroup."""
    stab = ref_stabilizer(img)
    assert np.array_equal(shim.oth_stabilizer(L, k), stab)
    assert set(np.unique(stab).tolist()) <= set(SUBGROUPS)
    for S in SUBGROUPS:
        gs = elements(S)
        want = ref_canon(img, S)
        got = shim.oth_canon(L, S, k)
        assert np.array_equal(got, want), hex(S)
        assert np.array_equal(shim.oth_canon(L, S, got), got), hex(S)                 # idempotent
        for g in gs:                                                                   # constant on the orbit
            assert np.array_equal(shim.oth_canon(L, S, img[g]), want), (hex(S), g)
        orb, cnt = shim.oth_orbit(L, S, k)
        assert np.array_equal(orb[:, 0], k), hex(S)
        # the distinct images, each once: rows equal as sorted lists with duplicates removed
        ref = np.full((len(k), 16), PAD, dtype=U64)
        ref[:, :len(gs)] = img[gs].T
        ref = sorted_rows(ref)
        ref[:, 1:][ref[:, 1:] == ref[:, :-1]] = PAD
        assert np.array_equal(sorted_rows(orb), sorted_rows(ref)), hex(S)
        inside = popcount(stab & np.uint32(S))
        assert np.array_equal(cnt * inside, np.full(len(k), len(gs))), hex(S)         # |S| / |S n stab(k)|
    return stab


def test_canon_orbit_stabilizer_4x4(shim, oth4):
    k, img = oth4
    stab = check_reduction(shim, 4, k, img)
    # the sample reaches every subgroup as a stabiliser
    assert set(np.unique(stab).tolist()) == set(SUBGROUPS)


def test_canon_orbit_stabilizer_2x2_exhaustive(shim):
    """L = 2 goes through the cell loop: all 3^4 boards, both turns, every pass count."""
    keys = []
    for cells in itertools.product(range(3), repeat=4):
        w = sum(1 << i for i, c in enumerate(cells) if c == 1)
        b = sum(1 << i for i, c in enumerate(cells) if c == 2)
        for turn in (1, 2):
            for ps in (0, 1, 2):
                keys.append((w << 20) | (b << 16) | (turn << 8) | ps)
    k = np.array(sorted(keys), dtype=U64)
    assert len(k) == 81 * 2 * 3 and shim.oth_valid(2, k).all()
    stab = check_reduction(shim, 2, k, ref_images(k, 2))
    # (on four cells a board the half turn fixes is fixed by both diagonal reflections too, so
    # 0x05, 0x0F and 0xC5 are no board's stabiliser)
    assert 0x01 in stab and 0xFF in stab and 0x35 in stab


# ---------------------------------------------------------------- Othello: the rules are equivariant
def play_keys(k):
    """Keys a solve expands children of: pass count 0 or 1."""
    return k[(k & U64(0xFF)) <= U64(1)]


def test_othello_rules_are_d4_equivariant(shim, oth4):
    k = play_keys(oth4[0])
    prim, tier = shim.oth_primitive(4, k), shim.oth_tier(4, k)
    kids, cnt = shim.oth_children(4, 0, k)
    passes = (cnt == 1) & (kids[:, 0] == k + U64(1))
    assert passes.sum() >= 100 and ((k & U64(0xFF)) == U64(1)).sum() >= 100
    assert (passes & ((k & U64(0xFF)) == U64(1))).sum() >= 10
    assert (cnt >= 1).all() and (cnt[~passes] >= 1).all() and (prim == UNDECIDED).sum() >= 1000
    for g in range(8):
        t = ref_xform(k, g, 4)
        assert np.array_equal(shim.oth_primitive(4, t), prim), g
        assert np.array_equal(shim.oth_tier(4, t), tier), g
        assert shim.oth_valid(4, t).all(), g
        tk, tc = shim.oth_children(4, 0, t)
        assert np.array_equal(tc, cnt), g
        want = ref_xform(kids.reshape(-1), g, 4).reshape(kids.shape)
        want[kids == PAD] = PAD
        assert np.array_equal(sorted_rows(tk), sorted_rows(want)), g


def test_othello_children_under_sym_are_canonical_children_in_order(shim, oth4):
    k = play_keys(oth4[0])
    kids, cnt = shim.oth_children(4, 0, k)
    flat = kids.reshape(-1)
    img = ref_images(np.where(flat == PAD, U64(0), flat), 4)
    for S in SUBGROUPS:
        want = ref_canon(img, S).reshape(kids.shape)
        want[kids == PAD] = PAD
        got, gc = shim.oth_children(4, S, k)
        assert np.array_equal(gc, cnt) and np.array_equal(got, want), hex(S)


@pytest.mark.parametrize("sym", [0, 0x35])
@pytest.mark.parametrize("nparts", [16, 4])
def test_visit_part_over_all_lanes_is_visit(shim, oth4, sym, nparts):
    """The children of all parts, put back in square order, are children(k); no part finds a
    move exactly when children(k) is the pass child.  The square of a child is the one the
    occupied plane gains, read from the unreduced (sym = 0) run of the same part."""
    k = play_keys(oth4[0])
    w, b, _ = oth_split(k, 4)
    occ = w | b
    by_square = np.full((len(k), 16), PAD, dtype=U64)
    total = np.zeros(len(k), dtype=np.int64)
    for part in range(nparts):
        plain, pc = shim.oth_visit_part(4, 0, part, nparts, k)
        got, gc = shim.oth_visit_part(4, sym, part, nparts, k)
        assert np.array_equal(gc, pc)
        total += gc
        for j in range(int(gc.max())):
            rows = np.nonzero(gc > j)[0]
            cw, cb, _ = oth_split(plain[rows, j], 4)
            placed = (cw | cb) & ~occ[rows]
            assert (popcount(placed) == 1).all()
            sq = np.log2(placed.astype(np.float64)).astype(np.int64)
            assert (sq % nparts == part).all()
            assert (by_square[rows, sq] == PAD).all()
            by_square[rows, sq] = got[rows, j]
    # squares in order, the empty ones squeezed out
    order = np.argsort(by_square == PAD, axis=1, kind="stable")
    packed = np.take_along_axis(by_square, order, axis=1)
    kids, cnt = shim.oth_children(4, sym, k)
    moved = total > 0
    assert moved.sum() >= 1000 and (~moved).sum() >= 100
    assert np.array_equal(cnt[moved], total[moved])
    assert np.array_equal(kids[moved][:, :16], packed[moved]) and (kids[moved][:, 16:] == PAD).all()
    assert (cnt[~moved] == 1).all()
    assert np.array_equal(kids[~moved][:, 0], shim.oth_pass_child(4, sym, k[~moved]))
    img = ref_images(k[~moved] + U64(1), 4)
    assert np.array_equal(kids[~moved][:, 0], ref_canon(img, sym | 1))


def test_othello_make_takes_even_square_boards_a_key_holds(shim):
    took = [(L, H) for L in range(0, 9) for H in range(0, 9) if shim.make("oth", L, H)]
    assert took == [(2, 2), (4, 4)]


# ---------------------------------------------------------------- Toot-and-Otto
TOOT_SHAPES = [(L, H) for L in range(1, 9) for H in range(1, 25) if L * H <= 24]
TOOT_ROOT = 0x6666   # empty planes, hands 6/6/6/6


def ref_mirror_plane(p, L, H):
    return planes_of(boards(p, L, H)[:, :, ::-1])


def toot_split(k, L, H):
    A = L * H
    k = np.asarray(k, dtype=U64)
    m = U64((1 << A) - 1)
    return (k >> U64(A + 16)) & m, (k >> U64(16)) & m, k & U64(0xFFFF)


def ref_mirror(k, L, H):
    t, o, low = toot_split(k, L, H)
    return (ref_mirror_plane(t, L, H) << U64(L * H + 16)) | (ref_mirror_plane(o, L, H) << U64(16)) | low


def test_toot_make_takes_every_board_the_tests_cover(shim):
    took = [(L, H) for L in range(0, 10) for H in range(0, 26) if shim.make("toot", L, H)]
    assert took == TOOT_SHAPES and len(TOOT_SHAPES) == 64


@pytest.mark.parametrize("L,H", TOOT_SHAPES)
def test_toot_mirror_plane_is_numpy(shim, L, H):
    A = L * H
    if A <= 16:
        p = np.arange(1 << A, dtype=np.uint32)
    else:
        p = np.random.default_rng(1000 * L + H).integers(0, 1 << A, 100000, dtype=np.uint32)
        p[:4] = [0, (1 << A) - 1, 1, 1 << (A - 1)]
    got = shim.toot_mirror_plane(L, H, p)
    assert np.array_equal(got, ref_mirror_plane(p, L, H).astype(np.uint32))
    assert np.array_equal(shim.toot_mirror_plane(L, H, got), p)           # an involution
    assert np.array_equal(popcount(got), popcount(p))


def toot_random_keys(L, H, n, seed):
    """Any bits below 2A + 16, a third of them made mirror-symmetric."""
    rng = np.random.default_rng(seed)
    A = L * H
    t = rng.integers(0, 1 << A, n, dtype=np.uint64)
    o = rng.integers(0, 1 << A, n, dtype=np.uint64)
    s = rng.random(n) < 1 / 3
    t[s] |= ref_mirror_plane(t[s], L, H)
    o[s] |= ref_mirror_plane(o[s], L, H)
    return np.unique((t << U64(A + 16)) | (o << U64(16)) | rng.integers(0, 1 << 16, n, dtype=np.uint64))


def check_toot_reduction(shim, L, H, k):
    m = ref_mirror(k, L, H)
    got = shim.toot_mirror(L, H, k)
    assert np.array_equal(got, m)
    assert np.array_equal(got & U64(0xFFFF), k & U64(0xFFFF))
    t, o, _ = toot_split(k, L, H)
    mt, mo, _ = toot_split(got, L, H)
    assert np.array_equal(mt, ref_mirror_plane(t, L, H)) and np.array_equal(mo, ref_mirror_plane(o, L, H))
    assert np.array_equal(shim.toot_mirror(L, H, got), k)
    # sym = 0: no reduction
    assert np.array_equal(shim.toot_canon(L, H, 0, k), k)
    orb, cnt = shim.toot_orbit(L, H, 0, k)
    assert (cnt == 1).all() and np.array_equal(orb[:, 0], k)
    # sym = 1: the smaller of the key and its mirror image; the orbit is both, or the one
    want = np.minimum(k, m)
    c = shim.toot_canon(L, H, 1, k)
    assert np.array_equal(c, want)
    assert np.array_equal(shim.toot_canon(L, H, 1, c), c) and np.array_equal(shim.toot_canon(L, H, 1, m), want)
    orb, cnt = shim.toot_orbit(L, H, 1, k)
    assert np.array_equal(orb[:, 0], k)
    assert np.array_equal(cnt, np.where(m == k, 1, 2))
    assert np.array_equal(orb[:, 1], np.where(m == k, PAD, m))
    return m


@pytest.mark.parametrize("L,H", TOOT_SHAPES)
def test_toot_mirror_canon_orbit(shim, L, H):
    k = toot_random_keys(L, H, 20000, 77 * L + H)
    m = check_toot_reduction(shim, L, H, k)
    if L > 1:
        assert (m == k).sum() >= 10 and (m != k).sum() >= 1000
    else:
        assert (m == k).all()
    # valid() does not tell a position from its mirror image
    assert np.array_equal(shim.toot_valid(L, H, m), shim.toot_valid(L, H, k))


def toot_playout_keys(shim, L, H, games, seed):
    """Every position of seeded random playouts from the empty board, through the shim's
    own children() so that gravity and the hands hold."""
    rng = np.random.default_rng(seed)
    cur = np.full(games, TOOT_ROOT, dtype=U64)
    seen = [cur]
    while len(cur):
        cur = cur[shim.toot_primitive(L, H, cur) == UNDECIDED]
        if not len(cur):
            break
        kids, cnt = shim.toot_children(L, H, 0, cur)
        live = cnt > 0
        pick = (rng.random(len(cur)) * cnt).astype(np.int64)
        cur = kids[np.arange(len(cur)), np.minimum(pick, np.maximum(cnt - 1, 0))][live]
        seen.append(cur)
    return np.unique(np.concatenate(seen))


@pytest.mark.parametrize("L,H", TOOT_SHAPES)
def test_toot_rules_are_mirror_equivariant(shim, L, H):
    k = toot_playout_keys(shim, L, H, 300, 31 * L + H)
    assert len(k) > min(L * H, 3) and shim.toot_valid(L, H, k).all()
    m = check_toot_reduction(shim, L, H, k)
    assert shim.toot_valid(L, H, m).all()
    assert np.array_equal(shim.toot_primitive(L, H, m), shim.toot_primitive(L, H, k))
    assert np.array_equal(shim.toot_tier(L, H, m), shim.toot_tier(L, H, k))
    assert np.array_equal(shim.toot_tier(L, H, k), popcount(k >> U64(16)))
    kids, cnt = shim.toot_children(L, H, 0, k)
    flat = kids.reshape(-1)
    mk = ref_mirror(np.where(flat == PAD, U64(0), flat), L, H).reshape(kids.shape)
    mk[kids == PAD] = PAD
    got, gc = shim.toot_children(L, H, 0, m)
    assert np.array_equal(gc, cnt) and np.array_equal(sorted_rows(got), sorted_rows(mk))
    red, rc = shim.toot_children(L, H, 1, k)
    assert np.array_equal(rc, cnt) and np.array_equal(red, np.minimum(kids, mk))
