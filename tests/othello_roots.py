"""Synthetic Othello roots for the sweeps of tests/test_gpu_othello_sweep.py, as literals: drawn sets
that a change of a generator cannot move (tools/draw_othello_roots.py drew them; no test calls it).
tests/test_othello_roots.py holds the conditions the sets were drawn to meet and walks every root's
subtree once with the reference generator below against the two C oracles.

The reference generator is a walk over squares and directions on a cell array, written here from
the rules of the reference plugin (test_games/othello_bit_new.py) and importing nothing of
gamesmanmpi_amd.  A position is the plugin's string read as one big-endian integer,

    I = W << (A + 16) | B << 16 | turn << 8 | pass        (A = L * L, turn 1 black, 2 white)

where string bit j = L * y + x of a plane is plane bit A - 1 - j.  On 4x4 that integer is the key
of DescOthello; on 8x8 its three little-endian u64 words are the ABI key of include/gmsolve.h.
"""

WIN, LOSS, TIE, UNDECIDED = 0, 1, 2, 4
BLACK, WHITE = 1, 2
# the plugin's legit_move walks dx outer, dy inner; the index into DIRS names a direction
DIRS = tuple((dx, dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if dx or dy)
CENTRE8 = ((3, 3), (4, 3), (3, 4), (4, 4))
MASK64 = (1 << 64) - 1


def words_of(key):
    """8x8: I -> (w0, w1, w2)."""
    return key & MASK64, (key >> 64) & MASK64, key >> 128


def key_of(words):
    return int(words[0]) | (int(words[1]) << 64) | (int(words[2]) << 128)


def split(L, key):
    """I -> (white plane, black plane, turn, pass)."""
    A = L * L
    m = (1 << A) - 1
    return (key >> (A + 16)) & m, (key >> 16) & m, (key >> 8) & 0xFF, key & 0xFF


def join(L, white, black, turn, npass):
    return (white << (L * L + 16)) | (black << 16) | (turn << 8) | npass


def cells_of(L, key):
    """The board as a list, cell[L * y + x] = 0 empty, 1 black, 2 white."""
    A = L * L
    white, black, _, _ = split(L, key)
    w, b = format(white, "0%db" % A), format(black, "0%db" % A)
    return [WHITE if w[j] == "1" else (BLACK if b[j] == "1" else 0) for j in range(A)]


def key_from_cells(L, cells, turn, npass):
    A = L * L
    white = sum(1 << (A - 1 - j) for j in range(A) if cells[j] == WHITE)
    black = sum(1 << (A - 1 - j) for j in range(A) if cells[j] == BLACK)
    return join(L, white, black, turn, npass)


def valid(L, key):
    """A position of the descriptor: disjoint planes, turn 1 or 2, pass byte at most 2, nothing
    above the string's bits; on 8x8 the four centre squares occupied (DescOthello8 reuses them)."""
    white, black, turn, npass = split(L, key)
    if key >> (2 * L * L + 16) or white & black or turn not in (1, 2) or npass > 2:
        return False
    if L == 8:
        cells = cells_of(L, key)
        return all(cells[8 * y + x] for x, y in CENTRE8)
    return True


def empties(L, key):
    white, black, _, _ = split(L, key)
    return L * L - bin(white | black).count("1")


def primitive(L, key):
    """A full board or a second pass ends the game: TIE on equal counts, else LOSS when
    (black > white) xor (black to move), else WIN."""
    white, black, turn, npass = split(L, key)
    nw, nb = bin(white).count("1"), bin(black).count("1")
    if nw + nb != L * L and npass < 2:
        return UNDECIDED
    if nw == nb:
        return TIE
    return LOSS if (nb > nw) != (turn == 1) else WIN


_RAYS = {}


def rays(L):
    """rays(L)[L * y + x] = ((direction index, squares from the one next to (x, y) outward), ...),
    only the directions with at least two squares: a run and the disc that closes it."""
    if L not in _RAYS:
        out = []
        for j in range(L * L):
            x, y = j % L, j // L
            sq = []
            for d, (dx, dy) in enumerate(DIRS):
                line, cx, cy = [], x + dx, y + dy
                while 0 <= cx < L and 0 <= cy < L:
                    line.append(L * cy + cx)
                    cx, cy = cx + dx, cy + dy
                if len(line) >= 2:
                    sq.append((d, tuple(line)))
            out.append(tuple(sq))
        _RAYS[L] = tuple(out)
    return _RAYS[L]


def expand(L, key):
    """(primitive value, moves): the moves of a non-primitive position in gen_moves order (squares
    x outer, y inner), each (child, (x, y), flip cases); without a legal square the single move is
    the pass, (key + 1, None, ()): the pass byte + 1 and the mover kept.  A flip case is (mover
    colour, x, y, direction index, run length): the mover playing (x, y) turns a run of that many
    opponent discs in that direction, closed by a disc of its own."""
    prim = primitive(L, key)
    if prim != UNDECIDED:
        return prim, []
    A = L * L
    white, black, turn, _ = split(L, key)
    cells = cells_of(L, key)
    me, opp = turn, 3 - turn
    R = rays(L)
    out = []
    for x in range(L):
        for y in range(L):
            j = L * y + x
            if cells[j]:
                continue
            turned, cases = [], []
            for d, line in R[j]:
                n = 0
                for s in line:
                    if cells[s] != opp:
                        break
                    n += 1
                if n and n < len(line) and cells[line[n]] == me:
                    turned.extend(line[:n])
                    cases.append((me, x, y, d, n))
            if not cases:
                continue
            f = sum(1 << (A - 1 - s) for s in turned)
            put = 1 << (A - 1 - j)
            if me == WHITE:
                nw, nb = white | f | put, black & ~f
            else:
                nw, nb = white & ~f, black | f | put
            out.append((join(L, nw, nb, opp, 0), (x, y), tuple(cases)))
    if not out:
        out.append((key + 1, None, ()))
    return prim, out


def feasible(L):
    """Every flip case the board admits: (x, y) + (run + 1) * direction is on the board.  On 8x8 the
    four centre squares are never empty, so they are no move squares."""
    out = set()
    for j, sq in enumerate(rays(L)):
        x, y = j % L, j // L
        if L == 8 and (x, y) in CENTRE8:
            continue
        for d, line in sq:
            for n in range(1, len(line)):
                out.add((BLACK, x, y, d, n))
                out.add((WHITE, x, y, d, n))
    return out


# 2 colours x squares x 8 directions x the runs that fit
assert len(feasible(8)) == 1920 and len(feasible(4)) == 136


class Walk:
    """Every position below a root, with what the sweeps and the coverage conditions read."""

    def __init__(self, L, root):
        self.L, self.root = L, root
        self.kids = {}      # position -> tuple of children in gen_moves order (primitive: ())
        self.prim = {}
        self.cases = set()
        self.squares = set()        # (mover colour, x, y) of every move
        self.most_dirs = 0          # directions one move flips in
        self.passes = 0             # positions whose mover passes and the game goes on
        self.double_pass_ends = 0   # games ended by the second pass with empty squares left
        todo = [root]
        self.prim[root] = None
        while todo:
            k = todo.pop()
            prim, mv = expand(L, k)
            self.prim[k] = prim
            self.kids[k] = tuple(c for c, _, _ in mv)
            if prim != UNDECIDED:
                if k & 0xFF == 2 and empties(L, k):
                    self.double_pass_ends += 1
                continue
            for c, sq, cases in mv:
                if sq is None:
                    self.passes += primitive(L, c) == UNDECIDED
                else:
                    self.cases.update(cases)
                    self.squares.add((cases[0][0],) + sq)
                    self.most_dirs = max(self.most_dirs, len(cases))
                if c not in self.prim:
                    self.prim[c] = None
                    todo.append(c)

    def __len__(self):
        return len(self.kids)


# ---------------------------------------------------------------- the drawn sets
# 8x8 roots as (w0, w1, w2): 1 to 7 empties, at most 3000 positions below each; constructed boards
# (mostly the mover's colour, a few empty squares that each start a closed ray of opponent discs)
# and random ones, about a quarter with pass byte 1
OTH8_ROOTS = (
    (0xDCDC80DD8FFF0101, 0x03227E226000E5FD, 0x0802),
    (0x014801E008080200, 0xFE35FE1FF7F70100, 0x7ECF),
    (0x45CA62BE00180200, 0x3A349D41DFA74863, 0x969C),
    (0x40C00184005A0201, 0xBF1FFC3BEFA580A8, 0x7F57),
    (0xFA7A7A7A7A070101, 0x05858585853883FA, 0x7800),
    (0xBCD7FC36FFCB0100, 0x422803810030EFF3, 0x0008),
    (0x9E7FBCE57FDF0100, 0x618041180000FA18, 0x0466),
    (0x029273B024000200, 0xFD6C8C4D5BF74101, 0xBE96),
    (0xA1818189010E0200, 0x5E7E7E76FEE16000, 0x8F7E),
    (0x76763636344E0100, 0x8989C9C983108F7A, 0x3085),
    (0x380060AC44810100, 0x87BD9F53AB1E8040, 0x3FBF),
    (0x4EB9E01022C40100, 0xA1461FE9DD2B0A1E, 0xA5E1),
    (0x0080808000380200, 0xFF7F7F7F7F873900, 0xC2FF),
    (0x7E7EFEFEFE120100, 0x81010101016481C3, 0x7C1C),
    (0x8D747DDFFCC70100, 0x620982000338775F, 0x0880),
    (0x00113D0442040201, 0xCEEE82FBBDF97E00, 0x80FF),
    (0x9FEDDEFCD3BF0200, 0x201221012C00DB7E, 0x0401),
    (0x5C2C7478FD8F0100, 0x03D38B85023003C4, 0x7C1A),
    (0x0200000000000201, 0xFDFFFFFFFFFF3C00, 0x83FF),
    (0x3C3E3E6F01E10101, 0x42C1C190BE0E8101, 0x1E7E),
    (0xFEFEFAFFFFE30100, 0x01010400000CFFFE, 0x0001),
    (0x8041002120100100, 0x7FBEFFDEDFA92202, 0xCCFD),
    (0x6D5FBF7EFEE60100, 0x92A0400101107743, 0x00AC),
    (0x046C7DECB40F0100, 0x3B9382034870FFFC, 0x0002),
    (0x0182FAFEF1E30100, 0x7E7801010618C7DF, 0x1820),
    (0x030808CA02080200, 0xF8B7F715F9F70405, 0xBBFA),
    (0xB7FDE972FCA70200, 0x4000168103587EAE, 0x8140),
    (0x015D78229C2B0200, 0xFEA287DD61D4229E, 0xDD60),
    (0x8502E80900CA0100, 0x7A7D13B4FE351928, 0xE695),
    (0x24E3AC9AFEF80101, 0xCB18516400077364, 0x8C8B),
    (0x84803E3C000C0201, 0x7B7F0183FFE31880, 0xC777),
    (0x8381CFC12FFF0100, 0x7C7C1036D000BE8D, 0x0062),
    (0xFE7E9BFFCA8F0201, 0x0000640035607CFD, 0x8202),
    (0x0020000800000200, 0xFFDFFFF7FFFF3C01, 0xC1FE),
    (0x0009420025040100, 0x5FF69DFBDAFB0908, 0xF675),
    (0x0000000000000200, 0xFFFFFFFFFFFF0E01, 0xE1FE),
    (0xC93FBEDD6EFD0100, 0x34C0400081027EB7, 0x0148),
    (0xBED6F5DFFBBF0100, 0x41290A000400FFB6, 0x0001),
    (0x87848891813C0200, 0x787A776E5E021800, 0xE3FF),
    (0xE0E1C1C106200200, 0x1E1E1E3E319F00E0, 0xFF1F),
    (0xB79B7FDEEFF70100, 0x080000210008F7BF, 0x0800),
    (0x8022001601000101, 0x7FDDFFE9FEEF00C0, 0xFF2F),
    (0x5707F7F783FF0100, 0x007808087800E703, 0x107C),
    (0xF97A726AFAFE0101, 0x02058D850500C3E1, 0x1C0E),
    (0x0BD683D7BF600101, 0x74297828401E07F5, 0x7802),
    (0x8381D1C1591E0200, 0x7C7E2E3E06817C7D, 0x0280),
    (0x0000100002080100, 0xFFFFEFF7FDF50500, 0xF2FF),
    (0x22260A5C3E830100, 0xDDD9D5A2003CFF1D, 0x00A2),
    (0x74EBFD7F3FF50101, 0x8B140280C00AFEF9, 0x0006),
    (0x04CC386065000101, 0xFB3387979A7B0000, 0xEDFF),
    (0x7E7A776F5FC50101, 0x81818890201A8EFE, 0x6001),
    (0xFF7E7E7E7EF00100, 0x00818181000EC7FF, 0x3000),
    (0x0C524A3434980100, 0xD3A9B1CBCB27BC16, 0x43E9),
    (0xBD910900007E0200, 0x026E76FAFF013041, 0xC7BE),
    (0x5E358A1510030101, 0x218875C26FDCD02A, 0x2FD5),
    (0xC2C2DA425A000200, 0x3D3D21BDA1BD0658, 0xF807),
    (0xA90031FC47210100, 0x56BFCE039856C993, 0x1664),
    (0xFBDF9A33FFD70100, 0x042021440008EFFB, 0x1004),
    (0x3A2E8A8234700200, 0xC1D1556D0B0F0008, 0xFFF5),
    (0x00207E7E00780200, 0xFDDF8001FB07707E, 0x8701),
    (0xFF7F074181030101, 0x0080B83C7C7CE09F, 0x1E40),
    (0x280115AA90AA0100, 0xC3FAE8556F55990A, 0x46F5),
    (0x83D99B7921370201, 0x5C046484DEC0C89E, 0x3161),
    (0x83282B9517C20100, 0x7CD7542AC81D9B22, 0x644D),
    (0xCA3996361D950101, 0x35066989E24A7B48, 0x04B7),
    (0x65143C8308040200, 0x12EB432CF7FBF152, 0x0EAD),
    (0x624383421E240200, 0x9D9C7C9CC1D30020, 0xFF9D),
    (0x4910010301040100, 0x36CFFE9CFEFA0090, 0x3F6F),
    (0x0080000000700200, 0xFF7FFFFFFF873000, 0x8FFF),
    (0x0000000808200100, 0xADFFFED7F7DD0420, 0xFB9F),
    (0xE703CAECFDFE0100, 0x187C14030200BFC3, 0x0034),
    (0x8080830202600200, 0x7F7D7C7CFD8F2600, 0x91FF),
    (0x0000000000300200, 0xFFFFFFFFFF8F1C00, 0xE1FF),
    (0x00335E1D841B0100, 0xFBC821E25BE0AE43, 0x5138),
    (0x10AC101C220B0100, 0x6F536F62DDF41484, 0x637B),
    (0xFCFDFD82FF810100, 0x030202790072C0FC, 0x3E00),
    (0x0880100010000100, 0xC77EAFBFEFFF0180, 0xFA6F),
    (0x2FDF75D7ECD70100, 0xC0208A281220D317, 0x2868),
    (0xD7B1A6AA787B0100, 0x284E595086843A72, 0x4488),
    (0x0082000800400100, 0xEE3DBFF7FFB71044, 0x6F3B),
    (0x00844816038A0100, 0xFD7BB768F4657000, 0x8DFF),
    (0xFFFFFFFFFFF30100, 0x000000000008FDEF, 0x0210),
    (0x080C0C18C2100101, 0xB7F3F3E73DEF1918, 0xE246),
    (0x20E0876D204A0100, 0xD71E7892DFB18584, 0x3A39),
    (0xFEFEFEFFFFC00100, 0x01010100003E80FE, 0x7E00),
    (0x5E947DDFCA7F0200, 0xA06B022010807B4F, 0x00B0),
    (0x93C8F61EB8D10101, 0x6C3209E0472C3379, 0x4886),
    (0x81DF80DEFE800100, 0x3E207D01017CE1DF, 0x1C20),
    (0xA33FFBCB72AA0200, 0x58C0041485440AA2, 0x755C),
    (0x1000000000000200, 0xEFFFFFFFFFFF3800, 0x87FF),
    (0xF4B37F15EB880100, 0x094880C81475577B, 0x8804),
    (0x07217FFD59BA0101, 0xF89E0002A441ABF1, 0x540E),
    (0x8A47AFB0038E0200, 0x75B8104F7C71CFB0, 0x304F),
    (0x0851A0807C1C0200, 0xF72E5E3F81C30C04, 0xE3FB),
    (0x8080800000180200, 0x7F7F7F7FFFC72080, 0xCF7F),
    (0x0001000010780200, 0xFFFEFFFFEF831C00, 0xC3FF),
    (0x0105088004490100, 0xFAFAF67FFBB4A102, 0x5AB9),
    (0x00C20290A3090100, 0xFF3DFD4F4CF60120, 0xFEDF),
    (0x0306040440000200, 0xF8F9F9BBBFFF4E00, 0x30FE),
    (0x480C006081300100, 0xB7F3FF997ECF04F4, 0xFB0B),
    (0x499E2B78A2AB0200, 0xB46194875954BCEE, 0x4311),
    (0x4A7B636341000200, 0xB4809C9C9CFF001A, 0xEFA1),
    (0xDECD69568EFE0200, 0x2132968920017C85, 0x8272),
    (0xFFFFFFBFFEC30101, 0x000000400138FBFF, 0x0400),
    (0x0102000808400200, 0xFEDDFEF1F5B77444, 0x8BBB),
    (0x9F80E3F1F93C0101, 0x607E180E0640C3BF, 0x3840),
    (0xE79E3BFFFFFF0201, 0x100140000000FAAF, 0x0050),
    (0xFFFFFFFFD3FE0101, 0x000000000801FFFD, 0x0000),
    (0x6BB23DC76A1C0100, 0x904CC03895C3B4AB, 0x4A50),
    (0xEEB73B313BF80100, 0x1148C4CE00069EDE, 0x4001),
    (0xE540EE0925DA0200, 0x12BD10B65A25F0B3, 0x0D4C),
    (0xA418106020410200, 0x5BC76F939FBE0003, 0x77FC),
    (0x8E7E3C5A67FF0100, 0x300141A59800F0FF, 0x0E00),
    (0x2AAA38E51F460200, 0xD155C71AE031E730, 0x188D),
    (0x04F8632D439D0200, 0xDB079CD2BC600130, 0xF48B),
    (0x8001808024400100, 0x7FFC5F7FDBBF4100, 0xBEEF),
    (0x8191A1A5897C0200, 0x7E4E5E5A66807C0D, 0x8170),
    (0x41010504680C0201, 0xBEDEF87A97F1600C, 0x1FE3),
    (0x8010941002100200, 0x3FEF69EF7DCF0600, 0xB1FD),
    (0xFAFFEFDBE5770100, 0x050010040088E235, 0x0D82),
)

# named 8x8 roots, added by hand: full boards for either side at every pass byte (a full white-to-move
# board is one bit away from the table's empty mark), roots that start with pass byte 1 or 2, and a
# square that nobody can play
OTH8_EDGE = {
    "full_black_pass0": (0x632472A596570100, 0x9CDB8D5A69A8D24C, 0x2DB3),
    "full_black_pass1": (0xAA55AA55AA550101, 0x55AA55AA55AAAA55, 0x55AA),
    "full_black_pass2": (0x632472A596570102, 0x9CDB8D5A69A8D24C, 0x2DB3),
    "full_white_pass0": (0x632472A596570200, 0x9CDB8D5A69A8D24C, 0x2DB3),
    "full_white_pass1": (0x632472A596570201, 0x9CDB8D5A69A8D24C, 0x2DB3),
    "full_white_pass2": (0xFFFFFFFFFFFF0202, 0x000000000000FFFF, 0x0000),
    "pass2_with_empties": (0xFFE7EFFF3FFE0102, 0x001810004000FF82, 0x007C),
    "pass1_passes_again": (0xFFFFFFFFFF7E0201, 0x000000000000FEFF, 0x0000),
    "pass1_has_a_move": (0xBF5FE7EBFDE10101, 0x40201814020E01FF, 0x7E00),
    "one_empty_unplayable": (0xFFF7EFFFFFFF0200, 0x0008100000007FFF, 0x0000),
}

# 4x4 keys: 1 to 12 empties and arbitrary contents (empty centres, one colour only, boards fixed by
# every non-trivial subgroup of D4), at most 4000 positions below each
OTH4_ROOTS = (
    0x00222E810200, 0x4140AEB70100, 0xEEDF00000100, 0x8A5101800100, 0x61E5160A0200, 0x0408D0C00200,
    0x00029C080100, 0x4A5221840200, 0x2E8310000100, 0x966960060100, 0x418296690200, 0x002AE0C40200,
    0x41020E590100, 0x72DD00020100, 0x205815010100, 0x1BE1A0020100, 0x542A01800100, 0x000033050200,
    0x800074B50201, 0x0200C0430200, 0x4820A7DA0101, 0x5CC020220101, 0x0419B9E40200, 0x00E420180100,
    0x5C1A20A10100, 0x287984000100, 0xD1610A000200, 0x101421280100, 0x209284200200, 0x8510588D0100,
    0x0420CA530200, 0x1E8940600200, 0x412E18910200, 0x561580820100, 0x204095120201, 0x0000A9FD0200,
    0x40763E810100, 0x005000A40200, 0x801855E50100, 0x00008C420200, 0x281496690100, 0x8661581A0200,
    0x04408AA80100, 0x002039400200, 0x281496690200, 0xC00B00000200, 0x6FF600000100, 0xA38000130100,
    0x181604000200, 0x24425AA50200, 0xC00303C00200, 0x916D06800201, 0x066009900200, 0x042092850100,
    0x0E0920500100, 0x080061990100, 0x060C41210200, 0x0A2044080200, 0x0600900F0100, 0x0040A3230101,
    0x552908D40100, 0x8E5D00800200, 0x404026280100, 0x090700E00200, 0xC1002A1D0200, 0x006999900100,
    0x44308A030100, 0xBFF600000200, 0xFD0002940200, 0x144021330200, 0x201004280100, 0x944843120200,
    0x41003EEA0200, 0x561781400201, 0x0000B7050100, 0x0400786B0100, 0x228111280100, 0x041022020200,
    0x2141821C0100, 0x00E86D170201, 0x4A1780400100, 0x6FF600000200, 0x042080410100, 0x966909900200,
    0x601499C80200, 0x0010CC210200, 0x960660600200, 0x82210C880100, 0x299292290200, 0x000CFFB30200,
    0x0000B6AF0100, 0x4304A0C00100, 0x490414080200, 0x010008880200, 0xF99F00000100, 0x020415800100,
)
