"""Custom roots of the SUBTRACT game for the sweeps of tests/test_gpu_sub_sweep.py, as literals: a
drawn set that a change of a generator cannot move.  tests/test_sub_roots.py holds the coverage
conditions the sets were drawn to meet and solves every root once with the C oracle.

A key's nibble i is heap i.  The box engines (csrc/box_common.hpp) cut heaps 0-3 (A) in quarters
and heaps 4-7 (B) in halves, so a root's region is a brick of boxes whose top box has the
coordinates box_limits(root); its box-tiers are the sums of box coordinates, 0 .. sum(limits).
"""


def digits(root, heaps=8):
    return [(root >> (4 * i)) & 15 for i in range(heaps)]


def positions(root, heaps=8):
    """Positions of a solve from `root`: every key whose nibbles are all <= the root's."""
    n = 1
    for d in digits(root, heaps):
        n *= d + 1
    return n


def box_limits(root):
    """Box coordinates of the root's top box: heaps 0-3 in quarters, heaps 4-7 in halves."""
    d = digits(root)
    return tuple(x >> 2 for x in d[:4]) + tuple(x >> 1 for x in d[4:])


def box_tiers(root):
    d = digits(root)
    return 1 + sum(x >> 2 for x in d[:4]) + sum(x >> 1 for x in d[4:])


def n_boxes(root):
    n = 1
    for c in box_limits(root):
        n *= c + 1
    return n


def outside_keys(root, heaps=8):
    """Three keys no solve from `root` holds: one nibble above the root's (the lowest heap that
    is not full; the nibble above the table when all are), one bit past the widest table and the
    largest key."""
    i = ([d < 15 for d in digits(root, heaps)] + [True]).index(True)
    return [root + (1 << (4 * i)), 1 << 32, 2 ** 64 - 1]


# Eight heaps, at most 300,000 positions, at least two boxes.  Every sixth or so is hand-picked:
# the deep ones (28 box-tiers and more: B heaps of 14 or 15 with next to nothing in the A heaps),
# 0xCECE0000 / 0xCECE0004 (27 and 28 box-tiers: the last root without and the first with a tail
# launch of the default hybrid range), 0x66660333 / 0x66664000 / 0x66664004 (13, 14, 15: the last
# with every tier in the head launch, the first with a tier launch) and four regions of a few
# positions.  The others were drawn over the sixteen combinations of how the box limits of heaps
# 4/5 and of heaps 6/7 compare (lower < upper, >, equal, both zero), half of each with at most
# 14 box-tiers.
ROOTS8 = (
    0x72856020, 0x0DE87000, 0x22750000, 0x00C75909, 0x201D5000, 0xEEEE0000, 0x3F3D5000, 0x224D0001,
    0x00AF00F0, 0x80762F00, 0x3DAAF000, 0xFFFF0003, 0x4555B000, 0x10DCD0D0, 0x86110B00, 0xCE00A000,
    0x4511E10E, 0xEFEF0040, 0x01117000, 0xC090040A, 0x02C5C0A2, 0x77843000, 0x00EB00D8, 0xFEFE4000,
    0x8703E013, 0x1F2A03B0, 0x330F5441, 0x115F0C46, 0xF233020D, 0xFFEE0300, 0x4B89F000, 0x89323F00,
    0x01BA0F0B, 0xB4110C1D, 0xCF010D0B, 0xEEEE0004, 0x541100DF, 0x101001B3, 0xB0C00000, 0x8BE00004,
    0x32C64000, 0xFFFF3000, 0x10A7808A, 0x501C2000, 0x1D8B0008, 0x44788000, 0x109F0C30, 0xEEEE0110,
    0x83335074, 0x3FBA0000, 0xBB230000, 0x10EFB000, 0x60010005, 0xCEEE0400, 0x5D01F0F5, 0xCD100000,
    0x100110FB, 0x60865920, 0x8F730090, 0xECEE0040, 0x54705B00, 0x11FAB00B, 0x710AB000, 0xCF240000,
    0x33280087, 0xEECE0004, 0x01BFF200, 0xB9230000, 0x4CFF1300, 0x7655E003, 0x01FE0038, 0xEEEC4000,
    0x75110430, 0xDF100268, 0x44118B40, 0x01118590, 0x61431BE0, 0xCECE0004, 0x8BF60060, 0x66813000,
    0x11E700F6, 0xA5159802, 0xAE2400A0, 0xDFCE0200, 0x335D0D20, 0x01CF0D00, 0x815403A3, 0x09DC7009,
    0x3233001B, 0xCECE0000, 0x11EFC050, 0xD9110000, 0x8A01CF00, 0x33004C70, 0x01100400, 0x66660333,
    0x504210AF, 0x78E50070, 0x44730000, 0x01C4EE00, 0x82164003, 0x66664000, 0x1A9B0F00, 0x23290B30,
    0x01BE000E, 0x72440E00, 0xCE770000, 0x66664004, 0x55540E00, 0x10DDB009, 0xD5116E00, 0xAF01D003,
    0x6710000D, 0x000000F0, 0x01016AA9, 0xC0E01000, 0x6EFA0004, 0x55743205, 0x10CBC000, 0x00020000,
    0x91561007, 0x5D0C0000, 0x98362200, 0x00BC0D01, 0x50770040, 0x20000000, 0x0E980001, 0x33230B00,
    0x01DD0F00, 0x210000C2, 0xAC11E000, 0x00000004, 0x67010882, 0x00010955, 0x63F10030, 0x0EA62C00,
    0x2362070C, 0x00F508E0, 0x713A1006, 0x473C900A, 0x3313011E, 0x018B088A, 0xE4224030, 0x26FE0007,
    0x98234040, 0x11FF0A00, 0x73100B05, 0xAF1000CE, 0x88010350, 0x10002E90,
)

# (r, r'): the same box limits, so the same top box: the second solve of a context keeps the
# lists, flags, epochs and the captured graph of the first
PAIRS8 = (
    (0x72856020, 0x62844002),
    (0x80762F00, 0x80760D22),
    (0x01117000, 0x00115032),
    (0x115F0C46, 0x015E1F75),
    (0x541100DF, 0x550121DF),
    (0x44788000, 0x44689200),
    (0x5D01F0F5, 0x5D01D0C5),
    (0xCF240000, 0xDF350223),
    (0x75110430, 0x64100720),
    (0xA5159802, 0xB5158B10),
    (0x11EFC050, 0x11EEE170),
    (0x01C4EE00, 0x11C5DF10),
    (0x55540E00, 0x44541F30),
    (0x55743205, 0x45750114),
    (0x0E980001, 0x1F881102),
    (0x0EA62C00, 0x1FA70D10),
    (0x98234040, 0x98225162),
    (0xEEEE0000, 0xFEFE1100),
    (0xFEFE4000, 0xEEFE4000),
)

# The block engine's heap counts below 8: every nibble takes 0, 15 and a value between; the first
# three of each have every nibble from the fourth on 0 (one block at three low heaps, one launch)
ROOTS_H = {
    3: (
        0x5DD, 0x0FF, 0x077, 0x400, 0xDF9, 0x20F, 0xFF2, 0x6A0,
        0xEF9, 0xFB0, 0x3FA, 0x2FF, 0xFED, 0x010, 0xB5A, 0xF9F,
    ),
    4: (
        0x0F0F, 0x00FF, 0x0F99, 0x0776, 0xF0FF, 0xA00B, 0xFF80, 0xFF0B,
        0x20DD, 0x4B60, 0xF140, 0x020A, 0x0CDB, 0x0FBC, 0x936C, 0xF03B,
    ),
    5: (
        0x0071F, 0x006F0, 0x00CFF, 0x00F10, 0xFD40B, 0xF030C, 0xF0F8F, 0x201E7,
        0x40EDB, 0x4600F, 0xFBFF0, 0xEF0E2, 0xF7935, 0x2BF0F, 0xFF4F0, 0x0099F,
    ),
    6: (
        0x0000C3, 0x000B53, 0x000900, 0xBF020D, 0x0F0509, 0x303DF4, 0xA0A0CE, 0x2C07EF,
        0xF70306, 0x00D5F0, 0x000977, 0x2FF20F, 0x93F0B9, 0x00F00F, 0xB0FE20, 0xA70F85,
    ),
    7: (
        0x0000976, 0x0000FF0, 0x000025F, 0xF109F10, 0xB2F0F17, 0x0FFF008, 0x200500D, 0xFF9F002,
        0x3BC0F00, 0x0A0F97F, 0x7FF0562, 0x1F0140F, 0x0E48F0F, 0x0AF0640, 0xC22FF20, 0x0F0FA8A,
    ),
}


def every(k):
    """Every k-th root of ROOTS8, and every root with 28 box-tiers or more."""
    return tuple(r for i, r in enumerate(ROOTS8) if i % k == 0 or box_tiers(r) >= 28)


def split_axes(root):
    """Heaps along which the root's region has more than one box: the split box engine
    (csrc/dist_box.hip bx_shape) cuts along up to three of them, one per factor 2 of the rank
    count, and with fewer the ranks of the missing axes hold nothing."""
    return sum(c > 0 for c in box_limits(root))


IDLE8 = tuple(r for r in ROOTS8 if split_axes(r) < 3)
