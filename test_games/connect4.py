"""Connect Four and its relatives: ``connect`` in a row on ``length`` columns of ``height`` rows.

Not part of the reference; written for this project as one of the plugins its README invites
(``gen_moves / do_move / primitive``).  A move names a column that is not full and the disc
falls to the lowest empty cell.  The first player moves when the number of discs on the board
is even.  A position is a LOSS for the player to move when the stones of the player who is NOT
to move hold ``connect`` in a row -- horizontal, vertical or along either diagonal -- a TIE when
the board is full without one, and UNDECIDED otherwise.  Only the stones of the player not to
move are looked at, so a custom root with an odd history means the same thing everywhere.

A position is one int.  Column ``x`` owns bits ``[x * (height + 1), (x + 1) * (height + 1))``;
a column of ``h`` discs holds ``2**h + s``, where bit ``y`` of ``s`` is set iff the disc in
row ``y`` (0 = bottom) is the first player's: the stones below a single cap bit.  The empty
board is one set bit per column, and a move in column ``x`` adds the column's cap when the
second player moves and twice the cap when the first player moves.

``length``, ``height`` and ``connect`` are read at call time, so tests and the launchers'
``--dims`` / ``--connect`` may patch them.
"""
import src.utils as U

length = 5
height = 4
connect = 4


def initial_position():
    return sum(1 << (x * (height + 1)) for x in range(length))


def _caps(pos):
    """The cap bit of every column, in place (a column field of 0 is no position)."""
    width = height + 1
    caps = []
    for x in range(length):
        field = (pos >> (x * width)) & ((1 << width) - 1)
        if not field:
            raise ValueError("column %d has no cap bit" % x)
        caps.append(1 << (field.bit_length() - 1 + x * width))
    return caps


def _discs(pos, caps):
    return sum(cap.bit_length() - 1 - x * (height + 1) for x, cap in enumerate(caps))


def gen_moves(pos):
    width = height + 1
    return [x for x, cap in enumerate(_caps(pos)) if cap >> (x * width + height) == 0]


def do_move(pos, move):
    caps = _caps(pos)
    first = _discs(pos, caps) % 2 == 0
    return pos + (2 * caps[move] if first else caps[move])


def primitive(pos):
    caps = _caps(pos)
    discs = _discs(pos, caps)
    width = height + 1
    below = sum(cap - (1 << (x * width)) for x, cap in enumerate(caps))   # every cell under a cap
    stones = pos & below if discs % 2 else below & ~pos   # of the player who just moved
    # the cell above a column's top row is never a stone, so a run of shifts cannot leave the board
    for step in (1, width, width - 1, width + 1):
        run = stones
        for _ in range(connect - 1):
            run &= run >> step
        if run:
            return U.LOSS
    return U.TIE if discs == length * height else U.UNDECIDED
