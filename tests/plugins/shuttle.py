"""Shuttle: a small game in which positions repeat (no device descriptor; needs a loopy solve).

Two counters (a, b) run from 0 to GOAL.  A move advances one counter by 1 or 2, never past
GOAL; a counter standing on RETREAT may instead be pulled back by one.  Both counters on GOAL:
the player to move has lost.  Pulling back makes positions repeat ((3, b) -> (2, b) -> (3, b)),
so the reference never finishes on it and the default graph solve refuses it; solved loopy,
the start (0, 0) is a DRAW -- both of its advances by one hand the opponent a WIN, both by two
keep the draw -- and (0, 1) is a WIN in 9.  64 positions, 19 of them drawn.
"""
from src.utils import LOSS, UNDECIDED

GOAL = 7
RETREAT = 3
START = (0, 0)


def initial_position():
    return START


def gen_moves(pos):
    moves = [(i, d) for d in (1, 2) for i in (0, 1) if pos[i] + d <= GOAL]
    return moves + [(i, -1) for i in (0, 1) if pos[i] == RETREAT]


def do_move(pos, move):
    i, d = move
    out = list(pos)
    out[i] += d
    return tuple(out)


def primitive(pos):
    return LOSS if pos == (GOAL, GOAL) else UNDECIDED
