"""Positions reachable under a move policy (gm_reach, include/gmsolve.h): the host side.

``Context.reach(starts, mover, other)`` asks the device; this module holds what surrounds it:

* ``POLICIES`` / ``policy(name)``: the policy names ``"all"``, ``"best"``, ``"first"``;
* ``reference(starts, table, expand, mover, other, max_plies)``: gm_reach on the host, a plain
  breadth-first search over a ``{key: record}`` dict and an ``expand`` callable, optionally
  closed under a list of symmetry maps -- what the tests compare the device against (Solver
  never calls it);
* ``is_closed(marks, table, expand, mover, other)``: whether a set of (position, side) pairs
  is closed under the policies;
* ``format_strategy``: the lines ``--strategy`` prints.

The side of a reached position is the parity of the ply at which it is reached: side bit 0 is
an even ply (the starts' mover to move), bit 1 an odd one.

The reference has no such route: it reopens the ``resolved`` shelves and walks the plugin ply
by ply (src/cache_dict.py:38-79, src/game_state.py:33-41).
"""
from . import _lib
from .solver import move_rank

UNDECIDED = 4
POLICIES = {"all": _lib.REACH_ALL, "best": _lib.REACH_BEST, "first": _lib.REACH_FIRST}


def policy(p):
    """A policy name or _lib.REACH_* code -> the code."""
    if isinstance(p, str):
        if p not in POLICIES:
            raise ValueError("unknown policy %r (one of %s)" % (p, ", ".join(sorted(POLICIES))))
        return POLICIES[p]
    p = int(p)
    if p not in POLICIES.values():
        raise ValueError("unknown policy %r" % p)
    return p


def selected(kids, recs, pol):
    """The children a side with policy `pol` follows among `kids` with u16 records `recs`:
    every child, every child of maximal move_rank, or the first of those."""
    if pol == _lib.REACH_ALL or not kids:
        return list(kids)
    ranks = [move_rank(r) for r in recs]
    top = max(ranks)
    best = [k for k, r in zip(kids, ranks) if r == top]
    return best if pol == _lib.REACH_BEST else best[:1]


def _getter(table):
    return (lambda k: table.get(k, _lib.REC_UNSOLVED)) if isinstance(table, dict) else table


def reference(starts, table, expand, mover="all", other="all", max_plies=0, symmetries=None, memo=None):
    """gm_reach on the host.  `table` is a {key: u16 record} dict (or a callable, 0xFFFF: none),
    `expand(key)` returns (primitive code, children in gen_moves order, tier) as Context.expand
    does.  `symmetries`: the maps (key -> key) of the whole symmetry group of a reduced table;
    a pair is then marked together with all its images, counted once each, and one member of
    the orbit is expanded -- what the device computes on one representative per orbit.
    `memo`: a dict the caller keeps between calls over the same table and expand; it holds what
    each policy selects at a position, so that a second policy pair does not rank again.
    Returns (out dict as Context.reach's, ply_counts list, marks {key: side bits})."""
    get = _getter(table)
    pol = (policy(mover), policy(other))
    syms = list(symmetries or [])
    marks, frontier, ply_counts = {}, [], []
    out = dict(n=0, n_mover=0, n_other=0, n_starts=0, edges=0, missing=0, plies=0)
    level = [0]

    def mark(k, side):
        bit = 1 << side
        if marks.get(k, 0) & bit:
            return
        frontier.append(k)
        for m in {k} | {int(s(k)) for s in syms}:
            if not marks.get(m, 0) & bit:
                marks[m] = marks.get(m, 0) | bit
                level[0] += 1

    for k in starts:
        k = int(k)
        if get(k) != _lib.REC_UNSOLVED:
            out["n_starts"] += 1
            mark(k, 0)
    ply = 0
    while frontier:
        ply_counts.append(level[0])
        level[0] = 0
        cur, frontier[:] = list(frontier), []
        if max_plies and ply >= max_plies:
            break
        for k in cur:
            chosen = None if memo is None else memo.get((k, pol[ply & 1]))
            if chosen is None:
                prim, kids, _ = expand(k)
                kids = [int(c) for c in kids] if prim == UNDECIDED else []
                chosen = selected(kids, [get(c) for c in kids], pol[ply & 1])
                if memo is not None:
                    memo[k, pol[ply & 1]] = chosen
            for c in chosen:
                out["edges"] += 1
                if get(c) == _lib.REC_UNSOLVED:
                    out["missing"] += 1
                else:
                    mark(c, (ply + 1) & 1)
        ply += 1
    out["n"] = len(marks)
    out["n_mover"] = sum(ply_counts[0::2])
    out["n_other"] = sum(ply_counts[1::2])
    out["plies"] = len(ply_counts)
    return out, ply_counts, marks


def is_closed(marks, table, expand, mover="all", other="all", starts=()):
    """Whether `marks` ({key: side bits}) holds the starts at side 0 and, for every pair in
    it whose position has a record and is not primitive, every child its side's policy selects
    (and that has a record) at the other side."""
    get = _getter(table)
    pol = (policy(mover), policy(other))
    for k in starts:
        if get(int(k)) != _lib.REC_UNSOLVED and not marks.get(int(k), 0) & 1:
            return False
    for k, bits in marks.items():
        if get(k) == _lib.REC_UNSOLVED:
            return False
        prim, kids, _ = expand(k)
        if prim != UNDECIDED:
            continue
        kids = [int(c) for c in kids]
        recs = [get(c) for c in kids]
        for side in (0, 1):
            if not bits >> side & 1:
                continue
            for c in selected(kids, recs, pol[side]):
                if get(c) != _lib.REC_UNSOLVED and not marks.get(c, 0) >> (side ^ 1) & 1:
                    return False
    return True


def format_strategy(side, root_text, out, total, ply_counts):
    """The lines of ``--strategy``: one naming the side, the root value, the reached positions
    of the total as a share and the deepest ply, then the per-ply counts."""
    share = 100.0 * out["n"] / total if total else 0.0
    lines = ["Strategy for the %s (root %s): %d of %d positions (%.2f%%), deepest ply %d"
             % (side, root_text, out["n"], total, share, out["plies"] - 1)]
    lines += ["  ply %d: %d" % (d, int(c)) for d, c in enumerate(ply_counts)]
    return lines
