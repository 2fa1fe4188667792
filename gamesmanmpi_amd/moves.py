"""Every move of a batch of positions, valued (gm_moves, include/gmsolve.h): the host side.

``Context.moves_batch(keys)`` asks the device; this module holds what surrounds that call:

* ``rank(records)``: ``solver.move_rank`` over a u16 array -- the mover prefers the child of the
  largest rank: LOSS (shortest) > TIE (shortest) > DRAW > WIN (longest) > not stored;
* ``optimal_mask(heads, child_records)``: per child, whether it is one of its parent's optimal
  moves (its rank equals the best child's);
* ``reference(keys, lookup, expand)``: the answer of gm_moves computed on the host from a
  (key -> record) table and an expand function -- what the CPU tests and a table loaded
  without a device compare against;
* ``format_rows``: the ``Moves:`` lines of the command lines.

The reference offers no batch route: it reopens the ``resolved`` shelves and calls the
plugin's gen_moves / do_move per position (src/cache_dict.py:38-79, src/game_state.py:33-41).
"""
import numpy as np

from . import _lib

UNDECIDED = 4


def rank(records):
    """move_rank of solver.py, element by element over u16 records (a uint32 array)."""
    rec = np.asarray(records, dtype=np.uint16).astype(np.uint32)
    val, rem = rec >> 14, rec & 0x3FFF
    score = np.where(val == 0, 0x4000 | rem, np.where(val == 2, 0x8000 | (0x3FFF - rem), 0xC000 | (0x3FFF - rem)))
    out = (2 * score).astype(np.uint32)
    out[rec == _lib.REC_UNSOLVED] = 0
    out[rec == _lib.REC_DRAW] = 0xFFFF
    return out


def segments(heads):
    """For every child of `heads` (in child-array order) the index of its parent key."""
    return np.repeat(np.arange(len(heads)), np.asarray(heads["count"], dtype=np.int64))


def optimal_mask(heads, child_records):
    """Boolean per child: its rank equals that of its parent's best child (heads.best)."""
    heads = np.asarray(heads)
    r = rank(child_records)
    if not len(r):
        return np.zeros(0, dtype=bool)
    seg = segments(heads)
    has = heads["count"] > 0
    best_rank = np.zeros(len(heads), dtype=np.uint32)
    at = (heads["first"][has].astype(np.int64) + heads["best"][has].astype(np.int64))
    best_rank[has] = r[at]
    return r == best_rank[seg]


def best_of(child_records, counts):
    """(best, n_best) per segment of `child_records` cut by `counts`: the first child of maximal
    rank (-1 without children) and the number of children of that rank."""
    r = rank(child_records).astype(np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    best = np.full(len(counts), -1, dtype=np.int16)
    n_best = np.zeros(len(counts), dtype=np.uint16)
    if not len(r):
        return best, n_best
    first = np.concatenate(([0], np.cumsum(counts)[:-1]))
    has = counts > 0
    top = np.zeros(len(counts), dtype=np.int64)
    top[has] = np.maximum.reduceat(r, first[has])
    seg = np.repeat(np.arange(len(counts)), counts)
    is_top = r == top[seg]
    n_best[:] = np.bincount(seg[is_top], minlength=len(counts))
    # the first of equals: the smallest in-segment index among the top children
    idx = np.arange(len(r)) - first[seg]
    lowest = np.full(len(counts), np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(lowest, seg[is_top], idx[is_top])
    best[has] = lowest[has]
    return best, n_best


def reference(keys, lookup, expand):
    """gm_moves on the host.  `lookup(key)` is the key's u16 record (0xFFFF: none) or a dict of
    them; `expand(key)` returns (primitive code, children in gen_moves order, tier), as
    Context.expand does.  Returns (heads, child_keys as a list of Python ints, child_records)."""
    get = (lambda k: lookup.get(k, _lib.REC_UNSOLVED)) if isinstance(lookup, dict) else lookup
    heads = np.zeros(len(keys), dtype=_lib.moves_dtype())
    child_keys, child_recs, counts = [], [], []
    for i, k in enumerate(keys):
        k = int(k)
        rec = int(get(k))
        kids = []
        if rec != _lib.REC_UNSOLVED:
            prim, kids, _ = expand(k)
            if prim != UNDECIDED:
                kids = []
        heads[i]["record"] = rec
        counts.append(len(kids))
        child_keys.extend(int(c) for c in kids)
        child_recs.extend(int(get(int(c))) for c in kids)
    child_recs = np.array(child_recs, dtype=np.uint16)
    counts = np.array(counts, dtype=np.int64)
    heads["count"] = counts
    heads["first"] = np.concatenate(([0], np.cumsum(counts)[:-1])) if len(counts) else 0
    heads["best"], heads["n_best"] = best_of(child_recs, counts)
    return heads, child_keys, child_recs


def record_of(value, remoteness):
    """The u16 record of a (value, remoteness) pair as split_record gives it."""
    return _lib.REC_UNSOLVED if value is None else (int(value) << 14) | int(remoteness)


def format_rows(rows, indent="  "):
    """One line per row (move, child position, value, remoteness) of Solver.moves /
    Solver.annotate: ``<move> -> <child position>: <VALUE> in <R>``, a trailing `` *`` on every
    optimal move."""
    from .verify import _record_text
    if not rows:
        return []
    r = rank([record_of(v, rem) for _, _, v, rem in rows])
    top = r.max()
    return ["%s%r -> %r: %s%s" % (indent, m, p, _record_text(v, rem), " *" if x == top else "")
            for (m, p, v, rem), x in zip(rows, r)]


def format_block(rows, title="Moves:"):
    return [title] + format_rows(rows)
