"""Plain reference for explicit position graphs (test infrastructure, CPU only).

A graph is the CSR triple gm_solve_graph takes: ``prim[i]`` is node i's primitive() code and
its children are ``kids[off[i]:off[i + 1]]``; node 0 is the root.  Everything here works on
(value, remoteness) pairs and the reduction of ``oracle/canonical.py: fold``; nothing comes
from ``gamesmanmpi_amd`` and no preference score appears.  A primitive node's listed children
are ignored: the reference never expands a primitive position, and neither does the device.
"""
import os
import sys
import types
from collections import deque

import numpy as np

_ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
if _ORACLE not in sys.path:
    sys.path.insert(0, _ORACLE)

from canonical import DRAW, LOSS, TIE, UNDECIDED, WIN, fold  # noqa: E402

MAX_RECORD_REMOTENESS = 0x3FFF   # the 14 remoteness bits of a u16 record


class GraphError(ValueError):
    """The graph has no solution: a DRAW primitive, a bad code, an undecided node without moves."""


class CycleError(GraphError):
    """Some nodes never resolve; ``unresolved`` is how many."""

    def __init__(self, unresolved):
        super().__init__("%d nodes never resolve: the graph has a cycle" % unresolved)
        self.unresolved = unresolved


class RemotenessOverflow(GraphError):
    """A true remoteness does not fit the 14 bits of a record."""


def _arrays(prim, off, kids):
    prim = np.asarray(prim, dtype=np.int64).ravel()
    off = np.asarray(off, dtype=np.int64).ravel()
    kids = np.asarray(kids, dtype=np.int64).ravel()
    n = len(prim)
    if len(off) != n + 1 or np.any(np.diff(off) < 0) or off[-1] > len(kids):
        raise ValueError("off is not a CSR offset array of the graph")
    if len(kids) and (kids.min() < 0 or kids.max() >= n):
        raise ValueError("a child index is out of range")
    return prim, off, kids


def _check_nodes(prim, off):
    """What canonical.solve rejects, node by node."""
    if np.any(prim == DRAW):
        raise GraphError("DRAW primitive is not supported")
    if np.any((prim < 0) | (prim > UNDECIDED)):
        raise GraphError("primitive() code outside 0..4")
    if np.any((prim == UNDECIDED) & (np.diff(off) == 0)):
        raise GraphError("non-primitive position without moves")


def _interior_edges(prim, off, kids):
    """(src, dst) of every edge out of an undecided node, in CSR order (duplicates kept)."""
    n = len(prim)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    dst = kids[off[0]:off[n]]
    keep = prim[src] == UNDECIDED
    return src[keep], dst[keep]


def solve_values(prim, off, kids):
    """(value, remoteness) arrays: fold() applied in reverse topological order (Kahn)."""
    prim, off, kids = _arrays(prim, off, kids)
    _check_nodes(prim, off)
    n = len(prim)
    src, dst = _interior_edges(prim, off, kids)
    order = np.argsort(dst, kind="stable")
    parents = src[order].tolist()                                   # reverse CSR
    poff = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))]).tolist()
    pending = np.bincount(src, minlength=n).tolist()                # unresolved edges per node
    p_l, off_l, kids_l = prim.tolist(), off.tolist(), kids.tolist()
    value = [None] * n
    rem = [0] * n
    queue = deque()
    for i in range(n):
        if p_l[i] != UNDECIDED:
            value[i] = p_l[i]
            queue.append(i)
    while queue:
        c = queue.popleft()
        for p in parents[poff[c]:poff[c + 1]]:
            pending[p] -= 1
            if pending[p] == 0:
                value[p], rem[p] = fold((value[k], rem[k]) for k in kids_l[off_l[p]:off_l[p + 1]])
                queue.append(p)
    unresolved = sum(v is None for v in value)
    if unresolved:
        raise CycleError(unresolved)
    return np.array(value, dtype=np.int64), np.array(rem, dtype=np.int64)


def _layers(prim, off, kids):
    """(value, remoteness, height): one numpy pass per level over the edges still unresolved."""
    prim, off, kids = _arrays(prim, off, kids)
    _check_nodes(prim, off)
    n = len(prim)
    value = np.where(prim == UNDECIDED, -1, prim)
    rem = np.zeros(n, dtype=np.int64)
    src, dst = _interior_edges(prim, off, kids)
    todo = np.flatnonzero(prim == UNDECIDED)
    height = 0
    big = np.int64(1) << 62
    while len(todo):
        # src is sorted and every node of todo has an edge, so its runs start where src changes
        start = np.flatnonzero(np.concatenate([[True], src[1:] != src[:-1]]))
        v, r = value[dst], rem[dst]
        ready = np.minimum.reduceat((v >= 0).astype(np.int8), start).astype(bool)
        if not ready.any():
            raise CycleError(len(todo))
        min_loss = np.minimum.reduceat(np.where(v == LOSS, r, big), start)[ready]
        min_tie = np.minimum.reduceat(np.where(v == TIE, r, big), start)[ready]
        max_win = np.maximum.reduceat(np.where(v == WIN, r, -1), start)[ready]
        node = todo[ready]
        has_loss, has_tie = min_loss < big, min_tie < big
        value[node] = np.where(has_loss, WIN, np.where(has_tie, TIE, LOSS))
        rem[node] = np.where(has_loss, min_loss, np.where(has_tie, min_tie, max_win)) + 1
        height += 1
        keep = ~np.repeat(ready, np.diff(np.concatenate([start, [len(src)]])))
        src, dst, todo = src[keep], dst[keep], todo[~ready]
    return value, rem, height


def pack(value, rem):
    """u16 records ``value << 14 | remoteness``."""
    if len(rem) and rem.max() > MAX_RECORD_REMOTENESS:
        raise RemotenessOverflow("remoteness %d does not fit a record" % rem.max())
    return ((value << 14) | rem).astype(np.uint16)


def solve_reference(prim, off, kids):
    """A u16 record per node."""
    return pack(*solve_values(prim, off, kids))


def solve_reference_layered(prim, off, kids):
    """solve_reference for graphs of millions of nodes (numpy, level by level)."""
    value, rem, _ = _layers(prim, off, kids)
    return pack(value, rem)


def height(prim, off, kids):
    """Levels of the graph above its primitives: the rounds a level-synchronous solve takes."""
    return _layers(prim, off, kids)[2]


def reachable(prim, off, kids):
    """Sorted indices of the nodes reachable from node 0 (primitives are not expanded)."""
    prim, off, kids = _arrays(prim, off, kids)
    seen = np.zeros(len(prim), dtype=bool)
    seen[0] = True
    stack = [0]
    while stack:
        i = stack.pop()
        if prim[i] != UNDECIDED:
            continue
        for k in kids[off[i]:off[i + 1]].tolist():
            if not seen[k]:
                seen[k] = True
                stack.append(k)
    return np.flatnonzero(seen)


def as_plugin(prim, off, kids):
    """The graph as a plugin module: positions are node indices, a move is a child's place."""
    prim, off, kids = _arrays(prim, off, kids)
    p_l, off_l, kids_l = prim.tolist(), off.tolist(), kids.tolist()
    mod = types.SimpleNamespace()
    mod.initial_position = lambda: 0
    mod.gen_moves = lambda pos: list(range(off_l[pos + 1] - off_l[pos]))
    mod.do_move = lambda pos, move: kids_l[off_l[pos] + move]
    mod.primitive = lambda pos: p_l[pos]
    return mod


# ---------------------------------------------------------------- generators
def _csr(prim, lists):
    off = np.zeros(len(prim) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    kids = np.array([k for x in lists for k in x], dtype=np.uint32)
    return np.asarray(prim, dtype=np.uint8), off, kids


def random_dag(n, levels, max_deg, skip, mix, seed):
    """n nodes in `levels` levels, node 0 alone on top; a node of the last level is a leaf with a
    value drawn from `mix` (weights of WIN, LOSS, TIE), every other node has 1..max_deg children:
    its first in the next level, so the levels are the graph's height, the others in the next
    level or, with `skip`, in any deeper one, so that they resolve in different rounds.
    Duplicate children are allowed.  A level's nodes are spread over the index range: the level
    of node i > 0 is 1 + (i - 1) % (levels - 1)."""
    rng = np.random.default_rng(seed)
    levels = max(2, min(levels, n))
    idx = np.arange(n, dtype=np.int64)
    level = np.where(idx == 0, 0, 1 + (idx - 1) % (levels - 1))
    members = [np.flatnonzero(level == lv) for lv in range(levels)]
    below = np.concatenate([[0], np.cumsum([len(m) for m in members])])   # by level, then index
    by_level = np.concatenate(members)
    mix = np.asarray(mix, dtype=np.float64)
    prim = np.full(n, UNDECIDED, dtype=np.uint8)
    last = members[levels - 1]
    prim[last] = rng.choice([WIN, LOSS, TIE], size=len(last), p=mix / mix.sum())
    deg = np.where(level < levels - 1, rng.integers(1, max_deg + 1, size=n), 0)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(deg)
    src = np.repeat(idx, deg)
    first = np.concatenate([[True], src[1:] != src[:-1]]) if len(src) else np.zeros(0, dtype=bool)
    lo = below[level[src] + 1]
    hi = np.where(first | (not skip), below[level[src] + 2], n)
    kids = by_level[lo + (rng.random(len(src)) * (hi - lo)).astype(np.int64)]
    return prim, off, kids.astype(np.uint32)


def chain(n, leaf_value):
    """0 -> 1 -> ... -> n - 1, the last a primitive of `leaf_value`."""
    prim = np.full(n, UNDECIDED, dtype=np.uint8)
    prim[n - 1] = leaf_value
    off = np.minimum(np.arange(n + 1, dtype=np.uint64), np.uint64(n - 1))
    return prim, off, np.arange(1, n, dtype=np.uint32)


def star(n_children, seed=0, distinct=64):
    """A root with n_children children drawn, with heavy duplication, from `distinct` nodes:
    WIN, LOSS and TIE primitives and short chains down to each, so the root's choice is between
    classes and between remotenesses."""
    rng = np.random.default_rng(seed)
    prim, lists = [UNDECIDED], [[]]
    tops = []
    for j in range(distinct):
        top = len(prim)
        depth = int(rng.integers(0, 4))
        for d in range(depth):
            prim.append(UNDECIDED)
            lists.append([len(prim)])
        prim.append((WIN, LOSS, TIE)[j % 3])
        lists.append([])
        tops.append(top)
    lists[0] = rng.choice(tops, size=n_children).tolist()
    return _csr(prim, lists)


def hang_under_chain(graph, length):
    """`graph` with a chain of `length` nodes above its root; the chain's top is the new node 0."""
    prim, off, kids = graph
    n, m = len(prim), len(kids)
    prim2 = np.concatenate([np.full(length, UNDECIDED, dtype=np.uint8), prim])
    off2 = np.concatenate([np.arange(length, dtype=np.uint64), np.asarray(off, dtype=np.uint64) + np.uint64(length)])
    kids2 = np.concatenate([np.arange(1, length + 1, dtype=np.uint32), np.asarray(kids, dtype=np.uint32) + np.uint32(length)])
    assert len(prim2) == n + length and len(kids2) == m + length
    return prim2, off2, kids2
