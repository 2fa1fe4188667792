"""Plain reference for the loopy solve of explicit position graphs (test infrastructure, CPU).

The graph is the CSR triple of tests/graph_ref.py; cycles and DRAW primitives are allowed.
``solve_loopy`` is the definition by levels, written pull-style: per level it scans the nodes
still undecided and looks at their children -- no reverse graph, no counters, no frontier,
on purpose unlike csrc/graph_loopy.hip.  ``check_rules`` is the local rule a loopy table must
satisfy (and that suffices: include/gmsolve.h gm_verify).  Nothing here comes from
``gamesmanmpi_amd`` and no preference score appears.
"""
import numpy as np

import graph_ref
from graph_ref import DRAW, LOSS, TIE, UNDECIDED, WIN, GraphError

REC_DRAW = DRAW << 14
REC_NONE = 0xFFFF


def _check_nodes(prim, off):
    if np.any((prim < 0) | (prim > UNDECIDED)):
        raise GraphError("primitive() code outside 0..4")
    if np.any((prim == UNDECIDED) & (np.diff(off) == 0)):
        raise GraphError("non-primitive position without moves")


def _runs(src):
    """Start of every run of equal values in the sorted array src."""
    return np.flatnonzero(np.concatenate([[True], src[1:] != src[:-1]]))


def solve_levels(prim, off, kids):
    """(value, remoteness, levels): the least fixed point by levels; `levels` counts the levels
    of both phases that decided a node."""
    prim, off, kids = graph_ref._arrays(prim, off, kids)
    _check_nodes(prim, off)
    n = len(prim)
    value = np.where(prim == UNDECIDED, -1, prim)
    rem = np.zeros(n, dtype=np.int64)
    src, dst = graph_ref._interior_edges(prim, off, kids)
    levels = 0
    for phase in ("winloss", "tie"):
        k = 1
        while len(src):
            keep = value[src] < 0              # the edges of the nodes still undecided
            src, dst = src[keep], dst[keep]
            if not len(src):
                break
            start = _runs(src)
            node = src[start]
            v, r = value[dst], rem[dst]
            if phase == "winloss":
                # WIN in k: a LOSS child of remoteness k - 1
                win = np.maximum.reduceat(((v == LOSS) & (r == k - 1)).astype(np.int8), start).astype(bool)
                # LOSS in k: every child WIN, the largest remoteness k - 1
                all_win = np.minimum.reduceat((v == WIN).astype(np.int8), start).astype(bool)
                longest = np.maximum.reduceat(np.where(v == WIN, r, -1), start)
                loss = ~win & all_win & (longest == k - 1)
                if not (win.any() or loss.any()):
                    break
                value[node[win]], value[node[loss]] = WIN, LOSS
                rem[node[win | loss]] = k
            else:
                tie = np.maximum.reduceat(((v == TIE) & (r == k - 1)).astype(np.int8), start).astype(bool)
                if not tie.any():
                    break
                value[node[tie]] = TIE
                rem[node[tie]] = k
            levels += 1
            k += 1
        src, dst = graph_ref._interior_edges(prim, off, kids)
    value[value < 0] = DRAW
    return value, rem, levels


def solve_loopy(prim, off, kids):
    """A u16 record per node; (DRAW, 0) is 0xC000."""
    value, rem, _ = solve_levels(prim, off, kids)
    return graph_ref.pack(value, rem)


def check_rules(prim, off, kids, recs):
    """The offenders of the local rule, sorted: (node, class) with class one of "bad_primitive",
    "missing_child" (a child with record 0xFFFF), "bad_value".  A primitive carries (value, 0);
    an interior node the reduction of its children under LOSS (shortest) > TIE (shortest) > DRAW
    > WIN (longest), a best child DRAW making the parent DRAW."""
    prim, off, kids = graph_ref._arrays(prim, off, kids)
    recs = np.asarray(recs, dtype=np.int64)
    bad = []
    for i in np.flatnonzero((prim != UNDECIDED) & (recs != (prim << 14))).tolist():
        bad.append((i, "bad_primitive"))
    src, dst = graph_ref._interior_edges(prim, off, kids)
    if len(src):
        start = _runs(src)
        node = src[start]
        rc = recs[dst]
        v, r = rc >> 14, rc & 0x3FFF
        present = rc != REC_NONE
        big = np.int64(1) << 40
        missing = ~np.minimum.reduceat(present.astype(np.int8), start).astype(bool)
        min_loss = np.minimum.reduceat(np.where(present & (v == LOSS), r, big), start)
        min_tie = np.minimum.reduceat(np.where(present & (v == TIE), r, big), start)
        any_draw = np.maximum.reduceat((present & (v == DRAW)).astype(np.int8), start).astype(bool)
        max_win = np.maximum.reduceat(np.where(present & (v == WIN), r, -1), start)
        want = np.where(min_loss < big, (WIN << 14) | (min_loss + 1),
                        np.where(min_tie < big, (TIE << 14) | (min_tie + 1),
                                 np.where(any_draw, REC_DRAW, (LOSS << 14) | (max_win + 1))))
        for i in node[missing].tolist():
            bad.append((i, "missing_child"))
        for i in node[~missing & (recs[node] != want)].tolist():
            bad.append((i, "bad_value"))
    return sorted(bad)


# ---------------------------------------------------------------- generators
def rewire(graph, frac, seed, draw_leaves=False):
    """`graph` (a graph_ref.random_dag) with a fraction `frac` of its edges redirected to
    uniformly random nodes -- up as well as down, so cycles appear -- and, with draw_leaves,
    a quarter of its leaves turned into DRAW primitives."""
    prim, off, kids = (np.array(a) for a in graph)
    rng = np.random.default_rng(seed)
    n = len(prim)
    hit = rng.random(len(kids)) < frac
    kids[hit] = rng.integers(0, n, size=int(hit.sum()))
    if draw_leaves:
        leaves = np.flatnonzero(prim != UNDECIDED)
        prim[leaves[rng.random(len(leaves)) < 0.25]] = DRAW
    return prim, off, kids


def ring(n, leaf_every=0, leaf_value=LOSS):
    """Nodes 0..n-1 in a ring (i -> i + 1 mod n); with leaf_every, every leaf_every-th node has
    a second child, the primitive node n of leaf_value."""
    lists = [[(i + 1) % n] + ([n] if leaf_every and i % leaf_every == 0 else []) for i in range(n)]
    prim = [UNDECIDED] * n
    if leaf_every:
        lists.append([])
        prim.append(leaf_value)
    return graph_ref._csr(prim, lists)
