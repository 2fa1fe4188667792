"""gm_moves without a device: the struct and the call's refusals, and the host side of
gamesmanmpi_amd/moves.py (rank, optimal_mask, reference) against solver.move_rank, solver.best_move
and the golden tic-tac-toe table."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import REPO, golden
from gamesmanmpi_amd import Context, _lib, moves
from gamesmanmpi_amd.solver import best_move, move_rank

TTT = 2
FIELDS = ("first", "count", "best", "record", "n_best")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "pin.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmsolve.h"\nint main(void){\n'
                   '  printf("%zu\\n", sizeof(gm_moves_t));\n'
                   + "".join('  printf("%%zu\\n", offsetof(gm_moves_t, %s));\n' % f for f in FIELDS)
                   + '  return 0;\n}\n')
    exe = tmp_path / "pin"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(_lib.Moves) == 16 == _lib.moves_dtype().itemsize
    assert vals[1:] == [getattr(_lib.Moves, f).offset for f in FIELDS]
    assert vals[1:] == [_lib.moves_dtype().fields[f][1] for f in FIELDS]
    assert "gm_moves" in _lib.SYMBOLS and _lib.lib().gm_version() == 2


def test_refusals_without_a_device():
    ctx = Context(TTT, ())
    keys = np.zeros(2, dtype=np.uint64)
    heads = np.zeros(2, dtype=_lib.moves_dtype())
    total = ctypes.c_uint64(77)
    call = ctx.L.gm_moves
    assert call(ctx.h, keys.ctypes.data, 2, heads.ctypes.data, None, None, 0, ctypes.byref(total)) == -5   # GM_E_STATE
    assert call(ctx.h, None, 0, None, None, None, 0, ctypes.byref(total)) == -5
    assert call(ctx.h, keys.ctypes.data, 2, heads.ctypes.data, None, None, 0, None) == -1                  # GM_E_ARG first
    assert call(ctx.h, None, 2, heads.ctypes.data, None, None, 0, ctypes.byref(total)) == -1
    assert call(ctx.h, keys.ctypes.data, 2, None, None, None, 0, ctypes.byref(total)) == -1
    ctx.close()


def test_rank_is_move_rank_over_every_record():
    recs = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got = moves.rank(recs)
    assert got.dtype == np.uint32
    assert got.tolist() == [move_rank(r) for r in range(65536)]


def test_reference_on_the_golden_ttt_table():
    keys, recs = golden("ttt")
    table = dict(zip(keys.tolist(), recs.tolist()))
    ctx = Context(TTT, ())
    heads, kids, krecs = moves.reference(keys, table, ctx.expand)
    root = int(np.flatnonzero(keys == ctx.initial())[0])
    h = heads[root]
    assert (int(h["count"]), int(h["best"]), int(h["n_best"]), int(h["record"])) == (9, 0, 9, 0x8009)
    first = int(h["first"])
    assert kids[first:first + 9] == ctx.expand(ctx.initial())[1]
    assert (krecs[first:first + 9] == 0x8008).all()
    assert np.array_equal(heads["record"], recs)
    assert np.array_equal(heads["first"], np.cumsum(heads["count"].astype(np.uint64)) - heads["count"])
    assert len(kids) == len(krecs) == int(heads["count"].sum())
    interior = 0
    for k, h in zip(keys.tolist(), heads):
        a, n = int(h["first"]), int(h["count"])
        if not n:
            assert ctx.expand(k)[0] != 4 and int(h["best"]) == -1 and int(h["n_best"]) == 0
            continue
        interior += 1
        best, (v, r) = best_move(krecs[a:a + n])
        assert int(h["best"]) == best
        assert int(h["record"]) == (v << 14 | r)          # the parent record its best child implies
        assert int(h["n_best"]) == sum(move_rank(x) == move_rank(krecs[a + best]) for x in krecs[a:a + n])
    assert interior == int((heads["count"] > 0).sum()) > 4000
    # a key without a record lists nothing and is never expanded (19683 is no tic-tac-toe key)
    h2, k2, r2 = moves.reference([19683, ctx.initial(), ctx.initial()], table, ctx.expand)
    assert h2["record"].tolist() == [0xFFFF, 0x8009, 0x8009] and h2["count"].tolist() == [0, 9, 9]
    assert h2["first"].tolist() == [0, 0, 9] and h2["best"].tolist() == [-1, 0, 0] and k2[:9] == k2[9:]
    ctx.close()


def test_optimal_mask_and_best_on_hand_made_heads():
    W = lambda r: r                      # noqa: E731  WIN in r
    L = lambda r: 0x4000 | r             # noqa: E731
    T = lambda r: 0x8000 | r             # noqa: E731
    DRAW, NONE = 0xC000, 0xFFFF
    segs = [
        [W(3), L(4), L(2), L(2), T(1)],      # two shortest losses tie for best: the first of them
        [W(3), W(5), W(5), NONE],            # the longest wins; a child without a record ranks lowest
        [],                                  # no children
        [W(9), DRAW, T(4), T(2)],            # a TIE child beats a DRAW child beats a WIN child
        [W(9), DRAW, DRAW],                  # DRAW over WIN
        [NONE, NONE],                        # nothing known: the first, both equal
        [L(0)],
    ]
    want_best = [2, 1, -1, 3, 1, 0, 0]
    want_n = [2, 2, 0, 1, 2, 2, 1]
    want_mask = [[0, 0, 1, 1, 0], [0, 1, 1, 0], [], [0, 0, 0, 1], [0, 1, 1], [1, 1], [1]]
    recs = np.array([r for s in segs for r in s], dtype=np.uint16)
    counts = np.array([len(s) for s in segs])
    best, n_best = moves.best_of(recs, counts)
    assert best.tolist() == want_best and n_best.tolist() == want_n
    assert best.tolist() == [-1 if not s else best_move(s)[0] for s in segs]
    heads = np.zeros(len(segs), dtype=_lib.moves_dtype())
    heads["count"], heads["best"], heads["n_best"] = counts, best, n_best
    heads["first"] = np.cumsum(counts) - counts
    mask = moves.optimal_mask(heads, recs)
    assert mask.tolist() == [bool(x) for s in want_mask for x in s]
    assert np.array_equal(np.bincount(moves.segments(heads)[mask], minlength=len(segs)), n_best)
    assert moves.optimal_mask(heads[2:3], recs[:0]).tolist() == []


def test_format_rows_stars_every_optimal_move():
    rows = [("a", "p1", 0, 3), ("b", "p2", 1, 2), ("c", "p3", 1, 2), ("d", "p4", None, None), ("e", "p5", 3, 0)]
    assert moves.format_rows(rows) == ["  'a' -> 'p1': WIN in 3", "  'b' -> 'p2': LOSS in 2 *", "  'c' -> 'p3': LOSS in 2 *",
                                       "  'd' -> 'p4': not stored", "  'e' -> 'p5': DRAW"]
    assert moves.format_block(rows[:1]) == ["Moves:", "  'a' -> 'p1': WIN in 3 *"]
    assert moves.format_rows([]) == [] and moves.format_rows(rows[4:], indent="    ") == ["    'e' -> 'p5': DRAW *"]
