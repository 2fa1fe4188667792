"""gm_reach without a device: the structs and the call's refusals, and the host side of
gamesmanmpi_amd/reach.py (reference, is_closed) on the golden tic-tac-toe table."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, golden
from gamesmanmpi_amd import Context, _lib, reach

TTT = 2
HOW = ("mover", "other", "max_plies", "reserved")
OUT = ("n", "n_mover", "n_other", "n_starts", "edges", "missing", "plies", "reserved")
# tic-tac-toe's positions by the ply at which they appear: 5,478 in all
TTT_PLIES = [1, 9, 72, 252, 756, 1260, 1520, 1140, 390, 78]
POLICIES = ("all", "best", "first")


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "pin.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmsolve.h"\nint main(void){\n'
                   '  printf("%zu\\n", sizeof(gm_reach_t));\n'
                   + "".join('  printf("%%zu\\n", offsetof(gm_reach_t, %s));\n' % f for f in HOW)
                   + '  printf("%zu\\n", sizeof(gm_reach_out_t));\n'
                   + "".join('  printf("%%zu\\n", offsetof(gm_reach_out_t, %s));\n' % f for f in OUT)
                   + '  printf("%d %d %d\\n", GM_REACH_ALL, GM_REACH_BEST, GM_REACH_FIRST);\n'
                   + '  return 0;\n}\n')
    exe = tmp_path / "pin"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(_lib.Reach) == 16
    assert vals[1:5] == [getattr(_lib.Reach, f).offset for f in HOW]
    assert vals[5] == ctypes.sizeof(_lib.ReachOut) == 56
    assert vals[6:14] == [getattr(_lib.ReachOut, f).offset for f in OUT]
    assert vals[14:] == [_lib.REACH_ALL, _lib.REACH_BEST, _lib.REACH_FIRST] == [0, 1, 2]
    assert "gm_reach" in _lib.SYMBOLS and _lib.lib().gm_version() == 2


def test_refusals_without_a_solve():
    ctx = Context(TTT, ())
    keys = np.zeros(2, dtype=np.uint64)
    out = _lib.ReachOut()
    call = ctx.L.gm_reach

    def go(how, kp=keys.ctypes.data, n=2, outp=ctypes.byref(out)):
        return call(ctx.h, how, kp, n, outp, None, 0, None, None, None, 0)

    ok = _lib.Reach(0, 0, 0, 0)
    assert go(ctypes.byref(ok)) == -5                                    # GM_E_STATE: nothing solved
    assert go(ctypes.byref(ok), None, 0) == -5
    assert go(None) == -1                                                # GM_E_ARG first
    assert go(ctypes.byref(ok), outp=None) == -1
    assert go(ctypes.byref(_lib.Reach(3, 0, 0, 0))) == -1
    assert go(ctypes.byref(_lib.Reach(0, 3, 0, 0))) == -1
    assert go(ctypes.byref(_lib.Reach(0, 0, 0, 1))) == -1
    assert go(ctypes.byref(ok), None, 2) == -1
    assert b"gm_reach" in ctx.L.gm_last_error()
    ctx.close()


def test_policy_names():
    assert [reach.policy(p) for p in POLICIES] == [0, 1, 2] == [reach.policy(i) for i in range(3)]
    with pytest.raises(ValueError):
        reach.policy("worst")
    with pytest.raises(ValueError):
        reach.policy(3)
    W, L, T = 3, 0x4000 | 2, 0x8000 | 1
    kids, recs = [10, 11, 12, 13, 14], [W, L, T, L, 0xFFFF]
    assert reach.selected(kids, recs, 0) == kids
    assert reach.selected(kids, recs, 1) == [11, 13] and reach.selected(kids, recs, 2) == [11]
    assert reach.selected([], [], 1) == []
    assert reach.selected([7, 8], [0xFFFF, 0xFFFF], 1) == [7, 8]         # nothing known: all equal


@pytest.fixture(scope="module")
def ttt():
    keys, recs = golden("ttt")
    ctx = Context(TTT, ())
    memo = {}

    def expand(k):
        if k not in memo:
            memo[k] = ctx.expand(k)
        return memo[k]

    yield dict(zip(keys.tolist(), recs.tolist())), expand, ctx.initial()
    ctx.close()


def test_reference_reaches_every_position_of_the_golden_ttt_table(ttt):
    table, expand, root = ttt
    out, plies, marks = reach.reference([root], table, expand)
    assert out["n"] == 5478 == len(table) and plies == TTT_PLIES and sum(plies) == 5478
    assert set(marks) == set(table)
    assert (out["n_mover"], out["n_other"]) == (sum(TTT_PLIES[0::2]), sum(TTT_PLIES[1::2]))
    assert out["n_mover"] + out["n_other"] == out["n"]                   # a board names its ply: one side each
    assert (out["n_starts"], out["missing"], out["plies"]) == (1, 0, 10)
    interior = [k for k in table if expand(k)[0] == 4]
    assert out["edges"] == sum(len(expand(k)[1]) for k in interior)


def k_ply(k):
    """The ply of a tic-tac-toe key: its non-empty base-3 digits."""
    n = 0
    while k:
        n += k % 3 != 0
        k //= 3
    return n


def test_side_is_the_parity_of_the_ply(ttt):
    table, expand, root = ttt
    _, _, marks = reach.reference([root], table, expand)
    assert all(bits == 1 << (k_ply(k) & 1) for k, bits in marks.items())


def test_every_policy_pair_is_closed_and_nested(ttt):
    table, expand, root = ttt
    got = {}
    for mover, other in itertools.product(POLICIES, POLICIES):
        out, plies, marks = reach.reference([root], table, expand, mover, other)
        assert reach.is_closed(marks, table, expand, mover, other, starts=[root]), (mover, other)
        assert out["n"] == len(marks) == sum(plies) and out["missing"] == 0
        got[mover, other] = marks
    for a, b in itertools.product(POLICIES, POLICIES):
        # a wider policy on either side reaches a superset: ALL >= BEST >= FIRST
        for wider in POLICIES[:POLICIES.index(a) + 1]:
            assert set(got[a, b]) <= set(got[wider, b])
        for wider in POLICIES[:POLICIES.index(b) + 1]:
            assert set(got[a, b]) <= set(got[a, wider])
    assert len(got["first", "first"]) == 10                              # one line of play
    assert len(got["first", "all"]) < len(got["best", "all"]) < len(got["all", "all"]) == 5478
    # a set that misses a selected child is not closed
    broken = dict(got["best", "all"])
    del broken[max(k for k in broken if k != root)]
    assert not reach.is_closed(broken, table, expand, "best", "all", starts=[root])
    assert not reach.is_closed({}, table, expand, "all", "all", starts=[root])


def test_reference_bounds_starts_and_missing_children(ttt):
    table, expand, root = ttt
    out, plies, marks = reach.reference([root], table, expand, max_plies=3)
    assert plies == TTT_PLIES[:4] and out["plies"] == 4 and out["n"] == sum(TTT_PLIES[:4])
    kids = expand(root)[1]
    out, plies, marks = reach.reference([kids[0], 19683, kids[0], 4, kids[1]], table, expand)
    assert out["n_starts"] == 3 and plies[0] == 2 and marks[kids[0]] & 1
    holed = dict(table)
    del holed[kids[4]]
    out, plies, marks = reach.reference([root], holed, expand)
    assert out["missing"] >= 1 and kids[4] not in marks and plies[1] == 8
    assert reach.is_closed(marks, holed, expand, starts=[root])


def test_reference_closes_under_symmetry_maps(ttt):
    """Closing under a map that fixes the table: every image is marked with its original, and
    the counts are those of the plain search when the starts are closed under the map."""
    table, expand, root = ttt

    def mirror(k):                                                       # swap the board's columns 0 and 2
        d = [(k // 3 ** i) % 3 for i in range(9)]
        d = [d[3 * (i // 3) + 2 - i % 3] for i in range(9)]
        return sum(x * 3 ** i for i, x in enumerate(d))

    assert all(mirror(k) in table and table[mirror(k)] == r for k, r in table.items())
    plain = reach.reference([root], table, expand, "best", "all")
    closed = reach.reference([root], table, expand, "best", "all", symmetries=[mirror])
    assert closed[1] == plain[1] and closed[2] == plain[2]
    assert closed[0]["edges"] < plain[0]["edges"]                        # one member of an orbit is expanded


def test_format_strategy():
    out = dict(n=30, plies=3)
    assert reach.format_strategy("player to move", "TIE in 9 moves", out, 120, [1, 9, 20]) == [
        "Strategy for the player to move (root TIE in 9 moves): 30 of 120 positions (25.00%), deepest ply 2",
        "  ply 0: 1", "  ply 1: 9", "  ply 2: 20"]
