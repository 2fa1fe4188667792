"""gamesmanmpi_amd/find.py without a GPU: the spec parser, the numpy reference of gm_select on
the golden tables, the pinned layout of gm_select_t and the text of --find on a stub solver.
"""
import ctypes
import io
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, golden

from gamesmanmpi_amd import _lib, find

WIN, LOSS, TIE, DRAW = _lib.SEL_WIN, _lib.SEL_LOSS, _lib.SEL_TIE, _lib.SEL_DRAW
ANY = find.ANY


# ---------------------------------------------------------------- specs
@pytest.mark.parametrize("text, want, normal", [
    ("win", (WIN, 0, ANY, False), "win"),
    ("loss:12", (LOSS, 12, 12, False), "loss:12"),
    ("Lose:3-5", (LOSS, 3, 5, False), "loss:3-5"),
    ("win,tie:0-2", (WIN | TIE, 0, 2, False), "win,tie:0-2"),
    ("tie:max", (TIE, 0, ANY, True), "tie:max"),
    ("draw", (DRAW, 0, ANY, False), "draw"),
    (" TIE , win : 7 ", (WIN | TIE, 7, 7, False), "win,tie:7"),
    ("loss:16383", (LOSS, ANY, ANY, False), "loss:16383"),
])
def test_parse_spec_accepts(text, want, normal):
    s = find.parse_spec(text)
    assert tuple(s) == want and find.spec_text(s) == normal
    assert find.parse_spec(normal) == s


@pytest.mark.parametrize("text, fault", [
    ("", "empty"),
    ("   ", "empty"),
    ("wins:3", "unknown value 'wins'"),
    ("win,:3", "unknown value ''"),
    ("win:5-3", "empty"),
    ("win,loss:max", "exactly one value"),
    ("win:16384", "exceeds"),
    ("win:0-99999", "exceeds"),
    ("win:x", "not a remoteness"),
    ("win:-3", "not a remoteness"),
    ("win:", "not a remoteness"),
])
def test_parse_spec_rejects(text, fault):
    with pytest.raises(ValueError, match=fault):
        find.parse_spec(text)


def test_max_is_resolved_from_the_histogram():
    hist = np.zeros((3, 10), dtype=np.uint64)
    hist[0, 5] = 3
    hist[2, 9] = 1
    assert find.resolve("tie:max", hist) == find.Spec(TIE, 9, 9, False)
    assert find.resolve("win:max", hist) == find.Spec(WIN, 5, 5, False)
    assert find.resolve("loss:max", hist) == find.Spec(LOSS, 0, 0, False)     # a value nobody has
    assert find.resolve("draw:max", hist) == find.Spec(DRAW, 0, 0, False)     # DRAW records carry 0
    assert find.resolve("win:2-4", hist) == find.parse_spec("win:2-4")
    with pytest.raises(ValueError, match="resolve"):
        find.match(np.zeros(1, dtype=np.uint16), "tie:max")


# ---------------------------------------------------------------- the numpy reference
@pytest.mark.parametrize("table, spec, count", [
    ("ttt", "tie:9", 1), ("ttt", "win:5", 122), ("ttt", "loss:4", 124),
    ("othello_4x4", "loss:12", 1), ("othello_4x4", "win:11", 4), ("othello_4x4", "tie:7", 12),
    ("toot_4x3", "tie:12", 1), ("toot_4x3", "win:9", 92), ("toot_4x3", "loss:8", 112),
])
def test_from_records_on_golden_tables(table, spec, count):
    keys, recs = golden(table)
    k, r = find.from_records(keys, recs, spec)
    s = find.parse_spec(spec)
    assert len(k) == len(r) == count
    assert (np.diff(k.astype(object)) > 0).all()                              # ascending, distinct
    want = (s.values.bit_length() - 1) << 14 | s.rem_lo
    assert (r == want).all()
    # exactly the keys a plain loop selects
    assert sorted(int(x) for x in k) == sorted(int(x) for x, y in zip(keys, recs) if int(y) == want)


def test_from_records_edges():
    assert int(find.from_records(*golden("ttt"), "tie:9")[0][0]) == 0         # the empty board
    keys = np.array([9, 3, 7, 5, 1], dtype=np.uint64)
    recs = np.array([0x0002, 0xFFFF, 0x4002, 0xC000, 0x8000], dtype=np.uint16)
    k, r = find.from_records(keys, recs, "win,loss:2")
    assert k.tolist() == [7, 9] and r.tolist() == [0x4002, 0x0002]
    assert find.from_records(keys, recs, "draw")[0].tolist() == [5]
    assert find.from_records(keys, recs, "win,loss,tie,draw")[0].tolist() == [1, 5, 7, 9]   # 0xFFFF never matches
    assert find.from_records(keys, recs, "tie:1-9")[0].tolist() == []
    # multi-word keys: ascending as one integer, words least significant first
    wide = np.array([[5, 0, 1], [9, 0, 0], [1, 2, 0]], dtype=np.uint64)
    k, r = find.from_records(wide, np.array([1, 1, 1], dtype=np.uint16), "win:1")
    assert k.tolist() == [[9, 0, 0], [1, 2, 0], [5, 0, 1]]


# ---------------------------------------------------------------- header layout
def test_select_layout_pinned(tmp_path):
    """gcc's sizeof / offsetof of gm_select_t equal the ctypes mirror's; the ABI version stays 2."""
    fields = [n for n, _ in _lib.Select._fields_]
    src = tmp_path / "pin.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmsolve.h"\nint main(void){\n'
                   '  printf("%zu\\n", sizeof(gm_select_t));\n'
                   + "".join('  printf("%%zu\\n", offsetof(gm_select_t, %s));\n' % f for f in fields)
                   + '  printf("%d %d %d %d\\n", GM_SEL_WIN, GM_SEL_LOSS, GM_SEL_TIE, GM_SEL_DRAW);\n'
                   + '  printf("%d\\n", GM_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "pin"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    vals = [int(x) for x in lines[:1 + len(fields)]]
    assert vals[0] == ctypes.sizeof(_lib.Select) == 16
    assert vals[1:] == [getattr(_lib.Select, f).offset for f in fields] == [0, 4, 8, 12]
    assert [int(x) for x in lines[1 + len(fields)].split()] == [WIN, LOSS, TIE, DRAW] == [1, 2, 4, 8]
    assert int(lines[2 + len(fields)]) == _lib.ABI_VERSION == 2
    assert "gm_select" in _lib.SYMBOLS


# ---------------------------------------------------------------- text
class _StubCodec:
    game_id = _lib.GAME_TTT
    gens = ()

    def pos(self, key):
        return "p%d" % key


class _StubSolver:
    """Answers find() from a fixed table, as Solver.find does from the device."""
    codec = _StubCodec()
    keys = np.array([4, 2, 8, 6], dtype=np.uint64)
    recs = np.array([0x0005, 0x8009, 0x0005, 0xC000], dtype=np.uint16)

    def analysis(self):
        from gamesmanmpi_amd import analysis
        return analysis.from_records(self.recs[self.recs != 0xC000])

    def find(self, spec, rem=None, cap=16, with_keys=False):
        spec = find.resolve(spec, self.analysis())
        k, r = find.from_records(self.keys, self.recs, spec)
        rows = [(self.codec.pos(int(x)), int(y) >> 14, int(y) & 0x3FFF) for x, y in zip(k[:cap], r[:cap])]
        return (len(k), rows, [int(x) for x in k[:cap]]) if with_keys else (len(k), rows)


def test_format_lines():
    assert find.format_lines(2, [("p4", 0, 5), ("p8", 0, 5)], "Win:5") == \
        ["Found 2 positions: win:5", "  'p4': WIN in 5", "  'p8': WIN in 5"]
    assert find.format_lines(1, [((0, 1), 3, 0)], "draw") == ["Found 1 positions: draw", "  (0, 1): DRAW"]
    assert find.format_lines(0, [], "loss:2-3") == ["Found 0 positions: loss:2-3"]


def test_report_text_and_json(tmp_path):
    out = io.StringIO()
    find.report(_StubSolver(), ["tie:max", "win:5", "draw", "loss"], 1, out, str(tmp_path))
    assert out.getvalue().splitlines() == [
        "Found 1 positions: tie:9", "  'p2': TIE in 9",
        "Found 2 positions: win:5", "  'p4': WIN in 5",                       # cap 1: the smallest key
        "Found 1 positions: draw", "  'p6': DRAW",
        "Found 0 positions: loss",
    ]
    j = json.load(open(tmp_path / "stats" / "find.json"))
    assert j == [{"spec": "tie:9", "n": 1, "keys": ["0x2"], "records": [0x8009]},
                 {"spec": "win:5", "n": 2, "keys": ["0x4"], "records": [0x0005]},
                 {"spec": "draw", "n": 1, "keys": ["0x6"], "records": [0xC000]},
                 {"spec": "loss", "n": 0, "keys": [], "records": []}]
    quiet = io.StringIO()
    find.report(_StubSolver(), ["win:5"], 4, quiet, rank=1)                   # only rank 0 writes
    assert quiet.getvalue() == ""


def test_report_merges_the_ranks_of_a_sharded_solve(tmp_path):
    """Two gloo ranks, each holding every other pair of a 40-position table: the counts are
    summed, the rows merged ascending and cut at the cap, ':max' comes from the summed
    histogram, and rank 0 alone writes."""
    import socket
    from mp_ranks import run_ranks
    from select_ranks import report_main
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    texts = run_ranks(report_main, 2, (["win:max", "loss:2-3", "tie"], 4, str(tmp_path)), timeout=120)
    keys = np.arange(40, dtype=np.uint64)
    recs = ((keys % 3) << 14 | (keys % 7)).astype(np.uint16)
    want = []
    for spec in ("win:6", "loss:2-3", "tie"):
        k, r = find.from_records(keys, recs, spec)
        want += find.format_lines(len(k), [("p%d" % x, int(y) >> 14, int(y) & 0x3FFF) for x, y in zip(k[:4], r[:4])], spec)
    assert texts[1] == "" and texts[0].splitlines() == want
    j = json.load(open(tmp_path / "stats" / "find.json"))
    assert [b["spec"] for b in j] == ["win:6", "loss:2-3", "tie"]
    assert j[1]["n"] == 4 and j[1]["keys"] == [hex(x) for x in (10, 16, 31, 37)]
