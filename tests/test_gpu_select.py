"""gm_select on the device: the positions of a solved table with a wanted value and a remoteness
in range (csrc/select_common.hpp), for every engine and every way a context holds a solve, and
what is built on it: Solver.find, Solver.line, --find and --line.

Expected sets come from `find.from_records` over golden or C-oracle tables, or from
tests/loopy_ref.py, never from the device's own export (the one exception is named in its test).
"""
import ctypes
import io
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO, golden, load_plugin

pytestmark = pytest.mark.gpu

from gamesmanmpi_amd import Context, GMError, Solver, _lib, analysis, find  # noqa: E402

F2O, TTT, TOOT, OTH, SUB = 1, 2, 3, 4, 5
WIN, LOSS, TIE, DRAW = _lib.SEL_WIN, _lib.SEL_LOSS, _lib.SEL_TIE, _lib.SEL_DRAW
ANY = _lib.SEL_ANY_REM


def _solve(game, params=(), root=None, engine=None, **opts):
    ctx = Context(game, params, device=0)
    if engine is not None:
        ctx.set_option(_lib.OPT_ENGINE, engine)
    for k, v in opts.items():
        ctx.set_option(getattr(_lib, "OPT_" + k.upper()), v)
    ctx.solve(ctx.initial() if root is None else root)
    return ctx


def _cells(recs):
    """The non-empty (value, remoteness) cells of a table: record -> count."""
    u, c = np.unique(np.asarray(recs, dtype=np.uint16), return_counts=True)
    return {int(r): int(k) for r, k in zip(u, c) if int(r) != 0xFFFF}


def _check_cells(ctx, keys, recs):
    """Every non-empty cell of the expected table: select with that one cell returns the cell's
    count and exactly its keys, ascending, with its record; the counts sum to the digest's."""
    keys, recs = np.asarray(keys, dtype=np.uint64), np.asarray(recs, dtype=np.uint16)
    total = 0
    for rec, count in sorted(_cells(recs).items()):
        n, k, r = ctx.select(1 << (rec >> 14), rec & 0x3FFF, rec & 0x3FFF, count + 3, as_array=True)
        assert n == count == len(k), (hex(rec), n, count)
        assert np.array_equal(k, np.sort(keys[recs == rec])), hex(rec)
        assert (r == rec).all()
        total += n
    assert total == ctx.digest()[1] == len(keys)


def _select_spec(ctx, spec, cap):
    s = find.parse_spec(spec)
    return ctx.select(s.values, s.rem_lo, s.rem_hi, cap, as_array=True)


# ---------------------------------------------------------------- small games
@pytest.mark.parametrize("engine", [_lib.ENGINE_DENSE, _lib.ENGINE_SPARSE])
def test_ttt(engine):
    ctx = _solve(TTT, engine=engine)
    _check_cells(ctx, *golden("ttt"))
    n, k, r = ctx.select(TIE, 9, 9)
    assert (n, k, r.tolist()) == (1, [ctx.initial()], [0x8009])
    ctx.close()


def test_four_to_one_root_6():
    ctx = _solve(F2O, root=6)
    _check_cells(ctx, *golden("four_to_one_six"))
    ctx.close()


# ---------------------------------------------------------------- orbit members, virtual ranks
@pytest.mark.parametrize("ranks", [1, 4])
@pytest.mark.parametrize("sym", [1, 0])
def test_othello_4x4_orbits_and_virtual_ranks(sym, ranks):
    keys, recs = golden("othello_4x4")
    ctx = _solve(OTH, (4, 4), symmetry=sym, virtual_ranks=ranks)
    _check_cells(ctx, keys, recs)                                       # every orbit member once
    want_k, want_r = find.from_records(keys, recs, "win,tie:2-5")
    n, k, r = _select_spec(ctx, "win,tie:2-5", len(want_k) + 1)
    assert n == len(want_k) and np.array_equal(k, want_k) and np.array_equal(r, want_r)
    ctx.close()


@pytest.mark.parametrize("sym", [1, 0])
def test_toot_4x3_orbits(sym):
    ctx = _solve(TOOT, (4, 3), symmetry=sym)
    _check_cells(ctx, *golden("toot_4x3"))
    ctx.close()


def test_toot_4x4_vs_oracle(oracle):
    ctx = _solve(TOOT, (4, 4), symmetry=1)
    _check_cells(ctx, *oracle.solve(TOOT, (4, 4)))
    ctx.close()


# ---------------------------------------------------------------- 128-bit keys, 32-byte slots
@pytest.mark.parametrize("ranks", [1, 8])
def test_othello_8x8_endgame_10(ranks):
    """The golden keys of this table are hashes, not ABI keys: the counts per cell come from
    the golden records, and what was selected is checked through query()."""
    s = Solver(load_plugin("tests/plugins/othello8_endgame.py"), device=0)
    assert s.ctx.words == 3
    if ranks > 1:
        s.ctx.set_option(_lib.OPT_VIRTUAL_RANKS, ranks)
    s.solve()
    total = 0
    for rec, count in sorted(_cells(golden("othello_8x8_endgame")[1]).items()):
        n, k, r = s.ctx.select(1 << (rec >> 14), rec & 0x3FFF, rec & 0x3FFF, count, as_array=True)
        assert n == count and k.shape == (count, 3) and (r == rec).all()
        assert (s.ctx.query(k) == rec).all()
        ints = [_lib.words_to_int(w) for w in k]
        assert ints == sorted(set(ints))                                 # ascending, distinct
        total += n
    assert total == 56552 == s.ctx.digest()[1]
    assert s.ctx.select(LOSS, 11, 11)[:2] == (1, [s.root_key])
    assert s.ctx.select(WIN, 10, 10)[0] == 1 and s.ctx.select(TIE, 6, 6)[0] == 1
    n, rows = s.find("loss:11")
    assert n == 1 and rows == [(s.root, 1, 11)]
    s.close()


# ---------------------------------------------------------------- block engine
@pytest.mark.parametrize("interleave", [1, 6, 10])
@pytest.mark.parametrize("heaps", [3, 5])
def test_subtract_block_engine(oracle, heaps, interleave):
    recs = oracle.subtract_dense(heaps)
    ctx = _solve(SUB, (heaps,), sub_interleave=interleave)
    _check_cells(ctx, np.arange(len(recs), dtype=np.uint64), recs)
    ctx.close()


# ---------------------------------------------------------------- box engine, 8 heaps
def _region(table, root, heaps):
    """(keys, records) of the root's region of a (16,) * heaps record table (heap heaps - 1
    first): every heap at most the root's."""
    dims = [((root >> (4 * j)) & 15) + 1 for j in range(heaps)]
    part = table[tuple(slice(0, d) for d in reversed(dims))]
    idx = np.indices(part.shape)
    keys = sum(idx[a].astype(np.uint64) << np.uint64(4 * (heaps - 1 - a)) for a in range(heaps))
    return keys.ravel(), part.ravel()


@pytest.mark.parametrize("root", [0x00000003, 0x000F0FFF, 0x12345678])
def test_box_engine_custom_roots(oracle, root):
    """One box; unaligned nibbles in the quarter heaps; a stone on every heap.  Heaps 5 to 7 of
    the first two roots are empty, so their regions are the 5-heap game's."""
    ctx = _solve(SUB, (8,), root=root)
    assert ctx.stats()["engine"] == _lib.ENGINE_DENSE
    if root < 16 ** 5:
        keys, recs = _region(oracle.subtract_dense(5).reshape((16,) * 5), root, 5)
    else:
        keys, recs = oracle.solve(SUB, (8,), root)
    _check_cells(ctx, keys, recs)
    ctx.close()


@pytest.fixture(scope="module")
def root_3355(oracle):
    return oracle.solve(SUB, (8,), root=0x33557777)


@pytest.mark.parametrize("opts", [{}, {"virtual_ranks": 2}, {"virtual_ranks": 8},
                                  {"sub_interleave": 10, "virtual_ranks": 4}],
                         ids=["one", "split2", "split8", "dist_sub4"])
def test_box_engine_split_and_dist_sub(root_3355, opts):
    ctx = _solve(SUB, (8,), root=0x33557777, **opts)
    assert ctx.stats()["engine"] == (_lib.ENGINE_DIST_DENSE if opts else _lib.ENGINE_DENSE)
    _check_cells(ctx, *root_3355)
    ctx.close()


def _swap_heaps(keys, a, b):
    keys = np.asarray(keys, dtype=np.uint64)
    sa, sb = np.uint64(4 * a), np.uint64(4 * b)
    ha, hb = (keys >> sa) & np.uint64(15), (keys >> sb) & np.uint64(15)
    return (keys & ~((np.uint64(15) << sa) | (np.uint64(15) << sb))) | (ha << sb) | (hb << sa)


def test_full_2_32():
    ref = json.load(open(os.path.join(GOLDEN, "histograms.json")))["subtract_8"]
    assert sum(ref["loss"][78:81]) == 2048 and ref["loss"][80] == 128 and len(ref["loss"]) == 81
    ctx = _solve(SUB, (8,))
    n, k, r = ctx.select(LOSS, 78, 80, 4096, as_array=True)
    assert n == 2048 == len(k) and (np.diff(k.astype(np.int64)) > 0).all()
    assert np.array_equal(ctx.query(k), r) and set((r & 0x3FFF).tolist()) <= {78, 79, 80} and (r >> 14 == 1).all()
    assert [int((r == (1 << 14 | x)).sum()) for x in (78, 79, 80)] == ref["loss"][78:81]
    # the game does not tell heaps 0 and 1 apart, nor heaps 4 and 5
    have = set(k.tolist())
    assert set(_swap_heaps(k, 0, 1).tolist()) == have and set(_swap_heaps(k, 4, 5).tolist()) == have
    n0, k0, r0 = ctx.select(LOSS, 0, 0)
    assert (n0, k0, r0.tolist()) == (1, [0], [0x4000])
    n, k, r = ctx.select(WIN | LOSS, 0, ANY, 8, as_array=True)
    assert n == 2 ** 32 and len(k) == 8 and (np.diff(k.astype(np.int64)) > 0).all()
    assert np.array_equal(ctx.query(k), r) and (r != 0xFFFF).all()
    assert ctx.select(TIE | DRAW)[0] == 0                                # no code says TIE or DRAW
    ctx.close()


# ---------------------------------------------------------------- cap and the second pass
def test_cap_below_the_count():
    keys, recs = golden("ttt")
    want = set(find.from_records(keys, recs, "win:5")[0].tolist())
    for engine in (_lib.ENGINE_DENSE, _lib.ENGINE_SPARSE):
        ctx = _solve(TTT, engine=engine)
        n, k, r = ctx.select(WIN, 5, 5, 10)
        assert n == 122 and len(k) == 10 and k == sorted(set(k)) and set(k) <= want and (r == 5).all()
        assert ctx.select(WIN, 5, 5, 0)[:2] == (122, [])
        what, cnt = _lib.Select(WIN, 5, 5, 0), ctypes.c_uint64()
        rbuf = np.full(4, 7, dtype=np.uint16)
        assert ctx.L.gm_select(ctx.h, ctypes.byref(what), None, rbuf.ctypes.data, 4, ctypes.byref(cnt)) == 0
        assert cnt.value == 122 and (rbuf == 7).all()                    # key_words == NULL: the count only
        kbuf = np.zeros(4, dtype=np.uint64)
        assert ctx.L.gm_select(ctx.h, ctypes.byref(what), kbuf.ctypes.data, None, 4, ctypes.byref(cnt)) == 0
        assert cnt.value == 122 and set(kbuf.tolist()) <= want and len(set(kbuf.tolist())) == 4   # records may be NULL
        ctx.close()


@pytest.mark.parametrize("sym", [1, 0])
def test_second_pass_beyond_the_first_list(sym):
    """Toot 4x3 has 148,677 TIE positions: more than the 2^16 pairs the first pass keeps."""
    keys, recs = golden("toot_4x3")
    want_k, want_r = find.from_records(keys, recs, "tie")
    assert len(want_k) == 148677
    ctx = _solve(TOOT, (4, 3), symmetry=sym)
    n, k, r = ctx.select(TIE, 0, ANY, 200000, as_array=True)
    assert n == 148677 and np.array_equal(k, want_k) and np.array_equal(r, want_r)
    n, k, r = ctx.select(TIE, 0, ANY, 70000, as_array=True)               # a second pass that still falls short
    assert n == 148677 and len(k) == 70000 and (np.diff(k.astype(np.int64)) > 0).all()
    assert np.isin(k, want_k).all() and np.array_equal(ctx.query(k), r)
    ctx.close()


# ---------------------------------------------------------------- the call's contract
def _raw(ctx, what, n=True, cap=0):
    cnt = ctypes.c_uint64(77)
    rc = ctx.L.gm_select(ctx.h, ctypes.byref(what) if what is not None else None, None, None, cap,
                         ctypes.byref(cnt) if n else None)
    return rc, cnt.value


def test_call_contract():
    ctx = Context(TTT, (), device=0)
    ok = _lib.Select(WIN, 0, ANY, 0)
    assert _raw(ctx, ok)[0] == -5                                        # GM_E_STATE before a solve
    with pytest.raises(GMError, match="GM_E_STATE"):
        ctx.select(WIN)
    bad = [None, _lib.Select(0, 0, ANY, 0), _lib.Select(16, 0, ANY, 0), _lib.Select(WIN | 32, 0, 1, 0),
           _lib.Select(WIN, 5, 4, 0), _lib.Select(WIN, 0, ANY, 1)]
    for what in bad:                                                     # GM_E_ARG, checked first
        assert _raw(ctx, what)[0] == -1
    assert _raw(ctx, ok, n=False)[0] == -1
    ctx.solve(ctx.initial())
    for what in bad:
        assert _raw(ctx, what)[0] == -1
    assert _raw(ctx, ok, n=False)[0] == -1
    assert _raw(ctx, ok) == (0, int(analysis.from_records(golden("ttt")[1])[0].sum()))
    assert _raw(ctx, _lib.Select(DRAW, 0, ANY, 0)) == (0, 0)              # no DRAW here: nothing, no error
    assert _raw(ctx, _lib.Select(WIN, 0, 0xFFFFFFFF, 0))[0] == 0         # rem_hi past 0x3FFF: no upper bound
    ctx.close()


@pytest.mark.parametrize("engine", [_lib.ENGINE_DENSE, _lib.ENGINE_SPARSE])
def test_poke_moves_a_key_between_cells(engine):
    ctx = _solve(TTT, engine=engine)
    root = ctx.initial()
    before = ctx.select(WIN, 3, 3, 4096)[1]
    assert root not in before and ctx.select(TIE, 9, 9)[1] == [root]
    ctx.poke(root, 3)                                                    # WIN in 3
    assert ctx.select(TIE, 9, 9)[:2] == (0, [])
    assert ctx.select(WIN, 3, 3, 4096)[1] == sorted(before + [root])
    ctx.poke(root, 0xFFFF)                                               # removed: matches nothing
    assert ctx.select(WIN, 3, 3, 4096)[1] == before
    assert ctx.select(WIN | LOSS | TIE | DRAW)[0] == 5477
    ctx.close()


def test_poke_in_a_byte_table(oracle):
    ctx = _solve(SUB, (8,), root=0x00000333)
    key = 0x123
    rec = int(ctx.query([key])[0])
    cell = (1 << (rec >> 14), rec & 0x3FFF, rec & 0x3FFF)
    other = (rec ^ 0x4000) + 1
    assert key in ctx.select(*cell, 4096)[1]
    ctx.poke(key, other)
    assert key not in ctx.select(*cell, 4096)[1]
    assert key in ctx.select(1 << (other >> 14), other & 0x3FFF, other & 0x3FFF, 4096)[1]
    ctx.close()


def test_import_then_select():
    keys, recs = golden("othello_4x4")
    ctx = Context(OTH, (4, 4), device=0)
    ctx.import_table(keys, recs, ctx.initial())
    for spec in ("loss:12", "tie", "win,loss:3-6"):
        want_k, want_r = find.from_records(keys, recs, spec)
        n, k, r = _select_spec(ctx, spec, len(want_k) + 1)
        assert n == len(want_k) and np.array_equal(k, want_k) and np.array_equal(r, want_r)
    ctx.close()


def test_second_solve_replaces_the_answer():
    ctx = Context(F2O, (), device=0)
    for root, name in ((6, "four_to_one_six"), (4, "four_to_one_four"), (6, "four_to_one_six")):
        ctx.solve(root)
        want_k, want_r = find.from_records(*golden(name), "loss")
        n, k, r = ctx.select(LOSS, 0, ANY, 64, as_array=True)
        assert n == len(want_k) and np.array_equal(k, want_k) and np.array_equal(r, want_r)
    ctx.close()


# ---------------------------------------------------------------- graph engine
def test_graph_chain():
    n = 5000
    prim = np.full(n, 4, dtype=np.uint8)
    prim[-1] = 1
    off = np.minimum(np.arange(n + 1), n - 1).astype(np.uint64)
    kids = np.arange(1, n, dtype=np.uint32)
    ctx = Context(_lib.GAME_GRAPH, (), device=0)
    ctx.solve_graph(prim, off, kids)
    assert ctx.select(LOSS, 4998, 4998)[:2] == (1, [1])
    assert ctx.select(WIN, 4999, 4999)[:2] == (1, [0])
    n_l, k, r = ctx.select(LOSS, 0, ANY, n, as_array=True)
    assert n_l == 2500 and np.array_equal(k, np.arange(1, n, 2)) and np.array_equal(r & 0x3FFF, 4999 - k)
    assert ctx.select(DRAW)[0] == 0
    ctx.close()


def test_graph_plugin_nim3():
    """No golden table for this plugin: the graph engine's export is pinned to the canonical
    oracle by tests/test_graph.py, and the selection must agree with it."""
    s = Solver(load_plugin("tests/plugins/nim3.py"), device=0, graph=True)
    s.solve()
    _check_cells(s.ctx, *s.table())
    s.close()


def test_graph_plugin_with_symmetry_counts_every_member():
    s = Solver(load_plugin("tests/plugins/ttt_symmetric.py"), device=0, graph=True)
    s.solve()
    n, rows = s.find("tie:9")
    assert n == 1 and rows == [(s.root, 2, 9)]
    n, rows = s.find("win:5")
    assert n == 122 and len(rows) == 16 and all(v == 0 and r == 5 for _, v, r in rows)
    assert len({str(p) for p, _, _ in rows}) == 16
    assert s.ctx.select(WIN, 5, 5)[0] < 122                              # the device counts representatives
    assert sum(s.find(v)[0] for v in ("win", "loss", "tie")) == 5478
    s.close()


# ---------------------------------------------------------------- loopy tables
@pytest.fixture(scope="module")
def shuttle():
    import loopy_ref
    from gamesmanmpi_amd.graph import enumerate_graph
    mod = load_plugin("tests/plugins/shuttle.py")
    positions, prim, off, kids = enumerate_graph(mod, mod.initial_position(), workers=1)
    return mod, positions, loopy_ref.solve_loopy(prim, off, kids)


def test_loopy_draws_are_selectable(shuttle):
    mod, positions, recs = shuttle
    s = Solver(mod, device=0, loopy=True)
    s.solve()
    n, rows = s.find("draw", cap=64)
    want = sorted(p for p, r in zip(positions, recs) if int(r) == 0xC000)
    assert n == 19 == len(want) and sorted(p for p, _, _ in rows) == want
    assert all((v, r) == (3, 0) for _, v, r in rows)
    n, rows = s.find("win:9", cap=64)
    assert (0, 1) in [p for p, _, _ in rows]
    assert n == sum(int(r) == 9 for r in recs)
    assert s.find(DRAW | LOSS, rem=0, cap=0)[0] == 19 + sum(int(r) == 0x4000 for r in recs)
    s.close()


# ---------------------------------------------------------------- Solver.line
def test_line_ttt():
    mod = load_plugin("test_games/mttt.py")
    s = Solver(mod, device=0)
    s.solve()
    rows = s.line()
    assert len(rows) == 10 and rows[0][0] is None and rows[0][1] == s.root
    assert [r for _, _, _, r in rows] == list(range(9, -1, -1)) and all(v == 2 for _, _, v, _ in rows)
    assert mod.primitive(rows[-1][1]) != 4 and all(mod.primitive(p) == 4 for _, p, _, _ in rows[:-1])
    for (_, p, _, _), (m, q, _, _) in zip(rows, rows[1:]):                # each step is the move it names
        assert mod.do_move(p, m) == q
    assert s.line(rows[4][1]) == [(None,) + rows[4][1:]] + rows[5:]
    s.close()


def test_line_othello_4x4():
    mod = load_plugin("test_games/othello_bit_new.py", length=4, height=4, area=16)
    s = Solver(mod, device=0)
    s.solve()
    rows = s.line()
    assert len(rows) == s.remoteness + 1 and rows[0][2:] == (s.value, s.remoteness)
    assert [v for _, _, v, _ in rows] == [(s.value + i) % 2 for i in range(len(rows))]   # WIN and LOSS alternate
    assert [r for _, _, _, r in rows] == list(range(s.remoteness, -1, -1))
    assert all(s.lookup(p) == (v, r) for _, p, v, r in rows)
    assert mod.primitive(rows[-1][1]) != 4
    s.close()


def test_line_from_a_draw_ends_on_a_repeat(shuttle):
    mod = shuttle[0]
    s = Solver(mod, device=0, loopy=True)
    s.solve()
    rows = s.line()
    assert all((v, r) == (3, 0) for _, _, v, r in rows) and len(rows) <= 65
    seen = [p for _, p, _, _ in rows]
    assert seen[-1] in seen[:-1] and len(set(seen[:-1])) == len(seen) - 1
    assert len(s.line(max_plies=3)) == 4
    s.close()


# ---------------------------------------------------------------- processes
def _run_ranks(world, game, params, opts, sel):
    import socket
    from select_ranks import rank_main
    from mp_ranks import run_ranks
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    return run_ranks(rank_main, world, (game, params, opts) + sel, timeout=240)


def _check_partition(res, keys, recs):
    want_k, want_r = find.from_records(keys, recs, "win")
    parts = [set(r["keys"]) for r in res]
    assert all(r["count"] == r["found"] == len(r["keys"]) > 0 and r["keys"] == sorted(r["keys"]) for r in res)
    assert not (parts[0] & parts[1]) and sorted(parts[0] | parts[1]) == want_k.tolist()
    table = dict(zip(want_k.tolist(), want_r.tolist()))
    assert all(table[k] == x for r in res for k, x in zip(r["keys"], r["recs"]))


def test_two_processes_sparse_ipc():
    res = _run_ranks(2, OTH, (4, 4), {"sparse_transport": 1}, (WIN, 0, ANY))
    _check_partition(res, *golden("othello_4x4"))


def test_two_processes_box_ipc(root_3355):
    res = _run_ranks(2, SUB, (8,), {"box_transport": 1, "root": 0x33557777}, (WIN, 0, ANY))
    _check_partition(res, *root_3355)


# ---------------------------------------------------------------- command lines
TTT_NP = os.path.join(REPO, "test_games/tic_tac_toe_np.py")
EMPTY = repr(np.zeros((3, 3), dtype=np.int8))


def _blocks(text):
    """The --find blocks of an output: [(header line, number of rows)]; a row starts with two
    spaces and a repr and ends with a record (a numpy board's repr spans lines)."""
    out = []
    for ln in text.splitlines():
        if ln == "Line:":
            break
        if ln.startswith("Found "):
            out.append([ln, 0])
        elif out and re.search(r": (WIN|LOSS|TIE) in \d+$|: DRAW$", ln):
            out[-1][1] += 1
    return [tuple(b) for b in out]


def test_launcher_find_and_line(tmp_path):
    import solver_launcher
    parse = solver_launcher.build_parser().parse_args
    plain = io.StringIO()
    assert solver_launcher.run(parse([TTT_NP]), out=plain) == 0
    assert plain.getvalue() == "TIE in 9 moves\n"                        # without the flags: the root line only
    out = io.StringIO()
    args = parse([TTT_NP, "--find", "tie:max", "--find", "win:5", "-sd", str(tmp_path), "--sd-format", "npz"])
    assert solver_launcher.run(args, out=out) == 0
    text = out.getvalue()
    assert text.startswith(plain.getvalue() + "Found 1 positions: tie:9\n  " + EMPTY + ": TIE in 9\n")
    assert _blocks(text) == [("Found 1 positions: tie:9", 1), ("Found 122 positions: win:5", 16)]
    keys, recs = golden("ttt_np")
    j = json.load(open(tmp_path / "stats" / "find.json"))
    assert [b["spec"] for b in j] == ["tie:9", "win:5"] and [b["n"] for b in j] == [1, 122]
    assert j[0]["keys"] == [hex(0)] and j[0]["records"] == [0x8009]
    assert j[1]["records"] == [5] * 16 and j[1]["keys"] == sorted(j[1]["keys"], key=lambda h: int(h, 16))
    assert {int(h, 16) for h in j[1]["keys"]} <= set(find.from_records(keys, recs, "win:5")[0].tolist())
    out = io.StringIO()
    assert solver_launcher.run(parse([TTT_NP, "--find", "win:5", "--find-cap", "3", "--line"]), out=out) == 0
    text = out.getvalue()
    assert _blocks(text) == [("Found 122 positions: win:5", 3)]
    line = text[text.index("Line:\n"):].splitlines()
    plies = [ln for ln in line if re.match(r"  \d+\. ", ln)]
    assert len(plies) == 10 and plies[0].startswith("  0. array(") and re.match(r"  1\. .* -> array\(", plies[1])
    assert [ln for ln in line if ln.endswith(": TIE in 8")] and line[-1].endswith(": TIE in 0")
    for bad in ("win:5-3", "wins", "win,loss:max"):
        assert solver_launcher.run(parse([TTT_NP, "--find", bad]), out=io.StringIO()) == 2


def test_launcher_line_with_load_and_loopy(tmp_path):
    import solver_launcher
    parse = solver_launcher.build_parser().parse_args
    game = os.path.join(REPO, "test_games/mttt.py")
    assert solver_launcher.run(parse([game, "-sd", str(tmp_path), "--sd-format", "npz"]), out=io.StringIO()) == 0
    out = io.StringIO()
    assert solver_launcher.run(parse([game, "--load", str(tmp_path), "--line", "--find", "tie:max"]), out=out) == 0
    lines = out.getvalue().splitlines()
    assert lines[:4] == ["TIE in 9 moves", "Found 1 positions: tie:9", "  '_________': TIE in 9", "Line:"]
    assert len(lines) == 14 and lines[4] == "  0. '_________': TIE in 9" and lines[-1].endswith(": TIE in 0")
    out = io.StringIO()
    shuttle_py = os.path.join(REPO, "tests", "plugins", "shuttle.py")
    assert solver_launcher.run(parse([shuttle_py, "--loopy", "--line", "--find", "draw", "--find-cap", "64"]), out=out) == 0
    lines = out.getvalue().splitlines()
    assert lines[0] == "DRAW" and lines[1] == "Found 19 positions: draw" and lines[21] == "Line:"
    assert lines[22] == "  0. (0, 0): DRAW" and all(ln.endswith(": DRAW") for ln in lines[2:21] + lines[22:])


def test_solve_local_find_and_line(capsys):
    import solve_local
    solve_local.main([TTT_NP])
    plain = capsys.readouterr().out
    assert plain == "Tie\n"
    assert solve_local.main([TTT_NP, "--find", "tie:max", "--find", "win:5", "--line"]) == 0
    text = capsys.readouterr().out
    assert text.startswith(plain + "Found 1 positions: tie:9\n  " + EMPTY + ": TIE in 9\n")
    assert _blocks(text) == [("Found 1 positions: tie:9", 1), ("Found 122 positions: win:5", 16)]
    assert len([ln for ln in text[text.index("Line:\n"):].splitlines() if re.match(r"  \d+\. ", ln)]) == 10
    assert solve_local.main([TTT_NP, "--find", "nothing"]) == 2
    assert "unknown value" in capsys.readouterr().err


def test_launcher_find_under_torchrun_prints_one_block():
    import socket
    import subprocess
    import sys
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(REPO, "solver_launcher.py"),
           os.path.join(REPO, "test_games/four_to_one.py"), "--find", "loss"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=180,
                       env=dict(os.environ, PYTHONUNBUFFERED="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    roots = json.load(open(os.path.join(GOLDEN, "roots.json")))
    assert lines[0] == roots["four_to_one/four"]["canonical"]
    want_k, want_r = find.from_records(*golden("four_to_one_four"), "loss")
    assert lines[1] == "Found %d positions: loss" % len(want_k) and sum(ln.startswith("Found") for ln in lines) == 1
    from gamesmanmpi_amd.games import FourToOneCodec
    assert lines[2:] == ["  %r: LOSS in %d" % (FourToOneCodec().pos(int(k)), int(x) & 0x3FFF)
                         for k, x in zip(want_k, want_r)]
