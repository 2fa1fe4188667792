"""gm_histogram on the device: positions by value and remoteness, counted in one pass over the
solved table (csrc/hist_common.hpp), for every engine and every way a context holds a solve.

Expected arrays always come from `analysis.from_records` over golden or C-oracle records,
never from the device's own export (the one exception is named in its test); every case also
checks hist.sum() == gm_digest's count == n_positions.
"""
import ctypes
import io
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, REPO, golden, load_plugin

pytestmark = pytest.mark.gpu

from gamesmanmpi_amd import Context, GMError, Solver, _lib, analysis  # noqa: E402

F2O, TTT, TOOT, OTH, SUB = 1, 2, 3, 4, 5


def _solve(game, params=(), root=None, engine=None, **opts):
    ctx = Context(game, params, device=0)
    if engine is not None:
        ctx.set_option(_lib.OPT_ENGINE, engine)
    for k, v in opts.items():
        ctx.set_option(getattr(_lib, "OPT_" + k.upper()), v)
    n, rec = ctx.solve(ctx.initial() if root is None else root)
    return ctx, n


def _check(ctx, n, want):
    """The context's histogram equals `want`, and its sum the digest's count and n."""
    h = ctx.histogram()
    assert h.dtype == np.uint64 and h.shape == want.shape, (h.shape, want.shape)
    assert np.array_equal(h, want)
    assert int(h.sum()) == ctx.digest()[1] == n
    ctx.close()


@pytest.fixture(scope="module")
def sub7(oracle):
    """The 7-heap oracle table as a (16,) * 7 array, heap 6 first (heap 7 of a root below 16^7 is 0)."""
    return oracle.subtract_dense_mt(7).reshape((16,) * 7)


def _region(table, root, heaps):
    """The records of the root's region: every heap at most the root's (a mask by slicing)."""
    return table[tuple(slice(0, ((root >> (4 * j)) & 15) + 1) for j in reversed(range(heaps)))]


# ---------------------------------------------------------------- small games
@pytest.mark.parametrize("engine", [_lib.ENGINE_DENSE, _lib.ENGINE_SPARSE])
def test_ttt(engine):
    ctx, n = _solve(TTT, engine=engine)
    _check(ctx, n, analysis.from_records(golden("ttt")[1]))


def test_four_to_one_root_6():
    ctx, n = _solve(F2O, root=6)
    _check(ctx, n, analysis.from_records(golden("four_to_one_six")[1]))


# ---------------------------------------------------------------- orbit weights, virtual ranks
@pytest.mark.parametrize("ranks", [1, 4])
@pytest.mark.parametrize("sym", [1, 0])
def test_othello_4x4_orbits_and_virtual_ranks(sym, ranks):
    ctx, n = _solve(OTH, (4, 4), symmetry=sym, virtual_ranks=ranks)
    st = ctx.stats()
    assert (st["n_stored"] < n) == bool(sym) and n == 54089
    _check(ctx, n, analysis.from_records(golden("othello_4x4")[1]))


@pytest.mark.parametrize("sym", [1, 0])
def test_toot_4x3_orbits(sym):
    ctx, n = _solve(TOOT, (4, 3), symmetry=sym)
    _check(ctx, n, analysis.from_records(golden("toot_4x3")[1]))


def test_toot_4x4_vs_oracle(oracle):
    keys, recs = oracle.solve(TOOT, (4, 4))
    ctx, n = _solve(TOOT, (4, 4), symmetry=1)
    assert ctx.stats()["n_stored"] < n == len(keys)
    _check(ctx, n, analysis.from_records(recs))


# ---------------------------------------------------------------- 128-bit keys, 32-byte slots
@pytest.mark.parametrize("ranks", [1, 8])
def test_othello_8x8_endgame_10(ranks):
    mod = load_plugin("tests/plugins/othello8_endgame.py")
    s = Solver(mod, device=0)
    assert s.ctx.words == 3
    if ranks > 1:
        s.ctx.set_option(_lib.OPT_VIRTUAL_RANKS, ranks)
    n, rec = s.solve()
    want = analysis.from_records(golden("othello_8x8_endgame")[1])
    assert n == 56552 and np.array_equal(s.analysis(), want)
    _check(s.ctx, n, want)


# ---------------------------------------------------------------- block engine
@pytest.mark.parametrize("interleave", [1, 6, 10])
@pytest.mark.parametrize("heaps", [3, 5])
def test_subtract_block_engine(oracle, heaps, interleave):
    ctx, n = _solve(SUB, (heaps,), sub_interleave=interleave)
    _check(ctx, n, analysis.from_records(oracle.subtract_dense(heaps)))


# ---------------------------------------------------------------- box engine, 8 heaps
@pytest.mark.parametrize("root", [0x00000003, 0x000F0FFF, 0x12345678, 0x0FFFFFFF])
def test_box_engine_custom_roots(oracle, sub7, root):
    """One box; unaligned nibbles in the quarter and the half heaps; 2^28 positions whose
    interior chunks skip the region mask.  The 7-heap oracle table holds the regions of roots
    below 16^7; 0x12345678 has a stone on heap 7, so its region comes from the generic oracle."""
    ctx, n = _solve(SUB, (8,), root=root)
    want = analysis.from_records(_region(sub7, root, 7) if root < 16 ** 7 else oracle.solve(SUB, (8,), root)[1])
    region = 1
    for j in range(8):
        region *= ((root >> (4 * j)) & 15) + 1
    assert n == region == int(want.sum())
    _check(ctx, n, want)


@pytest.fixture(scope="module")
def root_3355(oracle):
    keys, recs = oracle.solve(SUB, (8,), root=0x33557777)
    return len(keys), analysis.from_records(recs)


@pytest.mark.parametrize("opts", [{}, {"virtual_ranks": 2}, {"virtual_ranks": 4}, {"virtual_ranks": 8},
                                  {"sub_interleave": 10, "virtual_ranks": 4}],
                         ids=["one", "split2", "split4", "split8", "dist_sub4"])
def test_box_engine_split_and_dist_sub(root_3355, opts):
    ctx, n = _solve(SUB, (8,), root=0x33557777, **opts)
    assert n == root_3355[0]
    want_engine = _lib.ENGINE_DIST_DENSE if opts else _lib.ENGINE_DENSE
    assert ctx.stats()["engine"] == want_engine
    _check(ctx, n, root_3355[1])


def test_full_2_32():
    ref = json.load(open(os.path.join(GOLDEN, "histograms.json")))["subtract_8"]
    want = np.array([ref["win"], ref["loss"], ref["tie"]], dtype=np.uint64)
    ctx, n = _solve(SUB, (8,))
    assert n == 1 << 32 and want.shape[1] == 81
    _check(ctx, n, want)


# ---------------------------------------------------------------- the call's contract
def _raw(ctx, counts, cap):
    n_rem, n = ctypes.c_int(-1), ctypes.c_uint64(0)
    rc = ctx.L.gm_histogram(ctx.h, counts.ctypes.data if counts is not None else None, cap, ctypes.byref(n_rem),
                            ctypes.byref(n))
    return rc, n_rem.value, n.value


def test_call_contract():
    want = analysis.from_records(golden("ttt")[1])
    ctx = Context(TTT, (), device=0)
    assert _raw(ctx, None, 0)[0] == -5                                   # GM_E_STATE before a solve
    with pytest.raises(GMError, match="GM_E_STATE"):
        ctx.histogram()
    n, _ = ctx.solve(ctx.initial())
    depth = want.shape[1]
    assert _raw(ctx, None, 0) == (0, depth, n)                           # NULL: n_rem and n only
    short = np.full((3, depth - 1), 7, dtype=np.uint64)
    assert _raw(ctx, short, depth - 1) == (-8, depth, n)                 # GM_E_CAP, n_rem still set
    assert _raw(ctx, short, depth - 1) == (-8, depth, n)                 # (also without a query before it)
    wide = np.full((3, depth + 5), 7, dtype=np.uint64)
    assert _raw(ctx, wide, depth + 5) == (0, depth, n)
    assert np.array_equal(wide[:, :depth], want) and not wide[:, depth:].any()
    exact = np.full((3, depth), 7, dtype=np.uint64)
    assert _raw(ctx, None, 0) == (0, depth, n) and _raw(ctx, exact, depth) == (0, depth, n)
    assert np.array_equal(exact, want)
    ctx.close()


def test_second_solve_replaces_the_histogram():
    """Another root on the same context, then the first again (a sparse replay): the histogram
    is always the last solve's, also when a query of the solve before was left unfilled."""
    six = analysis.from_records(golden("four_to_one_six")[1])
    four = analysis.from_records(golden("four_to_one_four")[1])
    ctx = Context(F2O, (), device=0)
    for root, want in ((6, six), (4, four), (6, six), (6, six)):
        n, _ = ctx.solve(root)
        assert np.array_equal(ctx.histogram(), want) and int(want.sum()) == n == ctx.digest()[1]
        assert _raw(ctx, None, 0)[0] == 0                                # a query the next solve must drop
    ctx.close()


# ---------------------------------------------------------------- graph engine
def test_graph_chain_takes_the_global_bins():
    """5,000 nodes, node i -> i + 1, the last a LOSS primitive: the remoteness reaches 4,999,
    past the 4,096 bins per value that fit the score kernels' LDS budget, so the census is
    taken with global bins."""
    n = 5000
    prim = np.full(n, 4, dtype=np.uint8)
    prim[-1] = 1
    off = np.minimum(np.arange(n + 1), n - 1).astype(np.uint64)
    kids = np.arange(1, n, dtype=np.uint32)
    ctx = Context(_lib.GAME_GRAPH, (), device=0)
    ctx.solve_graph(prim, off, kids)
    want = np.zeros((3, n), dtype=np.uint64)
    want[1, 0::2] = 1    # even distance from the end: LOSS
    want[0, 1::2] = 1
    _check(ctx, n, want)


def test_graph_plugin_nim3():
    """No golden table for this plugin: the graph engine's export is pinned to the canonical
    oracle by tests/test_graph.py, and the census must agree with it."""
    s = Solver(load_plugin("tests/plugins/nim3.py"), device=0, graph=True)
    n, _ = s.solve()
    want = analysis.from_records(s.table()[1])
    assert np.array_equal(s.analysis(), want)
    _check(s.ctx, n, want)


def test_graph_plugin_with_symmetry_is_weighted_by_orbit():
    s = Solver(load_plugin("tests/plugins/ttt_symmetric.py"), device=0, graph=True)
    n, _ = s.solve()
    h = s.analysis()
    assert n == 5478 == int(h.sum()) and np.array_equal(h, analysis.from_records(golden("ttt")[1]))
    assert int(s.ctx.histogram().sum()) == 765 == s.ctx.digest()[1]      # the device counts nodes
    s.close()


# ---------------------------------------------------------------- processes
def _run_ranks(world, game, params, opts):
    import socket
    from hist_ranks import rank_main
    from mp_ranks import run_ranks
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    return run_ranks(rank_main, world, (game, params, opts), timeout=240)


def _summed(res):
    parts = [np.array(r["hist"], dtype=np.uint64).reshape(3, -1) for r in res]
    for r, p in zip(res, parts):
        assert int(p.sum()) == r["m"]                                    # each rank: its digest count
    depth = max(p.shape[1] for p in parts)
    return sum(analysis.pad(p, depth) for p in parts)


def test_two_processes_sparse_ipc():
    res = _run_ranks(2, OTH, (4, 4), {"sparse_transport": 1})
    want = analysis.from_records(golden("othello_4x4")[1])
    assert all(r["n"] == 54089 and 0 < r["m"] < 54089 for r in res)
    assert np.array_equal(_summed(res), want)


def test_two_processes_box_ipc(root_3355):
    res = _run_ranks(2, SUB, (8,), {"box_transport": 1, "root": 0x33557777})
    assert all(r["n"] == root_3355[0] and 0 < r["m"] < root_3355[0] for r in res)
    assert np.array_equal(_summed(res), root_3355[1])


# ---------------------------------------------------------------- command lines
def _table_of(lines):
    return analysis.parse_table("\n".join(lines))


def test_launcher_analysis_flag(tmp_path):
    import solver_launcher
    game = os.path.join(REPO, "test_games/tic_tac_toe_np.py")
    want = analysis.from_records(golden("ttt_np")[1])
    plain = io.StringIO()
    assert solver_launcher.run(solver_launcher.build_parser().parse_args([game]), out=plain) == 0
    assert plain.getvalue().count("\n") == 1                             # without the flag: the root line only
    out = io.StringIO()
    assert solver_launcher.run(solver_launcher.build_parser().parse_args([game, "--analysis"]), out=out) == 0
    lines = out.getvalue().splitlines()
    assert lines[0] + "\n" == plain.getvalue()
    h = _table_of(lines[1:])
    assert int(h.sum()) == 5478 and np.array_equal(h, want)
    out = io.StringIO()
    args = solver_launcher.build_parser().parse_args([game, "--analysis", "-sd", str(tmp_path)])
    assert solver_launcher.run(args, out=out) == 0
    j = json.load(open(tmp_path / "stats" / "analysis.json"))
    assert [j["win_by_remoteness"], j["loss_by_remoteness"], j["tie_by_remoteness"]] == want.tolist()
    assert j["positions"] == 5478 and j == analysis.as_json(_table_of(out.getvalue().splitlines()[1:]))


def test_solve_local_analysis_flag(capsys):
    import solve_local
    game = os.path.join(REPO, "test_games/tic_tac_toe_np.py")
    solve_local.main([game])
    plain = capsys.readouterr().out
    solve_local.main([game, "--analysis"])
    got = capsys.readouterr().out
    assert got.startswith(plain) and plain.count("\n") == 1
    assert np.array_equal(_table_of(got.splitlines()[1:]), analysis.from_records(golden("ttt_np")[1]))


def test_launcher_analysis_under_torchrun_prints_one_table():
    import socket
    import subprocess
    import sys
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(REPO, "solver_launcher.py"),
           os.path.join(REPO, "test_games/four_to_one.py"), "--analysis"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=180,
                       env=dict(os.environ, PYTHONUNBUFFERED="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    roots = json.load(open(os.path.join(GOLDEN, "roots.json")))
    assert lines[0] == roots["four_to_one/four"]["canonical"]
    assert sum(ln.split()[:1] == ["Remoteness"] for ln in lines) == 1
    assert np.array_equal(_table_of(lines[1:]), analysis.from_records(golden("four_to_one_four")[1]))
