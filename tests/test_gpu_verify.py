"""gm_verify on the device: a solved table checked against the game rules, for every engine and
every way a context holds a solve; gm_poke plants the errors it must find.

Clean solves report nothing.  A planted error is reported exactly as the CPU reference
(tests/verify_ref.py, built on oracle / golden tables and canonical.fold) reports the same
overlay: same class counts, same keys.  Errors are planted on interior positions only: the
device answers a primitive child from the rules without a lookup, as its backward pass does,
so a record planted on a leaf is seen at the leaf alone.
"""
import ctypes
import hashlib
import io
import json
import os

import numpy as np
import pytest

import canonical
import graph_ref
import verify_ref
from conftest import REPO, golden, load_plugin

pytestmark = pytest.mark.gpu

from gamesmanmpi_amd import Context, GMError, Solver, _lib, games  # noqa: E402

F2O, TTT, TOOT, OTH, SUB = 1, 2, 3, 4, 5
LOSS_IN_0 = 1 << 14
REMOVE = 0xFFFF
BOX_ROOT = 0x000F0FFF
DAG = (2000, 12, 5, True, (1, 1, 1), 11)
CLASSES = _lib.Verify.CLASSES


def _solve(game, params=(), root=None, engine=None, **opts):
    ctx = Context(game, params, device=0)
    if engine is not None:
        ctx.set_option(_lib.OPT_ENGINE, engine)
    for k, v in opts.items():
        ctx.set_option(getattr(_lib, "OPT_" + k.upper()), v)
    root = ctx.initial() if root is None else root
    n, rec = ctx.solve(root)
    return ctx, n, root, rec


def _assert_clean(ctx, n):
    res, keys = ctx.verify()
    st = ctx.stats()
    assert {c: res[c] for c in CLASSES} == {c: 0 for c in CLASSES} and res["n_bad"] == 0 and keys == []
    assert res["root_ok"] == 1
    assert res["checked"] == (st["n_stored"] or n)
    assert res["child_lookups"] > 0
    return res


def _endgame_solver(ranks=1):
    s = Solver(load_plugin("tests/plugins/othello8_endgame.py"), device=0)
    if ranks > 1:
        s.ctx.set_option(_lib.OPT_VIRTUAL_RANKS, ranks)
    n, rec = s.solve()
    return s, n, rec


def _blake(pos):
    return int.from_bytes(hashlib.blake2b(pos.encode("ISO-8859-1"), digest_size=8).digest(), "big")


# ---------------------------------------------------------------- clean solves
@pytest.mark.parametrize("engine", [_lib.ENGINE_DENSE, _lib.ENGINE_SPARSE])
def test_clean_ttt(engine):
    ctx, n, _, _ = _solve(TTT, engine=engine)
    assert _assert_clean(ctx, n)["checked"] == 5478
    ctx.close()


def test_clean_four_to_one_root_6():
    ctx, n, _, _ = _solve(F2O, root=6)
    assert _assert_clean(ctx, n)["checked"] == 8
    ctx.close()


@pytest.mark.parametrize("sym", [1, 0])
def test_clean_toot_4x3(sym):
    ctx, n, _, _ = _solve(TOOT, (4, 3), symmetry=sym)
    res = _assert_clean(ctx, n)
    assert n == 200127 and (res["checked"] < n) == bool(sym)
    ctx.close()


@pytest.mark.parametrize("ranks", [1, 4])
@pytest.mark.parametrize("sym", [1, 0])
def test_clean_othello_4x4(sym, ranks):
    ctx, n, _, _ = _solve(OTH, (4, 4), symmetry=sym, virtual_ranks=ranks)
    res = _assert_clean(ctx, n)
    assert n == 54089 and (res["checked"] < n) == bool(sym)
    ctx.close()


@pytest.mark.parametrize("ranks", [1, 8])
def test_clean_othello_8x8_endgame(ranks):
    s, n, _ = _endgame_solver(ranks)
    assert s.ctx.words == 3 and n == 56552
    res, keys = s.verify()
    assert res["n_bad"] == 0 and keys == [] and res["root_ok"] == 1 and res["checked"] == n
    assert res["child_lookups"] > 0
    s.close()


@pytest.mark.parametrize("interleave", [1, 6, 10])
@pytest.mark.parametrize("heaps", [3, 5])
def test_clean_subtract_block_engine(heaps, interleave):
    ctx, n, _, _ = _solve(SUB, (heaps,), sub_interleave=interleave)
    assert _assert_clean(ctx, n)["checked"] == 16 ** heaps
    ctx.close()


@pytest.mark.parametrize("opts", [{}, {"virtual_ranks": 2}, {"virtual_ranks": 4}, {"virtual_ranks": 8},
                                  {"sub_interleave": 10, "virtual_ranks": 4}],
                         ids=["one", "split2", "split4", "split8", "dist_sub4"])
@pytest.mark.parametrize("root", [0x00000003, BOX_ROOT, 0x33557777])
def test_clean_box_engine(root, opts):
    ctx, n, _, _ = _solve(SUB, (8,), root=root, **opts)
    region = 1
    for j in range(8):
        region *= ((root >> (4 * j)) & 15) + 1
    assert ctx.stats()["engine"] == (_lib.ENGINE_DIST_DENSE if opts else _lib.ENGINE_DENSE)
    assert _assert_clean(ctx, n)["checked"] == region == n
    ctx.close()


def test_clean_full_2_32():
    ctx, n, _, _ = _solve(SUB, (8,))
    res = _assert_clean(ctx, n)
    assert res["checked"] == 1 << 32
    # every position but the empty one looks up each child that is not the empty position
    assert res["child_lookups"] > 1 << 35
    ctx.close()


def test_clean_random_dag():
    prim, off, kids = graph_ref.random_dag(*DAG)
    ctx = Context(_lib.GAME_GRAPH, (), device=0)
    n, _ = ctx.solve_graph(prim, off, kids)
    res = _assert_clean(ctx, n)
    assert res["checked"] == 2000 and res["child_lookups"] == len(kids)
    ctx.close()


def test_clean_graph_plugin_nim3():
    s = Solver(load_plugin("tests/plugins/nim3.py"), device=0, graph=True)
    s.solve()
    res, keys = s.verify()
    assert res["n_bad"] == 0 and keys == [] and res["root_ok"] == 1
    assert res["checked"] == len(s.codec.prim) and res["child_lookups"] == len(s.codec.kids)
    s.close()


# ---------------------------------------------------------------- references, built once
class Held:
    """A solved context with what a test needs beside it."""

    def __init__(self, ctx, root, rec, resolve, keep=None):
        self.ctx, self.root, self.rec, self.resolve, self.keep = ctx, root, rec, resolve, keep

    def close(self):
        (self.keep or self.ctx).close()


@pytest.fixture(scope="module")
def refs(oracle):
    cache = {}

    def table(name):
        if name in cache:
            return cache[name]
        if name == "ttt":
            k, r = golden("ttt")
            ref = verify_ref.VerifyRef(k, r, lambda key: oracle.expand(TTT, (), key))
        elif name == "f2o":
            k, r = golden("four_to_one_six")
            ref = verify_ref.VerifyRef(k, r, lambda key: oracle.expand(F2O, (), key))
        elif name == "toot43":
            k, r = golden("toot_4x3")
            ref = verify_ref.VerifyRef(k, r, lambda key: oracle.expand(TOOT, (4, 3), key))
        elif name == "oth44":
            k, r = golden("othello_4x4")
            ref = verify_ref.VerifyRef(k, r, lambda key: oracle.expand(OTH, (4, 4), key))
        elif name == "sub3":
            r = oracle.subtract_dense(3)
            ref = verify_ref.VerifyRef(range(len(r)), r, lambda key: oracle.expand(SUB, (3,), key))
        elif name == "box":
            k, r = oracle.solve(SUB, (8,), BOX_ROOT)
            ref = verify_ref.VerifyRef(k, r, lambda key: oracle.expand(SUB, (8,), key))
        elif name == "dag":
            prim, off, kids = graph_ref.random_dag(*DAG)
            r = graph_ref.solve_reference(prim, off, kids)
            ref = verify_ref.VerifyRef(range(len(r)), r,
                                       lambda key: (prim[key], kids[int(off[key]):int(off[key + 1])]))
        elif name == "end8":
            # the full keys come from a device export whose records are the reference plugin's
            # (golden, keyed by a hash of the position string); the moves are the host twin's
            s, n, _ = _endgame_solver()
            k, r = s.table()
            keys = [_lib.words_to_int(w) for w in k.tolist()]
            gk, gr = golden("othello_8x8_endgame")
            assert {_blake(s.codec.pos(x)): int(y) for x, y in zip(keys, r)} == dict(zip(gk.tolist(), gr.tolist()))
            host = games.HostDescriptor(s.codec)
            ref = verify_ref.VerifyRef(keys, r, host.expand)
            ref.offenders()   # expands every key while the descriptor is open
            host.close()
            s.close()
        else:
            raise KeyError(name)
        assert ref.offenders() == {}
        cache[name] = ref
        return ref

    return table


def _open(case):
    """case -> Held: a fresh solve of the case's game on its engine."""
    if case in ("ttt_sparse", "ttt_dense"):
        eng = _lib.ENGINE_SPARSE if case == "ttt_sparse" else _lib.ENGINE_DENSE
        ctx, n, root, rec = _solve(TTT, engine=eng)
        return Held(ctx, root, rec, lambda: ctx.solve(root))
    if case == "end8":
        s, n, rec = _endgame_solver()
        return Held(s.ctx, s.root_key, rec, s.solve, keep=s)
    if case == "dag":
        g = graph_ref.random_dag(*DAG)
        ctx = Context(_lib.GAME_GRAPH, (), device=0)
        _, rec = ctx.solve_graph(*g)
        return Held(ctx, 0, rec, lambda: ctx.solve_graph(*g))
    game, params, root, opts = {
        "f2o": (F2O, (), 6, {}),
        "toot43": (TOOT, (4, 3), None, {"symmetry": 0}),
        "toot43_sym": (TOOT, (4, 3), None, {}),
        "oth44_sym": (OTH, (4, 4), None, {}),
        "oth44_ranks4": (OTH, (4, 4), None, {"symmetry": 0, "virtual_ranks": 4}),
        "sub3": (SUB, (3,), None, {}),
        "box": (SUB, (8,), BOX_ROOT, {}),
        "box_split4": (SUB, (8,), BOX_ROOT, {"virtual_ranks": 4}),
        "dist_sub4": (SUB, (8,), BOX_ROOT, {"sub_interleave": 10, "virtual_ranks": 4}),
    }[case]
    ctx, n, root, rec = _solve(game, params, root=root, **opts)
    return Held(ctx, root, rec, lambda: ctx.solve(root))


REF_OF = {"ttt_sparse": "ttt", "ttt_dense": "ttt", "f2o": "f2o", "toot43": "toot43", "sub3": "sub3", "box": "box",
          "end8": "end8", "dag": "dag", "box_split4": "box", "oth44_ranks4": "oth44"}


def _pick(ref, root):
    """A deterministic interior position from the middle of the sorted keys on, not the root,
    with a parent that is not already WIN in 1 (which a planted LOSS in 0 must change)."""
    keys = sorted(ref.table)
    for k in keys[len(keys) // 2:] + keys[:len(keys) // 2]:
        if k == root or ref.expand(k)[0] != canonical.UNDECIDED:
            continue
        if any(ref.table[p] != 1 for p in ref.parents(k)):
            return k
    raise AssertionError("no position to plant an error on")


# ---------------------------------------------------------------- planted errors, exact
@pytest.mark.parametrize("case", ["ttt_sparse", "ttt_dense", "f2o", "toot43", "sub3", "box", "end8", "dag"])
def test_planted_loss_in_0_is_reported_as_the_reference_reports_it(refs, case):
    ref = refs(REF_OF[case])
    h = _open(case)
    key = _pick(ref, h.root)
    want = ref.offenders({key: LOSS_IN_0})
    assert len(want) >= 2 and key in want
    h.ctx.poke(key, LOSS_IN_0)
    res, keys = h.ctx.verify(cap=len(want) + 64)
    print(case, hex(key), res)
    assert {c: res[c] for c in CLASSES} == verify_ref.counts(want)
    assert keys == sorted(want) and res["n_bad"] == len(want)
    assert h.ctx.query([key])[0] == LOSS_IN_0
    assert res["root_ok"] == 1 and res["checked"] == len(ref.table)
    h.resolve()                                                          # the next solve rewrites every table
    res, keys = h.ctx.verify()
    assert res["n_bad"] == 0 and keys == [] and res["root_ok"] == 1
    h.close()


# ---------------------------------------------------------------- the root
def _other_value(rec):
    v, r = rec >> 14, rec & 0x3FFF
    return ((1 - v if v < 2 else 0) << 14) | r


@pytest.mark.parametrize("case", ["ttt_sparse", "ttt_dense", "f2o", "toot43_sym", "oth44_sym", "oth44_ranks4", "end8",
                                  "sub3", "box", "box_split4", "dist_sub4", "dag"])
def test_poked_root_fails_the_root_check_alone(case):
    h = _open(case)
    h.ctx.poke(h.root, _other_value(h.rec))
    res, keys = h.ctx.verify()
    assert res["root_ok"] == 0 and keys == [h.root] and res["n_bad"] == 1 and res["bad_value"] == 1
    h.ctx.poke(h.root, h.rec)
    res, keys = h.ctx.verify()
    assert res["root_ok"] == 1 and keys == [] and res["n_bad"] == 0
    h.close()


# ---------------------------------------------------------------- a position removed
@pytest.mark.parametrize("case", ["ttt_sparse", "end8", "sub3"])
def test_removed_position_is_missed_by_every_parent(refs, case):
    ref = refs(REF_OF[case])
    h = _open(case)
    key = _pick(ref, h.root)
    parents = set(ref.parents(key))
    assert parents
    h.ctx.poke(key, REMOVE)
    assert h.ctx.query([key])[0] == REMOVE
    res, keys = h.ctx.verify(cap=len(ref.table))
    print(case, hex(key), res)
    assert len(keys) == res["n_bad"] and parents <= set(keys)
    stored = sorted(ref.table)
    gone = {k for k, r in zip(stored, h.ctx.query(stored)) if r == REMOVE}   # the key, and keys whose probe chain it cut
    assert key in gone
    allowed = parents | gone | {p for g in gone for p in ref.parents(g)}
    assert set(keys) <= allowed
    assert res["missing_child"] >= len(parents) and res["root_ok"] == 1
    if case == "sub3":
        assert gone == {key} and res["misplaced"] == 0                   # a dense slot has no chain to cut
    h.resolve()
    assert h.ctx.verify()[0]["n_bad"] == 0
    h.close()


# ---------------------------------------------------------------- split engines
@pytest.mark.parametrize("case", ["box_split4", "oth44_ranks4"])
def test_split_engines_report_a_poked_position(refs, case):
    """Which copy of a halo box a parent read depends on the split, so the set is not pinned."""
    ref = refs(REF_OF[case])
    h = _open(case)
    assert h.ctx.stats()["world"] == 4
    key = _pick(ref, h.root)
    h.ctx.poke(key, LOSS_IN_0)
    res, keys = h.ctx.verify(cap=4096)
    assert res["n_bad"] >= 1 and key in keys and h.ctx.query([key])[0] == LOSS_IN_0
    assert set(keys) <= set(ref.offenders({key: LOSS_IN_0}))
    h.close()


# ---------------------------------------------------------------- the call's contract
def _raw(ctx, buf, cap):
    out, n_bad = _lib.Verify(), ctypes.c_uint64(0)
    rc = ctx.L.gm_verify(ctx.h, ctypes.byref(out), buf.ctypes.data if buf is not None else None, cap,
                         ctypes.byref(n_bad))
    return rc, out.as_dict(), n_bad.value


def test_call_contract(refs):
    ref = refs("ttt")
    ctx, n, root, _ = _solve(TTT, engine=_lib.ENGINE_SPARSE)
    key = _pick(ref, root)
    want = ref.offenders({key: LOSS_IN_0})
    assert len(want) >= 3
    ctx.poke(key, LOSS_IN_0)
    full, keys = ctx.verify(cap=64)
    assert keys == sorted(want)
    cap = len(want) - 1
    buf = np.full(cap + 2, 0xABCD, dtype=np.uint64)
    rc, res, n_bad = _raw(ctx, buf, cap)                                 # a short list: any cap of them
    assert rc == 0 and res == full and n_bad == len(want)
    assert len(set(buf[:cap].tolist())) == cap and set(buf[:cap].tolist()) <= set(want)
    assert buf[cap:].tolist() == [0xABCD, 0xABCD]
    assert _raw(ctx, None, 64) == (0, full, len(want))                   # NULL list: the counts only
    assert _raw(ctx, buf, 0) == (0, full, len(want))
    assert ctx.L.gm_verify(ctx.h, None, None, 0, None) == -1             # GM_E_ARG: out == NULL
    out = _lib.Verify()
    assert ctx.L.gm_verify(ctx.h, ctypes.byref(out), None, 0, None) == 0   # n_bad is optional
    with pytest.raises(GMError, match="GM_E_KEY"):
        ctx.poke(19683, 0)                                               # no position
    with pytest.raises(GMError, match="GM_E_KEY"):
        ctx.poke(1 + 3, 0)                                               # X X on an empty board: valid, not reachable
    ctx.close()


def test_verify_after_a_failed_graph_solve():
    ctx = Context(_lib.GAME_GRAPH, (), device=0)
    ctx.solve_graph(*graph_ref.chain(5, 1))
    assert ctx.verify()[0]["n_bad"] == 0
    prim = np.array([4, 4], dtype=np.uint8)
    with pytest.raises(GMError):
        ctx.solve_graph(prim, np.array([0, 1, 2], dtype=np.uint64), np.array([1, 0], dtype=np.uint32))   # a cycle
    with pytest.raises(GMError, match="GM_E_STATE"):
        ctx.verify()
    with pytest.raises(GMError, match="GM_E_STATE"):
        ctx.poke(0, 0)
    ctx.close()


def test_poke_drops_a_kept_histogram(refs):
    ref = refs("ttt")
    ctx, n, root, _ = _solve(TTT, engine=_lib.ENGINE_SPARSE)
    before = ctx.histogram()
    n_rem, cnt = ctypes.c_int(), ctypes.c_uint64()
    assert ctx.L.gm_histogram(ctx.h, None, 0, ctypes.byref(n_rem), ctypes.byref(cnt)) == 0   # kept for the fill
    key = _pick(ref, root)
    v, r = verify_ref.split(ref.table[key])
    ctx.poke(key, LOSS_IN_0)
    after = np.zeros((3, n_rem.value), dtype=np.uint64)
    assert ctx.L.gm_histogram(ctx.h, after.ctypes.data, n_rem.value, ctypes.byref(n_rem), ctypes.byref(cnt)) == 0
    want = before.copy()
    want[v, r] -= 1
    want[1, 0] += 1
    assert np.array_equal(after, want) and not np.array_equal(after, before)
    ctx.close()


# ---------------------------------------------------------------- moves
def _check_moves(s, mod, positions, record_of):
    """Solver.moves at each position: the plugin's children in its order, the golden records,
    and a chosen child whose record reduces to the parent's."""
    seen_interior = seen_leaf = 0
    for pos in positions:
        rows, best = s.moves(pos)
        if mod.primitive(pos) != canonical.UNDECIDED:
            assert rows == [] and best is None
            seen_leaf += 1
            continue
        seen_interior += 1
        moves = list(mod.gen_moves(pos))
        assert [row[0] for row in rows] == moves
        assert [row[1] for row in rows] == [mod.do_move(pos, m) for m in moves]
        assert [(row[2] << 14) | row[3] for row in rows] == [record_of(row[1]) for row in rows]
        assert best in rows
        assert canonical.fold([best[2:]]) == verify_ref.split(record_of(pos))
        assert canonical.fold([row[2:] for row in rows]) == verify_ref.split(record_of(pos))
    assert seen_interior and seen_leaf


def _sample(keys, n=200):
    return [int(k) for k in keys[::max(1, len(keys) // n)][:n]]


def test_moves_ttt():
    mod = load_plugin("test_games/mttt.py")
    s = Solver(mod, device=0)
    s.solve()
    keys, recs = golden("ttt")
    table = dict(zip(keys.tolist(), recs.tolist()))
    _check_moves(s, mod, [s.codec.pos(k) for k in _sample(keys)], lambda p: table[s.codec.key(p)])
    kids, krecs, best = s.ctx.moves(0)
    assert len(kids) == 9 == len(krecs) and best == 0                    # every first move ties: the first is played
    leaf = s.ctx.moves(0x4c68)
    assert leaf[0] == [] and len(leaf[1]) == 0 and leaf[2] is None       # a finished game: no moves
    s.close()


def test_moves_othello_4x4_default_symmetry():
    mod = load_plugin("test_games/othello_bit_new.py", length=4, height=4, area=16)
    s = Solver(mod, device=0)
    n, _ = s.solve()
    assert s.ctx.stats()["n_stored"] < n                                 # children are looked up by representative
    keys, recs = golden("othello_4x4")
    table = dict(zip(keys.tolist(), recs.tolist()))
    _check_moves(s, mod, [s.codec.pos(k) for k in _sample(keys)], lambda p: table[s.codec.key(p)])
    s.close()


def test_moves_othello_8x8_endgame():
    s, n, _ = _endgame_solver()
    mod = s.module
    gk, gr = golden("othello_8x8_endgame")
    table = dict(zip(gk.tolist(), gr.tolist()))
    k, _ = s.table()
    positions = [s.codec.pos(_lib.words_to_int(w)) for w in k[::len(k) // 200][:200].tolist()]
    _check_moves(s, mod, positions, lambda p: table[_blake(p)])
    s.close()


# ---------------------------------------------------------------- command lines
def test_launcher_verify_flag(tmp_path):
    import solver_launcher
    game = os.path.join(REPO, "test_games/tic_tac_toe_np.py")
    plain = io.StringIO()
    assert solver_launcher.run(solver_launcher.build_parser().parse_args([game]), out=plain) == 0
    out = io.StringIO()
    args = solver_launcher.build_parser().parse_args([game, "--verify", "-sd", str(tmp_path)])
    assert solver_launcher.run(args, out=out) == 0
    lines = out.getvalue().splitlines()
    assert lines[0] + "\n" == plain.getvalue()
    assert lines[1:] == ["Verified 5478 positions: consistent"]
    j = json.load(open(tmp_path / "stats" / "verify.json"))
    assert j["consistent"] is True and j["checked"] == 5478 and j["n_bad"] == 0 and j["root_ok"] == 1
    assert j["offenders"] == []


def test_solve_local_verify_flag(capsys):
    import solve_local
    game = os.path.join(REPO, "test_games/tic_tac_toe_np.py")
    assert solve_local.main([game]) == 0
    plain = capsys.readouterr().out
    assert solve_local.main([game, "--verify"]) == 0
    got = capsys.readouterr().out
    assert got == plain + "Verified 5478 positions: consistent\n"


def test_report_of_an_inconsistent_table(refs):
    """The lines --verify prints when the check fails, and its non-zero verdict."""
    from gamesmanmpi_amd import verify
    ref = refs("ttt")
    mod = load_plugin("test_games/mttt.py")
    s = Solver(mod, device=0)
    s.solve()
    key = _pick(ref, s.root_key)
    want = ref.offenders({key: LOSS_IN_0})
    s.ctx.poke(key, LOSS_IN_0)
    out = io.StringIO()
    assert verify.report(s, out) is False
    lines = out.getvalue().splitlines()
    assert lines[0] == ("Verified 5478 positions: %d inconsistent (bad_key 0, misplaced 0, bad_primitive 0, "
                        "missing_child 0, bad_value %d)" % (len(want), len(want)))
    assert sum(ln.startswith("  ") and not ln.startswith("    ") for ln in lines[1:]) == len(want)
    assert any(repr(s.codec.pos(key)) in ln and "LOSS in 0" in ln for ln in lines[1:])
    s.close()


# ---------------------------------------------------------------- two processes
def test_two_processes_refuse():
    import socket
    from mp_ranks import run_ranks
    from verify_ranks import rank_main
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    res = run_ranks(rank_main, 2, (OTH, (4, 4), {"sparse_transport": 1}), timeout=240)
    assert [r["rc"] for r in res] == [-5, -5] and [r["rc_poke"] for r in res] == [-5, -5]
    assert all("2-process" in r["msg"] for r in res)
    assert all(r["n"] == 54089 and 0 < r["m"] < 54089 for r in res) and sum(r["m"] for r in res) == 54089
