"""Connect (k in a row with gravity, games.hpp DescConnect) on the device against the fixtures of
tests/golden/make_connect_golden.py (the plugin test_games/connect4.py solved on the CPU by
oracle/canonical.py): whole tables on the small boards, summaries on 4x5 / 5x4 and on custom
roots of the standard 7x6 board and of 9x6 (63 key bits), the mirror reduction, virtual ranks,
every table reader, and the launcher."""
import io
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_plugin

sys.path.insert(0, GOLDEN)
import make_connect_golden as mcg  # noqa: E402

pytestmark = pytest.mark.gpu

from gamesmanmpi_amd import Context, GMError, _lib  # noqa: E402
from gamesmanmpi_amd.solver import best_move  # noqa: E402

PLUGIN = os.path.join(REPO, "test_games/connect4.py")
CONNECT = _lib.GAME_CONNECT
UNDECIDED = 4
J = mcg.load_json()


def solve(dims, root=None, **opts):
    ctx = Context(CONNECT, dims, device=0)
    for k, v in opts.items():
        ctx.set_option(getattr(_lib, "OPT_" + k.upper()), v)
    root = ctx.initial() if root is None else root
    n, rec = ctx.solve(root)
    return ctx, n, rec


def assert_summary(ctx, n, rec, e):
    assert (n, rec) == (e["positions"], e["root_record"])
    assert ctx.tier_counts().tolist() == e["per_tier"]
    assert ctx.digest() == (e["digest"], e["positions"])
    assert ctx.histogram().tolist() == e["histogram"]
    assert ctx.stats()["n_positions"] == e["positions"]
    assert sum(row[0] for row in e["histogram"]) == e["primitive"]   # remoteness 0: the primitive positions


@pytest.fixture(scope="module")
def solved43():
    ctx, n, rec = solve((4, 3, 3))
    yield ctx, n, rec
    ctx.close()


@pytest.fixture(scope="module")
def table43():
    keys, recs = mcg.load_table("connect_4x3_3")
    return keys, recs, dict(zip(keys.tolist(), recs.tolist()))


# (4, 3, 3): a WIN root that is its own mirror image; (2, 5, 4): L < K, vertical lines only;
# (5, 2, 4): H < K, horizontal lines only, columns full after two discs
@pytest.mark.parametrize("dims", [(3, 3, 3), (4, 3, 3), (2, 5, 4), (5, 2, 4), (4, 4, 4)])
def test_exported_table_equals_the_fixture(dims):
    name = mcg.name_of(*dims)
    keys, recs = mcg.load_table(name)
    ctx, n, rec = solve(dims)
    try:
        assert ctx.initial() == J[name]["root"]
        assert ctx.stats()["engine"] == _lib.ENGINE_SPARSE   # GM_ENGINE_AUTO
        k, r = ctx.export()
        assert np.array_equal(k, keys) and np.array_equal(r, recs)
        assert_summary(ctx, n, rec, J[name])
        some = keys[:: max(1, len(keys) // 500)]
        assert np.array_equal(ctx.query(some), recs[:: max(1, len(keys) // 500)])
    finally:
        ctx.close()


@pytest.mark.parametrize("dims", [(4, 5, 4), (5, 4, 4)])   # the pair catches a swapped L and H
def test_summary_equals_the_fixture(dims):
    ctx, n, rec = solve(dims)
    try:
        assert_summary(ctx, n, rec, J[mcg.name_of(*dims)])
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["c7x6_a", "c7x6_b", "c7x6_sym", "c9x6_a"])
def test_custom_roots_of_the_standard_and_the_widest_board(name):
    e = J[name]
    assert e["dims"][:2] in ([7, 6], [9, 6]) and 1000 <= e["positions"] <= 300000
    ctx, n, rec = solve(tuple(e["dims"]), e["root"])
    try:
        assert_summary(ctx, n, rec, e)
        st = ctx.stats()
        assert (st["n_stored"] < n) == e["root_symmetric"]
        res, bad = ctx.verify()
        assert res["n_bad"] == 0 and bad == [] and res["root_ok"] == 1 and res["checked"] == st["n_stored"]
    finally:
        ctx.close()
    assert not J["c7x6_a"]["root_symmetric"] and J["c9x6_a"]["root"] >> 61


@pytest.mark.parametrize("name", ["connect_4x4_4", "c7x6_sym"])
def test_symmetry_on_and_off_agree_on_a_symmetric_root(name):
    e = J[name]
    assert e["root_symmetric"]
    on, n1, rec1 = solve(tuple(e["dims"]), e["root"], symmetry=1)
    off, n0, rec0 = solve(tuple(e["dims"]), e["root"], symmetry=0)
    try:
        assert (n1, rec1) == (n0, rec0) == (e["positions"], e["root_record"])
        assert on.digest() == off.digest() == (e["digest"], e["positions"])
        assert on.histogram().tolist() == off.histogram().tolist() == e["histogram"]
        assert on.stats()["n_stored"] < n1 and off.stats()["n_stored"] == n0
        # one representative per mirror pair, both of a pair's positions counted
        k, _ = off.export()
        own = sum(1 for q in k.tolist() if mcg.mirror(q, *e["dims"][:2]) == q)
        assert on.stats()["n_stored"] == (n1 + own) // 2
    finally:
        on.close()
        off.close()


def test_an_asymmetric_root_is_not_reduced():
    e = J["c7x6_a"]
    ctx, n, rec = solve(tuple(e["dims"]), e["root"], symmetry=1)
    try:
        assert ctx.stats()["n_stored"] == n == e["positions"]
    finally:
        ctx.close()


def test_toggling_symmetry_between_solves_of_one_root():
    """The recorded plan of the first solve must not be replayed for the second: the tables of
    a reduced and of an unreduced solve differ in size (sparse.hip plan_key_of)."""
    e = J["connect_4x4_4"]
    ctx = Context(CONNECT, (4, 4, 4), device=0)
    try:
        for sym in (1, 1, 0, 0, 1):
            ctx.set_option(_lib.OPT_SYMMETRY, sym)
            n, rec = ctx.solve(e["root"])
            assert_summary(ctx, n, rec, e)
            assert (ctx.stats()["n_stored"] < n) == bool(sym)
    finally:
        ctx.close()


@pytest.mark.parametrize("ranks", [3, 8])
def test_virtual_ranks_give_the_fixture(ranks):
    e = J["connect_4x4_4"]
    ctx, n, rec = solve((4, 4, 4), engine=_lib.ENGINE_DIST_SPARSE, virtual_ranks=ranks)
    try:
        assert ctx.stats()["engine"] == _lib.ENGINE_DIST_SPARSE and ctx.stats()["world"] == ranks
        assert (n, rec) == (e["positions"], e["root_record"])
        assert ctx.digest() == (e["digest"], e["positions"])
        assert ctx.tier_counts().tolist() == e["per_tier"]
    finally:
        ctx.close()


def test_roots_that_are_no_position_are_refused_by_gm_solve():
    good = 33825 + 2 + 32   # 4x4 after one move each in columns 0 and 1
    ctx = Context(CONNECT, (4, 4, 4), device=0)
    try:
        for k in (good & ~(31 << 10), good | 1 << 20, 33825 + 2 + 64):   # a zero field, a high bit, two first-player discs
            with pytest.raises(GMError) as err:
                ctx.solve(k)
            assert err.value.code == -10   # GM_E_KEY
        n, _ = ctx.solve(good)
        assert n > 1
    finally:
        ctx.close()


# ---------------------------------------------------------------- the readers, on 4x3 connect 3
def test_histogram(solved43):
    ctx, n, _ = solved43
    h = ctx.histogram()
    assert h.tolist() == J["connect_4x3_3"]["histogram"] and int(h.sum()) == n


def test_select_equals_the_histogram_cell(solved43):
    ctx, _, _ = solved43
    h = J["connect_4x3_3"]["histogram"]
    keys, recs = mcg.load_table("connect_4x3_3")
    for sel, value, rem in ((_lib.SEL_TIE, 2, 3), (_lib.SEL_WIN, 0, 5), (_lib.SEL_LOSS, 1, 0)):
        want = keys[recs == (value << 14 | rem)]
        n, k, r = ctx.select(sel, rem, rem, cap=len(keys), as_array=True)
        assert n == h[value][rem] == len(want) > 0
        assert np.array_equal(k, want) and set(r.tolist()) == {value << 14 | rem}


def test_reach_everything_from_the_root(solved43):
    ctx, n, _ = solved43
    out, plies, _, _, _ = ctx.reach([J["connect_4x3_3"]["root"]], _lib.REACH_ALL, _lib.REACH_ALL)
    assert out["n"] == n and out["missing"] == 0 and out["plies"] == len(J["connect_4x3_3"]["per_tier"])
    assert plies.tolist() == J["connect_4x3_3"]["per_tier"]


def test_moves_batch_follows_the_plugin(solved43, table43):
    ctx, _, _ = solved43
    keys, recs, rec_of = table43
    mod = load_plugin(PLUGIN, length=4, height=3, connect=3)
    sample = keys[::5]
    heads, ck, cr = ctx.moves_batch(sample)
    assert np.array_equal(heads["record"], recs[::5])
    for p, h in zip(sample.tolist(), heads):
        first, cnt = int(h["first"]), int(h["count"])
        if mod.primitive(p) != UNDECIDED:
            assert cnt == 0 and h["best"] == -1
            continue
        kids = [mod.do_move(p, m) for m in mod.gen_moves(p)]
        assert ck[first:first + cnt].tolist() == kids
        want = [rec_of[c] for c in kids]
        assert cr[first:first + cnt].tolist() == want
        assert h["best"] == best_move(np.array(want, dtype=np.uint16))[0]


def test_export_import_round_trip(solved43):
    ctx, n, rec = solved43
    keys, recs = ctx.export()
    other = Context(CONNECT, (4, 3, 3), device=0)
    try:
        assert other.import_table(keys[::-1].copy(), recs[::-1].copy(), J["connect_4x3_3"]["root"]) == (n, rec)
        assert other.digest() == ctx.digest()
        res, bad = other.verify()
        assert res["n_bad"] == 0 and bad == [] and res["root_ok"] == 1
        assert other.stats()["n_stored"] == ctx.stats()["n_stored"] < n
        k2, r2 = other.export()
        assert np.array_equal(k2, keys) and np.array_equal(r2, recs)
    finally:
        other.close()


def test_verify_is_clean_and_finds_a_poked_record(table43):
    keys, recs, _ = table43
    ctx, n, _ = solve((4, 3, 3))
    try:
        res, bad = ctx.verify()
        assert res["n_bad"] == 0 and bad == [] and res["root_ok"] == 1
        assert res["checked"] == ctx.stats()["n_stored"] < n
        # an interior TIE position, in its stored form (the smaller of the mirror pair), made a LOSS in 0
        i = next(i for i in range(len(keys) // 2, len(keys))
                 if recs[i] >> 14 == 2 and recs[i] & 0x3FFF > 0 and mcg.mirror(int(keys[i]), 4, 3) >= int(keys[i]))
        ctx.poke(int(keys[i]), 1 << 14)
        res, bad = ctx.verify()
        assert res["n_bad"] >= 1 and int(keys[i]) in bad
        ctx.poke(int(keys[i]), int(recs[i]))
        assert ctx.verify()[0]["n_bad"] == 0
    finally:
        ctx.close()


# ---------------------------------------------------------------- the launcher
def _launch(argv):
    import solver_launcher
    out = io.StringIO()
    status = solver_launcher.run(solver_launcher.build_parser().parse_args(argv), out=out)
    return status, out.getvalue()


def test_launcher_prints_the_root_line():
    status, out = _launch([PLUGIN, "--dims", "4x4"])
    assert status == 0 and out.splitlines()[0] == "TIE in 16 moves"


def test_launcher_options_work_on_the_new_game(tmp_path):
    T = str(tmp_path / "T")
    game = [PLUGIN, "--dims", "4x3", "--connect", "3"]
    status, out = _launch(game + ["--analysis", "--verify", "--moves", "--line", "--strategy", "-sd", T, "--sd-format", "npz"])
    lines = out.splitlines()
    assert status == 0 and lines[0] == "WIN in 9 moves"
    assert any(l.startswith("Strategy for the player to move (root WIN in 9 moves)") for l in lines)
    assert any(l.startswith("Verified ") and l.endswith("consistent") for l in lines)
    at = lines.index("Line:")
    assert lines[at + 1].startswith("  0. ") and lines[at + 10].startswith("  9. ") and lines[at + 10].endswith("LOSS in 0")
    # the root's moves in column order, the winning ones starred
    moves = lines[lines.index("Moves:") + 1:]
    assert [l.split(" -> ")[0].strip() for l in moves] == ["0", "1", "2", "3"]
    assert 1 <= sum(l.endswith(" in 8 *") for l in moves) and all(("LOSS in 8" in l) == l.endswith(" *") for l in moves)
    # the stored table answers in place of a solve; with --find every position found lists its own moves
    status, loaded = _launch(game + ["--load", T, "--verify", "--find", "tie:3", "--find-cap", "2", "--moves"])
    lines = loaded.splitlines()
    assert status == 0 and lines[0] == "WIN in 9 moves"
    assert any(l.startswith("Verified ") and l.endswith("consistent") for l in lines)
    assert "Found %d positions: tie:3" % J["connect_4x3_3"]["histogram"][2][3] in lines
    assert "Moves:" not in lines and sum(" -> " in l for l in lines) >= 2
