"""Connect (k in a row with gravity) without a GPU: the plugin test_games/connect4.py against
the fixtures of tests/golden/make_connect_golden.py, the descriptor's host twin
(gm_expand_host, games.hpp DescConnect) against the plugin, the binding, and what gm_open and
the root check refuse."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_plugin

sys.path.insert(0, GOLDEN)
import make_connect_golden as mcg  # noqa: E402

from gamesmanmpi_amd import GMError, _lib, games  # noqa: E402

PLUGIN = "test_games/connect4.py"
SMALL = [(3, 3, 3), (4, 3, 3), (2, 5, 4), (5, 2, 4)]
UNDECIDED = 4


def plugin(L, H, K):
    return load_plugin(PLUGIN, length=L, height=H, connect=K)


def host(L, H, K):
    return games.HostDescriptor(games.ConnectCodec(L, H, K))


def rc_open(params):
    h = ctypes.c_void_p()
    arr = (ctypes.c_int32 * len(params))(*params)
    rc = _lib.lib().gm_open(_lib.GAME_CONNECT, arr, len(params), -1, ctypes.byref(h))
    if rc == 0:
        _lib.lib().gm_close(h)
    return rc


_walks = {}


def walk(L, H, K):
    """Every position reachable from the empty board, over the plugin: {pos: (primitive,
    children in gen_moves order)}.  Made once per board and left unchanged."""
    if (L, H, K) not in _walks:
        mod = plugin(L, H, K)
        out = {}
        frontier = [mod.initial_position()]
        while frontier:
            nxt = []
            for p in frontier:
                if p in out:
                    continue
                prim = mod.primitive(p)
                kids = [mod.do_move(p, m) for m in mod.gen_moves(p)] if prim == UNDECIDED else []
                out[p] = (prim, kids)
                nxt.extend(kids)
            frontier = nxt
        _walks[(L, H, K)] = out
    return _walks[(L, H, K)]


@pytest.mark.parametrize("L,H,K", SMALL)
def test_plugin_solves_to_the_fixture_table(L, H, K):
    import canonical
    mod = plugin(L, H, K)
    table, _ = canonical.solve(mod)
    keys, recs = mcg.load_table(mcg.name_of(L, H, K))
    assert len(table) == len(keys)
    got = np.array([(table[int(k)][0] << 14) | table[int(k)][1] for k in keys], dtype=np.uint16)
    assert np.array_equal(got, recs)
    e = mcg.load_json()[mcg.name_of(L, H, K)]
    assert e == {**e, **mcg.summary(keys, recs, mod.initial_position(), L, H, K)}


def test_fixture_counts_are_the_expected_ones():
    """Positions, primitive positions and the root line per board."""
    J = mcg.load_json()
    want = {(3, 3, 3): (694, 189, "TIE", 9), (4, 3, 3): (7157, 2526, "WIN", 9), (2, 5, 4): (537, 122, "TIE", 10),
            (5, 2, 4): (4688, 313, "TIE", 10), (4, 4, 4): (161029, 26740, "TIE", 16),
            (4, 5, 4): (1706255, 357814, "TIE", 20), (5, 4, 4): (3945711, 845332, "TIE", 20)}
    for (L, H, K), (n, prim, v, r) in want.items():
        e = J[mcg.name_of(L, H, K)]
        assert (e["positions"], e["primitive"]) == (n, prim), (L, H, K)
        assert e["root_record"] == ("WIN", "LOSS", "TIE").index(v) << 14 | r, (L, H, K)
        assert sum(e["per_tier"]) == n and sum(map(sum, e["histogram"])) == n


def test_plugin_matches_the_4x4_summary(oracle):
    """The 4x4 table is too long to solve twice by the Python solver in a quick test: the walk gives
    the positions, the primitive ones and the tiers, and the fixture's records must be the canonical
    fold of their children's records at every position.  The C oracle does solve it again: the whole
    table, key for key."""
    import canonical
    w = walk(4, 4, 4)
    keys, recs = mcg.load_table("connect_4x4_4")
    e = mcg.load_json()["connect_4x4_4"]
    assert len(w) == e["positions"] == len(keys) and set(w) == set(int(k) for k in keys)
    assert sum(1 for prim, _ in w.values() if prim != UNDECIDED) == e["primitive"]
    assert e == {**e, **mcg.summary(keys, recs, 33825, 4, 4, 4)}
    rec = dict(zip((int(k) for k in keys), (int(r) for r in recs)))
    for p, (prim, kids) in w.items():
        want = (prim, 0) if prim != UNDECIDED else canonical.fold((rec[c] >> 14, rec[c] & 0x3FFF) for c in kids)
        assert (rec[p] >> 14, rec[p] & 0x3FFF) == want, p
    k, r = oracle.solve(_lib.GAME_CONNECT, (4, 4, 4))
    assert np.array_equal(k, keys) and np.array_equal(r, recs)


@pytest.mark.parametrize("L,H,K", SMALL + [(4, 4, 4)])
def test_host_twin_agrees_with_the_plugin_everywhere(L, H, K):
    """Primitive code, children in gen_moves order and tier (the disc count) at every position."""
    w = walk(L, H, K)
    ps = list(w)
    tiers = mcg.discs(np.array(ps, dtype=np.uint64), L, H)
    mod = plugin(L, H, K)
    hd = host(L, H, K)
    try:
        assert hd.initial() == mod.initial_position()
        for p, t in zip(ps, tiers):
            assert hd.expand(p) == (w[p][0], w[p][1], t), p
        for p, t in list(zip(ps, tiers))[::97]:
            assert mod._discs(p, mod._caps(p)) == t
    finally:
        hd.close()


def test_identify_binds_the_plugin_and_not_a_changed_copy(tmp_path):
    mod = plugin(4, 3, 3)
    c = games.identify(mod)
    assert isinstance(c, games.ConnectCodec) and c.params == (4, 3, 3) and c.game_id == _lib.GAME_CONNECT
    # by the exhaustive check as well (7,157 positions), as a plugin of another interpreter binds
    c = games.identify(mod, exhaustive_max=10000)
    assert isinstance(c, games.ConnectCodec)
    # the default board binds by its code alone (3.9 M positions: no exhaustive replay)
    c = games.identify(load_plugin(PLUGIN), exhaustive_max=0)
    assert isinstance(c, games.ConnectCodec) and c.params == (5, 4, 4)
    # one rule changed -- diagonals not counted: nothing binds, the plugin goes to the graph engine
    src = open(os.path.join(REPO, PLUGIN)).read()
    assert "(1, width, width - 1, width + 1)" in src
    changed = tmp_path / "connect4_no_diagonals.py"
    changed.write_text(src.replace("(1, width, width - 1, width + 1)", "(1, width)"))
    bad = load_plugin(str(changed), length=4, height=3, connect=3)
    assert games.identify(bad) is None
    # a plugin without `connect` is not offered this codec
    assert not any(isinstance(c, games.ConnectCodec) for c in games._candidates(load_plugin("test_games/subtraction.py")))


def test_gm_open_takes_the_boards_of_at_most_63_bits():
    for params in [(7, 6, 4), (9, 6, 4), (1, 62, 4), (16, 2, 8), (5, 4, 2)]:
        assert rc_open(params) == 0, params
    assert rc_open(()) == 0   # the defaults 5, 4, 4
    hd = games.HostDescriptor(games.ConnectCodec(5, 4, 4))
    dflt = ctypes.c_void_p()
    _lib.check(_lib.lib().gm_open(_lib.GAME_CONNECT, None, 0, -1, ctypes.byref(dflt)))
    k = ctypes.c_uint64()
    _lib.check(_lib.lib().gm_pack_initial(dflt, ctypes.byref(k)))
    _lib.lib().gm_close(dflt)
    assert k.value == hd.initial()
    hd.close()
    for params in [(8, 7, 4), (17, 2, 4), (5, 4, 1), (5, 4, 9), (0, 4, 4), (5, 0, 4), (1, 63, 4)]:
        assert rc_open(params) == -2, params   # GM_E_GAME
    with pytest.raises(ValueError):
        games.ConnectCodec(8, 7, 4)


@pytest.mark.parametrize("L,H,K", [(5, 4, 4), (7, 6, 4), (9, 6, 4), (1, 62, 4), (3, 1, 2)])
def test_pack_initial_is_the_bottom_mask(L, H, K):
    hd = host(L, H, K)
    assert hd.initial() == sum(1 << (x * (H + 1)) for x in range(L))
    assert hd.expand(hd.initial())[0] == UNDECIDED and hd.expand(hd.initial())[2] == 0
    hd.close()


def pack(fields, H):
    """A key from its column fields, column 0 first."""
    return sum(f << (x * (H + 1)) for x, f in enumerate(fields))


def test_roots_that_are_no_position_are_refused():
    # 4x4 fields: 0b00001 empty, 0b00010 one second-player disc, 0b00011 one first-player disc,
    # 0b00101 a first-player disc under a second-player one, 0b01111 three first-player discs
    good = pack([0b00010, 0b00101, 0b00011, 0b00001], 4)   # 4 discs, 2 of them the first player's
    bad = {"a zero column field": pack([0b00010, 0b00011, 0, 0b00001], 4),
           "a bit above the board": good | 1 << 20,
           "bit 63": good | 1 << 63,
           "3 first-player stones of 3 discs": pack([0b01111, 1, 1, 1], 4),
           "no first-player stone of 2 discs": pack([0b00010, 0b00010, 1, 1], 4)}
    hd = host(4, 4, 4)
    try:
        assert hd.expand(good)[2] == 4
        for why, k in bad.items():
            with pytest.raises(GMError) as e:
                hd.expand(k)
            assert e.value.code == -10, why   # GM_E_KEY
    finally:
        hd.close()


def test_codec_is_the_identity_with_range_checks():
    c = games.ConnectCodec(4, 4, 4)
    assert c.key(33825) == 33825 and c.pos(33825) == 33825 and c.key(np.uint64(33825)) == 33825
    for bad in (True, "33825", -1, 1 << 20, 0b00001_00000_00001_00001, np.zeros((3, 3))):
        with pytest.raises(ValueError):
            c.key(bad)


@pytest.mark.parametrize("L,H,K", [(7, 6, 4), (9, 6, 4), (4, 3, 3)])
def test_mirror_is_an_involution_that_commutes_with_the_rules(L, H, K):
    """The descriptor's mirror is not exported; the rules it must commute with are: the host
    twin's primitive and child SET at mirror(p) are the mirror images of those at p, on random
    playouts, and the plugin agrees with the twin on the way."""
    hd = host(L, H, K)
    mod = plugin(L, H, K)
    rng = random.Random(L * 100 + H)
    seen = 0
    try:
        for _ in range(60):
            p = mod.initial_position()
            while True:
                m = mcg.mirror(p, L, H)
                assert mcg.mirror(m, L, H) == p
                prim, kids, tier = hd.expand(p)
                mprim, mkids, mtier = hd.expand(m)
                assert prim == mprim == mod.primitive(p) == mod.primitive(m) and tier == mtier
                assert sorted(mcg.mirror(c, L, H) for c in kids) == sorted(mkids)
                assert mkids == [mcg.mirror(c, L, H) for c in reversed(kids)]   # columns, ascending
                seen += 1
                if prim != UNDECIDED:
                    break
                assert kids == [mod.do_move(p, x) for x in mod.gen_moves(p)]
                p = kids[rng.randrange(len(kids))]
    finally:
        hd.close()
    assert seen >= 60 * (2 * K - 1)   # no game ends before the first player's K-th disc


def test_launchers_take_connect_and_dims():
    import solve_local
    import solver_launcher
    a = solver_launcher.build_parser().parse_args([os.path.join(REPO, PLUGIN), "--dims", "4x3", "--connect", "3"])
    game, root = solver_launcher.prepare_game(a)
    assert (game.length, game.height, game.connect, root) == (4, 3, 3, 4369)
    a = solve_local.build_parser().parse_args([os.path.join(REPO, PLUGIN), "--connect", "3"])
    a.heaps = None
    game, root = solver_launcher.prepare_game(a)
    assert (game.length, game.height, game.connect) == (5, 4, 3)
