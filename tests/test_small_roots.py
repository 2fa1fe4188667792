"""tests/small_roots.py on the CPU: the coverage conditions of the tic-tac-toe subset, the C oracle
against both tic-tac-toe plugins on every root of it, the Four-To-One closed form against the C
oracle up to the deepest root a record holds, the oracles' refusal past it, and the host twin of
the tic-tac-toe descriptor on all 19,683 keys."""
import numpy as np
import pytest

import canonical
from conftest import load_plugin
from small_roots import (F2O_CPU, F2O_DEEPEST, F2O_FIRST_REFUSED, LOSS, TIE, TTT_ALL, TTT_BY_PIECES, TTT_STRATA, WIN,
                         f2o_histogram, f2o_record, f2o_table, shuffled, ttt_counts, ttt_outside_key, ttt_pieces)

from gamesmanmpi_amd import games

F2O, TTT = 1, 2
UNDECIDED = 4


@pytest.fixture(scope="module")
def ttt_sweep(oracle):
    """The oracle's root record and position count of every one of the 19,683 roots."""
    recs, sizes = {}, {}
    for k in TTT_ALL:
        keys, r = oracle.solve(TTT, (), k)
        recs[k] = int(r[np.searchsorted(keys, k)])
        sizes[k] = len(keys)
    return recs, sizes


def test_ttt_full_sweep_figures(ttt_sweep):
    recs, sizes = ttt_sweep
    assert sum(sizes.values()) == 453458 and max(sizes.values()) == sizes[0] == 5478
    assert sum(r == LOSS << 14 for r in recs.values()) == 8558   # a line on the board
    classes = sorted({(r >> 14, r & 0x3FFF) for r in recs.values()})
    # 17 root records: WIN in 1, 3, 5; LOSS in 0, 2, 4, 6; TIE in 0 .. 9
    assert classes == [(WIN, r) for r in (1, 3, 5)] + [(LOSS, r) for r in (0, 2, 4, 6)] + [(TIE, r) for r in range(10)]


def test_ttt_strata_coverage(oracle, ttt_sweep):
    recs, sizes = ttt_sweep
    assert len(TTT_STRATA) == len(set(TTT_STRATA)) == 1873
    pairs = {ttt_counts(k) for k in TTT_STRATA}
    assert len(pairs) == 55 and pairs == {(x, o) for x in range(10) for o in range(10 - x)}
    assert sum(oracle.expand(TTT, (), k)[0] == UNDECIDED for k in TTT_STRATA) >= 700
    assert sum(x - o not in (0, 1) for x, o in map(ttt_counts, TTT_STRATA)) >= 1500
    assert {recs[k] for k in TTT_STRATA} == set(recs.values()) and len(set(recs.values())) == 17
    assert sum(sizes[k] for k in TTT_STRATA) == 131195


def test_ttt_helpers():
    assert sum(len(p) for p in TTT_BY_PIECES) == 19683 and [len(p) for p in TTT_BY_PIECES][:3] == [1, 18, 144]
    assert all(ttt_pieces(k) == p for p, ks in enumerate(TTT_BY_PIECES) for k in ks[::97])
    for k in TTT_ALL:
        out = ttt_outside_key(k)
        assert 0 <= out < 19683 and out != k and (ttt_pieces(out) < ttt_pieces(k) or k == 0)
    assert sorted(shuffled(TTT_STRATA)) == list(TTT_STRATA) and shuffled(TTT_STRATA) == shuffled(TTT_STRATA)
    assert shuffled(TTT_STRATA) != list(TTT_STRATA)


@pytest.mark.parametrize("rel,codec", [("test_games/mttt.py", games.TTTStringCodec()),
                                       ("test_games/tic_tac_toe_np.py", games.TTTNumpyCodec())],
                         ids=["mttt", "tic_tac_toe_np"])
def test_oracle_equals_plugin_on_every_strata_root(oracle, rel, codec):
    """Keys and records of the C oracle against the canonical solve over the plugin's own functions."""
    mod = load_plugin(rel)
    for root in TTT_STRATA:
        table, positions = canonical.solve(mod, root=codec.pos(root))
        got = sorted((codec.key(positions[k]), (v << 14) | r) for k, (v, r) in table.items())
        keys, recs = oracle.solve(TTT, (), root)
        assert [k for k, _ in got] == keys.tolist() and [r for _, r in got] == recs.tolist(), root


def test_host_descriptor_equals_oracle_on_every_ttt_key(oracle):
    """gm_expand_host on all 3^9 keys: primitive value, children and tier -- unbalanced boards and
    boards with two lines too.  The children come in the plugin's move order, cell by cell, which
    for this key is ascending: the order the oracle's (sorted) list has."""
    hd = games.HostDescriptor(games.TTTStringCodec())
    for k in TTT_ALL:
        p, kids, t = hd.expand(k)
        assert (p, kids, t) == oracle.expand(TTT, (), k), k
        assert t == ttt_pieces(k)
    hd.close()


@pytest.mark.parametrize("root", F2O_CPU)
def test_f2o_closed_form_equals_oracle(oracle, root):
    keys, recs = f2o_table(root)
    ok, orec = oracle.solve(F2O, (), root % (1 << 64))
    assert keys.dtype == np.uint64 and recs.dtype == np.uint16
    assert np.array_equal(keys, ok) and np.array_equal(recs, orec)
    assert np.all(np.diff(keys.astype(object)) > 0)
    if root >= 1:
        n, _, rec, tiers = oracle.solve_layered(F2O, (), root)
        assert n == root + 2 and rec == f2o_record(root) and set(tiers) == {1}
    assert int(f2o_histogram(root).sum()) == len(keys)


def test_f2o_limit_records():
    assert f2o_record(F2O_DEEPEST) == 0x3FFF                  # WIN in 0x3FFF
    assert f2o_record(F2O_DEEPEST - 1) == 0x3FFF
    assert f2o_record(F2O_DEEPEST - 2) == LOSS << 14 | 0x3FFE
    with pytest.raises(ValueError):
        f2o_record(F2O_FIRST_REFUSED)
    keys, recs = f2o_table(F2O_DEEPEST)
    assert len(keys) == 24577 and int(keys[-1]) == 2 ** 64 - 1 and int(recs[-1]) == LOSS << 14


@pytest.mark.parametrize("root", [F2O_FIRST_REFUSED, 30000])
def test_oracles_refuse_a_remoteness_past_14_bits(oracle, root):
    """LOSS in 0x4000 has no record: oracle_solve and oracle_solve_layered fail and say why (they
    used to carry into the value bits: root 24576 came back as 0x4000, LOSS in 0)."""
    with pytest.raises(RuntimeError, match="remoteness exceeds 14 bits"):
        oracle.solve(F2O, (), root)
    with pytest.raises(RuntimeError, match="remoteness exceeds 14 bits"):
        oracle.solve_layered(F2O, (), root)


def test_canonical_refuses_a_remoteness_past_14_bits():
    """canonical.solve, whose callers pack (value << 14) | remoteness; fold itself stays the plain
    reduction (tests/graph_ref.py folds unpacked remotenesses and reports the overflow itself)."""
    assert canonical.fold([(LOSS, 0x3FFE)]) == (WIN, 0x3FFF)
    assert canonical.fold([(WIN, 0x3FFF)]) == (LOSS, 0x4000)
    mod = load_plugin("test_games/four_to_one.py")
    table, _ = canonical.solve(mod, root=str(F2O_DEEPEST))
    assert table[str(F2O_DEEPEST)] == (WIN, 0x3FFF) and max(r for _, r in table.values()) == 0x3FFF
    with pytest.raises(canonical.OracleError, match="remoteness exceeds 14 bits"):
        canonical.solve(mod, root=str(F2O_FIRST_REFUSED))
