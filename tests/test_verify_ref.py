"""CPU side of gm_verify: the reference checker (tests/verify_ref.py) on the golden tables, the
entry points' answers without a solve, the pinned layout of gm_verify_t, and the one place
Python states the choice of the best child (solver.best_move) against canonical.fold.
"""
import ctypes
import os
import random
import subprocess

import pytest

import canonical
import verify_ref
from conftest import REPO, golden
from gamesmanmpi_amd import _lib

F2O, TTT, TOOT = 1, 2, 3
LOSS_IN_0 = 1 << 14


@pytest.fixture(scope="module")
def ttt_ref(oracle):
    keys, recs = golden("ttt")
    return verify_ref.VerifyRef(keys, recs, lambda k: oracle.expand(TTT, (), k))


@pytest.mark.parametrize("name,game,params,n", [("ttt", TTT, (), 5478), ("four_to_one_six", F2O, (), 8),
                                                ("toot_3x3", TOOT, (3, 3), 11097), ("toot_4x3", TOOT, (4, 3), 200127)])
def test_golden_tables_have_no_offenders(oracle, name, game, params, n):
    keys, recs = golden(name)
    assert len(keys) == n
    assert verify_ref.verify(keys, recs, lambda k: oracle.expand(game, params, k)) == {}


def test_flipped_ttt_leaf_is_seen_with_its_parents(ttt_ref):
    """0x4c68 is a LOSS-in-0 leaf.  As WIN in 0 it contradicts primitive(), and each of its three
    parents loses the child that made it WIN in 1."""
    assert ttt_ref.table[0x4c68] == LOSS_IN_0 and ttt_ref.expand(0x4c68)[0] == canonical.LOSS
    bad = ttt_ref.offenders({0x4c68: 0})
    parents = ttt_ref.parents(0x4c68)
    assert len(parents) == 3 and len(bad) == 4
    want = {p: verify_ref.BAD_VALUE for p in parents}
    want[0x4c68] = verify_ref.BAD_PRIMITIVE
    assert bad == want
    assert verify_ref.counts(bad) == {"bad_key": 0, "misplaced": 0, "bad_primitive": 1, "missing_child": 0,
                                      "bad_value": 3}


def test_planted_loss_in_0_on_an_interior_ttt_position(ttt_ref):
    """0x2268 is WIN in 1 with two parents: as LOSS in 0 it and both parents are wrong."""
    assert ttt_ref.table[0x2268] == 1 and ttt_ref.expand(0x2268)[0] == canonical.UNDECIDED
    bad = ttt_ref.offenders({0x2268: LOSS_IN_0})
    assert bad == {k: verify_ref.BAD_VALUE for k in [0x2268] + ttt_ref.parents(0x2268)} and len(bad) == 3
    assert ttt_ref.offenders() == {}                                     # the overlay left the table alone


def test_removed_position_is_missed_by_its_parents(ttt_ref):
    bad = ttt_ref.offenders({0x2268: None})
    assert bad == {p: verify_ref.MISSING_CHILD for p in ttt_ref.parents(0x2268)} and len(bad) == 2


def test_toot_leaf_flip_changes_no_parent_but_a_planted_loss_does(oracle):
    """A WIN <-> TIE flip of a Toot leaf is seen at the leaf alone -- its parents' best child is
    another -- so the device tests plant LOSS in 0 on an interior position, which every parent
    that is not already WIN in 1 must answer."""
    keys, recs = golden("toot_3x3")
    ref = verify_ref.VerifyRef(keys, recs, lambda k: oracle.expand(TOOT, (3, 3), k))
    leaf = next(int(k) for k, r in zip(keys, recs) if int(r) == 2 << 14 and ref.parents(int(k)))
    assert ref.offenders({leaf: 0}) == {leaf: verify_ref.BAD_PRIMITIVE}
    plant = next(int(k) for k in keys[::-1] if ref.expand(int(k))[0] == canonical.UNDECIDED
                 and any(ref.table[p] != 1 for p in ref.parents(int(k))))
    bad = ref.offenders({plant: LOSS_IN_0})
    want = {plant} | {p for p in ref.parents(plant) if ref.table[p] != 1}
    assert set(bad) == want and len(bad) >= 2 and set(bad.values()) == {verify_ref.BAD_VALUE}


def test_unsolved_context_answers_state_error():
    """No solve, no table: both entry points say GM_E_STATE (and need no GPU to say it)."""
    from gamesmanmpi_amd import Context, GMError
    ctx = Context(TTT, ())
    out, n_bad = _lib.Verify(), ctypes.c_uint64()
    assert ctx.L.gm_verify(ctx.h, ctypes.byref(out), None, 0, ctypes.byref(n_bad)) == -5
    key = (ctypes.c_uint64 * 1)(0)
    assert ctx.L.gm_poke(ctx.h, key, 0) == -5
    with pytest.raises(GMError, match="GM_E_STATE"):
        ctx.verify()
    with pytest.raises(GMError, match="GM_E_STATE"):
        ctx.poke(0, 0)
    ctx.close()


def test_verify_layout_pinned(tmp_path):
    """gcc's sizeof / offsetof of gm_verify_t equal the ctypes mirror's; the ABI version stays 2."""
    fields = [n for n, _ in _lib.Verify._fields_]
    src = tmp_path / "pin.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmsolve.h"\nint main(void){\n'
                   '  printf("%zu\\n", sizeof(gm_verify_t));\n'
                   + "".join('  printf("%%zu\\n", offsetof(gm_verify_t, %s));\n' % f for f in fields)
                   + '  printf("%d\\n", GM_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "pin"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(_lib.Verify) == 64
    assert vals[1:-1] == [getattr(_lib.Verify, f).offset for f in fields]
    assert vals[-1] == _lib.ABI_VERSION == 2
    assert fields[1:6] == list(_lib.Verify.CLASSES) == list(verify_ref.CLASSES)   # the class order


@pytest.mark.parametrize("rel,attrs,name", [("test_games/mttt.py", {}, "ttt"),
                                            ("test_games/othello_bit_new.py", {"length": 4, "height": 4, "area": 16},
                                             "othello_4x4"),
                                            ("test_games/toot_and_otto_bitstring.py", {"length": 4, "height": 3},
                                             "toot_4x3")])
def test_expand_host_gives_the_plugins_move_order(rel, attrs, name):
    """Context.moves pairs gm_expand_host's children with gen_moves' labels, so the ORDER must be
    the plugin's (the set is pinned by tests/test_abi.py): 300 golden positions of each game."""
    from conftest import load_plugin
    from gamesmanmpi_amd import games
    mod = load_plugin(rel, **attrs)
    codec = games.identify(mod, mod.initial_position())
    host = games.HostDescriptor(codec)
    keys = golden(name)[0]
    interior = 0
    for k in keys[::max(1, len(keys) // 300)].tolist():
        pos = codec.pos(k)
        prim, kids, _ = host.expand(k)
        assert prim == mod.primitive(pos)
        if prim == canonical.UNDECIDED:
            interior += 1
            assert kids == [codec.key(mod.do_move(pos, m)) for m in mod.gen_moves(pos)]
    assert interior > 100
    host.close()


def _record(v, r):
    return (v << 14) | r


def test_best_move_agrees_with_fold():
    """solver.best_move (max over score_of_record) picks a child whose record reduces to
    canonical.fold of all of them: random lists over the three values, equal remotenesses
    included, and every single-class list."""
    from gamesmanmpi_amd.solver import best_move, score_of_record
    rng = random.Random(7)
    lists = [[(v, r)] * k for v in (0, 1, 2) for r in (0, 3) for k in (1, 3)]
    for _ in range(2000):
        vals = rng.choice([(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)])
        lists.append([(rng.choice(vals), rng.randrange(0, 5)) for _ in range(rng.randrange(1, 9))])
    for kids in lists:
        recs = [_record(v, r) for v, r in kids]
        i, parent = best_move(recs)
        assert parent == canonical.fold(kids), (kids, i)
        v, r = kids[i]
        assert canonical.fold([(v, r)]) == parent                        # the chosen child alone gives it
        assert i == min(j for j, x in enumerate(recs) if score_of_record(x) == score_of_record(recs[i]))
    assert best_move([]) == (None, None)
    assert score_of_record(0xFFFF) == 0 < min(score_of_record(_record(v, r)) for v in (0, 1, 2) for r in (0, 9))
