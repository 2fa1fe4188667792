"""The 8x8 Othello chain on the CPU: reference plugin -> fixtures -> C oracle (-> device, in
tests/test_gpu_othello8.py).

Fixtures written by the REFERENCE's own plugin (tests/golden/make_golden.py):
* othello_8x8_playouts.npz    whole games from the 8x8 start: positions, primitive(), children
                              in gen_moves order (passes above 20 empties, games ended by the
                              second pass, all three outcomes, moves flipping 4+ directions);
* othello_8x8_endgame.npz     the full table below the 10-empty root;
* othello_8x8_reference.json  summaries of the 12-empty root and three pass roots.

Pinned to them here: the C oracle (oracle/othello8.c, a square-and-direction walk) and the host
twin of the device descriptor (csrc/games.hpp DescOthello8, shift-and-mask bitboards).  The
oracle then carries the comparison to sizes Python does not reach (oracle_digests.json
othello_8x8_e12 / _e14).  Everything compares bit-exactly.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, digest, golden

sys.path.insert(0, GOLDEN)
import othello8_words as ow  # noqa: E402
import othello8  # noqa: E402  (oracle/)

ENDGAME10_HEX = "303800204018057a4646bfdebfe6fa800200"
SUMMARY = ("positions", "per_tier", "root_record", "word_digest")


@pytest.fixture(scope="module")
def o8():
    return othello8.Othello8Oracle()


@pytest.fixture(scope="module")
def playouts():
    d = np.load(os.path.join(GOLDEN, "othello_8x8_playouts.npz"))
    pos = [tuple(int(x) for x in w) for w in ow.bytes_to_words(d["positions"])]
    kids = [tuple(int(x) for x in w) for w in ow.bytes_to_words(d["children"])]
    off = d["child_off"]
    return {"pos": pos, "prim": d["primitive"].tolist(), "kids": [kids[off[i]:off[i + 1]] for i in range(len(pos))],
            "meta": json.loads(str(d["meta"]))}


@pytest.fixture(scope="module")
def reference():
    return json.load(open(os.path.join(GOLDEN, "othello_8x8_reference.json")))


def _root(hexpos):
    return ow.words_of(bytes.fromhex(hexpos).decode("latin-1"))


def _int(w):
    return w[0] | (w[1] << 64) | (w[2] << 128)


def test_words_round_trip():
    pos = bytes.fromhex(ENDGAME10_HEX).decode("latin-1")
    w = ow.words_of(pos)
    assert ow.pos_of(w) == pos and _int(w) == int.from_bytes(pos.encode("latin-1"), "big")
    arr = ow.words_array([pos])
    assert tuple(int(x) for x in arr[0]) == w and ow.words_to_bytes(arr).tobytes() == pos.encode("latin-1")
    assert int(ow.tiers(arr)[0]) == 3 * 54


def test_playout_fixture_coverage(playouts):
    """The conditions the generator asserted, re-counted from the stored data."""
    m = playouts["meta"]
    nonprim = [i for i, p in enumerate(playouts["prim"]) if p == 4]
    assert len(nonprim) == m["non_primitive"] >= 2000
    assert all(len(playouts["kids"][i]) >= 1 for i in nonprim)
    passes = [i for i in nonprim if len(playouts["kids"][i]) == 1 and
              (playouts["kids"][i][0][0] & 0xFF) == (playouts["pos"][i][0] & 0xFF) + 1]
    early = [i for i in passes if int(ow.tiers(np.array([playouts["pos"][i]], dtype=np.uint64))[0]) // 3 <= 44]
    assert len(passes) == m["pass_positions"] and len(early) == m["pass_positions_20_empties"] >= 5
    ends = {v: sum(1 for p in playouts["prim"] if p == v) for v in (0, 1, 2)}
    assert (ends[0], ends[1], ends[2]) == (m["terminal_win"], m["terminal_loss"], m["terminal_tie"]) and min(ends.values()) >= 1
    second = [i for i, p in enumerate(playouts["prim"]) if p != 4 and (playouts["pos"][i][0] & 0xFF) == 2]
    assert len(second) >= 1 and m["games_ended_by_second_pass_with_empties"] >= 1
    assert m["moves_flipping_4_directions"] >= 1


def test_oracle_expand_vs_reference_playouts(o8, playouts):
    """oracle_othello8_expand on every playout position: primitive value, and the children in
    gen_moves order."""
    for w, prim, kids in zip(playouts["pos"], playouts["prim"], playouts["kids"]):
        p, tier, got = o8.expand(w)
        assert p == prim, hex(_int(w))
        assert got == kids, hex(_int(w))
        assert tier == int(ow.tiers(np.array([w], dtype=np.uint64))[0])


def test_host_twin_vs_reference_playouts(playouts):
    """gm_expand_host_key (the bitboard generator the device kernels run, on the host) on every
    playout position: primitive value, child set and -- as include/gmsolve.h promises -- the
    children in the plugin's gen_moves order.  (DescOthello8::visit itself walks the plane's
    lowest bit first, the string's last square; gm_expand_host_key reorders.)"""
    from gamesmanmpi_amd import games
    hd = games.HostDescriptor(games.OthelloCodec(8, 8))
    try:
        for w, prim, kids in zip(playouts["pos"], playouts["prim"], playouts["kids"]):
            p, got, tier = hd.expand(_int(w))
            assert p == prim, hex(_int(w))
            want = [_int(k) for k in kids]
            assert sorted(got) == sorted(want), hex(_int(w))
            assert got == want, hex(_int(w))
            assert tier == int(ow.tiers(np.array([w], dtype=np.uint64))[0])
    finally:
        hd.close()


def test_oracle_solve_vs_golden_table_10_empties(o8):
    """The oracle's full table below the 10-empty root equals othello_8x8_endgame.npz, the
    reference plugin's (keys = blake2b-8 of the position string)."""
    r = o8.solve(_root(ENDGAME10_HEX), want=1 << 62)
    keys, recs = golden("othello_8x8_endgame")
    assert r["positions"] == len(r["words"]) == len(keys) == 56552
    raw = ow.words_to_bytes(r["words"])
    got = {int.from_bytes(hashlib.blake2b(row.tobytes(), digest_size=8).digest(), "big"): int(x)
           for row, x in zip(raw, r["records"])}
    assert got == dict(zip(keys.tolist(), recs.tolist()))
    # the returned table is in key order and its digests are the solve's
    ints = [_int(tuple(int(x) for x in w)) for w in r["words"]]
    assert ints == sorted(ints)
    assert digest(ow.fold(r["words"]), r["records"]) == r["word_digest"]
    # a sample is every floor(i * n / m)-th entry of that table
    s = o8.solve(_root(ENDGAME10_HEX), want=100)
    pick = (np.arange(100, dtype=np.uint64) * np.uint64(56552)) // np.uint64(100)
    assert np.array_equal(s["words"], r["words"][pick]) and np.array_equal(s["records"], r["records"][pick])


@pytest.mark.parametrize("name", ["e12", "pass_e9", "pass_e10", "pass_e11"])
def test_oracle_solve_vs_reference_summaries(o8, reference, name):
    """Count, per-tier counts, root record and word_digest of the canonical solve over the
    reference plugin, at 1 and 3 threads."""
    e = reference[name]
    for threads in (1, 3):
        r = o8.solve(_root(e["root_hex"]), threads=threads)
        assert {k: r[k] for k in SUMMARY} == {k: e[k] for k in SUMMARY}, threads


def test_oracle_thread_counts_agree(o8, reference):
    """1 and 3 threads give one result, the gm_digest-form digest and the table included."""
    e = reference["pass_e10"]
    a = o8.solve(_root(e["root_hex"]), threads=1, want=1 << 62)
    b = o8.solve(_root(e["root_hex"]), threads=3, want=1 << 62)
    assert {k: a[k] for k in SUMMARY + ("digest",)} == {k: b[k] for k in SUMMARY + ("digest",)}
    assert np.array_equal(a["words"], b["words"]) and np.array_equal(a["records"], b["records"])


def test_committed_oracle_digests_match_reference_and_sample(o8, reference):
    """oracle_digests.json othello_8x8_e12 is the solve the reference summary pins (its
    gm_digest-form digest is what the device must reproduce), and the 14-empty sample holds
    valid, distinct positions in key order whose records the oracle's expand explains: each
    sampled primitive position has its primitive value's record."""
    dg = json.load(open(os.path.join(GOLDEN, "oracle_digests.json")))
    e12 = dg["othello_8x8_e12"]
    assert {k: e12[k] for k in SUMMARY} == {k: reference["e12"][k] for k in SUMMARY}
    assert e12["root_hex"] == reference["e12"]["root_hex"]
    assert o8.solve(_root(e12["root_hex"]))["digest"] == e12["digest"]
    e14 = dg["othello_8x8_e14"]
    assert sum(e14["per_tier"]) == e14["positions"] == 53672134
    d = np.load(os.path.join(GOLDEN, "othello_8x8_e14_sample.npz"))
    words, recs = d["words"], d["records"]
    assert len(words) == len(recs) == 4096
    ints = [_int(tuple(int(x) for x in w)) for w in words]
    assert ints == sorted(set(ints))
    assert int(ow.tiers(words).min()) >= 3 * 50
    for w, rec in zip(words[::16], recs[::16]):
        p, _, kids = o8.expand(tuple(int(x) for x in w))
        assert (rec == p << 14) if p != 4 else ((rec & 0x3FFF) >= 1 and len(kids) >= 1)
