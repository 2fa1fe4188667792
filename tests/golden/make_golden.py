#!/usr/bin/env python3
"""Generate the golden fixtures in ``tests/golden/`` from the REFERENCE's own plugins.

Run in the build container (``/root/reference`` present; never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py [--live]

What it does:

1. imports the reference's ``src.utils`` and plugin modules from
   ``/root/reference/test_games`` (with an empty ``mpi4py`` stub for
   ``tic_tac_toe_np.py:2`` and ``bitstring_shim.BitArray`` standing in for the
   absent third-party ``bitstring`` package);
2. strong-solves them with the canonical fixed point of ``oracle/canonical.py``
    and writes, per config, the sorted ``(key u64, record u16)``
   table as ``<name>.npz`` (record = value << 14 | remoteness);
3. writes ``roots.json``: the root line for the 9 cases of the reference's
   ``game_tests/four_to_one_test.py`` and ``game_tests/mttt_test.py`` (custom roots
   loaded from ``game_tests/*_init_pos.py`` exactly as ``--custom/--init_pos``
   intends), next to the line those tests expect;
4. with ``--live``: also drives the reference's live engine
   (``src/new_process.Process`` + ``src/new_job.Job``) single-rank under an
   in-process fake MPI and records how its values / remoteness compare with the
   canonical table (``live.json``).

Keys:
  four_to_one: the pile as a signed int64 (stored two's complement in u64);
  ttt:         sum of c * 3**(x + 3y), c = 0 blank, 1 X / player 1, 2 O / player 2;
  toot:        the first 2A+16 bits of the position string (planes + hands), MSB-first;
  othello:     all 2A+16 bits of the position string, MSB-first;
  othello 8x8: the first 8 bytes of blake2b(position string bytes), big-endian (2A+16 = 144
               bits do not fit a u64; tests/plugins/othello8_endgame.py).

``--only othello8`` writes just the 8x8 endgame fixture (othello_8x8_endgame.npz) and its
entry in roots.json.

``--only othello8-playouts`` writes othello_8x8_playouts.npz (whole games of the 8x8 plugin:
positions, primitive(), children in gen_moves order; the coverage counts it asserts are in its
meta), ``--only othello8-reference [--roots NAME ...]`` writes othello_8x8_reference.json (the
12-empty root and three pass roots solved over the plugin: count, root record, per-tier counts,
word_digest of tests/golden/othello8_words.py; the 12-empty solve takes minutes).  Neither
touches the other outputs.
"""
import argparse
import importlib.util
import json
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

sys.dont_write_bytecode = True


def _install_stubs():
    mpi4py = types.ModuleType("mpi4py")
    mpi4py.MPI = types.ModuleType("mpi4py.MPI")
    sys.modules["mpi4py"] = mpi4py
    sys.modules["mpi4py.MPI"] = mpi4py.MPI
    sys.path.insert(0, HERE)
    import bitstring_shim
    bs = types.ModuleType("bitstring")
    bs.BitArray = bitstring_shim.BitArray
    sys.modules["bitstring"] = bs
    cachetools = types.ModuleType("cachetools")

    class LRUCache(dict):
        def __init__(self, maxsize=None):
            super().__init__()
    cachetools.LRUCache = LRUCache
    sys.modules["cachetools"] = cachetools
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REPO, "oracle"))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def key_f2o(pos):
    return int(pos) & 0xFFFFFFFFFFFFFFFF


def key_ttt_str(pos):
    digit = {"_": 0, "X": 1, "O": 2}
    return sum(digit[ch] * 3 ** i for i, ch in enumerate(pos))


def key_ttt_np(state):
    return sum(int(state[x][y]) * 3 ** (x + 3 * y) for x in range(3) for y in range(3))


def key_bits(nkeep):
    def k(pos):
        raw = pos.encode("ISO-8859-1")
        v = int.from_bytes(raw, "big")
        return v >> (8 * len(raw) - nkeep)
    return k


def key_blake8(pos):
    import hashlib
    return int.from_bytes(hashlib.blake2b(pos.encode("ISO-8859-1"), digest_size=8).digest(), "big")


# tests/plugins/othello8_endgame.py's root: the reference's default 8x8 board after a fixed
# random playout from the start (seed 5), 10 empty squares left
OTHELLO8_ENDGAME_HEX = "303800204018057a4646bfdebfe6fa800200"


def othello8_endgame(canonical, ref_utils, roots):
    oth = _load("game_module", os.path.join(REF, "test_games/othello_bit_new.py"))   # 8x8 as shipped
    ref_utils.game_module = oth
    assert (oth.length, oth.height) == (8, 8)
    root = bytes.fromhex(OTHELLO8_ENDGAME_HEX).decode("latin-1")
    t0 = time.time()
    table, positions = canonical.solve(oth, root)
    save_table("othello_8x8_endgame", table, positions, key_blake8,
               {"game": "othello_bit_new", "dims": [8, 8], "root_hex": OTHELLO8_ENDGAME_HEX, "key": "blake2b-8"})
    v, r = table[canonical.default_key(root)]
    roots["othello_8x8_endgame"] = {"root_hex": OTHELLO8_ENDGAME_HEX, "canonical": canonical.root_line(v, r),
                                    "positions": len(table), "seconds": round(time.time() - t0, 1)}


# ---- Othello 8x8 beyond the 10-empty table: playouts and reference summaries ---------------
# (--only othello8-playouts / othello8-reference; words, tier and fold: othello8_words.py)
OTHELLO8_PLAYOUT_SEED, OTHELLO8_PLAYOUT_GAMES = 0, 50
# tests/test_gpu_othello8.py ROOT12 (the seed-5 playout at 12 empties), and three roots of 9 to
# 11 empties from other playouts: (seed, empties) of _othello8_playout_root
OTHELLO8_ROOT12_HEX = "30380028503841784646bfd6afc6be000200"
OTHELLO8_PASS_ROOTS = {"pass_e9": (21, 9), "pass_e10": (22, 10), "pass_e11": (23, 11)}


def _oth8(ref_utils):
    oth = _load("game_module", os.path.join(REF, "test_games/othello_bit_new.py"))   # 8x8 as shipped
    ref_utils.game_module = oth
    assert (oth.length, oth.height) == (8, 8)
    return oth


def _oth8_empties(pos):
    b = pos.encode("ISO-8859-1")
    return 64 - bin(int.from_bytes(b[0:8], "big") | int.from_bytes(b[8:16], "big")).count("1")


def _othello8_playout_root(oth, seed, empties):
    """The position with `empties` empty squares of the uniform random playout `seed`."""
    import random
    rng = random.Random(seed)
    p = oth.initial_position()
    while _oth8_empties(p) > empties:
        assert oth.primitive(p) == 4, "playout %d ended above %d empties" % (seed, empties)
        ms = oth.gen_moves(p)
        p = oth.do_move(p, ms[rng.randrange(len(ms))])
    assert oth.primitive(p) == 4
    return p


def _flip_directions(parent, child):
    """Directions in which the move parent -> child flipped discs (0 for a pass)."""
    a, b = parent.encode("ISO-8859-1"), child.encode("ISO-8859-1")
    occ = lambda s: int.from_bytes(s[0:8], "big") | int.from_bytes(s[8:16], "big")
    placed = occ(a) ^ occ(b)
    if not placed:
        return 0
    j0 = 63 - (placed.bit_length() - 1)          # string bit j = 8y + x
    flipped = (int.from_bytes(a[0:8], "big") ^ int.from_bytes(b[0:8], "big")) & occ(a)
    dirs = set()
    for j in range(64):
        if (flipped >> (63 - j)) & 1:
            dx, dy = j % 8 - j0 % 8, j // 8 - j0 // 8
            assert dx == 0 or dy == 0 or abs(dx) == abs(dy)
            dirs.add(((dx > 0) - (dx < 0), (dy > 0) - (dy < 0)))
    return len(dirs)


def othello8_playouts(ref_utils, seed=OTHELLO8_PLAYOUT_SEED, games=OTHELLO8_PLAYOUT_GAMES):
    """othello_8x8_playouts.npz: every distinct position the seeded random playouts of the
    reference plugin visit from its 8x8 start, with primitive() and, for non-primitive
    positions, the children do_move(p, m) for m in gen_moves(p), in that order (CSR).
    Even games move uniformly at random; odd games squeeze the opponent's mobility three moves
    in four, because uniform play passes above 20 empties about once in 800 games."""
    import random
    oth = _oth8(ref_utils)
    rng = random.Random(seed)
    t0 = time.time()
    index, pos, prim, kids = {}, [], [], []
    cover = {"games": games, "seed": seed, "non_primitive": 0, "pass_positions": 0,
             "pass_positions_20_empties": 0, "games_ended_by_second_pass_with_empties": 0,
             "terminal_win": 0, "terminal_loss": 0, "terminal_tie": 0, "max_flip_directions": 0,
             "moves_flipping_4_directions": 0}
    for g in range(games):
        p = oth.initial_position()
        while True:
            i = index.get(p)
            if i is None:
                i = index[p] = len(pos)
                pr = oth.primitive(p)
                ch = []
                if pr == 4:
                    ms = oth.gen_moves(p)
                    ch = [oth.do_move(p, m) for m in ms]
                    cover["non_primitive"] += 1
                    if ms == [None]:
                        cover["pass_positions"] += 1
                        cover["pass_positions_20_empties"] += _oth8_empties(p) >= 20
                    for c in ch:
                        d = _flip_directions(p, c)
                        cover["max_flip_directions"] = max(cover["max_flip_directions"], d)
                        cover["moves_flipping_4_directions"] += d >= 4
                else:
                    cover[{0: "terminal_win", 1: "terminal_loss", 2: "terminal_tie"}[pr]] += 1
                pos.append(p)
                prim.append(pr)
                kids.append(ch)
            if prim[i] != 4:
                if ord(p[17]) >= 2 and _oth8_empties(p) > 0:
                    cover["games_ended_by_second_pass_with_empties"] += 1
                break
            ch = kids[i]
            if g % 2 and rng.random() < 0.75:
                # squeeze: the child whose mover has the fewest moves (a pass counts as none)
                mob = [0 if oth.primitive(c) != 4 or oth.gen_moves(c) == [None] else len(oth.gen_moves(c))
                       for c in ch]
                p = ch[mob.index(min(mob))]
            else:
                p = ch[rng.randrange(len(ch))]
    assert cover["non_primitive"] >= 2000, cover
    assert cover["pass_positions_20_empties"] >= 5, cover
    assert cover["games_ended_by_second_pass_with_empties"] >= 1, cover
    assert min(cover["terminal_win"], cover["terminal_loss"], cover["terminal_tie"]) >= 1, cover
    assert cover["moves_flipping_4_directions"] >= 1, cover
    cover["seconds"] = round(time.time() - t0, 1)
    enc = lambda ps: np.frombuffer(b"".join(q.encode("ISO-8859-1") for q in ps), dtype=np.uint8).reshape(-1, 18)
    off = np.zeros(len(pos) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(c) for c in kids])
    path = os.path.join(HERE, "othello_8x8_playouts.npz")
    np.savez_compressed(path, positions=enc(pos), primitive=np.array(prim, dtype=np.uint8), child_off=off,
                        children=enc([c for ch in kids for c in ch]),
                        meta=json.dumps({"game": "othello_bit_new", "dims": [8, 8], **cover}))
    size = os.path.getsize(path)
    print("othello_8x8_playouts: %d positions, %d children, %d bytes" % (len(pos), off[-1], size))
    print(json.dumps(cover, indent=1))
    assert size <= 512 * 1024, size


def othello8_reference(canonical, ref_utils, names=None):
    """othello_8x8_reference.json: per root, the canonical solve over the reference plugin
    summarised as count, root record, per-tier counts (index = tier - root's tier, tier =
    3 * discs + pass count) and word_digest.  Entries not named are kept."""
    import othello8_words as ow
    sys.path.insert(0, os.path.dirname(HERE))
    from conftest import digest
    oth = _oth8(ref_utils)
    path = os.path.join(HERE, "othello_8x8_reference.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    roots = {"e12": bytes.fromhex(OTHELLO8_ROOT12_HEX).decode("latin-1")}
    for name, (seed, empties) in OTHELLO8_PASS_ROOTS.items():
        roots[name] = _othello8_playout_root(oth, seed, empties)
    for name in names or list(roots):
        root = roots[name]
        t0 = time.time()
        table, positions = canonical.solve(oth, root)
        words = ow.words_array(positions[k] for k in table)
        recs = np.array([(v << 14) | r for v, r in table.values()], dtype=np.uint16)
        del positions
        tr = ow.tiers(words)
        tier0 = int(ow.tiers(ow.words_array([root]))[0])
        passbyte = (words[:, 0] & np.uint64(0xFF)).astype(np.int64)
        v, r = table[canonical.default_key(root)]
        e = {"root_hex": root.encode("latin-1").hex(), "empties": _oth8_empties(root), "positions": len(table),
             "root_record": (v << 14) | r, "root_tier": tier0,
             "per_tier": [int(x) for x in np.bincount(tr - tier0)],
             "word_digest": digest(ow.fold(words), recs),
             # a position with pass byte 1 is a pass the game goes on from (it is expanded: the
             # mover, kept by the pass, has no move either); pass byte 2 ends the game, and the
             # board is never full there
             "passes_continued": int((passbyte == 1).sum()), "double_pass_terminals": int((passbyte == 2).sum()),
             "seconds": round(time.time() - t0, 1)}
        if name in OTHELLO8_PASS_ROOTS:
            e["playout_seed"] = OTHELLO8_PASS_ROOTS[name][0]
            assert e["passes_continued"] >= 1 and e["double_pass_terminals"] >= 1, e
        del table
        out[name] = e
        print(name, json.dumps(e), flush=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)


def save_table(name, table, positions, keyfn, meta):
    keys = np.empty(len(table), dtype=np.uint64)
    recs = np.empty(len(table), dtype=np.uint16)
    for i, (k, (v, r)) in enumerate(table.items()):
        keys[i] = keyfn(positions[k])
        recs[i] = (v << 14) | r
    order = np.argsort(keys, kind="stable")
    keys, recs = keys[order], recs[order]
    if len(np.unique(keys)) != len(keys):
        raise SystemExit("%s: key collision" % name)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), keys=keys, records=recs,
                        meta=json.dumps(meta))
    vals = recs >> 14
    print("%-14s %9d positions  W %d  L %d  T %d" % (
        name, len(keys), (vals == 0).sum(), (vals == 1).sum(), (vals == 2).sum()))
    return keys, recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--live", action="store_true")
    ap.add_argument("--skip-big", action="store_true")
    ap.add_argument("--only", choices=("othello8", "othello8-playouts", "othello8-reference"), default=None)
    ap.add_argument("--seed", type=int, default=OTHELLO8_PLAYOUT_SEED, help="othello8-playouts: rng seed")
    ap.add_argument("--games", type=int, default=OTHELLO8_PLAYOUT_GAMES, help="othello8-playouts: games")
    ap.add_argument("--roots", nargs="*", default=None, help="othello8-reference: entries to (re)solve")
    args = ap.parse_args()
    _install_stubs()
    import canonical
    import src.utils as ref_utils

    if args.only == "othello8-playouts":
        return othello8_playouts(ref_utils, args.seed, args.games)
    if args.only == "othello8-reference":
        return othello8_reference(canonical, ref_utils, args.roots)

    roots = {}
    if args.only == "othello8":
        path = os.path.join(HERE, "roots.json")
        roots = json.load(open(path))
        othello8_endgame(canonical, ref_utils, roots)
        with open(path, "w") as f:
            json.dump(roots, f, indent=1, sort_keys=True)
        print(json.dumps(roots["othello_8x8_endgame"], indent=1))
        return

    def root_line(table, positions, root, keyfn=None):
        v, r = table[canonical.default_key(root)]
        return canonical.root_line(v, r)

    # ---- Four-To-One (config 1) and the four golden roots --------------------
    f2o = _load("game_module", os.path.join(REF, "test_games/four_to_one.py"))
    ref_utils.game_module = f2o
    f2o_roots = _load("custom_f2o", os.path.join(REF, "game_tests/four_to_one_init_pos.py"))
    expect_f2o = {"four": (None, "WIN in 3 moves"), "six": ("six", "LOSS in 4 moves"),
                  "one": ("one", "WIN in 1 moves"), "zero": ("zero", "LOSS in 0 moves")}
    for case, (attr, expected) in expect_f2o.items():
        root = f2o.initial_position() if attr is None else getattr(f2o_roots, attr)()
        table, positions = canonical.solve(f2o, root)
        save_table("four_to_one_%s" % case, table, positions, key_f2o,
                   {"game": "four_to_one", "root": root})
        roots["four_to_one/%s" % case] = {
            "root": root, "canonical": root_line(table, positions, root),
            "reference_test_expects": expected,
            "test": "game_tests/four_to_one_test.py::test_%s" % case}

    # ---- mttt (config 2 twin) + the five golden roots ------------------------
    mttt = _load("game_module", os.path.join(REF, "test_games/mttt.py"))
    ref_utils.game_module = mttt
    mttt_roots = _load("custom_mttt", os.path.join(REF, "game_tests/mttt_test_init_pos.py"))
    table, positions = canonical.solve(mttt)
    ttt_keys, ttt_recs = save_table("ttt", table, positions, key_ttt_str,
                                    {"game": "mttt", "root": mttt.initial_position()})
    expect_mttt = {"blank": (None, "TIE in 9 moves"), "tie_in_one": ("tie_in_one", "TIE in 1 moves"),
                   "win_in_one": ("win_in_one", "WIN in 1 moves"),
                   "side_columns": ("side_columns", "TIE in 3 moves"),
                   "one_row": ("one_row", "TIE in 3 moves")}
    for case, (attr, expected) in expect_mttt.items():
        root = mttt.initial_position() if attr is None else getattr(mttt_roots, attr)()
        t2, p2 = canonical.solve(mttt, root)
        roots["mttt/%s" % case] = {
            "root": root, "root_key": key_ttt_str(root), "positions": len(t2),
            "canonical": root_line(t2, p2, root), "reference_test_expects": expected,
            "test": "game_tests/mttt_test.py::test_%s" % case}
        if case != "blank":
            save_table("mttt_%s" % case, t2, p2, key_ttt_str, {"game": "mttt", "root": root})

    # ---- tic_tac_toe_np (config 2) -----------------------------------------
    ttt_np = _load("game_module", os.path.join(REF, "test_games/tic_tac_toe_np.py"))
    ref_utils.game_module = ttt_np
    table, positions = canonical.solve(ttt_np)
    k2, r2 = save_table("ttt_np", table, positions, key_ttt_np, {"game": "tic_tac_toe_np"})
    if not (np.array_equal(k2, ttt_keys) and np.array_equal(r2, ttt_recs)):
        raise SystemExit("mttt and tic_tac_toe_np tables differ")

    # ---- Othello 4x4 (config 4) ---------------------------------------------
    oth = _load("game_module", os.path.join(REF, "test_games/othello_bit_new.py"))
    ref_utils.game_module = oth
    oth.length, oth.height = 4, 4
    oth.area = 16
    t0 = time.time()
    table, positions = canonical.solve(oth)
    root = oth.initial_position()
    save_table("othello_4x4", table, positions, key_bits(48),
               {"game": "othello_bit_new", "dims": [4, 4], "root_hex": root.encode("latin-1").hex()})
    roots["othello_4x4"] = {"root_hex": root.encode("latin-1").hex(),
                            "canonical": root_line(table, positions, root),
                            "positions": len(table), "seconds": round(time.time() - t0, 1)}

    # ---- Toot-and-Otto (config 3, small boards) ------------------------------
    toot = _load("game_module", os.path.join(REF, "test_games/toot_and_otto_bitstring.py"))
    ref_utils.game_module = toot
    toot_dims = [(3, 3), (4, 3)] if not args.skip_big else [(3, 3)]
    for (L, H) in toot_dims:
        toot.length, toot.height, toot.area = L, H, L * H
        t0 = time.time()
        table, positions = canonical.solve(toot)
        root = toot.initial_position()
        name = "toot_%dx%d" % (L, H)
        save_table(name, table, positions, key_bits(2 * L * H + 16),
                   {"game": "toot_and_otto_bitstring", "dims": [L, H],
                    "root_hex": root.encode("latin-1").hex()})
        roots[name] = {"root_hex": root.encode("latin-1").hex(),
                       "canonical": root_line(table, positions, root),
                       "positions": len(table), "seconds": round(time.time() - t0, 1)}

    othello8_endgame(canonical, ref_utils, roots)

    with open(os.path.join(HERE, "roots.json"), "w") as f:
        json.dump(roots, f, indent=1, sort_keys=True)
    print(json.dumps(roots, indent=1, sort_keys=True))

    if args.live:
        import live_reference
        out = live_reference.run_all(_load, canonical, ref_utils)
        with open(os.path.join(HERE, "live.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
        print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
