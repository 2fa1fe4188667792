#!/usr/bin/env python3
"""Drop-in for the reference's ``solve_local.py``: one process, one line of output.

    python solve_local.py GAME_FILE [--custom FILE --init_pos NAME] [--dims LxH] [--connect K] [--remoteness] [--analysis] [--verify]
                          [--loopy] [--load DIR] [--find SPEC ...] [--find-cap N] [--line] [--moves]
                          [--strategy [best|first]]

The reference (solve_local.py:4-72) loads the plugin by path, solves it in one
process and prints "Winning position", "Losing position", "Tie" or "Draw"
(:29-40).  As committed it prints "Draw" for every game: its result constants
are strings while plugins return src.utils ints (:6), and its TIE
branch tests LOSS twice (:34).  This drop-in prints the message the reference
intends for the root's canonical value, computed on the GPU by libgmsolve.so;
``--remoteness`` adds the launcher's "<V> in <R> moves" line, ``--analysis`` the table of
positions by value and remoteness (gamesmanmpi_amd/analysis.py), ``--verify`` the check of the
solved table against the game rules (gm_verify, gamesmanmpi_amd/verify.py: one line, then any
offending positions; the exit status is non-zero when the table is inconsistent).
``--find SPEC`` (repeatable) prints ``Found N positions: SPEC`` and up to ``--find-cap`` (16)
positions with that value and remoteness, selected on the device (gm_select,
gamesmanmpi_amd/find.py; a bad spec exits 2 before the solve), and ``--line`` the principal
variation from the root, one row per ply.  ``--moves`` prints ``Moves:`` and the root's moves, each
with its child position and value and a trailing `` *`` on every optimal one; with ``--find`` every
position found is followed by its own moves instead (gm_moves, gamesmanmpi_amd/moves.py).
``--strategy [best|first]`` prints, after the root line, how many positions can occur when the side
that does not lose at the root plays perfectly and the other plays anything (gm_reach,
gamesmanmpi_amd/reach.py), then the positions first reached per ply; ``first`` on a solve that stores
one representative per symmetry orbit says so and exits 1.
``--loopy`` solves a game in which positions can repeat (explicit graph, GM_OPT_LOOPY): "Draw"
is then a real answer, ``--remoteness`` prints ``DRAW`` alone for it and ``--analysis`` adds a
line ``Draw  N`` under its table.  ``--load DIR`` takes the place of the solve: the
``DIR/stats/<rank>/table.npz`` files of a ``solver_launcher.py -sd DIR`` run are loaded onto the
device (gm_import) and everything else answers for that table; refused with exit status 2 together
with ``--loopy`` or for a plugin solved as an explicit graph, and a table without the root prints
``root not in table`` on stderr and exits 1.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import solver_launcher  # noqa: E402

MESSAGES = {0: "Winning position", 1: "Losing position", 2: "Tie", 3: "Draw"}


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("game_file")
    p.add_argument("--custom")
    p.add_argument("--init_pos")
    p.add_argument("--dims")
    p.add_argument("--connect", type=int, metavar="K")
    p.add_argument("--heaps", type=int)
    p.add_argument("--remoteness", action="store_true")
    p.add_argument("--analysis", action="store_true")
    p.add_argument("--verify", action="store_true")
    p.add_argument("--find", action="append", metavar="SPEC", default=[],
                   help="name the positions with a value and remoteness: VALUE[,VALUE...][:R | :LO-HI | :max]")
    p.add_argument("--find-cap", type=int, default=16, metavar="N")
    p.add_argument("--line", action="store_true", help="print the principal variation from the root")
    p.add_argument("--moves", action="store_true",
                   help="print the root's moves with their values, or with --find the moves of every position found")
    p.add_argument("--strategy", nargs="?", const="best", choices=("best", "first"), metavar="best|first",
                   help="print how many positions can occur when the side that does not lose at the root plays perfectly")
    p.add_argument("--loopy", action="store_true")
    p.add_argument("--load", metavar="DIR",
                   help="in place of the solve, load the table.npz files a solver_launcher.py -sd DIR run wrote")
    p.add_argument("--device", type=int, default=-1)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    args.engine = "auto"
    if args.load and args.loopy:
        print("--load and --loopy exclude each other: a stored table loads into a descriptor game, a loopy solve is "
              "an explicit graph", file=sys.stderr)
        return 2
    try:
        specs = solver_launcher.find_specs(args)
    except ValueError as e:
        print("--find: %s" % e, file=sys.stderr)
        return 2
    game, root = solver_launcher.prepare_game(args)
    from gamesmanmpi_amd import Solver, _lib
    s = Solver(game, root, device=args.device, loopy=True) if args.loopy else Solver(game, root, device=args.device)
    if args.load:
        if s.codec.game_id == _lib.GAME_GRAPH:
            print("--load needs a game with a device descriptor: %s is solved as an explicit graph, whose keys a "
                  "stored table does not carry" % args.game_file, file=sys.stderr)
            s.close()
            return 2
        try:
            s.load_statsdir(args.load)
            refused = None
        except _lib.GMError as e:   # a table gm_import refuses (a key twice, orbit mates that disagree, ...)
            refused = "--load %s: %s" % (args.load, e)
        if refused or s.value is None:
            print(refused or "root not in table", file=sys.stderr)
            s.close()
            return 1
    else:
        s.solve()
    print(MESSAGES[s.value])
    if args.remoteness:
        print(s.root_line())
    if args.strategy and not solver_launcher.write_strategy(s, args.strategy, sys.stdout):
        s.close()
        return 1
    if args.analysis:
        from gamesmanmpi_amd import analysis
        print(analysis.format_table(s.analysis()))
        if args.loopy:
            print("Draw  %d" % s.draw_count())
    if specs:
        from gamesmanmpi_amd import find
        find.report(s, specs, max(0, args.find_cap), sys.stdout, moves=args.moves)
    if args.line:
        solver_launcher.write_line(s, sys.stdout)
    status = 0
    if args.verify:
        from gamesmanmpi_amd import verify
        status = 0 if verify.report(s, sys.stdout) else 1
    if args.moves and not specs:
        solver_launcher.write_moves(s, sys.stdout)
    s.close()
    return status


if __name__ == "__main__":
    sys.exit(main())
