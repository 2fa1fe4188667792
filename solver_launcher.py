#!/usr/bin/env python3
"""Drop-in for the reference's ``solver_launcher.py`` (GamesmanMPI), solving on MI355X.

    python solver_launcher.py GAME_FILE [--debug] [-sd DIR] [--custom FILE --init_pos NAME] [--cp]
    python -m torch.distributed.run --nproc-per-node N solver_launcher.py GAME_FILE ...

Same arguments and the same single stdout line as the reference
(``"<WIN|LOSS|TIE> in <R> moves"``, printed by the root rank,
reference src/new_process.py:47-52).  The reference's flags are at
solver_launcher.py:9-41; the plugin is loaded by path and published as
``src.utils.game_module`` (:56-57) and checked with ``validate`` (:70-81).

Differences, on purpose:
* ``--custom/--init_pos`` takes effect (the reference freezes the root at import,
  src/game_state.py:15, so it silently ignores them -- SURVEY §0.3);
* the solve runs in libgmsolve.so on the GPU; ranks come from
  torch.distributed.run's environment instead of mpiexec.  With one GPU per rank
  the ranks shard the solve (RCCL); with more ranks than GPUs -- the reference's
  own tests run ``mpiexec --oversubscribe -n 2`` on one host
  (game_tests/four_to_one_test.py:20) -- rank 0 solves for all of them, running
  the same sharded algorithm over ``world`` loopback ranks on its GPU, and the
  other ranks wait at a barrier and exit 0.  Either way the root line is printed
  once.  Values and remoteness are the canonical ones;
* ``-sd DIR`` writes the solved table in the reference's layout -- shelve
  databases ``DIR/stats/<rank>/resolved`` and ``remote`` keyed by ``str(pos)``,
  each position on rank ``md5(str(pos)) % world`` (src/cache_dict.py:19-42,
  gamesmanmpi_amd/persist.py) -- and as ``DIR/stats/<rank>/table.npz`` (sorted
  u64 keys + u16 records); ``--sd-format`` picks one (shelves are written for
  tables of up to 2 million positions unless asked for explicitly);
* extras: ``--dims LxH`` patches board plugins' ``length``/``height``, ``--connect K``
  the connect4 plugin's ``connect``, ``--heaps`` patches the subtraction plugin, ``--engine``, ``--device``, ``--stats``;
* ``--analysis`` prints, after the root line, the whole solve's positions by value and
  remoteness (gm_histogram, gamesmanmpi_amd/analysis.py); with ``-sd DIR`` rank 0 also
  writes them to ``DIR/stats/analysis.json``;
* ``--verify`` checks the solved table against the game rules on the device (gm_verify,
  gamesmanmpi_amd/verify.py) and prints ``Verified N positions: consistent`` -- or the
  counts by class and up to 16 offending positions with their moves -- after the root line;
  the exit status is non-zero when anything is inconsistent, and with ``-sd DIR`` rank 0
  writes ``DIR/stats/verify.json``.  Ranks that share one solve on rank 0 verify as one
  process does; a solve sharded over processes is refused before it starts, since no rank
  holds the tables of its children's owners;
* ``--find SPEC`` (repeatable) names the positions behind a statistic: after the root line (and
  the ``--analysis`` table) it prints ``Found N positions: SPEC`` and up to ``--find-cap`` (16)
  positions with their records, ascending by key, selected on the device (gm_select,
  gamesmanmpi_amd/find.py).  SPEC is ``VALUE[,VALUE...][:R | :LO-HI | :max]`` with values win,
  loss, tie, draw; a bad spec exits 2 before the solve.  Sharded ranks each select among their
  own keys and rank 0 prints the merged result; with ``-sd DIR`` rank 0 writes
  ``DIR/stats/find.json``;
* ``--line`` prints ``Line:`` and the principal variation from the root, one row per ply
  (``  K. <move> -> <position>: TIE in 8``); like ``--verify`` it needs the whole table in one
  process and is refused (exit status 2) when the solve is sharded over processes;
* ``--moves`` prints ``Moves:`` and one line per move of the root (``  <move> -> <child position>:
  <VALUE> in <R>``, a trailing `` *`` on every optimal move) after everything above; together
  with ``--find`` every position found is followed by its own moves instead, indented two more
  spaces, all of them valued by one device call (gm_moves, gamesmanmpi_amd/moves.py).  A solve
  sharded over processes goes ahead without the moves and says so in one line on stderr: no
  rank holds the whole table (``--load DIR`` of its ``-sd`` output does);
* ``--strategy [best|first]`` prints, right after the root line, ``Strategy for the <side> (root
  <root line>): N of TOTAL positions (S%), deepest ply D`` and one line ``  ply K: COUNT`` per ply:
  the positions that can occur when the side that does not lose at the root plays perfectly
  (``best``: every optimal move, ``first``: the one move the solver plays) and the other side
  plays anything, found on the device (gm_reach, gamesmanmpi_amd/reach.py).  ``first`` on a solve
  that stores one representative per symmetry orbit says so on stderr and exits 1; a solve
  sharded over processes is refused (exit status 2).  Combines with ``--loopy`` and ``--load``
  as ``--moves`` does;
* ``--loopy`` is for games in which a position can repeat: the plugin is enumerated on the
  host and solved as an explicit graph with cycles allowed (GM_OPT_LOOPY, one process); a
  position neither side can decide is a draw, the root line of a drawn root is ``DRAW``
  alone, ``--analysis`` adds a line ``Draw  N`` under its table and ``analysis.json`` a key
  ``"draw"``;
* ``--load DIR`` takes the place of the solve: every ``DIR/stats/<rank>/table.npz`` (what ``-sd``
  wrote, one share per rank of a sharded solve) is loaded onto the device (gm_import), the root
  line is printed from the stored root record, and ``--analysis``, ``--verify``, ``--stats`` and
  ``-sd`` behave as after a solve -- which is how a solve sharded over processes is verified.
  A table without the root prints ``root not in table`` on stderr and exits 1.  Refused (exit
  status 2, one line on stderr) together with ``--loopy``, for a plugin solved as an explicit
  graph, and when the ranks would shard (one GPU per rank); ranks that share rank 0's GPU let
  rank 0 load.
"""
import argparse
import cProfile
import importlib.util
import json
import logging
import os
import sys

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import src.utils  # noqa: E402


SHELVE_AUTO_LIMIT = 2_000_000


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("game_file", help="Game to solve for.")
    p.add_argument("--debug", help="Enables or disables logging.", action="store_true")
    p.add_argument("-sd", "--statsdir", help="Location to store statistics about game.", action="store")
    p.add_argument("--custom", help="Specifies custom file to modify provided game file.")
    p.add_argument("--init_pos", help="Initial position to start at for the game. "
                   "If none is specified, the default is used.")
    p.add_argument("--cp", action="store_true")
    p.add_argument("--dims", help="board plugins: LxH (sets the module's length/height)")
    p.add_argument("--connect", type=int, metavar="K", help="connect4 plugin: stones in a row that win (sets the module's connect)")
    p.add_argument("--heaps", type=int, help="subtraction plugin: number of heaps")
    p.add_argument("--engine", choices=("auto", "dense", "sparse"), default="auto")
    p.add_argument("--device", type=int, default=None)
    p.add_argument("--stats", action="store_true", help="print solve statistics (JSON) to stderr")
    p.add_argument("--analysis", action="store_true",
                   help="after the root line, print the positions by value and remoteness")
    p.add_argument("--verify", action="store_true",
                   help="after the root line, check the solved table against the game rules on the device")
    p.add_argument("--find", action="append", metavar="SPEC", default=[],
                   help="after the root line, name the positions with a value and remoteness: "
                        "VALUE[,VALUE...][:R | :LO-HI | :max] (repeatable)")
    p.add_argument("--find-cap", type=int, default=16, metavar="N", help="positions printed per --find (default 16)")
    p.add_argument("--line", action="store_true", help="after the root line, print the principal variation from the root")
    p.add_argument("--moves", action="store_true",
                   help="print the root's moves with their values, or with --find the moves of every position found")
    p.add_argument("--strategy", nargs="?", const="best", choices=("best", "first"), metavar="best|first",
                   help="print how many positions can occur when the side that does not lose at the root plays "
                        "perfectly (best: every optimal move; first: the one move the solver plays)")
    p.add_argument("--loopy", action="store_true",
                   help="solve a game with cycles: explicit graph, undecidable positions are DRAW")
    p.add_argument("--load", metavar="DIR",
                   help="in place of the solve, load the table.npz files a run with -sd DIR wrote")
    p.add_argument("--sd-format", choices=("auto", "npz", "reference", "both"), default="auto",
                   help="-sd output: npz table, the reference's shelve layout, or both (auto: both up to "
                        "%d positions, else npz)" % SHELVE_AUTO_LIMIT)
    return p


def load_module(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    if spec is None:
        raise FileNotFoundError(path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def validate(mod):
    """The four plugin functions must exist (reference solver_launcher.py:70-81)."""
    for attr in ("initial_position", "do_move", "gen_moves", "primitive"):
        if not hasattr(mod, attr):
            print("Could not find method", attr)
            raise AttributeError(attr)


def custom_root(game, custom_path, name):
    """Initial position from ``--custom FILE --init_pos NAME`` (reference :83-111)."""
    try:
        custom = load_module("custom", custom_path)
    except (FileNotFoundError, OSError):
        print("Custom file was not found. Using default initial position instead.")
        return None
    except AttributeError:
        print("Custom file with new initial position not specified. "
              "Using default initial position instead.")
        return None
    fn = getattr(custom, name, None)
    if fn is None:
        print("Initial position was not found in custom file. Using default initial position instead.")
        return None
    game.initial_position = fn
    return fn()


def prepare_game(args):
    game = load_module("game_module", args.game_file)
    src.utils.game_module = game
    if args.dims:
        L, H = (int(v) for v in args.dims.lower().split("x"))
        game.length, game.height = L, H
        if hasattr(game, "area"):
            game.area = L * H
    if getattr(args, "connect", None) is not None:
        game.connect = args.connect
    if args.heaps is not None:
        game.HEAPS = args.heaps
    validate(game)
    root = None
    if args.init_pos:
        root = custom_root(game, args.custom, args.init_pos)
    if root is None:
        root = game.initial_position()
    return game, root


def dist_env():
    return int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))


MAX_VIRTUAL_RANKS = 64   # GM_OPT_VIRTUAL_RANKS range (include/gmsolve.h)


def rank_plan(world, local_world, n_devices):
    """How `world` launcher ranks share the solve (the reference's mpiexec -n N).

    "solo"     one rank: it solves;
    "sharded"  one GPU per rank on one node: every rank joins the RCCL solve;
    "single"   more ranks than GPUs (mpiexec --oversubscribe): rank 0 solves for all,
               the others wait at a barrier and exit 0."""
    if world <= 1:
        return "solo"
    if local_world == world and world <= n_devices:
        return "sharded"
    return "single"


def run(args, out=sys.stdout):
    rank, world, local = dist_env()
    if getattr(args, "load", None) and getattr(args, "loopy", False):
        print("--load and --loopy exclude each other: a stored table loads into a descriptor game, a loopy solve is "
              "an explicit graph", file=sys.stderr)
        return 2
    try:
        find_specs(args)
    except ValueError as e:
        print("--find: %s" % e, file=sys.stderr)
        return 2
    if args.debug:
        os.makedirs("logs", exist_ok=True)
        logging.basicConfig(filename="logs/proc%d" % rank, level=logging.DEBUG)
    game, root = prepare_game(args)

    from gamesmanmpi_amd import Solver, _lib
    plan = "solo"
    if world > 1:
        from gamesmanmpi_amd import dist
        dist.init_group()
        plan = dist.broadcast(rank_plan(world, int(os.environ.get("LOCAL_WORLD_SIZE", world)),
                                        _lib.lib().gm_device_count()) if rank == 0 else None)
        logging.debug("rank %d of %d: %s", rank, world, plan)
        if plan == "sharded" and getattr(args, "verify", False):
            if rank == 0:
                print("--verify needs the whole table in one process: this solve is sharded over %d processes, and "
                      "a rank does not hold the tables of its children's owners.  Run it on one process (virtual "
                      "ranks included)." % world, file=sys.stderr)
            return 2
        if plan == "sharded" and getattr(args, "line", False):
            if rank == 0:
                print("--line needs the whole table in one process: this solve is sharded over %d processes.  Run it "
                      "on one process (virtual ranks included)." % world, file=sys.stderr)
            return 2
        if plan == "sharded" and getattr(args, "moves", False):
            # no refusal: the solve and everything else asked for go ahead without the moves
            if rank == 0:
                print("--moves needs the whole table in one process: this solve is sharded over %d processes; solve "
                      "with -sd DIR, then ask for the moves of the stored table (--load DIR)" % world, file=sys.stderr)
            args.moves = False
        if plan == "sharded" and getattr(args, "strategy", None):
            if rank == 0:
                print("--strategy needs the whole table in one process: this solve is sharded over %d processes.  Run "
                      "it on one process (virtual ranks included)." % world, file=sys.stderr)
            return 2
        if plan == "sharded" and getattr(args, "load", None):
            if rank == 0:
                print("--load builds the whole table in one process: run it on one process, or with more ranks than "
                      "GPUs (rank 0 then loads)", file=sys.stderr)
            return 2
        if plan == "single" and rank != 0:
            # rank 0 solves for every rank and prints the root line; wait for it by polling
            # the group's store (a barrier would time out under a solve longer than the
            # group timeout)
            return dist.wait_for_root()
    if plan == "single":
        try:
            return _solve_and_report(args, game, root, rank, world, local, plan, out)
        except BaseException:
            dist.release_waiters(world, ok=False)
            raise
    return _solve_and_report(args, game, root, rank, world, local, plan, out)


def _solve_and_report(args, game, root, rank, world, local, plan, out):
    from gamesmanmpi_amd import Solver, _lib
    if world > 1:
        from gamesmanmpi_amd import dist
    engine = {"auto": None, "dense": _lib.ENGINE_DENSE, "sparse": _lib.ENGINE_SPARSE}[args.engine]
    device = args.device if args.device is not None else (local if plan == "sharded" else -1)
    loopy = getattr(args, "loopy", False)
    if loopy and plan == "sharded":
        raise SystemExit("--loopy solves in one process: the graph engine is not sharded")
    solver = Solver(game, root, device=device, engine=engine, loopy=True) if loopy else \
        Solver(game, root, device=device, engine=engine)
    load = getattr(args, "load", None)
    if load and solver.codec.game_id == _lib.GAME_GRAPH:
        print("--load needs a game with a device descriptor: %s is solved as an explicit graph, whose keys a stored "
              "table does not carry" % args.game_file, file=sys.stderr)
        solver.close()
        if plan == "single":
            dist.release_waiters(world, ok=False)
        return 2
    if plan == "sharded":
        dist.join(solver.ctx, rank, world)
    elif load:
        pass   # one context holds the whole table: no virtual ranks
    elif plan == "single" and solver.codec.game_id != _lib.GAME_GRAPH and world <= MAX_VIRTUAL_RANKS:
        # the sharded algorithm over `world` loopback ranks on this one GPU
        solver.ctx.set_option(_lib.OPT_VIRTUAL_RANKS, world)
    logging.debug("solving %s from %r on device %s", args.game_file, root, device)
    if load:
        try:
            solver.load_statsdir(load)
            refused = None
        except _lib.GMError as e:   # a table gm_import refuses (a key twice, orbit mates that disagree, ...)
            refused = "--load %s: %s" % (load, e)
        if refused or solver.value is None:
            print(refused or "root not in table", file=sys.stderr)
            solver.close()
            if plan == "single":
                dist.release_waiters(world, ok=False)
            return 1
    elif args.cp:
        prof = cProfile.Profile()
        prof.runcall(solver.solve)
        prof.dump_stats("time")
    else:
        solver.solve()
    if rank == 0:
        out.write(solver.root_line() + "\n")
        out.flush()
    if getattr(args, "strategy", None) and rank == 0 and not write_strategy(solver, args.strategy, out):
        solver.close()
        if plan == "single":
            dist.release_waiters(world, ok=False)
        return 1
    if getattr(args, "analysis", False):
        report_analysis(args, solver, rank, world, plan, out)
    if find_specs(args):
        from gamesmanmpi_amd import find
        find.report(solver, find_specs(args), max(0, args.find_cap), out, args.statsdir, rank, world,
                    sharded=plan == "sharded", moves=getattr(args, "moves", False))
    if getattr(args, "line", False) and rank == 0:
        write_line(solver, out)
    status = 0
    if getattr(args, "verify", False) and rank == 0:
        from gamesmanmpi_amd import verify
        status = 0 if verify.report(solver, out, args.statsdir) else 1
    if getattr(args, "moves", False) and not find_specs(args) and rank == 0:
        write_moves(solver, out)
    if args.stats:
        st = solver.ctx.stats()
        st["rank"] = rank
        print(json.dumps(st), file=sys.stderr)
    if args.statsdir:
        write_statsdir(args, solver, rank, world, gather=plan == "sharded")
    solver.close()
    if plan == "single":
        dist.release_waiters(world)
    return status


def find_specs(args):
    """The parsed --find specs (ValueError, with the parser's message, for a bad one)."""
    texts = getattr(args, "find", None) or []
    if not texts:
        return []
    from gamesmanmpi_amd import find
    return [find.parse_spec(t) for t in texts]


def write_line(solver, out):
    """--line: the principal variation from the root, one row per ply."""
    from gamesmanmpi_amd.verify import _record_text
    out.write("Line:\n")
    for ply, (move, pos, value, remoteness) in enumerate(solver.line()):
        step = "" if move is None else "%r -> " % (move,)
        out.write("  %d. %s%r: %s\n" % (ply, step, pos, _record_text(value, remoteness)))
    out.flush()


def write_moves(solver, out):
    """--moves without --find: the root's moves, each with its child position and value, the
    optimal ones starred (gm_moves through Solver.annotate)."""
    from gamesmanmpi_amd import moves
    rows, _ = solver.annotate([solver.root])[0]
    for ln in moves.format_block(rows):
        out.write(ln + "\n")
    out.flush()


def write_strategy(solver, mode, out):
    """--strategy: the positions that can occur when the side that does not lose at the root
    plays perfectly and the other plays anything (gm_reach through Solver.strategy): one line,
    then the positions first reached per ply.  False when the table cannot answer: "first" on a
    solve that stores one representative per symmetry orbit."""
    from gamesmanmpi_amd import _lib, reach
    try:
        s = solver.strategy(first=mode == "first")
    except _lib.GMError as e:
        if e.code != -1:
            raise
        print("--strategy first follows one move per position, which the symmetry reduction of this solve does not "
              "preserve: rerun with the reduction off (GM_OPT_SYMMETRY 0), or ask for --strategy best",
              file=sys.stderr)
        return False
    side = "player to move" if s["side"] == "mover" else "opponent"
    for ln in reach.format_strategy(side, solver.root_line(), s, solver.n_positions, s["ply_counts"]):
        out.write(ln + "\n")
    out.flush()
    return True


def report_analysis(args, solver, rank, world, plan, out):
    """--analysis: the whole solve's histogram, printed by rank 0 (and written to
    DIR/stats/analysis.json with -sd DIR).  Sharded ranks each count their own keys and the
    arrays, padded to a common depth, are summed over the process group; a solo or single
    solve's context already holds every position."""
    from gamesmanmpi_amd import analysis
    hist = solver.analysis()
    if plan == "sharded" and world > 1:
        import torch.distributed as tdist
        parts = [None] * world
        tdist.all_gather_object(parts, hist)
        depth = max(p.shape[1] for p in parts)
        hist = sum(analysis.pad(p, depth) for p in parts)
    if rank != 0:
        return
    out.write(analysis.format_table(hist) + "\n")
    loopy = getattr(args, "loopy", False)
    if loopy:
        out.write("Draw  %d\n" % solver.draw_count())
    out.flush()
    if args.statsdir:
        path = os.path.join(args.statsdir, "stats", "analysis.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(analysis.as_json(hist), draw=solver.draw_count()) if loopy else analysis.as_json(hist),
                      f, indent=1)
            f.write("\n")


def write_statsdir(args, solver, rank, world, gather=True):
    """-sd DIR: this rank's npz table and/or the reference's shelve layout (rank 0
    writes every rank's shelves, gathering the sharded ranks' tables first; with
    gather False rank 0 holds the whole table)."""
    from gamesmanmpi_amd.persist import write_reference_tables
    from gamesmanmpi_amd.solver import dump_table
    keys, recs = solver.table()
    fmt = args.sd_format
    if fmt == "auto":
        total = solver.n_positions or len(keys)
        fmt = "both" if total <= SHELVE_AUTO_LIMIT else "npz"
        if fmt == "npz" and rank == 0:
            print("-sd: %d positions; writing table.npz only (--sd-format reference forces the shelves)" % total,
                  file=sys.stderr)
    if fmt in ("npz", "both"):
        dump_table(os.path.join(args.statsdir, "stats", str(rank), "table.npz"), keys, recs,
                   {"game": args.game_file, "codec": solver.codec.name, "params": solver.codec.params})
    if fmt in ("reference", "both"):
        if world > 1 and gather:
            import numpy as np
            import torch.distributed as tdist
            parts = [None] * world
            tdist.all_gather_object(parts, (keys, recs))
            keys = np.concatenate([p[0] for p in parts])
            recs = np.concatenate([p[1] for p in parts])
        if rank == 0:
            write_reference_tables(args.statsdir, solver.codec, keys, recs, world)


def main(argv=None):
    args = build_parser().parse_args(argv)
    return run(args)


if __name__ == "__main__":
    sys.exit(main())
