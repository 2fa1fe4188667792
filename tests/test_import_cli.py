"""``--load DIR`` of solver_launcher.py / solve_local.py and the reader behind it
(persist.read_npz_tables): a table written by ``-sd`` comes back onto the device (gm_import) and
the CLIs report on it as they do after a solve."""
import io
import os

import numpy as np
import pytest

from conftest import REPO

import solve_local  # noqa: E402
import solver_launcher  # noqa: E402
from gamesmanmpi_amd.persist import read_npz_tables  # noqa: E402
from gamesmanmpi_amd.solver import dump_table  # noqa: E402

TOOT = os.path.join(REPO, "test_games", "toot_and_otto_bitstring.py")


def _two_ranks(tmp_path, meta1=None):
    meta = {"game": "g.py", "codec": "toot_and_otto", "params": (4, 3)}
    k0, r0 = np.array([1, 5, 9], dtype=np.uint64), np.array([1, 2, 3], dtype=np.uint16)
    k1, r1 = np.array([2, 7], dtype=np.uint64), np.array([0x4001, 0x8002], dtype=np.uint16)
    dump_table(str(tmp_path / "stats" / "0" / "table.npz"), k0, r0, meta)
    dump_table(str(tmp_path / "stats" / "1" / "table.npz"), k1, r1, meta1 or meta)
    return meta, np.concatenate([k0, k1]), np.concatenate([r0, r1])


def test_read_npz_tables_round_trips_two_ranks(tmp_path):
    meta, keys, recs = _two_ranks(tmp_path)
    k, r, m = read_npz_tables(str(tmp_path))
    assert k.dtype == np.uint64 and r.dtype == np.uint16
    assert np.array_equal(k, keys) and np.array_equal(r, recs)   # rank order, each part as written
    assert m == meta


@pytest.mark.parametrize("other", [{"codec": "othello", "params": (4, 3)}, {"codec": "toot_and_otto", "params": (4, 4)}])
def test_read_npz_tables_refuses_parts_of_different_games(tmp_path, other):
    _two_ranks(tmp_path, dict(other, game="g.py"))
    with pytest.raises(ValueError):
        read_npz_tables(str(tmp_path))


def test_read_npz_tables_needs_a_table(tmp_path):
    with pytest.raises(FileNotFoundError):
        read_npz_tables(str(tmp_path))


def test_both_parsers_accept_load():
    assert solver_launcher.build_parser().parse_args(["g.py", "--load", "T"]).load == "T"
    assert solve_local.build_parser().parse_args(["g.py", "--load", "T"]).load == "T"
    assert solver_launcher.build_parser().parse_args(["g.py"]).load is None
    assert solve_local.build_parser().parse_args(["g.py"]).load is None


def test_load_with_loopy_is_refused_before_anything_runs(capsys, monkeypatch):
    # neither the plugin nor the library is touched: the game file does not exist
    monkeypatch.setattr(solver_launcher, "prepare_game", lambda args: pytest.fail("went on to load the plugin"))
    assert solver_launcher.main(["no_such_game.py", "--load", "T", "--loopy"]) == 2
    assert solve_local.main(["no_such_game.py", "--load", "T", "--loopy"]) == 2
    cap = capsys.readouterr()
    assert cap.out == "" and len(cap.err.splitlines()) == 2 and "--loopy" in cap.err


def _launch(argv):
    out = io.StringIO()
    status = solver_launcher.run(solver_launcher.build_parser().parse_args(argv), out=out)
    return status, out.getvalue()


@pytest.mark.gpu
def test_launcher_load_reports_as_a_solve_does(tmp_path, capsys):
    T = str(tmp_path / "T")
    game = [TOOT, "--dims", "4x3"]
    assert _launch(game + ["-sd", T, "--sd-format", "npz"])[0] == 0
    status, solved = _launch(game + ["--analysis", "--verify"])
    assert status == 0
    status, loaded = _launch(game + ["--load", T, "--analysis", "--verify"])
    assert status == 0
    assert loaded == solved
    lines = loaded.splitlines()
    assert lines[0].endswith("moves") and lines[-1].startswith("Verified ") and lines[-1].endswith(": consistent")
    capsys.readouterr()
    assert solve_local.main(game + ["--load", T, "--remoteness"]) == 0
    local = capsys.readouterr().out.splitlines()
    assert local[0] in solve_local.MESSAGES.values() and local[1] == lines[0]

    # one interior record changed in the file: --verify finds it, exit status 1
    from gamesmanmpi_amd import Context, _lib
    path = os.path.join(T, "stats", "0", "table.npz")
    with np.load(path) as z:
        keys, recs, meta = z["keys"], z["records"].copy(), str(z["meta"])
    def own_mirror(k):   # its own left-right mirror image (4x3: two planes of three 4-bit rows above the hands)
        planes = (int(k) >> 16) & 0xFFFFFF
        return all(int("{:04b}".format((planes >> s) & 15)[::-1], 2) == (planes >> s) & 15 for s in range(0, 24, 4))

    # (a position that is its own mirror image: the table then still loads under the symmetry
    # reduction, which wants one record per orbit, and it is gm_verify that objects)
    ctx = Context(_lib.GAME_TOOT, (4, 3), device=0)
    i = next(i for i in range(len(keys) // 2, len(keys))
             if own_mirror(keys[i]) and ctx.expand(int(keys[i]))[0] == 4)
    ctx.close()
    recs[i] = ((int(recs[i]) >> 14) + 1) % 3 << 14 | (int(recs[i]) & 0x3FFF)
    np.savez(path, keys=keys, records=recs, meta=meta)
    status, out = _launch(game + ["--load", T, "--verify"])
    assert status == 1 and "inconsistent" in out
