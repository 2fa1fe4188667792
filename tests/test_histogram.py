"""Value-by-remoteness analysis, host side (gamesmanmpi_amd/analysis.py): the numpy reference
`from_records` against a plain Python loop over the golden tables, the text table's round
trip, `summarize`, and the committed census of the 2^32-position game
(tests/golden/histograms.json, written by tests/golden/make_histograms.py from the C oracle).
The device side (gm_histogram) is tests/test_gpu_histogram.py.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

from gamesmanmpi_amd import analysis


def _loop(records, weights=None):
    """counts[value][remoteness] by a plain loop."""
    counts = {}
    for i, rec in enumerate(records.tolist()):
        key = (rec >> 14, rec & 0x3FFF)
        counts[key] = counts.get(key, 0) + (1 if weights is None else int(weights[i]))
    n_rem = 1 + max(r for _, r in counts)
    out = [[counts.get((v, r), 0) for r in range(n_rem)] for v in range(3)]
    return out


@pytest.mark.parametrize("name", ["ttt", "othello_4x4", "toot_4x3"])
def test_from_records_matches_a_plain_loop(name):
    keys, recs = golden(name)
    h = analysis.from_records(recs)
    assert h.dtype == np.uint64 and h.shape[0] == 3
    assert h.tolist() == _loop(recs)
    assert int(h.sum()) == len(recs)
    assert h.shape[1] == 1 + int((recs & 0x3FFF).max())


def test_from_records_weights_and_unsolved():
    keys, recs = golden("ttt")
    w = (np.arange(len(recs)) % 8 + 1).astype(np.uint64)
    h = analysis.from_records(recs, w)
    assert h.tolist() == _loop(recs, w) and int(h.sum()) == int(w.sum())
    # unsolved entries are skipped, with their weights
    r2 = recs.copy()
    r2[::3] = 0xFFFF
    keep = r2 != 0xFFFF
    assert analysis.from_records(r2, w).tolist() == analysis.pad(analysis.from_records(recs[keep], w[keep]), 0).tolist()
    assert analysis.from_records(np.zeros(0, np.uint16)).shape == (3, 0)
    with pytest.raises(ValueError):
        analysis.from_records(recs, w[:-1])


def test_format_table_round_trips_and_keeps_zero_rows():
    h = np.zeros((3, 6), dtype=np.uint64)
    h[0, 1], h[1, 0], h[2, 5], h[0, 5] = 16, 1, 12345678901, 7   # rows 2, 3, 4 are all zero
    text = analysis.format_table(h)
    lines = text.splitlines()
    assert lines[0].split() == ["Remoteness", "Win", "Lose", "Tie", "Total"]
    assert len(lines) == 1 + 6 + 1 and lines[-1].split()[0] == "Total"
    assert [ln.split() for ln in lines[3:6]] == [[str(r), "0", "0", "0", "0"] for r in (2, 3, 4)]
    assert len({len(ln) for ln in lines}) == 1   # fixed width
    assert lines[-1].split()[1:] == ["23", "1", "12345678901", "12345678925"]
    assert np.array_equal(analysis.parse_table(text), h)
    _, recs = golden("othello_4x4")
    g = analysis.from_records(recs)
    assert np.array_equal(analysis.parse_table(analysis.format_table(g)), g)
    empty = analysis.format_table(np.zeros((3, 0), dtype=np.uint64))
    assert analysis.parse_table(empty).shape == (3, 0)


def test_summarize_and_json():
    h = np.array([[0, 16, 0, 408, 0], [1, 0, 36, 0, 0], [0, 0, 0, 0, 0]], dtype=np.uint64)
    s = analysis.summarize(h)
    assert s == {"positions": 461, "n_remoteness": 5, "win": 424, "loss": 37, "tie": 0,
                 "max_remoteness_win": 3, "max_remoteness_loss": 2, "max_remoteness_tie": None}
    j = json.loads(json.dumps(analysis.as_json(h)))
    assert j["win_by_remoteness"] == [0, 16, 0, 408, 0] and j["loss_by_remoteness"] == [1, 0, 36, 0, 0]
    assert j["tie_by_remoteness"] == [0] * 5 and j["positions"] == 461
    assert np.array_equal(analysis.trim(h), h[:, :4])
    assert np.array_equal(analysis.pad(h, 7)[:, :5], h) and not analysis.pad(h, 7)[:, 5:].any()


def test_committed_subtract_8_census():
    ref = json.load(open(os.path.join(GOLDEN, "histograms.json")))["subtract_8"]
    win, loss, tie = ref["win"], ref["loss"], ref["tie"]
    assert len(win) == len(loss) == len(tie) == ref["n_rem"] == 81
    assert sum(win) == 3_220_369_280 and sum(loss) == 1_074_598_016 and sum(tie) == 0
    assert sum(win) + sum(loss) + sum(tie) == ref["positions"] == 1 << 32
    assert win[:8] == [0, 16, 0, 408, 0, 3656, 0, 20352]
    assert loss[:8] == [1, 0, 36, 0, 358, 0, 2360, 0]
    assert win[80] + loss[80] > 0
    s = analysis.summarize(np.array([win, loss, tie], dtype=np.uint64))
    assert max(s["max_remoteness_win"], s["max_remoteness_loss"]) == 80
