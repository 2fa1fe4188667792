"""The bench.py contract on the GPU: one JSON line with the driver's fields, the roofline
and parity objects, at N = 1 and with 4 virtual ranks (the split box engine); a plain run
(no --full) that only times the headline and writes its outputs."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
          "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "3", "--warmup", "1", "--full",
                        "--no-toot", "--no-cpu-baseline", *args], capture_output=True, text=True, timeout=300,
                       cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_line_one_gpu():
    d = _bench()
    assert all(k in d for k in FIELDS)
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["value"] > 0 and d["parity"]["ok"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and 0 < rf["frac"] < 1 and rf["peak"] == 8000.0
    assert rf["launches_per_solve"] == 41 and rf["kernel"].startswith("box_tier_kernel<false>")


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """Without --full: the headline fields and the roofline from the timed steps' events, none
    of the separate measurements or digest checks; --dump-outputs writes float arrays of at
    most 64 MB in all.  Every sampled slot of the table is decoded to its position (box
    layout, include/gmsolve.h gm_dense_table) and its code's class checked against the
    game's closed form: LOSS iff the xor over heaps of (heap mod 3) is 0."""
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert all(k in d for k in FIELDS)
    assert d["steps"] == 2 and d["value"] > 0 and d["unit"] == "positions/s" and d["dtype"] == "u8"
    assert d["higher_is_better"] is True and d["full"] is False
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 2 ** 32) < 1.0   # value = positions / step time
    assert d["cpu_baseline"] is None and "other_configs" not in d
    assert d["roofline"]["measured_copy_gbs"] is None and d["roofline"]["launches_per_solve"] == 41
    assert d["parity"]["digest"] is None and d["parity"]["root_closed_form_ok"]
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == ["solve.npy", "table_histogram.npy", "table_sample.npy", "table_sample_index.npy"]
    a = {f[:-4]: np.load(tmp_path / "out" / f) for f in files}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["solve"].tolist() == [2.0 ** 32, float(d["parity"]["root_record"] >> 14),
                                   float(d["parity"]["root_record"] & 0x3FFF)]
    assert a["table_histogram"].sum() == 2.0 ** 32 and a["table_histogram"][:, 0].sum() == 0   # every slot solved
    s, code = a["table_sample_index"].astype(np.int64), a["table_sample"].astype(np.int64)
    assert len(s) == len(code) == 1 << 22 and s.min() >= 0 and s.max() < 2 ** 32
    box, A, B = s >> 12, (s >> 4) & 255, s & 15
    g = np.zeros_like(s)
    for i in range(4):
        g ^= ((((box >> (2 * i)) & 3) << 2) | ((A >> (2 * i)) & 3)) % 3
    for j in range(4):
        g ^= ((((box >> (8 + 3 * j)) & 7) << 1) | ((B >> j) & 1)) % 3
    assert np.array_equal(code >= 128, g == 0) and code.min() >= 1 and code.max() <= 255


def test_bench_line_virtual_ranks_split():
    """4 virtual ranks: the split box engine -- every box on one rank (work_vs_one_gpu = 1),
    the ranks' tier launches, halo bytes per rank, parity of the whole table."""
    d = _bench("--virtual-ranks", "4")
    sh = d["sharding"]
    assert d["parity"]["ok"] and sh["boxes_per_rank"] == [262144] * 4 and sh["work_vs_one_gpu"] == 1.0
    assert sum(sh["halo_bytes_received_per_step_by_rank"]) > 0
    rf = d["roofline"]
    assert rf["launches_per_solve"] > 4 * 30 and rf["kernel"].startswith("box_tier_kernel<true>")
    assert rf["traffic"] is None   # the committed PMC summary is the one-GPU solve's


def test_bench_rehearsal_two_processes_one_gpu():
    """bench.py at N = 2 as the driver launches it (torch.distributed.run, one process per
    rank), both ranks on this one GPU (--rehearse-one-gpu: gloo for the bench's collectives,
    the IPC transport for the halos): the IPC probe passes (no fallback), every rank's owned
    digest equals the oracle's, the side configs shard over the sparse IPC transport, and the
    line says it is a rehearsal."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29531", os.path.join(REPO, "bench.py"),
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--rehearse-one-gpu", "--dist-batch", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["parity"]["ok"] and d["halo_transport_fallback"] is None
    assert d["rehearsal"] and d["sharding"]["work_vs_one_gpu"] == 1.0
    assert d["parity"]["per_rank_vs_oracle"]["wrong_ranks"] == []
    # the side configs' hash-sharded solves at N = 2, over the sparse IPC transport (RCCL refuses
    # two ranks on one GPU): summed digests, counts and root records equal the oracle's
    oc = d["other_configs"]
    for name in ("othello_4x4", "toot_6x4"):
        assert oc[name]["ok"] and oc[name]["ranks"] == 2 and "IPC" in oc[name]["transport"], oc[name]
    assert oc["toot_6x4"]["symmetry_off"]["digest_matches_oracle"]


def test_bench_rehearsal_failed_probe_exits_cleanly():
    """a rehearsal whose IPC probe fails (forced by the GM_BENCH_PROBE_FAIL
    hook) has nothing to fall back to, so bench.py ends at once with status 4 and one JSON
    error line -- no autotune or timed solves on the broken transport, no traceback cascade."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29533", os.path.join(REPO, "bench.py"),
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--rehearse-one-gpu", "--dist-batch", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=REPO,
                       env=dict(os.environ, GM_BENCH_PROBE_FAIL="1"))
    assert r.returncode != 0
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["value"] is None and "probe failed" in d["error"]
    assert 'bench.py", line' not in r.stderr, r.stderr[-3000:]   # no traceback through bench.py (torchrun
    # itself reports the failed child with its own traceback)
