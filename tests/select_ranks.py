"""Rank target of the multi-process gm_select tests (tests/test_gpu_select.py), run by
tests/mp_ranks.run_ranks: one process per rank, the ranks sharing the GPU over the IPC
transports, with the set_comm flow of tests/hist_ranks.py.  Each rank returns the keys and
records it selects among its own share, and its digest count."""
import os


def rank_main(rank, world, phase, game, params, opts, values, rem_lo, rem_hi):
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # as bench.py: a queue per stream
    import ctypes
    import torch.distributed as tdist
    from gamesmanmpi_amd import Context, _lib
    tdist.init_process_group("gloo", rank=rank, world_size=world)   # MASTER_* from the parent
    opts = dict(opts)
    ctx = Context(game, params, device=rank % _lib.lib().gm_device_count())
    phase("unique id")
    uid = [None]
    if rank == 0:
        buf = ctypes.create_string_buffer(128)
        _lib.check(_lib.lib().gm_comm_unique_id(buf, 128))
        uid[0] = buf.raw
    tdist.broadcast_object_list(uid, src=0)
    phase("communicator")
    ctx.set_comm(rank, world, uid[0])
    root = opts.pop("root", None)
    for k, v in opts.items():
        ctx.set_option(getattr(_lib, "OPT_" + k.upper()), v)
    phase("solve")
    n, rec = ctx.solve(ctx.initial() if root is None else root)
    phase("count")
    count = ctx.select(values, rem_lo, rem_hi, 0)[0]
    phase("select")
    found, keys, recs = ctx.select(values, rem_lo, rem_hi, count, as_array=True)
    phase("digest")
    d, m = ctx.digest()
    ctx.close()
    return {"rank": rank, "n": n, "m": m, "count": count, "found": found, "keys": keys.tolist(), "recs": recs.tolist()}


def report_main(rank, world, phase, specs, cap, statsdir):
    """No GPU: find.report over the process group with a stub solver per rank that holds every
    world-th pair of a fixed table (tests/test_find.py).  Returns what the rank wrote."""
    import io
    import numpy as np
    import torch.distributed as tdist
    from gamesmanmpi_amd import analysis, find
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    keys = np.arange(40, dtype=np.uint64)[rank::world]
    recs = ((keys % 3) << 14 | (keys % 7)).astype(np.uint16)

    class Codec:
        def pos(self, key):
            return "p%d" % key

    class Ctx:
        def select(self, values, rem_lo, rem_hi, cap):
            k, r = find.from_records(keys, recs, find.Spec(values, rem_lo, rem_hi, False))
            return len(k), [int(x) for x in k[:cap]], r[:cap]

    class Stub:
        codec, ctx = Codec(), Ctx()

        def analysis(self):
            return analysis.from_records(recs)

    out = io.StringIO()
    phase("report")
    find.report(Stub(), specs, cap, out, statsdir, rank, world, sharded=True)
    tdist.destroy_process_group()
    return out.getvalue()
