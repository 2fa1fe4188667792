"""Rank target of the multi-process gm_histogram tests (tests/test_gpu_histogram.py), run by
tests/mp_ranks.run_ranks: one process per rank, the ranks sharing the GPU over the IPC
transports, with the set_comm flow of tests/test_gpu_multiproc.py.  Each rank returns its own
histogram and its digest count."""
import os


def rank_main(rank, world, phase, game, params, opts):
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
    phase("histogram")
    hist = ctx.histogram()
    phase("digest")
    d, m = ctx.digest()
    ctx.close()
    return {"rank": rank, "n": n, "rec": rec, "m": m, "hist": hist.tolist()}
