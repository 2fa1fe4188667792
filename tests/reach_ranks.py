"""Rank target of the multi-process gm_reach test (tests/test_gpu_reach.py), run by
tests/mp_ranks.run_ranks with the set_comm flow of tests/moves_ranks.py.  A rank of a
multi-process solve does not hold its children's owners' tables: each rank returns the status
and the message gm_reach gives it."""
import os


def rank_main(rank, world, phase, game, params, opts):
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # as bench.py: a queue per stream
    import ctypes
    import numpy as np
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
    root = ctx.initial() if root is None else root
    n, rec = ctx.solve(root)
    phase("reach")
    keys = np.array([root], dtype=np.uint64)
    how, out = _lib.Reach(0, 0, 0, 0), _lib.ReachOut()
    rc = ctx.L.gm_reach(ctx.h, ctypes.byref(how), keys.ctypes.data, 1, ctypes.byref(out), None, 0, None, None, None, 0)
    msg = ctx.L.gm_last_error().decode()
    phase("digest")
    d, m = ctx.digest()
    ctx.close()
    return {"rank": rank, "n": n, "m": m, "rc": rc, "message": msg}
