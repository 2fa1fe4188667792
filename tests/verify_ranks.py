"""Rank target of the multi-process gm_verify test (tests/test_gpu_verify.py), run by
tests/mp_ranks.run_ranks with the set_comm flow of tests/hist_ranks.py: a rank of a solve
sharded over processes holds its share of the table only, so gm_verify and gm_poke refuse
(GM_E_STATE) and the context goes on answering."""
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
    for k, v in opts.items():
        ctx.set_option(getattr(_lib, "OPT_" + k.upper()), v)
    phase("solve")
    root = ctx.initial()
    n, rec = ctx.solve(root)
    phase("verify")
    out, n_bad = _lib.Verify(), ctypes.c_uint64()
    rc = ctx.L.gm_verify(ctx.h, ctypes.byref(out), None, 0, ctypes.byref(n_bad))
    msg = ctx.L.gm_last_error().decode()
    key = (ctypes.c_uint64 * 1)(root)
    rc_poke = ctx.L.gm_poke(ctx.h, key, rec)
    phase("digest")
    d, m = ctx.digest()
    ctx.close()
    return {"rank": rank, "n": n, "rc": rc, "msg": msg, "rc_poke": rc_poke, "digest": d, "m": m}
