"""dist.broadcast_state on CPU (gloo, world size 2): every optimizer slot rank 0 holds and
both counters reach rank 1, which starts with one slot of its own (as a fresh Engine does)."""
import os
import socket
from types import SimpleNamespace

import numpy as np
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake_engine(n, nslots, fill, step, iterations):
    """The attributes broadcast_state touches, with Engine's own ensure_slots."""
    from cnn_itmo_amd.engine import Engine
    accum = torch.full((n,), float(fill))
    e = SimpleNamespace(params=torch.full((n,), 10.0 + fill), bufs=torch.full((5,), 20.0 + fill), accum=accum,
                        slots=[accum], step=step, iterations=iterations, weights_dirty=False)
    e.ensure_slots = lambda k: Engine.ensure_slots(e, k)
    for i, s in enumerate(e.ensure_slots(nslots)):
        s.fill_(fill + i)
    return e


def _worker(rank, world, port, errq):
    try:
        import sys
        sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
        import torch.distributed as dist
        from cnn_itmo_amd import dist as D
        D.init_from_env(backend="gloo")
        # rank 0: Adam after 7 applied updates out of 9 steps; rank 1: a fresh engine
        e = _fake_engine(48, 2, 1.0, 9, 7) if rank == 0 else _fake_engine(48, 1, 0.0, 0, 0)
        D.broadcast_state(e)
        assert (e.step, e.iterations, len(e.slots)) == (9, 7, 2), (e.step, e.iterations, len(e.slots))
        assert e.slots[0] is e.accum and e.weights_dirty
        np.testing.assert_array_equal(e.params.numpy(), np.full(48, 11.0))
        np.testing.assert_array_equal(e.bufs.numpy(), np.full(5, 21.0))
        for i, s in enumerate(e.slots):
            np.testing.assert_array_equal(s.numpy(), np.full(48, 1.0 + i))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as ex:  # surface to the parent
        import traceback
        errq.put(f"rank {rank}: {ex!r}\n{traceback.format_exc()}")
        raise


def test_broadcast_covers_every_slot_and_iterations():
    world = 2
    ctx = mp.get_context("spawn")
    errq = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, errq)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, "\n".join(errs)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
