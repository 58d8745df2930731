"""Training controls under data parallelism, rehearsed on ONE GPU like tools/dp_rehearsal.py (N ranks
share device 0 over gloo): a clipped optimizer, a LearningRateScheduler and an
EarlyStopping(restore_best_weights=True), all through ``Model.fit(..., distributed=True)``.
Callbacks run on rank 0 only, so without fit_generator's synchronisation rank 1 would keep its
own learning rate and its own weights.

Checks:
  * scheduler: two epochs of two steps with RMSprop(clipnorm) and the rates 1e-3, 5e-4 set by the
    scheduler; every rank ends with the same ``optimizer.lr`` and bit-identical parameters and moving
    statistics, and they equal a single-process replay of the global batches (the ranks' shares run
    with their dropout seeds, gradients summed, moving statistics averaged, then cnnitmo_grad_sumsq,
    cnnitmo_grad_clip with grad_scale = 1 / world and RMSprop at that epoch's rate): bit-identical, as
    in dp_rehearsal.  The replay also asserts that the clip bit in every step.
  * restore: training goes on with EarlyStopping(monitor='lr', mode='max', patience=1,
    restore_best_weights=True) behind a scheduler that lowers the rate: epoch 0 is the best, epoch 1
    stops and puts epoch 0's weights back on rank 0; every rank must end with them (the replay
    continued by epoch 0's two steps), and with rank 0's learning rate.

  CNNITMO_DEVICE=0 CNNITMO_DIST_BACKEND=gloo python -m torch.distributed.run \\
      --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29534 tools/dp_controls.py
"""
import contextlib
import hashlib
import io
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cnn_itmo_amd as C  # noqa: E402
from cnn_itmo_amd import dist as D  # noqa: E402
from cnn_itmo_amd import ops  # noqa: E402

H, W, B, NFR = 64, 96, 2, 8
CLIPNORM = 1e-3
RATES = [1e-3, 5e-4, 2.5e-4]


def model(dtype):
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        return C.U_net(input_size=(H, W, 3), dtype=dtype, seed=3, verbose=False)


def digests(eng, lr, world):
    torch.cuda.synchronize()
    p, bufs = eng.params.cpu().numpy(), eng.bufs.cpu().numpy()
    out = [None] * world
    dist.all_gather_object(out, (hashlib.sha256(p.tobytes() + bufs.tobytes()).hexdigest(), lr))
    return p, bufs, out


class Replay:
    """One process, the global batches: see the module docstring."""

    def __init__(self, dtype, world):
        self.world = world
        self.eng = model(dtype)._engine()
        self.step = 0

    def run(self, batches, lr):
        e, world = self.eng, self.world
        for xb, yb in batches:
            acc = torch.zeros_like(e.grads)
            b0, bacc = e.bufs.clone(), torch.zeros_like(e.bufs)
            for k, ix in enumerate(np.array_split(np.arange(len(xb)), world)):
                ix = torch.as_tensor(ix, device=xb.device)
                e.bufs.copy_(b0)
                e.train_step(xb[ix], yb[ix], seed=self.step * world + k, apply=False, grad_frames=len(xb) / world)
                acc += e.grads
                bacc += e.bufs
            e.bufs.copy_(bacc * (1.0 / world))
            S = ops.grad_sumsq(acc)
            norm = float(S.cpu()[0]) ** 0.5 / world
            assert norm >= CLIPNORM, f"the clip does not bite: ||g|| = {norm}"
            ops.grad_clip(acc, S, 1.0 / world, CLIPNORM, 0.0)
            ops.rmsprop(e.params, acc, e.accum, lr, 0.9, 1e-7, 1.0 / world)
            e.weights_dirty = True
            self.step += 1
        torch.cuda.synchronize()
        return e.params.cpu().numpy(), e.bufs.cpu().numpy()


def main():
    rank, world, local = D.init_from_env()
    torch.cuda.set_device(local)
    dtype = os.environ.get("DTYPE", "float32")
    rng = np.random.default_rng(42)
    X = rng.uniform(size=(NFR, H, W, 3)).astype(np.float32)
    Y = rng.uniform(size=(NFR, H, W, 3)).astype(np.float32)
    m = model(dtype)
    m.compile(C.RMSprop(lr=0.123 if rank else 1e-3, clipnorm=CLIPNORM), "mse", ["accuracy"])
    if rank != 0:  # rank 0's initial state must win (DDP broadcast)
        m.set_named_weights({k: v + 0.25 for k, v in m.named_weights().items() if k.endswith("/kernel")})
    gb = B * world
    dev = torch.device("cuda", local)
    batches = [(torch.as_tensor(X[i:i + gb], device=dev), torch.as_tensor(Y[i:i + gb], device=dev))
               for i in range(0, NFR, gb)]
    rep = Replay(dtype, world) if rank == 0 else None

    # ---- scheduler: the rates reach every rank
    # (fit_generator drops the callbacks of every rank but 0: only rank 0 runs the schedule)
    sched = C.LearningRateScheduler(lambda epoch, lr: RATES[epoch])
    hist = m.fit(X, Y, batch_size=B, epochs=2, shuffle=False, verbose=0, distributed=True, callbacks=[sched])
    p, bufs, out = digests(m.engine, m.optimizer.lr, world)
    assert m.engine.step == 4 and m.optimizer.lr == RATES[1], (rank, m.engine.step, m.optimizer.lr)
    if rank == 0:
        assert len(set(out)) == 1, f"ranks diverged: {out}"
        assert hist.history["lr"] == RATES[:2], hist.history
        for epoch in range(2):
            q, qb = rep.run(batches, RATES[epoch])
        err, berr = float(np.abs(p - q).max()), float(np.abs(bufs - qb).max())
        print(f"scheduler: ranks identical ({out[0][0][:12]}, lr {out[0][1]}), max |dp - replay| params = {err:.3e}, "
              f"moving stats = {berr:.3e}")
        assert err == 0.0 and berr == 0.0, (err, berr)
    dist.barrier()

    # ---- restore: rank 0's restored weights reach every rank
    es = C.EarlyStopping(monitor="lr", mode="max", patience=1, restore_best_weights=True)
    hist = m.fit(X, Y, batch_size=B, epochs=3, shuffle=False, verbose=0, distributed=True, callbacks=[sched, es])
    p, bufs, out = digests(m.engine, m.optimizer.lr, world)
    assert m.stop_training and hist.epoch == [0, 1] and m.engine.step == 8, (rank, hist.epoch, m.engine.step)
    assert m.optimizer.lr == RATES[1]
    if rank == 0:
        assert es.stopped_epoch == 1
        assert len(set(out)) == 1, f"ranks diverged after the restore: {out}"
        q, qb = rep.run(batches, RATES[0])  # epoch 0 of this fit: the weights EarlyStopping kept
        err, berr = float(np.abs(p - q).max()), float(np.abs(bufs - qb).max())
        print(f"restore: ranks identical ({out[0][0][:12]}, lr {out[0][1]}), max |dp - replay of the best epoch| "
              f"params = {err:.3e}, moving stats = {berr:.3e}")
        assert err == 0.0 and berr == 0.0, (err, berr)
    dist.barrier()


if __name__ == "__main__":
    main()
