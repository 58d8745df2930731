"""Poisoned arena (test infrastructure, CPU and GPU).

The per-kernel tests take their operands from torch's allocator: 512-byte aligned, zero more
often than not, and surrounded by memory nobody looks at.  An ``Arena`` owns the memory around
every operand instead:

* one ``uint8`` allocation filled with a poison byte -- ``fill="nan"``: 0xFF, which reads as
  a NaN in fp32 and bf16 and as an invalid window index in ``uint8``; ``fill="zero"``: 0x00;
* ``take`` carves tensors out of it with at least ``guard`` (1 MiB) bytes of poison on either
  side, at a base address that is 16-byte aligned and deliberately not more (address = 16
  mod 128) unless a stronger ``align`` is asked for (an operand for which include/cnn_itmo.h
  states one);
* ``view`` carves a ``[P, ld]`` buffer of which only the channels ``[off, off + c)`` are
  payload (an ``ops.View``): the other channels -- the other member of a concat -- stay poison;
* ``check_untouched`` asserts that every byte that was not declared payload still holds the
  poison pattern, naming the carve and the first offending offset relative to it.

A carve without ``data`` keeps the poison in its payload: that is how outputs, partial-sum
buffers, index bytes and workspaces are handed to a kernel (``poison_count`` then counts the
elements a launch left unwritten).
"""
from __future__ import annotations

import numpy as np
import torch

GUARD = 1 << 20
FILLS = {"nan": 0xFF, "zero": 0x00}
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """The elements of t as integers of the same width (contiguous copy of a strided view)."""
    t = t.contiguous()
    return t.view(_INT[t.element_size()])


def poison_count(t):
    """Number of elements of t whose bytes are all 0xFF (the ``fill="nan"`` poison)."""
    b = bits(t)
    return int((b == (255 if b.dtype == torch.uint8 else -1)).sum())


class Arena:
    def __init__(self, nbytes, fill="nan", device="cpu", guard=GUARD):
        self.byte = FILLS[fill]
        self.fill, self.guard = fill, int(guard)
        self.buf = torch.full((int(nbytes),), self.byte, dtype=torch.uint8, device=device)
        self.payload = torch.zeros(int(nbytes), dtype=torch.bool, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.pos = 0
        self.carves = []  # (name, first byte, bytes)

    # ---- carving ------------------------------------------------------------------------
    def _carve(self, nbytes, align, name):
        base = self.buf.data_ptr()
        start = self.pos + self.guard
        if align <= 16:  # 16-byte aligned and no more: address = 16 (mod 128)
            start += (16 - (base + start)) % 128
        else:
            assert align % 16 == 0
            start += -(base + start) % align
        end = start + nbytes
        assert end + self.guard <= self.buf.numel(), \
            f"arena of {self.buf.numel()} bytes is full (carve '{name}' of {nbytes} bytes ends at {end} + guard)"
        self.pos = end
        self.carves.append((name or f"carve{len(self.carves)}", start, nbytes))
        return start

    def take(self, numel, dtype, data=None, name=None, align=16, payload=True):
        """A 1-D tensor of `numel` elements of `dtype` inside the arena.  data (numpy or torch, any
        shape with numel elements) fills it; without data the payload stays poison."""
        es = torch.empty((), dtype=dtype).element_size()
        nb = int(numel) * es
        start = self._carve(nb, align, name)
        t = self.buf[start:start + nb].view(dtype)
        if payload:
            self.payload[start:start + nb] = True
        if data is not None:
            t.copy_(self._as(data, dtype).reshape(-1))
        return t

    def view(self, n, h, w, c, ld, off, dtype, data=None, name=None, align=16, channels=None):
        """An ops.View of an [n*h*w, ld] buffer: the channels [off, off + c) are payload (data
        [n, h, w, c] fills them), every other channel stays poison.  channels = [(lo, hi), ...]
        (columns of the ld-wide row) overrides which columns are payload, for an entry point
        that writes only part of its view."""
        from cnn_itmo_amd.ops import View
        assert 0 <= off and off + c <= ld
        p = n * h * w
        t = self.take(p * ld, dtype, name=name, align=align, payload=False)
        es = t.element_size()
        start = self.carves[-1][1]
        rows = self.payload[start:start + p * ld * es].view(p, ld * es)
        for lo, hi in ([(off, off + c)] if channels is None else channels):
            assert 0 <= lo <= hi <= ld
            rows[:, lo * es:hi * es] = True
        v = View(t, n, h, w, c, ld, off)
        if data is not None:
            v.tensor().copy_(self._as(data, dtype).reshape(n, h, w, c))
        return v

    def _as(self, data, dtype):
        if isinstance(data, np.ndarray):
            data = torch.from_numpy(np.ascontiguousarray(data))
        if data.dtype.is_floating_point and dtype.is_floating_point and dtype != torch.float64:
            data = data.to(torch.float32)  # one rounding: fp64 -> fp32 -> dtype, as the per-kernel tests
        return data.to(self.buf.device).to(dtype)

    # ---- the check ----------------------------------------------------------------------
    def check_untouched(self):
        """Every byte outside the declared payloads still holds the poison pattern."""
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        bad = (self.buf != self.byte) & ~self.payload
        if not bool(bad.any()):
            return
        first = int(bad.nonzero()[0])
        # the carve the byte belongs to: inside one (a non-payload channel), else the nearest
        best = None
        for name, start, nb in self.carves:
            dist = 0 if start <= first < start + nb else min(abs(first - start), abs(first - (start + nb - 1)))
            if best is None or dist < best[0]:
                best = (dist, name, start, nb)
        _, name, start, nb = best
        where = "a non-payload byte inside" if start <= first < start + nb else "the guard of"
        raise AssertionError(f"stray write: {int(bad.sum())} bytes outside every payload changed; the first is "
                             f"{where} carve '{name}' ({nb} bytes) at offset {first - start:+d} from its start "
                             f"(value 0x{int(self.buf[first]):02x}, poison 0x{self.byte:02x})")
