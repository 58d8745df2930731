"""tests/arena.py on the CPU: layout of the carves and the teeth of check_untouched (one byte
written into a guard, one into a non-view channel, each must fail it and be named)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from arena import GUARD, Arena, bits, poison_count  # noqa: E402


def _arena(fill):
    return Arena(8 * GUARD, fill, "cpu")


@pytest.mark.parametrize("fill", ["nan", "zero"])
def test_layout_alignment_and_poison(fill):
    a = _arena(fill)
    x = a.take(1000, torch.float32, data=np.arange(1000.0), name="x")
    out = a.take(77, torch.bfloat16, name="out")
    idx = a.take(13, torch.uint8, name="idx")
    al = a.take(64, torch.float32, name="aligned", align=256)
    v = a.view(2, 3, 5, 32, 96, 64, torch.bfloat16, data=np.ones((2, 3, 5, 32)), name="v")
    for t in (x, out, idx, v.buf):
        assert t.data_ptr() % 128 == 16  # 16-byte aligned and no more
    assert al.data_ptr() % 256 == 0
    # >= 1 MiB of poison on either side of every carve, and between neighbours
    prev_end = 0
    for _, start, nb in a.carves:
        assert start - prev_end >= GUARD
        prev_end = start + nb
    assert a.buf.numel() - prev_end >= GUARD
    assert torch.equal(x, torch.arange(1000.0))
    if fill == "nan":  # payload without data stays poison: NaN in fp32 / bf16, 0xFF index bytes
        assert poison_count(out) == 77 and bool(torch.isnan(out).all()) and poison_count(idx) == 13
        assert bool(torch.isnan(al).all())
        assert bool(torch.isnan(v.buf.view(30, 96)[:, :64]).all())
    else:
        assert int(bits(out).abs().max()) == 0 and poison_count(out) == 0
    assert float(v.tensor().float().min()) == 1.0 and v.tensor().shape == (2, 3, 5, 32)
    a.check_untouched()
    # payload may be written freely: outputs, in-place operands, the view's own channels
    out.fill_(3.0)
    idx.fill_(2)
    v.tensor().fill_(5.0)
    a.check_untouched()
    assert poison_count(out) == 0 and poison_count(idx) == 0


@pytest.mark.parametrize("fill", ["nan", "zero"])
@pytest.mark.parametrize("side", ["before", "after"])
def test_guard_write_is_detected(fill, side):
    a = _arena(fill)
    a.take(100, torch.float32, name="first")
    t = a.take(100, torch.float32, name="victim")
    a.take(100, torch.float32, name="last")
    a.check_untouched()
    start = a.carves[1][1]
    pos = start - 3 if side == "before" else start + 400 + 4096  # a whole page past the end
    a.buf[pos] = 0x5A
    where = r"-3 " if side == "before" else r"\+4496 "
    with pytest.raises(AssertionError, match=r"guard of carve 'victim'.*offset " + where):
        a.check_untouched()
    assert t.numel() == 100


@pytest.mark.parametrize("fill", ["nan", "zero"])
def test_foreign_channel_write_is_detected(fill):
    a = _arena(fill)
    v = a.view(1, 4, 4, 32, 96, 32, torch.bfloat16, data=np.zeros((1, 4, 4, 32)), name="concat")
    a.check_untouched()
    v.buf.view(torch.uint8)[(5 * 96 + 70) * 2] = 0x5A  # pixel 5, channel 70: the other member's
    with pytest.raises(AssertionError, match=r"non-payload byte inside carve 'concat'.*offset \+1100 "):
        a.check_untouched()


def test_partial_channels_payload():
    """channels=[...]: only those columns of the view may change."""
    a = _arena("nan")
    v = a.view(1, 2, 2, 96, 96, 0, torch.float32, name="dx", channels=[(0, 32)])
    v.tensor()[..., :32] = 1.0
    a.check_untouched()
    v.tensor()[0, 1, 1, 32] = 1.0
    with pytest.raises(AssertionError, match="carve 'dx'"):
        a.check_untouched()


def test_full_arena_is_an_error():
    a = Arena(3 * GUARD, "zero", "cpu")
    a.take(16, torch.float32)
    with pytest.raises(AssertionError, match="is full"):
        a.take(GUARD, torch.uint8)
