"""The persistent kernels at shapes where a workgroup WALKS several items (tests/walk_cases.py: at
least three per workgroup, every kind of step inside some range, partial edges, idle workgroups).

Basic run: each case calls its ops entry point directly under launch_check.LaunchChecker: operands
are views inside wider buffers (ld = c + 32, off = 32, as test_gpu_ops.conv3x3_case), outputs and
sums buffers are handed over as NaN, the reference is the checker's own (fp64 on the GPU over the
whole output, torch GEMMs per image and tap) with the bounds launch_check.py states, taken as they
are.  chk.unchecked must stay empty and the entry point must appear in chk.calls.

On top of that:
* weight gradients (every wgrad_halo case, the two-source form, conv_c3_wgrad): integer operands
  x, dz in {-2..2}, so that sum |dz x| <= 4 P < 2^24 (asserted on the reference) and the fp32 result is
  exact in any order; compared in every bit with the fp64 reference cast to fp32.  The checker's
  rel-L2 of 1e-3 cannot tell a missing boundary row from a reordered sum;
* BN partial sums across a walk: no row is NaN, and the rows of a (stream, wave) / (group, wave
  row) that owns no tile are exactly zero;
* image 1 of an N = 3 launch equals, in every bit, the same image launched alone (another split,
  the same arithmetic per output element), for one forward of each family.

Before anything launches each case re-proves its split on the device's own queries and prints it.
"""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from launch_check import LaunchChecker, _atb  # noqa: E402
from tests import exact_cases as E  # noqa: E402
from tests import walk_cases as WC  # noqa: E402

TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
F64 = torch.float64
PAD = 32  # channels in front of every view: ld = c + PAD, off = PAD


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.backends.cuda.matmul.allow_tf32 = False
    from cnn_itmo_amd import _lib as L
    L.load()


def _ids(c):
    return "-".join(str(v) for v in c).replace(" ", "")


def gen(*key):
    g = torch.Generator(device="cuda")
    g.manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 7)
    return g


def randn(g, shape, T, scale=1.0):
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(T)


def nans(numel, T=torch.float32):
    return torch.full((int(numel),), float("nan"), dtype=T, device="cuda")


def wide(ops, t4):
    """A View of t4 [n, h, w, c] inside a buffer PAD channels wider (the channels in front hold 3.0)."""
    n, h, w, c = t4.shape
    buf = torch.empty(n, h, w, c + PAD, dtype=t4.dtype, device="cuda")
    buf[..., :PAD] = 3.0
    buf[..., PAD:] = t4
    return ops.View(buf.view(-1), n, h, w, c, c + PAD, PAD)


def wide_nan(ops, n, h, w, c, T):
    return ops.View(nans(n * h * w * (c + PAD), T), n, h, w, c, c + PAD, PAD)


def untouched(v):
    """The PAD channels in front of an output view are still NaN."""
    assert bool(torch.isnan(v.buf.view(v.n, v.h, v.w, v.ld)[..., :v.off]).all()), "the launch wrote outside its view"


def conv_weights(ops, g, d, T, cout, cin):
    w32 = randn(g, (cout, 3, 3, cin), torch.float32, 0.1)
    wf = torch.empty(w32.numel(), dtype=T, device="cuda")
    wflip = torch.empty(w32.numel(), dtype=T, device="cuda")
    ops.prep_conv3x3(d, w32, cout, cin, wf, wflip)
    return wf, wflip


class checked:
    """LaunchChecker around one entry point: nothing unchecked, the entry point checked once."""

    def __init__(self, ops, d, entry):
        self.ops, self.d, self.entry = ops, d, entry

    def __enter__(self):
        torch.cuda.synchronize()
        self.chk = LaunchChecker(self.ops, self.d)
        return self.chk

    def __exit__(self, et, ev, tb):
        self.chk.restore()
        if et is None:
            assert not self.chk.unchecked, f"library calls outside a checked entry point: {self.chk.unchecked}"
            assert self.chk.calls == {self.entry: 1}, self.chk.calls


def idle_rows_zero(sums, rows_of, ranges, what):
    """sums [rows, ...]: no NaN anywhere; the rows of an owner without items are exactly zero, and some
    row of every other owner is not."""
    s = sums.view(len(ranges), rows_of, -1)
    assert not bool(torch.isnan(s).any()), f"{what}: a sums row was never written"
    empty = torch.tensor([a == b for a, b in ranges], device=s.device)
    if bool(empty.any()):
        assert bool((s[empty] == 0).all()), f"{what}: the sums rows of an owner without items are not zero"
    assert bool((s[~empty] != 0).flatten(1).any(1).all()), f"{what}: an owner of items wrote only zeros"


# ---- halo_conv_kernel ----------------------------------------------------------------------------
def halo_forward(ops, L, case, xv, x2v, wf, bias, n):
    """Launch the forward form of `case` on n images of xv (and x2v); returns (out view or yhat, stats,
    extras).  Outputs and sums are NaN before the launch."""
    op, dt, _n, w, cin, cout, _ = case
    h, d, T = WC.HALO_H, WC.DT[dt], TDT[dt]
    g = gen(7, cin, cout)
    rows = ops.conv3x3_stat_rows(d, n, h, w, cin, cout)
    aff = (torch.rand(cout, generator=g, device="cuda") * 2.5 - 1.0, randn(g, (cout,), torch.float32))
    if op == "fwd_head":
        hv = h - 1
        yhat = nans(n * hv * w * 3)
        ops.conv3x3_fwd_head(d, xv, wf, bias, cout, L.RELU | L.AFFINE, aff, hv, randn(g, (3 * cout,), torch.float32, 0.2),
                             randn(g, (3,), torch.float32), yhat)
        return yhat, None, ()
    out = wide_nan(ops, n, h, w, cout, T)
    train = op in ("fwd", "fwd_pool", "fwd_cat")
    stats = nans(rows * 2 * cout) if train else None
    flags = L.RELU | (L.STATS if train else L.AFFINE)
    kw = dict(flags=flags, aff=None if train else aff, stats=stats)
    if op in ("fwd_pool", "fwd_pool_affine"):
        pv = nans(n * (h // 2) * (w // 2) * cout, T)
        pi = torch.full((n * (h // 2) * (w // 2) * cout,), 255, dtype=torch.uint8, device="cuda")
        sign = torch.tensor([1.0, -0.5, 0.0, 3.0], device="cuda").repeat(cout // 4) if train else None
        ops.conv3x3_fwd_pool(d, xv, wf, bias, out, pv, pi, sign, **kw)
        assert not bool(torch.isnan(pv).any()) and int(pi.max()) < 4
        return out, stats, (pv, pi)
    if op == "fwd_cat":
        ops.conv3x3_fwd_cat(d, xv, x2v, wf, bias, out, **kw)
    else:
        ops.conv3x3_fwd(d, xv, wf, bias, out, **kw)
    return out, stats, ()


def halo_forward_operands(ops, case, n):
    op, dt, _n, w, cin, cout, _ = case
    h, d, T = WC.HALO_H, WC.DT[dt], TDT[dt]
    g = gen(1, w, cin, cout, d)
    wf, _ = conv_weights(ops, g, d, T, cout, cin)
    bias = randn(g, (cout,), torch.float32)
    if op == "fwd_cat":
        return wide(ops, randn(g, (n, h, w, 32), T)), wide(ops, randn(g, (n, h, w, cin - 32), T)), wf, bias
    return wide(ops, randn(g, (n, h, w, cin), T)), None, wf, bias


HALO_ENTRY = {"fwd": "conv3x3_fwd", "fwd_nosum": "conv3x3_fwd", "fwd_pool": "conv3x3_fwd_pool",
              "fwd_pool_affine": "conv3x3_fwd_pool", "fwd_head": "conv3x3_fwd_head", "fwd_cat": "conv3x3_fwd_cat",
              "dgrad": "conv3x3_dgrad", "dgrad_bn": "conv3x3_dgrad_bn", "dgrad_bn_pooled": "conv3x3_dgrad_bn_pooled"}


@pytest.mark.parametrize("case", list(WC.HALO), ids=_ids)
def test_halo_walk(case):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    op, dt, n, w, cin, cout, extra = case
    h, d, T = WC.HALO_H, WC.DT[dt], TDT[dt]
    sp = WC.check_halo(L.query, case)  # (e) and the split, on this device's queries
    print(f"{case}: {sp['name']}: {sp['streams']} streams x {sp['nblocks']} blocks of {sp['grid']} workgroups, "
          f"{sp['tiles']} tiles, {sp['per_stream']:.2f} per stream, {sp['idle']} idle")
    P = n * h * w
    if op in WC.HALO_FWD_OPS:
        xv, x2v, wf, bias = halo_forward_operands(ops, case, n)
        with checked(ops, d, HALO_ENTRY[op]):
            out, stats, _ = halo_forward(ops, L, case, xv, x2v, wf, bias, n)
        if op == "fwd_head":
            assert not bool(torch.isnan(out).any())
        else:
            untouched(out)
        if stats is not None:
            idle_rows_zero(stats, WC.NWAVE, sp["ranges"], "BN sums")
        return
    g = gen(2, w, cin, cout, d)
    cl = cin + 64 if op == "dgrad_bn_pooled" else cin  # pooled: the skip rows of a concat consumer's weights
    _, wflip = conv_weights(ops, g, d, T, cout, cl)
    dz = randn(g, (P * cout,), T)
    if op == "dgrad":
        dx = wide_nan(ops, n, h, w, cin, T)
        with checked(ops, d, HALO_ENTRY[op]):
            ops.conv3x3_dgrad(d, dz, n, h, w, cout, wflip, cin, dx)
        untouched(dx)
        return
    c0, c1, par = extra if extra else (0, cin, False)
    c = c1 - c0
    rv = wide(ops, randn(g, (n, h, w, c), T).clamp_min(0))
    coef = randn(g, (3 * c,), torch.float32)
    zf = nans(P * c, T)
    npar = 4 if par else 1
    if op == "dgrad_bn":
        rows = ops.conv3x3_dgrad_bn_rows(d, n, h, w, cout, cin, c0, c1)
        part = nans(rows * npar * c)
        dx = None if (c0 == 0 and c1 == cin) else wide_nan(ops, n, h, w, cin, T)
        with checked(ops, d, HALO_ENTRY[op]):
            ops.conv3x3_dgrad_bn(d, dz, n, h, w, cout, wflip, cin, dx, c0, c1, coef, rv, zf, part, par)
        if dx is not None:
            untouched(dx)
            assert bool(torch.isnan(dx.tensor()[..., c0:c1]).all()), "fused columns are not written to dx"
    else:
        rows = ops.conv3x3_dgrad_bn_pooled_rows(d, n, h, w, cout, cin)
        part = nans(rows * c)
        dyp = randn(g, (n * (h // 2) * (w // 2) * cin,), T)
        idx = torch.randint(0, 4, (n * (h // 2) * (w // 2) * cin,), generator=g, device="cuda", dtype=torch.uint8)
        with checked(ops, d, HALO_ENTRY[op]):
            ops.conv3x3_dgrad_bn_pooled(d, dz, n, h, w, cout, wflip, cin, coef, rv, dyp, idx, zf, part)
    assert not bool(torch.isnan(zf).any())
    idle_rows_zero(part, WC.NWAVE, sp["ranges"], "column sums")


def test_halo_image_alone_equals_image_in_batch():
    """Image 1 of the three-image training forward, 3.02 tiles per stream, against the same image
    launched alone (258 tiles over 256 streams: one tile per stream)."""
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    case = ("fwd", "bf16", 3, 4100, 32, 64, None)
    assert case in WC.HALO
    op, dt, n, w, cin, cout, _ = case
    xv, _, wf, bias = halo_forward_operands(ops, case, n)
    out, _, _ = halo_forward(ops, L, case, xv, None, wf, bias, n)
    x1 = ops.View(xv.buf.view(n, -1)[1].clone(), 1, xv.h, xv.w, xv.c, xv.ld, xv.off)
    one, _, _ = halo_forward(ops, L, case, x1, None, wf, bias, 1)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(one.tensor()).any())
    E.assert_bits_equal(out.tensor()[1], one.tensor()[0], "image 1 of 3 vs alone")
    assert not torch.equal(out.tensor()[1], out.tensor()[0])


# ---- tconv_stream_kernel -------------------------------------------------------------------------
def tconv_operands(ops, case, n):
    op, cin, cout = case
    h, w, d, T = WC.TS_H, WC.TS_W, WC.DT["bf16"], torch.bfloat16
    g = gen(3, cin, cout)
    k32 = randn(g, (2, 2, cout, cin), torch.float32, 0.1)
    kf = torch.empty(k32.numel(), dtype=T, device="cuda")
    kT = torch.empty(k32.numel(), dtype=T, device="cuda")
    ops.prep_tconv(d, k32, cout, cin, kf, kT)
    x = randn(g, (n, h, w, cin), T)
    return g, kf, kT, x


def tconv_forward(ops, L, case, x, kf, bias, n):
    op, cin, cout = case
    h, w, d = WC.TS_H, WC.TS_W, WC.DT["bf16"]
    xv = ops.View(x.reshape(-1), n, h, w, cin, cin, 0)
    out = wide_nan(ops, n, 2 * h, 2 * w, cout, torch.bfloat16)
    stats = nans(ops.tconv_stat_rows(d, n, h, w, cin, cout) * 2 * 4 * cout)
    ops.tconv_fwd(d, xv, kf, bias, out, flags=L.RELU | L.STATS, stats=stats)
    return out, stats


@pytest.mark.parametrize("case", list(WC.TCONV), ids=_ids)
def test_tconv_stream_walk(case):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    op, cin, cout = case
    n, h, w, d, T = WC.TS_N, WC.TS_H, WC.TS_W, WC.DT["bf16"], torch.bfloat16
    sp = WC.check_tconv(L.query, case)
    print(f"{case}: {sp['name']}: {sp['groups']} groups, {sp['ntiles']} tiles, {sp['per']} per group, {sp['idle']} idle")
    g, kf, kT, x = tconv_operands(ops, case, n)
    P = n * h * w
    if op == "fwd":
        bias = randn(g, (cout,), torch.float32)
        with checked(ops, d, "tconv_fwd"):
            out, stats = tconv_forward(ops, L, case, x, kf, bias, n)
        untouched(out)
        idle_rows_zero(stats, sp["wm"], sp["ranges"], "BN sums")
        return
    dout = randn(g, (n * 4 * h * w * cout,), T)
    if op == "dgrad":
        dx = nans(P * cin, T)
        with checked(ops, d, "tconv_dgrad"):
            ops.tconv_dgrad(d, dout, n, h, w, cout, kT, cin, dx)
        assert not bool(torch.isnan(dx).any())
        return
    rv = wide(ops, x.clamp_min(0))
    coef = randn(g, (3 * cin,), torch.float32)
    zf = nans(P * cin, T)
    part = nans(ops.tconv_dgrad_bn_rows(d, n, h, w, cout, cin) * cin)
    with checked(ops, d, "tconv_dgrad_bn"):
        ops.tconv_dgrad_bn(d, dout, n, h, w, cout, kT, cin, coef, rv, zf, part)
    assert not bool(torch.isnan(zf).any())
    idle_rows_zero(part, sp["wm"], sp["ranges"], "column sums")


def test_tconv_image_alone_equals_image_in_batch():
    """Image 1 of three (555 tiles, three per group) against the image alone (185 tiles, one per group)."""
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    case = ("fwd", 128, 64)
    assert case in WC.TCONV
    g, kf, _, x = tconv_operands(ops, case, WC.TS_N)
    bias = randn(g, (case[2],), torch.float32)
    out, _ = tconv_forward(ops, L, case, x, kf, bias, WC.TS_N)
    one, _ = tconv_forward(ops, L, case, x[1:2].clone(), kf, bias, 1)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(one.tensor()).any())
    E.assert_bits_equal(out.tensor()[1], one.tensor()[0], "image 1 of 3 vs alone")
    assert not torch.equal(out.tensor()[1], out.tensor()[0])


# ---- weight gradients: exact ---------------------------------------------------------------------
def ints(g, shape, T):
    return torch.randint(-2, 3, shape, generator=g, device="cuda").to(T)


def dw_exact(x4, d4):
    """[cout, 3, 3, cin] fp64 weight gradient of a 'same' 3x3 conv over all images at once, with the
    sum of |terms| and the share of nonzero products of every element."""
    n, h, w, cin = x4.shape
    cout = d4.shape[-1]
    xp = torch.nn.functional.pad(x4.to(F64), (0, 0, 1, 1, 1, 1))
    d = d4.to(F64).reshape(-1, cout)
    ones = torch.nn.functional.pad(torch.ones(n, h, w, 1, dtype=F64, device=x4.device), (0, 0, 1, 1, 1, 1))
    ref, tot, cnt, field = (torch.zeros(cout, 3, 3, cin, dtype=F64, device=x4.device) for _ in range(4))
    for r in range(3):
        for q in range(3):
            win = xp[:, r:r + h, q:q + w].reshape(-1, cin)
            ref[:, r, q] = _atb(d, win)
            tot[:, r, q] = _atb(d.abs(), win.abs())
            cnt[:, r, q] = _atb((d != 0).to(F64), (win != 0).to(F64))
            field[:, r, q] = ones[:, r:r + h, q:q + w].sum()
    return ref, float(tot.max()), float((cnt / field).min())


def assert_exact_dw(dw, ref, tot, frac, what):
    assert tot < E.LIM24, f"{what}: sum |dz x| = {tot}: the reference is not exact in fp32"
    assert frac >= 1.0 / 8, f"{what}: only {frac:.3f} of an element's products are nonzero"
    assert bool((ref == ref.round()).all())
    E.assert_bits_equal(dw.view(ref.shape), ref.to(torch.float32), what)


@pytest.mark.parametrize("case", list(WC.WGRAD), ids=_ids)
def test_wgrad_halo_walk(case):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    dt, w, cin, cout, cat = case
    n, h, d, T = WC.WG_N, WC.WG_H, WC.DT[dt], TDT[dt]
    sp = WC.check_wgrad(L.query, case)
    print(f"{case}: {sp['name']}: {sp['strips']} strips, {sp['rows']} rows; workgroups per CU -> (rows per range, "
          f"ranges): { {o: (rp, len(r)) for o, (rp, r) in sp['plans'].items()} }")
    g = gen(4, w, cin, cout, d)
    x4 = ints(g, (n, h, w, cin), T)
    dz = ints(g, (n, h, w, cout), T)
    dw = nans(cout * 9 * cin)
    if cat:
        v1, v2 = wide(ops, x4[..., :32].contiguous()), wide(ops, x4[..., 32:].contiguous())
        with checked(ops, d, "conv_wgrad_cat"):
            ops.conv_wgrad_cat(d, v1, v2, dz.view(-1), cout, dw)
    else:
        with checked(ops, d, "conv_wgrad"):
            ops.conv_wgrad(d, 9, wide(ops, x4), dz.view(-1), cout, dw)
    assert_exact_dw(dw, *dw_exact(x4, dz), f"{sp['name']} weight gradient")


@pytest.mark.parametrize("case", [c for c in WC.C3 if c[0] == "wgrad"], ids=_ids)
def test_conv_c3_wgrad_walk(case):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    n, hv, h, w = WC.C3[case]
    d, T = WC.DT[case[1]], TDT[case[1]]
    sp = WC.check_c3(L.query, case)
    print(f"{case}: {sp['units']} units over at most {sp['groups']} workgroups, {sp['share']} each")
    g = gen(5, w, d)
    x = ints(g, (n, hv, w, 3), torch.float32)
    dz = ints(g, (n, h, w, 32), T)
    dw = nans(32 * 27)
    with checked(ops, d, "conv_c3_wgrad"):
        ops.conv_c3_wgrad(d, x.view(-1), n, hv, h, w, dz.view(-1), dw)
    xp = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, h - hv))
    ref, tot, frac = dw_exact(xp, dz)
    assert_exact_dw(dw, ref, tot, frac, "conv_c3 weight gradient")


# ---- conv_c3 forward -----------------------------------------------------------------------------
def c3_forward(ops, L, dt, x, n, hv, h, w, wp, bias):
    d, T = WC.DT[dt], TDT[dt]
    out = wide_nan(ops, n, h, w, 32, T)
    stats = nans(ops.conv_c3_stat_rows(n, h, w) * 64)
    ops.conv_c3_fwd(d, x.reshape(-1), n, hv, h, w, wp, bias, out, flags=L.RELU | L.STATS, stats=stats)
    return out, stats


def c3_operands(ops, dt, n, hv, w):
    g = gen(6, w, WC.DT[dt])
    wp = torch.empty(32 * 32, dtype=TDT[dt], device="cuda")
    ops.prep_c3(WC.DT[dt], randn(g, (32, 3, 3, 3), torch.float32, 0.3), 32, wp)
    return torch.rand((n, hv, w, 3), generator=g, device="cuda"), wp, randn(g, (32,), torch.float32)


@pytest.mark.parametrize("case", [c for c in WC.C3 if c[0] == "fwd"], ids=_ids)
def test_conv_c3_fwd_walk(case):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    n, hv, h, w = WC.C3[case]
    sp = WC.check_c3(L.query, case)
    print(f"{case}: {sp['units']} units over {sp['groups']} workgroups, {sp['share']} each")
    x, wp, bias = c3_operands(ops, case[1], n, hv, w)
    with checked(ops, WC.DT[case[1]], "conv_c3_fwd"):
        out, stats = c3_forward(ops, L, case[1], x, n, hv, h, w, wp, bias)
    untouched(out)
    assert not bool(torch.isnan(stats).any())


def test_conv_c3_image_alone_equals_image_in_batch():
    """Image 1 of three (2304 units, three per workgroup) against the image alone (768: one each)."""
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    n, hv, h, w = WC.C3[("fwd", "bf16")]
    x, wp, bias = c3_operands(ops, "bf16", n, hv, w)
    out, _ = c3_forward(ops, L, "bf16", x, n, hv, h, w, wp, bias)
    one, _ = c3_forward(ops, L, "bf16", x[1:2].clone(), 1, hv, h, w, wp, bias)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(one.tensor()).any())
    E.assert_bits_equal(out.tensor()[1], one.tensor()[0], "image 1 of 3 vs alone")
    assert not torch.equal(out.tensor()[1], out.tensor()[0])
