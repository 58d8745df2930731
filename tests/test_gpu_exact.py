"""Bit-for-bit tests of the GEMM-like kernels and their fused epilogues on exactly representable
integer operands (tests/exact_cases.py: the two regimes and their preconditions, which are asserted
on the fp64 oracle while the operands are built, and again without a GPU in test_exact_host.py).

Every comparison is of the storage bits (exact_cases.assert_bits_equal); no tolerance appears in
this file.  Outputs are handed over as NaN and must be finite wherever they are compared.  Each
case first asserts, like the tolerance tests, that the planner still chooses the kernels written
next to its shape in tests/kernel_cases.py.  The stored bf16 tensor required is
torch.tensor(exact, dtype=float32).to(bfloat16); fp32 outputs equal the exact value.

The sigmoid head, BN finalize and the other elementwise kernels are not GEMM-like and stay with
the tolerance tests.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import exact_cases as E  # noqa: E402
from tests import kernel_cases as KC  # noqa: E402
from tests.exact_cases import assert_bits_equal  # noqa: E402
from tests.kernel_cases import expect_kernels  # noqa: E402
from tests.test_gpu_ops import DT, TDT, dev, nans  # noqa: E402

RELU, STATS, AFFINE = 1, 2, 4
DTS = ("f32", "bf16")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_itmo_amd import _lib as L
    L.load()


def grid(cases, dts=DTS):
    """(case, regime, dtype) with the dtype innermost: the operands of a (case, regime) are built once."""
    return [(sh, rg, dt) for sh in cases for rg in E.REGIMES for dt in dts]


def ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def cu(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


def want(exact, dt):
    """The one tensor a correct kernel stores for the exact value."""
    return torch.tensor(np.ascontiguousarray(exact), dtype=torch.float32).to(TDT[dt])


def stored(t, what):
    """A compared output region: every element written (it was handed over as NaN)."""
    assert bool(torch.isfinite(t).all()), f"{what}: elements left unwritten or not finite"
    return t


def widen(a, ld, off, fill=5.0):
    """a [..., c] as the slice [off, off + c) of an ld-wide buffer whose other columns hold `fill`."""
    b = np.full(a.shape[:-1] + (ld,), fill)
    b[..., off:off + a.shape[-1]] = a
    return b


def sums_equal(rows, exact, what):
    """Partial-sum rows folded in fp64 equal the exact sums (no row left as NaN)."""
    assert_bits_equal(stored(rows, what).double().sum(0).cpu(), torch.tensor(np.ascontiguousarray(exact)), what)


# ---- Conv2D 3x3 ----------------------------------------------------------------------------------
def conv3x3_exact(dt, cin, cout, H, W, regime, names):
    """Forward (ReLU + BN sums) from a slice of a wider buffer, input gradient into a slice, weight
    gradient (fp32), all against the oracle bit for bit.  Also halo0_child.py's body."""
    from cnn_itmo_amd import ops
    from cnn_itmo_amd import _lib as L
    expect_kernels(KC.conv3x3_names(L.query, dt, cin, cout, H, W), names)
    C = E.conv3x3(cin, cout, H, W, regime)
    N, d, T = C.n, DT[dt], TDT[dt]
    ld, off = cin + 32, 32
    xv = ops.View(dev(widen(C.x, ld, off), dt).reshape(-1), N, H, W, cin, ld, off)
    wf = torch.empty(C.w.size, dtype=T, device="cuda")
    wflip = torch.empty(C.w.size, dtype=T, device="cuda")
    ops.prep_conv3x3(d, cu(C.w), cout, cin, wf, None)
    ops.prep_conv3x3(d, cu(C.wd), cout, cin, torch.empty_like(wf), wflip)
    out = ops.View(nans(N * H * W * cout, T), N, H, W, cout, cout, 0)
    stats = nans((ops.conv3x3_stat_rows(d, N, H, W, cin, cout), 2, cout))
    ops.conv3x3_fwd(d, xv, wf, cu(C.b), out, flags=RELU | STATS, stats=stats)
    dxb = nans(N * H * W * ld, T)
    ops.conv3x3_dgrad(d, dev(C.dz, dt), N, H, W, cout, wflip, cin, ops.View(dxb, N, H, W, cin, ld, off))
    dw = nans((cout, 3, 3, cin))
    ops.conv_wgrad(d, 9, xv, dev(C.dz, dt), cout, dw)
    torch.cuda.synchronize()
    assert_bits_equal(stored(out.buf, "fwd").view(N, H, W, cout), want(C.out, dt), "conv3x3 fwd")
    if regime == "small":
        sums_equal(stats, C.stats, "conv3x3 stat rows (sum r, sum r^2)")
    dx = dxb.view(N, H, W, ld)
    assert_bits_equal(stored(dx[..., off:], "dgrad"), want(C.dx, dt), "conv3x3 dgrad")
    assert bool(torch.isnan(dx[..., :off]).all()), "the other slice of dx was written"
    assert_bits_equal(stored(dw, "wgrad"), want(C.dw, "f32"), "conv3x3 wgrad")


@pytest.mark.parametrize("sh,regime,dt", grid(KC.CONV3X3_OPS), ids=ids)
def test_conv3x3(sh, regime, dt):
    conv3x3_exact(dt, *sh, regime, KC.CONV3X3_OPS[sh][dt])


def affine_exact(dt, H, W, cin, cout, regime, name, n=1):
    """The inference forward: ReLU, then a dyadic affine, no sums.  Also halo0_child.py's body."""
    from cnn_itmo_amd import ops
    from cnn_itmo_amd import _lib as L
    expect_kernels(KC.conv3x3_names(L.query, dt, cin, cout, H, W, n)[0], name)
    C = E.conv3x3(cin, cout, H, W, regime, False, True, n)
    d, T = DT[dt], TDT[dt]
    wf = torch.empty(C.w.size, dtype=T, device="cuda")
    ops.prep_conv3x3(d, cu(C.w), cout, cin, wf, None)
    out = ops.View(nans(n * H * W * cout, T), n, H, W, cout, cout, 0)
    ops.conv3x3_fwd(d, ops.View(dev(C.x, dt).reshape(-1), n, H, W, cin, cin), wf, cu(C.b), out,
                    flags=RELU | AFFINE, aff=(cu(C.sc), cu(C.sh)))
    torch.cuda.synchronize()
    assert_bits_equal(stored(out.buf, "affine").view(n, H, W, cout), want(C.out, dt), "conv3x3 relu + affine")


@pytest.mark.parametrize("sh,regime,dt", grid(KC.CONV3X3_FOLD), ids=ids)
def test_conv3x3_folded(sh, regime, dt):
    """fold_conv3x3's outputs; the folded forward with its border correction; border_sums + colsum;
    the folded weight gradient == the oracle's gradient w.r.t. W on the true input y = r*s + h."""
    from cnn_itmo_amd import ops
    from cnn_itmo_amd import _lib as L
    cin, cout, H, W = sh
    expect_kernels(KC.conv3x3_names(L.query, dt, cin, cout, H, W), KC.CONV3X3_FOLD[sh][dt])
    C = E.conv3x3(cin, cout, H, W, regime, True)
    N, d, T = C.n, DT[dt], TDT[dt]
    wout = nans(C.w.size, T)
    bout, border = nans(cout), nans((cout, 8))
    ops.fold_conv3x3(d, cu(C.w), cu(C.b), cu(C.s), cu(C.h), cout, cin, wout, bout, border)
    ld, off = cin + 32, 32
    rv = ops.View(dev(widen(C.r, ld, off), dt).reshape(-1), N, H, W, cin, ld, off)
    out = ops.View(nans(N * H * W * cout, T), N, H, W, cout, cout, 0)
    stats = nans((ops.conv3x3_stat_rows(d, N, H, W, cin, cout), 2, cout))
    ops.conv3x3_fwd(d, rv, wout, bout, out, flags=RELU | STATS, stats=stats, border=border)
    dzt = dev(C.dz, dt)
    brows = ops.border_rows(N)
    bpart = nans((brows, 8, cout))
    ops.border_sums(d, dzt, N, H, W, cout, bpart)
    bsum = nans((8, cout))
    ops.colsum(bpart, brows, 8 * cout, 1, bsum)
    dw = nans((cout, 3, 3, cin))
    ops.conv_wgrad(d, 9, rv, dzt, cout, dw, fold=(cu(C.s), cu(C.h), cu(C.db), bsum))
    torch.cuda.synchronize()
    assert_bits_equal(stored(wout, "wout").view(cout, 3, 3, cin), want(C.wout, dt), "fold: w*s")
    assert_bits_equal(stored(bout, "bout"), want(C.bout, "f32"), "fold: b + sum w*h")
    assert_bits_equal(stored(border, "border"), want(C.border, "f32"), "fold: the eight border sums")
    assert_bits_equal(stored(out.buf, "fwd").view(N, H, W, cout), want(C.out, dt), "folded fwd")
    if regime == "small":
        sums_equal(stats, C.stats, "folded fwd stat rows")
    assert_bits_equal(stored(bsum, "bsum"), want(C.bsum, "f32"), "border_sums + colsum")
    assert_bits_equal(stored(dw, "wgrad"), want(C.dw, "f32"), "folded wgrad")


# ---- Conv2DTranspose 2x2 -------------------------------------------------------------------------
@pytest.mark.parametrize("sh,regime,dt", grid(KC.TCONV_OPS), ids=ids)
def test_tconv(sh, regime, dt):
    """Forward (ReLU + BN sums) into a concat slice, input gradient, weight gradient."""
    from cnn_itmo_amd import ops
    from cnn_itmo_amd import _lib as L
    cin, cout, H, W = sh
    expect_kernels(KC.tconv_names(L.query, dt, cin, cout, H, W), KC.TCONV_OPS[sh][dt])
    C = E.tconv(cin, cout, H, W, regime)
    N, d, T = C.n, DT[dt], TDT[dt]
    kf = torch.empty(C.k.size, dtype=T, device="cuda")
    kT = torch.empty(C.k.size, dtype=T, device="cuda")
    ops.prep_tconv(d, cu(C.k), cout, cin, kf, torch.empty_like(kT))
    ops.prep_tconv(d, cu(C.kd), cout, cin, torch.empty_like(kf), kT)
    ld = cout + 64
    ob = nans(N * 2 * H * 2 * W * ld, T)
    stats = nans((ops.tconv_stat_rows(d, N, H, W, cin, cout), 2, 4 * cout))
    xv = ops.View(dev(C.x, dt).reshape(-1), N, H, W, cin, cin)
    ops.tconv_fwd(d, xv, kf, cu(C.b), ops.View(ob, N, 2 * H, 2 * W, cout, ld, 64), flags=RELU | STATS, stats=stats)
    dx = nans(N * H * W * cin, T)
    dout = dev(C.dout, dt)
    ops.tconv_dgrad(d, dout, N, H, W, cout, kT, cin, dx)
    dk = nans((2, 2, cout, cin))
    ops.tconv_wgrad(d, xv, dout, cout, dk)
    torch.cuda.synchronize()
    got = ob.view(N, 2 * H, 2 * W, ld)
    assert_bits_equal(stored(got[..., 64:], "fwd"), want(C.out, dt), "tconv fwd")
    assert bool(torch.isnan(got[..., :64]).all()), "the other concat member was written"
    if regime == "small":
        assert bool(torch.isfinite(stats).all())
        sums_equal(stats.view(-1, 2, 4, cout).double().sum(2), C.stats, "tconv stat rows")
    assert_bits_equal(stored(dx, "dgrad").view(N, H, W, cin), want(C.dx, dt), "tconv dgrad")
    assert_bits_equal(stored(dk, "wgrad"), want(C.dk, "f32"), "tconv wgrad")


@pytest.mark.parametrize("sh,regime,dt", grid(KC.TCONV_AFFINE), ids=ids)
def test_tconv_affine(sh, regime, dt):
    from cnn_itmo_amd import ops
    from cnn_itmo_amd import _lib as L
    cin, cout, H, W = sh
    expect_kernels(KC.tconv_names(L.query, dt, cin, cout, H, W), KC.TCONV_AFFINE[sh][dt])
    C = E.tconv(cin, cout, H, W, regime, False, True)
    N, d, T = C.n, DT[dt], TDT[dt]
    kf = torch.empty(C.k.size, dtype=T, device="cuda")
    ops.prep_tconv(d, cu(C.k), cout, cin, kf, torch.empty_like(kf))
    out = nans(N * 2 * H * 2 * W * cout, T)
    ops.tconv_fwd(d, ops.View(dev(C.x, dt).reshape(-1), N, H, W, cin, cin), kf, cu(C.b),
                  ops.View(out, N, 2 * H, 2 * W, cout, cout, 0), flags=RELU | AFFINE, aff=(cu(C.sc), cu(C.sh)))
    torch.cuda.synchronize()
    assert_bits_equal(stored(out, "affine").view(N, 2 * H, 2 * W, cout), want(C.out, dt), "tconv relu + affine")


@pytest.mark.parametrize("sh,regime,dt", grid(KC.TCONV_FOLD), ids=ids)
def test_tconv_folded(sh, regime, dt):
    from cnn_itmo_amd import ops
    from cnn_itmo_amd import _lib as L
    cin, cout, H, W = sh
    expect_kernels(KC.tconv_names(L.query, dt, cin, cout, H, W), KC.TCONV_FOLD[sh][dt])
    C = E.tconv(cin, cout, H, W, regime, True)
    N, d, T = C.n, DT[dt], TDT[dt]
    kout, bout = nans(C.k.size, T), nans(4 * cout)
    ops.fold_tconv(d, cu(C.k), cu(C.b), cu(C.s), cu(C.h), cout, cin, kout, bout)
    xv = ops.View(dev(C.r, dt).reshape(-1), N, H, W, cin, cin)
    out = ops.View(nans(N * 2 * H * 2 * W * cout, T), N, 2 * H, 2 * W, cout, cout, 0)
    ops.tconv_fwd(d, xv, kout, bout, out, flags=L.RELU | L.BIAS_PER_COL)
    dk = nans((2, 2, cout, cin))
    ops.tconv_wgrad(d, xv, dev(C.dout, dt), cout, dk, fold=(cu(C.s), cu(C.h), cu(C.par)))
    torch.cuda.synchronize()
    assert_bits_equal(stored(kout, "kout").view(2, 2, cout, cin), want(C.kout, dt), "fold: k*s")
    assert_bits_equal(stored(bout, "bout").view(2, 2, cout), want(C.bout, "f32"), "fold: b + sum k*h per tap")
    assert_bits_equal(stored(out.buf, "fwd").view(N, 2 * H, 2 * W, cout), want(C.out, dt), "folded tconv fwd")
    assert_bits_equal(stored(dk, "wgrad"), want(C.dk, "f32"), "folded tconv wgrad")


# ---- fused BN-backward input gradients -----------------------------------------------------------
def fused_outputs(C, dt, zf, pf, npar, regime, what):
    c = zf.shape[-1]
    assert_bits_equal(stored(zf, what + " dz_out"), want(C.dz_exact[dt], dt), what + " dz_out")
    if regime == "small":
        sums_equal(pf.view(-1, npar, c), C.part[dt], what + " column partials")


@pytest.mark.parametrize("sh,regime,dt", grid(KC.DGRAD_BN), ids=ids)
def test_conv3x3_dgrad_bn(sh, regime, dt):
    """dz_out, the plain columns of dx outside [c0, c1), the column partials (by parity where the
    case asks): kernel_cases.DGRAD_BN_BRANCH's rows put all three store paths among these cases."""
    from cnn_itmo_amd import ops
    from cnn_itmo_amd import _lib as L
    cin, cout, H, W, c0, c1, par = sh
    expect_kernels(KC.dgrad_bn_name(L.query, dt, cin, cout, H, W, c0, c1), KC.DGRAD_BN[sh][dt])
    C = E.dgrad_bn(cin, cout, H, W, c0, c1, par, regime)
    N, d, T, c = C.n, DT[dt], TDT[dt], c1 - c0
    wflip = torch.empty(C.w.size, dtype=T, device="cuda")
    ops.prep_conv3x3(d, cu(C.w), cout, cin, torch.empty_like(wflip), wflip)
    rv = ops.View(dev(widen(C.r, cin, c0), dt).reshape(-1), N, H, W, c, cin, c0)
    P, npar = N * H * W, 4 if par else 1
    frows = ops.conv3x3_dgrad_bn_rows(d, N, H, W, cout, cin, c0, c1)
    assert frows > 0
    whole = c0 == 0 and c1 == cin
    dx = None if whole else ops.View(nans(P * cin, T), N, H, W, cin, cin)
    zf, pf = nans(P * c, T), nans(frows * npar * c)
    ops.conv3x3_dgrad_bn(d, dev(C.dz, dt), N, H, W, cout, wflip, cin, dx, c0, c1, cu(C.coef), rv, zf, pf, par)
    torch.cuda.synchronize()
    fused_outputs(C, dt, zf.view(N, H, W, c), pf, npar, regime, "conv3x3_dgrad_bn")
    if not whole:
        gx = dx.buf.view(N, H, W, cin)
        plain = [i for i in range(cin) if not c0 <= i < c1]
        assert_bits_equal(stored(gx[..., plain], "dx"), want(C.g[..., plain], dt), "conv3x3_dgrad_bn plain dx columns")
        assert bool(torch.isnan(gx[..., c0:c1]).all()), "fused columns were written to dx"


@pytest.mark.parametrize("sh,regime,dt", grid(KC.DGRAD_BN_POOLED), ids=ids)
def test_conv3x3_dgrad_bn_pooled(sh, regime, dt):
    from cnn_itmo_amd import ops
    from cnn_itmo_amd import _lib as L
    cin, cout, H, W = sh
    expect_kernels(KC.dgrad_bn_pooled_name(L.query, dt, cin, cout, H, W), KC.DGRAD_BN_POOLED[sh][dt])
    C = E.dgrad_bn_pooled(cin, cout, H, W, regime)
    N, d, T = C.n, DT[dt], TDT[dt]
    wflip = torch.empty(C.w.size, dtype=T, device="cuda")
    ops.prep_conv3x3(d, cu(C.w), cout, C.cl, torch.empty_like(wflip), wflip)
    rv = ops.View(dev(C.r, dt).reshape(-1), N, H, W, cin, cin, 0)
    P = N * H * W
    frows = ops.conv3x3_dgrad_bn_pooled_rows(d, N, H, W, cout, cin)
    assert frows > 0
    zf, pf = nans(P * cin, T), nans(frows * cin)
    ops.conv3x3_dgrad_bn_pooled(d, dev(C.dz, dt), N, H, W, cout, wflip, cin, cu(C.coef), rv, dev(C.dyp, dt).reshape(-1),
                                torch.tensor(C.idx.reshape(-1)).cuda(), zf, pf)
    torch.cuda.synchronize()
    fused_outputs(C, dt, zf.view(N, H, W, cin), pf, 1, regime, "conv3x3_dgrad_bn_pooled")


@pytest.mark.parametrize("sh,regime,dt", grid(KC.TCONV_DGRAD_BN, ("bf16",)), ids=ids)
def test_tconv_dgrad_bn(sh, regime, dt):
    from cnn_itmo_amd import ops
    from cnn_itmo_amd import _lib as L
    cin, cout, H, W = sh
    expect_kernels(KC.tconv_dgrad_bn_name(L.query, dt, cin, cout, H, W), KC.TCONV_DGRAD_BN[sh])
    C = E.tconv_dgrad_bn(cin, cout, H, W, regime)
    N, d, T = C.n, DT[dt], TDT[dt]
    kT = torch.empty(C.k.size, dtype=T, device="cuda")
    ops.prep_tconv(d, cu(C.k), cout, cin, torch.empty_like(kT), kT)
    ld, off = cin + 32, 32
    rv = ops.View(dev(widen(C.r, ld, off), dt).reshape(-1), N, H, W, cin, ld, off)
    P = N * H * W
    frows = ops.tconv_dgrad_bn_rows(d, N, H, W, cout, cin)
    assert frows > 0
    zf, pf = nans(P * cin, T), nans(frows * cin)
    ops.tconv_dgrad_bn(d, dev(C.dout, dt).reshape(-1), N, H, W, cout, kT, cin, cu(C.coef), rv, zf, pf)
    torch.cuda.synchronize()
    fused_outputs(C, dt, zf.view(N, H, W, cin), pf, 1, regime, "tconv_dgrad_bn")


# ---- the 3-channel first layer -------------------------------------------------------------------
@pytest.mark.parametrize("sh,regime,dt", grid(E.FIRST_LAYER), ids=ids)
def test_first_layer_direct(sh, regime, dt):
    """conv_c3_fwd (ReLU + BN sums, output view, zero rows >= h_valid) and conv_c3_wgrad."""
    from cnn_itmo_amd import ops
    n, hv, H, W = sh
    ld, off = E.FIRST_LAYER_LD[sh]
    C = E.first_layer(n, hv, H, W, regime)
    d, T = DT[dt], TDT[dt]
    wp = torch.empty(32 * 32, dtype=T, device="cuda")
    ops.prep_c3(d, cu(C.w), 32, wp)
    buf = nans(n * H * W * ld, T)
    rows = ops.conv_c3_stat_rows(n, H, W)
    stats = nans(rows * 64)
    xd = cu(C.x)
    ops.conv_c3_fwd(d, xd, n, hv, H, W, wp, cu(C.b), ops.View(buf, n, H, W, 32, ld, off), flags=RELU | STATS, stats=stats)
    dw = nans((32, 27))
    ops.conv_c3_wgrad(d, xd, n, hv, H, W, dev(C.dz, dt), dw)
    torch.cuda.synchronize()
    got = buf.view(n, H, W, ld)
    assert_bits_equal(stored(got[..., off:off + 32], "fwd"), want(C.out, dt), "conv_c3_fwd")
    assert bool(torch.isnan(got[..., :off]).all()) and bool(torch.isnan(got[..., off + 32:]).all())
    if regime == "small":
        sums_equal(stats.view(rows, 2, 32), C.stats, "conv_c3_fwd stat rows")
    assert_bits_equal(stored(dw, "wgrad").view(32, 3, 3, 3), want(C.dw, "f32"), "conv_c3_wgrad")


@pytest.mark.parametrize("sh,regime,dt", grid(E.FIRST_LAYER[:1]), ids=ids)
def test_first_layer_im2col(sh, regime, dt):
    """im2col_c3's columns, conv1tap_fwd over them, and the one-tap weight gradient (27 columns)."""
    from cnn_itmo_amd import ops
    n, hv, H, W = sh
    C = E.first_layer(n, hv, H, W, regime)
    d, T = DT[dt], TDT[dt]
    cols = nans(n * H * W * 32, T)
    ops.im2col_c3(d, cu(C.x), n, hv, H, W, cols)
    wp = torch.empty(32 * 32, dtype=T, device="cuda")
    ops.prep_c3(d, cu(C.w), 32, wp)
    out = ops.View(nans(n * H * W * 32, T), n, H, W, 32, 32, 0)
    ops.conv1tap_fwd(d, cols, 32, n * H * W, wp, cu(C.b), out, flags=RELU)
    dw = nans((32, 27))
    ops.conv_wgrad(d, 1, ops.View(cols, n, H, W, 32, 32), dev(C.dz, dt), 32, dw, dw_cols=27)
    torch.cuda.synchronize()
    assert_bits_equal(stored(cols, "cols").view(n, H, W, 32), want(C.cols, dt), "im2col_c3")
    assert_bits_equal(stored(out.buf, "fwd").view(n, H, W, 32), want(C.out, dt), "conv1tap_fwd")
    assert_bits_equal(stored(dw, "wgrad").view(32, 3, 3, 3), want(C.dw, "f32"), "one-tap wgrad")


# ---- fused pooling and the concat readers --------------------------------------------------------
@pytest.mark.parametrize("sh,regime,dt", grid(E.POOL), ids=ids)
def test_conv3x3_fwd_pool(sh, regime, dt):
    """conv3x3_fwd_pool: the conv output as above; the pooled value and window index follow the rule
    launch_check_elem.py (_chk_pool_of_stored) and test_maxpool_ties state, restated in
    exact_cases.pool_first: per channel the first maximum, in window order (0,0), (0,1), (1,0),
    (1,1), of sign(pool_sign) * the STORED output (no sign: of the output; sign 0: the first
    element).  Integer outputs tie constantly, above all at the ReLU's zeros."""
    from cnn_itmo_amd import ops
    cin, cout, H, W = sh
    C = E.conv3x3(cin, cout, H, W, regime)
    N, d, T = C.n, DT[dt], TDT[dt]
    if not ops.pool_supported(d, N, H, W, cin, cout):
        pytest.skip("halo kernel does not take this shape")
    wf = torch.empty(C.w.size, dtype=T, device="cuda")
    ops.prep_conv3x3(d, cu(C.w), cout, cin, wf, None)
    xv = ops.View(dev(C.x, dt).reshape(-1), N, H, W, cin, cin)
    rows = ops.conv3x3_stat_rows(d, N, H, W, cin, cout)
    y = E.expected(C.out, dt)
    sign = np.resize([1.0, -0.5, 0.0, 3.0], cout)
    for sg in (sign, None):
        out = ops.View(nans(N * H * W * cout, T), N, H, W, cout, cout, 0)
        np_ = N * (H // 2) * (W // 2) * cout
        pv, pi = nans(np_, T), torch.full((np_,), 255, dtype=torch.uint8, device="cuda")
        st = nans((rows, 2, cout))
        ops.conv3x3_fwd_pool(d, xv, wf, cu(C.b), out, pv, pi, None if sg is None else cu(sg), flags=RELU | STATS, stats=st)
        torch.cuda.synchronize()
        assert_bits_equal(stored(out.buf, "fwd").view(N, H, W, cout), want(C.out, dt), "conv3x3_fwd_pool output")
        if regime == "small":
            sums_equal(st, C.stats, "conv3x3_fwd_pool stat rows")
        val, first = E.pool_first(y, sg)
        assert_bits_equal(pi.view(N, H // 2, W // 2, cout), torch.tensor(first), "pooled window index")
        assert_bits_equal(stored(pv, "pool").view(N, H // 2, W // 2, cout), want(val, dt), "pooled value")
    # the inference launch: ReLU + a dyadic affine (negative scales too) before the pooling, no sums;
    # pooled by the maximum of the stored output
    A = E.conv3x3(cin, cout, H, W, regime, False, True)
    ops.prep_conv3x3(d, cu(A.w), cout, cin, wf, None)
    out = ops.View(nans(N * H * W * cout, T), N, H, W, cout, cout, 0)
    pv, pi = nans(np_, T), torch.full((np_,), 255, dtype=torch.uint8, device="cuda")
    ops.conv3x3_fwd_pool(d, ops.View(dev(A.x, dt).reshape(-1), N, H, W, cin, cin), wf, cu(A.b), out, pv, pi, None,
                         flags=RELU | AFFINE, aff=(cu(A.sc), cu(A.sh)))
    torch.cuda.synchronize()
    assert_bits_equal(stored(out.buf, "fwd").view(N, H, W, cout), want(A.out, dt), "conv3x3_fwd_pool relu + affine output")
    val, first = E.pool_first(E.expected(A.out, dt))
    assert_bits_equal(pi.view(N, H // 2, W // 2, cout), torch.tensor(first), "pooled window index (affine)")
    assert_bits_equal(stored(pv, "pool").view(N, H // 2, W // 2, cout), want(val, dt), "pooled value (affine)")


@pytest.mark.parametrize("sh,regime,dt", grid(E.CAT, ("bf16",)), ids=ids)
def test_conv3x3_cat(sh, regime, dt):
    """conv3x3_fwd_cat and conv_wgrad_cat on dec9's [32 | 64] -> 64, each member a slice of a wider buffer."""
    from cnn_itmo_amd import ops
    H, W = sh
    c1, cin, cout = 32, 96, 64
    C = E.conv3x3(cin, cout, H, W, regime)
    N, d, T = C.n, DT[dt], TDT[dt]
    assert ops.fwd_cat_supported(d, N, H, W, c1, cin, cout) and ops.wgrad_cat_supported(N, H, W, c1, cin, cout)
    v1 = ops.View(dev(widen(C.x[..., :c1], 64, 32), dt).reshape(-1), N, H, W, c1, 64, 32)
    v2 = ops.View(dev(widen(C.x[..., c1:], 96, 32), dt).reshape(-1), N, H, W, cin - c1, 96, 32)
    wf = torch.empty(C.w.size, dtype=T, device="cuda")
    ops.prep_conv3x3(d, cu(C.w), cout, cin, wf, None)
    out = ops.View(nans(N * H * W * cout, T), N, H, W, cout, cout, 0)
    st = nans((ops.conv3x3_stat_rows(d, N, H, W, cin, cout), 2, cout))
    ops.conv3x3_fwd_cat(d, v1, v2, wf, cu(C.b), out, RELU | STATS, stats=st)
    dw = nans((cout, 3, 3, cin))
    ops.conv_wgrad_cat(d, v1, v2, dev(C.dz, dt), cout, dw)
    torch.cuda.synchronize()
    assert_bits_equal(stored(out.buf, "fwd").view(N, H, W, cout), want(C.out, dt), "conv3x3_fwd_cat")
    if regime == "small":
        sums_equal(st, C.stats, "conv3x3_fwd_cat stat rows")
    assert_bits_equal(stored(dw, "wgrad"), want(C.dw, "f32"), "conv_wgrad_cat")
