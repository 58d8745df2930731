"""Without a GPU: the operands of every case tests/test_gpu_exact.py (and tests/halo0_child.py) runs
meet their regime's preconditions (tests/exact_cases.py asserts them on the fp64 oracle while it
builds a case; the figures are asserted again and printed here), the method notices one removed
product and a truncating store, and every kernel the shared case lists launch has an exact case."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import exact_cases as E  # noqa: E402
from tests import kernel_cases as KC  # noqa: E402
from tests.exact_cases import assert_bits_equal  # noqa: E402

TDT = {"f32": torch.float32, "bf16": torch.bfloat16}


def want(exact, dt):
    return torch.tensor(np.ascontiguousarray(exact), dtype=torch.float32).to(TDT[dt])


def differs(a, b, dt, what):
    """assert_bits_equal must fail on the two expected tensors."""
    with pytest.raises(AssertionError, match="differ in their bits"):
        assert_bits_equal(want(a, dt), want(b, dt), what)


def figures(C, dirs):
    """The recorded figures of a built case against the regime's bounds."""
    p = C.pre
    print(C.regime, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in p.items()})
    for d in dirs:
        if C.regime == "small":
            assert p[d + "_sum_abs"] <= 256 and p[d + "_min_frac"] >= p[d + "_floor"] >= 28.0 / 256
        else:
            assert p[d + "_sum_abs"] < 2 ** 24 and p[d + "_nonrep"] >= 0.05 and p[d + "_ties"] >= 1
    if "wgrad_sum_abs" in p:
        assert p["wgrad_sum_abs"] < 2 ** 24 and p["wgrad_min_frac"] >= 1.0 / 8


def rne_is_torch(*arrays):
    """exact_cases.bf16_rne (used for the contracts' intermediate roundings) is torch's conversion."""
    for a in arrays:
        assert np.array_equal(E.bf16_rne(a), want(a, "bf16").double().numpy())


# ---- preconditions of every GPU case -------------------------------------------------------------
C3_SHAPES = sorted(set(KC.CONV3X3_OPS) | set(KC.CONV3X3_HALO0) | set(E.POOL) | {(96, 64) + hw for hw in E.CAT})


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("sh", C3_SHAPES, ids=str)
def test_conv3x3_cases(sh, regime):
    C = E.conv3x3(*sh, regime)
    figures(C, ("fwd", "dgrad"))
    rne_is_torch(C.out, C.dx)
    assert C.dw.dtype == np.float64 and np.array_equal(C.dw, np.round(C.dw))


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("sh", list(KC.CONV3X3_FOLD), ids=str)
def test_conv3x3_fold_cases(sh, regime):
    C = E.conv3x3(*sh, regime, True)
    figures(C, ("fwd",))
    assert set(np.abs(C.s)) <= {0.5, 1.0, 2.0, 4.0} and np.array_equal(C.h, np.round(C.h)) and (C.r >= 0).all()
    # the folded kernel's own operands give the same exact z: sum (w*s) r + bout - border correction
    z = E.c3(C.r, C.wout) + C.bout
    top, bot, lef, rig = (np.zeros((C.H, C.W, 1), bool) for _ in range(4))
    top[0], bot[-1], lef[:, 0], rig[:, -1] = True, True, True, True
    U = C.border
    z -= (top * U[:, 0] + bot * U[:, 1] + lef * U[:, 2] + rig * U[:, 3] - (top & lef) * U[:, 4] - (top & rig) * U[:, 5]
          - (bot & lef) * U[:, 6] - (bot & rig) * U[:, 7])
    assert np.array_equal(z, C.z)


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("key", sorted({(cin, cout, H, W, 1) for (_dt, H, W, cin, cout) in KC.AFFINE_HALO0}
                                        | {sh + (E.N,) for sh in E.POOL}), ids=str)
def test_conv3x3_affine_cases(key, regime):
    """The ReLU + dyadic-affine forwards: AFFINE_HALO0's (one image) and the pooled inference launch's."""
    cin, cout, H, W, n = key
    C = E.conv3x3(cin, cout, H, W, regime, False, True, n)
    figures(C, ("fwd",))
    assert set(np.abs(C.sc)) <= {0.5, 1.0, 2.0, 4.0} and np.array_equal(C.sh, np.round(C.sh))


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("sh", list(KC.TCONV_OPS), ids=str)
def test_tconv_cases(sh, regime):
    C = E.tconv(*sh, regime)
    figures(C, ("fwd", "dgrad"))
    rne_is_torch(C.out, C.dx)


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("sh", list(KC.TCONV_FOLD), ids=str)
def test_tconv_fold_cases(sh, regime):
    C = E.tconv(*sh, regime, True)
    figures(C, ("fwd",))
    z = E.tf(C.r, C.kout) + np.broadcast_to(C.bout[None, None, :, None, :, :], (C.n, C.H, 2, C.W, 2, C.cout)).reshape(C.z.shape)
    assert np.array_equal(z, C.z)


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("sh", list(KC.TCONV_AFFINE), ids=str)
def test_tconv_affine_cases(sh, regime):
    figures(E.tconv(*sh, regime, False, True), ("fwd",))


def fused_figures(C):
    figures(C, ())
    p, c = C.pre, C.coef
    assert set(c[0]) <= {0.5, 1.0, 2.0} and set(c[1]) <= {0.5, 1.0, 2.0} and np.array_equal(c[2] * 2, np.round(c[2] * 2))
    if C.regime == "small":
        assert p["dgrad_sum_abs"] <= 256 and p["dgrad_min_frac"] >= 1.0 / 8
        for dt in ("bf16", "f32"):
            v = C.dz_exact[dt]
            assert np.array_equal(v * 4, np.round(v * 4)) and E.is_bf16(v).all()
            assert np.array_equal(C.dz_out[dt], v)
    else:
        assert p["dz_bf16_nonrep"] >= 0.05 and p["dz_bf16_ties"] >= 1
        # the named intermediate rounding matters: the expected value is not the rounding of a*g - b*r + e
        a, b, e = c
        g = C.g[..., C.c0:C.c1] if hasattr(C, "c0") else C.g
        once = E.bf16_rne(np.where(C.r > 0, a * (g + getattr(C, "routed", 0.0)) - b * C.r + e, 0.0))
        assert np.mean(once != C.dz_out["bf16"]) > 0.01
    rne_is_torch(C.g, C.dz_exact["bf16"])


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("sh", list(KC.DGRAD_BN), ids=str)
def test_dgrad_bn_cases(sh, regime):
    fused_figures(E.dgrad_bn(*sh, regime))


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("sh", list(KC.DGRAD_BN_POOLED), ids=str)
def test_dgrad_bn_pooled_cases(sh, regime):
    C = E.dgrad_bn_pooled(*sh, regime)
    fused_figures(C)
    assert np.count_nonzero(C.routed) == np.count_nonzero(C.dyp)


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("sh", list(KC.TCONV_DGRAD_BN), ids=str)
def test_tconv_dgrad_bn_cases(sh, regime):
    fused_figures(E.tconv_dgrad_bn(*sh, regime))


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("sh", E.FIRST_LAYER, ids=str)
def test_first_layer_cases(sh, regime):
    C = E.first_layer(*sh, regime)
    print(regime, C.pre)
    assert sh in E.FIRST_LAYER_LD and C.pre["fwd_min_frac"] >= 1.0 / 8
    if regime == "wide":
        assert C.pre["fwd_nonrep"] >= 0.05 and C.pre["fwd_ties"] >= 1
    below = C.out[:, C.hv + 1:]  # rows that see only the zero rows >= h_valid: relu(bias)
    assert np.array_equal(below, np.broadcast_to(np.maximum(C.b, 0), below.shape))


def test_pool_rule_is_the_oracles():
    """exact_cases.pool_first without a sign is oracle.maxpool2x2 (first maximum in window order), on
    integer data full of ties; with a sign: max, min (negative) and the first element (zero)."""
    from oracle import unet_ref as R
    y = np.random.default_rng(5).integers(-2, 3, (2, 6, 8, 8)).astype(np.float64)
    v, i = E.pool_first(y)
    vr, ir = R.maxpool2x2(y)
    assert np.array_equal(v, vr) and np.array_equal(i, ir)
    v, i = E.pool_first(y, np.resize([1.0, -0.5, 0.0, 3.0], 8))
    vn, inn = R.maxpool2x2(-y)
    assert np.array_equal(v[..., 0::4], vr[..., 0::4]) and np.array_equal(v[..., 1::4], -vn[..., 1::4])
    assert np.array_equal(i[..., 1::4], inn[..., 1::4]) and not i[..., 2::4].any()
    assert np.array_equal(v[..., 2::4], y[:, 0::2, 0::2, 2::4])


# ---- the method notices what the tolerances hid --------------------------------------------------
def test_assert_bits_equal_reports():
    a = torch.zeros(2, 3, 4, 8, dtype=torch.bfloat16)
    b = a.clone()
    b[0, 1, 2, 3] = -0.0
    assert_bits_equal(a, b, "signed zero")
    b[1, 2, 3, 7] = 2.0 ** -133  # one bit
    with pytest.raises(AssertionError, match=r"(?s)1 of 192 elements differ.*\[7\].*\(1, 2, 3, 7\): got 0.0, want"):
        assert_bits_equal(a, b, "one bit")
    c = a.clone()
    c[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="got nan"):
        assert_bits_equal(c, a, "unwritten")
    with pytest.raises(AssertionError):
        assert_bits_equal(a.float(), a, "dtype")


def pixels(H, W):
    return [(0, 0), (0, W // 2), (H // 2, W // 2), (H - 1, W - 1)]  # corner, edge, interior, last corner


def first_and_last(nz):
    """The first and the last index (in storage order) of a boolean field's True entries."""
    idx = np.argwhere(nz)
    return [tuple(idx[0]), tuple(idx[-1])]


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_one_removed_product_is_noticed_conv(dt):
    """3x3 forward (through the ReLU: positive outputs) and input gradient, small regime: the element
    recomputed from its receptive field equals the oracle's, and with one nonzero product left out
    (first / last nonzero (tap, channel) of corner, edge and interior pixels) the comparison fails."""
    C = E.conv3x3(96, 64, 6, 10, "small")
    xp = np.pad(C.x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    tried = 0
    for n in (0, C.n - 1):
        for (h, w) in pixels(C.H, C.W):
            field = xp[n, h:h + 3, w:w + 3]  # [3,3,cin]
            for co in (int(np.argmax(C.z[n, h, w] > 0)), C.cout - 1 - int(np.argmax(C.z[n, h, w, ::-1] > 0))):
                prod = field * C.w[co]
                assert prod.sum() + C.b[co] == C.z[n, h, w, co] > 0
                for k in first_and_last(prod != 0):
                    z = C.z.copy()
                    z[n, h, w, co] -= prod[k]
                    differs(np.maximum(z, 0), C.out, dt, "forward")
                    tried += 1
    dzp = np.pad(C.dz, ((0, 0), (1, 1), (1, 1), (0, 0)))
    for (h, w) in pixels(C.H, C.W):
        for ci in (0, C.cin - 1):
            # dx[h, w, ci] = sum_{r,s,co} dz[h - (r-1), w - (s-1), co] * wd[co, r, s, ci]
            prod = dzp[0, h:h + 3, w:w + 3][::-1, ::-1] * C.wd[:, :, :, ci].transpose(1, 2, 0)
            assert prod.sum() == C.dx[0, h, w, ci]
            for k in first_and_last(prod != 0):
                dx = C.dx.copy()
                dx[0, h, w, ci] -= prod[k]
                differs(dx, C.dx, dt, "input gradient")
                tried += 1
    assert tried == 2 * 4 * 2 * 2 + 4 * 2 * 2


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_one_removed_product_is_noticed_tconv(dt):
    C = E.tconv(128, 64, 3, 70, "small")
    for (h, w) in pixels(2 * C.H, 2 * C.W):
        for co in (int(np.argmax(C.z[0, h, w] > 0)), C.cout - 1 - int(np.argmax(C.z[0, h, w, ::-1] > 0))):
            prod = C.x[0, h // 2, w // 2] * C.k[h % 2, w % 2, co]
            assert prod.sum() + C.b[co] == C.z[0, h, w, co] > 0
            for k in first_and_last(prod != 0):
                z = C.z.copy()
                z[0, h, w, co] -= prod[k]
                differs(np.maximum(z, 0), C.out, dt, "tconv forward")
    for (h, w) in pixels(C.H, C.W):
        for ci in (0, C.cin - 1):
            prod = C.dout[1, 2 * h:2 * h + 2, 2 * w:2 * w + 2] * C.kd[:, :, :, ci]
            assert prod.sum() == C.dx[1, h, w, ci]
            for k in first_and_last(prod != 0):
                dx = C.dx.copy()
                dx[1, h, w, ci] -= prod[k]
                differs(dx, C.dx, dt, "tconv input gradient")


def test_one_removed_product_is_noticed_wgrad():
    """Weight gradients (fp32 outputs, both regimes): one (pixel) product left out of one element."""
    for regime in E.REGIMES:
        C = E.conv3x3(96, 64, 6, 10, regime)
        xp = np.pad(C.x, ((0, 0), (1, 1), (1, 1), (0, 0)))
        for co, r, s, ci in ((0, 0, 0, 0), (C.cout - 1, 2, 2, C.cin - 1), (5, 1, 1, 40), (C.cout - 1, 0, 2, 0)):
            prod = xp[:, r:r + C.H, s:s + C.W, ci] * C.dz[..., co]
            assert prod.sum() == C.dw[co, r, s, ci]
            for k in first_and_last(prod != 0):
                dw = C.dw.copy()
                dw[co, r, s, ci] -= prod[k]
                differs(dw, C.dw, "f32", "weight gradient")
        T = E.tconv(128, 64, 3, 70, regime)
        for a, b, co, ci in ((0, 0, 0, 0), (1, 1, T.cout - 1, T.cin - 1), (0, 1, 7, 64)):
            prod = T.x[..., ci] * T.dout[:, a::2, b::2, co]
            assert prod.sum() == T.dk[a, b, co, ci]
            for k in first_and_last(prod != 0):
                dk = T.dk.copy()
                dk[a, b, co, ci] -= prod[k]
                differs(dk, T.dk, "f32", "tconv weight gradient")


def test_truncation_and_double_rounding_are_noticed():
    """Wide regime: a store that truncates, or rounds to nearest with ties away from zero, differs
    from the expected tensor (the preconditions put non-representable values and ties in every case)."""
    cases = [E.conv3x3(32, 32, 8, 12, "wide").out, E.conv3x3(32, 32, 8, 12, "wide").dx, E.tconv(64, 32, 3, 5, "wide").out,
             E.tconv(64, 32, 3, 5, "wide").dx, E.dgrad_bn(32, 32, 20, 40, 0, 32, False, "wide").dz_exact["bf16"],
             E.first_layer(2, 13, 16, 10, "wide").out]
    for exact in cases:
        rne = want(exact, "bf16")
        trunc = torch.tensor(E.bf16_trunc(exact), dtype=torch.float32).to(torch.bfloat16)
        with pytest.raises(AssertionError, match="differ in their bits"):
            assert_bits_equal(trunc, rne, "truncating store")
        lo = E.bf16_trunc(exact)  # towards zero; a tie's other neighbour is 2 |exact - lo| further out
        away = np.where(E.is_tie(exact), lo + np.sign(exact) * 2 * np.abs(exact - lo), E.bf16_rne(exact))
        with pytest.raises(AssertionError, match="differ in their bits"):
            assert_bits_equal(torch.tensor(away, dtype=torch.float32).to(torch.bfloat16), rne, "ties away from zero")


# ---- every kernel of the shared lists has an exact case ------------------------------------------
def test_every_tested_kernel_has_an_exact_case():
    """Every name in kernel_cases.tested(q) and tested(q, halo0=True) is launched by an exact case
    (exact_cases.launched, the same name queries): a kernel added to the lists later needs one too.
    CNNITMO_HALO is read once per process, so each world is asked in a child of its own."""
    from tests.test_abi_and_host import run_child
    from cnn_itmo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    n = 0
    for env in (None, {"CNNITMO_HALO": "0"}):
        out = json.loads(run_child("exact_names", env=env)[-1])
        missing = {k: v for k, v in out["tested"].items() if k not in out["launched"]}
        assert not missing, f"kernels the shared lists launch but no exact case does: {missing}"
        n += len(out["launched"])
    assert n > 90
