"""Every launching entry point under poison: kernels read and write only their operands.

Each case places EVERY operand of its launches (activations, weights, bias, coefficients,
partials, index bytes, outputs, workspaces) in a ``tests/arena.py`` Arena -- 1 MiB of poison
around each, bases 16-byte aligned and no more, views with ld > c and off > 0 -- launches
through the ``ops`` wrappers with a ``LaunchChecker`` active (each launch is compared with its
fp64 restatement from the very buffers it read, at launch_check.py's / launch_check_elem.py's
tolerances), and runs twice from the same seeded data: poison 0xFF (NaN in fp32 / bf16, an
invalid window index) and poison 0x00.  Workspaces the wrappers allocate themselves come from
the arena too (``ops.workspace`` is redirected).  Three properties are asserted:

  P1  complete writes: after the NaN run no element of a promised output is poison (or
      non-finite): every channel of an output view, every row and column of the stat /
      partial buffer its ``*_rows`` query reports, every index byte, dx on the padding rows,
      yhat, g3.  The totals of the BN sums (sum and sum of squares) are checked by the
      LaunchChecker at its own bound (1e-5 of the channel's sum of |values| / of squares).
  P2  no stray writes: ``check_untouched()`` under both fills (guards, the other member's
      channels of every view).
  P3  no stray reads: the outputs of the two runs are equal bit for bit (the kernels are
      deterministic, test_gpu_determinism.py).

In-place operands (maxpool_bwd's dx, optimizer slots, BN moving statistics) are payload.
adam, sgd and head_fwd_bwd_loss are not LaunchChecker entry points: they are compared with
tests/ref_objectives.py under test_gpu_losses.py's rules.

entry point (launch_check.LAUNCHES)      case
---------------------------------------  -----------------------------------------------
conv3x3_fwd (STATS / AFFINE / folded)    test_conv3x3
conv3x3_dgrad, conv_wgrad (9, + folded)  test_conv3x3
prep_conv3x3, fold_conv3x3               test_conv3x3
border_sums, colsum                      test_conv3x3 (colsum also test_bn, test_pool_route, the *_dgrad_bn cases)
bn_consumer_sums                         test_conv3x3 (mode 1), test_tconv (mode 2), test_head (mode 3)
conv3x3_fwd_pool, pool_bnsums_pooled     test_conv3x3_fwd_pool
conv3x3_fwd_head                         test_conv3x3_fwd_head
conv3x3_fwd_cat, conv_wgrad_cat          test_cat
conv3x3_dgrad_bn                         test_conv3x3_dgrad_bn
conv3x3_dgrad_bn_pooled                  test_conv3x3_dgrad_bn_pooled
tconv_dgrad_bn                           test_tconv_dgrad_bn
tconv_fwd (STATS / AFFINE / folded)      test_tconv
tconv_dgrad, tconv_wgrad (+ folded)      test_tconv
prep_tconv, fold_tconv                   test_tconv
conv_c3_fwd, conv_c3_wgrad, prep_c3      test_conv_c3
im2col_c3, conv1tap_fwd, conv_wgrad (1)  test_im2col_conv1tap
maxpool_fwd (+ folded), maxpool_bwd      test_maxpool
bn_fwd_finalize                          test_bn; test_conv3x3, test_tconv (groups 4): the kernels' own rows
bn_infer_coeffs                          test_bn
bn_apply (+ Dropout)                     test_bn
bn_bwd_reduce, bn_bwd_finalize           test_bn
bn_bwd_apply (+ Dropout, parity)         test_bn
pool_bnsums, bn_bwd_apply_pooled         test_pool_route
head_fwd, head_fwd_bwd, head_finalize    test_head
head_fwd_bwd_g3, bn_bwd_apply_g3         test_head
head_fwd_bwd_loss (logcosh; no checker)  test_head
rmsprop; adam, sgd (no checker)          test_optimizers
augment_affine, image_metrics (extra)    test_dense_pixel_kernels
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ref_objectives as RO  # noqa: E402
import kernel_cases as KC  # noqa: E402
from kernel_cases import expect_kernels  # noqa: E402
from arena import Arena, bits, poison_count  # noqa: E402
from launch_check import LaunchChecker  # noqa: E402

DT = {"f32": 0, "bf16": 1}
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
F32, U8 = torch.float32, torch.uint8
MiB = 1 << 20
# library calls made outside a LaunchChecker entry point that the cases check themselves
UNCHECKED_OK = {"cnnitmo_head_fwd_bwd_loss", "cnnitmo_adam", "cnnitmo_sgd"}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():  # the only skip: a machine without a GPU
        pytest.skip("no GPU")
    torch.backends.cuda.matmul.allow_tf32 = False
    from cnn_itmo_amd import _lib as L
    L.load()


class Run:
    """One run of a case: places operands in the arena."""

    def __init__(self, arena, dt):
        self.A, self.dt, self.d, self.T = arena, dt, DT[dt], TDT[dt]

    def put(self, a, dtype=F32, name=None):
        a = np.asarray(a)
        return self.A.take(a.size, dtype, data=a, name=name)

    def out(self, numel, dtype=F32, name=None):
        return self.A.take(numel, dtype, name=name)

    def act(self, a, ld, off, name=None, dtype=None):
        n, h, w, c = a.shape
        return self.A.view(n, h, w, c, ld, off, dtype or self.T, data=a, name=name)

    def outv(self, n, h, w, c, ld, off, name=None, channels=None):
        return self.A.view(n, h, w, c, ld, off, self.T, name=name, channels=channels)


def run_case(dt, body, expect, nbytes=64 * MiB, unchecked_ok=UNCHECKED_OK):
    """body(run) -> {name: tensor} of everything the launches promise to write.  Runs it under
    both fills and asserts P1, P2, P3; returns the NaN run's outputs."""
    from cnn_itmo_amd import ops
    outs = {}
    for fill in ("nan", "zero"):
        arena = Arena(nbytes, fill, "cuda")
        chk = LaunchChecker(ops, DT[dt], verbose=False)
        real_ws = ops.workspace
        ops.workspace = lambda nb, device="cuda": arena.take(max(16, int(nb)), U8, name="workspace")
        try:
            res = body(Run(arena, dt))
            torch.cuda.synchronize()
        finally:
            ops.workspace = real_ws
            chk.restore()
        arena.check_untouched()  # P2
        stray = set(chk.unchecked) - set(unchecked_ok)
        assert not stray, f"library calls outside a checked entry point: {stray}"
        missing = set(expect) - set(chk.calls)
        assert not missing, f"entry points never launched/checked: {missing}"
        outs[fill] = {k: v.clone() for k, v in res.items()}
        del arena
    for k, v in outs["nan"].items():  # P1
        assert v.numel() > 0
        bad = poison_count(v)
        assert bad == 0, f"{k}: {bad} of {v.numel()} promised elements were not written (still poison)"
        if v.dtype.is_floating_point:
            assert bool(torch.isfinite(v.float()).all()), f"{k}: non-finite values"
    for k, v in outs["nan"].items():  # P3
        z = outs["zero"][k]
        diff = int((bits(v) != bits(z)).sum())
        assert diff == 0, f"{k}: {diff} elements depend on memory outside the operands (NaN fill vs zero fill)"
    return outs["nan"]


def relu(a):
    return np.maximum(a, 0)


def rnd(a, T):
    """host values as the device dtype holds them (fp64)"""
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32).to(T).double().numpy()


# ---- Conv2D 3x3 ------------------------------------------------------------------------------
CONV_SHAPES = list(KC.CONV3X3_ARENA)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("cin,cout,H,W", CONV_SHAPES)
def test_conv3x3(dt, cin, cout, H, W):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    expect_kernels(KC.conv3x3_names(L.query, dt, cin, cout, H, W), KC.CONV3X3_ARENA[(cin, cout, H, W)][dt])

    def body(r):
        rng = np.random.default_rng(cin + cout)
        d, T, N = r.d, r.T, 2
        ld, off = cin + 32, 32
        xa = relu(rng.standard_normal((N, H, W, cin)))
        x = r.act(xa, ld, off, "x")
        w = (rng.standard_normal((cout, 3, 3, cin)) * 0.1).astype(np.float32)
        w32, bias = r.put(w, name="w32"), r.put(rng.standard_normal(cout), name="bias")
        wf, wflip = r.out(w.size, T, "wf"), r.out(w.size, T, "wflip")
        ops.prep_conv3x3(d, w32, cout, cin, wf, wflip)
        rows = ops.conv3x3_stat_rows(d, N, H, W, cin, cout)
        out = r.outv(N, H, W, cout, cout + 32, 32, "out")
        stats = r.out(rows * 2 * cout, name="stats")
        ops.conv3x3_fwd(d, x, wf, bias, out, L.RELU | L.STATS, stats=stats)
        # the finalize folds every row the query reports, idle workgroups' included
        gamma, beta = r.put(rng.uniform(0.5, 1.5, cout), name="gamma"), r.put(rng.standard_normal(cout), name="beta")
        mm = r.put(rng.uniform(0, 0.5, cout), name="moving_mean")
        mv = r.put(rng.uniform(0.5, 2, cout), name="moving_var")
        bn = [r.out(cout, name=nm) for nm in ("scale", "shift", "save_mean", "save_invstd")]
        ops.bn_fwd_finalize(stats, rows, cout, 1, N * H * W, gamma, beta, mm, mv, 0.99, 1e-3, *bn)
        sc, sh = r.put(rng.uniform(-2, 2, cout), name="aff_scale"), r.put(rng.standard_normal(cout), name="aff_shift")
        out2 = r.outv(N, H, W, cout, cout + 32, 32, "out_affine")
        ops.conv3x3_fwd(d, x, wf, bias, out2, L.RELU | L.AFFINE, aff=(sc, sh))
        dza = rng.standard_normal((N, H, W, cout))
        dz = r.put(dza, T, "dz")
        dx = r.outv(N, H, W, cin, ld, off, "dx")
        ops.conv3x3_dgrad(d, dz, N, H, W, cout, wflip, cin, dx)
        dw = r.out(w.size, name="dw")
        ops.conv_wgrad(d, 9, x, dz, cout, dw)
        # the folded-BN forms: x holds r, the conv's input is r*s + h
        s, h = r.put(rng.uniform(0.3, 2.0, cin), name="fold_s"), r.put(rng.standard_normal(cin), name="fold_h")
        wout, bout, border = r.out(w.size, T, "wout"), r.out(cout, name="bout"), r.out(cout * 8, name="border")
        ops.fold_conv3x3(d, w32, bias, s, h, cout, cin, wout, bout, border)
        # (no STATS here: conv + folded bias - border cancel, and with this data a channel that ReLU
        # clips almost everywhere keeps a few values of the size of that fp32 cancellation error,
        # which the checker's 1e-5 bound on the totals does not model; the sums path is the plain
        # launch's above)
        outf = r.outv(N, H, W, cout, cout + 32, 32, "out_folded")
        ops.conv3x3_fwd(d, x, wout, bout, outf, L.RELU, border=border)
        brows = ops.border_rows(N)
        bpart, bsum = r.out(brows * 8 * cout, name="border_part"), r.out(8 * cout, name="border_sum")
        ops.border_sums(d, dz, N, H, W, cout, bpart)
        ops.colsum(bpart, brows, 8 * cout, 1, bsum)
        db = r.put(rnd(dza, T).reshape(-1, cout).sum(0), name="db")
        dwf, raw = r.out(w.size, name="dw_folded"), r.out(w.size, name="dw_raw")
        ops.conv_wgrad(d, 9, x, dz, cout, dwf, fold=(s, h, db, bsum), raw=raw)
        c, ci0 = 32, cin - 32
        mean, inv = r.put(rng.uniform(0.2, 0.8, c), name="mean"), r.put(rng.uniform(0.5, 2.0, c), name="invstd")
        pm = r.out(L.CONSUMER_ROWS * 2 * c, name="consumer_part")
        ops.bn_consumer_sums(1, w32, raw, cout, cin, ci0, c, db, bsum, mean, inv, pm)
        return dict(wf=wf, wflip=wflip, out=out.tensor(), stats=stats, out_affine=out2.tensor(), dx=dx.tensor(),
                    dw=dw, wout=wout, bout=bout, border=border, out_folded=outf.tensor(),
                    border_part=bpart, border_sum=bsum, dw_folded=dwf, dw_raw=raw, consumer_part=pm,
                    moving_mean=mm, moving_var=mv, scale=bn[0], shift=bn[1], save_mean=bn[2], save_invstd=bn[3])

    run_case(dt, body, ["prep_conv3x3", "conv3x3_fwd", "bn_fwd_finalize", "conv3x3_dgrad", "conv_wgrad",
                        "fold_conv3x3", "border_sums", "colsum", "bn_consumer_sums"], nbytes=192 * MiB)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("cin,cout,H,W", [(32, 32, 6, 34), (64, 64, 18, 70)])
def test_conv3x3_fwd_pool(dt, cin, cout, H, W):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops

    def body(r):
        rng = np.random.default_rng(cin + H)
        d, T, N = r.d, r.T, 2
        assert ops.pool_supported(d, N, H, W, cin, cout)
        x = r.act(rng.standard_normal((N, H, W, cin)), cin + 32, 32, "x")
        w = (rng.standard_normal((cout, 3, 3, cin)) * 0.1).astype(np.float32)
        w32, bias = r.put(w, name="w32"), r.put(rng.standard_normal(cout), name="bias")
        wf, wflip = r.out(w.size, T, "wf"), r.out(w.size, T, "wflip")
        ops.prep_conv3x3(d, w32, cout, cin, wf, wflip)
        rows = ops.conv3x3_stat_rows(d, N, H, W, cin, cout)
        np_ = N * (H // 2) * (W // 2) * cout
        sign = r.put(np.resize([1.0, -0.5, 0.0, 3.0], cout), name="pool_sign")
        sc = r.put(np.resize([1.5, -0.75, 0.25, -2.0], cout), name="aff_scale")
        sh = r.put(rng.standard_normal(cout), name="aff_shift")
        res = {}
        for tag, sg, flags, aff in (("sign", sign, L.RELU | L.STATS, None), ("max", None, L.RELU | L.STATS, None),
                                    ("infer", None, L.RELU | L.AFFINE, (sc, sh))):
            out = r.outv(N, H, W, cout, cout + 32, 32, "out_" + tag)
            pv, pi = r.out(np_, T, "pool_out_" + tag), r.out(np_, U8, "pool_idx_" + tag)
            st = r.out(rows * 2 * cout, name="stats_" + tag) if flags & L.STATS else None
            ops.conv3x3_fwd_pool(d, x, wf, bias, out, pv, pi, sg, flags=flags, aff=aff, stats=st)
            res.update({"out_" + tag: out.tensor(), "pool_out_" + tag: pv, "pool_idx_" + tag: pi})
            if st is not None:
                res["stats_" + tag] = st
        # the pool's share of the producer's BN-backward sums, from the pooled r
        dyp = r.put(rng.standard_normal(np_), T, "dy_pool")
        mean, inv = r.put(rng.uniform(0.2, 0.8, cout), name="mean"), r.put(rng.uniform(0.5, 2.0, cout), name="invstd")
        prow = ops.bn_bwd_rows(N * (H // 2) * (W // 2), cout)
        pm = r.out(prow * 2 * cout, name="pool_bnsums_part")
        ops.pool_bnsums_pooled(d, dyp, res["pool_out_sign"], N, H, W, cout, mean, inv, pm)
        res["pool_bnsums_part"] = pm
        return res

    run_case(dt, body, ["conv3x3_fwd_pool", "pool_bnsums_pooled"])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("cin,H,W,hv", [(64, 5, 33, 3), (96, 18, 70, 17)])
def test_conv3x3_fwd_head(dt, cin, H, W, hv):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops

    def body(r):
        rng = np.random.default_rng(cin + H + hv)
        d, T, N, cout = r.d, r.T, 2, 64
        assert ops.head_supported(d, N, H, W, cin, cout)
        x = r.act(rng.standard_normal((N, H, W, cin)), cin + 32, 32, "x")
        w = (rng.standard_normal((cout, 3, 3, cin)) * 0.05).astype(np.float32)
        w32, bias = r.put(w, name="w32"), r.put(rng.standard_normal(cout) * 0.1, name="bias")
        wf = r.out(w.size, T, "wf")
        ops.prep_conv3x3(d, w32, cout, cin, wf, None)
        s, h = r.put(rng.uniform(0.5, 1.5, cout), name="aff_scale"), r.put(rng.normal(0, 0.2, cout), name="aff_shift")
        hw = r.put(rng.standard_normal((3, cout)) * 0.2, name="head_w")
        hb = r.put(rng.standard_normal(3), name="head_b")
        yhat = r.out(N * hv * W * 3, name="yhat")
        ops.conv3x3_fwd_head(d, x, wf, bias, cout, L.RELU | L.AFFINE, (s, h), hv, hw, hb, yhat)
        return dict(wf=wf, yhat=yhat)

    run_case(dt, body, ["conv3x3_fwd_head", "prep_conv3x3"])


@pytest.mark.parametrize("H,W", [(20, 70), (8, 40)])
def test_cat(H, W):
    """[32 | 64] -> 64 read from the two members (bf16), each a slice of a wider buffer."""
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops

    def body(r):
        rng = np.random.default_rng(H + W)
        d, T, N, c1, cin, cout = r.d, r.T, 2, 32, 96, 64
        assert ops.fwd_cat_supported(d, N, H, W, c1, cin, cout) and ops.wgrad_cat_supported(N, H, W, c1, cin, cout)
        x1 = r.act(relu(rng.standard_normal((N, H, W, 32))), 64, 32, "x1")
        x2 = r.act(relu(rng.standard_normal((N, H, W, 64))), 96, 32, "x2")
        w = (rng.standard_normal((cout, 3, 3, cin)) * 0.1).astype(np.float32)
        w32, bias = r.put(w, name="w32"), r.put(rng.standard_normal(cout), name="bias")
        wf = r.out(w.size, T, "wf")
        ops.prep_conv3x3(d, w32, cout, cin, wf, None)
        rows = ops.conv3x3_stat_rows(d, N, H, W, cin, cout)
        out, st = r.outv(N, H, W, cout, cout + 32, 32, "out"), r.out(rows * 2 * cout, name="stats")
        ops.conv3x3_fwd_cat(d, x1, x2, wf, bias, out, L.RELU | L.STATS, stats=st)
        dz = r.put(rng.standard_normal((N, H, W, cout)), T, "dz")
        dw = r.out(w.size, name="dw")
        ops.conv_wgrad_cat(d, x1, x2, dz, cout, dw)
        return dict(wf=wf, out=out.tensor(), stats=st, dw=dw)

    run_case("bf16", body, ["conv3x3_fwd_cat", "conv_wgrad_cat"])


@pytest.mark.parametrize("cin,cout,H,W,c0,c1,par", list(KC.DGRAD_BN))
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_conv3x3_dgrad_bn(cin, cout, H, W, c0, c1, par, dt):
    """The columns [c0, c1) leave through the producer's BN backward (dz_out, part); dx gets the
    others only: its columns [c0, c1) are NOT payload."""
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    expect_kernels(KC.dgrad_bn_name(L.query, dt, cin, cout, H, W, c0, c1), KC.DGRAD_BN[(cin, cout, H, W, c0, c1, par)][dt])

    def body(r):
        rng = np.random.default_rng(cin + c0 + H)
        d, T, N, c = r.d, r.T, 2, c1 - c0
        P = N * H * W
        w = (rng.standard_normal((cout, 3, 3, cin)) * 0.1).astype(np.float32)
        w32 = r.put(w, name="w32")
        wf, wflip = r.out(w.size, T, "wf"), r.out(w.size, T, "wflip")
        ops.prep_conv3x3(d, w32, cout, cin, wf, wflip)
        dz = r.put(rng.standard_normal((N, H, W, cout)), T, "dz")
        rv = r.act(relu(rng.standard_normal((N, H, W, c))), c + 32, 32, "r")
        coef = r.put(rng.standard_normal(3 * c), name="coef")
        frows = ops.conv3x3_dgrad_bn_rows(d, N, H, W, cout, cin, c0, c1)
        assert frows > 0
        whole = c0 == 0 and c1 == cin
        dx = None if whole else r.outv(N, H, W, cin, cin + 32, 32, "dx",
                                       channels=[(32, 32 + c0), (32 + c1, 32 + cin)])
        npar = 4 if par else 1
        zf, pf = r.out(P * c, T, "dz_out"), r.out(frows * npar * c, name="part")
        ops.conv3x3_dgrad_bn(d, dz, N, H, W, cout, wflip, cin, dx, c0, c1, coef, rv, zf, pf, par)
        sf = r.out(npar * c, name="part_sums")
        ops.colsum(pf, frows, npar * c, 1, sf)
        res = dict(dz_out=zf, part=pf, part_sums=sf)
        if dx is not None:
            t = dx.tensor()
            res["dx"] = torch.cat([t[..., :c0], t[..., c1:]], 3)
        return res

    run_case(dt, body, ["conv3x3_dgrad_bn", "colsum"])


@pytest.mark.parametrize("cin,cout,H,W", list(KC.DGRAD_BN_POOLED))
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_conv3x3_dgrad_bn_pooled(cin, cout, H, W, dt):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    expect_kernels(KC.dgrad_bn_pooled_name(L.query, dt, cin, cout, H, W), KC.DGRAD_BN_POOLED[(cin, cout, H, W)][dt])

    def body(r):
        rng = np.random.default_rng(cin + cout + H + W)
        d, T, N = r.d, r.T, 2
        P, cl = N * H * W, cin + 64
        w = (rng.standard_normal((cout, 3, 3, cl)) * 0.1).astype(np.float32)
        w32 = r.put(w, name="w32")
        wf, wflip = r.out(w.size, T, "wf"), r.out(w.size, T, "wflip")
        ops.prep_conv3x3(d, w32, cout, cl, wf, wflip)
        dz = r.put(rng.standard_normal((N, H, W, cout)), T, "dz")
        rv = r.act(relu(rng.standard_normal((N, H, W, cin))), cin + 32, 32, "r")
        np_ = N * (H // 2) * (W // 2) * cin
        dyp = r.put(rng.standard_normal(np_), T, "dy_pool")
        idx = r.put(rng.integers(0, 4, np_).astype(np.uint8), U8, "idx")
        coef = r.put(rng.standard_normal(3 * cin), name="coef")
        frows = ops.conv3x3_dgrad_bn_pooled_rows(d, N, H, W, cout, cin)
        assert frows > 0
        zf, pf = r.out(P * cin, T, "dz_out"), r.out(frows * cin, name="part")
        ops.conv3x3_dgrad_bn_pooled(d, dz, N, H, W, cout, wflip, cin, coef, rv, dyp, idx, zf, pf)
        sf = r.out(cin, name="part_sums")
        ops.colsum(pf, frows, cin, 1, sf)
        return dict(dz_out=zf, part=pf, part_sums=sf)

    run_case(dt, body, ["conv3x3_dgrad_bn_pooled", "colsum"])


# ---- Conv2DTranspose 2x2 ---------------------------------------------------------------------
TCONV_SHAPES = list(KC.TCONV_ARENA)


@pytest.mark.parametrize("cin,cout,H,W", list(KC.TCONV_DGRAD_BN))
def test_tconv_dgrad_bn(cin, cout, H, W):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    expect_kernels(KC.tconv_dgrad_bn_name(L.query, "bf16", cin, cout, H, W), KC.TCONV_DGRAD_BN[(cin, cout, H, W)])

    def body(r):
        rng = np.random.default_rng(cin + W)
        d, T, N = r.d, r.T, 2
        P = N * H * W
        k = (rng.standard_normal((2, 2, cout, cin)) * 0.1).astype(np.float32)
        k32 = r.put(k, name="k32")
        kf, kT = r.out(k.size, T, "kf"), r.out(k.size, T, "kT")
        ops.prep_tconv(d, k32, cout, cin, kf, kT)
        dout = r.put(rng.standard_normal((N, 2 * H, 2 * W, cout)), T, "dout")
        rv = r.act(relu(rng.standard_normal((N, H, W, cin))), cin + 32, 32, "r")
        coef = r.put(rng.standard_normal(3 * cin), name="coef")
        frows = ops.tconv_dgrad_bn_rows(d, N, H, W, cout, cin)
        assert frows > 0
        zf, pf = r.out(P * cin, T, "dz_out"), r.out(frows * cin, name="part")
        ops.tconv_dgrad_bn(d, dout, N, H, W, cout, kT, cin, coef, rv, zf, pf)
        sf = r.out(cin, name="part_sums")
        ops.colsum(pf, frows, cin, 1, sf)
        return dict(kf=kf, kT=kT, dz_out=zf, part=pf, part_sums=sf)

    run_case("bf16", body, ["tconv_dgrad_bn", "prep_tconv", "colsum"])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("cin,cout,H,W", TCONV_SHAPES)
def test_tconv(dt, cin, cout, H, W):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    expect_kernels(KC.tconv_names(L.query, dt, cin, cout, H, W), KC.TCONV_ARENA[(cin, cout, H, W)][dt])

    def body(r):
        rng = np.random.default_rng(cin)
        d, T, N = r.d, r.T, 2
        P = N * H * W
        xa = relu(rng.standard_normal((N, H, W, cin)))
        x = r.act(xa, cin, 0, "x")  # the tconv input is dense by contract
        k = (rng.standard_normal((2, 2, cout, cin)) * 0.1).astype(np.float32)
        k32, bias = r.put(k, name="k32"), r.put(rng.standard_normal(cout), name="bias")
        kf, kT = r.out(k.size, T, "kf"), r.out(k.size, T, "kT")
        ops.prep_tconv(d, k32, cout, cin, kf, kT)
        ld, off = cout + 64, 64
        rows = ops.tconv_stat_rows(d, N, H, W, cin, cout)
        out, stats = r.outv(N, 2 * H, 2 * W, cout, ld, off, "out"), r.out(rows * 2 * 4 * cout, name="stats")
        ops.tconv_fwd(d, x, kf, bias, out, L.RELU | L.STATS, stats=stats)
        # the finalize folds the four tap groups of every row the query reports
        gamma, beta = r.put(rng.uniform(0.5, 1.5, cout), name="gamma"), r.put(rng.standard_normal(cout), name="beta")
        mm = r.put(rng.uniform(0, 0.5, cout), name="moving_mean")
        mv = r.put(rng.uniform(0.5, 2, cout), name="moving_var")
        bn = [r.out(cout, name=nm) for nm in ("scale", "shift", "save_mean", "save_invstd")]
        ops.bn_fwd_finalize(stats, rows, cout, 4, 4 * P, gamma, beta, mm, mv, 0.99, 1e-3, *bn)
        sc, sh = r.put(rng.uniform(-2, 2, cout), name="aff_scale"), r.put(rng.standard_normal(cout), name="aff_shift")
        out2 = r.outv(N, 2 * H, 2 * W, cout, ld, off, "out_affine")
        ops.tconv_fwd(d, x, kf, bias, out2, L.RELU | L.AFFINE, aff=(sc, sh))
        s, h = r.put(rng.uniform(0.3, 2.0, cin), name="fold_s"), r.put(rng.standard_normal(cin), name="fold_h")
        kout, bout = r.out(k.size, T, "kout"), r.out(4 * cout, name="bout")
        ops.fold_tconv(d, k32, bias, s, h, cout, cin, kout, bout)
        out3 = r.outv(N, 2 * H, 2 * W, cout, ld, off, "out_folded")
        ops.tconv_fwd(d, x, kout, bout, out3, L.RELU | L.BIAS_PER_COL)
        da = rng.standard_normal((N, 2 * H, 2 * W, cout))
        dout = r.put(da, T, "dout")
        dx = r.out(P * cin, T, "dx")
        ops.tconv_dgrad(d, dout, N, H, W, cout, kT, cin, dx)
        dk = r.out(k.size, name="dk")
        ops.tconv_wgrad(d, x, dout, cout, dk)
        dor = rnd(da, T)
        par = r.put(np.stack([dor[:, i::2, j::2].sum((0, 1, 2)) for i in (0, 1) for j in (0, 1)]), name="parity_sums")
        dkf, raw = r.out(k.size, name="dk_folded"), r.out(k.size, name="dk_raw")
        ops.tconv_wgrad(d, x, dout, cout, dkf, fold=(s, h, par), raw=raw)
        c, ci0 = 32, cin - 32
        mean, inv = r.put(rng.uniform(0.2, 0.8, c), name="mean"), r.put(rng.uniform(0.5, 2.0, c), name="invstd")
        pm = r.out(L.CONSUMER_ROWS * 2 * c, name="consumer_part")
        ops.bn_consumer_sums(2, k32, raw, cout, cin, ci0, c, None, par, mean, inv, pm)
        return dict(kf=kf, kT=kT, out=out.tensor(), stats=stats, out_affine=out2.tensor(), kout=kout, bout=bout,
                    out_folded=out3.tensor(), dx=dx, dk=dk, dk_folded=dkf, dk_raw=raw, consumer_part=pm,
                    moving_mean=mm, moving_var=mv, scale=bn[0], shift=bn[1], save_mean=bn[2], save_invstd=bn[3])

    run_case(dt, body, ["prep_tconv", "tconv_fwd", "bn_fwd_finalize", "fold_tconv", "tconv_dgrad", "tconv_wgrad",
                        "bn_consumer_sums"], nbytes=160 * MiB)


# ---- first layer -----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("N,Hv,H,W,ld,off", [(2, 5, 6, 517, 32, 0), (1, 6, 7, 300, 96, 64)])
def test_conv_c3(N, Hv, H, W, ld, off, dt):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops

    def body(r):
        rng = np.random.default_rng(19)
        d, T = r.d, r.T
        x = r.put(rng.uniform(size=(N, Hv, W, 3)), name="x")
        w32 = r.put(rng.standard_normal((32, 3, 3, 3)) * 0.3, name="w32")
        bias = r.put(rng.standard_normal(32), name="bias")
        wp = r.out(32 * 32, T, "w_packed")
        ops.prep_c3(d, w32, 32, wp)
        rows = ops.conv_c3_stat_rows(N, H, W)
        out, stats = r.outv(N, H, W, 32, ld, off, "out"), r.out(rows * 64, name="stats")
        ops.conv_c3_fwd(d, x, N, Hv, H, W, wp, bias, out, L.RELU | L.STATS, stats=stats)
        sc, sh = r.put(rng.uniform(-2, 2, 32), name="aff_scale"), r.put(rng.standard_normal(32), name="aff_shift")
        out2 = r.outv(N, H, W, 32, ld, off, "out_affine")
        ops.conv_c3_fwd(d, x, N, Hv, H, W, wp, bias, out2, L.RELU | L.AFFINE, aff=(sc, sh))
        dz = r.put(rng.standard_normal((N, H, W, 32)), T, "dz")
        dw = r.out(32 * 27, name="dw")
        ops.conv_c3_wgrad(d, x, N, Hv, H, W, dz, dw)
        return dict(w_packed=wp, out=out.tensor(), stats=stats, out_affine=out2.tensor(), dw=dw)

    run_case(dt, body, ["prep_c3", "conv_c3_fwd", "conv_c3_wgrad"])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_im2col_conv1tap(dt):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops

    def body(r):
        rng = np.random.default_rng(9)
        d, T = r.d, r.T
        N, Hv, H, W = 2, 13, 16, 10
        m = N * H * W
        x = r.put(rng.uniform(size=(N, Hv, W, 3)), name="x")
        w32 = r.put(rng.standard_normal((32, 3, 3, 3)) * 0.3, name="w32")
        bias = r.put(rng.standard_normal(32), name="bias")
        cols = r.out(m * 32, T, "cols")
        ops.im2col_c3(d, x, N, Hv, H, W, cols)
        wp = r.out(32 * 32, T, "w_packed")
        ops.prep_c3(d, w32, 32, wp)
        out = r.outv(N, H, W, 32, 96, 64, "out")
        ops.conv1tap_fwd(d, cols, 32, m, wp, bias, out, L.RELU)
        sc, sh = r.put(rng.uniform(-2, 2, 32), name="aff_scale"), r.put(rng.standard_normal(32), name="aff_shift")
        out2 = r.outv(N, H, W, 32, 96, 64, "out_affine")
        ops.conv1tap_fwd(d, cols, 32, m, wp, bias, out2, L.RELU | L.AFFINE, aff=(sc, sh))
        dz = r.put(rng.standard_normal((N, H, W, 32)), T, "dz")
        dw = r.out(32 * 27, name="dw")
        ops.conv_wgrad(d, 1, ops.View(cols, N, H, W, 32, 32), dz, 32, dw, dw_cols=27)
        return dict(cols=cols, w_packed=wp, out=out.tensor(), out_affine=out2.tensor(), dw=dw)

    run_case(dt, body, ["im2col_c3", "conv1tap_fwd", "conv_wgrad", "prep_c3"])


# ---- pooling, BatchNormalization, head -------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_maxpool(dt):
    from cnn_itmo_amd import ops

    def body(r):
        rng = np.random.default_rng(4)
        d, T = r.d, r.T
        N, H, W, C, ld, off = 2, 6, 8, 32, 96, 64
        np_ = N * (H // 2) * (W // 2) * C
        x = r.act(rng.integers(-2, 3, size=(N, H, W, C)).astype(np.float64), ld, off, "x")  # many ties
        y, idx = r.out(np_, T, "y"), r.out(np_, U8, "idx")
        ops.maxpool_fwd(d, x, y, idx)
        dy = r.put(rng.standard_normal(np_), T, "dy")
        dx = r.act(rng.standard_normal((N, H, W, C)), ld, off, "dx")  # in place: payload
        ops.maxpool_bwd(d, dy, idx, dx)
        # over a folded BN output r*s + h with some negative scales
        x2 = r.act(relu(rng.standard_normal((N, H, W, C))), ld, off, "r")
        s = rng.uniform(0.3, 2.0, C) * np.where(rng.uniform(size=C) < 0.3, -1.0, 1.0)
        sc, sh = r.put(s, name="scale"), r.put(rng.standard_normal(C), name="shift")
        y2, idx2 = r.out(np_, T, "y_folded"), r.out(np_, U8, "idx_folded")
        ops.maxpool_fwd(d, x2, y2, idx2, aff=(sc, sh))
        return dict(y=y, idx=idx, dx=dx.tensor(), y_folded=y2, idx_folded=idx2)

    out = run_case(dt, body, ["maxpool_fwd", "maxpool_bwd"])
    assert int(out["idx"].max()) <= 3 and int(out["idx_folded"].max()) <= 3


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("C", [64, 96])
def test_bn(dt, drop, C):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops

    def body(r):
        rng = np.random.default_rng(5)
        d, T = r.d, r.T
        N, H, W = 2, 5, 7
        P = N * H * W
        ra = relu(rng.standard_normal((N, H, W, C)))
        rr = rnd(ra, T).reshape(-1, C)
        rt = r.put(ra, T, "r")
        rv = r.act(ra, C + 32, 32, "r_view")
        # partial sums as three workgroups' rows (the split is arbitrary: the finalize folds them)
        tot = np.stack([rr.sum(0), (rr ** 2).sum(0)])
        stats = r.put(np.stack([tot * 0.5, tot * 0.25, tot * 0.25]), name="stats")
        gamma, beta = r.put(rng.uniform(0.5, 1.5, C), name="gamma"), r.put(rng.standard_normal(C), name="beta")
        mm, mv = r.put(rng.uniform(0, 0.5, C), name="moving_mean"), r.put(rng.uniform(0.5, 2, C), name="moving_var")
        sc, sh, sm, si = (r.out(C, name=nm) for nm in ("scale", "shift", "save_mean", "save_invstd"))
        ops.bn_fwd_finalize(stats, 3, C, 1, P, gamma, beta, mm, mv, 0.99, 1e-3, sc, sh, sm, si)
        isc, ish = r.out(C, name="infer_scale"), r.out(C, name="infer_shift")
        ops.bn_infer_coeffs(C, gamma, beta, mm, mv, 1e-3, isc, ish)
        ld, off = C + 32, 32
        y = r.outv(N, H, W, C, ld, off, "y")
        seed, layer, flags = 123, 1, (L.DROPOUT if drop else 0)
        ops.bn_apply(d, rt, P, C, sc, sh, y, flags=flags, seed=seed, layer=layer)
        dyv = r.act(rng.standard_normal((N, H, W, C)), ld, off, "dy")
        rows = ops.bn_bwd_rows(P, C)
        part = r.out(rows * 2 * C, name="part")
        ops.bn_bwd_reduce(d, dyv, rv, C, sm, si, flags, seed, layer, part)
        dgam, dbet, coef = r.out(C, name="dgamma"), r.out(C, name="dbeta"), r.out(3 * C, name="coef")
        ops.bn_bwd_finalize(part, rows, C, P, gamma, sm, si, dgam, dbet, coef)
        dz, part2 = r.out(P * C, T, "dz"), r.out(rows * C, name="db_part")
        ops.bn_bwd_apply(d, dyv, rv, C, coef, flags, seed, layer, dz, part2)
        db = r.out(C, name="db")
        ops.colsum(part2, rows, C, 1, db)
        dz4, part4 = r.out(P * C, T, "dz_parity"), r.out(rows * 4 * C, name="parity_part")
        ops.bn_bwd_apply(d, dyv, rv, C, coef, flags | L.PARITY, seed, layer, dz4, part4)
        par = r.out(4 * C, name="parity_sums")
        ops.colsum(part4, rows, 4 * C, 1, par)
        dzn, partn = r.out(P * C, T, "dz_nobn"), r.out(rows * 4 * C, name="nobn_part")
        ops.bn_bwd_apply(d, dyv, rv, C, None, L.NO_BN | L.PARITY, 0, 0, dzn, partn)
        return dict(moving_mean=mm, moving_var=mv, scale=sc, shift=sh, save_mean=sm, save_invstd=si,
                    infer_scale=isc, infer_shift=ish, y=y.tensor(), part=part, dgamma=dgam, dbeta=dbet, coef=coef,
                    dz=dz, db_part=part2, db=db, dz_parity=dz4, parity_part=part4, parity_sums=par, dz_nobn=dzn,
                    nobn_part=partn)

    run_case(dt, body, ["bn_fwd_finalize", "bn_infer_coeffs", "bn_apply", "bn_bwd_reduce", "bn_bwd_finalize",
                        "bn_bwd_apply", "colsum"])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("H,W", [(6, 10), (7, 9)])
def test_pool_route(dt, H, W):
    from cnn_itmo_amd import ops

    def body(r):
        rng = np.random.default_rng(14)
        d, T = r.d, r.T
        N, C, ld, off = 2, 64, 96, 32
        Ho, Wo = H // 2, W // 2
        P, np_ = N * H * W, N * Ho * Wo * C
        rv = r.act(relu(rng.standard_normal((N, H, W, C))), ld, off, "r")
        dyv = r.act(rng.standard_normal((N, H, W, C)), ld, off, "dy")
        dyp = r.put(rng.standard_normal(np_), T, "dy_pool")
        idx = r.put(rng.integers(0, 4, np_).astype(np.uint8), U8, "idx")
        mean, inv = r.put(rng.uniform(0.2, 0.8, C), name="mean"), r.put(rng.uniform(0.5, 2.0, C), name="invstd")
        coef = r.put(rng.standard_normal(3 * C), name="coef")
        rows = ops.bn_bwd_rows(N * Ho * Wo, C)
        pm = r.out(rows * 2 * C, name="pool_part")
        ops.pool_bnsums(d, dyp, idx, rv, mean, inv, pm)
        sums = r.out(2 * C, name="pool_sums")
        ops.colsum(pm, rows, 2 * C, 1, sums)
        rows2 = ops.bn_bwd_rows(P, C)
        dz, pa = r.out(P * C, T, "dz"), r.out(rows2 * C, name="db_part")
        ops.bn_bwd_apply_pooled(d, dyv, rv, C, coef, dyp, idx, dz, pa)
        return dict(pool_part=pm, pool_sums=sums, dz=dz, db_part=pa)

    run_case(dt, body, ["pool_bnsums", "bn_bwd_apply_pooled", "colsum"])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C,H,W", [(16, 5, 13), (256, 4, 9)])
def test_head(dt, C, H, W):
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    from tests.test_gpu_ops import close
    N, Hv = 2, H - 1
    P, numel = N * H * W, N * Hv * W * 3
    rng0 = np.random.default_rng(6 + C)
    xa = relu(rng0.standard_normal((N, H, W, C)))
    wa = (rng0.standard_normal((3, C)) * 0.2).astype(np.float32)
    ba = rng0.standard_normal(3).astype(np.float32)
    ta = rng0.uniform(size=(N, Hv, W, 3)).astype(np.float32)

    def body(r):
        rng = np.random.default_rng(60 + C)
        d, T = r.d, r.T
        x = r.act(xa, C, 0, "x")  # the head input is dense by contract
        w, b, t = r.put(wa, name="head_w"), r.put(ba, name="head_b"), r.put(ta, name="target")
        yh = r.out(N * Hv * W * 3, name="yhat")
        ops.head_fwd(d, x, Hv, w, b, yh)
        rows = ops.head_rows(P)
        part, dx = r.out(rows * (5 + 3 * C), name="part"), r.out(P * C, T, "dx")
        ops.head_fwd_bwd(d, x, Hv, w, b, t, dx, part)
        la, dw, db = r.out(2, name="loss_acc"), r.out(3 * C, name="dw"), r.out(3, name="db")
        ops.head_finalize(part, rows, C, numel, la, dw, db)
        # the rank-3 form over a folded BN input, its finalize with the raw dW, the consumer-derived BN sums
        s, h = r.put(rng.uniform(0.3, 2.0, C), name="fold_s"), r.put(rng.standard_normal(C), name="fold_h")
        yh2 = r.out(N * Hv * W * 3, name="yhat_folded")
        ops.head_fwd(d, x, Hv, w, b, yh2, aff=(s, h))
        g3, part3 = r.out(P * 3, name="g3"), r.out(rows * (5 + 3 * C), name="part_g3")
        ops.head_fwd_bwd_g3(d, x, Hv, w, b, t, g3, part3, aff=(s, h))
        la3, dw3, db3, raw = (r.out(2, name="loss_acc_g3"), r.out(3 * C, name="dw_g3"), r.out(3, name="db_g3"),
                              r.out(3 * C, name="dw_raw"))
        ops.head_finalize(part3, rows, C, numel, la3, dw3, db3, aff=(s, h), raw=raw)
        mean, inv = r.put(rng.uniform(0.2, 0.8, C), name="mean"), r.put(rng.uniform(0.5, 2.0, C), name="invstd")
        pm = r.out(L.CONSUMER_ROWS * 2 * C, name="consumer_part")
        ops.bn_consumer_sums(3, w, raw, 3, C, 0, C, db3, None, mean, inv, pm)
        coef = r.put(rng.standard_normal(3 * C), name="coef")
        rv = r.act(xa, C + 32, 32, "r_view")
        brow = ops.bn_bwd_rows(P, C)
        dz, pz = r.out(P * C, T, "dz"), r.out(brow * C, name="db_part")
        ops.bn_bwd_apply_g3(d, g3, w, rv, C, P, coef, dz, pz)
        # one non-MSE loss (not a LaunchChecker entry point: checked below against ref_objectives)
        partl, dxl = r.out(rows * (5 + 3 * C), name="part_logcosh"), r.out(P * C, T, "dx_logcosh")
        ops.head_fwd_bwd_loss(L.LOSSES["logcosh"], d, x, Hv, w, b, t, partl, dx=dxl)
        lal, dwl, dbl = r.out(2, name="loss_acc_logcosh"), r.out(3 * C, name="dw_logcosh"), r.out(3, name="db_logcosh")
        ops.head_finalize(partl, rows, C, numel, lal, dwl, dbl)
        return dict(yhat=yh, part=part, dx=dx, loss_acc=la, dw=dw, db=db, yhat_folded=yh2, g3=g3, part_g3=part3,
                    loss_acc_g3=la3, dw_g3=dw3, db_g3=db3, dw_raw=raw, consumer_part=pm, dz=dz, db_part=pz,
                    part_logcosh=partl, dx_logcosh=dxl, loss_acc_logcosh=lal, dw_logcosh=dwl, db_logcosh=dbl)

    out = run_case(dt, body, ["head_fwd", "head_fwd_bwd", "head_fwd_bwd_g3", "head_finalize", "bn_consumer_sums",
                              "bn_bwd_apply_g3"])
    # logcosh against the fp64 reference, test_gpu_losses._check_head's rules
    xin = rnd(xa, TDT[dt])[:, :Hv]
    yref = RO.sigmoid(xin @ wa.T.astype(np.float64) + ba)
    t64 = ta.astype(np.float64)
    gz = RO.grad_z("logcosh", yref, t64)
    dx_ref = np.zeros((N, H, W, C))
    dx_ref[:, :Hv] = gz @ wa.astype(np.float64)
    host = lambda v: v.float().cpu().numpy().astype(np.float64)  # noqa: E731
    assert abs(float(out["loss_acc_logcosh"][0]) - RO.loss("logcosh", yref, t64)) < 1e-5
    close(host(out["dw_logcosh"]).reshape(3, C), gz.reshape(-1, 3).T @ xin.reshape(-1, C), "f32", "logcosh dw")
    close(host(out["db_logcosh"]), gz.reshape(-1, 3).sum(0), "f32", "logcosh db")
    close(host(out["dx_logcosh"]).reshape(dx_ref.shape) * 1e3, dx_ref * 1e3, dt, "logcosh dx")


def test_optimizers():
    """n = 1003 (a scalar tail after the 16-byte vectors); the slots and p are in-place payload."""
    from cnn_itmo_amd import ops
    n = 1003
    rng0 = np.random.default_rng(7)
    v = {k: rng0.standard_normal(n).astype(np.float32) for k in ("p", "g", "m")}
    v["a"] = rng0.uniform(size=n).astype(np.float32)

    def body(r):
        g = r.put(v["g"], name="g")
        p1, a1 = r.put(v["p"], name="rmsprop_p"), r.put(v["a"], name="rmsprop_a")
        ops.rmsprop(p1, g, a1, 1e-3, 0.9, 1e-7, grad_scale=0.5)
        p2, m2, v2 = r.put(v["p"], name="adam_p"), r.put(v["m"] * 0.1, name="adam_m"), r.put(v["a"], name="adam_v")
        lr_t = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
        ops.adam(p2, g, m2, v2, lr_t, 0.9, 0.999, 1e-7, grad_scale=0.5)
        p3, m3 = r.put(v["p"], name="sgd_p"), r.put(v["m"] * 0.1, name="sgd_mom")
        ops.sgd(p3, g, m3, 1e-2, momentum=0.9, nesterov=True, grad_scale=0.5)
        p4, m4 = r.put(v["p"], name="sgd0_p"), r.put(v["m"] * 0.1, name="sgd0_mom")
        ops.sgd(p4, g, m4, 1e-2, grad_scale=0.5)
        return dict(rmsprop_p=p1, rmsprop_a=a1, adam_p=p2, adam_m=m2, adam_v=v2, sgd_p=p3, sgd_mom=m3, sgd0_p=p4,
                    sgd0_mom=m4)

    out = run_case("f32", body, ["rmsprop"])
    f64 = {k: a.astype(np.float64) for k, a in v.items()}
    g = f64["g"] * 0.5
    got = {k: t.cpu().numpy() for k, t in out.items()}
    p, a = RO.rmsprop(f64["p"], g, f64["a"])
    np.testing.assert_allclose(got["rmsprop_p"], p, atol=1e-6)
    np.testing.assert_allclose(got["rmsprop_a"], a, atol=1e-6)
    m0 = (v["m"] * 0.1).astype(np.float32).astype(np.float64)
    p, m, vv = RO.adam(f64["p"], g, m0, f64["a"], 0)
    for k, want in (("adam_p", p), ("adam_m", m), ("adam_v", vv)):
        np.testing.assert_allclose(got[k], want, atol=1e-6, err_msg=k)
    p, m = RO.sgd(f64["p"], g, m0, momentum=0.9, nesterov=True)
    np.testing.assert_allclose(got["sgd_p"], p, atol=1e-6)
    np.testing.assert_allclose(got["sgd_mom"], m, atol=1e-6)
    p, m = RO.sgd(f64["p"], g, m0)
    np.testing.assert_allclose(got["sgd0_p"], p, atol=1e-6)
    np.testing.assert_allclose(got["sgd0_mom"], m, atol=1e-6)


@pytest.mark.parametrize("u8", [False, True])
def test_dense_pixel_kernels(u8):
    """augment_affine and image_metrics (one thread per pixel over dense tensors; no LaunchChecker
    entry): P1-P3, plus the values that have a closed form here -- an identity map returns the
    source times scale exactly, MSE / PSNR against fp64 numpy.  Their interpolation and SSIM
    values are pinned by test_gpu_metrics.py and the data-generator tests."""
    from cnn_itmo_amd import ops
    n, h, w = 2, 13, 19  # 3*w % 4 != 0: image_metrics' one-element path; odd sizes
    rng0 = np.random.default_rng(31)
    src = rng0.integers(0, 256, (n, h, w, 3)).astype(np.uint8) if u8 else rng0.uniform(size=(n, h, w, 3))
    other = np.random.default_rng(32).uniform(size=(n, h, w, 3))
    th = 0.3
    mats = np.array([[1, 0, 0, 0, 1, 0],
                     [np.cos(th), -np.sin(th), 2.5, np.sin(th), np.cos(th), -1.25]], np.float64)
    scale = 1.0 / 255.0 if u8 else 0.5

    def body(r):
        s = r.put(src, U8 if u8 else F32, "src")
        m = r.put(mats, torch.float64, "mats")
        fl = r.put(np.array([0, 3], np.int32), torch.int32, "flips")
        dst = r.out(n * h * w * 3, name="dst")
        ops.augment_affine(s.view(n, h, w, 3), m, fl, scale, dst.view(n, h, w, 3))
        b = r.put(other, name="b")
        met = r.out(n * 3, torch.float64, "metrics")
        ops.image_metrics(ops.MSE_PSNR | ops.SSIM, dst.view(n, h, w, 3), b.view(n, h, w, 3), 1.0, met.view(n, 3))
        return dict(dst=dst, metrics=met, b=b)

    out = run_case("f32", body, [], unchecked_ok={"cnnitmo_augment_affine", "cnnitmo_image_metrics"})
    dst = out["dst"].view(n, h, w, 3).cpu().numpy()
    want0 = (src[0].astype(np.float32) * np.float32(scale))
    np.testing.assert_array_equal(dst[0], want0)  # identity map, no flip
    d64, b64 = dst.astype(np.float64), out["b"].view(n, h, w, 3).double().cpu().numpy()
    mse = ((d64 - b64) ** 2).reshape(n, -1).mean(1)
    met = out["metrics"].view(n, 3).cpu().numpy()
    np.testing.assert_allclose(met[:, 0], mse, rtol=1e-12)
    np.testing.assert_allclose(met[:, 1], 10 * np.log10(1.0 / mse), rtol=1e-12)
    assert (np.abs(met[:, 2]) <= 1.0).all()


def test_checker_has_teeth_on_the_gpu():
    """A plain torch write into a guard, and one into a view's foreign channel, each fail
    check_untouched on the device arena."""
    a = Arena(8 * MiB, "nan", "cuda")
    t = a.take(256, torch.float32, name="victim")
    v = a.view(1, 4, 4, 32, 96, 32, torch.bfloat16, name="concat")
    t.fill_(1.0)
    v.tensor().fill_(2.0)
    a.check_untouched()
    start = a.carves[0][1]
    a.buf[start + 1024 + 64:start + 1024 + 68] = 0  # one float past the end, 64 bytes on
    with pytest.raises(AssertionError, match=r"guard of carve 'victim'.*offset \+1088 "):
        a.check_untouched()
    a.buf[start + 1024 + 64:start + 1024 + 68] = 0xFF
    a.check_untouched()
    v.buf.view(4 * 4, 96)[3, 5] = 1.0  # pixel 3, channel 5: the other concat member's
    with pytest.raises(AssertionError, match="non-payload byte inside carve 'concat'"):
        a.check_untouched()
