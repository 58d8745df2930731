"""Operands for the bit-for-bit conv kernel tests (host only: numpy and the oracle, no device).

The tolerance tests feed the GEMM-like kernels standard_normal data, where a wrong kernel and a
reordered sum look the same.  Here every operand is a small integer (scales: signed powers of
two), chosen per case so that no order of summation, with or without FMA contraction, rounds
anything.  A correct kernel then equals the fp64 oracle in every bit, and a missing or doubled
(tap, channel) product, a wrong tile-edge mask or a wrong rounding mode moves a result by at
least one unit.

Two regimes:

"small"  everything is exact wherever a rounding could happen.  Asserted on the reference:
         every value is an integer (a multiple of 1/4 after a dyadic affine or the fused BN
         backward) that bf16 holds; sum_k |w_k x_k| <= 256 for every output element, so every
         partial sum in any order is a bf16 integer as well; per channel sum |r| and sum r^2
         over the whole case are below 2^24 (fp32 stat partials are exact however rows are
         split); weight gradients and column partials are below 2^24 in sum of absolute terms;
         at least 1/8 of the products of every output element's receptive field (the in-image
         taps x channels) are nonzero.
"wide"   dense, larger integers: |z| reaches the hundreds to thousands, far past bf16's 256
         exact integers, with sum |w x| < 2^24 so that the fp32 accumulation is still exact.  The
         stored bf16 tensor must be the one round-to-nearest-even of the exact value (fp32 stores
         equal it).  Asserted on the reference: at least 5 % of the stored values are not bf16
         numbers and at least one is an exact tie, so a truncating or twice-rounding store
         cannot pass.  Only stored tensors are compared in this regime.

How "small" meets its bounds: weights carry exactly m nonzero entries per (output column, tap),
activations are nonzero almost everywhere, and m * taps * max|x| * max|w| (+ max|bias|) <= 256.
The product floor and the sum bound exclude each other where taps * channels / 8 > 256 (each
nonzero integer product is at least 1): the 3x3 conv from 256 channels (K = 2304).  There the
sum bound stands, since exactness rests on it, and the floor is the densest the bound allows,
m = 28 of 256 channels per tap (floor()).  After a dyadic affine the stored relu(z)*sc + sh must stay a
bf16 number as well: sum |w x| <= 60 with scales up to 4, or, where 1/8 of the products is more than
that (K = 512 and the 3x3 conv from 128 channels), <= 240 with scales +-1/2 and +-1 only.

Intermediate roundings the contracts name are part of the expected value: the fused BN backward
applies its coefficients to bf16(g) (include/cnn_itmo.h, cnnitmo_conv3x3_dgrad_bn_pooled: "a*(bf16(g) +
routed) - b*r + e"; launch_check.py::_bnb_ref for the other two fused input gradients).
"""
import functools
import zlib
from types import SimpleNamespace as NS

import numpy as np

from oracle import unet_ref as R
from tests import kernel_cases as KC

N = KC.N
REGIMES = ("small", "wide")
LIM24 = float(2 ** 24)
F32 = np.float32


# ---- number formats ------------------------------------------------------------------------------
def bf16_rne(a):
    """Round-to-nearest-even to bf16 (finite values), as float64."""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F32).astype(np.float64).reshape(np.shape(a))


def bf16_trunc(a):
    """Truncation to bf16 (what a store that drops the low 16 bits gives), as float64."""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(F32).astype(np.float64).reshape(np.shape(a))


def is_bf16(a):
    return bf16_trunc(a) == np.asarray(a, dtype=np.float64)


def is_tie(a):
    """Exactly halfway between two neighbouring bf16 numbers (a holds fp32-exact values)."""
    return (np.ascontiguousarray(a, dtype=F32).view(np.uint32) & np.uint32(0xFFFF)) == 0x8000


def expected(exact, dt):
    """The tensor a correct kernel stores for the exact value: one RNE rounding in bf16."""
    return bf16_rne(exact) if dt == "bf16" else np.asarray(exact, dtype=np.float64)


# ---- the comparison ------------------------------------------------------------------------------
def assert_bits_equal(got, want, what):
    """got and want (torch tensors of one dtype, or numpy arrays) agree in every bit of their
    storage, -0.0 counting as +0.0.  The report names how many elements differ and the first few
    as (n, h, w, c) with both values: 'last column of a tile' or 'channel 31 of every block' show."""
    import torch
    g = got if isinstance(got, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(got))
    w = want if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want))
    g, w = g.detach().cpu(), w.detach().cpu()
    assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {g.dtype}{tuple(g.shape)} vs {w.dtype}{tuple(w.shape)}"
    iv = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[g.element_size()]
    gb, wb = g.contiguous().view(iv), w.contiguous().view(iv)
    if g.dtype.is_floating_point:  # -0.0 == +0.0: clear the sign bit of zeros
        gb = torch.where(g == 0, torch.zeros_like(gb), gb)
        wb = torch.where(w == 0, torch.zeros_like(wb), wb)
    bad = gb != wb
    nbad = int(bad.sum())
    if nbad:
        idx = bad.nonzero()[:8]
        rows = [f"{tuple(int(v) for v in i)}: got {g[tuple(i)].item()!r}, want {w[tuple(i)].item()!r}" for i in idx]
        last = bad.nonzero()[:, -1]
        raise AssertionError(f"{what}: {nbad} of {bad.numel()} elements differ in their bits; last-axis indices "
                             f"{sorted(set(last.tolist()))[:16]}; first at (n, h, w, c)-style index\n  " + "\n  ".join(rows))


# ---- the linear maps (float32 in: float32 out, exact for these integers; float64 for the references)
def c3(x, w):
    return R.conv2d_same(x, w)


def c3d(dz, w):
    """Input gradient of the 3x3 conv with weights w [cout,3,3,cin], as conv2d_same_bwd computes it."""
    return R.conv2d_same(dz, np.ascontiguousarray(w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0)))


def tf(x, k):
    return R.tconv2x2s2(x, k)


def td(dout, k):
    n, h2, w2, co = dout.shape
    d = dout.reshape(n, h2 // 2, 2, w2 // 2, 2, co)
    return sum(d[:, :, a, :, b, :] @ k[a, b] for a in (0, 1) for b in (0, 1))


def floor(taps, c, cap=256):
    """The nonzero-product floor of a map with `taps` taps of c channels: 1/8, or the densest that
    sum |w x| <= cap allows with integer operands (module doc)."""
    return min(1.0 / 8, (cap // taps) / c)


def _products(op, act, wt):
    """(max sum |w x|, min share of nonzero products) over the outputs of op(act, wt)."""
    tot = op(np.abs(act).astype(F32), np.abs(wt).astype(F32))
    cnt = op((act != 0).astype(F32), (wt != 0).astype(F32))
    field = op(np.ones(act.shape, F32), np.ones(wt.shape, F32))
    return float(tot.max()), float((cnt / field).min())


# ---- operand generators --------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else int(k) for k in key])


def _ints(rng, shape, amax, pz=0.0, nonneg=False):
    """Integers of magnitude 1..amax, random sign (or none), zero with probability pz."""
    v = rng.integers(1, amax + 1, size=shape).astype(np.float64)
    if not nonneg:
        v *= rng.choice([-1.0, 1.0], size=shape)
    if pz:
        v *= rng.random(shape) >= pz
    return v


def _dense(rng, shape, amax):
    return rng.integers(-amax, amax + 1, size=shape).astype(np.float64)


def _sparse_rows(rng, rows, k, m, wmax):
    """[rows, k] with exactly m nonzero integers (magnitude 1..wmax) per row."""
    pos = np.argsort(rng.random((rows, k)), axis=1)[:, :m]
    out = np.zeros((rows, k))
    np.put_along_axis(out, pos, _ints(rng, (rows, m), wmax), axis=1)
    return out


def _small_plan(taps, c, cap):
    """(m nonzero weights per (column, tap), max |activation|, max |weight|): m * taps * amax * wmax <= cap."""
    lim = cap // taps
    m = min(max(-(-c // 8), c // 4), lim)
    amax, wmax = {1: (1, 1), 2: (2, 1), 3: (3, 1)}.get(lim // m, (2, 2))
    return m, amax, wmax


def _wide_amps(k):
    """(max |activation|, max |weight|) for std(z) of about 600 over k dense products."""
    ab = 1800.0 / np.sqrt(k)
    b = int(max(2, min(8, round(np.sqrt(ab / 4)))))
    return int(max(3, min(120, round(ab / b)))), b


def _weights(rng, kind, cin, cout, m, wmax, dense):
    """Weights of one map.  kind c3f / c3d: [cout,3,3,cin]; tf / td: [2,2,cout,cin].  Sparse along the
    summed channel axis: cin for the forwards, cout for the input gradients."""
    t = 9 if kind[0] == "c" else 4
    if dense:
        return _dense(rng, (cout, 3, 3, cin) if t == 9 else (2, 2, cout, cin), wmax)
    if kind == "c3f":
        return _sparse_rows(rng, cout * 9, cin, m, wmax).reshape(cout, 3, 3, cin)
    if kind == "c3d":
        return np.ascontiguousarray(_sparse_rows(rng, cin * 9, cout, m, wmax).reshape(cin, 3, 3, cout).transpose(3, 1, 2, 0))
    if kind == "tf":
        return _sparse_rows(rng, 4 * cout, cin, m, wmax).reshape(2, 2, cout, cin)
    return np.ascontiguousarray(_sparse_rows(rng, 4 * cin, cout, m, wmax).reshape(2, 2, cin, cout).transpose(0, 1, 3, 2))


OPS = {"c3f": (c3, 9), "c3d": (c3d, 9), "tf": (tf, 1), "td": (td, 4)}


def _gemm_operands(rng, kind, regime, ashape, cin, cout, cap=256, nonneg=False, act=None):
    """(activation, weights, figures) of one map meeting its regime's product preconditions.
    ashape: the activation's shape (channels last: cin for a forward, cout for an input gradient);
    act(rng, amax) -> a ready activation bounded by amax (the folded inputs)."""
    op, taps = OPS[kind]
    c = ashape[-1]
    if regime == "wide":
        amax, wmax = _wide_amps(taps * c)
        a = act(rng, amax) if act else (_ints(rng, ashape, amax, 0.1, True) if nonneg else _dense(rng, ashape, amax))
        w = _weights(rng, kind, cin, cout, 0, wmax, True)
        tot, frac = _products(op, a, w)
        assert tot < LIM24, f"{kind} wide: sum |w x| = {tot}"
        return a, w, dict(sum_abs=tot, min_frac=frac)
    m, amax, wmax = _small_plan(taps, c, cap)
    fl = floor(taps, c, cap)
    # (a frame of a few pixels: no zeros, or some weight-gradient element's few products all vanish)
    for pz in (0.15, 0.0) if np.prod(ashape[:-1]) >= 256 else (0.0,):
        a = act(rng, amax) if act else _ints(rng, ashape, amax, pz, nonneg)
        w = _weights(rng, kind, cin, cout, m, wmax, False)
        tot, frac = _products(op, a, w)
        if tot <= cap and frac >= fl:
            return a, w, dict(sum_abs=tot, min_frac=frac, floor=fl, m=m)
    raise AssertionError(f"{kind} small {ashape} {cin}->{cout}: sum |w x| = {tot} (<= {cap}), nonzero share {frac} (>= {fl})")


def _check_stored(exact, regime, what):
    """Preconditions on a stored tensor's exact value."""
    if regime == "small":
        assert np.all(exact * 4 == np.round(exact * 4)) and is_bf16(exact).all(), f"{what}: not exact in bf16"
        return {}
    nonrep, ties = float(np.mean(~is_bf16(exact))), int(is_tie(exact).sum())
    assert float(np.abs(exact).max()) < LIM24
    assert nonrep >= 0.05 and ties >= 1, f"{what}: {nonrep:.3f} of the values are no bf16 numbers, {ties} ties"
    return {"nonrep": nonrep, "ties": ties, "max": float(np.abs(exact).max())}


def _check_stats(r, what):
    """Per channel sum |r| and sum r^2 below 2^24; returns the exact (sum r, sum r^2) [2][c]."""
    r2 = r.reshape(-1, r.shape[-1])
    s = np.stack([r2.sum(0), (r2 * r2).sum(0)])
    assert np.abs(r2).sum(0).max() < LIM24 and s[1].max() < LIM24, f"{what}: stat sums reach {s.max()}"
    return s


def _check_wgrad(op_bwd, x, d, what, fl=1.0 / 8):
    """Weight gradient sums below 2^24 in absolute terms, the 1/8 floor over each element's products
    (none for the raw sum over r of a folded input: the reference is the gradient on y)."""
    tot = op_bwd(np.abs(x).astype(F32), np.abs(d).astype(F32))
    cnt = op_bwd((x != 0).astype(F32), (d != 0).astype(F32))
    field = op_bwd(np.ones(x.shape, F32), np.ones(d.shape, F32))
    frac = float((cnt[field > 0] / field[field > 0]).min())  # (a one-row frame: the taps above and below see nothing)
    assert float(tot.max()) < LIM24 and frac >= fl, f"{what}: sum |dz x| = {tot.max()}, nonzero share {frac}"
    return dict(wgrad_sum_abs=float(tot.max()), wgrad_min_frac=frac)


def _c3_dw(x, d):
    return R.conv2d_same_bwd(x, np.zeros((d.shape[-1], 3, 3, x.shape[-1]), x.dtype), d, need_dx=False)[1]


def _t_dw(x, d):
    n, h, w, ci = x.shape
    d6 = d.reshape(n, h, 2, w, 2, -1)
    x2 = x.reshape(-1, ci)
    return np.stack([np.stack([np.ascontiguousarray(d6[:, :, a, :, b, :]).reshape(-1, d6.shape[-1]).T @ x2
                               for b in (0, 1)]) for a in (0, 1)])


def _dyadic(rng, c, mags):
    return rng.choice(mags, c) * rng.choice([-1.0, 1.0], c)


def _folded(rng, shape, amax):
    """A folded BN input: r >= 0 (integers), s a signed power of two, h an integer with
    y = r*s + h an integer in [-amax, amax] (r is even where |s| = 1/2)."""
    c = shape[-1]
    s = _dyadic(rng, c, [m for m in (0.5, 1.0, 2.0, 4.0) if m <= 2 * amax])
    q = np.where(np.abs(s) < 1, 2.0, 1.0)
    h = -np.sign(s) * amax
    nu = np.floor(2 * amax / (np.abs(s) * q))
    u = np.floor(rng.random(shape) * (nu + 1))
    u2 = np.floor(rng.random(shape) * (nu + 1))
    u = np.where(u * q * s + h == 0, u2, u)  # few zeros of y: the product floor counts w*y
    r = u * q
    return r, s, h, r * s + h


# ---- cases ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def conv3x3(cin, cout, H, W, regime, fold=False, aff=False, n=N):
    """Forward z = conv(x, w) + b and relu(z) [with a folded input y = r*s + h, or followed by a dyadic
    affine]; input gradient dx of dz through its own weights wd; weight gradient dw of (x or y, dz)."""
    rng = _rng("conv3x3", cin, cout, H, W, regime, fold, aff)
    pre = {}
    capf = 253  # |bias| <= 3
    mags = (0.5, 1.0, 2.0, 4.0)
    if aff and regime == "small":  # relu(z)*sc + sh must stay a bf16 number
        capf, mags = (60, mags) if 60 // 9 >= -(-cin // 8) else (240, (0.5, 1.0))
    C = NS(cin=cin, cout=cout, H=H, W=W, n=n, regime=regime, pre=pre)
    if fold:
        keep = {}

        def act(g, amax):
            keep["rshy"] = _folded(g, (n, H, W, cin), amax)
            return keep["rshy"][3]
        y, C.w, p = _gemm_operands(rng, "c3f", regime, (n, H, W, cin), cin, cout, capf, act=act)
        C.r, C.s, C.h, C.x = keep["rshy"]
        assert (C.r >= 0).all() and np.array_equal(C.x, y)
    else:
        C.x, C.w, p = _gemm_operands(rng, "c3f", regime, (n, H, W, cin), cin, cout, capf)
    pre.update({"fwd_" + k: v for k, v in p.items()})
    C.b = _dense(rng, cout, 3)
    C.z = c3(C.x, C.w) + C.b
    C.out = np.maximum(C.z, 0)
    assert np.all(C.z == np.round(C.z))
    if aff:
        C.sc, C.sh = _dyadic(rng, cout, mags), _dense(rng, cout, 3)
        C.out = C.out * C.sc + C.sh
    pre.update({"fwd_" + k: v for k, v in _check_stored(C.out, regime, "forward").items()})
    if regime == "small":
        assert np.abs(C.z).max() <= 256
        C.stats = _check_stats(C.out, "forward")
    if fold:
        ws = C.w * C.s
        assert is_bf16(ws).all() and is_bf16(C.r).all()
        u = np.einsum("orsc,c->ors", C.w, C.h)
        C.wout, C.bout = ws, C.b + u.sum((1, 2))
        C.border = np.stack([u[:, 0].sum(1), u[:, 2].sum(1), u[:, :, 0].sum(1), u[:, :, 2].sum(1),
                             u[:, 0, 0], u[:, 0, 2], u[:, 2, 0], u[:, 2, 2]], 1)
        fabs = c3(np.abs(C.r).astype(F32), np.abs(ws).astype(F32)).max() + np.abs(C.bout).max() + 4 * np.abs(C.border).max()
        assert fabs < LIM24
    if aff:
        return C
    C.dz, C.wd, p = _gemm_operands(rng, "c3d", regime, (n, H, W, cout), cin, cout)
    pre.update({"dgrad_" + k: v for k, v in p.items()})
    C.dx, C.dw, C.db = R.conv2d_same_bwd(C.x, C.wd, C.dz)
    pre.update({"dgrad_" + k: v for k, v in _check_stored(C.dx, regime, "input gradient").items()})
    pre.update(_check_wgrad(_c3_dw, C.x, C.dz, "weight gradient"))
    if fold:
        d = C.dz
        C.bsum = np.stack([d[:, 0].sum((0, 1)), d[:, -1].sum((0, 1)), d[:, :, 0].sum((0, 1)), d[:, :, -1].sum((0, 1)),
                           d[:, 0, 0].sum(0), d[:, 0, -1].sum(0), d[:, -1, 0].sum(0), d[:, -1, -1].sum(0)])
        # the kernel sums dz (x) r, then corrects: both below 2^24 in absolute terms
        pre["raw_sum_abs"] = _check_wgrad(_c3_dw, C.r, C.dz, "raw weight gradient", 0.0)["wgrad_sum_abs"]
        assert np.abs(C.h).max() * np.abs(d).reshape(-1, cout).sum(0).max() < LIM24
    return C


@functools.lru_cache(maxsize=2)
def tconv(cin, cout, H, W, regime, fold=False, aff=False, n=N, grads=True):
    """Conv2DTranspose 2x2: forward (K = cin per output), input gradient (K = 4 cout) through its own
    weights kd, weight gradient of (x or y, dout)."""
    rng = _rng("tconv", cin, cout, H, W, regime, fold, aff)
    pre = {}
    capf = 253
    mags = (0.5, 1.0, 2.0, 4.0)
    if aff and regime == "small":
        capf, mags = (60, mags) if 60 >= -(-cin // 8) else (240, (0.5, 1.0))
    C = NS(cin=cin, cout=cout, H=H, W=W, n=n, regime=regime, pre=pre)
    if fold:
        keep = {}

        def act(g, amax):
            keep["rshy"] = _folded(g, (n, H, W, cin), amax)
            return keep["rshy"][3]
        y, C.k, p = _gemm_operands(rng, "tf", regime, (n, H, W, cin), cin, cout, capf, act=act)
        C.r, C.s, C.h, C.x = keep["rshy"]
        assert (C.r >= 0).all() and np.array_equal(C.x, y)
    else:
        C.x, C.k, p = _gemm_operands(rng, "tf", regime, (n, H, W, cin), cin, cout, capf)
    pre.update({"fwd_" + k: v for k, v in p.items()})
    C.b = _dense(rng, cout, 3)
    C.z = tf(C.x, C.k) + C.b
    C.out = np.maximum(C.z, 0)
    assert np.all(C.z == np.round(C.z))
    if aff:
        C.sc, C.sh = _dyadic(rng, cout, mags), _dense(rng, cout, 3)
        C.out = C.out * C.sc + C.sh
    pre.update({"fwd_" + k: v for k, v in _check_stored(C.out, regime, "forward").items()})
    if regime == "small":
        assert np.abs(C.z).max() <= 256
        C.stats = _check_stats(C.out, "forward")
    if fold:
        assert is_bf16(C.k * C.s).all() and is_bf16(C.r).all()
        C.kout = C.k * C.s
        C.bout = C.b + np.einsum("aboc,c->abo", C.k, C.h)  # [2][2][cout]: one bias per (tap, column)
        assert tf(np.abs(C.r).astype(F32), np.abs(C.kout).astype(F32)).max() + np.abs(C.bout).max() < LIM24
    if aff or not grads:
        return C
    C.dout, C.kd, p = _gemm_operands(rng, "td", regime, (n, 2 * H, 2 * W, cout), cin, cout)
    pre.update({"dgrad_" + k: v for k, v in p.items()})
    C.dx, C.dk, _ = R.tconv2x2s2_bwd(C.x, C.kd, C.dout)
    pre.update({"dgrad_" + k: v for k, v in _check_stored(C.dx, regime, "input gradient").items()})
    pre.update(_check_wgrad(_t_dw, C.x, C.dout, "weight gradient"))
    if fold:
        d = C.dout
        C.par = np.stack([d[:, i::2, j::2].sum((0, 1, 2)) for i in (0, 1) for j in (0, 1)])
        _check_wgrad(_t_dw, C.r, C.dout, "raw weight gradient", 0.0)
        assert np.abs(C.h).max() * np.abs(d).reshape(-1, cout).sum(0).max() < LIM24
    return C


def _coef(rng, c, regime):
    """Fused BN-backward coefficients (a, b, e) [3][c]: a, b powers of two, e an integer or a half.
    small: where a = 1 the value a*g - b*r + e stays an integer (b >= 1, e an integer); where a = 1/2
    it is a multiple of 1/2 below 128."""
    if regime == "wide":
        a, b = rng.choice([0.5, 1.0, 2.0], c), rng.choice([0.5, 1.0, 2.0], c)
        return np.stack([a, b, rng.integers(-5, 6, c) / 2.0])
    a = rng.choice([0.5, 1.0], c)
    b = np.where(a == 1.0, rng.choice([1.0, 2.0], c), rng.choice([0.5, 1.0, 2.0], c))
    e = np.where(a == 1.0, rng.integers(-3, 4, c).astype(np.float64), rng.integers(-3, 4, c) / 2.0)
    return np.stack([a, b, e])


def _bnb(g, r, coef, dt, routed=0.0):
    """dz = [r>0]*(a*(g' + routed) - b*r + e), g' = bf16(g) in bf16 (the contract's intermediate rounding)."""
    a, b, e = coef
    gb = bf16_rne(g) if dt == "bf16" else g
    return np.where(r > 0, a * (gb + routed) - b * r + e, 0.0)


def _part(v, parity):
    """Column sums of the stored dz, [4][c] by (h&1, w&1) with parity, else [1][c]."""
    if not parity:
        return v.sum((0, 1, 2))[None]
    return np.stack([v[:, i::2, j::2].sum((0, 1, 2)) for i in (0, 1) for j in (0, 1)])


def _bnb_finish(C, g, rng, regime, routed=0.0, parity=False):
    """r, coef and per dtype the exact dz / stored dz / partial sums of a fused BN-backward case."""
    c = g.shape[-1]
    C.r = _ints(rng, g.shape, 3 if regime == "wide" else 2, 0.3, True)
    C.coef = _coef(rng, c, regime)
    C.dz_exact, C.dz_out, C.part = {}, {}, {}
    for dt in ("bf16", "f32"):
        v = _bnb(g, C.r, C.coef, dt, routed)
        C.pre.update({f"dz_{dt}_{k}": x for k, x in _check_stored(v, regime, "fused dz").items()})
        assert float(np.abs(v).max()) * 4 < LIM24
        C.dz_exact[dt], C.dz_out[dt] = v, expected(v, dt)
        if regime == "small":
            C.part[dt] = _part(C.dz_out[dt], parity)
            assert np.abs(C.dz_out[dt]).reshape(-1, c).sum(0).max() < LIM24
    return C


@functools.lru_cache(maxsize=2)
def dgrad_bn(cin, cout, H, W, c0, c1, par, regime, n=N):
    """cnnitmo_conv3x3_dgrad_bn: g = the input gradient of dz through w; columns [c0, c1) go through
    the producer's BN backward with r (a view of c1 - c0 channels at offset c0 of a cin-wide buffer)."""
    rng = _rng("dgrad_bn", cin, cout, H, W, c0, regime)
    C = NS(cin=cin, cout=cout, H=H, W=W, n=n, c0=c0, c1=c1, par=par, regime=regime, pre={})
    C.dz, C.w, p = _gemm_operands(rng, "c3d", regime, (n, H, W, cout), cin, cout, cap=244)
    C.pre.update({"dgrad_" + k: v for k, v in p.items()})
    C.g = c3d(C.dz, C.w)
    C.pre.update({"g_" + k: v for k, v in _check_stored(C.g, regime, "g").items()})
    return _bnb_finish(C, C.g[..., c0:c1], rng, regime, parity=par)


@functools.lru_cache(maxsize=2)
def dgrad_bn_pooled(cin, cout, H, W, regime, n=N):
    """cnnitmo_conv3x3_dgrad_bn_pooled: the skip rows [0, cin) of a concat consumer's flipped weights
    (cin + 64 input channels), plus the pooled gradient dyp routed by the window index bytes."""
    rng = _rng("dgrad_bn_pooled", cin, cout, H, W, regime)
    cl = cin + 64
    C = NS(cin=cin, cout=cout, H=H, W=W, n=n, cl=cl, regime=regime, pre={})
    C.dz, C.w, p = _gemm_operands(rng, "c3d", regime, (n, H, W, cout), cl, cout, cap=236)
    C.pre.update({"dgrad_" + k: v for k, v in p.items()})
    C.g = c3d(C.dz, C.w)[..., :cin]
    C.dyp = _ints(rng, (n, H // 2, W // 2, cin), 60 if regime == "wide" else 4, 0.1)
    C.idx = rng.integers(0, 4, (n, H // 2, W // 2, cin)).astype(np.uint8)
    C.routed = R.maxpool2x2_bwd(C.dyp, C.idx, (n, H, W, cin))
    return _bnb_finish(C, C.g, rng, regime, routed=C.routed)


@functools.lru_cache(maxsize=2)
def tconv_dgrad_bn(cin, cout, H, W, regime, n=N):
    """cnnitmo_tconv2x2_dgrad_bn (bf16): g = the tconv input gradient of dout through k."""
    rng = _rng("tconv_dgrad_bn", cin, cout, H, W, regime)
    C = NS(cin=cin, cout=cout, H=H, W=W, n=n, regime=regime, pre={})
    C.dout, C.k, p = _gemm_operands(rng, "td", regime, (n, 2 * H, 2 * W, cout), cin, cout, cap=244)
    C.pre.update({"dgrad_" + k: v for k, v in p.items()})
    C.g = td(C.dout, C.k)
    return _bnb_finish(C, C.g, rng, regime)


@functools.lru_cache(maxsize=2)
def first_layer(n, hv, H, W, regime):
    """The 3-channel first layer: x [n, hv, W, 3] fp32 (rows >= hv read as zero), w [32,3,3,3], K = 27."""
    rng = _rng("first_layer", n, hv, H, W, regime)
    C = NS(n=n, hv=hv, H=H, W=W, regime=regime, pre={})
    amax, wmax = (3, 2) if regime == "small" else (255, 7)
    C.x = _ints(rng, (n, hv, W, 3), amax, 0.1, True)
    C.w = _ints(rng, (32, 3, 3, 3), wmax, 0.1)
    C.b = _dense(rng, 32, 3)
    C.xp = np.zeros((n, H, W, 3))
    C.xp[:, :hv] = C.x
    tot, frac = _products(c3, C.xp[:, :hv], C.w)  # rows >= hv have no nonzero product by construction
    C.pre.update(fwd_sum_abs=tot, fwd_min_frac=frac)
    C.z = c3(C.xp, C.w) + C.b
    C.out = np.maximum(C.z, 0)
    C.pre.update({"fwd_" + k: v for k, v in _check_stored(C.out, regime, "first layer").items()})
    if regime == "small":
        assert tot + 3 <= 256 and frac >= 1.0 / 8
        C.stats = _check_stats(C.out, "first layer")
    else:
        assert tot < LIM24
    C.dz = _ints(rng, (n, H, W, 32), 3 if regime == "small" else 15, 0.1)
    C.dw = R.conv2d_same_bwd(C.xp, C.w, C.dz, need_dx=False)[1]
    assert _c3_dw(np.abs(C.xp).astype(F32), np.abs(C.dz).astype(F32)).max() < LIM24
    cols = np.zeros((n, H, W, 32))
    xq = np.pad(C.xp, ((0, 0), (1, 1), (1, 1), (0, 0)))
    for r in range(3):
        for s in range(3):
            cols[..., (r * 3 + s) * 3:(r * 3 + s) * 3 + 3] = xq[:, r:r + H, s:s + W]
    C.cols = cols
    return C


def pool_first(y, sign=None):
    """The 2x2 pooling of a conv epilogue on the STORED output y [n,h,w,c] (launch_check_elem.py,
    _chk_pool_of_stored; test_maxpool_ties and oracle.maxpool2x2 for the plain maximum): per channel
    the first maximum of sign(pool_sign) * y in window order (0,0), (0,1), (1,0), (1,1); without a
    sign the maximum of y; sign 0: the first element.  Returns (value stored there, window index)."""
    n, h, w, c = y.shape
    ho, wo = h // 2, w // 2
    win = y[:, :2 * ho, :2 * wo].reshape(n, ho, 2, wo, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, ho, wo, 4, c)
    key = win * (1.0 if sign is None else np.sign(sign))
    first = np.argmax(key == key.max(3, keepdims=True), axis=3)
    return np.take_along_axis(win, first[:, :, :, None, :], 3)[:, :, :, 0], first.astype(np.uint8)


# ---- the case lists the GPU file runs, and the kernels they launch -------------------------------
FIRST_LAYER = [(2, 13, 16, 10), (1, 6, 7, 300), (3, 9, 9, 256), (2, 5, 6, 517)]  # test_first_layer_direct's (N, Hv, H, W)
FIRST_LAYER_LD = {(2, 13, 16, 10): (32, 0), (1, 6, 7, 300): (96, 64), (3, 9, 9, 256): (32, 0), (2, 5, 6, 517): (32, 0)}
POOL = [(32, 32, 16, 64), (64, 64, 18, 70), (128, 128, 8, 96), (64, 64, 6, 34)]  # test_conv3x3_fwd_pool's
CAT = [(16, 64), (20, 70), (8, 40)]  # test_conv3x3_fwd_cat_dec9's (H, W): [32 | 64] -> 64, bf16


def launched(q, halo0=False):
    """{kernel name: the exact case that launches it}: the same name queries as kernel_cases.tested,
    over the lists tests/test_gpu_exact.py (and with halo0 tests/halo0_child.py) parametrise over."""
    out = {}

    def triples(label, cases, namer, prefix="", n=N):
        for sh, exp in cases.items():
            for dt in ("bf16", "f32"):
                for what, nm, e in zip(("fwd", "dgrad", "wgrad"), namer(q, dt, *sh, n), exp[dt]):
                    if e is not None and (not prefix or what != "wgrad"):
                        out.setdefault(prefix + nm, f"{label} {sh} {dt} {what}")

    if halo0:
        triples("CONV3X3_HALO0", KC.CONV3X3_HALO0, KC.conv3x3_names, KC.HALO0)
        for (dt, h, w, cin, cout) in KC.AFFINE_HALO0:
            out.setdefault(KC.HALO0 + KC.conv3x3_names(q, dt, cin, cout, h, w, 1)[0], f"AFFINE_HALO0 {(dt, h, w, cin, cout)}")
        return out
    triples("CONV3X3_OPS", KC.CONV3X3_OPS, KC.conv3x3_names)
    triples("CONV3X3_FOLD", KC.CONV3X3_FOLD, KC.conv3x3_names)
    for label in ("TCONV_OPS", "TCONV_FOLD", "TCONV_AFFINE"):
        triples(label, getattr(KC, label), KC.tconv_names)
    for (cin, cout, h, w, c0, c1, _par) in KC.DGRAD_BN:
        for dt in ("bf16", "f32"):
            out.setdefault(KC.dgrad_bn_name(q, dt, cin, cout, h, w, c0, c1), f"DGRAD_BN {(cin, cout, h, w, c0, c1)} {dt}")
    for sh in KC.DGRAD_BN_POOLED:
        for dt in ("bf16", "f32"):
            out.setdefault(KC.dgrad_bn_pooled_name(q, dt, *sh), f"DGRAD_BN_POOLED {sh} {dt}")
    for sh in KC.TCONV_DGRAD_BN:
        out.setdefault(KC.tconv_dgrad_bn_name(q, "bf16", *sh), f"TCONV_DGRAD_BN {sh} bf16")
    return out
