"""Host side of the highlight-weighted training loss: the numpy reference (tests/hlweight_ref.py)
against central differences, gain 0 and hand-worked values, the C ABI's size query and argument
checks without a GPU, the HighlightWeighted class and its round trip through the saved training
config."""
import json

import numpy as np
import pytest

import cnn_itmo_amd as C
from cnn_itmo_amd import hdf5, losses
import hlweight_ref as HR

CASES = [(b, s) for b in ("mse", "mae") for s in ("input", "target")]
IDS = [f"{b}-{s}" for b, s in CASES]


def _tiny():
    C.clear_session()
    return C.TinyNet(seed=3)


# ---------------------------------------------------------------- reference
def _fd_case(source):
    """A float64 (3,5,7) case: a ramp and clipped pixels in every image.  No |y - t| inside
    (0, 1e-3] (some exactly 0); with source 'target' no pixel has m == tau."""
    rng = np.random.default_rng(17)
    t = rng.uniform(0.0, 1.0, (3, 5, 7, 3))
    t[:, ::2, ::3, 1] = rng.uniform(0.8, 1.0, t[:, ::2, ::3, 1].shape)
    t[:, 1, 1] = 1.0
    d = rng.uniform(0.01, 0.2, t.shape) * rng.choice([-1.0, 1.0], t.shape)
    d.reshape(-1)[::11] = 0.0
    y = t + d
    if source == "target":
        return t, y, t
    s = rng.uniform(0.0, 1.0, t.shape)
    s[:, ::2, 1::3, 2] = rng.uniform(0.8, 1.0, s[:, ::2, 1::3, 2].shape)
    s[:, 2, 2] = 1.0
    s[:, 3, 3] = (0.75, 0.3, 0.2)  # m == tau
    return s, y, t


@pytest.mark.parametrize("base,source", CASES, ids=IDS)
def test_reference_gradient_matches_central_differences(base, source):
    """Every element of a float64 (3,5,7) case, e = 1e-6, against d(sum_i L_i / F)/dy with F = 3
    and F = 5: within 1e-6 of max|dy|.  Both base terms are at most quadratic in y away from
    y == t, so the central difference is exact there up to the rounding of L (<= 1) at
    2^-53 / 2e-6 = 6e-11, and max|dy| >= 1 / (5 * 105).  The MAE base leaves out the elements with
    y == t; with source 'target' no pixel has m == tau (the mask does not depend on y either way)."""
    tau, gain, e = 0.75, 3.0, 1e-6
    s, y, t = _fd_case(source)
    m = s.max(axis=-1)
    assert (m > tau).any() and (m < tau).any() and (m >= 1.0).any()
    if source == "target":
        assert not (m == tau).any()
    else:
        assert (m == tau).any()
    dist = np.abs(y - t)
    assert (dist == 0).any() and not ((dist > 0) & (dist <= 1e-3)).any()
    idx = np.arange(y.size) if base == "mse" else np.flatnonzero(dist.reshape(-1) > 0)
    for frames in (None, 5.0):
        f = 3.0 if frames is None else frames
        dy = HR.loss_grad(s, y, t, base, tau, gain, frames)[1]
        fd = np.empty(idx.size)
        for k, i in enumerate(idx):
            yp, ym = y.copy(), y.copy()
            yp.flat[i] += e
            ym.flat[i] -= e
            sp = t if source == "target" else s
            fd[k] = (HR.loss_grad(sp, yp, t, base, tau, gain)[0][:, 2].sum()
                     - HR.loss_grad(sp, ym, t, base, tau, gain)[0][:, 2].sum()) / f / (2 * e)
        err = np.abs(fd - dy.reshape(-1)[idx]).max() / np.abs(dy).max()
        print(f"{base}/{source} frames {frames}: central-difference error {err:.2e} of max|dy|")
        assert err <= 1e-6, err
    if base == "mae":  # sign(0) = 0
        assert (HR.loss_grad(s, y, t, base, tau, gain)[1][dist == 0] == 0).all()


@pytest.mark.parametrize("base", ["mse", "mae"])
def test_gain_zero_is_the_base_loss(base):
    s, y, t = (v.astype(np.float64) for v in HR.make_case((2, 5, 7), 0.75, 3))
    out, dy = HR.loss_grad(s, y, t, base, 0.75, 0.0)
    assert np.array_equal(out[:, 2], out[:, 1]) and (out[:, 0] > 0).all()
    d = y - t
    want = (d * d if base == "mse" else np.abs(d)).mean(axis=(1, 2, 3))
    assert np.abs(out[:, 1] - want).max() <= 1e-15
    plain = (2.0 * d if base == "mse" else np.sign(d)) / (2.0 * 5 * 7 * 3)
    assert np.array_equal(dy, plain)
    out4, dy4 = HR.loss_grad(s, y, t, base, 0.75, 2.0, frames=4)
    assert np.array_equal(dy4, 0.5 * HR.loss_grad(s, y, t, base, 0.75, 2.0)[1])
    assert (out4[:, 2] > out4[:, 1]).all()


def test_hand_worked_two_pixel_image():
    """tau 0.5, gain 2.  Pixel 0: m = 0.75, a = 0.5, wgt = 2; pixel 1: m == tau, a = 0, wgt = 1.
    y - t = (0.25, 0, 0.5) and (-0.5, 0, 0.25): every value below is a dyadic fraction or a
    quotient by 6 of one."""
    s = np.array([[[0.2, 0.75, 0.1], [0.5, 0.1, 0.3]]])
    y = np.array([[[0.5, 0.25, 1.0], [0.0, 0.5, 0.5]]])
    t = np.array([[[0.25, 0.25, 0.5], [0.5, 0.5, 0.25]]])
    out, dy = HR.loss_grad(s, y, t, "mse", 0.5, 2.0)
    assert out.shape == (1, 4) and dy.shape == (1, 1, 2, 3)
    assert np.array_equal(out[0], [0.25, 0.625 / 6, 0.9375 / 6, 0.15625 / 1.5])
    assert np.array_equal(dy[0, 0], [[1.0 / 6, 0.0, 2.0 / 6], [-1.0 / 6, 0.0, 0.5 / 6]])
    out, dy = HR.loss_grad(s, y, t, "mae", 0.5, 2.0)
    assert np.array_equal(out[0], [0.25, 0.25, 0.375, 0.25])
    assert np.array_equal(dy[0, 0], [[2.0 / 6, 0.0, 2.0 / 6], [-1.0 / 6, 0.0, 1.0 / 6]])
    # no masked pixel: A = H = 0 exactly, L == B; a NaN source counts as unmasked
    for dark in (np.full_like(s, 0.5), np.full_like(s, np.nan)):
        out, _ = HR.loss_grad(dark, y, t, "mae", 0.5, 2.0)
        assert np.array_equal(out[0], [0.0, 0.25, 0.25, 0.0])
    # (s, y, t above are [h,w,3], a batch of one) the same as [n,h,w,3], twice
    s2, y2, t2 = (np.stack([v, v]) for v in (s, y, t))
    out, dy = HR.loss_grad(s2, y2, t2, "mae", 0.5, 2.0)
    assert np.array_equal(out, [[0.25, 0.25, 0.375, 0.25]] * 2)
    assert np.array_equal(dy[1, 0], [[1.0 / 6, 0.0, 1.0 / 6], [-0.5 / 6, 0.0, 0.5 / 6]])  # F = 2
    with pytest.raises(ValueError):
        HR.loss_grad(s, y, t, None, 0.5, 2.0)


# ---------------------------------------------------------------- C ABI (no GPU)
def test_workspace_bytes_without_gpu():
    from cnn_itmo_amd import _lib, ops
    for name in ("cnnitmo_highlight_workspace_bytes", "cnnitmo_highlight_loss_grad"):
        assert name in _lib.SIGNATURES
    q = ops.highlight_workspace_bytes
    # four fp64 sums per workgroup of 1024 pixels, workgroups never straddle images
    assert q(1, 1, 1) == 32 and q(2, 1, 1024) == 64 and q(2, 1, 1025) == 128 and q(1, 3, 683) == 3 * 32
    assert q(32, 1080, 1920) == 32 * 2025 * 32
    for bad in ((0, 64, 64), (1, 0, 64), (1, 64, 0), (-1, 64, 64), (1, -3, 5), (65536, 4, 4)):
        assert q(*bad) <= 0, bad


def test_bad_arguments_are_einval_before_any_launch():
    """Every refusal of the entry point comes from the argument checks, which run before any
    device call (no GPU here)."""
    from cnn_itmo_amd import _lib
    lib = _lib.load()
    nan, inf = float("nan"), float("inf")
    ok = dict(base=2, tau=0.95, gain=1.0, s=16, y=16, t=16, n=1, h=16, w=16, frames=0.0, out=16, dy=None, ws=16,
              nb=1 << 20)
    for change, msg in [(dict(s=None), b"null"), (dict(y=None), b"null"), (dict(t=None), b"null"),
                        (dict(out=None), b"null"), (dict(ws=None), b"null"),
                        (dict(n=0), b"shape"), (dict(h=0), b"shape"), (dict(w=-1), b"shape"),
                        (dict(n=65536), b"too large"),
                        (dict(tau=1.0), b"tau"), (dict(tau=-0.01), b"tau"), (dict(tau=nan), b"tau"),
                        (dict(gain=-1.0), b"gain"), (dict(gain=inf), b"gain"), (dict(gain=nan), b"gain"),
                        (dict(base=_lib.DSSIM_BASES[None]), b"base"), (dict(base=3), b"base"), (dict(base=-1), b"base"),
                        (dict(nb=24), b"workspace too small"), (dict(ws=20), b"8-byte"),
                        (dict(dy=18), b"4-byte"), (dict(s=18), b"4-byte")]:
        a = dict(ok, **change)
        rc = lib.cnnitmo_highlight_loss_grad(a["base"], a["tau"], a["gain"], a["s"], a["y"], a["t"], a["n"], a["h"],
                                             a["w"], a["frames"], a["out"], a["dy"], a["ws"], a["nb"], None)
        assert rc < 0 and msg in lib.cnnitmo_last_error(), (change, lib.cnnitmo_last_error())


# ---------------------------------------------------------------- front end
def test_class_validation():
    hw = C.HighlightWeighted()
    assert (hw.base, hw.threshold, hw.gain, hw.source) == ("mse", 0.95, 1.0, "input")
    assert losses.HighlightWeighted is C.HighlightWeighted and "HighlightWeighted" in C.__all__
    assert "starting point" in C.HighlightWeighted.__doc__  # gain = 1.0 is not a tuned value
    assert hw.get_config() == {"base": "mse", "threshold": 0.95, "gain": 1.0, "source": "input"}
    assert hw == C.HighlightWeighted("mse", 0.95, 1, "input") and hash(hw) == hash(C.HighlightWeighted())
    assert hw != C.HighlightWeighted(gain=2.0) and hw != C.HighlightWeighted(source="target") and hw != "mse"
    assert hw != C.DSSIM("mse") and eval(repr(hw), {"HighlightWeighted": C.HighlightWeighted}) == hw
    assert C.HighlightWeighted("mae", 0.0, 0.0).base_id == 1 and hw.base_id == 2
    for kw in (dict(base=None), dict(base="MSE"), dict(base="logcosh"), dict(threshold=1.0), dict(threshold=-0.1),
               dict(threshold=float("nan")), dict(threshold="high"), dict(gain=-1.0), dict(gain=float("inf")),
               dict(gain=float("nan")), dict(gain=None), dict(source="output"), dict(source=None)):
        with pytest.raises(ValueError):
            C.HighlightWeighted(**kw)


def test_serialize_get_round_trip_and_compile():
    hw = C.HighlightWeighted("mae", 0.1 + 0.2, 4.0, "target")
    d = losses.serialize(hw)
    assert d == {"class_name": "HighlightWeighted",
                 "config": {"base": "mae", "threshold": 0.1 + 0.2, "gain": 4.0, "source": "target"}}
    back = losses.get(json.loads(json.dumps(d)))
    assert back == hw and back.threshold == 0.1 + 0.2 and losses.get(hw) is hw
    with pytest.raises(ValueError):
        losses.get({"class_name": "HighlightWeighted", "config": {"gain": -2.0}})
    assert losses.get({"class_name": "HighlightWeighted"}) == C.HighlightWeighted()
    assert losses.get("highlight") is None and losses.serialize("mae") == "mae"
    m = _tiny()
    m.compile("adam", hw, ["accuracy"])
    assert m.loss is hw and m.metrics_names == ["loss", "acc"]
    before = (m.optimizer, m.loss)
    with pytest.raises(ValueError):
        m.compile("adam", {"class_name": "HighlightWeighted", "config": {"threshold": 1.5}})
    with pytest.raises(NotImplementedError):
        m.compile("adam", "highlight_weighted")
    assert (m.optimizer, m.loss) == before
    m.compile("adam", "mse")
    assert m.loss == "mse"


@pytest.mark.parametrize("ext", ["h5", "npz"])
def test_training_config_round_trip(tmp_path, ext):
    """base, threshold, gain and source survive save / load_model exactly (0.1 + 0.2 is not 0.3)."""
    m = _tiny()
    hw = C.HighlightWeighted("mae", 0.1 + 0.2, 2.5, "target")
    m.compile(C.Adam(lr=2e-3), hw, ["accuracy", "psnr"])
    p = str(tmp_path / f"m.{ext}")
    m.save(p)
    if ext == "h5":
        tc = json.loads(bytes(hdf5.File(p).attrs["training_config"]).decode())
        assert tc["loss"] == {"class_name": "HighlightWeighted", "config": hw.get_config()}
    C.clear_session()
    m2 = C.load_model(p)
    assert isinstance(m2.loss, C.HighlightWeighted) and m2.loss == hw and m2.loss.threshold == 0.1 + 0.2
    assert m2.metrics_names == ["loss", "acc", "psnr"] and type(m2.optimizer) is C.Adam
