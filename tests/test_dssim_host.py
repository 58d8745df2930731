"""Host side of the DSSIM training loss: the numpy reference's gradient against central
differences (tests/dssim_ref.py), the C ABI's size query and argument checks without a GPU,
compile()'s DSSIM forms and their round trip through the saved training config."""
import json

import numpy as np
import pytest

import cnn_itmo_amd as C
from cnn_itmo_amd import hdf5
import dssim_ref as DR
import metrics_ref as MR

CASES = [(None, 1.0), ("mae", 0.84), ("mse", 0.84)]
IDS = ["none", "mae", "mse"]


def _tiny():
    C.clear_session()
    return C.TinyNet(seed=3)


# ---------------------------------------------------------------- reference
def _central(y, t, base, alpha, idx, e=1e-6):
    out = np.empty(len(idx))
    for k, i in enumerate(idx):
        yp, ym = y.copy(), y.copy()
        yp.flat[i] += e
        ym.flat[i] -= e
        out[k] = (DR.loss(yp, t, base, alpha)[2].mean() - DR.loss(ym, t, base, alpha)[2].mean()) / (2 * e)
    return out


@pytest.mark.parametrize("base,alpha", CASES, ids=IDS)
def test_reference_gradient_matches_central_differences(base, alpha):
    """Every element of a (1,13,14) pair and 40 sampled elements of a (1,27,29) pair, e = 1e-6:
    within 1e-6 of max|dy| (observed 2e-8).  For 'mae' no |y - t| lies inside (0, e], an input
    condition (at y == t both the central difference of |.| and sign(0) are 0)."""
    for shape, seed, sample in (((1, 13, 14), 3, None), ((1, 27, 29), 4, 40)):
        p, t = MR.make_pair(shape, seed)
        y, t = p.astype(np.float64), t.astype(np.float64)
        if base == "mae":
            d = np.abs(y - t)
            assert not ((d > 0) & (d <= 2e-6)).any()
        dy = DR.loss_grad(y, t, base, alpha)[3]
        idx = np.arange(y.size) if sample is None else np.random.default_rng(seed).choice(y.size, sample, False)
        fd = _central(y, t, base, alpha, idx)
        err = np.abs(fd - dy.reshape(-1)[idx]).max() / np.abs(dy).max()
        print(f"{shape} base {base}: central-difference error {err:.2e} of max|dy|")
        assert err <= 1e-6, err


def test_reference_loss_grad_agrees_with_loss_and_scales_with_frames():
    p, t = MR.make_pair((2, 13, 14), 5)
    for base, alpha in CASES:
        ssim, b, l, dy = DR.loss_grad(p, t, base, alpha)
        s2, b2, l2 = DR.loss(p, t, base, alpha)
        assert np.abs(ssim - MR.ssim(p, t)).max() < 1e-14 and np.abs(ssim - s2).max() < 1e-14
        assert np.array_equal(b, b2) and np.abs(l - l2).max() < 1e-14
        assert np.array_equal(DR.loss_grad(p, t, base, alpha, grad_frames=4)[3], 0.5 * dy)
    assert np.array_equal(DR.loss(p, t, None, 0.3)[2], 1.0 - MR.ssim(p, t))  # no base: alpha is 1


# ---------------------------------------------------------------- C ABI (no GPU)
def test_workspace_bytes_without_gpu():
    from cnn_itmo_amd import _lib, ops
    for name in ("cnnitmo_dssim_workspace_bytes", "cnnitmo_dssim_loss_grad", "cnnitmo_head_fwd_bwd_given"):
        assert name in _lib.SIGNATURES
    q = ops.dssim_workspace_bytes
    assert q(1, 11, 11, 0) > 0 and q(1, 11, 11, 1) == q(1, 11, 11, 0) + 3 * 3 * 8  # one map element per channel
    assert q(8, 1080, 1920, 1) - q(8, 1080, 1920, 0) == 8 * 3 * 1070 * 1910 * 3 * 8  # fp64 planes
    assert q(3, 64, 64, 1) == 3 * q(1, 64, 64, 1) and q(3, 64, 64, 0) == 3 * q(1, 64, 64, 0)
    for bad in ((0, 64, 64), (1, 10, 64), (1, 64, 10), (-1, 64, 64), (1, 0, 0)):
        assert q(*bad, 0) <= 0 and q(*bad, 1) <= 0, bad


def test_bad_arguments_are_einval_before_any_launch():
    """Null pointers, a small frame, an unknown base, alpha outside [0, 1]: refused by the
    argument checks, which come before any device call (no GPU here)."""
    from cnn_itmo_amd import _lib
    lib = _lib.load()
    ok = dict(base=0, alpha=1.0, y=16, t=16, n=1, h=16, w=16, frames=0.0, out=16, dy=None, ws=16, nb=1 << 20)
    for change, msg in [(dict(y=None), b"null"), (dict(t=None), b"null"), (dict(out=None), b"null"),
                        (dict(ws=None), b"null"), (dict(h=10), b"10 x 16"), (dict(w=10), b"16 x 10"),
                        (dict(base=3), b"base"), (dict(base=1, alpha=1.5), b"alpha"), (dict(alpha=0.5), b"alpha"),
                        (dict(nb=8), b"workspace too small"), (dict(n=0), b"shape")]:
        a = dict(ok, **change)
        rc = lib.cnnitmo_dssim_loss_grad(a["base"], a["alpha"], a["y"], a["t"], a["n"], a["h"], a["w"], a["frames"],
                                         a["out"], a["dy"], a["ws"], a["nb"], None)
        assert rc < 0 and msg in lib.cnnitmo_last_error(), (change, lib.cnnitmo_last_error())
    rc = lib.cnnitmo_head_fwd_bwd_given(0, 16, 1, 4, 4, 4, 64, 16, 16, None, None, 16, None, 16, None, 16, None)
    assert rc < 0 and b"null dy" in lib.cnnitmo_last_error()
    rc = lib.cnnitmo_head_fwd_bwd_given(0, 16, 1, 4, 4, 4, 64, 16, 16, None, None, 16, 16, 16, 16, 16, None)
    assert rc < 0 and b"exactly one" in lib.cnnitmo_last_error()
    # the given-gradient head has its own entry point: the per-element call refuses its id
    assert _lib.LOSS_GIVEN == 5 and _lib.DSSIM_BASES == DR.BASE_IDS
    rc = lib.cnnitmo_head_fwd_bwd_loss(_lib.LOSS_GIVEN, 0, 16, 1, 4, 4, 4, 64, 16, 16, None, None, 16, 16, None, 16,
                                       0.0, None)
    assert rc < 0 and b"unknown loss" in lib.cnnitmo_last_error()


# ---------------------------------------------------------------- front end
def test_compile_accepts_the_dssim_forms():
    m = _tiny()
    m.compile("adam", "dssim", ["accuracy"])
    assert isinstance(m.loss, C.DSSIM) and m.loss == C.DSSIM() and (m.loss.base, m.loss.alpha) == (None, 1.0)
    assert m.metrics_names == ["loss", "acc"]
    m.compile("adam", C.DSSIM("mae"))
    assert (m.loss.base, m.loss.alpha) == ("mae", 0.84)
    m.compile("adam", C.DSSIM(base="mse", alpha=0.5))
    assert (m.loss.base, m.loss.alpha) == ("mse", 0.5) and m.loss != C.DSSIM("mse")
    assert C.DSSIM(None, alpha=0.3).alpha == 1.0  # no base: the loss is 1 - SSIM
    m.compile("adam", "mae")
    assert m.loss == "mae"


def test_bad_dssim_arguments_are_rejected():
    for kw in (dict(base="huber"), dict(base="MAE"), dict(base="mae", alpha=-0.1), dict(base="mse", alpha=1.01),
               dict(base="mse", alpha=float("nan"))):
        with pytest.raises(ValueError):
            C.DSSIM(**kw)
    m = _tiny()
    m.compile("adam", C.DSSIM("mae", 0.7), ["accuracy", "ssim"])
    before = (m.optimizer, m.loss, list(m.metrics_names))
    for bad in ("ssim", "ms_ssim", {"class_name": "MSSSIM", "config": {}}):
        with pytest.raises(NotImplementedError):
            m.compile("adam", bad)
    with pytest.raises(ValueError):
        m.compile("adam", {"class_name": "DSSIM", "config": {"base": "mae", "alpha": 2.0}})
    assert (m.optimizer, m.loss, m.metrics_names) == before


@pytest.mark.parametrize("ext", ["h5", "npz"])
@pytest.mark.parametrize("loss", ["dssim", C.DSSIM("mae"), C.DSSIM("mse", 0.1 + 0.2)], ids=["dssim", "mae", "mse"])
def test_training_config_round_trip(tmp_path, loss, ext):
    """The choice and alpha survive save / load_model exactly (0.1 + 0.2 is not 0.3)."""
    m = _tiny()
    m.compile(C.Adam(lr=2e-3), loss, ["accuracy", "ssim"])
    p = str(tmp_path / f"m.{ext}")
    m.save(p)
    if ext == "h5":
        tc = json.loads(bytes(hdf5.File(p).attrs["training_config"]).decode())
        assert tc["loss"] == {"class_name": "DSSIM", "config": {"base": m.loss.base, "alpha": m.loss.alpha}}
    C.clear_session()
    m2 = C.load_model(p)
    assert isinstance(m2.loss, C.DSSIM) and m2.loss == m.loss and m2.loss.alpha == m.loss.alpha
    assert m2.metrics_names == ["loss", "acc", "ssim"] and type(m2.optimizer) is C.Adam
