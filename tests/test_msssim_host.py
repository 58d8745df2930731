"""Host side of multi-scale SSIM: the numpy reference (tests/msssim_ref.py) against central
differences and its closed forms, the C ABI's size query and argument checks without a GPU, the
MSSSIM loss object and its round trip through the saved training config, the metric key and the
command lines' flags."""
import json

import numpy as np
import pytest

import cnn_itmo_amd as C
from cnn_itmo_amd import hdf5, losses
import dssim_ref as DR
import metrics_ref as MR
import msssim_ref as MS

CASES = [(None, 1.0), ("mae", 0.84), ("mse", 0.84)]
IDS = ["none", "mae", "mse"]
W3 = MS.WEIGHTS[:3]


def _tiny():
    C.clear_session()
    return C.TinyNet(seed=3)


# ---------------------------------------------------------------- reference
def _central(y, t, base, alpha, w, idx, e=1e-6):
    out = np.empty(len(idx))
    for k, i in enumerate(idx):
        yp, ym = y.copy(), y.copy()
        yp.flat[i] += e
        ym.flat[i] -= e
        out[k] = (MS.loss(yp, t, base, alpha, w)[2].mean() - MS.loss(ym, t, base, alpha, w)[2].mean()) / (2 * e)
    return out


@pytest.mark.parametrize("base,alpha", CASES, ids=IDS)
def test_reference_gradient_matches_central_differences(base, alpha):
    """Three scales on (1,45,43) (odd at levels 0 and 1 both ways: 45 -> 23 -> 12, 43 -> 22 -> 11)
    and two on (2,24,21): 40 sampled elements plus the last row, the last column and the corner,
    which take the folded pad's double share; e = 1e-6, within 1e-6 of max|dy| (dssim_host's bound;
    observed 1.0e-7).  For 'mae' no |y - t| lies inside (0, 2e]."""
    for shape, seed, w in (((1, 45, 43), 2, W3), ((2, 24, 21), 3, MS.WEIGHTS[:2])):
        p, t = MS.blocky_pair(shape, seed, 0.1)
        y, t = p.astype(np.float64), t.astype(np.float64)
        if base == "mae":
            d = np.abs(y - t)
            assert not ((d > 0) & (d <= 2e-6)).any()
        assert MS.factors(y, t, w).min() >= 0.1  # away from the clamp
        dy = MS.loss_grad(y, t, base, alpha, w)[4]
        n, h, ww = shape
        idx = np.random.default_rng(seed).choice(y.size, 40, False)
        edge = [y.size - 1, y.size - 3 * ww - 2, 3 * ww * (h - 1) + 4, 3 * (ww - 1) + 3 * ww * 5 + 1]
        idx = np.concatenate([idx, edge])
        fd = _central(y, t, base, alpha, w, idx)
        err = np.abs(fd - dy.reshape(-1)[idx]).max() / np.abs(dy).max()
        print(f"{shape} base {base}: central-difference error {err:.2e} of max|dy|")
        assert err <= 1e-6, err


def test_pool_and_its_adjoint():
    """Odd sides repeat the last row / column; <pool(x), g> = <x, pool_adjoint(g)>."""
    rng = np.random.default_rng(0)
    x = rng.uniform(size=(2, 5, 7, 3))
    p = MS.pool(x)
    assert p.shape == (2, 3, 4, 3)
    assert np.allclose(p[:, 0, 0], x[:, :2, :2].mean(axis=(1, 2)))
    assert np.allclose(p[:, 2, 3], x[:, 4, 6])  # the corner: four copies of one pixel
    assert np.allclose(p[:, 2, 0], x[:, 4, :2].mean(axis=1))
    g = rng.normal(size=p.shape)
    assert abs((p * g).sum() - (x * MS.pool_adjoint(g, 5, 7)).sum()) < 1e-12
    x = rng.uniform(size=(1, 4, 6, 3))
    g = rng.normal(size=(1, 2, 3, 3))
    assert abs((MS.pool(x) * g).sum() - (x * MS.pool_adjoint(g, 4, 6)).sum()) < 1e-12


def test_closed_forms():
    p, t = MS.blocky_pair((2, 45, 43), 5, 0.1)
    # identical images: every factor is 1
    assert np.array_equal(MS.factors(t, t, W3), np.ones((2, 3, 3)))
    assert np.abs(MS.ms_ssim(t, t, power_factors=W3) - 1.0).max() <= 1e-15
    # one scale of weight 1: the mean over channels of the per-channel SSIM
    per_channel = MR.ssim_map(p, t).mean(axis=(1, 2))
    assert np.abs(MS.ms_ssim(p, t, power_factors=(1.0,)) - per_channel.mean(axis=1)).max() <= 1e-15
    assert np.abs(MS.ms_ssim(p, t, power_factors=(1.0,)) - MR.ssim(p, t)).max() <= 1e-15
    # max_val scales with the images (scaled in float64: 255 p is not exact in float32)
    p64, t64 = p.astype(np.float64), t.astype(np.float64)
    assert np.abs(MS.ms_ssim(p64 * 255.0, t64 * 255.0, 255.0, W3) - MS.ms_ssim(p, t, 1.0, W3)).max() <= 1e-12
    # the weights are used as given: the product over scales per channel, then the channel mean
    f = MS.factors(p, t, W3)
    want = np.prod(f ** np.asarray(W3)[None, :, None], axis=1).mean(axis=1)
    assert np.abs(MS.ms_ssim(p, t, power_factors=W3) - want).max() <= 1e-15
    # loss_grad agrees with loss; grad_frames scales exactly
    for base, alpha in CASES:
        ms, b, l, f2, dy = MS.loss_grad(p, t, base, alpha, W3)
        ms2, b2, l2 = MS.loss(p, t, base, alpha, W3)
        assert np.abs(ms - ms2).max() < 1e-14 and np.array_equal(b, b2) and np.abs(l - l2).max() < 1e-14
        assert np.array_equal(f2, f)
        assert np.array_equal(MS.loss_grad(p, t, base, alpha, W3, grad_frames=4)[4], 0.5 * dy)
    with pytest.raises(ValueError, match="40 x 43"):
        MS.ms_ssim(p[:, :40], t[:, :40], power_factors=W3)


def test_clamped_channel_has_zero_score_and_gradient():
    """y = 1 - t: every cs mean is negative, so MS_c = 0 and the gradient is exactly 0 (finite);
    with a base term the gradient is the base term's alone."""
    _, t = MS.blocky_pair((1, 45, 43), 6, 0.1)
    t = t.astype(np.float64)
    y = 1.0 - t
    f = MS.factors(y, t, W3)
    assert f.max() < -0.5
    ms, b, l, _, dy = MS.loss_grad(y, t, None, 1.0, W3)
    assert ms[0] == 0.0 and l[0] == 1.0 and np.isfinite(dy).all() and not dy.any()
    dy = MS.loss_grad(y, t, "mae", 0.84, W3)[4]
    assert np.array_equal(dy, (1.0 - 0.84) / y[0].size * np.sign(y - t))


# ---------------------------------------------------------------- C ABI (no GPU)
def _levels(h, w, m):
    out = [(h, w)]
    for _ in range(m - 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def _tiles(h, w):
    return -(-(h - 10) // 16) * -(-(3 * (w - 10)) // 48)


def test_workspace_bytes_without_gpu():
    """The query is exact: fp64 levels >= 1 of y and t, 4 sums per tile and level, 3 scalars per
    image and scale; with a gradient the planes of every level and the level gradients."""
    from cnn_itmo_amd import _lib, ops
    for name in ("cnnitmo_msssim_workspace_bytes", "cnnitmo_msssim_loss_grad"):
        assert name in _lib.SIGNATURES
    q = ops.msssim_workspace_bytes
    for n, h, w, m in ((1, 176, 176, 5), (2, 183, 205, 5), (3, 44, 44, 3), (1, 45, 84, 3), (2, 11, 30, 1)):
        lv = _levels(h, w, m)
        loss = sum(2 * 3 * a * b for a, b in lv[1:]) + sum(4 * _tiles(a, b) for a, b in lv) + 3 * m
        grad = sum(9 * (a - 10) * (b - 10) for a, b in lv) + sum(3 * a * b for a, b in lv[1:])
        assert q(n, h, w, m, 0) == 8 * n * loss, (n, h, w, m)
        assert q(n, h, w, m, 1) == 8 * n * (loss + grad), (n, h, w, m)
    per_pixel = q(32, 1080, 1920, 5, 1) / (32 * 1080 * 1920)
    assert 110 < per_pixel <= 120  # DSSIM: 72
    assert 16 < q(32, 1080, 1920, 5, 0) / (32 * 1080 * 1920) < 16.25  # the levels, and 32 B per 16 x 16 tile
    for bad in ((0, 176, 176, 5), (1, 160, 176, 5), (1, 176, 160, 5), (1, 40, 44, 3), (1, 176, 176, 0),
                (1, 176, 176, 6), (-1, 176, 176, 5), (1, 10, 10, 1)):
        assert q(*bad, 0) <= 0 and q(*bad, 1) <= 0, bad
    assert q(1, 161, 161, 5, 0) > 0 and q(1, 41, 41, 3, 1) > 0 and q(1, 11, 11, 1, 1) > 0
    assert [losses.min_side(m) for m in range(1, 6)] == [11, 21, 41, 81, 161] == [MS.min_side(m) for m in range(1, 6)]
    assert _lib.load().cnnitmo_version() == 2


def test_bad_arguments_are_einval_before_any_launch():
    """Every bad argument of the ABI is refused by the argument checks, which come before any
    device call (no GPU here)."""
    import ctypes
    from cnn_itmo_amd import _lib
    lib = _lib.load()

    def run(**ch):
        a = dict(dict(base=0, alpha=1.0, pf=MS.WEIGHTS, m=None, max_val=1.0, y=16, t=16, n=1, h=176, w=176,
                      frames=0.0, out=16, dy=None, ws=16, nb=1 << 30), **ch)
        m = len(a["pf"]) if a["m"] is None else a["m"]
        pf = (ctypes.c_double * max(len(a["pf"]), 1))(*a["pf"])
        rc = lib.cnnitmo_msssim_loss_grad(a["base"], a["alpha"], None if a.get("nopf") else ctypes.addressof(pf), m,
                                          a["max_val"], a["y"], a["t"], a["n"], a["h"], a["w"], a["frames"], a["out"],
                                          a["dy"], a["ws"], a["nb"], None)
        return rc, lib.cnnitmo_last_error()

    inf, nan = float("inf"), float("nan")
    for change, msg in [(dict(y=None), b"null"), (dict(t=None), b"null"), (dict(out=None), b"null"),
                        (dict(ws=None), b"null"), (dict(nopf=True), b"null"),
                        (dict(base=3), b"base"), (dict(base=-1), b"base"), (dict(base=1, alpha=1.5), b"alpha"),
                        (dict(base=1, alpha=-0.1), b"alpha"), (dict(base=1, alpha=nan), b"alpha"),
                        (dict(alpha=0.5), b"without a base"),
                        (dict(m=0), b"scales"), (dict(m=6), b"scales"),
                        (dict(pf=(0.1, -0.2, 0.3)), b"power factor 1"), (dict(pf=(0.1, 0.2, inf)), b"power factor 2"),
                        (dict(pf=(nan,)), b"power factor 0"),
                        (dict(max_val=0.0), b"max_val"), (dict(max_val=-1.0), b"max_val"), (dict(max_val=nan), b"max_val"),
                        (dict(h=160), b"160 x 176"), (dict(w=160), b"176 x 160"), (dict(pf=W3, h=40, w=44), b"40 x 44"),
                        (dict(n=0), b"shape"), (dict(nb=8), b"workspace too small"), (dict(ws=20), b"aligned")]:
        rc, err = run(**change)
        assert rc < 0 and msg in err, (change, err)


# ---------------------------------------------------------------- front end
def test_msssim_object():
    d = C.MSSSIM()
    assert (d.base, d.alpha, d.power_factors, d.min_side) == (None, 1.0, MS.WEIGHTS, 161)
    assert C.MSSSIM(None, alpha=0.3).alpha == 1.0  # no base: the loss is 1 - MS-SSIM
    d = C.MSSSIM("mae")
    assert (d.base, d.alpha, d.base_id) == ("mae", 0.84, 1)
    d3 = C.MSSSIM("mse", 0.5, power_factors=[0.2, 0.3, 0.5])
    assert d3.power_factors == (0.2, 0.3, 0.5) and d3.min_side == 41
    assert d3.get_config() == {"base": "mse", "alpha": 0.5, "power_factors": [0.2, 0.3, 0.5]}
    assert C.MSSSIM(**d3.get_config()) == d3 and hash(C.MSSSIM(**d3.get_config())) == hash(d3)
    assert d3 != C.MSSSIM("mse", 0.5) and d3 != C.MSSSIM("mse", 0.6, (0.2, 0.3, 0.5)) and d3 != C.DSSIM("mse", 0.5)
    assert C.DSSIM("mse", 0.5) != d3 and len({d3, C.MSSSIM("mse", 0.5, (0.2, 0.3, 0.5)), C.DSSIM("mse", 0.5)}) == 2
    assert repr(d3) == "MSSSIM(base='mse', alpha=0.5, power_factors=(0.2, 0.3, 0.5))"
    for kw in (dict(base="huber"), dict(base="mae", alpha=-0.1), dict(base="mse", alpha=1.01),
               dict(base="mse", alpha=float("nan")), dict(power_factors=()), dict(power_factors=(0.1,) * 6),
               dict(power_factors=(0.5, -0.1)), dict(power_factors=(0.5, float("inf"))),
               dict(power_factors=(float("nan"),)), dict(power_factors=3.0)):
        with pytest.raises(ValueError):
            C.MSSSIM(**kw)


def test_losses_get_and_serialize():
    assert losses.get("ms_ssim") == C.MSSSIM() == losses.get("msssim")
    d = C.MSSSIM("mae", 0.1 + 0.2, (0.25, 0.75))
    ser = losses.serialize(d)
    assert ser == {"class_name": "MSSSIM", "config": {"base": "mae", "alpha": 0.1 + 0.2, "power_factors": [0.25, 0.75]}}
    back = losses.get(json.loads(json.dumps(ser)))
    assert isinstance(back, C.MSSSIM) and back == d and back.alpha == d.alpha and losses.get(d) is d
    assert losses.get({"class_name": "MSSSIM", "config": {}}) == C.MSSSIM()
    with pytest.raises(ValueError):
        losses.get({"class_name": "MSSSIM", "config": {"base": "mae", "alpha": 2.0}})
    # the single-scale forms are what they were
    assert losses.get("dssim") == C.DSSIM() and losses.get("mae") is None and losses.serialize("mae") == "mae"
    assert losses.serialize(C.DSSIM("mae")) == {"class_name": "DSSIM", "config": {"base": "mae", "alpha": 0.84}}


def test_compile_takes_the_object_and_the_metric():
    from cnn_itmo_amd import metrics as M
    m = _tiny()
    m.compile("adam", C.MSSSIM("mae", power_factors=W3), ["accuracy", "ms_ssim"])
    assert isinstance(m.loss, C.MSSSIM) and m.loss == C.MSSSIM("mae", 0.84, W3)
    assert m.metrics_names == ["loss", "acc", "ms_ssim"] and m.image_metrics == ["ms_ssim"]
    m.compile("adam", "mse", [M.ms_ssim, "ssim", "accuracy", M.psnr, "ms_ssim"])
    assert m.loss == "mse" and m.metrics_names == ["loss", "ms_ssim", "ssim", "acc", "psnr"]
    assert m.image_metrics == ["ms_ssim", "ssim", "psnr"]
    from cnn_itmo_amd.callbacks import ModelCheckpoint
    assert ModelCheckpoint("x.npz", monitor="val_ms_ssim").mode == "max"


@pytest.mark.parametrize("ext", ["h5", "npz"])
@pytest.mark.parametrize("loss", [C.MSSSIM(), C.MSSSIM("mae", power_factors=W3), C.MSSSIM("mse", 0.1 + 0.2, (0.7, 0.1 + 0.2))],
                         ids=["default", "mae3", "mse2"])
def test_training_config_round_trip(tmp_path, loss, ext):
    """The choice, alpha and the weights survive save / load_model exactly (0.1 + 0.2 is not 0.3)."""
    m = _tiny()
    m.compile(C.Adam(lr=2e-3), loss, ["accuracy", "ms_ssim", "ssim"])
    p = str(tmp_path / f"m.{ext}")
    m.save(p)
    if ext == "h5":
        tc = json.loads(bytes(hdf5.File(p).attrs["training_config"]).decode())
        assert tc["loss"] == {"class_name": "MSSSIM", "config": {"base": loss.base, "alpha": loss.alpha,
                                                                "power_factors": list(loss.power_factors)}}
        assert tc["metrics"] == ["accuracy", "ms_ssim", "ssim"]
    C.clear_session()
    m2 = C.load_model(p)
    assert isinstance(m2.loss, C.MSSSIM) and m2.loss == loss and m2.loss.alpha == loss.alpha
    assert m2.loss.power_factors == loss.power_factors
    assert m2.metrics_names == ["loss", "acc", "ms_ssim", "ssim"] and type(m2.optimizer) is C.Adam


# ---------------------------------------------------------------- command lines
def test_cli_flags(tmp_path, capsys):
    """--ms-ssim is opt-in on both command lines; predict's needs --reference (checked before
    the model is read).  The CSV writers add the column only when asked."""
    from cnn_itmo_amd import evaluate_hdr as EH, predict as P
    with pytest.raises(SystemExit):
        P.main(["--model", "none.h5", "--ms-ssim"])
    assert "--ms-ssim needs --reference" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        EH.main(["--pred", str(tmp_path), "--reference", str(tmp_path), "--ms-ssim", "--anchor", "nope"])
    assert "anchor" in capsys.readouterr().err
    with pytest.raises(FileNotFoundError):  # the flag parses; the empty directory is what stops it
        EH.main(["--pred", str(tmp_path), "--reference", str(tmp_path), "--ms-ssim"])
    csv = tmp_path / "s.csv"
    EH.write_csv(str(csv), [("a.hdr", 30.0, 0.9, 2.0, 3.0)])
    assert csv.read_text().splitlines() == [EH.CSV_HEADER, "a.hdr;30;0.9;2;3"]
    EH.write_csv(str(csv), [("a.hdr", 30.0, 0.9, 2.0, 3.0, 0.95)], ms_ssim=True)
    assert csv.read_text().splitlines() == [EH.CSV_HEADER + ";ms_ssim", "a.hdr;30;0.9;2;3;0.95"]
    lines = []
    EH.log_score(lines.append, "a.hdr", (30.0, 0.9, 2.0, 3.0, 0.95))
    EH.log_mean(lines.append, [("a.hdr", 30.0, 0.9, 2.0, 3.0, 0.95)])
    assert "ms_ssim 0.950000" in lines[0] and "ms_ssim 0.950000" in lines[1]
    lines = []
    EH.log_score(lines.append, "a.hdr", (30.0, 0.9, 2.0, 3.0))
    EH.log_mean(lines.append, [("a.hdr", 30.0, 0.9, 2.0, 3.0)])
    assert "ms_ssim" not in lines[0] + lines[1]
