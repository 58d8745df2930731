"""GPU HDR quality metrics (csrc/hdrmetrics.hip, cnn_itmo_amd/hdrmetrics.py, evaluate_hdr and
``predict --hdr-reference``) against the numpy float64 reference (tests/hdrmetrics_ref.py).

Bounds.  Encode: every element within 1 fp32 ulp of the reference and at most 1e-3 of the elements
not identical (expected ~1e-7: OpenCL bounds fp64 pow at 16 ulp, so the cast to float flips with a
probability of about 16 * 2^-29; a systematic error would move every element).  Percentile: the
bits of the reference (integer counts).  Metric: tests/test_gpu_metrics.py's own bounds,
|ssim - ref| <= 1e-6 and |psnr - ref| <= 1e-4 dB; the encode adds isolated 6e-8 flips on top.
"""
import contextlib
import csv
import io
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cnn_itmo_amd as C  # noqa: E402
from cnn_itmo_amd import hdrio as H  # noqa: E402
from cnn_itmo_amd import hdrmetrics as HM  # noqa: E402
from cnn_itmo_amd import metrics as M  # noqa: E402
from cnn_itmo_amd import tonemap as T  # noqa: E402
import hdrmetrics_ref as HR  # noqa: E402
from arena import Arena, bits, poison_count  # noqa: E402

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-6
PSNR_TOL = 1e-4
# (2,11,11): a single window; odd widths (3*h*w % 4 != 0: the one-value paths); partial tiles
SHAPES = [(2, 11, 11), (1, 12, 27), (5, 45, 83), (1, 139, 261)]
ENCODINGS = ["pq", "log"]
ALIGNS = ["logmean", "median", "none"]
ANCHORS = ["key", "percentile", 50.0]
IDS = dict(ids=lambda s: "x".join(map(str, s)))
_PAIRS = {}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _pair(shape):
    """(prediction, reference) of a shape, made once; five images get five noise levels."""
    if shape not in _PAIRS:
        level = np.linspace(0.02, 0.4, 5) if shape[0] == 5 else 0.1
        _PAIRS[shape] = HR.make_pair(shape, seed=shape[1] * 1000 + shape[2], level=level)
    return _PAIRS[shape]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32).astype(np.int64)


def _host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------ encode
SPECIALS = np.array([0.0, -1.0, np.nan, np.inf, 1e30, 1e-45], np.float32)


@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_encode_matches_reference(shape, encoding):
    img = _pair(shape)[1].copy()
    n = shape[0]
    flat = img.reshape(n, -1)
    pos = np.arange(len(SPECIALS)) * 7 + 3  # (also inside a 16-byte group of the vector path)
    flat[0, pos] = SPECIALS
    flat[-1, -1] = np.nan  # the very last element
    scale = np.linspace(0.7, 90.0, n)  # a different scale per image
    got = HM.encode(img, encoding, scale)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == img.shape
    got = _host(got)
    want = HR.encode(img, encoding, scale)
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    ulps = np.abs(_u32(got) - _u32(want))
    share = float((ulps != 0).mean())
    print(f"{encoding} {shape}: max {ulps.max()} ulp, {share:.3g} of {ulps.size} elements not identical")
    assert ulps.max() <= 1
    assert share <= 1e-3
    # the planted values: their closed forms, exactly
    lo = np.float32(HR.C1 ** HR.M2) if encoding == "pq" else np.float32(0.0)
    p = got.reshape(n, -1)[0, pos]
    assert (p[:3] == lo).all() and (p[3:5] == np.float32(1.0)).all(), p
    assert p[5] == want.reshape(n, -1)[0, pos[5]] and (p[5] == 0.0 if encoding == "log" else p[5] > lo)
    assert got.reshape(-1)[-1] == lo
    # one scale for all images, [h,w,3] input, a CUDA tensor as the scale
    one = HM.encode(img[0], encoding, scale[0])
    assert tuple(one.shape) == (1,) + img.shape[1:] and np.array_equal(_u32(_host(one)[0]), _u32(got[0]))
    same = HM.encode(torch.from_numpy(img).cuda(), encoding, torch.from_numpy(scale).cuda())
    assert np.array_equal(_u32(_host(same)), _u32(got))


# ------------------------------------------------------------------------------ percentile
def _percentile_images(shape):
    img = _pair(shape)[1].copy()
    n = shape[0]
    img *= (np.float32(1.7) ** np.arange(n, dtype=np.float32)).reshape(n, 1, 1, 1)  # n different medians
    img[0, 0, :4] = 0.0
    img[0, 1, 2] = [-3.0, -1.0, -2.0]
    img[0, 2, 3] = [np.nan, 1.0, 1.0]
    img[-1, -1, -1] = [np.inf, 1.0, 1.0]
    if n == 5:  # a third of image 3 black, a tenth of image 4 negative or NaN
        img[3].reshape(-1, 3)[::3] = 0.0
        img[4].reshape(-1, 3)[::10] = [-1.0, np.nan, 0.5]
    return img


@pytest.mark.parametrize("q", [0.5, 0.99, 0.999, 1.0])
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_percentile_is_bitwise_the_reference(shape, q):
    img = _percentile_images(shape)
    got = HM.luminance_percentile(img, q)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (shape[0],)
    want = HR.percentile(img, q)
    assert np.array_equal(_u32(_host(got)), _u32(want)), (_host(got), want)
    if shape[0] == 5:
        assert len(set(want.tolist())) == 5, want
    lum = (0.3, 0.5, 0.2)
    assert np.array_equal(_u32(_host(HM.luminance_percentile(img, q, lum=lum))), _u32(HR.percentile(img, q, lum)))


# ------------------------------------------------------------------------------ the metric
@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_metric_matches_reference(shape, encoding):
    p, r = _pair(shape)
    pd, rd = torch.from_numpy(p).cuda(), torch.from_numpy(r).cuda()
    for align in ALIGNS:
        for anchor in ANCHORS:
            kw = dict(align=align, anchor=anchor)
            rp, rs = HR.psnr_ssim(p, r, encoding, **kw)
            ps, ss = HM.hdr_psnr_ssim(pd, rd, encoding, **kw)
            assert ps.is_cuda and ps.dtype == torch.float64 and tuple(ps.shape) == (shape[0],) == tuple(ss.shape)
            ep, es = np.abs(_host(ps) - rp).max(), np.abs(_host(ss) - rs).max()
            print(f"{encoding} {align} {anchor} {shape}: psnr err {ep:.3g} dB, ssim err {es:.3g}")
            assert ep <= PSNR_TOL, (kw, _host(ps), rp)
            assert es <= SSIM_TOL, (kw, _host(ss), rs)
            sp, sr = HM.hdr_scales(pd, rd, **kw)
            wp, wr = HR.scales(p, r, **kw)
            assert sp.dtype == torch.float64 and sp.is_cuda and tuple(sp.shape) == (shape[0],)
            np.testing.assert_allclose(_host(sp), wp, rtol=1e-12)
            np.testing.assert_allclose(_host(sr), wr, rtol=1e-12)
            if shape[0] == 5:  # five noise levels: five different values, each its own image's
                assert len(set(np.round(rp, 2))) == 5 and len(set(np.round(rs, 3))) == 5
            # composition: the metric of the encoded planes, bit for bit
            ea, eb = HM.encode(pd, encoding, sp), HM.encode(rd, encoding, sr)
            cp, cs = M.psnr_ssim(ea, eb)
            assert torch.equal(cp, ps) and torch.equal(cs, ss)
            # (PSNR alone takes image_metrics' plain reduction, whose sum is folded in another order)
            assert torch.equal(HM.hdr_psnr(pd, rd, encoding, **kw), M.psnr(ea, eb))
            assert torch.equal(HM.hdr_ssim(pd, rd, encoding, **kw), M.ssim(ea, eb))


def test_alignment_matters_and_other_options():
    p, r = _pair((5, 45, 83))
    aligned, none = _host(HM.hdr_psnr(p, r)), _host(HM.hdr_psnr(p, r, align="none"))
    assert (aligned - none > 10).all() and aligned[0] - none[0] > 20, (aligned, none)
    kw = dict(anchor="percentile", q=0.99, peak_nits=4000.0, lum=(0.3, 0.5, 0.2), align="median")
    rp, rs = HR.psnr_ssim(p, r, "pq", **kw)
    ps, ss = HM.hdr_psnr_ssim(p, r, "pq", **kw)  # numpy in
    assert np.abs(_host(ps) - rp).max() <= PSNR_TOL and np.abs(_host(ss) - rs).max() <= SSIM_TOL
    kw = dict(key=0.36, white_nits=100.0)
    rp, rs = HR.psnr_ssim(p[2], r[2], "log", **kw)
    ps, ss = HM.hdr_psnr_ssim(p[2], r[2], "log", **kw)  # [h,w,3]
    assert tuple(ps.shape) == (1,)
    assert abs(ps.item() - rp[0]) <= PSNR_TOL and abs(ss.item() - rs[0]) <= SSIM_TOL


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_identical_images(encoding):
    r = _pair((5, 45, 83))[1]
    for align in ALIGNS:
        ps, ss = HM.hdr_psnr_ssim(r, r.copy(), encoding, align=align)
        assert np.isposinf(_host(ps)).all() and (np.abs(1 - _host(ss)) <= SSIM_TOL).all()


def test_bitwise_deterministic():
    p, r = _pair((5, 45, 83))
    img = _percentile_images((5, 45, 83))

    def everything():
        out = [HM.encode(p, e, np.linspace(1, 5, 5)) for e in ENCODINGS]
        out += [HM.luminance_percentile(img, q) for q in (0.5, 0.999)]
        for align in ALIGNS:
            out += list(HM.hdr_psnr_ssim(p, r, align=align, anchor="percentile"))
            out += list(HM.hdr_scales(p, r, align=align))
        return [_host(t).tobytes() for t in out]

    assert everything() == everything()


def test_errors():
    p, r = _pair((1, 12, 27))
    with pytest.raises(ValueError, match="differ in shape"):
        HM.hdr_psnr_ssim(p, r[:, :11])
    with pytest.raises(ValueError, match="differ in shape"):
        HM.hdr_scales(p, r[:, :, :20])
    small_p, small_r = p[:, :10], r[:, :10]
    for fn in (HM.hdr_psnr_ssim, HM.hdr_ssim):
        with pytest.raises(ValueError, match="at least 11"):
            fn(small_p, small_r)
    sp, sr = HR.scales(small_p, small_r)  # PSNR alone has no minimum size
    want = HR.MR.psnr(HR.encode(small_p, "pq", sp), HR.encode(small_r, "pq", sr))[0]
    assert abs(HM.hdr_psnr(small_p, small_r).item() - want) <= PSNR_TOL
    for kw in (dict(encoding="pu21"), dict(align="mean"), dict(anchor="peak"), dict(anchor=-1.0),
               dict(anchor="percentile", q=1.5)):
        with pytest.raises(ValueError):
            HM.hdr_psnr_ssim(p, r, **kw)
    with pytest.raises(ValueError, match="encoding"):
        HM.encode(p, "pu21")
    with pytest.raises(ValueError, match="scale has"):
        HM.encode(p, "pq", [1.0, 2.0])
    with pytest.raises(ValueError, match="NHWC"):
        HM.encode(p[0, 0], "pq")


# ------------------------------------------------------------------------------ poisoned arena
@pytest.mark.parametrize("shape", [(2, 13, 19), (2, 12, 19)], **IDS)  # odd w; one-value and 16-byte paths
def test_poisoned_arena(shape):
    """Both launches with every operand inside an arena (bases 16-byte aligned and no more, 1 MiB
    of poison around each), outputs and the workspace handed over poisoned: complete writes, no
    byte outside the operands touched, the same bits under NaN and zero poison."""
    from cnn_itmo_amd import ops
    n, h, w = shape
    img = HR.make_pair(shape, seed=5)[1]
    img[0, 0, 0] = [np.nan, -1.0, 0.0]
    scale = np.array([2.5, 40.0])
    outs = {}
    for fill in ("nan", "zero"):
        arena = Arena(24 << 20, fill, "cuda")
        x = arena.take(img.size, torch.float32, data=img, name="img").view(n, h, w, 3)
        sc = arena.take(n, torch.float64, data=scale, name="scale")
        assert x.data_ptr() % 128 == 16
        res = {}
        for enc in ENCODINGS:
            out = arena.take(img.size, torch.float32, name="encoded_" + enc)
            ops.hdr_encode(ops.HDR_ENCODINGS[enc], x, sc, out.view(n, h, w, 3))
            res["encoded_" + enc] = out
        real_ws = ops.workspace
        ops.workspace = lambda nb, device="cuda": arena.take(max(16, int(nb)), torch.uint8, name="workspace")
        try:
            for q in (0.5, 1.0):
                res[f"Q{q}"] = ops.lum_percentile(x, q, out=arena.take(n, torch.float32, name=f"Q{q}"))
        finally:
            ops.workspace = real_ws
        torch.cuda.synchronize()
        arena.check_untouched()
        outs[fill] = {k: v.clone() for k, v in res.items()}
    for k, v in outs["nan"].items():
        assert poison_count(v) == 0, f"{k}: {poison_count(v)} of {v.numel()} elements were not written"
        assert bool(torch.isfinite(v).all()), k
        assert int((bits(v) != bits(outs["zero"][k])).sum()) == 0, f"{k} depends on memory outside the operands"
    for enc in ENCODINGS:
        want = HR.encode(img, enc, scale)
        assert np.abs(_u32(_host(outs["nan"]["encoded_" + enc]).reshape(img.shape)) - _u32(want)).max() <= 1
    for q in (0.5, 1.0):
        assert np.array_equal(_u32(_host(outs["nan"][f"Q{q}"])), _u32(HR.percentile(img, q)))


# ------------------------------------------------------------------------------ files and the CLIs
def test_evaluate_hdr_cli(tmp_path):
    from cnn_itmo_amd import evaluate_hdr as EH
    p, r = HR.make_pair((3, 24, 37), seed=9, level=[0.05, 0.1, 0.2])
    pred, ref = tmp_path / "pred", tmp_path / "ref"
    os.makedirs(pred)
    os.makedirs(ref)
    names = [("a.hdr", "a.hdr"), ("b.pfm", "b.hdr"), ("c.hdr", "c.pfm")]
    for i, (pn, rn) in enumerate(names):
        H.write_image(str(pred / pn), p[i])
        H.write_image(str(ref / rn), r[i])
    H.write_image(str(pred / "d.hdr"), p[0])  # no reference: reported and skipped
    csvp = str(tmp_path / "scores.csv")
    opts = ["--align", "median", "--anchor", "percentile", "--percentile", "0.99"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert EH.main(["--pred", str(pred), "--reference", str(ref), "--csv", csvp] + opts) == 0
    log = buf.getvalue()
    with open(csvp, newline="") as fh:
        rows = list(csv.reader(fh, delimiter=";"))
    assert rows[0] == ["name", "psnr", "ssim", "scale_pred", "scale_ref"]
    assert [row[0] for row in rows[1:]] == ["a.hdr", "b.pfm", "c.hdr"]
    assert "d.hdr: no reference" in log and "mean of 3 scored HDR files" in log
    kw = dict(align="median", anchor="percentile", q=0.99)
    psnrs = []
    for (pn, rn), row in zip(names, rows[1:]):
        a, b = H.read_image(str(pred / pn)), H.read_image(str(ref / rn))  # the files read back (RGBE is lossy)
        ps, ss = HM.hdr_psnr_ssim(a, b, **kw)
        sp, sr = HM.hdr_scales(a, b, **kw)
        assert float(row[1]) == float(f"{ps.item():.10g}") and float(row[2]) == float(f"{ss.item():.10g}")
        assert float(row[3]) == sp.item() and float(row[4]) == sr.item()
        assert f"{pn}: hdr psnr {ps.item():.4f} dB, ssim {ss.item():.6f}" in log
        rp, rs = HR.psnr_ssim(_host(a), _host(b), **kw)
        assert abs(ps.item() - rp[0]) <= PSNR_TOL and abs(ss.item() - rs[0]) <= SSIM_TOL
        psnrs.append(ps.item())
    assert psnrs[0] > psnrs[1] > psnrs[2]
    assert f"psnr {np.mean(psnrs):.4f} dB" in log
    # a reference of another size is an error
    H.write_image(str(ref / "d.pfm"), r[0][:20])
    with pytest.raises(ValueError, match="d.pfm"), contextlib.redirect_stdout(io.StringIO()):
        EH.main(["--pred", str(pred), "--reference", str(ref)])


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """A small saved model, two 32 x 48 PNGs, HDR references for them and the default run's output
    (the fixture pattern of tests/test_gpu_hdrio.py)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from PIL import Image
    from cnn_itmo_amd import predict as PR
    d = tmp_path_factory.mktemp("hdrmetricscli")
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        m = C.U_net(input_size=(32, 32, 3), seed=5, verbose=False)
    rng = np.random.default_rng(2)
    m.set_named_weights({k: rng.uniform(0.5, 1.5, v.shape) for k, v in m.named_weights().items()
                         if k.endswith("/moving_variance")})
    ck = str(d / "tiny.hdf5")
    m.save(ck)
    os.makedirs(str(d / "in"))
    for name in ("first", "second"):
        Image.fromarray(rng.integers(0, 256, (32, 48, 3), dtype=np.uint8)).save(str(d / "in" / f"{name}.png"))
    refs = HR.make_pair((2, 32, 48), seed=12)[1] * np.float32([[[[1.0]]], [[[5.0]]]])
    os.makedirs(str(d / "ref_both"))
    os.makedirs(str(d / "ref_one"))
    H.write_image(str(d / "ref_both" / "first.hdr"), refs[0])
    H.write_image(str(d / "ref_both" / "second.pfm"), refs[1])
    H.write_image(str(d / "ref_one" / "first.pfm"), refs[0])

    def run(out, *extra):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            assert PR.main(["--model", ck, "--input", str(d / "in"), "--output", str(d / out)] + list(extra)) == 0
        return {n: open(str(d / out / n), "rb").read() for n in sorted(os.listdir(str(d / out)))}, buf.getvalue()

    base, _ = run("out0")
    assert sorted(base) == ["first.png", "second.png"]
    return {"dir": d, "run": run, "base": base}


def test_predict_hdr_reference(cli):
    from cnn_itmo_amd import evaluate_hdr as EH
    d = cli["dir"]
    csvp = str(d / "hdr_scores.csv")
    pngs, log = cli["run"]("out1", "--hdr", str(d / "hdr1"), "--hdr-reference", str(d / "ref_one"),
                           "--hdr-metrics-csv", csvp)
    assert pngs == cli["base"]  # the PNGs are byte-identical with and without the new flags
    assert sorted(os.listdir(str(d / "hdr1"))) == ["first.hdr", "second.hdr"]
    with open(csvp, newline="") as fh:
        rows = list(csv.reader(fh, delimiter=";"))
    assert rows[0] == ["name", "psnr", "ssim", "scale_pred", "scale_ref"] and len(rows) == 2  # one referenced file
    assert "second.hdr: no reference" in log and "mean of 1 scored HDR files" in log
    # the written file, read back from disk, against the reference with the defaults; script-mode
    # reconstructions hold zeros, so the log-average alignment is what the defaults give, not a good one
    a, b = H.read_image(str(d / "hdr1" / "first.hdr")), H.read_image(str(d / "ref_one" / "first.pfm"))
    ps, ss = HM.hdr_psnr_ssim(a, b)
    sp, sr = HM.hdr_scales(a, b)
    assert rows[1][0] == "first.hdr"
    assert float(rows[1][1]) == float(f"{ps.item():.10g}") and float(rows[1][2]) == float(f"{ss.item():.10g}")
    assert float(rows[1][3]) == sp.item() and float(rows[1][4]) == sr.item()
    assert EH.score_files(str(d / "hdr1" / "first.hdr"), str(d / "ref_one" / "first.pfm")) == \
        (ps.item(), ss.item(), sp.item(), sr.item())


def test_predict_hdr_log_average_from_reference(cli):
    d = cli["dir"]
    exact = ["--hdr-mode", "exact", "--hdr-format", "pfm"]
    pngs, log = cli["run"]("out2", "--hdr", str(d / "hdr2"), "--hdr-reference", str(d / "ref_both"),
                           "--hdr-log-average", "reference", *exact)
    assert pngs == cli["base"] and "mean of 2 scored HDR files" in log
    g = {"first": T.log_average(H.read_image(str(d / "ref_both" / "first.hdr"))).item(),
         "second": T.log_average(H.read_image(str(d / "ref_both" / "second.pfm"))).item()}
    assert g["second"] > 4 * g["first"]
    for name in ("first", "second"):  # a run given that file's log-average as a float
        cli["run"]("out_" + name, "--hdr", str(d / ("hdr_" + name)), "--hdr-log-average", repr(g[name]), *exact)
        assert open(str(d / "hdr2" / f"{name}.pfm"), "rb").read() == \
            open(str(d / ("hdr_" + name) / f"{name}.pfm"), "rb").read()
