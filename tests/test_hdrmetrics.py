"""HDR quality metrics without a GPU: the numpy reference (tests/hdrmetrics_ref.py) against the
definition's check values, the argument checks of the two new entry points, and the host logic of
``python -m cnn_itmo_amd.evaluate_hdr`` with the scorer stubbed."""
import contextlib
import csv
import io
import os

import numpy as np
import pytest

import hdrmetrics_ref as HR
from oracle import tonemap_ref as TR


# ------------------------------------------------------------------------------ the reference
def test_pq_check_values():
    e = HR.pq(np.array([0.0, 100.0, 1e4]))
    assert abs(e[0] - 7.309559e-7) < 5e-14 and abs(e[1] - 0.5080784) < 5e-8 and e[2] == 1.0
    assert HR.pq(1e4) == 1.0 and HR.log_encoding(1e4) == 1.0 and HR.log_encoding(HR.LOG_FLOOR) == 0.0


@pytest.mark.parametrize("encoding", ["pq", "log"])
def test_encodings_are_monotonic_and_clamp(encoding):
    x = np.concatenate(([0.0], 2.0 ** np.linspace(-40, 14, 4000)))
    e = HR.ENCODINGS[encoding](x)
    assert (np.diff(e) >= 0).all() and e[0] >= 0.0 and e[-1] == 1.0
    inside = (x > HR.LOG_FLOOR) & (x < HR.PEAK)
    assert (np.diff(e[inside]) > 0).all()
    # NaN and negatives encode like the bottom, +inf and 1e30 like the top (fmax / fmin, not clip)
    lo, hi = HR.ENCODINGS[encoding](np.array([0.0, 1e4]))
    np.testing.assert_array_equal(HR.ENCODINGS[encoding](np.array([np.nan, -1.0, -np.inf, np.inf, 1e30])),
                                  [lo, lo, lo, hi, hi])
    img = np.array([[[np.nan, -1.0, 0.0]]], np.float32)
    assert HR.encode(img, encoding, 2.0).dtype == np.float32
    np.testing.assert_array_equal(HR.encode(img, encoding, 2.0).ravel(), np.float32([lo, lo, lo]))


@pytest.mark.parametrize("q", [0.01, 0.5, 0.99, 0.999, 1.0])
def test_percentile_brackets_the_order_statistic(q):
    _, r = HR.make_pair((3, 45, 83), seed=7)
    Q = HR.percentile(r, q)
    for i in range(3):
        Y = TR.rgb2lum(r[i]).astype(np.float32).astype(np.float64).reshape(-1)
        need = max(1, int(np.ceil(q * Y.size)))
        stat = np.sort(Y)[need - 1]  # the order statistic of rank need
        assert stat <= Q[i] <= stat * (1 + 1 / 64), (q, i, stat, Q[i])
        lo = np.quantile(Y, q, method="lower") if need > 1 else Y.min()
        assert lo <= stat <= np.quantile(Y, q, method="higher")


def test_percentile_edge_bins():
    img = np.zeros((1, 4, 4, 3), np.float32)
    assert HR.percentile(img, 0.5)[0] == np.float32(2.0 ** -32 * (1 + 1 / 64))  # bin 0's upper edge
    img[0, 0, 0] = [np.nan, -1.0, 0.0]
    img[0, 1, 1] = -5.0
    assert HR.percentile(img, 0.5)[0] == np.float32(2.0 ** -32 * (1 + 1 / 64))
    img[:] = np.inf
    assert HR.percentile(img, 1.0)[0] == np.float32(2.0 ** 32)
    img[:] = 1.0  # 1.0 is the lower edge of its bin
    assert HR.percentile(img, 1.0)[0] == np.float32(1 + 1 / 64)


def test_logmean_is_scale_invariant_and_none_is_not():
    p, r = HR.make_pair((1, 45, 83), seed=3, level=0.02)
    base = np.concatenate(HR.psnr_ssim(p, r))
    sp, sr = HR.scales(p, r)
    for c in (0.25, 3.7, 1e-3, 12345.678):  # (float64 products: no fp32 image holds p * 3.7 exactly)
        pc = p.astype(np.float64) * c
        spc, src = HR.scales(pc, r)
        assert abs(spc[0] * c / sp[0] - 1) <= 1e-12 and src[0] == sr[0]
        got = np.concatenate(HR.psnr_ssim(pc, r))
        assert np.abs(got - base).max() <= 1e-9, (c, got, base)
    ps_aligned = HR.psnr_ssim(p, r)[0][0]
    ps_none = HR.psnr_ssim(p, r, align="none")[0][0]
    print("aligned", ps_aligned, "dB, unaligned", ps_none, "dB")
    assert ps_aligned - ps_none > 20.0


# ------------------------------------------------------------------------------ the C ABI's checks
@pytest.fixture(scope="module")
def lib():
    from cnn_itmo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


P = 4096  # a non-null, aligned stand-in pointer: the checks return before anything is dereferenced


def test_hdr_encode_argument_checks(lib):
    assert lib.cnnitmo_hdr_encode(0, None, 1, 11, 11, P, P, None) < 0 and b"null" in lib.cnnitmo_last_error()
    assert lib.cnnitmo_hdr_encode(0, P, 1, 11, 11, None, P, None) < 0
    assert lib.cnnitmo_hdr_encode(1, P, 1, 11, 11, P, None, None) < 0
    assert lib.cnnitmo_hdr_encode(2, P, 1, 11, 11, P, P, None) < 0 and b"encoding" in lib.cnnitmo_last_error()
    assert lib.cnnitmo_hdr_encode(-1, P, 1, 11, 11, P, P, None) < 0
    assert lib.cnnitmo_hdr_encode(0, P, 0, 11, 11, P, P, None) < 0 and b"shape" in lib.cnnitmo_last_error()
    assert lib.cnnitmo_hdr_encode(0, P + 2, 1, 11, 11, P, P, None) < 0 and b"misaligned" in lib.cnnitmo_last_error()


def test_lum_percentile_argument_checks(lib):
    ws = lib.cnnitmo_lum_percentile_workspace_bytes(3)
    assert ws == 3 * 4096 * 4 and lib.cnnitmo_lum_percentile_workspace_bytes(0) <= 0
    args = (P, 3, 11, 11, None, 0.5, P, P, ws, None)

    def call(**kw):
        a = list(args)
        for k, v in kw.items():
            a[{"img": 0, "n": 1, "q": 5, "out": 6, "ws": 7, "bytes": 8}[k]] = v
        return lib.cnnitmo_lum_percentile(*a)

    for k in ("img", "out", "ws"):
        assert call(**{k: None}) < 0 and b"null" in lib.cnnitmo_last_error()
    for q in (0.0, -0.5, 1.0000001, float("nan")):
        assert call(q=q) < 0 and b"outside (0, 1]" in lib.cnnitmo_last_error()
    assert call(bytes=ws - 1) < 0 and b"workspace too small" in lib.cnnitmo_last_error()
    assert call(n=0) < 0 and b"shape" in lib.cnnitmo_last_error()


def test_python_option_errors_need_no_gpu():
    from cnn_itmo_amd import hdrmetrics as HM
    assert HM._anchor("key") == "key" and HM._anchor("percentile") == "percentile" and HM._anchor("2.5") == 2.5
    for bad in ("peak", 0.0, -1.0, float("nan"), None):
        with pytest.raises(ValueError, match="anchor"):
            HM._anchor(bad)
    with pytest.raises(ValueError, match="encoding"):
        HM._encoding_id("pu21")
    with pytest.raises(ValueError, match="outside"):
        HM.luminance_percentile(np.zeros((4, 4, 3), np.float32), q=0.0)


# ------------------------------------------------------------------------------ evaluate_hdr, scorer stubbed
def test_evaluate_hdr_pairing_skipping_and_csv(tmp_path, monkeypatch):
    from cnn_itmo_amd import evaluate_hdr as EH
    pred, ref = tmp_path / "pred", tmp_path / "ref"
    os.makedirs(pred)
    os.makedirs(ref)
    for name in ("b.hdr", "a.pfm", "c.pic", "d.hdr", "notes.txt", "e.png"):
        (pred / name).write_bytes(b"x")
    for name in ("a.hdr", "b.pfm", "c.pic", "x.hdr", "d.png"):  # d has no HDR reference
        (ref / name).write_bytes(b"x")
    calls = []

    def fake(pred_path, ref_path, encoding="pq", **opts):
        calls.append((os.path.basename(pred_path), os.path.basename(ref_path), encoding, opts))
        k = len(calls)
        return 30.0 + k, 0.9 + 0.01 * k, 1.5 * k, 0.125 * k

    monkeypatch.setattr(EH, "score_files", fake)
    csvp = str(tmp_path / "scores.csv")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert EH.main(["--pred", str(pred), "--reference", str(ref), "--encoding", "log", "--align", "median",
                        "--anchor", "percentile", "--percentile", "0.99", "--peak-nits", "4000", "--csv", csvp]) == 0
    # sorted by name, paired by stem across the extensions
    assert [c[:3] for c in calls] == [("a.pfm", "a.hdr", "log"), ("b.hdr", "b.pfm", "log"), ("c.pic", "c.pic", "log")]
    assert calls[0][3] == dict(align="median", anchor="percentile", key=0.18, white_nits=203.0, q=0.99,
                               peak_nits=4000.0)
    log = buf.getvalue()
    assert "d.hdr: no reference" in log and "mean of 3 scored HDR files: psnr 32.0000 dB, ssim 0.920000" in log
    assert "a.pfm: hdr psnr 31.0000 dB, ssim 0.910000" in log and "scored 3 of 4 files" in log
    with open(csvp, newline="") as fh:
        rows = list(csv.reader(fh, delimiter=";"))
    assert rows[0] == ["name", "psnr", "ssim", "scale_pred", "scale_ref"]
    assert [r[0] for r in rows[1:]] == ["a.pfm", "b.hdr", "c.pic"]
    assert [float(v) for v in rows[2][1:]] == [32.0, 0.92, 3.0, 0.25]
    # the defaults, a calibrated anchor, and the option errors
    calls.clear()
    with contextlib.redirect_stdout(io.StringIO()):
        assert EH.main(["--pred", str(pred), "--reference", str(ref), "--anchor", "80"]) == 0
    assert calls[0][2] == "pq" and calls[0][3] == dict(align="logmean", anchor=80.0, key=0.18, white_nits=203.0,
                                                       q=0.999, peak_nits=1000.0)
    for bad in (["--anchor", "peak"], ["--encoding", "pu21"], ["--align", "mean"], ["--percentile", "0"]):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            EH.main(["--pred", str(pred), "--reference", str(ref)] + bad)
    os.makedirs(tmp_path / "empty")
    with pytest.raises(FileNotFoundError):
        EH.main(["--pred", str(tmp_path / "empty"), "--reference", str(ref)])


def test_predict_hdr_reference_flags_are_checked_before_the_model_loads():
    from cnn_itmo_amd import predict as PR
    for flags in (["--hdr-reference", "ref"],                                      # needs --hdr
                  ["--hdr", "out", "--hdr-metrics-csv", "s.csv"],                    # needs --hdr-reference
                  ["--hdr", "out", "--hdr-log-average", "reference"],                # needs --hdr-reference
                  ["--hdr", "out", "--hdr-reference", "ref", "--hdr-log-average", "reference"],  # needs exact mode
                  ["--hdr", "out", "--hdr-log-average", "refrence"]):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            PR.main(["--model", "missing.hdf5"] + flags)
    assert PR._log_average_arg("2.5") == 2.5 and PR._log_average_arg("reference") == "reference"
