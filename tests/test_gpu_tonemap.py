"""Tone mapping on the GPU (csrc/tonemap.hip behind cnnitmo_tonemap_stats, cnnitmo_tonemap_apply and
cnnitmo_inverse_reinhard_apply; cnn_itmo_amd/tonemap.py) against oracle/tonemap_ref.py (float64, one image
at a time).  Inputs and references: tests/tonemap_cases.py.

The contract: the statistics pass gives every image its own [sum of log(max(f, realmin)), count of zero
luminance] whatever the size of the image and of the batch; the maps are the oracle's, pixel by pixel,
MATLAB's special values included; a call writes its outputs and its workspace and nothing else, and
nothing at all when its arguments are bad; the same input gives the same bits, alone or in a batch.

Tolerances (the project's, from the header of test_tonemap.py):
  fp32 outputs  rtol 2e-6, equal_nan: float64 arithmetic on both sides, the last bits of log / exp / pow
                differ.  atol 1e-37 only where values underflow in the cast to float (the script-mode
                inverse, the fp32 denormal of the special pixels), 0 everywhere else.
  G             rtol 1e-12, against exp(math.fsum(logs) / hw) and against the oracle's sequential sum.  The
                two references agree to 7e-15 at these sizes, and one lost pixel of 130 000 moves G by
                more than 1e-6.
  stats[2i]     fp32 in: |sum - fsum(logs)| <= 1e-12 * hw * max|log|.  uint8 in (inverse_Reinhard.m's
                X = I/(I-1) <= 0, so every term is log(realmin)): hw * log(realmin) to rtol 1e-15 -- a lost or
                doubled pixel is 1.5e-5 of it.  A tree of equal terms adds without rounding, so only the
                tail block and the last bit of log() are left: 0 to 2.2e-16 measured.  (The sequential
                final fold this test found was off by 4.4e-15 from 256x256 on; the fold is a tree now.)
  stats[2i+1]   exact.
  uint8 outputs equal im2uint8(oracle) exactly, except where the oracle's 255 x lies within 1e-6 of a .5
                tie; there a difference of 1 is allowed.  Such elements must stay below 0.1 % of the
                image; measured on the CPU for the seeds used here: 2x257x259 Reinhard 0, Reinhard key 0.5
                / Rec. 601 1 of 399 378, camera 1 of 399 378; 3x37x61 and the special-pixel batches 0 of
                20 313 each.
  bits          G3 and G4 compare bits, no tolerance.

test_tonemap.py::test_gpu_exact_roundtrip_full_hd maps with the GPU's own G and inverts with the same G, so
G cancels: it passes for any G.  test_log_average and test_raw_stats_hdr below are what pin G past one
sweep of the statistics grid (256 blocks x 256 threads = 65 536 pixels).
"""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
# the cached inputs are read-only numpy arrays; torch.as_tensor remarks on that
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

import tonemap_cases as K  # noqa: E402
from arena import Arena, poison_count  # noqa: E402
from oracle import tonemap_ref as T  # noqa: E402
from tonemap_cases import same_bits  # noqa: E402

# 16x16: one block; 1x257: a second block of one pixel; 256x256: every thread one pixel; 1x65537: one thread
# takes a second pixel; 300x437: just past two sweeps; 65 and 130 images: more than 64 and than 128 images
STAT_SHAPES = ["1x1x1", "1x16x16", "1x1x257", "1x256x256", "1x1x65537", "2x257x259", "1x300x437", "65x3x5",
               "130x2x3"]
STAT_SHAPES_U8 = STAT_SHAPES[:6]
EINVAL = -1


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_itmo_amd import _lib as L
    L.load()


def tm():
    from cnn_itmo_amd import tonemap
    return tonemap


def lib():
    from cnn_itmo_amd import _lib as L
    return L.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def ws_bytes(n):
    return int(lib().cnnitmo_tonemap_workspace_bytes(n))


def _p(t):
    return None if t is None else t.data_ptr()


def _lump(lum):
    if lum is None:
        return None, None
    arr = (ctypes.c_double * 3)(*lum)
    return arr, ctypes.addressof(arr)


def raw_stats(mode, img, n, h, w, stats, ws, nb, lum=None):
    from cnn_itmo_amd import ops
    keep, lp = _lump(lum)
    return lib().cnnitmo_tonemap_stats(mode, _p(img), n, h, w, lp, _p(stats), _p(ws), nb, ops.stream_ptr())


def raw_apply(curve, hdr, n, h, w, params, stats, out_u8, out, lum=None):
    from cnn_itmo_amd import ops
    keep, lp = _lump(lum)
    return lib().cnnitmo_tonemap_apply(curve, _p(hdr), n, h, w, lp, _p(params), _p(stats), out_u8, _p(out),
                                       ops.stream_ptr())


def raw_inverse(mode, sdr, n, h, w, stats, a, g, out, lum=None):
    from cnn_itmo_amd import ops
    keep, lp = _lump(lum)
    return lib().cnnitmo_inverse_reinhard_apply(mode, _p(sdr), n, h, w, lp, _p(stats), a, g, _p(out),
                                                ops.stream_ptr())


def last_error():
    return lib().cnnitmo_last_error().decode(errors="replace")


def stats_of(img, mode, lum=None):
    """[n, 2] float64 through the raw ABI, from NaN-filled stats and workspace."""
    t = dev(img)
    n, h, w, _ = t.shape
    nb = ws_bytes(n)
    ws = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((2 * n,), float("nan"), dtype=torch.float64, device="cuda")
    assert raw_stats(mode, t, n, h, w, st, ws, nb, lum) == 0, last_error()
    return host(st).reshape(n, 2)


def close32(got, ref64, atol=0.0):
    assert got.dtype == np.float32
    with np.errstate(over="ignore"):
        want = np.asarray(ref64, np.float64).astype(np.float32)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=atol, equal_nan=True)


def per_image(fn, batch, *per):
    return np.stack([fn(im, *[p[i] for p in per]) for i, im in enumerate(batch)])


# ---------------------------------------------------------------- G1: the statistics, where the partition changes
@pytest.mark.parametrize("case", STAT_SHAPES)
def test_log_average(case):
    hdr = K.hdr_batch(case)
    n, h, w = K.shape_of(case)
    G = host(tm().log_average(hdr))
    assert G.dtype == np.float64 and G.shape == (n,)
    refs = K.cached(("g_refs", case), lambda: np.array([K.g_refs(im) for im in hdr]))
    np.testing.assert_allclose(G, refs[:, 0], rtol=1e-12, err_msg="against exp(fsum(logs) / hw)")
    np.testing.assert_allclose(G, refs[:, 1], rtol=1e-12, err_msg="against the oracle's log_average")


@pytest.mark.parametrize("rot", [0, 1, 2])
@pytest.mark.parametrize("case", STAT_SHAPES)
def test_raw_stats_hdr(case, rot):
    """stats[2i] against the exactly rounded sum of the logs, stats[2i+1] the planted zero-luminance
    pixels: 0, 1 or 7 per image (rot turns which image gets which), some past pixel 65 536."""
    hdr, counts = K.plant_zeros(K.hdr_batch(case), rot)
    n, h, w = K.shape_of(case)
    st = stats_of(hdr, 0)
    for i in range(n):
        s, m = K.log_sum_exact(hdr[i])
        assert abs(st[i, 0] - s) <= 1e-12 * h * w * m, (i, st[i, 0], s)
    np.testing.assert_array_equal(st[:, 1], np.array(counts, np.float64))


@pytest.mark.parametrize("rot", [0, 1, 2])
@pytest.mark.parametrize("case", STAT_SHAPES_U8)
def test_raw_stats_sdr(case, rot):
    """Mode 1: every term is log(realmin), so the sum is hw * log(realmin) and any lost or doubled pixel
    shows; the count is that of the all-zero pixels."""
    sdr, counts = K.plant_zeros(K.sdr_batch(case), rot)
    n, h, w = K.shape_of(case)
    st = stats_of(sdr, 1)
    print(case, rot, "relative error of the sum", np.abs(st[:, 0] / (h * w * math.log(T.REALMIN)) - 1))
    np.testing.assert_array_equal(st[:, 1], np.array(counts, np.float64))
    np.testing.assert_allclose(st[:, 0], h * w * math.log(T.REALMIN), rtol=1e-15, atol=0)


def test_stats_with_luminance_weights():
    """Custom weights reach the statistics pass (Rec. 601 against the Rec. 709 default)."""
    hdr = K.hdr_batch("2x257x259")
    G = host(tm().log_average(hdr, lum=K.LUM601))
    for i in range(2):
        for ref in K.g_refs(hdr[i], K.LUM601):
            np.testing.assert_allclose(G[i], ref, rtol=1e-12)
    assert not np.allclose(G, host(tm().log_average(hdr)), rtol=1e-6)


# ---------------------------------------------------------------- G2: the maps against the oracle
@pytest.mark.parametrize("key,lum", [(0.18, None), (0.5, K.LUM601)], ids=["default", "key0.5-rec601"])
@pytest.mark.parametrize("case", K.MAP_SHAPES)
def test_reinhard(case, key, lum):
    hdr = K.map_hdr(case)
    ref = K.cached(("reinhard", case, key), lambda: per_image(lambda im: T.reinhard(im, key, lum or T.REC709), hdr))
    assert np.isnan(ref[0, 0, 0]).all() and np.isfinite(ref[0, 0, 1]).all()
    close32(host(tm().reinhard(hdr, key=key, lum=lum)), ref)
    K.check_u8(host(tm().reinhard(hdr, key=key, lum=lum, out_u8=True)), ref)


@pytest.mark.parametrize("case", K.MAP_SHAPES)
def test_virtual_camera(case):
    """Per-image (v, n, y) as the script draws them, and one extreme image where min(1, .) binds."""
    hdr = K.map_hdr(case)
    v, cn, cy = K.camera_params(len(hdr))
    ref = K.cached(("camera", case), lambda: per_image(T.virtual_camera, hdr, v, cn, cy))
    clipped = np.isclose(T.rgb2lum(ref[-1]), 1.0, rtol=1e-12, atol=0).mean()  # the luminance of the output is L
    assert clipped > 0.2, f"only {clipped:.3f} of the extreme image reaches min(1, .)"
    close32(host(tm().virtual_camera(hdr, v, cn, cy)), ref)
    K.check_u8(host(tm().virtual_camera(hdr, v, cn, cy, out_u8=True)), ref)


@pytest.mark.parametrize("white", [False, True], ids=["plain", "white-pixel"])
@pytest.mark.parametrize("case", list(K.SCRIPT_KINDS))
def test_inverse_script(case, white):
    """inverse_Reinhard.m as written, per image with no, some and only zero-luminance pixels, without and
    with an all-255 pixel (I = 1: X = inf, so G_X = inf; that pixel's E clamps to 2^32)."""
    sdr = K.script_sdr(case, white)
    ref = K.cached(("script", case, white), lambda: per_image(lambda im: T.inverse_reinhard(im, mode="script"), sdr))
    if white:
        for r in ref:
            assert (r == 2.0 ** 32).sum() == 3
    close32(host(tm().inverse_reinhard(sdr, mode="script")), ref, atol=1e-37)


@pytest.mark.parametrize("case", K.MAP_SHAPES)
def test_inverse_exact(case):
    """The exact inverse against the oracle (not against the forward map), with a pixel of exactly 1
    (clamped to 2^32), one of 1.5 (negative) and a zero pixel (NaN)."""
    sdr = K.exact_sdr(case)
    ref = K.cached(("exact", case),
                   lambda: per_image(lambda im: T.inverse_reinhard(im, mode="exact", g=K.EXACT_G), sdr))
    assert (ref[:, 1, 1] == 2.0 ** 32).all() and (ref[:, 2, 0] < 0).all() and np.isnan(ref[:, 0, 2]).all()
    close32(host(tm().inverse_reinhard(sdr, mode="exact", g=K.EXACT_G)), ref)
    ref_a = per_image(lambda im: T.inverse_reinhard(im, a=0.3, lum=K.LUM601, mode="exact", g=2.5), sdr[:1])
    close32(host(tm().inverse_reinhard(sdr[:1], a=0.3, lum=K.LUM601, mode="exact", g=2.5)), ref_a)


@pytest.mark.parametrize("kind", ["finite", "inf", "nan"])
def test_special_pixels_stay_in_their_image(kind):
    """Image 1 of three holds a negative pixel, an fp32 denormal and a zero pixel ('finite'), those and a
    +inf channel ('inf': G = inf), or a NaN pixel ('nan': G = NaN and Reinhard's whole image is NaN).
    Every image, the special one included, is the oracle's of that image alone."""
    hdr = K.special_hdr(kind)
    v, cn, cy = K.camera_params(3, seed=6)
    G = host(tm().log_average(hdr))
    Gref = np.array([T.log_average(T.rgb2lum(im)) for im in hdr])
    np.testing.assert_allclose(G, Gref, rtol=1e-12, equal_nan=True)
    assert {"finite": np.isfinite, "inf": np.isposinf, "nan": np.isnan}[kind](G[K.SPECIAL_IMAGE])
    ref_r = per_image(T.reinhard, hdr)
    ref_c = per_image(T.virtual_camera, hdr, v, cn, cy)
    got_r, got_c = host(tm().reinhard(hdr)), host(tm().virtual_camera(hdr, v, cn, cy))
    if kind == "nan":  # Reinhard: all NaN.  The camera's min(1, NaN) = 1 leaves hdr / Y
        assert np.isnan(ref_r[1]).all() and np.isnan(got_r[1]).all()
        assert np.isnan(ref_c[1]).sum() == 3 and np.isnan(got_c[1]).sum() == 3
    for i in (0, 2):
        assert np.isfinite(got_r[i]).all() and np.isfinite(got_c[i]).all()
    close32(got_r, ref_r, atol=1e-37)
    close32(got_c, ref_c, atol=1e-37)
    K.check_u8(host(tm().reinhard(hdr, out_u8=True)), ref_r)
    K.check_u8(host(tm().virtual_camera(hdr, v, cn, cy, out_u8=True)), ref_c)


# ---------------------------------------------------------------- G3: batch independence and repeatability
def _bits_inputs(case):
    n, h, w = K.shape_of(case)
    rng = np.random.default_rng(77)
    hdr = np.array(K.hdr_batch(case, seed=600))
    hdr[n - 1, 1, 1] = 0.0
    sdr = np.array(K.sdr_batch(case, seed=650))
    sdr[::2, 0, :3] = 0  # PB1 differs from image to image
    lin = rng.uniform(0.0, 1.2, (n, h, w, 3)).astype(np.float32)
    v, cn, cy = K.camera_params(n, seed=9)
    return dict(hdr=hdr, sdr=sdr, lin=lin, v=v, cn=cn, cy=cy)


def _all_maps(a, sl=slice(None)):
    """Every map and both statistics of the images a[...][sl], as numpy."""
    t = tm()
    hdr, sdr, lin, v, cn, cy = (a[k][sl] for k in ("hdr", "sdr", "lin", "v", "cn", "cy"))
    return {
        "stats hdr": stats_of(hdr, 0), "stats sdr": stats_of(sdr, 1), "stats hdr rec601": stats_of(hdr, 0, K.LUM601),
        "log_average": host(t.log_average(hdr)),
        "reinhard": host(t.reinhard(hdr)), "reinhard u8": host(t.reinhard(hdr, out_u8=True)),
        "reinhard key lum": host(t.reinhard(hdr, key=0.5, lum=K.LUM601)),
        "camera": host(t.virtual_camera(hdr, v, cn, cy)),
        "camera u8": host(t.virtual_camera(hdr, v, cn, cy, out_u8=True)),
        "inverse script": host(t.inverse_reinhard(sdr)),
        "inverse exact": host(t.inverse_reinhard(lin, mode="exact", g=K.EXACT_G)),
    }


@pytest.mark.parametrize("case", ["5x33x40", "2x257x259"])
def test_image_in_a_batch_equals_image_alone(case):
    """stats[2 * im] and params[3 * im]: image i of a batch has the bits of image i alone, with camera
    parameters, zero counts and contents that differ from image to image."""
    a = _bits_inputs(case)
    n = K.shape_of(case)[0]
    assert len({tuple(p) for p in zip(a["v"], a["cn"], a["cy"])}) == n
    batch = _all_maps(a)
    for i in range(n):
        one = _all_maps(a, slice(i, i + 1))
        for name, got in batch.items():
            try:
                same_bits(got[i], one[name][0])
            except AssertionError as e:
                raise AssertionError(f"{name}, image {i} of {n}: {e}") from None
    for i in range(1, n):  # and the images do differ
        assert (batch["reinhard"][i] != batch["reinhard"][0]).any()
        assert batch["stats hdr"][i, 0] != batch["stats hdr"][0, 0]


@pytest.mark.parametrize("case", ["5x33x40", "2x257x259"])
def test_two_runs_give_equal_bits(case):
    a = _bits_inputs(case)
    first, second = _all_maps(a), _all_maps(a)
    for name in first:
        same_bits(first[name], second[name])


# ---------------------------------------------------------------- G4: poisoned arena and arguments
ARENA_SHAPE = (2, 67, 131)


def _arena_run(fill):
    """Every entry point with every operand carved from a poisoned arena; the outputs as numpy."""
    n, h, w = ARENA_SHAPE
    case = "x".join(str(v) for v in ARENA_SHAPE)
    hdr = K.hdr_batch(case, seed=700)
    sdr = K.sdr_batch(case, seed=750)
    lin = np.stack([T.reinhard(im) for im in hdr]).astype(np.float32)
    v, cn, cy = K.camera_params(n, seed=11)
    params = np.stack([0.18 * 2.0 ** v, cn, cy], axis=1)
    nb = ws_bytes(n)
    assert nb == n * 256 * 2 * 8
    ar = Arena(40 << 20, fill, "cuda")
    f32, f64, u8 = torch.float32, torch.float64, torch.uint8
    d_hdr = ar.take(hdr.size, f32, hdr, "hdr")
    d_sdr = ar.take(sdr.size, u8, sdr, "sdr")
    d_lin = ar.take(lin.size, f32, lin, "linear sdr")
    d_par = ar.take(params.size, f64, params, "camera params")
    key = np.array([[0.18, 0.0, 0.0]] * n)
    d_key = ar.take(key.size, f64, key, "reinhard params")
    st0 = ar.take(2 * n, f64, name="stats mode 0")
    st1 = ar.take(2 * n, f64, name="stats mode 1")
    ws0 = ar.take(nb, u8, name="workspace mode 0")  # exactly cnnitmo_tonemap_workspace_bytes(n)
    ws1 = ar.take(nb, u8, name="workspace mode 1")
    outs = {k: ar.take(hdr.size, u8 if k.endswith("u8") else f32, name=k)
            for k in ("reinhard", "reinhard u8", "camera", "camera u8", "inverse script", "inverse exact")}
    assert raw_stats(0, d_hdr, n, h, w, st0, ws0, nb) == 0, last_error()
    assert raw_stats(1, d_sdr, n, h, w, st1, ws1, nb) == 0, last_error()
    assert raw_apply(0, d_hdr, n, h, w, d_key, st0, 0, outs["reinhard"]) == 0, last_error()
    assert raw_apply(0, d_hdr, n, h, w, d_key, st0, 1, outs["reinhard u8"]) == 0, last_error()
    assert raw_apply(1, d_hdr, n, h, w, d_par, st0, 0, outs["camera"]) == 0, last_error()
    assert raw_apply(1, d_hdr, n, h, w, d_par, st0, 1, outs["camera u8"]) == 0, last_error()
    assert raw_inverse(1, d_sdr, n, h, w, st1, 0.18, 1.0, outs["inverse script"]) == 0, last_error()
    assert raw_inverse(2, d_lin, n, h, w, None, 0.18, K.EXACT_G, outs["inverse exact"]) == 0, last_error()
    ar.check_untouched()
    same_bits(host(d_hdr).reshape(hdr.shape), hdr)
    same_bits(host(d_sdr).reshape(sdr.shape), sdr)
    same_bits(host(d_lin).reshape(lin.shape), lin)
    same_bits(host(d_par).reshape(params.shape), params)
    same_bits(host(d_key).reshape(key.shape), key)
    if fill == "nan":  # a uint8 output may hold a legitimate 255: the zero fill and the equal bits cover those
        for name, t in list(outs.items()) + [("stats 0", st0), ("stats 1", st1), ("ws 0", ws0.view(f64)),
                                             ("ws 1", ws1.view(f64))]:
            if t.dtype != u8:
                assert poison_count(t) == 0, f"{name}: {poison_count(t)} elements left unwritten"
    res = {k: host(t).reshape(n, h, w, 3) for k, t in outs.items()}
    res.update({"stats 0": host(st0), "stats 1": host(st1), "ws 0": host(ws0.view(f64)), "ws 1": host(ws1.view(f64))})
    return res, dict(hdr=hdr, sdr=sdr, lin=lin, v=v, cn=cn, cy=cy)


def test_poisoned_arena():
    """2x67x131, operands 16-byte aligned and no more, between 1 MiB guards of NaN bytes and of zero bytes:
    nothing outside the outputs and the workspace is written, every output element is written, the
    inputs are unchanged, both fills give the bits the wrapper gives from torch's allocator."""
    nan, a = _arena_run("nan")
    zero, _ = _arena_run("zero")
    for name in nan:
        try:
            same_bits(nan[name], zero[name])
        except AssertionError as e:
            raise AssertionError(f"{name}, NaN fill against zero fill: {e}") from None
    t = tm()
    same_bits(nan["reinhard"], host(t.reinhard(a["hdr"])))
    same_bits(nan["reinhard u8"], host(t.reinhard(a["hdr"], out_u8=True)))
    same_bits(nan["camera"], host(t.virtual_camera(a["hdr"], a["v"], a["cn"], a["cy"])))
    same_bits(nan["camera u8"], host(t.virtual_camera(a["hdr"], a["v"], a["cn"], a["cy"], out_u8=True)))
    same_bits(nan["inverse script"], host(t.inverse_reinhard(a["sdr"])))
    same_bits(nan["inverse exact"], host(t.inverse_reinhard(a["lin"], mode="exact", g=K.EXACT_G)))
    close32(nan["reinhard"], per_image(T.reinhard, a["hdr"]))


def _bad_calls(fn, base, bad):
    for ch, msg in bad:
        rc = fn(**dict(base, **ch))
        assert rc == EINVAL, (ch, rc)
        assert msg in last_error(), (ch, last_error())


def test_bad_arguments_write_nothing():
    n, h, w = 2, 16, 16
    nan = float("nan")
    hdr = dev(K.hdr_batch("2x16x16", seed=800))
    sdr = dev(K.sdr_batch("2x16x16", seed=850))
    params = dev(np.array([[0.18, 0.6, 0.9]] * n))
    nb = ws_bytes(n)
    ws = torch.full((nb // 8,), nan, dtype=torch.float64, device="cuda")
    stats = torch.full((2 * n,), nan, dtype=torch.float64, device="cuda")
    out = torch.full((n, h, w, 3), nan, device="cuda")
    shapes = [(dict(n=0), "bad shape"), (dict(n=-1), "bad shape"), (dict(h=0), "bad shape"), (dict(h=-3), "bad shape"),
              (dict(w=0), "bad shape"), (dict(w=-1), "bad shape")]
    # statistics: n = 65536 is refused before any launch (the grid's y), so the small buffers are safe
    _bad_calls(raw_stats, dict(mode=0, img=hdr, n=n, h=h, w=w, stats=stats, ws=ws, nb=nb),
               [(dict(mode=-1), "mode"), (dict(mode=2), "mode"), (dict(img=None), "null"), (dict(stats=None), "null"),
                (dict(ws=None), "null"), (dict(n=65536), "bad shape"), (dict(nb=nb - 1), "workspace")] + shapes)
    # the maps: finite statistics, so that a launch would write numbers
    good = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    _bad_calls(raw_apply, dict(curve=0, hdr=hdr, n=n, h=h, w=w, params=params, stats=good, out_u8=0, out=out),
               [(dict(curve=-1), "curve"), (dict(curve=2), "curve"), (dict(hdr=None), "null"),
                (dict(params=None), "null"), (dict(stats=None), "null"), (dict(out=None), "null")] + shapes)
    _bad_calls(raw_inverse, dict(mode=1, sdr=sdr, n=n, h=h, w=w, stats=good, a=0.18, g=1.0, out=out),
               [(dict(mode=0), "mode"), (dict(mode=3), "mode"), (dict(sdr=None), "null"), (dict(out=None), "null"),
                (dict(stats=None), "null")] + shapes)
    _bad_calls(raw_inverse, dict(mode=2, sdr=hdr, n=n, h=h, w=w, stats=None, a=0.18, g=1.0, out=out),
               [(dict(sdr=None), "null"), (dict(out=None), "null")] + shapes)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(stats).all()) and bool(torch.isnan(ws).all())
    # one good call each
    assert raw_stats(0, hdr, n, h, w, stats, ws, nb) == 0, last_error()
    assert raw_apply(1, hdr, n, h, w, params, stats, 0, out) == 0, last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(stats).all()) and bool(torch.isfinite(ws).all()) and bool(torch.isfinite(out).all())
    out.fill_(nan)
    assert raw_inverse(2, hdr, n, h, w, None, 0.18, 1.0, out) == 0, last_error()  # mode 2 needs no stats
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())
    out.fill_(nan)
    assert raw_stats(1, sdr, n, h, w, stats, ws, nb) == 0, last_error()
    assert raw_inverse(1, sdr, n, h, w, stats, 0.18, 1.0, out) == 0, last_error()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())


def test_wrapper_input_forms():
    """One image as [h,w,3], a CUDA tensor and non-contiguous inputs give the bits of the numpy batch."""
    t = tm()
    hdr = np.array(K.hdr_batch("2x33x40", seed=900))
    v, cn, cy = K.camera_params(2, seed=12)
    want = host(t.virtual_camera(hdr, v, cn, cy))
    same_bits(host(t.virtual_camera(dev(hdr), v, cn, cy)), want)
    one = t.virtual_camera(hdr[1], v[1], cn[1], cy[1])
    assert tuple(one.shape) == (1, 33, 40, 3)
    same_bits(host(one)[0], want[1])
    wide = np.zeros((2, 66, 80, 4), np.float32)
    wide[:, ::2, ::2, :3] = hdr
    for view in (wide[:, ::2, ::2, :3], dev(wide)[:, ::2, ::2, :3]):
        assert not (view.flags.c_contiguous if isinstance(view, np.ndarray) else view.is_contiguous())
        same_bits(host(t.virtual_camera(view, v, cn, cy)), want)
        same_bits(host(t.log_average(view)), host(t.log_average(hdr)))
    sdr = np.array(K.sdr_batch("2x33x40", seed=950))
    same_bits(host(t.inverse_reinhard(dev(sdr)))[1], host(t.inverse_reinhard(sdr[1]))[0])
    same_bits(host(t.reinhard(hdr.astype(np.float64))), host(t.reinhard(hdr)))


def test_wrapper_refuses_bad_inputs():
    t = tm()
    hdr = np.array(K.hdr_batch("2x33x40", seed=900))
    for fn in (t.reinhard, t.log_average, lambda x: t.virtual_camera(x, 0.0, 0.6, 0.9),
               lambda x: t.inverse_reinhard(x, mode="exact"), lambda x: t.inverse_reinhard(x.astype(np.uint8))):
        with pytest.raises(ValueError):
            fn(hdr[..., :2])
        with pytest.raises(ValueError):
            fn(hdr[None])  # 5-D
    for mode in ("Script", "inverse", None, 1):
        with pytest.raises(ValueError):
            t.inverse_reinhard(hdr, mode=mode)


def test_crop_is_the_scripts_window():
    """imcrop(image, [704 284 511 511]), 1-based: rows 283..794 and columns 703..1214, 0-based."""
    r, c = np.mgrid[0:800, 0:1220]
    ramp = np.stack([r, c, 10000 * r + c], -1).astype(np.int32)
    for img in (ramp, ramp[None], torch.from_numpy(ramp)):
        win = np.asarray(tm().crop(img)).reshape(512, 512, 3)
        np.testing.assert_array_equal(win[..., 0], np.arange(283, 795)[:, None].repeat(512, 1))
        np.testing.assert_array_equal(win[..., 1], np.arange(703, 1215)[None, :].repeat(512, 0))
    assert tm().crop(ramp, top=1, left=2, size=3)[..., 2].tolist() == [[1, 2, 3], [10001, 10002, 10003],
                                                                      [20001, 20002, 20003]]
