"""cnnitmo_hdr_pairs_sensor and cnnitmo_sensor_noise (csrc/hdrpairs.hip, csrc/sensor_px.h) and the
generator's sensor arguments on the GPU against tests/sensor_ref.py.

Tolerances.  (a) normals and the noise law: one fp32 unit, 2^-23 of |e| + sigma |z| (of |z| for the
normals alone): the fp32 cast is half a unit, and the last-bit differences of fp64 log / sqrt / sincos
can move a value across one rounding boundary.  Any error in key, counter, round count or lane mapping
gives unrelated values.  (b) the channel response without noise: rtol 2e-6 against the reference
curve of the GPU's own warped pixels, test_gpu_hdrgen.py's bound for these curves; sanitised values
(0 and 1) exact.  (c) with noise, unquantised: the curve is increasing in e', so the GPU value lies in
[lo (1 - 2e-6), hi (1 + 2e-6)] with lo / hi the reference at e' -+ delta, delta = 16 * 2^-53 *
(e_c + sigma |z_c|): sixteen fp64 units for the five operations whose last bits may differ, with the
factor sqrt(-2 ln u) folded in.  (d) quantised: at most one 8-bit level apart on a share below 1e-3,
bit-equal elsewhere."""
import contextlib
import io

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from cnn_itmo_amd import degrade  # noqa: E402
from cnn_itmo_amd import hdrgen as G  # noqa: E402
import hdrgen_ref as R  # noqa: E402
import sensor_ref as S  # noqa: E402
from arena import Arena, poison_count  # noqa: E402
from test_gpu_hdrgen import (CAMERAS, H, KEY, W, case, launch as launch_plain, source_matrix,  # noqa: E402,F401
                             write_hdr_files)

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -23
NOISE = np.array([f[:2] for f in S.FRAME_NOISE], np.float64)
KEYS = np.array([f[2] for f in S.FRAME_NOISE], np.uint64)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def launch(srcs, windows, mats, flips, cams, quantize=0, response=1, noise=None, keys=None, extras=True, h=H, w=W,
           arena=None):
    """One cnnitmo_hdr_pairs_sensor call, as test_gpu_hdrgen.launch; noise [n,2] float64 and keys [n,2]
    uint64 host arrays or None.  Returns numpy (x, y, warped, logsum) and the device tensors."""
    from cnn_itmo_amd import ops
    n = len(srcs)
    cam = np.array([[KEY * 2.0 ** v, cn, cy] for v, cn, cy in cams], np.float64)
    win = [(t, l, t + ch - 1, l + cw - 1) for t, l, ch, cw in windows]

    def dev(a, dtype, name):
        a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if arena is None:
            return a.cuda()
        return arena.take(a.numel(), dtype, a, name).view(a.shape)

    def out(shape, dtype, name):
        if arena is None:
            return torch.empty(shape, dtype=dtype, device="cuda")
        return arena.take(int(np.prod(shape)), dtype, name=name).view(shape)

    pics = [dev(s, torch.uint8 if str(s.dtype).endswith("uint8") else torch.float32, f"src{i}")
            for i, s in enumerate(srcs)]
    desc = dev(ops.hdr_descriptors(pics, win).view(np.uint8).reshape(-1), torch.uint8, "descriptors")
    dm = dev(np.ascontiguousarray(mats, np.float64), torch.float64, "mats")
    df, dc = dev(np.asarray(flips, np.int32), torch.int32, "flips"), dev(cam, torch.float64, "cam")
    dn = None if noise is None else dev(np.ascontiguousarray(noise, np.float64), torch.float64, "noise")
    dk = None if keys is None else dev(np.ascontiguousarray(keys, np.uint64).view(np.int64), torch.int64, "keys")
    x, y = out((n, h, w, 3), torch.float32, "x"), out((n, h, w, 3), torch.float32, "y")
    warped = out((n, h, w, 3), torch.float32, "warped") if extras else None
    logsum = out((n,), torch.float64, "logsum") if extras else None
    ws = out((ops.hdr_pairs_workspace_bytes(n),), torch.uint8, "workspace")
    ops.hdr_pairs_sensor(desc, dm, df, dc, x, y, key=KEY, quantize=quantize, response=response, noise=dn, keys=dk,
                         warped=warped, logsum=logsum, ws=ws)
    torch.cuda.synchronize()
    res = [t if t is None else t.cpu().numpy() for t in (x, y, warped, logsum)]
    return res, (x, y, warped, logsum)


def same_bits(a, b):
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def scene():
    """sensor_ref.scene (the four-frame case's geometry on pictures whose exposures do not all clip)
    through cnnitmo_hdr_pairs, and through the channel response with FRAME_NOISE, unquantised; once."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert CAMERAS == S.CAMERAS
    srcs, _, windows, params = S.scene(H, W)
    mats, flips = zip(*[source_matrix(p, wd) for p, wd in zip(params, windows)])
    args = (srcs, windows, np.stack(mats), flips, CAMERAS)
    (x, y, warped, logsum), _ = launch_plain(*args)
    (nx, ny, nwarped, nlogsum), _ = launch(*args, noise=NOISE, keys=KEYS)
    return dict(args=args, x=x, y=y, warped=warped, logsum=logsum,
                noisy=dict(x=nx, y=ny, warped=nwarped, logsum=nlogsum))


# ---- 1, 2: the generator and the noise law ------------------------------------------------------
@pytest.mark.parametrize("key", [7, 2 ** 40 + 3, (2 ** 64 - 1, 2 ** 33 + 9)])
@pytest.mark.parametrize("shape", [(H, W), (1, 1)])
def test_normals_match_numpys_philox(key, shape):
    h, w = shape
    got = degrade.sensor_noise(np.zeros((h, w, 3), np.float32), shot=0.0, read=1.0, key=key)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (h, w, 3)
    ref = S.normals(key, h, w).astype(np.float32)
    got = got.cpu().numpy()
    d = np.abs(got.astype(np.float64) - ref) / np.abs(ref)
    print(f"key {key}, {h} x {w}: {int((got != ref).sum())} of {got.size} differ, max {d.max() / ULP32:.3f} units")
    np.testing.assert_allclose(got, ref, rtol=ULP32, atol=0)


def test_noise_law():
    rng = np.random.default_rng(4)
    e = R.radiance(rng, H, W)[None].repeat(3, 0) * np.array([1.0, 0.05, 3.0], np.float32)[:, None, None, None]
    e[1, ::3] *= -1  # negative exposures take the read noise alone
    shot, read, keys = [2e-3, 0.0, 1e-2], [1e-3, 4e-3, 0.0], [11, 2 ** 50 + 1, 2 ** 64 - 2]
    got = degrade.sensor_noise(e, shot, read, keys).cpu().numpy()
    assert (e[1] < 0).any() and (e == 0).any()
    worst = 0.0
    for i in range(3):
        z = S.normals(keys[i], H, W)
        ref = S.noisy(e[i], shot[i], read[i], z)
        scale = np.abs(e[i]) + S.sigma(e[i], shot[i], read[i]) * np.abs(z)
        err = np.abs(got[i] - ref)
        worst = max(worst, float((err[scale > 0] / scale[scale > 0]).max()))
        assert (err <= ULP32 * scale).all(), i
        # a single image, and the image at another place in a batch: the same bits
        same_bits(degrade.sensor_noise(e[i], shot[i], read[i], keys[i]).cpu().numpy(), got[i])
    print(f"noise law: worst error {worst / ULP32:.3f} fp32 units of |e| + sigma |z|")
    assert not np.array_equal(got[0], e[0])
    # no noise at all copies the image
    same_bits(degrade.sensor_noise(e, 0.0, 0.0, 5).cpu().numpy(), e)


# ---- 3: the channel response without noise ---------------------------------------------------
@pytest.mark.parametrize("which", ["case", "scene"])
def test_channel_response_matches_the_reference(case, scene, which):
    """test_gpu_hdrgen.py's four frames (2 % black pixels: most exposures clip), and this file's."""
    case = case if which == "case" else scene
    (x, y, warped, logsum), _ = launch(*case["args"])
    same_bits(warped, case["warped"])
    same_bits(y, case["y"])
    same_bits(logsum, case["logsum"])
    clipped = black = between = 0
    for i in range(4):
        ref, raw = S.channel_camera(warped[i], CAMERAS[i], KEY)
        assert np.isfinite(x[i]).all() and x[i].min() >= 0 and x[i].max() <= 1
        np.testing.assert_allclose(x[i], ref, rtol=2e-6, atol=1e-37)
        fixed = np.isnan(raw) | (raw >= 1) | (raw <= 0)
        np.testing.assert_array_equal(x[i][fixed], ref[fixed])
        clipped += int((raw >= 1).sum())
        black += int((raw <= 0).sum())
        between += int((~fixed).sum())
    print(f"{which}: {clipped} clipped, {black} black, {between} on the curve")
    assert clipped > 0 and black > 0 and between > (5000 if which == "scene" else 0)
    assert not np.array_equal(x, case["x"])  # it is another camera than the luminance one


def flat(rgb, cams, response):
    pic = np.empty((H, W, 3), np.float32)
    pic[:] = np.asarray(rgb, np.float32)
    args = ([pic], [(0, 0, H, W)], [np.array([1.0, 0, 0, 0, 1.0, 0])], [0], cams)
    (x, _, _, _), _ = launch(*args, response=response)
    return x[0], args


def test_grey_is_the_luminance_camera():
    rng = np.random.default_rng(8)
    pic = np.repeat(R.radiance(rng, H, W)[..., :1], 3, axis=-1)
    args = ([pic], [(0, 0, H, W)], [np.array([1.0, 0, 0, 0, 1.0, 0])], [0], CAMERAS[:1])
    (xc, yc, _, _), _ = launch(*args)
    (xl, yl, _, _), _ = launch_plain(*args)
    same_bits(yc, yl)
    assert 0 < (xl < 1).sum() and (xl == 1).any()
    np.testing.assert_allclose(xc, xl, rtol=2e-6, atol=1e-37)


def test_overexposed_red_goes_white():
    cams = [(4.0, 0.6, 0.9)]
    xc, _ = flat((4.0, 1.0, 1.0), cams, response=1)
    xl, args = flat((4.0, 1.0, 1.0), cams, response=0)
    assert (xc == 1.0).all()  # every channel reached full well
    assert (xl[..., 0] == 1.0).all() and (xl[..., 0] > xl[..., 1]).all() and (xl[..., 1] == xl[..., 2]).all()
    (xp, _, _, _), _ = launch_plain(*args)
    same_bits(xl, xp[0])


# ---- 4, 5: with noise ---------------------------------------------------------------------------
def test_noisy_inputs_lie_in_the_reference_interval(scene):
    case, noisy = scene, scene["noisy"]
    assert (case["warped"][0].max(-1) == 0).any()  # a black pixel takes the read noise alone
    same_bits(noisy["warped"], case["warped"])
    same_bits(noisy["y"], case["y"])  # the target carries no noise
    width = 0.0
    for i in range(4):
        # the ends in float64, sanitised as the store does (NaN -> 0, clamp), before the fp32 cast
        lo, hi = (R.sanitise(S.channel_camera(noisy["warped"][i], CAMERAS[i], KEY, noise=S.FRAME_NOISE[i], shift=s)[1])
                  for s in (-1.0, 1.0))
        assert (lo <= hi).all() and (lo < hi).any()
        width = max(width, float((hi - lo).max()))
        got = noisy["x"][i].astype(np.float64)
        assert ((got >= lo * (1 - 2e-6)) & (got <= hi * (1 + 2e-6))).all(), i
        assert (got[hi == 0] == 0).all() and (got[lo == 1] == 1).all()
        clean, _ = S.channel_camera(noisy["warped"][i], CAMERAS[i], KEY)
        assert (np.abs(got - clean) > 1e-4).mean() > 0.15  # and the noise is there
    print(f"largest width of the reference interval: {width:.3e}")


def test_noisy_inputs_quantised(scene):
    case = scene
    (x, y, warped, _), _ = launch(*case["args"], quantize=1, noise=NOISE, keys=KEYS)
    same_bits(warped, case["warped"])
    same_bits(y, case["y"])  # bit-equal to cnnitmo_hdr_pairs' y
    for i in range(4):
        ref, lo, hi = (S.channel_camera(warped[i], CAMERAS[i], KEY, 1, S.FRAME_NOISE[i], shift=s)[0]
                       for s in (0.0, -1.0, 1.0))
        moved = float(((lo != ref) | (hi != ref)).mean())
        assert moved < 1e-3, moved  # the reference itself is stable within the cap
        lv = np.rint(x[i].astype(np.float64) * 255).astype(int)
        np.testing.assert_array_equal(x[i], lv.astype(np.float32) * np.float32(1 / 255.))
        d = np.abs(lv - np.rint(ref.astype(np.float64) * 255).astype(int))
        print(f"frame {i}: {int((d > 0).sum())} of {d.size} levels differ, max {d.max()}; reference share moved "
              f"by the interval {moved:.1e}")
        assert d.max() <= 1 and (d > 0).mean() < 1e-3
        np.testing.assert_array_equal(x[i][d == 0], ref[d == 0])


# ---- 6: bits --------------------------------------------------------------------------------------
def test_luminance_response_is_the_old_entry(case):
    (x, y, warped, logsum), _ = launch(*case["args"], response=0)
    for a, b in ((x, case["x"]), (y, case["y"]), (warped, case["warped"]), (logsum, case["logsum"])):
        same_bits(a, b)
    (xq, yq, _, _), _ = launch(*case["args"], response=0, quantize=3, extras=False)
    (xp, yp, _, _), _ = launch_plain(*case["args"], quantize=3, extras=False)
    same_bits(xq, xp)
    same_bits(yq, yp)


def test_noise_is_reproducible_and_belongs_to_the_frame(scene):
    case, noisy = scene, scene["noisy"]
    (x, y, warped, logsum), _ = launch(*case["args"], noise=NOISE, keys=KEYS)
    for k, v in (("x", x), ("y", y), ("warped", warped), ("logsum", logsum)):
        same_bits(v, noisy[k])
    srcs, windows, mats, flips, cams = case["args"]
    # frame 3 alone: the counter is the pixel's index in its frame
    (x3, y3, _, _), _ = launch(srcs[3:], windows[3:], mats[3:], flips[3:], cams[3:], noise=NOISE[3:], keys=KEYS[3:])
    same_bits(x3[0], noisy["x"][3])
    same_bits(y3[0], noisy["y"][3])
    # another key, another noise; a = b = 0 is the call without noise
    other = KEYS.copy()
    other[3, 0] += np.uint64(1)
    (xo, _, _, _), _ = launch(*case["args"], noise=NOISE, keys=other)
    same_bits(xo[:3], noisy["x"][:3])
    assert (xo[3] != noisy["x"][3]).mean() > 0.2
    quiet = NOISE.copy()
    quiet[1] = 0.0
    (xz, _, _, _), _ = launch(*case["args"], noise=quiet, keys=KEYS)
    (xn, _, _, _), _ = launch(*case["args"])
    same_bits(xz[1], xn[1])
    same_bits(xz[0], noisy["x"][0])
    with pytest.raises(Exception, match="response 1"):
        launch(*case["args"], response=0, noise=NOISE, keys=KEYS)


# ---- 7: arena -------------------------------------------------------------------------------------
def test_operands_only(scene):
    case, noisy = scene, scene["noisy"]
    ar = Arena(40 << 20, "nan", "cuda")
    (x, y, warped, logsum), dev = launch(*case["args"], noise=NOISE, keys=KEYS, arena=ar)
    ar.check_untouched()
    assert all(poison_count(t) == 0 for t in dev)
    for k, v in (("x", x), ("y", y), ("warped", warped), ("logsum", logsum)):
        same_bits(v, noisy[k])


def test_sensor_noise_operands_only():
    from cnn_itmo_amd import ops
    rng = np.random.default_rng(9)
    e = R.radiance(rng, H, W)[None].repeat(2, 0)
    ab, keys = np.array([[1e-3, 2e-3], [0.0, 0.0]]), np.array([[3, 4], [5, 6]], np.uint64)
    ar = Arena(16 << 20, "nan", "cuda")
    de = ar.take(e.size, torch.float32, e, "e").view(e.shape)
    dn = ar.take(4, torch.float64, ab, "noise").view(2, 2)
    dk = ar.take(4, torch.int64, keys.view(np.int64), "keys").view(2, 2)
    out = ar.take(e.size, torch.float32, name="out").view(e.shape)
    ops.sensor_noise(de, dn, dk, out)
    ar.check_untouched()
    assert poison_count(out) == 0
    same_bits(out.cpu().numpy(), degrade.sensor_noise(e, ab[:, 0], ab[:, 1], keys).cpu().numpy())
    same_bits(de.cpu().numpy(), e)


# ---- the tone-map call's curve ----------------------------------------------------------------
def test_virtual_camera_channel_response(case):
    from cnn_itmo_amd import tonemap
    v, n, y = (np.array(c) for c in zip(*CAMERAS))
    got = tonemap.virtual_camera(case["warped"], v, n, y, key=KEY, response="channel").cpu().numpy()
    u8 = tonemap.virtual_camera(case["warped"], v, n, y, key=KEY, response="channel", out_u8=True).cpu().numpy()
    plain = tonemap.virtual_camera(case["warped"], v, n, y, key=KEY).cpu().numpy()
    same_bits(tonemap.virtual_camera(case["warped"], v, n, y, key=KEY, response="luminance").cpu().numpy(), plain)
    for i in range(4):
        ref, raw = S.channel_camera(case["warped"][i], CAMERAS[i], KEY)
        np.testing.assert_allclose(got[i], ref, rtol=2e-6, atol=1e-37)
        d = np.abs(u8[i].astype(int) - np.rint(S.channel_camera(case["warped"][i], CAMERAS[i], KEY, 1)[0]
                                               .astype(np.float64) * 255).astype(int))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3


# ---- 8: the generator -----------------------------------------------------------------------------
def test_generator_batches_are_the_kernel_on_its_draws(tmp_path):
    from cnn_itmo_amd import ops
    write_hdr_files(str(tmp_path), 4, 48, 64, seed=4)
    args = dict(rotation_range=90, horizontal_flip=True, vertical_flip=True, zoom_range=0.2)
    flow = dict(target_size=(32, 40), batch_size=2, seed=1)  # two batches of two frames an epoch
    with contextlib.redirect_stdout(io.StringIO()):
        it = G.HDRPairGenerator(**args, response="channel", noise_shot=(1e-4, 1e-2), noise_read=(1e-4, 1e-2)) \
            .flow_from_directory(str(tmp_path), **flow)
        old = G.HDRPairGenerator(**args).flow_from_directory(str(tmp_path), **flow)
        new = G.HDRPairGenerator(**args, response="luminance", noise_shot=None, noise_read=None) \
            .flow_from_directory(str(tmp_path), **flow)
        jp = G.HDRPairGenerator(**args, response="channel", noise_shot=1e-3, noise_read=(1e-4, 1e-2),
                                jpeg_quality=(30, 90)).flow_from_directory(str(tmp_path), **flow)
    for _ in range(3):
        x, y = next(it)
        draws = it.last_draws
        assert x.is_cuda and tuple(x.shape) == (2, 32, 40, 3) and all(d["noise"] is not None for d in draws)
        have = it._load([d["j"] for d in draws])
        desc = ops.hdr_descriptors([have[d["j"]] for d in draws],
                                   [(d["top"], d["left"], d["top"] + d["ch"] - 1, d["left"] + d["cw"] - 1)
                                    for d in draws])
        mats, flips = zip(*[it.source_matrix(d) for d in draws])
        cam = np.array([[KEY * 2.0 ** d["camera"][0], d["camera"][1], d["camera"][2]] for d in draws])
        noise = np.array([d["noise"][:2] for d in draws])
        keys = np.array([[d["noise"][2], 0] for d in draws], np.uint64)
        xr, yr = torch.empty_like(x), torch.empty_like(y)
        ops.hdr_pairs_sensor(torch.from_numpy(desc.view(np.uint8).reshape(-1)).cuda(),
                             torch.from_numpy(np.stack(mats)).cuda(),
                             torch.from_numpy(np.asarray(flips, np.int32)).cuda(), torch.from_numpy(cam).cuda(), xr, yr,
                             key=KEY, quantize=1, response=1, noise=torch.from_numpy(noise).cuda(),
                             keys=torch.from_numpy(keys.view(np.int64)).cuda())
        assert torch.equal(x, xr) and torch.equal(y, yr)
        # default arguments: today's batches, bit for bit.  Frame 0 is drawn before any noise value, so
        # its target is the same in the noisy stream
        xo, yo = next(old)
        xn, yn = next(new)
        assert torch.equal(xo, xn) and torch.equal(yo, yn)
        assert torch.equal(yo[0], y[0]) and not torch.equal(xo[0], x[0])
        # with JPEG after the noise, x is on the 8-bit levels
        xj, yj = next(jp)
        assert any(d["jpeg"] for d in jp.last_draws) and torch.equal(yj[0], y[0])
        assert torch.equal(torch.round(xj * 255).float() * np.float32(1 / 255.), xj)
