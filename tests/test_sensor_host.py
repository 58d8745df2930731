"""Host side of the sensor model (per-channel response, sensor noise) of the HDR pair generator: the
Philox counter convention, the random stream of HDRPairGenerator with the new arguments, their
checks and the C entry points' argument checks.  No GPU."""
import os

import numpy as np
import pytest

import hdrgen_ref as R
import sensor_ref as S
from cnn_itmo_amd import degrade
from cnn_itmo_amd import hdrgen as G
from test_hdrgen import REF_ARGS, flow, same, write_pictures

NOISE = dict(response="channel", noise_shot=(1e-4, 1e-2), noise_read=(1e-4, 1e-2))


# ---- the generator --------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(0, 0), (2 ** 64 - 1, 0x0123456789ABCDEF)])
def test_pure_python_philox_is_numpys(key):
    """Row p of random_raw is philox(counter = p + 1): numpy increments before it generates.  The
    second start makes the counter carry into its second word."""
    for start in (0, 2 ** 64 - 3):
        ctr = [start & S.MASK, start >> 64, 0, 0]
        bg = np.random.Philox(key=np.array(key, np.uint64), counter=np.array(ctr, np.uint64))
        raw = bg.random_raw(4 * 6).reshape(6, 4)
        for p in range(6):
            c = start + p + 1
            want = S.philox4x64_10((c & S.MASK, (c >> 64) & S.MASK, 0, 0), key)
            assert tuple(int(v) for v in raw[p]) == want, (key, start, p)
    # and the table the kernel is held to starts at counter 1
    assert tuple(int(v) for v in S.blocks(key, 3)[2]) == S.philox4x64_10((3, 0, 0, 0), key)
    assert tuple(int(v) for v in S.blocks(key[0], 1)[0]) == S.philox4x64_10((1, 0, 0, 0), (key[0], 0))


def test_reference_normals_are_standard_normals():
    z = S.normals(2 ** 40 + 3, 200, 200)
    assert z.shape == (200, 200, 3) and np.isfinite(z).all()
    # 120000 samples: the mean within 5 sigma / sqrt(N), the variance within 5 sqrt(2 / N)
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.var() - 1) < 5 * np.sqrt(2 / z.size)
    c = np.corrcoef(z.reshape(-1, 3).T)
    assert np.abs(c - np.eye(3)).max() < 5 / np.sqrt(z.size / 3)
    assert not np.array_equal(z, S.normals(2 ** 40 + 4, 200, 200))


def test_quantised_reference_is_stable_under_the_library_interval():
    """Test 5 of the GPU suite allows one level on a share below 1e-3.  The reference itself, moved to
    either end of the interval that the last bits of log / sqrt / sincos leave (sensor_ref.channel_camera's
    shift), changes far fewer levels on inputs like that test's."""
    _, pics, windows, params = S.scene()
    moved = total = 0
    for pic, wd, p, cam, noise in zip(pics, windows, params, S.CAMERAS, S.FRAME_NOISE):
        warped = R.warp(pic, wd, p, 24, 40)  # scipy's warp stands in for the kernel's
        x0, lo, hi = (S.channel_camera(warped, cam, quantize=1, noise=noise, shift=s)[0] for s in (0.0, -1.0, 1.0))
        clean, raw = S.channel_camera(warped, cam, quantize=1)
        print(f"clipped {(raw >= 1).mean():.3f}, levels changed by the noise {(x0 != clean).mean():.3f}")
        assert (raw >= 1).mean() < 0.75 and (x0 != clean).mean() > 0.15  # the frames do show their noise
        moved += int((lo != x0).sum() + (hi != x0).sum())
        total += 2 * x0.size
    print(f"{moved} of {total} levels move")
    assert moved / total < 1e-4


# ---- draws ----------------------------------------------------------------------------------
SIZES = [(37, 53), (41, 47), (30, 64), (64, 64), (25, 41)]


def test_default_arguments_leave_the_draws_alone(tmp_path):
    write_pictures(str(tmp_path), SIZES)
    for extra in (dict(), dict(jpeg_quality=(30, 90), jpeg_prob=0.5), dict(cameras="fixed", jpeg_quality=70)):
        old = flow(tmp_path, gen=G.HDRPairGenerator(**REF_ARGS, **extra), batch_size=2, seed=5)
        new = flow(tmp_path, gen=G.HDRPairGenerator(**REF_ARGS, **extra, response="luminance", noise_shot=None,
                                                    noise_read=None), batch_size=2, seed=5)
        chan = flow(tmp_path, gen=G.HDRPairGenerator(**REF_ARGS, **extra, response="channel"), batch_size=2, seed=5)
        for _ in range(7):
            da = old.next_draws()
            same(da, new.next_draws())
            same(da, chan.next_draws())  # the response alone draws nothing
            assert all(d["noise"] is None for d in da)


@pytest.mark.parametrize("jpeg", [None, (30, 90)])
def test_noise_draws_follow_the_stated_recipe(tmp_path, jpeg):
    write_pictures(str(tmp_path), SIZES)
    kw = dict() if jpeg is None else dict(jpeg_quality=jpeg, jpeg_prob=0.5)
    plain = flow(tmp_path, gen=G.HDRPairGenerator(**REF_ARGS, **kw), batch_size=2, seed=5)
    noisy = flow(tmp_path, gen=G.HDRPairGenerator(**REF_ARGS, **kw, **NOISE), batch_size=2, seed=5)
    half = flow(tmp_path, gen=G.HDRPairGenerator(**REF_ARGS, **kw, response="channel", noise_read=0.002),
                batch_size=2, seed=5)
    rs = np.random.RandomState()
    for seen in range(4):
        dp, dn, dh = plain.next_draws(), noisy.next_draws(), half.next_draws()
        # frame 0 comes before any noise draw: geometry, window, camera and JPEG are those without noise
        for k in ("j", "params", "top", "left", "ch", "cw", "camera", "jpeg"):
            assert dn[0][k] == dp[0][k] == dh[0][k], k
        assert [d["j"] for d in dn] == [d["j"] for d in dp]
        # replay: reseed, the permutation at an epoch start (every third batch), then per frame steps 1-5
        rs.seed(5 + seen)
        if seen % 3 == 0:
            rs.permutation(len(SIZES))
        for d in dn:
            rs.uniform(-90, 90)
            rs.uniform(0.8, 1.2, 2)
            rs.random_sample(), rs.random_sample()
            hs, ws = SIZES[d["j"]]
            rs.randint(0, hs - 24 + 1), rs.randint(0, ws - 40 + 1)
            rs.random_sample()
            for mean in (0.6, 0.9):
                while rs.normal(mean, np.sqrt(0.1)) <= 0:
                    pass
            if jpeg is not None:
                u, q = rs.random_sample(), int(rs.randint(jpeg[0], jpeg[1] + 1))
                assert d["jpeg"] == (q if u < 0.5 else 0)
            a = float(np.exp(np.log(1e-4) + rs.random_sample() * (np.log(1e-2) - np.log(1e-4))))
            b = float(np.exp(np.log(1e-4) + rs.random_sample() * (np.log(1e-2) - np.log(1e-4))))
            k0 = int(rs.randint(0, 2 ** 32)) * 2 ** 32 + int(rs.randint(0, 2 ** 32))
            assert d["noise"] == (a, b, k0)
            assert 1e-4 <= a <= 1e-2 and 1e-4 <= b <= 1e-2 and 0 <= k0 < 2 ** 64
        # floats draw nothing: only the key
        assert all(d["noise"][:2] == (0.0, 0.002) for d in dh)
        rs.seed(5 + seen)
        if seen % 3 == 0:
            rs.permutation(len(SIZES))
        d = dh[0]
        rs.uniform(-90, 90)
        rs.uniform(0.8, 1.2, 2)
        rs.random_sample(), rs.random_sample()
        rs.randint(0, SIZES[d["j"]][0] - 24 + 1), rs.randint(0, SIZES[d["j"]][1] - 40 + 1)
        rs.random_sample()
        for mean in (0.6, 0.9):
            while rs.normal(mean, np.sqrt(0.1)) <= 0:
                pass
        if jpeg is not None:
            rs.random_sample(), rs.randint(jpeg[0], jpeg[1] + 1)
        assert d["noise"][2] == int(rs.randint(0, 2 ** 32)) * 2 ** 32 + int(rs.randint(0, 2 ** 32))


def test_keys_use_all_64_bits(tmp_path):
    write_pictures(str(tmp_path), [(24, 40)] * 4)
    it = flow(tmp_path, gen=G.HDRPairGenerator(**NOISE), batch_size=4, seed=0)
    keys = [d["noise"][2] for _ in range(25) for d in it.next_draws()]
    assert len(set(keys)) == len(keys) and max(keys) >= 2 ** 63 and min(k & 0xFFFFFFFF for k in keys) < 2 ** 31


def test_fixed_cameras_repeat_their_noise(tmp_path):
    write_pictures(str(tmp_path), [(24, 40)] * 5)
    gen = G.HDRPairGenerator(cameras="fixed", jpeg_quality=(30, 90), **NOISE)
    it = flow(tmp_path, gen=gen, batch_size=5, seed=7, shuffle=False, window="full")
    first, second = it.next_draws(), it.next_draws()
    same(first, second)
    lone = flow(tmp_path, gen=G.HDRPairGenerator(cameras="fixed", jpeg_quality=(30, 90)), batch_size=5, seed=7,
                shuffle=False, window="full").next_draws()
    from cnn_itmo_amd import tonemap
    for d, e in zip(first, lone):
        own = np.random.default_rng(7 + d["j"])
        v, n, y = tonemap.virtual_camera_params(1, own)
        assert d["camera"] == (v[0], n[0], y[0]) == e["camera"]
        u, q = own.random(), int(own.integers(30, 91))
        assert d["jpeg"] == q == e["jpeg"] and u < 1.0
        a = float(np.exp(np.log(1e-4) + own.random() * (np.log(1e-2) - np.log(1e-4))))
        b = float(np.exp(np.log(1e-4) + own.random() * (np.log(1e-2) - np.log(1e-4))))
        k0 = int(own.integers(0, 2 ** 32)) * 2 ** 32 + int(own.integers(0, 2 ** 32))
        assert d["noise"] == (a, b, k0) and e["noise"] is None
    assert len({d["noise"][2] for d in first}) == 5


def test_rank_shares_are_slices_of_the_global_batch(tmp_path):
    write_pictures(str(tmp_path), [(30 + k, 50 + k) for k in range(11)])
    gen = G.HDRPairGenerator(**REF_ARGS, **NOISE)
    single = flow(tmp_path, gen=gen, batch_size=4, seed=3, world=1)
    ranks = [flow(tmp_path, gen=gen, batch_size=2, seed=3, rank=r, world=2) for r in range(2)]
    for _ in range(7):
        want = single.next_draws()
        while len(want) < 2:
            want = single.next_draws()
        got = [it.next_draws() for it in ranks]
        same([d for g in got for d in g], want)
        assert all(d["noise"] is not None for d in want)


def test_bad_arguments():
    with pytest.raises(ValueError, match="channel"):
        G.HDRPairGenerator(noise_shot=1e-3)
    with pytest.raises(ValueError, match="channel"):
        G.HDRPairGenerator(response="luminance", noise_read=(1e-4, 1e-3))
    with pytest.raises(ValueError, match="noise_shot"):
        G.HDRPairGenerator(response="channel", noise_shot=(1e-2, 1e-3))  # lo > hi
    with pytest.raises(ValueError, match="noise_read"):
        G.HDRPairGenerator(response="channel", noise_read=(0.0, 1e-3))  # a range needs lo > 0
    with pytest.raises(ValueError, match="noise_read"):
        G.HDRPairGenerator(response="channel", noise_read=-1e-3)
    with pytest.raises(ValueError, match="noise_shot"):
        G.HDRPairGenerator(response="channel", noise_shot=(-1e-3, 1e-3))
    with pytest.raises(ValueError, match="noise_shot"):
        G.HDRPairGenerator(response="channel", noise_shot=float("nan"))
    with pytest.raises(ValueError, match="response"):
        G.HDRPairGenerator(response="rgb")
    g = G.HDRPairGenerator(response="channel", noise_shot=0.0, noise_read=(1e-3, 1e-3))
    assert g.noise == ((0.0, 0.0), (1e-3, 1e-3)) and g.noise_range == (False, True)
    assert G.HDRPairGenerator(response="channel").noise is None
    from cnn_itmo_amd import make_dataset, tonemap
    with pytest.raises(ValueError, match="response"):
        make_dataset.make_dataset("nowhere", response="rgb")
    with pytest.raises(ValueError, match="response"):
        tonemap.virtual_camera(np.ones((2, 2, 3), np.float32), 0, 0.6, 0.9, response="rgb")


def test_noise_keys_and_levels():
    k = degrade.noise_keys(2 ** 64 - 1, 3)
    assert k.dtype == np.uint64 and k.tolist() == [[2 ** 64 - 1, 0]] * 3
    assert degrade.noise_keys([1, 2 ** 40], 2).tolist() == [[1, 0], [2 ** 40, 0]]
    assert degrade.noise_keys([[1, 2], [3, 4]], 2).tolist() == [[1, 2], [3, 4]]
    assert degrade.noise_keys((5, 6), 1, single=True).tolist() == [[5, 6]]
    for bad in (2 ** 64, -1, 1.5, [1, 2, 3], [[1, 2, 3]] * 2):
        with pytest.raises(ValueError, match="key"):
            degrade.noise_keys(bad, 2)
    assert degrade.noise_levels(0.5, [1, 2], 2).tolist() == [[0.5, 1.0], [0.5, 2.0]]
    for shot, read in ((-1, 0), (0, float("inf")), ([1, 2, 3], 0)):
        with pytest.raises(ValueError, match="shot|read"):
            degrade.noise_levels(shot, read, 2)


# ---- the entry points' own checks -------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from cnn_itmo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_entry_points_reject_bad_arguments_without_a_device(lib):
    need = lib.cnnitmo_hdr_pairs_workspace_bytes(4)
    p = 4096  # never dereferenced: every call below fails its argument checks
    good = dict(srcs=p, n=4, h=8, w=8, mats=p, flips=p, lum=None, key=0.18, cam=p, quantize=1, response=1, noise=p,
                keys=p, x=p, y=p, warped=None, logsum=None, ws=p, ws_bytes=need, stream=None)

    def rc(**kw):
        return lib.cnnitmo_hdr_pairs_sensor(*{**good, **kw}.values())

    for name in ("srcs", "mats", "flips", "cam", "x", "y", "ws"):
        assert rc(**{name: None}) == -1, name
        assert b"null" in lib.cnnitmo_last_error()
    assert rc(response=0) == -1  # noise with the luminance response
    assert b"response 1" in lib.cnnitmo_last_error()
    assert rc(keys=None) == -1
    assert b"keys" in lib.cnnitmo_last_error()
    for kw in (dict(response=2), dict(response=-1), dict(noise=p + 4), dict(keys=p + 4), dict(n=0), dict(h=0),
               dict(quantize=4), dict(ws_bytes=need - 1), dict(ws=p + 4), dict(h=1 << 16, w=1 << 15)):
        assert rc(**kw) == -1, kw
    ok = dict(e=p, n=2, h=8, w=8, noise=p, keys=p, out=p + 4096, stream=None)
    for kw in (dict(e=None), dict(noise=None), dict(keys=None), dict(out=None), dict(n=0), dict(h=0), dict(w=-1),
               dict(noise=p + 4), dict(keys=p + 2), dict(e=p + 1), dict(out=p + 2), dict(h=1 << 16, w=1 << 15)):
        assert lib.cnnitmo_sensor_noise(*{**ok, **kw}.values()) == -1, kw
    # the tone-map call: the per-channel flag goes with curve 1 alone
    for curve in (2, 3, 16, 18, 33):
        assert lib.cnnitmo_tonemap_apply(curve, p, 1, 8, 8, None, p, p, 0, p, None) == -1, curve
        assert b"curve" in lib.cnnitmo_last_error()
    assert lib.cnnitmo_tonemap_apply(17, None, 1, 8, 8, None, p, p, 0, p, None) == -1
    assert b"null" in lib.cnnitmo_last_error()  # 17 passes the curve check
