"""GPU RGBE codec (csrc/hdrio.hip), HDR files, ``predict --hdr`` and ``make_dataset`` against the
numpy restatement and the independent file readers / writers of tests/rgbe_ref.py.

The codec is exact by construction (power-of-two scaling and a floor), so every comparison is
bitwise: uint8 bytes for the encoder, fp32 bit patterns for the decoder.  Round-trip bound:
truncation loses less than one mantissa step 2^(e-8) per component and max(r,g,b) >= 2^(e-1), so
x - decode(encode(x)) < 2^-7 * max(r,g,b)."""
import contextlib
import io
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cnn_itmo_amd as C  # noqa: E402
from cnn_itmo_amd import hdrio as H  # noqa: E402
from cnn_itmo_amd import tonemap as T  # noqa: E402
import rgbe_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

# the four-pixel tails and the 256-thread block edges; 801 and 1500 end inside the third and the second
# store of decode's last workgroup (768 output float4 = 1024 pixels each)
NPIX = [1, 3, 4, 5, 255, 256, 257, 1027, 801, 1500]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _encode(x, offset=0):
    """ops.rgbe_encode of x [npix,3]; offset 1: on views one pixel into their buffers, so the input
    is 12 bytes and the output 4 bytes off the 16-byte alignment (the one-pixel path)."""
    from cnn_itmo_amd import ops
    n = x.shape[0]
    src = torch.zeros(n + offset, 3, dtype=torch.float32, device="cuda")
    dst = torch.full((n + offset + 1, 4), 99, dtype=torch.uint8, device="cuda")
    src[offset:] = torch.from_numpy(x)
    assert (src[offset:].data_ptr() % 16 == 0) == (offset == 0)
    ops.rgbe_encode(src[offset:], dst[offset:offset + n])
    out = dst.cpu().numpy()
    assert (out[:offset] == 99).all() and (out[offset + n:] == 99).all()  # nothing written outside
    return out[offset:offset + n]


def _decode(q, offset=0):
    from cnn_itmo_amd import ops
    n = q.shape[0]
    src = torch.zeros(n + offset, 4, dtype=torch.uint8, device="cuda")
    dst = torch.full((n + offset + 1, 3), -7.0, dtype=torch.float32, device="cuda")
    src[offset:] = torch.from_numpy(q)
    ops.rgbe_decode(src[offset:], dst[offset:offset + n])
    out = dst.cpu().numpy()
    assert (out[:offset] == -7).all() and (out[offset + n:] == -7).all()
    return out[offset:offset + n]


def _pixels(npix):
    """random pixels over the whole exponent range, the specials block inside once it fits"""
    x = RR.random_hdr((npix,), seed=npix)
    sp = RR.specials()
    if npix >= 255:
        x[101:101 + len(sp)] = sp
    return x


def _codes(npix):
    """all 256 exponent bytes with random (also non-normalised) mantissas, after the special codes"""
    rng = np.random.default_rng(npix)
    q = rng.integers(0, 256, (max(npix, 8), 4), dtype=np.uint8)
    q[:, 3] = (np.arange(q.shape[0]) * 37 + 5) % 256
    q[:5] = [[255, 255, 255, 255], [1, 2, 3, 0], [255, 255, 255, 0], [255, 1, 128, 1], [0, 0, 1, 1]]
    return q[3:4] if npix == 1 else q[:npix]  # (a single pixel: the E = 1 code)


@pytest.mark.parametrize("npix", NPIX)
def test_encode_bit_equal(npix):
    x = _pixels(npix)
    want = RR.encode(x)
    got = _encode(x)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(1))[:8]
    assert np.array_equal(_encode(x, offset=1), got)


def test_encode_specials():
    x = RR.specials()
    want = RR.encode(x)
    for off in (0, 1):
        got = _encode(x, off)
        assert np.array_equal(got, want), [(x[i], got[i], want[i]) for i in np.flatnonzero((got != want).any(1))]
    assert (want[[0, 1, 2, 3, 5]] == 0).all() and (want[4] == 255).all()  # 0, -1, -0, NaN, -inf black; +inf clamped
    assert (want[6] == 0).all() and want[7, 3] != 0  # 1e-33 black, 1e-32 not
    big = want[(want[:, 3] != 0)]
    assert (big[:, :3].max(1) >= 128).all()  # normalised: the largest mantissa is in 128..255


@pytest.mark.parametrize("npix", NPIX)
def test_decode_bit_equal(npix):
    q = _codes(npix)
    want = RR.decode(q)
    got = _decode(q)
    assert np.array_equal(_bits(got), _bits(want)), np.flatnonzero((_bits(got) != _bits(want)).any(1))[:8]
    assert np.array_equal(_bits(_decode(q, offset=1)), _bits(got))


def test_decode_every_exponent_and_mantissa():
    """256 exponent bytes x 256 mantissas (in the red channel; green and blue follow other orders):
    the whole per-component map, the E = 1 denormals and E = 0 with non-zero mantissas included."""
    E, m = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    q = np.stack([m, 255 - m, (m * 7 + E) % 256, E], -1).reshape(-1, 4).astype(np.uint8)
    want = RR.decode(q)
    got = _decode(q)
    assert np.array_equal(_bits(got), _bits(want))
    assert (got[:256] == 0).all() and got[256 + 255, 0] == np.float32(255 * 2.0 ** -135) and got[256 + 255, 0] > 0
    assert got[-1, 0] == np.float32(255 * 2.0 ** 119)


def test_round_trip():
    x = RR.random_hdr((1027,), seed=11, hi=125)  # inside the RGBE range
    q = _encode(x)
    d = _decode(q)
    assert (d <= x).all()
    err = (x.astype(np.float64) - d) / x.max(-1, keepdims=True)
    print("largest relative truncation error", err.max())
    assert (err < 2.0 ** -7).all()
    assert np.array_equal(_encode(d), q)
    # the public wrappers: numpy or tensor, [h,w,c] or [n,h,w,c]
    img = x[:1000].reshape(2, 20, 25, 3)
    for arg in (img, torch.from_numpy(img).cuda(), img[0]):
        e = H.rgbe_encode(arg)
        assert e.is_cuda and e.dtype == torch.uint8 and tuple(e.shape) == tuple(arg.shape[:-1]) + (4,)
        assert np.array_equal(e.cpu().numpy().reshape(-1, 4), q[:e.numel() // 4])
        b = H.rgbe_decode(e if arg is not img else e.cpu().numpy())
        assert b.is_cuda and b.dtype == torch.float32 and tuple(b.shape) == tuple(arg.shape)
        assert np.array_equal(_bits(b.cpu().numpy().reshape(-1, 3)), _bits(d[:b.numel() // 3]))
    with pytest.raises(ValueError):
        H.rgbe_encode(np.zeros((4, 4), np.float32))


def test_hdr_and_pfm_files(tmp_path):
    x = RR.random_hdr((37, 53), seed=5, lo=-12, hi=12)
    x[3, 4] = 0
    want_q, want = RR.encode(x), RR.decode(RR.encode(x))
    for name, arg in (("a.hdr", x), ("b.pic", torch.from_numpy(x).cuda())):
        p = str(tmp_path / name)
        H.write_image(p, arg)
        back = H.read_image(p)
        assert back.is_cuda and back.dtype == torch.float32 and tuple(back.shape) == (37, 53, 3)
        assert np.array_equal(_bits(back.cpu().numpy()), _bits(want))
        exposure, q = RR.read_hdr(open(p, "rb").read())  # the independent reader opens it
        assert exposure == 1.0 and np.array_equal(q, want_q)
    H.write_hdr(str(tmp_path / "flat.hdr"), x, rle=False)
    assert open(str(tmp_path / "flat.hdr"), "rb").read().endswith(b"-Y 37 +X 53\n" + want_q.tobytes())
    assert np.array_equal(_bits(H.read_hdr(str(tmp_path / "flat.hdr")).cpu().numpy()), _bits(want))
    # a reference-written run-length file with two EXPOSURE lines, stored bottom to top
    p = str(tmp_path / "ref.hdr")
    with open(p, "wb") as fh:
        fh.write(RR.write_hdr(want_q, rle=True, lines=["EXPOSURE=2.0", "EXPOSURE=0.25"], orientation="+Y"))
    plain = H.read_hdr(p)
    scaled, header = H.read_hdr(p, apply_exposure=True, return_header=True)
    assert header["exposure"] == 0.5 and header["width"] == 53
    assert np.array_equal(_bits(plain.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(scaled.cpu().numpy()), _bits(want / np.float32(0.5)))
    # PFM: lossless
    y = x.copy()
    y[0, 0] = [-1.5, np.inf, 1e-45]
    for arg in (y, torch.from_numpy(y).cuda()):
        p = str(tmp_path / "c.pfm")
        H.write_image(p, arg)
        back = H.read_image(p)
        assert back.is_cuda and np.array_equal(_bits(back.cpu().numpy()), _bits(y))
        assert np.array_equal(_bits(RR.read_pfm(open(p, "rb").read())), _bits(y))


# ------------------------------------------------------------------------------ predict --hdr
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """A small saved model (as tests/test_predict_cli.py builds its own), two 32 x 48 PNGs and the
    default run's output."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from PIL import Image
    from cnn_itmo_amd import predict as PR
    d = tmp_path_factory.mktemp("hdrcli")
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        m = C.U_net(input_size=(32, 32, 3), seed=5, verbose=False)
    rng = np.random.default_rng(2)
    m.set_named_weights({k: rng.uniform(0.5, 1.5, v.shape) for k, v in m.named_weights().items()
                         if k.endswith("/moving_variance")})
    ck = str(d / "tiny.hdf5")
    m.save(ck)
    os.makedirs(str(d / "in"))
    frames = [rng.integers(0, 256, (32, 48, 3), dtype=np.uint8) for _ in range(2)]
    for name, f in zip(("first", "second"), frames):
        Image.fromarray(f).save(str(d / "in" / f"{name}.png"))

    def run(out, *extra):
        with contextlib.redirect_stdout(io.StringIO()):
            assert PR.main(["--model", ck, "--input", str(d / "in"), "--output", str(d / out)] + list(extra)) == 0
        return {n: open(str(d / out / n), "rb").read() for n in sorted(os.listdir(str(d / out)))}

    base = run("out0")
    assert sorted(base) == ["first.png", "second.png"]
    return {"dir": d, "ck": ck, "frames": frames, "run": run, "base": base}


def _png(path):
    from PIL import Image
    return np.array(Image.open(path))


def test_predict_hdr_script_mode(cli):
    d = cli["dir"]
    pngs = cli["run"]("out1", "--hdr", str(d / "hdr1"))
    assert pngs == cli["base"]  # the PNGs are byte-identical with and without --hdr
    assert sorted(os.listdir(str(d / "hdr1"))) == ["first.hdr", "second.hdr"]
    for name in ("first", "second"):
        written = _png(str(d / "out1" / f"{name}.png"))
        want = RR.encode(T.inverse_reinhard(written).cpu().numpy()[0])
        _, q = RR.read_hdr(open(str(d / "hdr1" / f"{name}.hdr"), "rb").read())
        assert np.array_equal(q, want)


def test_predict_hdr_exact_mode_pfm_and_tiles(cli):
    from cnn_itmo_amd import predict as PR
    d = cli["dir"]
    flags = ["--hdr-mode", "exact", "--hdr-key", "0.18", "--hdr-log-average", "2.0"]
    pngs = cli["run"]("out2", "--hdr", str(d / "hdr2"), *flags)
    assert pngs == cli["base"]
    m = PR.model_for_size(C.load_model(cli["ck"]), 32, 48)
    if m.optimizer is None:
        m.compile(optimizer="rmsprop", loss="mse", metrics=["accuracy"])
    pred = m.predict(np.stack([PR.to_input(f) for f in cli["frames"]]), batch_size=8)
    assert [PR.to_png(p).tobytes() for p in pred] == [_png(str(d / "out2" / f"{n}.png")).tobytes()
                                                      for n in ("first", "second")]
    want = T.inverse_reinhard(pred, g=2.0, mode="exact").cpu().numpy()
    for i, name in enumerate(("first", "second")):
        _, q = RR.read_hdr(open(str(d / "hdr2" / f"{name}.hdr"), "rb").read())
        assert np.array_equal(q, RR.encode(want[i]))
        assert q[..., 3].min() > 0  # a sigmoid output maps to positive radiance: no black pixel
    # PFM stores the fp32 tensor itself
    pngs = cli["run"]("out3", "--hdr", str(d / "hdr3"), "--hdr-format", "pfm", *flags)
    assert pngs == cli["base"] and sorted(os.listdir(str(d / "hdr3"))) == ["first.pfm", "second.pfm"]
    for i, name in enumerate(("first", "second")):
        got = RR.read_pfm(open(str(d / "hdr3" / f"{name}.pfm"), "rb").read())
        assert np.array_equal(_bits(got), _bits(want[i]))
    # tiled inference gives the same files
    pngs = cli["run"]("out4", "--hdr", str(d / "hdr4"), "--tile", "16,16", *flags)
    assert pngs == cli["base"]
    for name in ("first.hdr", "second.hdr"):
        assert open(str(d / "hdr4" / name), "rb").read() == open(str(d / "hdr2" / name), "rb").read()


# ------------------------------------------------------------------------------ make_dataset
def test_make_dataset(tmp_path):
    from cnn_itmo_amd import datagen as D, make_dataset as MD
    src = tmp_path / "hdr"
    os.makedirs(str(src))
    decoded = {}
    for i, name in enumerate(("b_scene.hdr", "a_scene.hdr")):
        q = RR.encode(RR.random_hdr((40, 56), seed=20 + i, lo=-6, hi=4))
        decoded[name[:-4]] = RR.decode(q)
        with open(str(src / name), "wb") as fh:
            fh.write(RR.write_hdr(q, rle=True))
    open(str(src / "notes.txt"), "w").write("not an image")
    out = tmp_path / "train"
    args = ["--hdr-dir", str(src), "--out", str(out), "--cameras", "2", "--seed", "3"]
    with contextlib.redirect_stdout(io.StringIO()):
        assert MD.main(args) == 0
    names = ["a_scene_0.png", "a_scene_1.png", "b_scene_0.png", "b_scene_1.png"]
    assert sorted(os.listdir(str(out / "input1" / "0"))) == names
    assert sorted(os.listdir(str(out / "output1" / "0"))) == names
    csv1 = open(str(out / "params.csv")).read()
    rows = [r.split(";") for r in csv1.splitlines()]
    assert rows[0] == ["name", "v", "n", "y"] and [r[0] for r in rows[1:]] == names
    inputs, targets = {}, {}
    for fi, stem in enumerate(("a_scene", "b_scene")):  # sorted order: file_index 0, 1
        v, cn, cy = T.virtual_camera_params(2, np.random.default_rng(3 + fi))
        target = T.reinhard(decoded[stem], out_u8=True).cpu().numpy()[0]
        for k in range(2):
            name, sv, sn, sy = rows[1 + 2 * fi + k]
            assert (float(sv), float(sn), float(sy)) == (v[k], cn[k], cy[k])  # repr round-trips
            targets[name] = _png(str(out / "output1" / "0" / name))
            inputs[name] = _png(str(out / "input1" / "0" / name))
            assert np.array_equal(targets[name], target)
            want = T.virtual_camera(decoded[stem], float(sv), float(sn), float(sy), out_u8=True).cpu().numpy()[0]
            assert np.array_equal(inputs[name], want)
        assert not np.array_equal(inputs[f"{stem}_0.png"], inputs[f"{stem}_1.png"])  # two cameras
    # reproducible
    out2 = tmp_path / "train2"
    with contextlib.redirect_stdout(io.StringIO()):
        assert MD.main(args[:3] + [str(out2)] + args[4:]) == 0
    assert open(str(out2 / "params.csv")).read() == csv1
    # the two trees pair up under the reference's seeded generators (main.py:82-100)
    with contextlib.redirect_stdout(io.StringIO()):
        gi = D.ImageDataGenerator().flow_from_directory(str(out / "input1"), target_size=(40, 56), class_mode=None,
                                                        batch_size=4, seed=1, world=1)
        go = D.ImageDataGenerator().flow_from_directory(str(out / "output1"), target_size=(40, 56), class_mode=None,
                                                        batch_size=4, seed=1, world=1)
    xi, yi = next(gi).cpu().numpy(), next(go).cpu().numpy()
    assert xi.shape == (4, 40, 56, 3) and yi.shape == xi.shape
    seen = set()
    for k in range(4):
        match = [n for n in names if np.abs(xi[k] - inputs[n]).max() < 1e-3]
        assert len(match) == 1, match
        assert np.abs(yi[k] - targets[match[0]]).max() < 1e-3
        seen.add(match[0])
    assert seen == set(names)
