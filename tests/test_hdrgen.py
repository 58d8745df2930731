"""Host side of the HDR pair generator (cnn_itmo_amd/hdrgen.py): the random stream, rank sharding,
windows, cameras, the source matrix and the C entry point's argument checks.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import hdrgen_ref as R
import rgbe_ref as RR
from cnn_itmo_amd import hdrgen as G
from cnn_itmo_amd import hdrio
from cnn_itmo_amd.model import _global_batch
from oracle import augment_ref as A

REF_ARGS = dict(rotation_range=90, horizontal_flip=True, vertical_flip=True, zoom_range=0.2)


def write_pictures(root, sizes, seed=0):
    """Pictures 00.hdr, 01.pfm, 02.hdr, ... of the given (h, w); returns them as the float32 the
    files hold (an RGBE file holds the decoded codes)."""
    rng = np.random.default_rng(seed)
    pics = []
    for k, (h, w) in enumerate(sizes):
        img = R.radiance(rng, h, w)
        if k % 2 == 0:
            q = RR.encode(img)
            with open(os.path.join(root, f"{k:02d}.hdr"), "wb") as fh:
                fh.write(hdrio.format_hdr(q))
            img = RR.decode(q)
        else:
            hdrio.write_pfm(os.path.join(root, f"{k:02d}.pfm"), img)
        pics.append(img)
    return pics


def flow(root, gen=None, **kw):
    gen = gen or G.HDRPairGenerator(**REF_ARGS)
    kw.setdefault("target_size", (24, 40))
    return gen.flow_from_directory(str(root), **kw)


def same(a, b):
    assert len(a) == len(b)
    for p, q in zip(a, b):
        assert p == q, (p, q)


def test_headers_and_sources(tmp_path):
    pics = write_pictures(str(tmp_path), [(37, 53), (41, 29), (24, 40)])
    it = flow(tmp_path, window="full")
    assert [os.path.basename(f) for f in it.filenames] == ["00.hdr", "01.pfm", "02.hdr"]
    assert it.sizes == [(37, 53), (41, 29), (24, 40)]
    q = G.read_source(it.filenames[0])
    assert q.dtype == np.uint8 and q.shape == (37, 53, 4)
    np.testing.assert_array_equal(RR.decode(q), pics[0])
    f = G.read_source(it.filenames[1])
    assert f.dtype == np.float32 and f.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(f, pics[1])


def test_same_seed_same_draws_in_the_stated_order(tmp_path):
    sizes = [(37, 53), (41, 47), (30, 64), (64, 64), (25, 41)]
    write_pictures(str(tmp_path), sizes)
    a, b = flow(tmp_path, batch_size=2, seed=5), flow(tmp_path, batch_size=2, seed=5)
    rs = np.random.RandomState()
    batch_index, perm = 0, None
    for seen in range(7):  # more than two epochs of three batches
        da = a.next_draws()
        same(da, b.next_draws())
        # the stream restated: reseed, permutation at an epoch start, then per frame the transform,
        # the window (top, then left) and the camera (v, n, y)
        rs.seed(5 + seen)
        if batch_index == 0:
            perm = rs.permutation(len(sizes))
        cur = (batch_index * 2) % len(sizes)
        batch_index = batch_index + 1 if len(sizes) > cur + 2 else 0
        idx = perm[cur:cur + 2]
        assert [d["j"] for d in da] == [int(j) for j in idx]
        for d, j in zip(da, idx):
            theta = rs.uniform(-90, 90)
            zx, zy = rs.uniform(1.0 - 0.2, 1.0 + 0.2, 2)
            fh, fv = rs.random_sample() < 0.5, rs.random_sample() < 0.5
            p = d["params"]
            assert (p["theta"], p["zx"], p["zy"], bool(p["flip_horizontal"]), bool(p["flip_vertical"])) == \
                (theta, zx, zy, fh, fv)
            hs, ws = sizes[j]
            top = rs.randint(0, hs - 24 + 1)
            left = rs.randint(0, ws - 40 + 1)
            assert (d["top"], d["left"], d["ch"], d["cw"]) == (top, left, 24, 40)
            v = 8 * rs.random_sample() - 4
            n = rs.normal(0.6, np.sqrt(0.1))
            while n <= 0:
                n = rs.normal(0.6, np.sqrt(0.1))
            y = rs.normal(0.9, np.sqrt(0.1))
            while y <= 0:
                y = rs.normal(0.9, np.sqrt(0.1))
            assert d["camera"] == (v, n, y)


def test_cameras_are_never_singular(tmp_path):
    write_pictures(str(tmp_path), [(24, 40)] * 4)
    it = flow(tmp_path, batch_size=4, seed=0)
    cams = np.array([d["camera"] for _ in range(200) for d in it.next_draws()])
    assert (cams[:, 1] > 0).all() and (cams[:, 2] > 0).all() and (np.abs(cams[:, 0]) <= 4).all()
    # N(0.6, sqrt(0.1)) is negative 2.9 % of the time: 800 draws without a redraw would show it
    assert cams[:, 1].min() < 0.1


@pytest.mark.parametrize("world,files,batch", [(2, 11, 2), (3, 7, 1)])
def test_rank_shards_are_the_global_stream(tmp_path, world, files, batch):
    write_pictures(str(tmp_path), [(30 + k, 50 + k) for k in range(files)])
    single = flow(tmp_path, batch_size=batch * world, seed=3, world=1)
    ranks = [flow(tmp_path, batch_size=batch, seed=3, rank=r, world=world) for r in range(world)]
    for _ in range(3 * len(ranks[0]) + 1):
        want = single.next_draws()
        while len(want) < world:  # a tail too short for every rank is dropped on all of them
            want = single.next_draws()
        got = [it.next_draws() for it in ranks]
        same([d for g in got for d in g], want)
        assert all(len(g) >= 1 for g in got)
        for it in ranks:
            assert it.last_global_batch == len(want) == _global_batch(it)


@pytest.mark.parametrize("window", ["random", "center", "full"])
def test_windows_lie_inside_their_pictures(tmp_path, window):
    sizes = [(24, 40), (37, 53), (64, 41), (25, 90)]
    write_pictures(str(tmp_path), sizes)
    it = flow(tmp_path, window=window, window_size=(24, 37), batch_size=4, seed=1)
    tops = set()
    for _ in range(50):
        for d in it.next_draws():
            hs, ws = sizes[d["j"]]
            assert 0 <= d["top"] and d["top"] + d["ch"] <= hs and 0 <= d["left"] and d["left"] + d["cw"] <= ws
            assert (d["ch"], d["cw"]) == ((hs, ws) if window == "full" else (24, 37))
            if window == "center":
                assert (d["top"], d["left"]) == ((hs - 24) // 2, (ws - 37) // 2)
            if d["j"] == 2:
                tops.add(d["top"])
    if window == "random":  # picture 2 has 41 places for the window's top; 50 draws see many of them
        assert tops <= set(range(41)) and len(tops) > 10
    else:
        assert tops == ({0} if window == "full" else {20})


def test_too_small_file_is_named(tmp_path):
    write_pictures(str(tmp_path), [(37, 53), (23, 53), (37, 53)])
    with pytest.raises(ValueError, match="01.pfm"):
        flow(tmp_path)
    flow(tmp_path, window="full")  # no window to fit
    flow(tmp_path, window_size=(23, 53))


def test_fixed_cameras_are_make_datasets(tmp_path):
    from cnn_itmo_amd import tonemap
    write_pictures(str(tmp_path), [(24, 40)] * 5)
    it = flow(tmp_path, gen=G.HDRPairGenerator(cameras="fixed", **REF_ARGS), batch_size=2, seed=7)
    free = flow(tmp_path, batch_size=2, seed=7)
    for _ in range(6):
        da, de = it.next_draws(), free.next_draws()
        for d, e in zip(da, de):
            v, n, y = tonemap.virtual_camera_params(1, np.random.default_rng(7 + d["j"]))
            assert d["camera"] == (v[0], n[0], y[0])
            assert d["j"] == e["j"]
        # the first frame's transform and window come before any camera draw: the same in both
        assert (da[0]["params"], da[0]["top"], da[0]["left"]) == (de[0]["params"], de[0]["top"], de[0]["left"])
    unshuffled = flow(tmp_path, gen=G.HDRPairGenerator(cameras="fixed"), batch_size=5, seed=7, shuffle=False,
                      window="full")
    same(unshuffled.next_draws(), unshuffled.next_draws())


def test_source_matrix_against_the_trusted_warps(tmp_path):
    pics = write_pictures(str(tmp_path), [(37, 53), (41, 47), (64, 64)])
    h, w = 24, 40
    # window of target size: S is the identity and the warp is keras' apply_transform of the crop
    it = flow(tmp_path, batch_size=3, seed=2)
    for _ in range(3):
        for d in it.next_draws():
            m6, flips = it.source_matrix(d)
            pic = pics[d["j"]]
            win = (d["top"], d["left"], d["top"] + h - 1, d["left"] + w - 1)
            got = R.sample(pic, m6, flips, win, h, w)
            crop = np.ascontiguousarray(pic[d["top"]:d["top"] + h, d["left"]:d["left"] + w])
            ref = A.apply_transform(crop.copy(), d["params"])
            assert np.abs(got - ref).max() <= 2e-6 * np.abs(crop).max()
            np.testing.assert_array_equal(ref, R.warp(pic, (d["top"], d["left"], h, w), d["params"], h, w))
    # resized windows: the whole picture, and a window of another size
    for kw in (dict(window="full"), dict(window="random", window_size=(30, 33))):
        it = flow(tmp_path, batch_size=3, seed=4, **kw)
        for d in it.next_draws():
            m6, flips = it.source_matrix(d)
            pic = pics[d["j"]]
            win = (d["top"], d["left"], d["top"] + d["ch"] - 1, d["left"] + d["cw"] - 1)
            got = R.sample(pic, m6, flips, win, h, w)
            ref = R.warp(pic, (d["top"], d["left"], d["ch"], d["cw"]), d["params"], h, w)
            assert np.abs(got - ref).max() <= 2e-6 * np.abs(pic[win[0]:win[2] + 1, win[1]:win[3] + 1]).max()
    # no transform, window of target size: the matrix is the translation, exactly
    it = flow(tmp_path, gen=G.HDRPairGenerator(), batch_size=3, seed=4, window="center")
    for d in it.next_draws():
        m6, flips = it.source_matrix(d)
        assert flips == 0 and m6.tolist() == [1, 0, d["top"], 0, 1, d["left"]]


@pytest.fixture(scope="module")
def lib():
    from cnn_itmo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_entry_point_rejects_bad_arguments_without_a_device(lib):
    assert lib.cnnitmo_hdr_pairs_workspace_bytes(0) == 0
    need = lib.cnnitmo_hdr_pairs_workspace_bytes(4)
    assert need >= 4 * 8 and lib.cnnitmo_hdr_pairs_workspace_bytes(8) == 2 * need
    p = 4096  # never dereferenced: every call below fails its argument checks
    good = dict(srcs=p, n=4, h=8, w=8, mats=p, flips=p, lum=None, key=0.18, cam=p, quantize=1, x=p, y=p,
                warped=None, logsum=None, ws=p, ws_bytes=need, stream=None)

    def rc(**kw):
        return lib.cnnitmo_hdr_pairs(*{**good, **kw}.values())

    for name in ("srcs", "mats", "flips", "cam", "x", "y", "ws"):
        assert rc(**{name: None}) == -1, name
        assert b"null" in lib.cnnitmo_last_error()
    for kw in (dict(n=0), dict(n=-1), dict(h=0), dict(w=0), dict(n=65536, ws_bytes=1 << 40)):
        assert rc(**kw) == -1, kw
    assert rc(ws_bytes=need - 1) == -1
    assert b"workspace" in lib.cnnitmo_last_error()
    assert rc(ws_bytes=0) == -1
    assert rc(ws=p + 4) == -1
    assert rc(quantize=4) == -1
    assert rc(h=1 << 16, w=1 << 15) == -1  # h * w = 2^31


def test_descriptor_checks(lib):
    torch = pytest.importorskip("torch")
    from cnn_itmo_amd import ops
    assert ops.HDR_SRC.itemsize == 40 and ctypes.sizeof(ctypes.c_void_p) == 8
    f = torch.zeros(5, 7, 3)
    q = torch.zeros(6, 4, 4, dtype=torch.uint8)
    d = ops.hdr_descriptors([f, q], [None, (1, 0, 5, 2)])
    assert d["pix"].tolist() == [f.data_ptr(), q.data_ptr()]
    assert [d[k].tolist() for k in ("h", "w", "fmt", "r0", "c0", "r1", "c1")] == \
        [[5, 6], [7, 4], [0, 1], [0, 1], [0, 0], [4, 5], [6, 2]]
    for bad in ((0, 0, 5, 6), (0, 0, 4, 7), (-1, 0, 4, 6), (3, 0, 2, 6)):
        with pytest.raises(ValueError, match="window"):
            ops.hdr_descriptors([f], [bad])
    with pytest.raises(ValueError, match="source 0"):
        ops.hdr_descriptors([torch.zeros(5, 7, 4)])
