"""Shapes at which the persistent kernels WALK: every workgroup that owns anything owns at least
three items of its range (host only: no torch, no GPU; the library's host-only queries).

The per-kernel lists of kernel_cases.py are sized for a single tile: with 85 - 256 streams and at
most 24 tiles every halo workgroup computes zero or one, the weight gradient's ring never reaches
its steady state, and nothing carried from item to item (ring slots and per-wave vmcnt
bookkeeping, the prefetch position running ahead of the compute position, BN partial sums kept in
registers for the whole launch, the y wrap at an image boundary) is exercised.  The lists here are
sized the other way round, and the helpers PROVE the work split of each case from the library's
queries and the index arithmetic the kernels' header comments state (restated next to each
helper), asserting:

(a) share        every workgroup (stream, group) that owns anything owns >= 3 items; somewhere in
                 each family a workgroup owns nothing where the split allows it (halo: the
                 leftover workgroups of a grid that the column blocks do not divide; tconv_stream:
                 the groups past the last tile);
(b) halo         some range contains each transition (next tile row of a strip, next column strip,
                 next image), over frames whose last tile row and last tile column are partial;
(c) wgrad_halo   every range spans two images and is at least 14 rows (twice the largest ring of
                 D + R + 2 <= 7 slots) whatever occupancy the runtime reports; the R = 2 blocks see
                 an odd and an even row count; both strip widths have a partial last strip;
(d) tconv_stream some range contains each transition (next tile of a row, next row, next image),
                 and the last tile of a row is partial;
(e) names        every case names the kernel it is there for (kernel_cases.expect_kernels).

test_walk_cases_host.py checks all of this without a GPU, and that every halo_conv / tconv_stream /
wgrad_halo name reachable in the documented domain (kernel_cases.reachable) is the name of a case
here; test_gpu_walk.py launches the cases.  Names and splits are those of an MI355X (256 CUs),
which the planners also assume without a device.
"""
from tests import kernel_cases as KC

DT = KC.DT
_s = KC._s

# ---- halo_conv_kernel ----------------------------------------------------------------------------
# conv_halo.hip: a workgroup owns a TH x TW = 16 x 32 output tile and a block of BN columns; logical
# ids form `streams` groups of nblocks = columns / BN workgroups; stream gs walks the tiles
#   [tiles * gs / streams, tiles * (gs + 1) / streams),  tiles = N * ceil(H / 16) * ceil(W / 32),
# tile -> (image, column strip, tile row), tile rows fastest; one BN partial-sum row per
# (stream, wave), NWAVE = 8 waves.  The grid is one workgroup per CU; workgroups with
# gs >= streams (fewer than nblocks of them) own nothing.
TH, TW, NWAVE = 16, 32, 8
HALO_H = 24  # a whole and a half tile row: any three consecutive tiles hold a row and a strip step

# (op, dtype, N, W, cin, cout, extra) -> kernel name.  cin / cout are the LAYER's (the input gradients
# have K = cout and cin columns).  extra: (c0, c1, parity) of the fused BN backward, else None.
# W is chosen per stream count S so that tiles >= 3 S: 4100 (S = 256), 2060 (128), 1370 (85),
# 1030 (64), 520 (32); 8200: six tiles per stream; 51 streams (five blocks): N = 4 and W = 630, since
# three images over 3 x 17 streams put every image boundary on a range boundary.  Every W % 32 != 0.
HALO = {
    # -- training forward (ReLU + BN sums), cnnitmo_conv3x3_fwd
    ("fwd", "bf16", 3, 8200, 32, 32, None): "halo_conv_kernel<32,1,wres>",
    ("fwd", "bf16", 3, 4100, 32, 64, None): "halo_conv_kernel<64,1,wres>",
    ("fwd", "bf16", 3, 2060, 64, 128, None): "halo_conv_kernel<64,1,wres>",    # two column blocks
    ("fwd", "bf16", 3, 1030, 128, 256, None): "halo_conv_kernel<64,1>",         # four, streamed weights
    ("fwd", "bf16", 3, 520, 256, 512, None): "halo_conv_kernel<64,1>",          # eight
    ("fwd", "bf16", 3, 1370, 128, 96, None): "halo_conv_kernel<32,1>",          # three: 85 streams, one workgroup left over
    ("fwd", "bf16", 3, 8200, 96, 32, None): "halo_conv_kernel<32,1>",
    ("fwd", "f32", 3, 8200, 32, 32, None): "halo_conv_kernel<f32,32,1,wres>",
    ("fwd", "f32", 3, 4100, 32, 64, None): "halo_conv_kernel<f32,64,1,wres>",
    ("fwd", "f32", 3, 2060, 64, 128, None): "halo_conv_kernel<f32,64,1>",
    ("fwd", "f32", 3, 1370, 128, 96, None): "halo_conv_kernel<f32,32,1>",
    # -- input gradient, cnnitmo_conv3x3_dgrad (K = cout; resident weights up to 64 bf16 / 32 fp32)
    ("dgrad", "bf16", 3, 4100, 32, 32, None): "halo_conv_kernel<32,0,wres>",
    ("dgrad", "bf16", 3, 4100, 32, 96, None): "halo_conv_kernel<32,0>",
    ("dgrad", "bf16", 3, 4100, 64, 32, None): "halo_conv_kernel<64,0,wres>",
    ("dgrad", "bf16", 3, 4100, 64, 96, None): "halo_conv_kernel<64,0>",
    ("dgrad", "bf16", 3, 1370, 96, 32, None): "halo_conv_kernel<32,0,wres>",    # three blocks, one workgroup left over
    ("dgrad", "f32", 3, 4100, 32, 32, None): "halo_conv_kernel<f32,32,0,wres>",
    ("dgrad", "f32", 3, 4100, 32, 64, None): "halo_conv_kernel<f32,32,0>",
    ("dgrad", "f32", 3, 4100, 64, 32, None): "halo_conv_kernel<f32,64,0,wres>",
    ("dgrad", "f32", 3, 4100, 64, 64, None): "halo_conv_kernel<f32,64,0>",
    # -- input gradient with the producer's BN backward fused, cnnitmo_conv3x3_dgrad_bn; the three
    #    store paths of kernel_cases.DGRAD_BN_BRANCH are among them (HALO_BRANCH below)
    ("dgrad_bn", "bf16", 3, 4100, 32, 32, (0, 32, False)): "halo_conv_kernel<32,2,wres>",      # all
    ("dgrad_bn", "bf16", 4, 630, 160, 128, (32, 160, True)): "halo_conv_kernel<32,2>",         # mixed, five blocks
    ("dgrad_bn", "bf16", 4, 630, 160, 64, (32, 160, True)): "halo_conv_kernel<32,2,wres>",     # neither
    ("dgrad_bn", "bf16", 3, 4100, 64, 32, (0, 64, False)): "halo_conv_kernel<64,2,wres>",
    ("dgrad_bn", "bf16", 3, 1370, 192, 128, (64, 192, True)): "halo_conv_kernel<64,2>",        # mixed, 64-column blocks
    ("dgrad_bn", "f32", 3, 4100, 32, 32, (0, 32, False)): "halo_conv_kernel<f32,32,2,wres>",
    ("dgrad_bn", "f32", 3, 4100, 32, 64, (0, 32, False)): "halo_conv_kernel<f32,32,2>",
    ("dgrad_bn", "f32", 4, 630, 160, 128, (32, 160, True)): "halo_conv_kernel<f32,32,2>",      # neither (fp32 has no mixed form)
    ("dgrad_bn", "f32", 3, 4100, 64, 32, (0, 64, False)): "halo_conv_kernel<f32,64,2,wres>",
    ("dgrad_bn", "f32", 3, 4100, 64, 64, (0, 64, True)): "halo_conv_kernel<f32,64,2>",
    # -- ... with the deferred MaxPooling2D gradient routed in, cnnitmo_conv3x3_dgrad_bn_pooled
    ("dgrad_bn_pooled", "bf16", 3, 4100, 32, 32, None): "halo_conv_kernel<32,2,wres,route>",
    ("dgrad_bn_pooled", "bf16", 3, 4100, 32, 96, None): "halo_conv_kernel<32,2,route>",
    ("dgrad_bn_pooled", "f32", 3, 4100, 32, 32, None): "halo_conv_kernel<f32,32,2,wres,route>",
    ("dgrad_bn_pooled", "f32", 3, 4100, 32, 64, None): "halo_conv_kernel<f32,32,2,route>",
    # -- forms the name queries do not enumerate: the name is the plain forward's, the form is the op
    # pooled forward, training (STATS) and inference (AFFINE, no sums): ",pool"
    ("fwd_pool", "bf16", 3, 4100, 32, 32, None): "halo_conv_kernel<32,1,wres>",
    ("fwd_pool", "f32", 3, 4100, 32, 32, None): "halo_conv_kernel<f32,32,1,wres>",
    ("fwd_pool_affine", "bf16", 3, 4100, 32, 64, None): "halo_conv_kernel<64,1,wres>",
    ("fwd_pool_affine", "f32", 3, 4100, 32, 64, None): "halo_conv_kernel<f32,64,1,wres>",
    # the sigmoid head in the epilogue (EPI 3), one 64-column block
    ("fwd_head", "bf16", 3, 4100, 64, 64, None): "halo_conv_kernel<64,1,wres>",
    ("fwd_head", "f32", 3, 4100, 64, 64, None): "halo_conv_kernel<f32,64,1>",
    # two sources [32 | 64] -> 64 (bf16 only), cnnitmo_conv3x3_fwd_cat
    ("fwd_cat", "bf16", 3, 4100, 96, 64, None): "halo_conv_kernel<64,1>",
    # inference forward without sums (NOSUM), both block widths
    ("fwd_nosum", "bf16", 3, 4100, 32, 32, None): "halo_conv_kernel<32,1,wres>",
    ("fwd_nosum", "bf16", 3, 4100, 32, 64, None): "halo_conv_kernel<64,1,wres>",
    ("fwd_nosum", "f32", 3, 4100, 32, 32, None): "halo_conv_kernel<f32,32,1,wres>",
    ("fwd_nosum", "f32", 3, 4100, 32, 64, None): "halo_conv_kernel<f32,64,1,wres>",
}
HALO_FWD_OPS = ("fwd", "fwd_pool", "fwd_pool_affine", "fwd_head", "fwd_cat", "fwd_nosum")
HALO_FORMS = ("fwd_pool", "fwd_pool_affine", "fwd_head", "fwd_cat", "fwd_nosum")
# the store path of each fused dgrad of kernel_cases.DGRAD_BN_BRANCH: (cin, cout, c0, c1, dtype) -> W of its case
HALO_BRANCH = {(32, 32, 0, 32, "bf16"): 4100, (160, 128, 32, 160, "bf16"): 630, (160, 64, 32, 160, "bf16"): 630,
               (160, 128, 32, 160, "f32"): 630}


def halo_name(q, case, h=HALO_H):
    """The kernel the planner chooses for a halo case ('' where a form is not supported)."""
    op, dt, n, w, cin, cout, extra = case
    d = DT[dt]
    if op == "dgrad":
        return _s(q("cnnitmo_conv3x3_kernel_name", d, n, h, w, cin, cout, 1))
    if op == "dgrad_bn":
        return KC.dgrad_bn_name(q, dt, cin, cout, h, w, extra[0], extra[1], n)
    if op == "dgrad_bn_pooled":
        return KC.dgrad_bn_pooled_name(q, dt, cin, cout, h, w, n)
    ok = {"fwd_pool": lambda: q("cnnitmo_conv3x3_pool_supported", d, n, h, w, cin, cout),
          "fwd_pool_affine": lambda: q("cnnitmo_conv3x3_pool_supported", d, n, h, w, cin, cout),
          "fwd_head": lambda: q("cnnitmo_conv3x3_head_supported", d, n, h, w, cin, cout),
          "fwd_cat": lambda: q("cnnitmo_conv3x3_fwd_cat_supported", d, n, h, w, 32, cin, cout)}.get(op, lambda: 1)()
    return _s(q("cnnitmo_conv3x3_kernel_name", d, n, h, w, cin, cout, 0)) if ok == 1 else ""


def name_bn(name):
    """The block width of a halo_conv_kernel / tconv_stream_kernel name (its first integer argument
    after the dtype / the mode)."""
    args = name.split("<")[1].rstrip(">").split(",")
    return int(args[1]) if name.startswith(("tconv_stream", "halo_conv_kernel<f32")) else int(args[0])


def halo_grid(q):
    """Workgroups of a halo launch (one per CU): the streams of a one-block launch."""
    return q("cnnitmo_conv3x3_stat_rows", DT["bf16"], 1, TH, TW, 32, 32) // NWAVE


def halo_split(q, case, h=HALO_H):
    """The split of a halo case: streams (from the rows query where one exists, cross-checked with
    grid // nblocks), the frame's tiles, each stream's range, the workgroups that own nothing."""
    op, dt, n, w, cin, cout, extra = case
    d = DT[dt]
    name = halo_name(q, case, h)
    assert name, f"{case}: the halo kernel does not take this shape"
    bn = name_bn(name)
    cols = cout if op in HALO_FWD_OPS else cin
    nblocks = cols // bn
    grid = halo_grid(q)
    streams = grid // nblocks
    if op in HALO_FWD_OPS:
        rows = q("cnnitmo_conv3x3_stat_rows", d, n, h, w, cin, cout)
    elif op == "dgrad_bn":
        rows = q("cnnitmo_conv3x3_dgrad_bn_rows", d, n, h, w, cout, cin, extra[0], extra[1])
    elif op == "dgrad_bn_pooled":
        rows = q("cnnitmo_conv3x3_dgrad_bn_pooled_rows", d, n, h, w, cout, cin)
    else:
        rows = None  # the plain input gradient writes no sums: no query
    if rows is not None:
        assert rows == streams * NWAVE, f"{case}: {rows} sums rows, {grid} // {nblocks} streams of {NWAVE} waves"
    ty, tx = -(-h // TH), -(-w // TW)
    tiles = n * ty * tx
    ranges = [(tiles * gs // streams, tiles * (gs + 1) // streams) for gs in range(streams)]
    return dict(name=name, bn=bn, nblocks=nblocks, grid=grid, streams=streams, rows=rows, tiles_x=tx, tiles_y=ty,
                tiles=tiles, ranges=ranges, idle=grid - streams * nblocks, per_stream=tiles / streams)


def halo_transitions(sp, t0, t1):
    """The kinds of step between consecutive tiles of [t0, t1): step() of conv_halo.hip."""
    tpi, ty = sp["tiles_x"] * sp["tiles_y"], sp["tiles_y"]
    kinds = set()
    for t in range(t0, t1 - 1):
        a, b = divmod(t, tpi), divmod(t + 1, tpi)
        if a[0] != b[0]:
            kinds.add("image")
        elif a[1] // ty != b[1] // ty:
            kinds.add("strip")
        else:
            kinds.add("row")
    return kinds


def check_halo(q, case, h=HALO_H):
    """Conditions (a), (b) and (e) of one halo case; returns its split."""
    KC.expect_kernels(halo_name(q, case, h), HALO[case])
    sp = halo_split(q, case, h)
    n, w = case[2], case[3]
    share = min(t1 - t0 for t0, t1 in sp["ranges"])
    assert share >= 3, f"{case}: a stream owns {share} tiles ({sp['tiles']} over {sp['streams']} streams)"
    assert h % TH and w % TW, f"{case}: the last tile row / column of {h} x {w} is whole"
    assert sp["tiles_x"] > 1 and sp["tiles_y"] > 1 and n > 1
    seen = set()
    for t0, t1 in sp["ranges"]:
        seen |= halo_transitions(sp, t0, t1)
    assert seen == {"row", "strip", "image"}, f"{case}: no range crosses {({'row', 'strip', 'image'} - seen)}"
    return sp


# ---- tconv_stream_kernel -------------------------------------------------------------------------
# tconv_stream.hip: 64-pixel tiles, image -> row -> 64-pixel strip, ntiles = N * H * ceil(W / 64);
# every launch has ONE column block (ts_plan: N == BN), so its G = grid groups are its workgroups;
# group g owns [g * per, min((g + 1) * per, ntiles)), per = ceil(ntiles / G); a group without
# tiles zeroes its sums rows.  One sums row per (group, wave row): WM = 2 for BN >= 128, else
# 8 / (BN / 32).
TS_N, TS_H, TS_W, TS_TW = 3, 37, 300, 64
# (op, cin, cout) -> name (bf16 only).  op: the forward (ReLU + BN sums), the input gradient, the
# input gradient with the producer's BN backward fused
TCONV = {
    ("fwd", 128, 64): "tconv_stream_kernel<0,256>",
    ("fwd", 256, 32): "tconv_stream_kernel<0,128>",
    ("dgrad", 128, 64): "tconv_stream_kernel<1,128>",
    ("dgrad", 256, 32): "tconv_stream_kernel<1,256>",
    ("dgrad", 64, 32): "tconv_stream_kernel<1,64>",
    ("dgrad_bn", 128, 64): "tconv_stream_kernel<1,128,bnb>",
    ("dgrad_bn", 64, 32): "tconv_stream_kernel<1,64,bnb>",
}


def tconv_name(q, case, n=TS_N, h=TS_H, w=TS_W):
    op, cin, cout = case
    if op == "dgrad_bn":
        return KC.tconv_dgrad_bn_name(q, "bf16", cin, cout, h, w, n)
    return KC.tconv_names(q, "bf16", cin, cout, h, w, n)[0 if op == "fwd" else 1]


def ts_wm(bn):
    return 2 if bn >= 128 else 8 // (bn // 32)


def tconv_split(q, case, n=TS_N, h=TS_H, w=TS_W):
    op, cin, cout = case
    name = tconv_name(q, case, n, h, w)
    assert name.startswith("tconv_stream_kernel"), f"{case}: {name}"
    bn = name_bn(name)
    d = DT["bf16"]
    # groups of a one-block stream launch: the forward's rows query over its WM (BN = 256: WM = 2)
    g_any = q("cnnitmo_tconv2x2_stat_rows", d, n, h, w, 128, 64) // ts_wm(256)
    if op == "fwd":
        rows = q("cnnitmo_tconv2x2_stat_rows", d, n, h, w, cin, cout)
    elif op == "dgrad_bn":
        rows = q("cnnitmo_tconv2x2_dgrad_bn_rows", d, n, h, w, cout, cin)
    else:
        rows = None
    groups = rows // ts_wm(bn) if rows is not None else g_any
    assert groups == g_any and (rows is None or rows == groups * ts_wm(bn)), (case, rows, groups, g_any)
    tx = -(-w // TS_TW)
    ntiles = n * h * tx
    per = -(-ntiles // groups)
    ranges = [(min(g * per, ntiles), min((g + 1) * per, ntiles)) for g in range(groups)]
    return dict(name=name, bn=bn, wm=ts_wm(bn), rows=rows, groups=groups, tiles_x=tx, ntiles=ntiles, per=per,
                ranges=ranges, idle=sum(1 for a, b in ranges if a == b))


def check_tconv(q, case, n=TS_N, h=TS_H, w=TS_W):
    """Conditions (a), (d) and (e) of one tconv_stream case; returns its split."""
    KC.expect_kernels(tconv_name(q, case, n, h, w), TCONV[case])
    sp = tconv_split(q, case, n, h, w)
    own = [b - a for a, b in sp["ranges"] if b > a]
    assert min(own) >= 3, f"{case}: a group owns {min(own)} tiles (per = {sp['per']}, {sp['ntiles']} tiles)"
    assert sp["idle"] >= 1, f"{case}: no group without tiles"
    assert w % TS_TW and sp["tiles_x"] > 1, f"{case}: the last tile of a row is whole"
    seen = set()
    tx = sp["tiles_x"]
    for a, b in sp["ranges"]:
        for t in range(a, b - 1):
            ra, rb = t // tx, (t + 1) // tx
            seen.add("tile" if ra == rb else ("image" if ra // h != rb // h else "row"))
    assert seen == {"tile", "row", "image"}, f"{case}: no range crosses {({'tile', 'row', 'image'} - seen)}"
    return sp


# ---- wgrad_halo_kernel (bf16 and fp32) -----------------------------------------------------------
# wgrad_halo.hip: workgroup (strip, row split rs) walks the global rows [rs * rows_per, (rs + 1) *
# rows_per) of the N * H (image, row) rows down one TW-pixel strip, through a ring of at most
# D + R + 2 <= 7 row slots, R = 2 rows per step for the 64 x 64 / 96 / 128 blocks; rows above and
# below an image read a zero row, chosen by the row index y that wraps at H.  wh_plan picks the row
# split rs <= 64 with the least idle tail over slots = CUs x (workgroups per CU), the latter from
# the runtime: restated below for 1 - 4 workgroups per CU, and the conditions hold for each.
WG_N, WG_H = 75, 13  # 975 rows: 64 ranges of 16 rows, the last of 15
# (dtype, W, cin, cout, cat) -> name; cat: the two-source [32 | cin - 32] form, cnnitmo_conv_wgrad_cat
WGRAD = {
    ("bf16", 70, 32, 32, False): "wgrad_halo_kernel<32,32,64>",
    ("bf16", 192, 32, 32, False): "wgrad_halo_kernel<32,32,128>",
    ("bf16", 70, 64, 32, False): "wgrad_halo_kernel<32,64,64>",
    ("bf16", 192, 64, 32, False): "wgrad_halo_kernel<32,64,128>",
    ("bf16", 70, 96, 32, False): "wgrad_halo_kernel<32,96,64>",
    ("bf16", 70, 32, 64, False): "wgrad_halo_kernel<64,32,64>",
    ("bf16", 192, 32, 64, False): "wgrad_halo_kernel<64,32,128>",
    ("bf16", 70, 64, 64, False): "wgrad_halo_kernel<64,64,64>",
    ("bf16", 70, 96, 64, False): "wgrad_halo_kernel<64,96,64>",
    ("bf16", 70, 128, 64, False): "wgrad_halo_kernel<64,128,64>",
    ("bf16", 70, 192, 64, False): "wgrad_halo_kernel<64,128+64,64>",
    ("bf16", 70, 96, 64, True): "wgrad_halo_kernel<64,96,64,cat>",
    ("bf16", 70, 96, 32, True): "wgrad_halo_kernel<32,96,64,cat>",
    ("f32", 70, 32, 32, False): "wgrad_halo_kernel<f32,32,32,64>",
    ("f32", 70, 64, 32, False): "wgrad_halo_kernel<f32,32,64,64>",
    ("f32", 70, 32, 64, False): "wgrad_halo_kernel<f32,64,32,64>",
    ("f32", 70, 64, 64, False): "wgrad_halo_kernel<f32,64,64,64>",
    ("f32", 70, 96, 64, False): "wgrad_halo_kernel<f32,64,96,64>",
}
WG_OCC = (1, 2, 3, 4)  # workgroups per CU the runtime may report
WG_RING = 7            # D + R + 2 row slots at most


def wgrad_name(q, case, n=WG_N, h=WG_H):
    dt, w, cin, cout, cat = case
    if cat:
        return _s(q("cnnitmo_wgrad_cat_kernel_name", n, h, w, 32, cin, cout))
    return _s(q("cnnitmo_wgrad_kernel_name", DT[dt], 9, n, h, w, cin, cout))


def wgrad_block(name):
    """(BM, BN, TW, one launch per column block?) of a wgrad_halo_kernel name."""
    a = name.split("<")[1].rstrip(">").split(",")
    a = [v for v in a if v not in ("f32", "cat")]
    return int(a[0]), (128 if a[1] == "128+64" else int(a[1])), int(a[2]), a[1] == "128+64"


def wgrad_rows2(name):
    """R = 2 rows per step: the bf16 64 x 64 / 96 / 128 blocks (wh_rows); the fp32 kernel steps one row."""
    bm, bn, _, _ = wgrad_block(name)
    return "f32" not in name and bm == 64 and bn >= 64


def wgrad_splits(q, case, n=WG_N, h=WG_H):
    """{workgroups per CU: (rows_per, [ranges])}: wh_plan's row split restated for each occupancy."""
    dt, w, cin, cout, cat = case
    name = wgrad_name(q, case, n, h)
    assert name.startswith("wgrad_halo_kernel"), f"{case}: {name}"
    bm, bn, tw, split = wgrad_block(name)
    strips = -(-w // tw)
    per = strips * (cout // bm) * (1 if split else cin // bn)
    rows = n * h
    cus = halo_grid(q)  # one halo workgroup per CU
    out = {}
    for occ in WG_OCC:
        slots = cus * occ
        best, best_eff = 1, -1.0
        for rs in range(1, min(64, rows) + 1):
            blocks = per * rs
            eff = blocks / (-(-blocks // slots) * slots)
            if blocks < slots // 2:
                eff *= 0.5
            if eff > best_eff + 1e-3:
                best_eff, best = eff, rs
        rows_per = -(-rows // best)
        rsplits = -(-rows // rows_per)
        out[occ] = (rows_per, [(r * rows_per, min((r + 1) * rows_per, rows)) for r in range(rsplits)])
    return dict(name=name, tw=tw, strips=strips, rows=rows, plans=out)


def check_wgrad(q, case, n=WG_N, h=WG_H):
    """Conditions (a), (c) and (e) of one wgrad_halo case; returns its splits."""
    KC.expect_kernels(wgrad_name(q, case, n, h), WGRAD[case])
    sp = wgrad_splits(q, case, n, h)
    assert n * h > 64 * h, "the planner splits rows at most 64 ways: rows_per > H needs N > 64"
    assert case[1] % sp["tw"], f"{case}: the last {sp['tw']}-pixel strip is whole"
    for occ, (rows_per, ranges) in sp["plans"].items():
        for g0, g1 in ranges:
            assert g1 - g0 >= 2 * WG_RING, f"{case}, {occ} per CU: {g1 - g0} rows do not lap a ring of {WG_RING} twice"
            assert g0 // h != (g1 - 1) // h, f"{case}, {occ} per CU: rows [{g0}, {g1}) lie in one image"
    return sp


def wgrad_parities(q, n=WG_N, h=WG_H):
    """{workgroups per CU: the set of row-count parities the R = 2 cases walk}."""
    out = {occ: set() for occ in WG_OCC}
    for case, name in WGRAD.items():
        if wgrad_rows2(name):
            for occ, (_, ranges) in wgrad_splits(q, case, n, h)["plans"].items():
                out[occ] |= {(g1 - g0) & 1 for g0, g1 in ranges}
    return out


# ---- conv_c3 (the 3-channel first layer) -----------------------------------------------------------
# conv_c3.hip: persistent workgroup b takes units b, b + G, ...  Forward: a unit is RPB = 4 output
# rows x SEG = 256 pixels, G = cnnitmo_conv_c3_stat_rows = min(units, grid).  Weight gradient: a
# unit is one row x 256 pixels over G = min(units, workspace slabs of 4 KiB) workgroups at most
# (the fp32 kernel launches fewer: a longer walk).
C3_RPB, C3_SEG = 4, 256
# (op, dtype) -> (N, h_valid, H, W): the forward needs 3 x 768 units of at most 4 x 256 pixels
C3 = {
    ("fwd", "bf16"): (3, 7, 9, 65320),
    ("fwd", "f32"): (3, 7, 9, 65320),
    ("wgrad", "bf16"): (3, 47, 49, 4000),
    ("wgrad", "f32"): (3, 47, 49, 4000),
}


def c3_split(q, case):
    op, _dt = case
    n, hv, h, w = C3[case]
    segs = -(-w // C3_SEG)
    if op == "fwd":
        units = n * -(-h // C3_RPB) * segs
        groups = q("cnnitmo_conv_c3_stat_rows", n, h, w)
    else:
        units = n * h * segs
        groups = min(units, q("cnnitmo_conv_c3_wgrad_workspace_bytes", n, h, w) // 4096)
    own = [len(range(b, units, groups)) for b in range(groups)]
    return dict(units=units, groups=groups, share=(min(own), max(own)), pixels=n * h * w)


def check_c3(q, case):
    sp = c3_split(q, case)
    n, hv, h, w = C3[case]
    assert sp["share"][0] >= 3, f"{case}: a workgroup owns {sp['share'][0]} units ({sp['units']} over {sp['groups']})"
    assert hv < h and w % C3_SEG and (case[0] != "fwd" or h % C3_RPB), f"{case}: no partial unit / no invalid row"
    return sp


# ---- coverage --------------------------------------------------------------------------------------
PERSISTENT = ("halo_conv_kernel", "tconv_stream_kernel", "wgrad_halo_kernel")


def walked(q):
    """{kernel name: the first walk case that launches it}, asking the queries as the GPU file does."""
    out = {}
    for case in HALO:
        if case[0] not in HALO_FORMS:
            out.setdefault(halo_name(q, case), f"HALO {case}")
    for case in TCONV:
        out.setdefault(tconv_name(q, case), f"TCONV {case}")
    for case in WGRAD:
        out.setdefault(wgrad_name(q, case), f"WGRAD {case}")
    return out
