"""The conv / transposed-conv / fused-dgrad shapes of the per-kernel GPU tests, each with the
kernel the planners choose for it (no torch, no GPU: the host-only cnnitmo_*_kernel_name queries).

test_gpu_ops.py, test_gpu_fold.py and test_gpu_arena.py parametrise over these lists and assert,
before launching, that the query still gives the name written here; test_abi_and_host.py's
test_dispatch_coverage asserts that every name the planners give anywhere in the documented
domain (DOMAIN_CH x DOMAIN_HW x both dtypes) is the name of some case here.  A planner change
therefore fails at the case whose comment it invalidates, and a newly reachable kernel fails the
coverage test until it gets a case.

Names are those of an MI355X (256 CUs), which the planners also assume without a device.  Every
case runs N = 2 images.  Triples are (forward, input gradient, weight gradient); None: the test
does not launch that direction.

The name does not show everything: with BN partial sums (CNNITMO_STATS) the fp32 implicit GEMM
runs 256-row tiles where cnnitmo_conv3x3_kernel_name, which asks for the inference forward,
says 128x128 (fwd2_plan); the three store paths of the fused BN-backward dgrad are pinned by
DGRAD_BN_BRANCH below.
"""
DT = {"f32": 0, "bf16": 1}
N = 2

# ---- Conv2D 3x3: (cin, cout, H, W) ------------------------------------------------------------
# halo_conv_kernel<[f32,]BN,EPI[,wres]>: BN-column blocks, EPI 1 forward / 0 input gradient,
# wres: the block's weights stay in LDS (K <= 64 bf16 / 32 fp32 channels; K = cout for the dgrad),
# otherwise they are streamed per 32- / 16-channel chunk.  Tiles are 16 rows x 32 columns (conv_halo.hip:
# TH = 16, TW = 32).  These shapes have at most 24 tiles for 85 - 256 streams: no workgroup walks from
# tile to tile here; tests/walk_cases.py holds the shapes where every workgroup does.
CONV3X3_OPS = {  # test_gpu_ops.test_conv3x3_fwd_dgrad_wgrad
    # one partial tile
    (32, 32, 8, 12): {
        "bf16": ("halo_conv_kernel<32,1,wres>", "halo_conv_kernel<32,0,wres>", "wgrad_halo_kernel<32,32,64>"),
        "f32": ("halo_conv_kernel<f32,32,1,wres>", "halo_conv_kernel<f32,32,0,wres>", "wgrad_halo_kernel<f32,32,32,64>"),
    },
    # two 64-column blocks; the dgrad streams its weights (K = 128)
    (64, 128, 5, 7): {
        "bf16": ("halo_conv_kernel<64,1,wres>", "halo_conv_kernel<64,0>", "wgrad_halo_kernel<64,64,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", "halo_conv_kernel<f32,64,0>", "wgrad_halo_kernel<f32,64,64,64>"),
    },
    # streamed forward (K = 96), three 32-column dgrad blocks, 96-column wgrad blocks
    (96, 64, 6, 10): {
        "bf16": ("halo_conv_kernel<64,1>", "halo_conv_kernel<32,0,wres>", "wgrad_halo_kernel<64,96,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", "halo_conv_kernel<f32,32,0>", "wgrad_halo_kernel<f32,64,96,64>"),
    },
    # four column blocks; the 32-column dgrad with streamed weights (K = 256)
    (32, 256, 4, 4): {
        "bf16": ("halo_conv_kernel<64,1,wres>", "halo_conv_kernel<32,0>", "wgrad_halo_kernel<64,32,64>"),
        "f32": ("halo_conv_kernel<f32,64,1,wres>", "halo_conv_kernel<f32,32,0>", "wgrad_halo_kernel<f32,64,32,64>"),
    },
    # two whole 32-column tiles, half-height (8 of 16 rows); bf16 wgrad on 128-pixel strips (w % 64 == 0)
    (32, 32, 8, 64): {
        "bf16": ("halo_conv_kernel<32,1,wres>", "halo_conv_kernel<32,0,wres>", "wgrad_halo_kernel<32,32,128>"),
        "f32": ("halo_conv_kernel<f32,32,1,wres>", "halo_conv_kernel<f32,32,0,wres>", "wgrad_halo_kernel<f32,32,32,64>"),
    },
    (96, 64, 4, 128): {
        "bf16": ("halo_conv_kernel<64,1>", "halo_conv_kernel<32,0,wres>", "wgrad_halo_kernel<64,96,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", "halo_conv_kernel<f32,32,0>", "wgrad_halo_kernel<f32,64,96,64>"),
    },
    # cin 192: the bf16 wgrad's 128-column launch followed by its 64-column launch
    (192, 128, 4, 64): {
        "bf16": ("halo_conv_kernel<64,1>", "halo_conv_kernel<64,0>", "wgrad_halo_kernel<64,128+64,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", "halo_conv_kernel<f32,64,0>", "wgrad_halo_kernel<f32,64,64,64>"),
    },
    # resident weights both ways in bf16 (K = 64); fp32 streams (K > 32)
    (64, 64, 12, 64): {
        "bf16": ("halo_conv_kernel<64,1,wres>", "halo_conv_kernel<64,0,wres>", "wgrad_halo_kernel<64,64,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", "halo_conv_kernel<f32,64,0>", "wgrad_halo_kernel<f32,64,64,64>"),
    },
    # six tiles across
    (32, 64, 12, 192): {
        "bf16": ("halo_conv_kernel<64,1,wres>", "halo_conv_kernel<32,0,wres>", "wgrad_halo_kernel<64,32,128>"),
        "f32": ("halo_conv_kernel<f32,64,1,wres>", "halo_conv_kernel<f32,32,0>", "wgrad_halo_kernel<f32,64,32,64>"),
    },
    # whole 16 x 32 tiles
    (96, 64, 16, 128): {
        "bf16": ("halo_conv_kernel<64,1>", "halo_conv_kernel<32,0,wres>", "wgrad_halo_kernel<64,96,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", "halo_conv_kernel<f32,32,0>", "wgrad_halo_kernel<f32,64,96,64>"),
    },
    (192, 128, 8, 64): {
        "bf16": ("halo_conv_kernel<64,1>", "halo_conv_kernel<64,0>", "wgrad_halo_kernel<64,128+64,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", "halo_conv_kernel<f32,64,0>", "wgrad_halo_kernel<f32,64,64,64>"),
    },
    (64, 64, 16, 64): {
        "bf16": ("halo_conv_kernel<64,1,wres>", "halo_conv_kernel<64,0,wres>", "wgrad_halo_kernel<64,64,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", "halo_conv_kernel<f32,64,0>", "wgrad_halo_kernel<f32,64,64,64>"),
    },
    # a whole and a half tile down
    (32, 64, 24, 192): {
        "bf16": ("halo_conv_kernel<64,1,wres>", "halo_conv_kernel<32,0,wres>", "wgrad_halo_kernel<64,32,128>"),
        "f32": ("halo_conv_kernel<f32,64,1,wres>", "halo_conv_kernel<f32,32,0>", "wgrad_halo_kernel<f32,64,32,64>"),
    },
    # 128-channel-deep bf16 wgrad blocks
    (128, 64, 6, 64): {
        "bf16": ("halo_conv_kernel<64,1>", "halo_conv_kernel<64,0,wres>", "wgrad_halo_kernel<64,128,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", "halo_conv_kernel<f32,64,0>", "wgrad_halo_kernel<f32,64,64,64>"),
    },
    # ... and a partial last strip
    (256, 128, 10, 70): {
        "bf16": ("halo_conv_kernel<64,1>", "halo_conv_kernel<64,0>", "wgrad_halo_kernel<64,128,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", "halo_conv_kernel<f32,64,0>", "wgrad_halo_kernel<f32,64,64,64>"),
    },
    # 32 output channels from more: fp32 streams the 32-column forward, its dgrad keeps the 64-column
    # block's weights resident (K = 32); 32 x 64 wgrad blocks on 64-pixel strips
    (64, 32, 5, 7): {
        "bf16": ("halo_conv_kernel<32,1,wres>", "halo_conv_kernel<64,0,wres>", "wgrad_halo_kernel<32,64,64>"),
        "f32": ("halo_conv_kernel<f32,32,1>", "halo_conv_kernel<f32,64,0,wres>", "wgrad_halo_kernel<f32,32,64,64>"),
    },
    # ... on 128-pixel strips (w % 64 == 0)
    (64, 32, 4, 64): {
        "bf16": ("halo_conv_kernel<32,1,wres>", "halo_conv_kernel<64,0,wres>", "wgrad_halo_kernel<32,64,128>"),
        "f32": ("halo_conv_kernel<f32,32,1>", "halo_conv_kernel<f32,64,0,wres>", "wgrad_halo_kernel<f32,32,64,64>"),
    },
    # the streamed 32-column forward in bf16 (K = 96): 2 x 2 tiles, partial both ways; 32 x 96 wgrad
    (96, 32, 18, 70): {
        "bf16": ("halo_conv_kernel<32,1>", "halo_conv_kernel<32,0,wres>", "wgrad_halo_kernel<32,96,64>"),
        "f32": ("halo_conv_kernel<f32,32,1>", "halo_conv_kernel<f32,32,0,wres>", "wgrad_halo_kernel<f32,32,32,64>"),
    },
    # cout 96 (no 64-row wgrad_halo block): the bf16 wgrad falls to igemm_wgrad2, 3 taps per block;
    # three streamed 32-column forward blocks
    (128, 96, 6, 10): {
        "bf16": ("halo_conv_kernel<32,1>", "halo_conv_kernel<64,0>", "igemm_wgrad2_kernel<32,128,tpb3>"),
        "f32": ("halo_conv_kernel<f32,32,1>", "halo_conv_kernel<f32,64,0>", "wgrad_halo_kernel<f32,32,64,64>"),
    },
    # ... 9 taps per block
    (64, 96, 3, 5): {
        "bf16": ("halo_conv_kernel<32,1,wres>", "halo_conv_kernel<64,0>", "igemm_wgrad2_kernel<32,64,tpb9>"),
        "f32": ("halo_conv_kernel<f32,32,1>", "halo_conv_kernel<f32,64,0>", "wgrad_halo_kernel<f32,32,64,64>"),
    },
}

CONV3X3_FOLD = {  # test_gpu_fold.test_conv3x3_folded_fwd_wgrad (the input is a folded BN's r)
    (32, 32, 8, 12): {
        "bf16": ("halo_conv_kernel<32,1,wres>", None, "wgrad_halo_kernel<32,32,64>"),
        "f32": ("halo_conv_kernel<f32,32,1,wres>", None, "wgrad_halo_kernel<f32,32,32,64>"),
    },
    (64, 128, 5, 7): {
        "bf16": ("halo_conv_kernel<64,1,wres>", None, "wgrad_halo_kernel<64,64,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", None, "wgrad_halo_kernel<f32,64,64,64>"),
    },
    # one row / one column: every pixel on the border
    (96, 64, 1, 6): {
        "bf16": ("halo_conv_kernel<64,1>", None, "wgrad_halo_kernel<64,96,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", None, "wgrad_halo_kernel<f32,64,96,64>"),
    },
    (32, 64, 6, 1): {
        "bf16": ("halo_conv_kernel<64,1,wres>", None, "wgrad_halo_kernel<64,32,64>"),
        "f32": ("halo_conv_kernel<f32,64,1,wres>", None, "wgrad_halo_kernel<f32,64,32,64>"),
    },
    (128, 256, 3, 4): {
        "bf16": ("halo_conv_kernel<64,1>", None, "wgrad_halo_kernel<64,128,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", None, "wgrad_halo_kernel<f32,64,64,64>"),
    },
    (64, 64, 8, 64): {
        "bf16": ("halo_conv_kernel<64,1,wres>", None, "wgrad_halo_kernel<64,64,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", None, "wgrad_halo_kernel<f32,64,64,64>"),
    },
    # cout 96: three 32-column forward blocks; the bf16 wgrad on igemm_wgrad2 (9 taps per block)
    (32, 96, 4, 128): {
        "bf16": ("halo_conv_kernel<32,1,wres>", None, "igemm_wgrad2_kernel<32,32,tpb9>"),
        "f32": ("halo_conv_kernel<f32,32,1,wres>", None, "wgrad_halo_kernel<f32,32,32,64>"),
    },
    (64, 64, 16, 96): {
        "bf16": ("halo_conv_kernel<64,1,wres>", None, "wgrad_halo_kernel<64,64,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", None, "wgrad_halo_kernel<f32,64,64,64>"),
    },
    (32, 32, 16, 128): {
        "bf16": ("halo_conv_kernel<32,1,wres>", None, "wgrad_halo_kernel<32,32,128>"),
        "f32": ("halo_conv_kernel<f32,32,1,wres>", None, "wgrad_halo_kernel<f32,32,32,64>"),
    },
}

CONV3X3_ARENA = {  # test_gpu_arena.test_conv3x3
    # one partial 16 x 32 tile; resident weights
    (32, 32, 5, 7): {
        "bf16": ("halo_conv_kernel<32,1,wres>", "halo_conv_kernel<32,0,wres>", "wgrad_halo_kernel<32,32,64>"),
        "f32": ("halo_conv_kernel<f32,32,1,wres>", "halo_conv_kernel<f32,32,0,wres>", "wgrad_halo_kernel<f32,32,32,64>"),
    },
    # last tile partial in both directions; streamed forward weights, 32-column dgrad blocks
    (96, 64, 18, 35): {
        "bf16": ("halo_conv_kernel<64,1>", "halo_conv_kernel<32,0,wres>", "wgrad_halo_kernel<64,96,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", "halo_conv_kernel<f32,32,0>", "wgrad_halo_kernel<f32,64,96,64>"),
    },
    # one whole-height tile, two column blocks
    (64, 128, 16, 32): {
        "bf16": ("halo_conv_kernel<64,1,wres>", "halo_conv_kernel<64,0>", "wgrad_halo_kernel<64,64,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", "halo_conv_kernel<f32,64,0>", "wgrad_halo_kernel<f32,64,64,64>"),
    },
    # streamed weights both ways, partial last strip, 128-deep bf16 wgrad blocks
    (256, 128, 10, 70): {
        "bf16": ("halo_conv_kernel<64,1>", "halo_conv_kernel<64,0>", "wgrad_halo_kernel<64,128,64>"),
        "f32": ("halo_conv_kernel<f32,64,1>", "halo_conv_kernel<f32,64,0>", "wgrad_halo_kernel<f32,64,64,64>"),
    },
}

# With CNNITMO_HALO=0 (read once per process: test_gpu_ops.test_conv3x3_without_halo_kernel's
# child) the forward and the input gradient run the 9-tap implicit GEMMs: igemm_fwd_kernel for 32
# output columns, igemm_fwd2_kernel<T,BMxBN> otherwise.  The weight gradients do not read the switch.
CONV3X3_HALO0 = {
    (32, 32, 8, 12): {
        "bf16": ("igemm_fwd_kernel<bf16,256x32>", "igemm_fwd_kernel<bf16,256x32>", "wgrad_halo_kernel<32,32,64>"),
        "f32": ("igemm_fwd_kernel<f32,256x32>", "igemm_fwd_kernel<f32,256x32>", "wgrad_halo_kernel<f32,32,32,64>"),
    },
    (96, 64, 6, 10): {
        "bf16": ("igemm_fwd2_kernel<bf16,256x64>", "igemm_fwd2_kernel<bf16,256x96>", "wgrad_halo_kernel<64,96,64>"),
        "f32": ("igemm_fwd2_kernel<f32,256x64>", "igemm_fwd2_kernel<f32,256x96>", "wgrad_halo_kernel<f32,64,96,64>"),
    },
    # (fp32 forward: this training launch has BN sums and so runs 256x128; the name is the inference one)
    (64, 128, 5, 7): {
        "bf16": ("igemm_fwd2_kernel<bf16,256x128>", "igemm_fwd2_kernel<bf16,256x64>", "wgrad_halo_kernel<64,64,64>"),
        "f32": ("igemm_fwd2_kernel<f32,128x128>", "igemm_fwd2_kernel<f32,256x64>", "wgrad_halo_kernel<f32,64,64,64>"),
    },
    (32, 96, 4, 128): {
        "bf16": ("igemm_fwd2_kernel<bf16,256x96>", "igemm_fwd_kernel<bf16,256x32>", "igemm_wgrad2_kernel<32,32,tpb9>"),
        "f32": ("igemm_fwd2_kernel<f32,256x96>", "igemm_fwd_kernel<f32,256x32>", "wgrad_halo_kernel<f32,32,32,64>"),
    },
    # the fp32 input gradient (no sums) on 128 x 128 tiles
    (128, 64, 6, 10): {
        "bf16": ("igemm_fwd2_kernel<bf16,256x64>", "igemm_fwd2_kernel<bf16,256x128>", "wgrad_halo_kernel<64,128,64>"),
        "f32": ("igemm_fwd2_kernel<f32,256x64>", "igemm_fwd2_kernel<f32,128x128>", "wgrad_halo_kernel<f32,64,64,64>"),
    },
    # 160 columns: five 32-column blocks of igemm_fwd2
    (32, 160, 4, 4): {
        "bf16": ("igemm_fwd2_kernel<bf16,256x32>", "igemm_fwd_kernel<bf16,256x32>", "igemm_wgrad2_kernel<32,32,tpb9>"),
        "f32": ("igemm_fwd2_kernel<f32,256x32>", "igemm_fwd_kernel<f32,256x32>", "wgrad_halo_kernel<f32,32,32,64>"),
    },
}
# test_conv_affine_inference_epilogue's body in the same child: (dtype, H, W, cin, cout) -> forward
# name; the last one is the fp32 inference forward (no BN sums) on igemm_fwd2's 128 x 128 tiles
AFFINE_HALO0 = {
    ("f32", 6, 9, 32, 64): "igemm_fwd2_kernel<f32,256x64>",
    ("bf16", 6, 9, 32, 64): "igemm_fwd2_kernel<bf16,256x64>",
    ("f32", 6, 9, 32, 128): "igemm_fwd2_kernel<f32,128x128>",
}

# ---- Conv2DTranspose 2x2: (cin, cout, H, W) ---------------------------------------------------
# forward GEMM: K = cin, N = 4 cout columns; input gradient: K = 4 cout, N = cin
TCONV_OPS = {  # test_gpu_ops.test_tconv
    # generic kernels
    (64, 32, 3, 5): {
        "bf16": ("igemm_fwd2_kernel<bf16,256x128>", "tconv_stream_kernel<1,64>", "igemm_wgrad2_kernel<32,64,tpb4>"),
        "f32": ("igemm_fwd2_kernel<f32,128x128>", "igemm_fwd2_kernel<f32,256x64>", "igemm_wgrad_kernel<f32,32,64>"),
    },
    # bf16: the streamed kernels (one resident column block); fp32: weight-stationary
    (128, 64, 4, 4): {
        "bf16": ("tconv_stream_kernel<0,256>", "tconv_stream_kernel<1,128>", "wgrad_tconv_kernel<64,128,32>"),
        "f32": ("tconv_ws_kernel<f32,0,128>", "tconv_ws_kernel<f32,1,128>", "wgrad_tconv_f32_kernel<64,64,32>"),
    },
    # bf16: the persistent 256 x 256 kernels (up6 - up8's); one partial tile
    (512, 256, 2, 3): {
        "bf16": ("tconv_fwd2p_kernel<bf16,256x256>", "igemm_fwd2p_kernel<bf16,256x256>", "wgrad_tconv_kernel<128,128,32>"),
        "f32": ("tconv_ws_kernel<f32,0,64>", "igemm_fwd2_kernel<f32,128x128>", "wgrad_tconv_f32_kernel<64,64,32>"),
    },
    # streamed (bf16), partial 64-pixel tiles
    (128, 64, 3, 70): {
        "bf16": ("tconv_stream_kernel<0,256>", "tconv_stream_kernel<1,128>", "wgrad_tconv_kernel<64,128,32>"),
        "f32": ("tconv_ws_kernel<f32,0,128>", "tconv_ws_kernel<f32,1,128>", "wgrad_tconv_f32_kernel<64,64,32>"),
    },
    # bf16: persistent kernels, two 256-column blocks (up8); fp32 dgrad weight-stationary at K = 512
    (256, 128, 5, 33): {
        "bf16": ("tconv_fwd2p_kernel<bf16,256x256>", "igemm_fwd2p_kernel<bf16,256x256>", "wgrad_tconv_kernel<128,128,32>"),
        "f32": ("tconv_ws_kernel<f32,0,128>", "tconv_ws_kernel<f32,1,64>", "wgrad_tconv_f32_kernel<64,64,32>"),
    },
    # streamed, 128-column forward block; cout 32: the wgrad on igemm_wgrad2 / igemm_wgrad
    (128, 32, 2, 130): {
        "bf16": ("tconv_stream_kernel<0,128>", "tconv_stream_kernel<1,128>", "igemm_wgrad2_kernel<32,128,tpb4>"),
        "f32": ("tconv_ws_kernel<f32,0,128>", "igemm_fwd2_kernel<f32,128x128>", "igemm_wgrad_kernel<f32,32,128>"),
    },
    # eight 256-column blocks (512 -> 512); ragged tiles
    (512, 512, 3, 7): {
        "bf16": ("tconv_fwd2p_kernel<bf16,256x256>", "igemm_fwd2p_kernel<bf16,256x256>", "wgrad_tconv_kernel<128,128,32>"),
        "f32": ("tconv_ws_kernel<f32,0,64>", "igemm_fwd2_kernel<f32,128x128>", "wgrad_tconv_f32_kernel<64,64,32>"),
    },
    (256, 128, 7, 9): {
        "bf16": ("tconv_fwd2p_kernel<bf16,256x256>", "igemm_fwd2p_kernel<bf16,256x256>", "wgrad_tconv_kernel<128,128,32>"),
        "f32": ("tconv_ws_kernel<f32,0,128>", "tconv_ws_kernel<f32,1,64>", "wgrad_tconv_f32_kernel<64,64,32>"),
    },
    # 1024 / 2048-deep gradients (up7 / up6); ragged tiles
    (512, 256, 5, 7): {
        "bf16": ("tconv_fwd2p_kernel<bf16,256x256>", "igemm_fwd2p_kernel<bf16,256x256>", "wgrad_tconv_kernel<128,128,32>"),
        "f32": ("tconv_ws_kernel<f32,0,64>", "igemm_fwd2_kernel<f32,128x128>", "wgrad_tconv_f32_kernel<64,64,32>"),
    },
    (512, 256, 17, 33): {
        "bf16": ("tconv_fwd2p_kernel<bf16,256x256>", "igemm_fwd2p_kernel<bf16,256x256>", "wgrad_tconv_kernel<128,128,32>"),
        "f32": ("tconv_ws_kernel<f32,0,64>", "igemm_fwd2_kernel<f32,128x128>", "wgrad_tconv_f32_kernel<64,64,32>"),
    },
    (256, 512, 9, 31): {
        "bf16": ("tconv_fwd2p_kernel<bf16,256x256>", "igemm_fwd2p_kernel<bf16,256x256>", "wgrad_tconv_kernel<128,128,32>"),
        "f32": ("tconv_ws_kernel<f32,0,128>", "igemm_fwd2_kernel<f32,128x128>", "wgrad_tconv_f32_kernel<64,64,32>"),
    },
    # > 256 tiles of 256 x 256: each persistent workgroup (one per CU) walks several
    (512, 256, 96, 176): {
        "bf16": ("tconv_fwd2p_kernel<bf16,256x256>", "igemm_fwd2p_kernel<bf16,256x256>", "wgrad_tconv_kernel<128,128,32>"),
        "f32": ("tconv_ws_kernel<f32,0,64>", "igemm_fwd2_kernel<f32,128x128>", "wgrad_tconv_f32_kernel<64,64,32>"),
    },
    # bf16 row-streaming wgrad: 4 rows per workgroup, 2 strips
    (512, 512, 16, 40): {
        "bf16": ("tconv_fwd2p_kernel<bf16,256x256>", "igemm_fwd2p_kernel<bf16,256x256>", "wgrad_tconv_kernel<128,128,32>"),
        "f32": ("tconv_ws_kernel<f32,0,64>", "igemm_fwd2_kernel<f32,128x128>", "wgrad_tconv_f32_kernel<64,64,32>"),
    },
    # the bf16 weight-stationary forward: the one 128-column block neither the streamed kernel (K = 512:
    # 64-column blocks) nor tconv_fwd2p (N % 256) takes; its dgrad on igemm_fwd2's 256 x 256 tiles, not the
    # persistent kernel (32 channels per tap: fwd2_plan wants a multiple of 64); two row tiles
    (512, 32, 9, 17): {
        "bf16": ("tconv_ws_kernel<0,128>", "igemm_fwd2_kernel<bf16,256x256>", "igemm_wgrad2_kernel<32,128,tpb4>"),
        "f32": ("tconv_ws_kernel<f32,0,64>", "igemm_fwd2_kernel<f32,128x128>", "igemm_wgrad_kernel<f32,32,128>"),
    },
    # the streamed dgrad with one 256-column block (K = 128); partial 64-pixel tiles
    (256, 32, 3, 70): {
        "bf16": ("tconv_stream_kernel<0,128>", "tconv_stream_kernel<1,256>", "igemm_wgrad2_kernel<32,128,tpb4>"),
        "f32": ("tconv_ws_kernel<f32,0,128>", "igemm_fwd2_kernel<f32,128x128>", "igemm_wgrad_kernel<f32,32,128>"),
    },
    # cout 96 (K = 384): the bf16 dgrad on igemm_fwd2's 128 x 128 tiles, three row tiles (the last partial)
    (128, 96, 9, 17): {
        "bf16": ("igemm_fwd2_kernel<bf16,256x128>", "igemm_fwd2_kernel<bf16,128x128>", "igemm_wgrad2_kernel<32,128,tpb4>"),
        "f32": ("igemm_fwd2_kernel<f32,128x128>", "igemm_fwd2_kernel<f32,128x128>", "igemm_wgrad_kernel<f32,32,128>"),
    },
    # cin 160 / 64 (K = 640) / 96 / 32: the input gradients on 32-, 64-, 96-column igemm_fwd2 blocks and
    # on igemm_fwd_kernel; 32 x 32 wgrad blocks
    (160, 32, 9, 17): {
        "bf16": ("igemm_fwd2_kernel<bf16,256x128>", "igemm_fwd2_kernel<bf16,256x32>", "igemm_wgrad2_kernel<32,32,tpb4>"),
        "f32": ("igemm_fwd2_kernel<f32,128x128>", "igemm_fwd2_kernel<f32,256x32>", "igemm_wgrad_kernel<f32,32,32>"),
    },
    (64, 160, 9, 17): {
        "bf16": ("igemm_fwd2_kernel<bf16,256x128>", "igemm_fwd2_kernel<bf16,256x64>", "igemm_wgrad2_kernel<32,64,tpb4>"),
        "f32": ("igemm_fwd2_kernel<f32,128x128>", "igemm_fwd2_kernel<f32,256x64>", "igemm_wgrad_kernel<f32,32,64>"),
    },
    (96, 32, 5, 7): {
        "bf16": ("igemm_fwd2_kernel<bf16,256x128>", "igemm_fwd2_kernel<bf16,256x96>", "igemm_wgrad2_kernel<32,32,tpb4>"),
        "f32": ("igemm_fwd2_kernel<f32,128x128>", "igemm_fwd2_kernel<f32,256x96>", "igemm_wgrad_kernel<f32,32,32>"),
    },
    (32, 32, 9, 17): {
        "bf16": ("igemm_fwd2_kernel<bf16,256x128>", "igemm_fwd_kernel<bf16,256x32>", "igemm_wgrad2_kernel<32,32,tpb4>"),
        "f32": ("igemm_fwd2_kernel<f32,128x128>", "igemm_fwd_kernel<f32,256x32>", "igemm_wgrad_kernel<f32,32,32>"),
    },
    # the remaining 4-tap wgrad blocks: 128 x 32, 128 x 64 (two taps per block), 64 x 32, 64 x 64
    (32, 128, 3, 5): {
        "bf16": ("igemm_fwd2_kernel<bf16,256x128>", "igemm_fwd_kernel<bf16,256x32>", "igemm_wgrad2_kernel<128,32,tpb4>"),
        "f32": ("igemm_fwd2_kernel<f32,128x128>", "igemm_fwd_kernel<f32,256x32>", "igemm_wgrad_kernel<f32,128,32>"),
    },
    (64, 128, 3, 5): {
        "bf16": ("tconv_fwd2p_kernel<bf16,256x256>", "tconv_stream_kernel<1,64>", "igemm_wgrad2_kernel<128,64,tpb2>"),
        "f32": ("igemm_fwd2_kernel<f32,128x128>", "tconv_ws_kernel<f32,1,64>", "wgrad_tconv_f32_kernel<64,64,32>"),
    },
    (32, 64, 5, 7): {
        "bf16": ("igemm_fwd2_kernel<bf16,256x128>", "igemm_fwd_kernel<bf16,256x32>", "igemm_wgrad2_kernel<64,32,tpb4>"),
        "f32": ("igemm_fwd2_kernel<f32,128x128>", "igemm_fwd_kernel<f32,256x32>", "igemm_wgrad_kernel<f32,64,32>"),
    },
    (64, 64, 4, 4): {
        "bf16": ("tconv_fwd2p_kernel<bf16,256x256>", "tconv_stream_kernel<1,64>", "igemm_wgrad2_kernel<64,64,tpb4>"),
        "f32": ("igemm_fwd2_kernel<f32,128x128>", "igemm_fwd2_kernel<f32,256x64>", "wgrad_tconv_f32_kernel<64,64,32>"),
    },
}

TCONV_ARENA = {  # test_gpu_arena.test_tconv
    (64, 32, 3, 5): TCONV_OPS[(64, 32, 3, 5)],          # generic kernels
    (128, 64, 3, 70): TCONV_OPS[(128, 64, 3, 70)],      # streamed (bf16), partial 64-pixel tiles
    (128, 32, 2, 130): TCONV_OPS[(128, 32, 2, 130)],
    (256, 128, 7, 9): TCONV_OPS[(256, 128, 7, 9)],      # the persistent 256 x 256 kernels (bf16);
    (512, 512, 3, 7): TCONV_OPS[(512, 512, 3, 7)],      # weight-stationary forward (fp32)
    (512, 256, 5, 7): TCONV_OPS[(512, 256, 5, 7)],
}

TCONV_FOLD = {  # test_gpu_fold.test_tconv_folded_fwd_wgrad (forward and weight gradient)
    sh: {dt: (TCONV_OPS[sh][dt][0], None, TCONV_OPS[sh][dt][2]) for dt in DT}
    for sh in [(64, 32, 3, 5), (128, 64, 4, 4), (512, 256, 2, 3)]
}

TCONV_AFFINE = {  # test_gpu_ops.test_tconv_affine_inference_epilogue (forward only)
    (512, 256, 5, 7): {"bf16": ("tconv_fwd2p_kernel<bf16,256x256>", None, None),
                       "f32": ("tconv_ws_kernel<f32,0,64>", None, None)},
    (256, 128, 9, 40): {"bf16": ("tconv_fwd2p_kernel<bf16,256x256>", None, None),
                        "f32": ("tconv_ws_kernel<f32,0,128>", None, None)},
}

# ---- fused BN-backward input gradients --------------------------------------------------------
# cnnitmo_conv3x3_dgrad_bn: (cin, cout, H, W, c0, c1, parity sums) -> halo_conv_kernel<[f32,]BN,2[,wres]>
# (test_gpu_fold.test_conv3x3_dgrad_bn_fused, test_gpu_arena.test_conv3x3_dgrad_bn); K = cout
DGRAD_BN = {
    # the whole input (enc1a -> enc1b), partial tiles
    (32, 32, 20, 40, 0, 32, False): {"bf16": "halo_conv_kernel<32,2,wres>", "f32": "halo_conv_kernel<f32,32,2,wres>"},
    # concat [skip 32 | up 64]: three 32-column blocks, the first one plain
    (96, 64, 18, 70, 32, 96, True): {"bf16": "halo_conv_kernel<32,2,wres>", "f32": "halo_conv_kernel<f32,32,2>"},
    # five 32-column blocks, resident weights in bf16 (K = 64)
    (160, 64, 16, 40, 32, 160, True): {"bf16": "halo_conv_kernel<32,2,wres>", "f32": "halo_conv_kernel<f32,32,2>"},
    # concat [skip 64 | up 128]: three 64-column blocks
    (192, 128, 16, 32, 64, 192, True): {"bf16": "halo_conv_kernel<64,2>", "f32": "halo_conv_kernel<f32,64,2>"},
    (128, 64, 17, 33, 0, 128, False): {"bf16": "halo_conv_kernel<64,2,wres>", "f32": "halo_conv_kernel<f32,64,2>"},
    # the streamed 32-column kernel (K = 128) with c0 on a block boundary: in bf16 the epilogue whose
    # blocks are each fused or plain (DGRAD_BN_BRANCH).  Its raw-buffer stores carry no tensor bound
    # (dma::brsrc: 2 GiB of records) but the in-image mask, so by hand, for the pixels m < P = 2*16*40
    # of the two 16 x 32 tiles' in-image part (h = 16: no partial rows; w = 40: columns 40..63 masked):
    #   plain block n0 = 0 -> dx element m * dx_ld + dx_off + 8g + k, 8g + k <= 31 < c0 = 32 <= the
    #     view's 160 channels: inside dx ([P][dx_ld], dx_off + 160 <= dx_ld);
    #   fused blocks n0 = 32..128 -> dz_out element m * 128 + (n0 - 32) + 8g + k <= m * 128 + 96 + 31:
    #     column <= 127 < c1 - c0 = 128, last element P * 128 - 1: inside dz_out [P][128];
    #   r pieces: r_off is OOB (zeros) below c0, else m * r_ld + r_off + (c - 32) + k, c - 32 + 7 <= 127
    #     < the view's 128 channels; the sums rows are written for c0 <= c < c1 only.
    (160, 128, 16, 40, 32, 160, True): {"bf16": "halo_conv_kernel<32,2>", "f32": "halo_conv_kernel<f32,32,2>"},
    # one 64-column block, every column fused, resident weights in both dtypes (K = 32)
    (64, 32, 17, 33, 0, 64, False): {"bf16": "halo_conv_kernel<64,2,wres>", "f32": "halo_conv_kernel<f32,64,2,wres>"},
}

# The store path of the fused dgrad, which the name does not show (conv_halo.hip, halo_plan, EPI 2):
#   allf = bnb_c1 == N && (bnb_c0 == 0 || (is bf16 && !res && bnb_c0 % BN == 0))
# (N = cin, res = the ",wres" of the name, BN its block width); test_dgrad_bn_branches restates it
# from the name of each row's DGRAD_BN case.  (cin, cout, c0, c1, dtype) -> branch
DGRAD_BN_BRANCH = {
    # "bnb_c1 == N && bnb_c0 == 0": every column fused, one raw-buffer store path
    (32, 32, 0, 32, "bf16"): "all",
    # "is bf16 && !res && bnb_c0 % BN == 0": each 32-column block either fused or plain
    (160, 128, 32, 160, "bf16"): "mixed",
    # neither: res (K = 64 <= 64), so the generic epilogue with per-column selects and global stores
    (160, 64, 32, 160, "bf16"): "neither",
    # fp32 never takes the mixed form
    (160, 128, 32, 160, "f32"): "neither",
}

# cnnitmo_conv3x3_dgrad_bn_pooled: (cin, cout, H, W) -> name (test_gpu_fold.test_conv3x3_dgrad_bn_pooled,
# test_gpu_arena.test_conv3x3_dgrad_bn_pooled); always 32-column blocks, K = cout
DGRAD_BN_POOLED = {
    # dec9's skip path (conv1 32 of the [32 | 64] concat), partial tiles
    (32, 64, 20, 40): {"bf16": "halo_conv_kernel<32,2,wres,route>", "f32": "halo_conv_kernel<f32,32,2,route>"},
    # ragged in both directions
    (32, 64, 34, 70): {"bf16": "halo_conv_kernel<32,2,wres,route>", "f32": "halo_conv_kernel<f32,32,2,route>"},
    # two column blocks, streamed weights (K = 128)
    (64, 128, 16, 32): {"bf16": "halo_conv_kernel<32,2,route>", "f32": "halo_conv_kernel<f32,32,2,route>"},
    (32, 96, 18, 66): {"bf16": "halo_conv_kernel<32,2,route>", "f32": "halo_conv_kernel<f32,32,2,route>"},
    # resident weights in fp32 too (K = 32)
    (32, 32, 18, 34): {"bf16": "halo_conv_kernel<32,2,wres,route>", "f32": "halo_conv_kernel<f32,32,2,wres,route>"},
}

# cnnitmo_tconv2x2_dgrad_bn (bf16 only): (cin, cout, H, W) -> name
# (test_gpu_fold.test_tconv_dgrad_bn_fused, test_gpu_arena.test_tconv_dgrad_bn)
TCONV_DGRAD_BN = {
    (128, 64, 3, 70): "tconv_stream_kernel<1,128,bnb>",
    (64, 32, 4, 64): "tconv_stream_kernel<1,64,bnb>",
    (128, 32, 2, 130): "tconv_stream_kernel<1,128,bnb>",
}

# test_gpu_fold.test_dgrad_bn_fused_vs_oracle (bf16): (kind, cin, cout, H, W, c0, c1) -> name
DGRAD_BN_ORACLE = {
    ("c3", 96, 64, 18, 70, 32, 96): "halo_conv_kernel<32,2,wres>",     # dec9-style concat [skip 32 | up 64]
    ("c3", 64, 64, 16, 64, 0, 64): "halo_conv_kernel<64,2,wres>",      # whole input (enc chain)
    ("c3", 192, 128, 16, 32, 64, 192): "halo_conv_kernel<64,2>",       # dec8-style
    ("t2", 128, 64, 3, 70, 0, 128): "tconv_stream_kernel<1,128,bnb>",  # up9 dgrad into conv8's BN
}

# ---- the documented domain ---------------------------------------------------------------------
DOMAIN_CH = (32, 64, 96, 128, 160, 192, 256, 384, 512)
DOMAIN_HW = ((4, 4), (6, 10), (16, 64), (18, 70), (16, 128))
HALO0 = "CNNITMO_HALO=0 "  # prefix of the names asked with the halo kernel switched off


def _s(v):
    return v.decode() if isinstance(v, bytes) else v


def conv3x3_names(q, dt, cin, cout, h, w, n=N):
    """(forward, input gradient, weight gradient) of a 3x3 conv; q(name, *args) asks the library."""
    d = DT[dt]
    return (_s(q("cnnitmo_conv3x3_kernel_name", d, n, h, w, cin, cout, 0)),
            _s(q("cnnitmo_conv3x3_kernel_name", d, n, h, w, cin, cout, 1)),
            _s(q("cnnitmo_wgrad_kernel_name", d, 9, n, h, w, cin, cout)))


def tconv_names(q, dt, cin, cout, h, w, n=N):
    d = DT[dt]
    return (_s(q("cnnitmo_tconv2x2_kernel_name", d, n, h, w, cin, cout, 0)),
            _s(q("cnnitmo_tconv2x2_kernel_name", d, n, h, w, cin, cout, 1)),
            _s(q("cnnitmo_wgrad_kernel_name", d, 4, n, h, w, cin, cout)))


def dgrad_bn_name(q, dt, cin, cout, h, w, c0, c1, n=N):
    return _s(q("cnnitmo_conv3x3_dgrad_bn_kernel_name", DT[dt], n, h, w, cout, cin, c0, c1))


def dgrad_bn_pooled_name(q, dt, cin, cout, h, w, n=N):
    return _s(q("cnnitmo_conv3x3_dgrad_bn_pooled_kernel_name", DT[dt], n, h, w, cout, cin))


def tconv_dgrad_bn_name(q, dt, cin, cout, h, w, n=N):
    return _s(q("cnnitmo_tconv2x2_dgrad_bn_kernel_name", DT[dt], n, h, w, cout, cin))


def expect_kernels(got, want):
    """Before a case launches: the planner still chooses the kernels the case is there for (the
    names next to its shape above; None: a direction the case does not launch)."""
    got, want = (got, want) if isinstance(want, tuple) else ((got,), (want,))
    for g, w in zip(got, want):
        assert w is None or g == w, f"the planner chooses {g}; this case is meant for {w}"


def dgrad_bn_branch(name, dt, cin, c0, c1):
    """halo_plan's choice (HaloPlan::alt) restated from the kernel name (BN and wres) and the column range."""
    bn = int(name.split("<")[1].replace("f32,", "").split(",")[0])
    res = ",wres" in name
    if c1 == cin and c0 == 0:
        return "all"
    if c1 == cin and dt == "bf16" and not res and c0 % bn == 0:
        return "mixed"
    return "neither"


def reachable(q, halo0=False):
    """{kernel name: the first domain point that reaches it} over DOMAIN_CH x DOMAIN_CH x DOMAIN_HW x
    dtypes.  halo0 (the process runs with CNNITMO_HALO=0): the 3x3 forward and dgrad only, prefixed."""
    out = {}
    for dt in ("bf16", "f32"):
        for cin in DOMAIN_CH:
            for cout in DOMAIN_CH:
                for h, w in DOMAIN_HW:
                    at = f"{dt} {cin}->{cout} {h}x{w}"
                    c3 = conv3x3_names(q, dt, cin, cout, h, w)
                    if halo0:
                        for what, nm in zip(("conv3x3 fwd", "conv3x3 dgrad"), c3):
                            out.setdefault(HALO0 + nm, f"{what} {at}")
                        continue
                    names = list(zip(("conv3x3 fwd", "conv3x3 dgrad", "conv3x3 wgrad"), c3))
                    names += zip(("tconv fwd", "tconv dgrad", "tconv wgrad"), tconv_names(q, dt, cin, cout, h, w))
                    names += [(f"dgrad_bn c0={c0}", dgrad_bn_name(q, dt, cin, cout, h, w, c0, cin)) for c0 in (0, 32, 64)]
                    names.append(("dgrad_bn_pooled", dgrad_bn_pooled_name(q, dt, cin, cout, h, w)))
                    names.append(("tconv_dgrad_bn", tconv_dgrad_bn_name(q, dt, cin, cout, h, w)))
                    for what, nm in names:
                        if nm:  # "": the fused path does not take these sizes (the caller runs the unfused pair)
                            out.setdefault(nm, f"{what} {at}")
    return out


def tested(q, halo0=False):
    """{kernel name: the first case that launches it}, asking the same queries for the case lists."""
    out = {}

    def triples(lists, namer, prefix=""):
        for label, cases in lists:
            for sh, exp in cases.items():
                for dt in ("bf16", "f32"):
                    got = namer(q, dt, *sh)
                    for what, nm, e in zip(("fwd", "dgrad", "wgrad"), got, exp[dt]):
                        if e is not None and (not prefix or what != "wgrad"):
                            out.setdefault(prefix + nm, f"{label} {sh} {dt} {what}")

    if halo0:
        triples([("CONV3X3_HALO0", CONV3X3_HALO0)], conv3x3_names, HALO0)
        for (dt, h, w, cin, cout) in AFFINE_HALO0:
            out.setdefault(HALO0 + conv3x3_names(q, dt, cin, cout, h, w, 1)[0], f"AFFINE_HALO0 {(dt, h, w, cin, cout)}")
        return out
    triples([("CONV3X3_OPS", CONV3X3_OPS), ("CONV3X3_FOLD", CONV3X3_FOLD), ("CONV3X3_ARENA", CONV3X3_ARENA)],
            conv3x3_names)
    triples([("TCONV_OPS", TCONV_OPS), ("TCONV_ARENA", TCONV_ARENA), ("TCONV_FOLD", TCONV_FOLD),
             ("TCONV_AFFINE", TCONV_AFFINE)], tconv_names)
    for (cin, cout, h, w, c0, c1, _par) in DGRAD_BN:
        for dt in ("bf16", "f32"):
            out.setdefault(dgrad_bn_name(q, dt, cin, cout, h, w, c0, c1), f"DGRAD_BN {(cin, cout, h, w, c0, c1)} {dt}")
    for sh in DGRAD_BN_POOLED:
        for dt in ("bf16", "f32"):
            out.setdefault(dgrad_bn_pooled_name(q, dt, *sh), f"DGRAD_BN_POOLED {sh} {dt}")
    for sh in TCONV_DGRAD_BN:
        out.setdefault(tconv_dgrad_bn_name(q, "bf16", *sh), f"TCONV_DGRAD_BN {sh} bf16")
    return out
