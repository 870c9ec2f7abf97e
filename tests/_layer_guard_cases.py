"""The cases tests/test_layer_guard_cases_host.py and tests/test_gpu_layer_guard_bands.py share: for each CNN layer entry point
the shapes to run and the plan each shape is meant to take -- K slices and workspace bytes as the library's host-only queries
state them (mv_conv3x3_k_slices, mv_linear_k_slices, mv_conv1x1_k_slices, mv_inverted_residual_k_slices and their
*_workspace_bytes; mv_conv2d_needs_workspace, mv_deform_conv2d_needs_workspace, mv_deform_conv2d_workspace_bytes) -- with the launcher flag or tile edge the shape is there for.  The host test asserts the plans on a machine
without a GPU, so a change to a plan cannot quietly empty a sweep; the GPU test runs the shapes inside guard bands.

A plain table: no fixtures, no device code."""

# ---- mv_conv3x3_bias_relu_f32 / _ws_f32 (csrc/conv3x3_gen.hip, conv3x3_mfma.hip, conv3x3_c3.hip) ---------------------------------
# shape = (n, cin, cout, h, w); env: MV_* knobs of the tuning build ({} = the product library); slices / slice_channels as
# mv_conv3x3_k_slices states them under that env (1 = the single chain, workspace 0); kernel: what mv_last_kernel() must
# contain when every pointer is aligned.
CONV3X3 = [
    # k_conv3x3_gen, the product library's own choice of wave tile: widths off the 4-column groups and below 4 (direct staging),
    # cin off the 4-channel K chunk (vec_w = 0 by shape), cout off the 32- and 128-channel tiles
    dict(shape=(2, 12, 40, 5, 3), env={}, slices=1, slice_channels=12, kernel="k_conv3x3_gen", why="w = 3 < 4: direct staging"),
    dict(shape=(1, 5, 8, 6, 5), env={}, slices=1, slice_channels=5, kernel="k_conv3x3_gen", why="w = 5, cin % 4 != 0, cout = 8"),
    dict(shape=(2, 4, 33, 7, 12), env={}, slices=1, slice_channels=4, kernel="k_conv3x3_gen", why="vec_w by pointer alone (cin = 4), cout = 33"),
    dict(shape=(1, 13, 130, 5, 13), env={}, slices=1, slice_channels=13, kernel="k_conv3x3_gen", why="w = 13 ragged, cin = 13, cout = 130"),
    dict(shape=(3, 16, 130, 9, 33), env={}, slices=1, slice_channels=16, kernel="k_conv3x3_gen", why="w = 33, two channel blocks"),
    dict(shape=(2, 5, 40, 6, 14), env={}, slices=1, slice_channels=5, kernel="k_conv3x3_gen", why="w = 14, cin = 5, cout = 40"),
    # cin < 4: K = 9 * cin < 36, so the one K chunk's weight items run past the end of a weight row (and of w, for the last row)
    dict(shape=(1, 1, 8, 5, 8), env={}, slices=1, slice_channels=1, kernel="k_conv3x3_gen", why="cin = 1: 27 of the chunk's 36 taps are padding"),
    dict(shape=(2, 2, 33, 6, 7), env={}, slices=1, slice_channels=2, kernel="k_conv3x3_gen", why="cin = 2"),
    # K slices across workgroups through the workspace + k_conv3x3_reduce
    dict(shape=(1, 130, 40, 9, 11), env={}, slices=2, slice_channels=68, kernel="k_conv3x3_reduce<ks2>", why="smallest sliced shape; cin = 130"),
    dict(shape=(1, 256, 33, 7, 7), env={}, slices=4, slice_channels=64, kernel="k_conv3x3_reduce<ks4>", why="cin >= 256 at 7 x 7"),
    # the three wave tiles forced, loader waves on and off, dense and first small-launch forms
    dict(shape=(3, 8, 40, 14, 14), env={"MV_CONV_SHAPE": "0", "MV_CONV_SPEC42": "0"}, slices=1, slice_channels=8, kernel="k_conv3x3_gen", why="4x2 tile, no loader waves"),
    dict(shape=(2, 13, 130, 7, 12), env={"MV_CONV_SHAPE": "0", "MV_CONV_SPEC42": "1"}, slices=1, slice_channels=13, kernel="k_conv3x3_gen", why="4x2 tile, loader waves, cin = 13"),
    dict(shape=(2, 8, 40, 14, 14), env={"MV_CONV_SHAPE": "1"}, slices=1, slice_channels=8, kernel="k_conv3x3_gen", why="2x1 tile"),
    dict(shape=(1, 5, 33, 7, 13), env={"MV_CONV_SHAPE": "1"}, slices=1, slice_channels=5, kernel="k_conv3x3_gen", why="2x1 tile, general staging"),
    dict(shape=(2, 20, 64, 8, 16), env={"MV_CONV_SHAPE": "2", "MV_CONV_DENSE": "1"}, slices=1, slice_channels=20, kernel="k_conv3x3_gen", why="1x1 tile, dense form"),
    dict(shape=(1, 8, 32, 7, 13), env={"MV_CONV_SHAPE": "2", "MV_CONV_DENSE": "1"}, slices=1, slice_channels=8, kernel="k_conv3x3_gen", why="dense form, ragged edge anchored at w - 4"),
    dict(shape=(2, 4, 64, 9, 5), env={"MV_CONV_SHAPE": "2", "MV_CONV_DENSE": "1"}, slices=1, slice_channels=4, kernel="k_conv3x3_gen", why="dense form, w = 5"),
    dict(shape=(1, 8, 32, 7, 13), env={"MV_CONV_SHAPE": "2", "MV_CONV_DENSE": "0"}, slices=1, slice_channels=8, kernel="k_conv3x3_gen", why="first small-launch form, ragged"),
    dict(shape=(1, 4, 33, 5, 12), env={"MV_CONV_SHAPE": "2", "MV_CONV_DENSE": "0"}, slices=1, slice_channels=4, kernel="k_conv3x3_gen", why="first small-launch form, cout = 33"),
    # a batch the image-stacking group does not divide
    dict(shape=(5, 8, 40, 14, 14), env={"MV_CONV_GROUP": "3"}, slices=1, slice_channels=8, kernel="k_conv3x3_gen", why="groups of 3 over 5 images"),
    dict(shape=(5, 8, 40, 14, 14), env={"MV_CONV_GROUP": "64"}, slices=1, slice_channels=8, kernel="k_conv3x3_gen", why="one group of 5"),
    dict(shape=(7, 16, 32, 7, 12), env={"MV_CONV_GROUP": "3"}, slices=1, slice_channels=16, kernel="k_conv3x3_gen", why="groups of 3 over 7 images"),
    dict(shape=(7, 16, 32, 7, 12), env={"MV_CONV_GROUP": "64"}, slices=1, slice_channels=16, kernel="k_conv3x3_gen", why="one group of 7"),
    # k_conv3x3 for maps wider than 510 pixels: vec_rows (conv3x3_mfma.hip) needs w % 4 == 0 and a 16-byte x
    dict(shape=(2, 3, 5, 4, 514), env={}, slices=1, slice_channels=3, kernel="k_conv3x3", why="w > 510, w % 4 != 0: vec_rows = 0 by shape"),
    dict(shape=(1, 4, 70, 3, 1032), env={}, slices=1, slice_channels=4, kernel="k_conv3x3", why="w > 510, w % 4 == 0: vec_rows by pointer"),
    dict(shape=(1, 4, 70, 3, 1030), env={}, slices=1, slice_channels=4, kernel="k_conv3x3", why="w > 510, w % 4 != 0"),
    # k_conv3x3_c3: cin = 3, cout <= 64, w % 4 == 0 and a 16-byte y; otherwise k_conv3x3_gen
    dict(shape=(2, 3, 64, 9, 16), env={}, slices=1, slice_channels=3, kernel="k_conv3x3_c3", why="full channel tiles; vec_rows by x"),
    dict(shape=(1, 3, 33, 5, 260), env={}, slices=1, slice_channels=3, kernel="k_conv3x3_c3", why="two column tiles (w > 256), cout = 33"),
    dict(shape=(1, 3, 8, 17, 12), env={}, slices=1, slice_channels=3, kernel="k_conv3x3_c3", why="ragged band height"),
    dict(shape=(1, 3, 8, 6, 13), env={}, slices=1, slice_channels=3, kernel="k_conv3x3_gen", why="w % 4 != 0: the c3 kernel's fallback"),
]

# mv_conv3x3_bias_relu_u8norm_f32: (n, cout, h, w); always k_conv3x3_c3; y odd or w % 4 != 0 is MV_ERR_UNSUPPORTED
CONV3X3_U8NORM = [(2, 64, 9, 16), (1, 33, 5, 260), (1, 8, 17, 12)]
CONV3X3_U8NORM_REFUSED_WIDTH = (1, 8, 6, 13)

# ---- mv_linear_bias_relu_f32 / _ws_f32 (csrc/linear_mfma.hip) ---------------------------------------------------------------------
# shape = (n, k, m); slices / slice_len / workspace as mv_linear_k_slices and mv_linear_workspace_bytes state them; kernel: the
# label with every pointer aligned, through the _ws entry point (k_linear_gemv needs n <= 4, k % 4 == 0 and 16-byte x and w:
# an odd x or w reroutes to k_linear)
LINEAR = [
    dict(shape=(5, 300, 70), slices=1, slice_len=320, workspace=0, kernel="k_linear", why="k % 4 == 0: vec_x / vec_w by pointer; m % 4 != 0"),
    dict(shape=(130, 257, 33), slices=1, slice_len=288, workspace=0, kernel="k_linear", why="k % 4 != 0; n past four 32-row tiles; m = 33"),
    dict(shape=(33, 2049, 129), slices=8, slice_len=288, workspace=136224, kernel="k_linear_reduce", why="sliced, k % 4 != 0, m past a 128-row block"),
    dict(shape=(5, 2048, 36), slices=8, slice_len=256, workspace=5760, kernel="k_linear_reduce", why="sliced, k % 4 == 0 and m % 4 == 0: vec_y by the workspace pointer"),
    dict(shape=(3, 100, 129), slices=1, slice_len=128, workspace=0, kernel="k_linear_gemv", why="gemv, m past a 128-row block"),
    dict(shape=(2, 68, 260), slices=1, slice_len=96, workspace=0, kernel="k_linear_gemv", why="gemv, a 4-k ragged stage"),
    dict(shape=(4, 100, 130), slices=1, slice_len=128, workspace=0, kernel="k_linear_gemv", why="gemv at its largest batch, m past a 128-row block, one chain"),
    dict(shape=(4, 1028, 130), slices=4, slice_len=288, workspace=8320, kernel="k_linear_reduce", why="gemv sliced, k % 4 == 0, m past a 128-row block"),
    dict(shape=(4, 1030, 130), slices=4, slice_len=288, workspace=8320, kernel="k_linear_reduce", why="n <= 4 with k % 4 != 0: k_linear sliced"),
]

# ---- the pools (csrc/cnn_ops.hip) ---------------------------------------------------------------------------------------------------
MAXPOOL2X2 = [(1, 7, 9), (5, 7, 9), (1, 6, 16), (5, 9, 24), (1, 2, 2), (5, 3, 30), (1, 1, 5)]  # (planes, h, w); w % 8 == 0: vec by pointer
MAXPOOL2D = [(1, 3, 3, 3, 2), (5, 13, 13, 3, 2), (1, 10, 12, 2, 2), (5, 9, 7, 4, 1)]  # (planes, h, w, k, stride)
AVGPOOL = [  # (planes, h, w, oh, ow), kernel
    ((1, 7, 7, 1, 1), "k_global_avgpool_small"), ((5, 7, 7, 1, 1), "k_global_avgpool_small"), ((5, 1, 1, 1, 1), "k_global_avgpool_small"),
    ((1, 5, 9, 1, 1), "k_global_avgpool_small"), ((300, 8, 8, 1, 1), "k_global_avgpool_small"),
    ((1, 9, 9, 1, 1), "k_adaptive_avgpool"), ((5, 9, 9, 1, 1), "k_adaptive_avgpool"), ((5, 14, 14, 7, 7), "k_adaptive_avgpool"),
    ((1, 14, 14, 7, 7), "k_adaptive_avgpool"), ((5, 5, 9, 3, 2), "k_adaptive_avgpool"),
]

# ---- mv_conv_norm_act_f32 (csrc/convnorm.hip) ----------------------------------------------------------------------------------------
# the stem, k_conv3x3_smallcin: (n, cin, cout, h, w, stride)
STEM = [(1, 3, 16, 33, 35, 2), (1, 2, 7, 1, 1, 1), (2, 3, 9, 2, 2, 2), (1, 4, 33, 6, 16, 1)]
# depthwise: (n, c, h, w, stride), the kernel with an aligned x, why
DEPTHWISE = [
    ((1, 5, 1, 1, 1), "k_dwpc3x3", "1 x 1 map"),
    ((1, 3, 2, 9, 2), "k_dwpc3x3", "stride 2, ragged"),
    ((1, 7, 13, 1, 2), "k_dwpc3x3", "one column"),
    ((1, 16, 15, 17, 2), "k_dwpc3x3", "stride 2, w = 17"),
    ((2, 8, 4, 16, 1), "k_dwpc3x3", "W % 4 == 0 and total % 64 == 0: `aligned` depends on x alone (stride 1)"),
    ((2, 16, 8, 16, 2), "k_dwpc3x3", "W % 8 == 0 and total % 64 == 0: `aligned` depends on x alone (stride 2)"),
    ((1, 7, 7, 7, 1), "k_dwpc3x3_small<7,s1>", "7 planes: the last workgroup is not full; odd x falls back to k_dwpc3x3"),
    ((1, 9, 3, 7, 2), "k_dwpc3x3_small<7,s2>", "h = 3, stride 2"),
    ((1, 11, 28, 14, 2), "k_dwpc3x3_small<14,s2>", "11 planes of 28 x 14"),
    ((1, 5, 9, 28, 1), "k_dwpc3x3_small<28,s1>", "w = 28"),
]
# pointwise: shape = (n, cin, cout, h, w); slices / slice_len as mv_conv1x1_k_slices states them; vec_w needs cin % 4 == 0,
# vec_x and vec_y need h * w % 4 == 0 (and 16-byte pointers, the residual included)
POINTWISE = [
    dict(shape=(2, 5, 3, 1, 1), slices=1, slice_len=5, why="hw = 1"),
    dict(shape=(2, 33, 130, 3, 5), slices=1, slice_len=33, why="hw = 15, cin = 33, two channel blocks"),
    dict(shape=(1, 130, 7, 6, 6), slices=1, slice_len=130, why="hw % 4 == 0, cin % 4 != 0: vec_x / vec_y by pointer"),
    dict(shape=(3, 8, 40, 4, 8), slices=1, slice_len=8, why="hw % 4 == 0 and cin % 4 == 0: every flag by pointer"),
    dict(shape=(64, 320, 40, 2, 2), slices=2, slice_len=160, why="K slices inside the workgroup, hw = 4"),
    dict(shape=(64, 960, 160, 3, 5), slices=4, slice_len=256, why="K slices, hw = 15, last slice shorter"),
]

# ---- mv_conv2d_bias_act_f32 (csrc/conv_igemm.hip; with a workspace csrc/deform.hip's plain im2col + k_conv1x1) -------------------
# shape = (n, cin, cout, h, w), k / stride / pad / dil pairs, groups.  Every row is a handful of workgroups, so
# mv_conv2d_needs_workspace answers 2: without a workspace k_conv_igemm's implicit form runs, with one (exactly
# mv_deform_conv2d_workspace_bytes of one image or of the batch) k_deform_im2col + k_conv1x1.  hw4 / k4: oh * ow % 4 == 0 and
# cin / groups * kh * kw % 4 == 0, the shape halves of vec_y and vec_w (conv_igemm.hip:265-266) -- where True the pointer decides.
CONV2D = [
    dict(shape=(1, 8, 12, 15, 17), k=(3, 5), stride=(2, 1), pad=(1, 2), dil=(2, 1), groups=4, hw4=False, k4=False, why="groups, dilation, anisotropic everything"),
    dict(shape=(3, 5, 7, 9, 9), k=(1, 1), stride=(1, 1), pad=(0, 0), dil=(1, 1), groups=1, hw4=False, k4=False, why="1 x 1, K = 5, two pixel tiles per image"),
    dict(shape=(1, 4, 6, 6, 6), k=(6, 6), stride=(1, 1), pad=(0, 0), dil=(1, 1), groups=2, hw4=False, k4=True, why="kernel = image: one output pixel; vec_w by pointer"),
    dict(shape=(5, 3, 8, 12, 12), k=(2, 2), stride=(1, 1), pad=(0, 0), dil=(1, 1), groups=1, hw4=False, k4=True, why="even kernel, batch 5; vec_w by pointer"),
    dict(shape=(2, 4, 8, 8, 8), k=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1), groups=1, hw4=True, k4=True, why="vec_w and vec_y by pointer alone"),
    dict(shape=(1, 3, 6, 6, 10), k=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1), groups=1,hw4=True, k4=False, why="vec_y by pointer, K = 27"),
    dict(shape=(2, 6, 70, 4, 8), k=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1), groups=2, hw4=True, k4=False, why="two groups of 35 channels: group pointers off 16 bytes, HW = 32"),
]

# ---- mv_deform_conv2d_f32 (csrc/deform_fused.hip, csrc/deform.hip) ----------------------------------------------------------------
# shape = (n, cin, cout, h, w), k / stride / pad / dil, groups, offset groups, mask, bias, scale of the normal offsets; needs =
# mv_deform_conv2d_needs_workspace: 2 = k_deform_fused without a workspace, the columns form (k_deform_im2col_lds, or
# k_deform_im2col where the LDS window of stride 2 x 2 outgrows 64 KiB, then k_conv1x1) with one; 1 = columns only (49 taps).
# ow4: ow % 4 == 0, the shape half of k_deform_fused's vec_y (deform_fused.hip:641).  far: one offset pair of +-1000 pixels.
DEFORM = [
    dict(shape=(1, 2, 3, 3, 3), k=(3, 3), stride=(1, 1), pad=(0, 0), dil=(1, 1), groups=1, og=1, mask=True, bias=True, scale=1.5, needs=2, ow4=False, far=False, why="single output pixel"),
    dict(shape=(1, 16, 8, 12, 12), k=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1), groups=1, og=1, mask=True, bias=True, scale=1.5, needs=2, ow4=True, far=True, why="3x3 / cb4, vec_y by pointer; far offsets"),
    dict(shape=(3, 6, 2, 5, 4), k=(3, 2), stride=(2, 1), pad=(1, 0), dil=(2, 1), groups=2, og=3, mask=True, bias=True, scale=1.5, needs=2, ow4=False, far=False, why="the reference test's configuration, batch 3"),
    dict(shape=(2, 8, 12, 8, 16), k=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1), groups=1, og=2, mask=False, bias=False, scale=3.0, needs=2, ow4=True, far=True, why="2 offset groups, no mask, no bias"),
    dict(shape=(2, 4, 6, 9, 10), k=(3, 3), stride=(2, 2), pad=(1, 1), dil=(1, 1), groups=2, og=1, mask=True, bias=True, scale=1.5, needs=2, ow4=False, far=True, why="stride 2 x 2: with a workspace the direct gather k_deform_im2col"),
    dict(shape=(2, 4, 4, 12, 12), k=(7, 7), stride=(1, 1), pad=(3, 3), dil=(1, 1), groups=1, og=2, mask=True, bias=True, scale=1.5, needs=1, ow4=True, far=False, why="49 taps: columns only, refused without a workspace"),
]

# ---- mv_inverted_residual_f32 (csrc/invres.hip): values ----------------------------------------------------------------------------
# block = (cin, hidden, cout, side, stride); plans = {batch: (slices, slice_len, workspace bytes)} as
# mv_inverted_residual_k_slices and mv_inverted_residual_workspace_bytes state them.  k_invres regions hold one image (28 and 14
# pixels) or two (7 pixels): batches 1, 2 and 3 are one image, the images-per-region count + 1, and a batch that leaves a 7 x 7
# region with one image.  Several slices go through the workspace and k_invres_reduce, whose total is n * cout * ow * ow (7840 =
# the smallest: 160 planes of 7 x 7, which 4-output groups straddle); one slice (a region per CU) writes y from the fused kernel.
INVRES = [
    dict(block=(160, 960, 160, 7, 1), kernel="k_invres<7,s1,", plans={1: (30, 32, 940800), 2: (30, 32, 1881600), 3: (30, 32, 2822400)}, why="two images per region; + x"),
    dict(block=(64, 384, 64, 14, 1), kernel="k_invres<14,s1,", plans={1: (12, 32, 602112), 3: (12, 32, 1806336)}, why="14 x 14, + x"),
    dict(block=(96, 576, 160, 14, 2), kernel="k_invres<14,s2,", plans={1: (18, 32, 564480), 2: (18, 32, 1128960)}, why="14 -> 7, reduce over 7 x 7 planes"),
    dict(block=(32, 192, 32, 28, 1), kernel="k_invres<28,s1,", plans={1: (6, 32, 602112), 3: (6, 32, 1806336), 64: (1, 192, 0)}, why="4 strips of 7 rows; batch 64: one chain, no workspace"),
    dict(block=(32, 192, 64, 28, 2), kernel="k_invres<28,s2,", plans={1: (6, 32, 301056), 2: (6, 32, 602112)}, why="28 -> 14, 2 strips"),
    dict(block=(24, 72, 20, 56, 1), kernel="k_invres_wide<56,s1,", plans={1: (3, 32, 752640), 32: (1, 72, 0)}, why="ragged hidden channels (72) and cout (20) in 32-wide tiles"),
    dict(block=(32, 32, 16, 112, 1), kernel="k_invres_wide<112,s1,", plans={1: (1, 32, 0)}, why="no expansion: hidden == cin, w_expand = a1 = b1 = NULL"),
]

# ---- mv_inverted_residual_f32 (csrc/invres.hip): the alignment refusals --------------------------------------------------------------
# (n, cin, hidden, cout, h, w, stride), slices, slice_len, workspace bytes
INVRES_REFUSAL = dict(shape=(1, 32, 192, 32, 28, 28, 1), slices=6, slice_len=32, workspace=602112)
INVRES_MESSAGE = "inverted_residual: x, y, the 1x1 weights and the workspace must be 16-byte aligned"
