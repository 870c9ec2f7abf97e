"""The host side of mv_deform_conv2d_f32, mv_conv2d_bias_act_f32 and mv_conv2d_affine_act_f32 at the C ABI, without a GPU: which
status each rejected call returns, the exact mv_last_error() text, the order in which a call with several faults reports them,
and what the three workspace queries answer.  Every call here is rejected, or returns at n == 0, before any launch; the
"pointers" are small integers that nothing dereferences.  Statuses and texts are part of the ABI: the literals pin them while the
host code behind the entries is reorganised."""
import pytest

from cpu_vision_amd import _lib

D, B, A = "mv_deform_conv2d_f32", "mv_conv2d_bias_act_f32", "mv_conv2d_affine_act_f32"
ALL = (D, B, A)
PTR = {name: (i + 1) << 24 for i, name in enumerate(("x", "weight", "offset", "mask", "bias", "alpha", "beta", "residual", "y"))}
# a valid call (2 x 4 x 8 x 8 -> 6 channels, 3x3, padding 1): every row below breaks it somewhere
BASE = dict(PTR, n=2, cin=4, h=8, w=8, cout=6, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, groups=1, offset_groups=1,
            use_mask=0, affine=0, act=1, workspace=None, workspace_bytes=0)
NULLS = dict.fromkeys(PTR)
DEFORM_7X7 = dict(n=64, cin=8, cout=8, h=20, w=20, kh=7, kw=7, ph=3, pw=3)     # 49 taps: no fused kernel
FAR = dict(x=1 << 40, weight=2 << 40, residual=3 << 40, y=4 << 40)             # tensors of GBs that do not overlap
LONG_K = dict(n=1, cin=65536, cout=1, h=1, w=1, kh=1, kw=1, ph=0, pw=0)        # K = 65536: outside the implicit kernel


def call(entry, **changes):
    """(status, mv_last_error()) of one entry with BASE's arguments except `changes`."""
    a = dict(BASE, **changes)
    geometry = [a[k] for k in ("kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw", "groups")]
    shape = [a["n"], a["cin"], a["h"], a["w"], a["cout"]]
    tail = [a["workspace"], a["workspace_bytes"], None]
    if entry == D:
        args = [a[k] for k in ("x", "weight", "offset", "mask", "bias", "y")] + shape + geometry + [a["offset_groups"], a["use_mask"]] + tail
    elif entry == B:
        args = [a[k] for k in ("x", "weight", "bias", "y")] + shape + geometry + [a["act"]] + tail
    else:
        args = [a[k] for k in ("x", "weight", "bias", "alpha", "beta", "residual", "y")] + shape + geometry + [a["affine"], a["act"]] + tail
    lib = _lib.load()
    status = getattr(lib, entry)(*args)
    return status, lib.mv_last_error().decode()


# (entries, what differs from BASE, status, mv_last_error())
REJECTED = [
    ((D,), dict(n=-1), -1, 'bad deform_conv2d shape n=-1 cin=4 cout=6'),
    ((B, A), dict(n=-1), -1, 'bad conv2d shape n=-1 cin=4 cout=6'),
    ((D,), dict(cin=0), -1, 'bad deform_conv2d shape n=2 cin=0 cout=6'),
    ((B, A), dict(cin=0), -1, 'bad conv2d shape n=2 cin=0 cout=6'),
    ((D,), dict(cout=0), -1, 'bad deform_conv2d shape n=2 cin=4 cout=0'),
    ((B, A), dict(cout=0), -1, 'bad conv2d shape n=2 cin=4 cout=0'),
    (ALL, dict(kh=0), -1, 'bad deform_conv2d shape (8, 8) kernel (0, 3)'),
    (ALL, dict(h=0), -1, 'bad deform_conv2d shape (0, 8) kernel (3, 3)'),
    (ALL, dict(sw=0), -1, 'stride_h: 1 stride_w: 0'),
    (ALL, dict(ph=-1), -1, 'pad_h: -1 pad_w: 1'),
    (ALL, dict(dh=0), -1, 'dil_h: 0 dil_w: 1'),
    (ALL, dict(kh=11, kw=11), -1, 'Calculated output size too small - out_h: 0 out_w: 0'),
    ((D,), dict(groups=3), -1, 'channels (4 -> 6) must divide into 3 weight groups and 1 offset groups'),
    ((B, A), dict(groups=3), -1, 'channels (4 -> 6) must divide into 3 groups'),
    ((D,), dict(groups=4), -1, 'channels (4 -> 6) must divide into 4 weight groups and 1 offset groups'),
    ((B, A), dict(groups=4), -1, 'channels (4 -> 6) must divide into 4 groups'),
    ((D,), dict(groups=0), -1, 'channels (4 -> 6) must divide into 0 weight groups and 1 offset groups'),
    ((B, A), dict(groups=0), -1, 'channels (4 -> 6) must divide into 0 groups'),
    ((D,), dict(offset_groups=3), -1, 'channels (4 -> 6) must divide into 1 weight groups and 3 offset groups'),
    ((D,), dict(offset_groups=0), -1, 'channels (4 -> 6) must divide into 1 weight groups and 0 offset groups'),
    ((B,), dict(act=5), -1, 'bad activation code 5'),
    ((A,), dict(act=5), -1, 'bad affine (0) / activation (5) code'),
    ((B,), dict(act=-1), -1, 'bad activation code -1'),
    ((A,), dict(act=-1), -1, 'bad affine (0) / activation (-1) code'),
    ((A,), dict(affine=3), -1, 'bad affine (3) / activation (1) code'),
    (ALL, dict(x=None), -1, 'null pointer'),
    (ALL, dict(weight=None), -1, 'null pointer'),
    (ALL, dict(y=None), -1, 'null pointer'),
    ((D,), dict(offset=None), -1, 'null pointer'),
    ((D,), dict(use_mask=1, mask=None), -1, 'null pointer'),
    ((A,), dict(affine=2, alpha=None), -1, 'affine without alpha / beta'),
    ((A,), dict(affine=1, beta=None), -1, 'affine without alpha / beta'),
    ((A,), dict(y=PTR['x']), -1, 'output must not overlap input, weight or residual'),
    ((A,), dict(y=PTR['x'] + 4 * (2 * 4 * 8 * 8 - 1)), -1, 'output must not overlap input, weight or residual'),
    ((A,), dict(y=PTR['weight']), -1, 'output must not overlap input, weight or residual'),
    ((A,), dict(y=PTR['residual']), -1, 'output must not overlap input, weight or residual'),
    ((A,), dict(y=PTR['residual'] - 4 * (2 * 6 * 8 * 8 - 1)), -1, 'output must not overlap input, weight or residual'),
    ((D,), dict(n=-1, kh=0), -1, 'bad deform_conv2d shape n=-1 cin=4 cout=6'),
    ((B, A), dict(n=-1, kh=0), -1, 'bad conv2d shape n=-1 cin=4 cout=6'),
    ((D,), dict(cout=0, sh=0), -1, 'bad deform_conv2d shape n=2 cin=4 cout=0'),
    ((B, A), dict(cout=0, sh=0), -1, 'bad conv2d shape n=2 cin=4 cout=0'),
    (ALL, dict(kh=0, sw=0), -1, 'bad deform_conv2d shape (8, 8) kernel (0, 3)'),
    (ALL, dict(sw=0, ph=-1), -1, 'stride_h: 1 stride_w: 0'),
    (ALL, dict(ph=-1, dw=0), -1, 'pad_h: -1 pad_w: 1'),
    (ALL, dict(dw=0, kh=11), -1, 'dil_h: 1 dil_w: 0'),
    (ALL, dict(kh=11, groups=3), -1, 'Calculated output size too small - out_h: 0 out_w: 8'),
    ((B, A), dict(groups=3, act=5), -1, 'channels (4 -> 6) must divide into 3 groups'),
    ((A,), dict(groups=3, affine=3), -1, 'channels (4 -> 6) must divide into 3 groups'),
    ((B,), dict(act=5, x=None), -1, 'bad activation code 5'),
    ((A,), dict(act=5, x=None), -1, 'bad affine (0) / activation (5) code'),
    ((D,), dict(offset_groups=3, x=None), -1, 'channels (4 -> 6) must divide into 1 weight groups and 3 offset groups'),
    ((A,), dict(x=None, affine=2, alpha=None), -1, 'null pointer'),
    ((A,), dict(affine=2, alpha=None, y=PTR['x']), -1, 'affine without alpha / beta'),
    ((A,), dict(y=PTR['x'], **LONG_K), -1, 'output must not overlap input, weight or residual'),
    ((D,), dict(DEFORM_7X7), -1, "deform_conv2d: workspace of at least 627200 bytes (one image's columns) needed, got 0"),
    ((D,), dict(DEFORM_7X7, workspace=1 << 30, workspace_bytes=8 * 49 * 400 * 4 - 1), -1, "deform_conv2d: workspace of at least 627200 bytes (one image's columns) needed, got 627199"),
    ((B, A), dict(LONG_K), -1, "deform_conv2d: workspace of at least 262144 bytes (one image's columns) needed, got 0"),
    ((B, A), dict(LONG_K, workspace=1 << 30, workspace_bytes=65536 * 4 - 4), -1, "deform_conv2d: workspace of at least 262144 bytes (one image's columns) needed, got 262140"),
    ((A,), dict(LONG_K, affine=2, residual=None), -1, "deform_conv2d: workspace of at least 262144 bytes (one image's columns) needed, got 0"),
    # one group image of exactly 2^30 elements (K, the output plane and its width all inside the implicit kernel's ranges): the kernel's
    # 32-bit byte offsets into an image end there; 357 x 1000000 x 3 = 2^30 - 2741824 elements is taken (tests/test_gpu_large_offsets.py)
    ((B, A), dict(FAR, n=1, cin=1024, cout=8, h=1024, w=1024, kh=3, kw=3, sh=2, sw=2, ph=1, pw=1), -2,
     "conv2d (implicit GEMM): one image of a group has 2^30 elements or more"),
    ((B, A), dict(FAR, n=1, cin=2048, cout=8, groups=2, h=1024, w=1024, kh=3, kw=3, sh=2, sw=2, ph=1, pw=1), -2,
     "conv2d (implicit GEMM): one image of a group has 2^30 elements or more"),
]


@pytest.mark.parametrize("row", range(len(REJECTED)), ids=lambda i: f"{i}: {sorted(REJECTED[i][1])}")
def test_rejected_calls_return_the_same_status_and_text(row):
    entries, changes, status, text = REJECTED[row]
    assert status != 0
    for entry in entries:
        assert call(entry, **changes) == (status, text), entry


def test_an_empty_batch_returns_before_the_pointers_are_looked_at():
    for entry in ALL:
        assert call(entry, n=0, **NULLS)[0] == 0
        assert call(entry, n=0, **NULLS, use_mask=1, affine=2)[0] == 0
        assert call(entry, n=0, **NULLS, kh=0)[0] == -1  # ... but after the shape checks


def test_workspace_queries():
    lib = _lib.load()
    deform, conv, nbytes = lib.mv_deform_conv2d_needs_workspace, lib.mv_conv2d_needs_workspace, lib.mv_deform_conv2d_workspace_bytes
    # 0 = the direct form (fused / implicit), 1 = the columns workspace is required, 2 = optional (a small launch)
    assert deform(8, 256, 256, 64, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1) == 0
    assert deform(1, 256, 256, 64, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1) == 2
    assert deform(3, 6, 2, 5, 4, 3, 2, 2, 1, 1, 0, 2, 1, 2, 3) == 2
    assert deform(64, 8, 8, 20, 20, 7, 7, 1, 1, 3, 3, 1, 1, 1, 1) == 1
    assert deform(64, 8, 8, 200, 200, 3, 3, 9, 9, 1, 1, 1, 1, 1, 1) == 1
    assert deform(64, 7, 8, 20, 20, 3, 3, 1, 1, 1, 1, 1, 1, 2, 1) == 1      # bad channel split
    assert deform(64, 8, 8, 20, 20, 3, 3, 0, 1, 1, 1, 1, 1, 1, 1) == 1      # stride_h = 0
    assert deform(0, 8, 8, 20, 20, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1) == 1       # no images
    assert conv(64, 64, 64, 56, 56, 3, 3, 1, 1, 1, 1, 1, 1, 1) == 0
    assert conv(1, 65536, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1) == 1          # K = 65536
    assert conv(1, 64, 64, 14, 14, 3, 3, 1, 1, 1, 1, 1, 1, 1) == 2          # 4 workgroups
    assert conv(3, 4, 6, 5, 5, 3, 3, 1, 1, 1, 1, 1, 1, 2) == 2
    assert conv(1, 64, 64, 14, 14, 0, 3, 1, 1, 1, 1, 1, 1, 1) == 1          # kh = 0
    assert conv(64, 64, 64, 56, 56, 3, 3, 1, 1, 1, 1, 1, 1, 3) == 1         # groups do not divide
    assert nbytes(2, 4, 8, 8, 3, 3, 1, 1, 0, 0, 1, 1) == 2 * 4 * 9 * 36 * 4
    assert nbytes(1, 4, 5, 5, 3, 3, 1, 1, 1, 1, 1, 1) == 4 * 9 * 25 * 4
    assert nbytes(2, 4, 8, 8, 3, 3, 1, 1, 0, 0, 0, 1) == 0                  # dilation_h = 0
    assert nbytes(0, 4, 8, 8, 3, 3, 1, 1, 0, 0, 1, 1) == 0
