/*
 * mi355vision.h -- C ABI of libmi355vision.so: the MI355X (gfx950) implementation of the
 * reference's data-parallel filtering / first-conv hot path.
 *
 * This is the drop-in boundary.  The reference (a torchvision 0.20 fork) is Python; its
 * "FFI" for this path is the pair of torch calls every filter kernel makes,
 *     torch.nn.functional.pad(x, [kx//2, kx//2, ky//2, ky//2], mode="reflect")
 *     torch.nn.functional.conv2d(x, kernel.expand(C,1,ky,kx), groups=C)
 * (transforms/v2/functional/_misc.py:153-155, _color.py:260,
 *  transforms/_functional_tensor.py:759-761, 818) and nn.Conv2d(3,64,3,padding=1)+ReLU
 * (models/vgg.py:81-85).  Each entry point below replaces one such call site (cited per
 * function, paths relative to the reference root).  The reference-side binding a maintainer
 * would add is the ctypes stub shown in INTEGRATION.md; cpu-vision_amd/_lib.py is that stub.
 *
 * Conventions (all entry points):
 *   - plain C: pointers + sizes, no torch / C++ types.
 *   - x, y, ... are DEVICE pointers owned by the caller; the library never allocates, frees or
 *     retains them.  Outputs must not alias inputs.
 *   - images are planar, contiguous: `planes` = product of all leading dims (N*C), each plane
 *     H x W, W fastest (the reference's NCHW layout).
 *   - filter taps are HOST pointers (a handful of floats, passed to the kernel by value),
 *     unless a parameter says otherwise.
 *   - `stream` is a hipStream_t (NULL = the null stream).  Calls are asynchronous with respect
 *     to the host, exactly like a torch op on that stream.
 *   - return 0 on success, a negative mv_status otherwise; mv_last_error() gives the message
 *     for the calling thread.  Nothing throws or aborts across this boundary.
 *   - re-entrant; no global mutable state besides the thread-local error / last-kernel strings, and no
 *     environment lookups: kernel selection depends on the arguments alone.
 *   - alignment, filter entry points (everything from mv_depthwise_conv2d_f32 down to the *_v entries): x, y / gx / gy, every
 *     frame of a *_v list and a device tap array need the alignment of their element type only (a contiguous view at any
 *     element offset of an allocation is fine); the workspace of mv_gaussian_blur_u8_ws must be 16-byte aligned
 *     (MV_ERR_INVALID_ARGUMENT otherwise), its content on entry does not matter.  Every output is written whole; nothing outside the outputs and the stated workspace size is
 *     written, and no value from outside an input reaches a result.  Alignment buys speed only: with W % 4 == 0 and x and y
 *     aligned to 4 pixels (16 bytes float32, 8 half types, 4 uint8) the 4-pixel kernels take their vector instantiation
 *     ("vec16" in mv_last_kernel()), and mv_separable_blur_f32 / mv_gaussian_sobel_f32 take k_sepfast only on 16-byte pointers.
 *   - alignment, CNN layer entry points (mv_conv3x3_bias_relu_*, mv_linear_bias_relu_*, the pools, mv_conv_norm_act_f32,
 *     mv_conv2d_bias_act_f32, mv_conv2d_affine_act_f32, mv_deform_conv2d_f32): every tensor -- x, weights, bias, alpha, beta, residual, offset, mask, y --
 *     needs the alignment of its element type only, and a workspace 4 bytes (mv_linear_bias_relu_ws_f32 checks it:
 *     MV_ERR_INVALID_ARGUMENT otherwise); a workspace's content on entry does not matter.  Every output is written whole, nothing
 *     outside y and the stated workspace size is written, and no value from outside an input reaches a result.  Alignment buys
 *     speed only -- each launcher tests its pointers once per launch and takes 16-byte loads / stores where the pointer is
 *     16-byte aligned and the shape keeps every row so (k % 4, cin % 4, h * w % 4, w % 4 or w % 8 == 0), the same kernel element
 *     by element otherwise, with the same bits -- except where another KERNEL is chosen:
 *       mv_conv3x3_bias_relu_f32 / _ws_f32, cin == 3: the first-layer kernel (k_conv3x3_c3) needs w % 4 == 0 and a 16-byte y;
 *         otherwise the general kernel runs (same bits);
 *       mv_conv3x3_bias_relu_u8norm_f32: has no other kernel -- w % 4 != 0 or a y that is not 16-byte aligned returns
 *         MV_ERR_UNSUPPORTED and writes nothing (x, uint8, may start at any byte);
 *       mv_linear_bias_relu_*: the batch <= 4 kernel (k_linear_gemv) needs k % 4 == 0 and 16-byte x and w, else k_linear runs;
 *       mv_conv_norm_act_f32, MV_CONV_DW3X3 on 7 / 14 / 28-pixel-wide maps: k_dwpc3x3_small needs a 16-byte x, else k_dwpc3x3 runs.
 *     mv_inverted_residual_f32 is the one layer with a 16-byte requirement: x, y, w_expand, w_project and the workspace
 *     (MV_ERR_INVALID_ARGUMENT, "inverted_residual: x, y, the 1x1 weights and the workspace must be 16-byte aligned", nothing
 *     written); w_dw and the six norm vectors need 4 bytes.  The columns workspace of mv_conv2d_bias_act_f32 and
 *     mv_deform_conv2d_f32 needs 4 bytes and may hold one image's columns or more (one pass per as many images as fit); a
 *     mv_deform_conv2d_f32 geometry without a fused kernel called with no or too small a workspace returns
 *     MV_ERR_INVALID_ARGUMENT ("... workspace of at least N bytes ...") and writes nothing.
 *   - numerics: fp32 taps and accumulation, one fused multiply-add chain per output in
 *     row-major tap order starting from +0 (bit-identical to oracle/oracle.c); uint8 paths
 *     convert to fp32, accumulate, round half-to-even (torch.round_) and narrow.
 *   - NaN and Inf: every tap of a filter is multiplied, a zero tap included (Sobel's centre column and row: an Inf under one
 *     gives NaN, as conv2d with those weights does), and nothing else is: zero padding, the padding of a kernel, a channel
 *     count or a K chunk to a tile, and cells staged for a neighbouring tile never reach an output, so a NaN or an Inf shows
 *     exactly in the outputs whose receptive field holds it.  An activation or clamp passes NaN and turns +-Inf into its bound.
 *     Grid sampling (mv_warp_*, mv_elastic_*), as torch's CPU grid_sample with zero padding: a NaN or infinite SOURCE COORDINATE
 *     (a perspective whose denominator is 0 inside the output) reads no cell -- a nearest sample is then 0 (or the fill), a
 *     bilinear sample NaN (its weights are NaN); a bilinear sample reads its four cells with their weights, a weight of 0 too.
 *     adjust_hue on a pixel with a NaN or infinite channel has no hue (Inf - Inf): all three channels become NaN.  (The
 *     reference picks the output sector from int(NaN), which differs between hosts.)
 */
#ifndef MI355VISION_H
#define MI355VISION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MV_ABI_VERSION 1

typedef enum mv_status {
  MV_OK = 0,
  MV_ERR_INVALID_ARGUMENT = -1, /* shapes / sizes / enum values the reference would also reject   */
  MV_ERR_UNSUPPORTED = -2,      /* valid request outside what the kernels cover (message says what) */
  MV_ERR_LAUNCH = -3,           /* HIP reported an error at launch                                 */
  MV_ERR_NO_DEVICE = -4         /* no gfx950 device visible                                        */
} mv_status;

typedef enum mv_border {
  MV_BORDER_VALID = 0,   /* no padding: output (H-ky+1) x (W-kx+1)      -- _color.py:260          */
  MV_BORDER_REFLECT = 1, /* pad(mode="reflect") then conv: output H x W  -- _misc.py:153-155       */
  MV_BORDER_ZERO = 2     /* zero padding k//2: output H x W              -- nn.Conv2d(padding=k//2) */
} mv_border;

/* Largest 2-D tap count that may be passed from a host pointer (by-value kernel argument). */
#define MV_MAX_HOST_TAPS_2D 121
/* Largest 1-D kernel size of the Gaussian / separable entry points. */
#define MV_MAX_TAPS_1D 63

int mv_abi_version(void);
const char* mv_last_error(void);
/* Name of the kernel instantiation the calling thread's last entry point launched (e.g.
 * "k_dwtile<f32,3x3,rpt4,vec16,tw256>"): what a benchmark reports next to its roofline numbers, taken from the
 * launcher that made the choice instead of being assumed by the caller.  "" before the first launch. */
const char* mv_last_kernel(void);
/* Identifies the build: first 16 hex digits of the SHA-256 over the library's sources and compile flags
 * ("+tuning" appended for a -DMV_TUNING build, the only kind that reads MV_* environment knobs). */
const char* mv_build_id(void);
/* Number of visible HIP devices (does not create a context). */
int mv_device_count(void);

/* ---- the primitive ------------------------------------------------------------------------
 * y = conv2d(pad(x, border), w.expand(C,1,ky,kx), groups=C): depthwise cross-correlation with one
 * (ky,kx) kernel shared by all planes.  Replaces the pad+conv2d pair at _misc.py:153-155 /
 * _functional_tensor.py:759-761 (REFLECT) and the bare conv2d at _color.py:260 (VALID).
 * `w`: ky*kx floats, row-major; host pointer when w_on_device == 0 (ky*kx <= MV_MAX_HOST_TAPS_2D),
 * device pointer otherwise.  REFLECT requires ky/2 < H and kx/2 < W (as ATen does). */
int mv_depthwise_conv2d_f32(const float* x, float* y, const float* w, int w_on_device, int64_t planes,
                            int h, int wdt, int ky, int kx, int border, void* stream);
/* Same with uint8 storage: x.to(float32) -> conv -> round_() -> .to(uint8)
 * (_misc.py:150, 160-161; _functional_tensor.py:516-542). */
int mv_depthwise_conv2d_u8(const uint8_t* x, uint8_t* y, const float* w, int w_on_device, int64_t planes,
                           int h, int wdt, int ky, int kx, int border, void* stream);

/* ---- gaussian_blur_image core (_misc.py:147-155, v1 _functional_tensor.py:746-764) -----------
 * kernel2d[j][i] = k1d_y[j] * k1d_x[i] (formed in-kernel, bit-identical to _misc.py:97), reflect
 * border, one 2-D pass exactly like the reference.  k1d_* are host pointers, kx, ky odd,
 * <= MV_MAX_TAPS_1D. */
int mv_gaussian_blur_f32(const float* x, float* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx,
                         const float* k1d_y, int ky, void* stream);
int mv_gaussian_blur_u8(const uint8_t* x, uint8_t* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx,
                        const float* k1d_y, int ky, void* stream);
/* mv_gaussian_blur_u8's result -- the reference's single 2-D pass: .to(float32) -> conv2d(outer-product kernel) -> round_() --
 * BIT FOR BIT, at the cost of the separable pair.  The separable sum is another association of the 2-D chain; the two differ by
 * at most M = (kx*ky + kx + ky + 2) * 2^-17 on uint8 data with Gaussian taps, so their roundings agree wherever the value is
 * farther than M from a tie n + 0.5.  Pass 1 (the separable kernel) stores every pixel and lists the lane-rows (16 / 4 / 2
 * pixels) that hold a value within M of a tie -- 1-4 % of them -- in `workspace`; pass 2 recomputes those pixels with the 2-D
 * chain (csrc/tiefix_u8.hip has the bound's derivation; a list that overflows makes pass 2 recompute every pixel).
 * 32 x 4K uint8: 5x5 0.64 -> 0.59 ms, 7x7 1.2 -> 0.77, 9x9 1.68 -> 0.96, 15x15 ~20 -> 1.6, 23x23 49 -> 3.1 ms.
 * mv_gaussian_blur_u8_workspace_bytes() == 0:
 * the plain 2-D pass is as fast (fewer than 25 taps) or the size / width is outside the separable kernels (images narrower than 16
 * pixels ...) -- the call then IS mv_gaussian_blur_u8 and `workspace` may be NULL.  Taps must be non-negative with sum <= 1 (every Gaussian), else the 2-D
 * pass runs as well. */
int64_t mv_gaussian_blur_u8_workspace_bytes(int64_t planes, int h, int wdt, int kx, int ky);
int mv_gaussian_blur_u8_ws(const uint8_t* x, uint8_t* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx,
                           const float* k1d_y, int ky, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- separable filtering (BASELINE cfg3; two calls of the primitive fused into one kernel) ----
 * tmp = conv(pad_reflect(x), k1d_x as 1 x kx); y = conv(pad_reflect(tmp), k1d_y as ky x 1).
 * One HBM read + one HBM write per pixel; the intermediate lives in LDS. */
int mv_separable_blur_f32(const float* x, float* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx,
                          const float* k1d_y, int ky, void* stream);

/* fp16 / bf16 storage (the reference computes these dtypes natively, _misc.py:139-155): fp32 arithmetic in the 2-D tile
 * kernel, one round-to-nearest-even on store -- the bits of `.to(float32)` -> mv_gaussian_blur_f32's 2-D pass -> `.to(dtype)`
 * at 4 B per pixel of traffic instead of 20.  x, y: IEEE binary16 / bfloat16 planes.  Kernel sides up to 11
 * (MV_ERR_UNSUPPORTED beyond: convert and use the fp32 entry points). */
int mv_gaussian_blur_f16(const void* x, void* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx, const float* k1d_y,
                         int ky, void* stream);
int mv_gaussian_blur_bf16(const void* x, void* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx, const float* k1d_y,
                          int ky, void* stream);

/* float64 images.  The reference computes a float64 image in float64 -- taps (`_get_gaussian_kernel2d(..., dtype=dtype)`),
 * padding and conv2d (_misc.py:139-155); adjust_sharpness likewise (_color.py:246-275).  k1d_* are HOST arrays of doubles
 * (the reference's own float64 taps), kernel2d[j][i] = k1d_y[j] * k1d_x[i] in fp64; one fp64 fma chain per output in
 * row-major tap order.  mv_depthwise_conv2d_f64 takes the (ky, kx) taps as a DEVICE array (any odd size the 64 x 16 LDS
 * tile + halo holds: up to 63 x 63 and beyond for narrow kernels). */
int mv_gaussian_blur_f64(const double* x, double* y, int64_t planes, int h, int wdt, const double* k1d_x, int kx,
                         const double* k1d_y, int ky, void* stream);
int mv_depthwise_conv2d_f64(const double* x, double* y, const double* w_dev, int64_t planes, int h, int wdt, int ky, int kx,
                            int border, void* stream);
int mv_sharpness_f64(const double* x, double* y, int64_t planes, int h, int wdt, double sharpness_factor, int v1, void* stream);

/* uint8 storage, separable form (kernel sides up to 63, e.g. SimCLR-style GaussianBlur(23) on uint8 images): the separable
 * pair in fp32, then round_() and narrow (sides <= 7, and 9 x 9 / 9 x 7 / 7 x 9, on the 16-pixel-per-lane register kernel for
 * W >= 16; larger ones on the streaming kernel).  The reference evaluates one 2-D fp32 sum; the two differ by at most one
 * fp32 ulp before rounding, i.e. the uint8 results agree except at exact rounding ties (within the reference's own
 * atol = 1 for this op, test_transforms_v2.py:3309).  MV_ERR_UNSUPPORTED for sides <= 7 on images narrower than 16 pixels: use
 * mv_gaussian_blur_u8 there. */
int mv_separable_blur_u8(const uint8_t* x, uint8_t* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx,
                         const float* k1d_y, int ky, void* stream);

/* ---- Sobel gradient (BASELINE cfg3; the primitive with taps [[-1,0,1],[-2,0,2],[-1,0,1]] and
 * its transpose, both outputs from one read of x). */
int mv_sobel_f32(const float* x, float* gx, float* gy, int64_t planes, int h, int wdt, int border, void* stream);
/* cfg3 graph fused: separable Gaussian (reflect) then Sobel (reflect) of the blurred image;
 * x is read once, gx and gy are written once (36 B / pixel). */
int mv_gaussian_sobel_f32(const float* x, float* gx, float* gy, int64_t planes, int h, int wdt, const float* k1d_x,
                          int kx, const float* k1d_y, int ky, void* stream);

/* ---- adjust_sharpness_image (_color.py:229-280; v1 _functional_tensor.py:809-838) -------------
 * Valid 3x3 smoothing [[1,1,1],[1,5,1],[1,1,1]]/13, integer inputs rounded, blended with the
 * input (v2: x + (1-f)*(blur-x) as one fma; v1: f*x + (1-f)*blur), clamped to [0, bound];
 * border pixels pass through.  `sharpness_factor` is the Python double; the library narrows
 * (1 - f) to float exactly as ATen does.  H <= 2 or W <= 2 copies the input.
 * The f32 entry also serves the reference's other integer dtypes after a caller-side .to(float32):
 * `bound` is _max_value(dtype) (1.0 for floating images) and `integer_semantics` != 0 rounds the
 * blurred value half-to-even before the blend, as the integer path does (_color.py:261-263). */
int mv_sharpness_f32(const float* x, float* y, int64_t planes, int h, int wdt, double sharpness_factor, int v1,
                     float bound, int integer_semantics, void* stream);
int mv_sharpness_u8(const uint8_t* x, uint8_t* y, int64_t planes, int h, int wdt, double sharpness_factor, int v1,
                    void* stream);

/* ---- separately allocated frames, ONE launch (the samples a DataLoader hands to Transform.forward,
 * transforms/v2/_transform.py:40-55, are allocated one by one; a launch per 1080p frame is launch-bound).
 * xs / ys: HOST arrays of `nframes` DEVICE pointers, frame i being `planes_per_frame` contiguous h x w planes; every frame has
 * the same shape.  The pointers travel by value in the kernel arguments (no device allocation, no copy, graph-capturable);
 * lists longer than 112 frames take one launch per 112.  Results are those of the single-frame entry points, bit for bit.
 * Frame pointers that are not 16-byte aligned are served by one launch per frame. */
int mv_gaussian_blur_f32_v(const float* const* xs, float* const* ys, int nframes, int64_t planes_per_frame, int h, int wdt,
                           const float* k1d_x, int kx, const float* k1d_y, int ky, void* stream);
int mv_gaussian_blur_u8_v(const uint8_t* const* xs, uint8_t* const* ys, int nframes, int64_t planes_per_frame, int h, int wdt,
                          const float* k1d_x, int kx, const float* k1d_y, int ky, void* stream);
int mv_separable_blur_f32_v(const float* const* xs, float* const* ys, int nframes, int64_t planes_per_frame, int h, int wdt,
                            const float* k1d_x, int kx, const float* k1d_y, int ky, void* stream);
int mv_separable_blur_u8_v(const uint8_t* const* xs, uint8_t* const* ys, int nframes, int64_t planes_per_frame, int h, int wdt,
                           const float* k1d_x, int kx, const float* k1d_y, int ky, void* stream);
int mv_sharpness_f32_v(const float* const* xs, float* const* ys, int nframes, int64_t planes_per_frame, int h, int wdt,
                       double sharpness_factor, int v1, float bound, int integer_semantics, void* stream);
int mv_sharpness_u8_v(const uint8_t* const* xs, uint8_t* const* ys, int nframes, int64_t planes_per_frame, int h, int wdt,
                      double sharpness_factor, int v1, void* stream);

/* ---- first CNN layer: nn.Conv2d(cin, cout, 3, padding=1) [+ bias] [+ ReLU] (vgg.py:81-85,
 * ops/misc.py:97-119).  x (n,cin,h,w), w (cout,cin,3,3) and b (cout, may be NULL) are DEVICE
 * pointers (they are model parameters); y (n,cout,h,w).  Implicit GEMM on the fp32 MFMA
 * (v_mfma_f32_32x32x2_f32): exact fp32, K = cin*9 in (ci,dy,dx) order, bias as the last tap.  cin = 3 takes the
 * first-layer kernel (HBM-write-bound); any other cin the K-chunked kernel (MFMA-bound; feature maps up to 510
 * pixels wide). */
int mv_conv3x3_bias_relu_f32(const float* x, const float* w, const float* b, float* y, int64_t n, int cin, int h,
                             int wdt, int cout, int relu, void* stream);

/* ---- rest of the small CNNs' feature extractor ---------------------------------
 * nn.MaxPool2d(kernel_size=2, stride=2) (vgg.py:78-79): y is planes x (h/2) x (w/2), floor mode, NaN propagates. */
int mv_maxpool2x2_f32(const float* x, float* y, int64_t planes, int h, int wdt, void* stream);
/* nn.AdaptiveAvgPool2d((oh, ow)) (vgg.py:41): y is planes x oh x ow. */
int mv_adaptive_avgpool_f32(const float* x, float* y, int64_t planes, int h, int wdt, int oh, int ow, void* stream);

/* ---- Conv2dNormActivation (ops/misc.py:68-128) for the MobileNet family -----------------------
 * One kernel per block: conv2d (zero padding = (k-1)/2, no dilation) -> `+ bias` (may be NULL: the reference drops the
 * conv bias when a norm follows) -> folded norm -> `+ residual` (NULL or a tensor shaped like y: InvertedResidual's
 * `x + self.conv(x)`, models/mobilenetv2.py:61-63) -> activation.  All pointers are DEVICE pointers.
 *   kind    MV_CONV_DENSE3X3  w (cout, cin, 3, 3), cin <= 4: the stem (mobilenetv2.py:126)
 *           MV_CONV_DW3X3     w (c, 1, 3, 3), cin == cout == c: depthwise blocks (mobilenetv2.py:43-50)
 *           MV_CONV_PW1X1     w (cout, cin, 1, 1): pointwise convs (mobilenetv2.py:39-41, 52-53); fp32 MFMA
 *   stride  1 or 2 (1 for MV_CONV_PW1X1);  y is (n, cout, (h-1)/stride+1, (w-1)/stride+1)
 *   affine  MV_AFFINE_NONE;  MV_AFFINE_MUL_ADD = FrozenBatchNorm2d.forward (ops/misc.py:52-61): x*alpha then +beta
 *           (two roundings);  MV_AFFINE_FMA = nn.BatchNorm2d in eval mode (ATen): fma(x, alpha, beta) with
 *           (alpha, beta) from mv_fold_batchnorm
 *   act     MV_ACT_NONE / RELU / RELU6 / HARDSWISH / SILU */
#define MV_CONV_DENSE3X3 0
#define MV_CONV_DW3X3 1
#define MV_CONV_PW1X1 2
#define MV_AFFINE_NONE 0
#define MV_AFFINE_MUL_ADD 1
#define MV_AFFINE_FMA 2
#define MV_ACT_NONE 0
#define MV_ACT_RELU 1
#define MV_ACT_RELU6 2
#define MV_ACT_HARDSWISH 3
#define MV_ACT_SILU 4
int mv_conv_norm_act_f32(int kind, const float* x, const float* w, const float* bias, const float* alpha, const float* beta,
                         const float* residual, float* y, int64_t n, int cin, int h, int wdt, int cout, int stride,
                         int affine, int act, void* stream);
/* Summation order of a MV_CONV_PW1X1 call of this shape.  Large launches sum every output as ONE ascending-channel chain
 * (return value 1, *slice_len = cin).  Launches of few workgroups with long K (MobileNet's 7x7 / 14x14 layers) are latency-
 * bound as one chain; the kernel then walks K in `return value` slices of *slice_len channels (a multiple of 32; the last
 * slice may be shorter) with separate wave groups of one workgroup: each slice is an ascending chain from +0, the slices are
 * added in ascending order, then bias / norm / residual / activation.  Deterministic (no atomics, no workspace); within
 * 1e-6 relative of the single chain; oracle/oracle.c restates it (orc_pointwise_sliced_affine_act_f32). */
int mv_conv1x1_k_slices(int64_t n, int cin, int h, int wdt, int cout, int* slice_len);
/* ---- FeaturePyramidNetwork's top-down merge (ops/feature_pyramid_network.py:  inner_lateral = inner_block(x);
 * inner_top_down = F.interpolate(last_inner, size=feat_shape, mode="nearest"); last_inner = inner_lateral + inner_top_down) in ONE
 * launch:  y[i, co, oy, ox] = act(top[i, co, iy(oy), ix(ox)] + norm(conv1x1(x)[i, co, oy, ox] + bias[co])).
 *   x (n, cin, h, w), w (cout, cin), top (n, cout, top_h, top_w), y (n, cout, h, w); bias / alpha / beta / affine / act as for
 *   mv_conv_norm_act_f32 (bias may be NULL; alpha and beta are required iff affine != 0).  All DEVICE pointers.
 * The pointwise kernel of MV_CONV_PW1X1 with a second residual addressing: same tiles, same plan and the summation order
 * mv_conv1x1_k_slices(n, cin, h, w, cout) states; epilogue order `+ bias` -> folded norm -> `top + v` -> activation.  Bit for bit
 * mv_conv_norm_act_f32(MV_CONV_PW1X1, ..., residual = R) with R = interpolate(top, size=(h, w), mode="nearest"), without R in memory.
 * Source index per axis = ATen's CPU nearest_idx: min((int)floorf((float)o * scale), in - 1) with scale = (float)in / (float)out,
 * one float division on the host and a plain rounded product on the device; for out == in and out == 2 * in this is ATen's `o` and
 * `o >> 1`.  Any top_h, top_w >= 1: equal size, 1 x 1 and a coarser OUTPUT give torch's values too (the integer o * in / out does not:
 * 65 -> 110 differs).  Kernels: k_conv1x1_up<NT,MW[,ksN]> (mv_last_kernel).
 * Refused before any launch, with a negative status and the text in mv_last_error(): a bad shape, top_h or top_w < 1, unknown affine /
 * act codes, NULL x / w / y / top, affine without alpha / beta, y overlapping x, w or top, sizes beyond one launch (n > 65535, a plane
 * of 2^31 elements).  n == 0 is a successful no-op.  Alignment: 4 bytes for every tensor; y is stored with 16-byte stores where
 * h * w % 4 == 0 and y is 16-byte aligned, else element by element; top is read element by element, never past its last element. */
int mv_conv1x1_upsample_add_f32(const float* x, const float* w, const float* bias, const float* alpha, const float* beta,
                                const float* top, float* y, int64_t n, int cin, int h, int wdt, int cout, int top_h, int top_w,
                                int affine, int act, void* stream);
/* ---- InvertedResidual (models/mobilenetv2.py:39-63) as ONE kernel -------------------------------------------------------
 * [1x1 expand cin -> hidden + norm + ReLU6] -> 3x3 depthwise (stride 1 | 2, zero padding 1) + norm + ReLU6 -> 1x1 project
 * hidden -> cout + norm [-> + x when `residual` (stride 1, cin == cout)].  The hidden tensor never reaches HBM: a workgroup
 * owns a region of output pixels and a slice of the hidden channels, expands a chunk of 32 channels on the fp32 MFMA into
 * LDS, runs the depthwise conv there and accumulates the projection in registers (csrc/invres.hip).
 *   x (n, cin, h, w), w_expand (hidden, cin), w_dw (hidden, 3, 3), w_project (cout, hidden), y (n, cout, oh, ow); a*, b*:
 *   the folded norms (`affine` = MV_AFFINE_MUL_ADD | MV_AFFINE_FMA for all three); all DEVICE pointers, 16-byte aligned.
 *   A block without expansion (the reference's expand_ratio == 1, mobilenetv2.py:37-38: hidden == cin, the depthwise conv runs
 *   on x itself) passes w_expand = a1 = b1 = NULL.
 * mv_inverted_residual_k_slices: 0 = no fused kernel for this shape (covered: square 28 / 14 / 7-pixel maps with MobileNetV2's
 * channel counts; 56-pixel maps with cin 24 and 112-pixel maps with cin 16 at stride 2 for any hidden % 8 == 0 and cout <= 32;
 * the 32 -> 32 -> cout <= 32 block without expansion on 112-pixel maps.  Else run the block as three mv_conv_norm_act_f32
 * calls); otherwise the number of slices of the projection's
 * summation order: expansion and depthwise conv are single ascending chains per output as in mv_conv_norm_act_f32; the
 * projection sums `return value` chains over *slice_len hidden channels each (ascending from +0; the last may be shorter),
 * adds them in ascending slice order, then norm, then `+ x`.  The plan depends on n (workgroup count), like
 * mv_conv3x3_k_slices.  More than one slice needs `workspace` of mv_inverted_residual_workspace_bytes() bytes (raw partial
 * sums, added by a second kernel of the same call); no atomics, deterministic.  oracle/oracle.c restates the block as
 * orc_conv2d_affine_act_f32 x 2 + orc_pointwise_sliced_affine_act_f32. */
int mv_inverted_residual_k_slices(int64_t n, int cin, int hidden, int cout, int h, int wdt, int stride, int* slice_len);
int64_t mv_inverted_residual_workspace_bytes(int64_t n, int cin, int hidden, int cout, int h, int wdt, int stride);
int mv_inverted_residual_f32(const float* x, const float* w_expand, const float* a1, const float* b1, const float* w_dw,
                             const float* a2, const float* b2, const float* w_project, const float* a3, const float* b3,
                             int residual, float* y, int64_t n, int cin, int hidden, int cout, int h, int wdt, int stride,
                             int affine, void* workspace, int64_t workspace_bytes, void* stream);
/* nn.BatchNorm2d(eval) -> (alpha, beta), HOST arrays in and out (weight / bias may be NULL = 1 / 0):
 * alpha = (1 / sqrt(var + eps)) * weight, beta = fma(-mean, alpha, bias) -- ATen batch_norm_cpu's own fp32 steps. */
void mv_fold_batchnorm(const float* weight, const float* bias, const float* mean, const float* var, double eps, int c,
                       float* alpha, float* beta);

/* ---- torchvision::deform_conv2d forward --------------------------------------------------------
 * The operator the reference registers with `TORCH_LIBRARY_FRAGMENT(torchvision, m)` (csrc/ops/deform_conv2d.cpp:164-169:
 * deform_conv2d(Tensor input, Tensor weight, Tensor offset, Tensor mask, Tensor bias, int stride_h, int stride_w, int pad_h,
 * int pad_w, int dilation_h, int dilation_w, int groups, int offset_groups, bool use_mask) -> Tensor); same arguments in
 * the same order, tensors as contiguous fp32 device pointers plus their sizes:
 *   x (n, cin, h, w), weight (cout, cin / groups, kh, kw), offset (n, 2 * offset_groups * kh * kw, oh, ow),
 *   mask (n, offset_groups * kh * kw, oh, ow) or NULL with use_mask = 0, bias (cout) or NULL, y (n, cout, oh, ow),
 *   oh = (h + 2*pad_h - (dilation_h*(kh-1) + 1)) / stride_h + 1, ow likewise.
 * One kernel (deformable gather fused into the GEMM's operand staging, no columns in memory) for every geometry whose tiles fit
 * in LDS -- kh*kw <= 40 and ordinary stride x dilation; then `workspace` may be NULL.  Otherwise `workspace` is device scratch
 * for the deformable im2col columns, at least mv_deform_conv2d_workspace_bytes(1, ...) (one image); the batch is processed in
 * passes of as many images as it holds.  mv_deform_conv2d_needs_workspace() says which: 0 = the fused kernel runs and no
 * workspace is used; 1 = the geometry needs one; 2 = optional: the launch is too small to fill the chip with the fused kernel's
 * tiles, the two-kernel form is faster if a workspace is passed (with NULL it runs fused).  Both forms compute the same chain
 * per output (bit-identical results). */
int64_t mv_deform_conv2d_workspace_bytes(int64_t images, int cin, int h, int wdt, int kh, int kw, int stride_h, int stride_w,
                                         int pad_h, int pad_w, int dilation_h, int dilation_w);
int mv_deform_conv2d_needs_workspace(int64_t images, int cin, int cout, int h, int wdt, int kh, int kw, int stride_h, int stride_w,
                                     int pad_h, int pad_w, int dilation_h, int dilation_w, int groups, int offset_groups);
int mv_deform_conv2d_f32(const float* x, const float* weight, const float* offset, const float* mask, const float* bias, float* y,
                         int64_t n, int cin, int h, int wdt, int cout, int kh, int kw, int stride_h, int stride_w, int pad_h,
                         int pad_w, int dilation_h, int dilation_w, int groups, int offset_groups, int use_mask, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* ---- any other nn.Conv2d of the small CNNs (AlexNet's 11x11 stride 4 and 5x5, models/alexnet.py:22-33) ------------
 * conv2d(zero padding, stride, dilation, groups) + bias (may be NULL) + activation (MV_ACT_*) as an IMPLICIT GEMM on the fp32
 * MFMA: the pointwise kernel gathers each K chunk's im2col columns from the input while it stages them, so the columns exist
 * in LDS only -- never in HBM -- and `workspace` is not needed (NULL / 0).  One accumulator per output in ascending
 * (channel, ky, kx) order, then `+ bias`, like every conv of this library.  mv_conv2d_needs_workspace() returns 0 for every
 * geometry the implicit kernel covers (K = cin/groups * kh * kw < 65536, oh * ow < 2^20); 1 beyond that: a pointwise GEMM then
 * reads columns written by a plain im2col pass into `workspace` (at least mv_deform_conv2d_workspace_bytes(1, ...), one image;
 * more images per pass with more bytes); 2 = optional: the launch is a handful of workgroups (batch 1) and the columns form,
 * which cuts smaller tiles, is faster when the caller brings the workspace -- bit-identical results in every case. */
int mv_conv2d_needs_workspace(int64_t n, int cin, int cout, int h, int wdt, int kh, int kw, int stride_h, int stride_w, int pad_h,
                              int pad_w, int dilation_h, int dilation_w, int groups);
int mv_conv2d_bias_act_f32(const float* x, const float* weight, const float* bias, float* y, int64_t n, int cin, int h, int wdt,
                           int cout, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h,
                           int dilation_w, int groups, int act, void* workspace, int64_t workspace_bytes, void* stream);
/* nn.MaxPool2d(kernel_size=k, stride=stride) without padding, floor mode (AlexNet's 3x3 stride 2): y is planes x
 * ((h-k)/stride+1) x ((w-k)/stride+1). */
int mv_maxpool2d_f32(const float* x, float* y, int64_t planes, int h, int wdt, int k, int stride, void* stream);
/* ---- nn.Conv2d + folded norm + residual + activation in one launch (ResNet: models/resnet.py:58-163) ----------------
 * mv_conv2d_bias_act_f32's convolution -- same geometry, groups (one launch per group), summation (one accumulator per output
 * in ascending (channel, ky, kx) order from +0), workspace rules and mv_conv2d_needs_workspace() answers -- followed by the whole
 * epilogue of mv_conv_norm_act_f32 in the same order: `+ bias` (may be NULL) -> folded norm (`affine`: MV_AFFINE_MUL_ADD rounds
 * v * alpha, then + beta; MV_AFFINE_FMA is one fmaf(v, alpha, beta); alpha / beta (cout) are required iff affine != 0) ->
 * `residual + v` (NULL, or shaped like y) -> activation (MV_ACT_*).  oracle/oracle.c::orc_conv2d_affine_act_f32 is the same
 * chain, bit for bit, in the implicit form (k_conv_igemm_full; with neither norm nor residual the instances of
 * mv_conv2d_bias_act_f32 run) and in the columns form (plain im2col into `workspace` + the pointwise GEMM) alike.
 * ResNet's 7x7 stride-2 stem, its 3x3 convs at any stride / dilation and its 1x1 stride-2 downsample run here; 1x1 convs at
 * stride 1 are mv_conv_norm_act_f32's (MV_CONV_PW1X1).  y must not overlap x, weight or residual (MV_ERR_INVALID_ARGUMENT);
 * alignment: as for mv_conv2d_bias_act_f32 -- the residual is read with 16-byte loads where y is stored so and the residual
 * pointer is 16-byte aligned, else element by element, never past h * w of a plane or the last channel; same bits.
 * Bad arguments return a negative status before any launch; n == 0 is a successful no-op. */
int mv_conv2d_affine_act_f32(const float* x, const float* weight, const float* bias, const float* alpha, const float* beta,
                             const float* residual, float* y, int64_t n, int cin, int h, int wdt, int cout, int kh, int kw,
                             int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w, int groups,
                             int affine, int act, void* workspace, int64_t workspace_bytes, void* stream);
/* nn.MaxPool2d(kernel_size=k, stride=stride, padding=pad), floor mode, dilation 1 (ResNet's stem: 3, 2, 1): y is planes x
 * ((h+2*pad-k)/stride+1) x ((w+2*pad-k)/stride+1).  Padded positions never win (the window is clipped to the image);
 * 0 <= pad <= k / 2, else MV_ERR_INVALID_ARGUMENT (torch's own rule), as is a non-positive output size.  NaN: torch's CPU kernel's
 * rule -- m = -inf, then `if (v > m || isnan(v)) m = v` over the window in row-major order. */
int mv_maxpool2d_pad_f32(const float* x, float* y, int64_t planes, int h, int wdt, int k, int stride, int pad, void* stream);
/* The same with ceil_mode=True (SSD's third VGG pool, 75 -> 38): per axis o = ceil((in + 2 pad - k) / stride) + 1, less one when
 * (o - 1) stride >= in + pad (the last window would start in the right padding); y is planes x oh x ow.  Windows are clipped to the
 * image, and none is empty.  Arguments, refusals and the NaN rule as for mv_maxpool2d_pad_f32; pad may be 0. */
int mv_maxpool2d_ceil_f32(const float* x, float* y, int64_t planes, int h, int wdt, int k, int stride, int pad, void* stream);

/* ---- the step BEFORE the path: ImageClassification's tail, transforms/_presets.py:58-60 -------
 * convert_image_dtype(float) = image.to(float32).mul_(1/255) (_misc.py:286-288), then normalize =
 * image.sub(mean).div_(std) (_misc.py:54-66).  x is (n, c, hw) planar; mean / std are HOST arrays of c floats
 * (c <= 16); NULL mean and std = conversion only. */
int mv_to_float_normalize_u8(const uint8_t* x, float* y, int64_t n, int c, int64_t hw, const float* mean, const float* stdv,
                             void* stream);
int mv_normalize_f32(const float* x, float* y, int64_t n, int c, int64_t hw, const float* mean, const float* stdv,
                     void* stream);
/* ---- the head of the same preset: F.resize(bilinear, antialias=True) + F.center_crop ---------------------------
 * (transforms/_presets.py:56-57; tensor path transforms/_functional_tensor.py:441-474 = .to(float32) ->
 * torch interpolate(bilinear, align_corners=False, antialias=True) -> torch.round + narrow for uint8;
 * transforms/functional.py:556-594 for the crop offsets and its zero padding).
 * x is (planes, h, w); the image is resized to (oh, ow) and y receives the (crop_h, crop_w) window whose top-left
 * corner is (crop_top, crop_left) in resized coordinates -- pass (0, 0, oh, ow) for a plain resize; parts of the
 * window outside the resized image are zero (center_crop's padding).  Only the rows and columns the window needs
 * are computed.  Scale factors up to 7 on both axes run as ONE kernel (width-pass rows in LDS): mv_resize_workspace_bytes(...)
 * returns 0 and `workspace` may be NULL.  Beyond, `workspace` is device scratch of at least that many bytes (fp32 width-pass
 * rows) and the call makes two launches on `stream`.  It allocates nothing; the results are the same bits either way. */
int64_t mv_resize_workspace_bytes(int64_t planes, int h, int wdt, int oh, int ow, int crop_top, int crop_left, int crop_h,
                                  int crop_w);
int mv_resize_bilinear_aa_u8(const uint8_t* x, uint8_t* y, int64_t planes, int h, int wdt, int oh, int ow, int crop_top,
                             int crop_left, int crop_h, int crop_w, void* workspace, int64_t workspace_bytes, void* stream);
int mv_resize_bilinear_aa_f32(const float* x, float* y, int64_t planes, int h, int wdt, int oh, int ow, int crop_top,
                              int crop_left, int crop_h, int crop_w, void* workspace, int64_t workspace_bytes, void* stream);
/* The whole ImageClassification.forward on a tensor image (transforms/_presets.py:56-63) in the same two launches:
 * resize -> center_crop -> convert_image_dtype(float) (v1: uint8 `.to(float32) / 255.0`,
 * _functional_tensor.py:93-99) -> normalize (`sub_(mean).div_(std)`, :928).  x is (n, c, h, w) with c <= 4,
 * y is fp32 (n, c, crop_h, crop_w); mean / std are HOST arrays of c floats. */
int mv_preset_classification_u8(const uint8_t* x, float* y, int64_t n, int c, int h, int wdt, int oh, int ow, int crop_top,
                                int crop_left, int crop_h, int crop_w, const float* mean, const float* stdv,
                                void* workspace, int64_t workspace_bytes, void* stream);
int mv_preset_classification_f32(const float* x, float* y, int64_t n, int c, int h, int wdt, int oh, int ow, int crop_top,
                                 int crop_left, int crop_h, int crop_w, const float* mean, const float* stdv,
                                 void* workspace, int64_t workspace_bytes, void* stream);
/* ---- ElasticTransform's resampling: F.elastic (transforms/v2/functional/_geometry.py elastic_image /
 * _apply_grid_transform) = grid_sample(image, identity grid + displacement, mode, padding_mode="zeros",
 * align_corners=False), then the fill blend of the resampled ones-mask (bilinear: ((v - fill) * m) + fill; nearest:
 * fill where the sample left the frame), then round half to even for uint8.  x, y are (planes, h, w); every plane is
 * resampled with the same field.  base_x / base_y are DEVICE arrays of w / h floats: the identity grid's
 * torch.linspace((1 - n) / n, (n - 1) / n, n) vectors as the caller's torch computed them (their bits are ATen's
 * vectorised arange, not a closed form).  disp is the DEVICE (1, h, w, 2) fp32 field, element (i, j, c) at
 * disp[i * disp_sh + j * disp_sw + c * disp_sc] (any strides: interleaved or the dx-plane / dy-plane permute of
 * ElasticTransform._get_params).  mode: 0 bilinear, 1 nearest.  fill: NULL (no blend) or a HOST array of `channels`
 * floats (plane p takes fill[p % channels]; at most 16); planes must be a multiple of channels.  h * w < 2^31. */
int mv_elastic_f32(const float* x, float* y, int64_t planes, int channels, int h, int wdt, const float* base_x,
                   const float* base_y, const float* disp, int64_t disp_sh, int64_t disp_sw, int64_t disp_sc, int mode,
                   const float* fill, void* stream);
int mv_elastic_u8(const uint8_t* x, uint8_t* y, int64_t planes, int channels, int h, int wdt, const float* base_x,
                  const float* base_y, const float* disp, int64_t disp_sh, int64_t disp_sw, int64_t disp_sc, int mode,
                  const float* fill, void* stream);
/* ---- F.affine / F.rotate / F.perspective (transforms/v2/functional/_geometry.py affine_image, rotate_image,
 * perspective_image / _apply_grid_transform) = grid_sample(image, grid, mode, padding_mode="zeros", align_corners=False), the
 * fill blend as mv_elastic_*, round half to even for uint8.  x is (planes, ih, iw), y is (planes, oh, ow); every plane is
 * resampled with the same grid, which is never materialised: output pixel (i, j) computes it from coeffs, a HOST array of 8
 * floats (ax, bx, cx, ay, by, cy, c6, c7) -- (a, b, c) of each axis = one column of the reference's rescaled theta:
 *   kind 0 (affine):      x = j - (ow - 1) / 2, y = i - (oh - 1) / 2, g = x * a + y * b + c              (c6, c7 unused)
 *   kind 1 (perspective): x = j + 0.5, y = i + 0.5, g = (x * a + y * b + c) / (x * c6 + y * c7 + 1) - 1
 * with the rounding of the reference's CPU bmm: order 1 = fma(y, b, x * a) + c (a blocked BLAS path that fuses), order 0 =
 * (x * a + y * b) + c (ATen's naive loop, taken when oh * ow * 3 * 2 < 400, or a blocked path that does not fuse).  mode: 0 bilinear, 1 nearest.  fill: NULL (no blend) or a HOST array
 * of `channels` floats (plane p takes fill[p % channels]; at most 16); planes must be a multiple of channels.  ih * iw and
 * oh * ow < 2^31. */
int mv_warp_f32(const float* x, float* y, int64_t planes, int channels, int ih, int iw, int oh, int ow, const float* coeffs,
                int kind, int order, int mode, const float* fill, void* stream);
int mv_warp_u8(const uint8_t* x, uint8_t* y, int64_t planes, int channels, int ih, int iw, int oh, int ow, const float* coeffs,
               int kind, int order, int mode, const float* fill, void* stream);
/* The same convolution with K SLICES ACROSS WORKGROUPS for launches too small to fill the chip with one chain per output (VGG's
 * 512 -> 512 layers at batch 1: ~50 workgroups walking 128 K chunks each).  mv_conv3x3_k_slices() states the summation order for a
 * shape -- 1: the single chain of mv_conv3x3_bias_relu_f32; otherwise that many chains over `slice_channels` input channels each
 * (the last may be shorter), every one from +0 in (channel, ky, kx) order, added in ascending slice order, then `+ bias`, then
 * ReLU: within 1e-6 relative of the single chain.  `workspace`: device scratch of mv_conv3x3_workspace_bytes() bytes (0 when the
 * shape is not sliced; then the call is mv_conv3x3_bias_relu_f32).
 * BATCH DEPENDENCE: the plan is a function of the workgroup count, hence of n -- the same image may differ in its last bits
 * between a batch-1 and a batch-8 call of the _ws entry (the same holds for mv_linear_k_slices and mv_conv1x1_k_slices).
 * mv_conv3x3_bias_relu_f32 / mv_linear_bias_relu_f32 (no workspace) keep ONE chain per output for every n: callers that need
 * batch-invariant bits use those (Python: functional.BATCH_INVARIANT_SUMMATION = True).  tests/golden/k_slice_plans.json
 * pins the plans of the VGG / AlexNet / MobileNetV2 shapes. */
int mv_conv3x3_k_slices(int64_t n, int cin, int h, int wdt, int cout, int* slice_channels);
int64_t mv_conv3x3_workspace_bytes(int64_t n, int cin, int h, int wdt, int cout);
int mv_conv3x3_bias_relu_ws_f32(const float* x, const float* w, const float* b, float* y, int64_t n, int cin, int h, int wdt, int cout,
                                int relu, void* workspace, int64_t workspace_bytes, void* stream);
/* The same conversion + normalisation fused into the first layer's load: x is the uint8 (n,3,h,w) image, the
 * fp32 normalised tensor never exists in HBM.  cout <= 64, w % 4 == 0. */
int mv_conv3x3_bias_relu_u8norm_f32(const uint8_t* x, const float* mean3, const float* std3, const float* w, const float* b,
                                    float* y, int64_t n, int h, int wdt, int cout, int relu, void* stream);

/* nn.Linear(k, m) [+ bias] [+ ReLU] (vgg.py:42-50): x (n, k), w (m, k) as nn.Linear stores it, b (m) or NULL,
 * y (n, m); all device pointers.  fp32 MFMA, one ascending-k chain per output (no split-K), bias as the last tap. */
int mv_linear_bias_relu_f32(const float* x, const float* w, const float* b, float* y, int64_t n, int k, int m, int relu,
                            void* stream);
/* The same layer for inference-size batches, where the single pass leaves most of the chip idle (25088 -> 4096 at batch 64
 * is 64 workgroups): K is cut into mv_linear_k_slices() contiguous slices of *slice_len k values (a multiple of 32); each
 * slice is an ascending-k chain from +0 whose partial sums go to workspace[slice][n][m]; a second kernel adds the partials
 * in ascending slice order, then the bias, then the ReLU.  Deterministic (no atomics); within 1e-6 relative of the single
 * chain.  mv_linear_workspace_bytes() == 0 (large batches): identical to mv_linear_bias_relu_f32, workspace may be NULL. */
int mv_linear_k_slices(int64_t n, int k, int m, int* slice_len);
int64_t mv_linear_workspace_bytes(int64_t n, int k, int m);
int mv_linear_bias_relu_ws_f32(const float* x, const float* w, const float* b, float* y, int64_t n, int k, int m, int relu,
                               void* workspace, int64_t workspace_bytes, void* stream);

/* ---- The v2 colour ops (transforms/v2/functional/_color.py adjust_brightness_image, adjust_contrast_image,
 * adjust_saturation_image, adjust_hue_image) and ColorJitter's chain of them.  x, y are (images, channels, h, w), channels
 * 1 or 3, contiguous, not aliased.  ops / factors are HOST arrays of n_ops (1-4) op codes and their factors, applied in order
 * to every pixel with the reference's rounding and its quantisation between ops (uint8: clamp, then truncation); at most one
 * MV_COLOR_CONTRAST.  Saturation and hue leave 1-channel images unchanged.  form: the rounding of the reference's
 * `add_(other, alpha=a)` -- 1 fma(other, a, self), 0 self + other * a -- for the grey value and the blends.  A chain with
 * contrast needs `workspace`, a DEVICE buffer of mv_color_workspace_bytes(images, h, w, u8) bytes (any content; the call
 * initialises what it uses): the per-image mean of the grey image of the chain so far is reduced there on the stream --
 * uint8 as an exact integer sum S, mean (float)S / (float)(h * w); float32 as double partials summed in a fixed order, the
 * mean rounded once to float32 -- so results are the same bits on every run and nothing is read back.  Without contrast,
 * workspace may be NULL. */
#define MV_COLOR_BRIGHTNESS 0
#define MV_COLOR_CONTRAST 1
#define MV_COLOR_SATURATION 2
#define MV_COLOR_HUE 3
int64_t mv_color_workspace_bytes(int64_t images, int h, int w, int u8);
int mv_color_chain_f32(const float* x, float* y, int64_t images, int channels, int h, int w, const int* ops,
                       const double* factors, int n_ops, int form, void* workspace, int64_t workspace_bytes, void* stream);
int mv_color_chain_u8(const uint8_t* x, uint8_t* y, int64_t images, int channels, int h, int w, const int* ops,
                      const double* factors, int n_ops, int form, void* workspace, int64_t workspace_bytes, void* stream);
/* rgb_to_grayscale of (images, 3, h, w) into (images, out_channels, h, w), out_channels 1 or 3: the grey value of the
 * reference's `r.mul(0.2989).add_(g, alpha=0.587).add_(b, alpha=0.114)` (form as above; uint8: truncated by .to(uint8)) in
 * every output plane. */
int mv_rgb_to_grayscale_f32(const float* x, float* y, int64_t images, int h, int w, int out_channels, int form, void* stream);
int mv_rgb_to_grayscale_u8(const uint8_t* x, uint8_t* y, int64_t images, int h, int w, int out_channels, int form,
                           void* stream);

/* ---- The automatic-augmentation colour ops (transforms/v2/functional/_color.py invert_image, posterize_image,
 * solarize_image, autocontrast_image, equalize_image): what AutoAugment / RandAugment / TrivialAugmentWide call besides the
 * geometric and F.adjust_* ops.  x, y are contiguous and not aliased.
 *
 * mv_pointwise_*: n elements of any layout, op applied to each.  MV_POINT_INVERT: float 1.0f - x, uint8 ~x (param unused).
 * MV_POINT_POSTERIZE, param = bits in [0, 8]: float floor(x * 2^bits) clamped to [0, 2^bits - 1], times 2^-bits (NaN stays
 * NaN); uint8 x & (((1 << bits) - 1) << (8 - bits)).  MV_POINT_SOLARIZE, param = threshold: (float)x >= (float)threshold ?
 * invert(x) : x -- the comparison of a uint8 image against a float threshold, which torch promotes to float32 (a host with an
 * integer threshold passes the uint8 value it wraps to).
 *
 * Alignment, for every entry point from the colour ops down to mv_mixup_labels_i64: x and y need the alignment of their
 * element type only (a contiguous view at any element offset of an allocation is fine); a workspace must be 16-byte
 * aligned, which the entry points check.  mv_pointwise_* moves 16 bytes per lane when both x and y are 16-byte aligned
 * (whatever n is: the last partial group goes element by element) and element by element otherwise -- "vec16" / "px" in
 * mv_last_kernel(); the colour and plane ops additionally need a plane length that is a multiple of 16 / elem_bytes for their
 * 16-byte path.  Nothing outside x, y and the stated workspace size is read or written. */
#define MV_POINT_INVERT 0
#define MV_POINT_POSTERIZE 1
#define MV_POINT_SOLARIZE 2
int mv_pointwise_f32(const float* x, float* y, int64_t n, int op, double param, void* stream);
int mv_pointwise_u8(const uint8_t* x, uint8_t* y, int64_t n, int op, double param, void* stream);
/* autocontrast on (planes, h, w): per plane, min and max in float32 (uint8 as its integer values), inv_scale =
 * (max - min) * (float)(1 / bound); a plane with max == min takes min = 0, inv_scale = 1; then (x - min) / inv_scale (a
 * correctly rounded division) clamped to [0, bound], uint8 truncated.  A NaN anywhere in a float32 plane makes the whole
 * plane NaN, as amin / amax propagate it.  Two launches: per-workgroup (min, max, NaN) partials in `workspace` (a DEVICE
 * buffer of mv_autocontrast_workspace_bytes bytes, any content), then the map, each workgroup reducing its plane's partials
 * in index order.  Nothing is read back. */
int64_t mv_autocontrast_workspace_bytes(int64_t planes, int h, int w, int u8);
int mv_autocontrast_f32(const float* x, float* y, int64_t planes, int h, int w, void* workspace, int64_t workspace_bytes,
                        void* stream);
int mv_autocontrast_u8(const uint8_t* x, uint8_t* y, int64_t planes, int h, int w, void* workspace, int64_t workspace_bytes,
                       void* stream);
/* equalize on (planes, h, w), h * w < 2^31: per plane the 256-bin histogram of the uint8 image (float32: of
 * (uint8)(x * 255.999f), with values outside [0, 1] and NaN saturated to bins 0 and 255), num_non_max = h * w - hist[max value],
 * step = num_non_max / 255, lut[0] = 0, lut[k] = min((cum_hist[k - 1] + step / 2) / step, 255); planes with step == 0 keep
 * their (quantised) values.  float32 output: (float)v * (float)(1 / 255.0).  The histogram is built per workgroup in LDS and
 * added with integer atomics into `workspace` (mv_equalize_workspace_bytes bytes: planes x 256 uint32, zeroed on the stream
 * by the call's first kernel); the map's workgroups each rebuild their plane's LUT from it.  Nothing is read back. */
int64_t mv_equalize_workspace_bytes(int64_t planes, int h, int w, int u8);
int mv_equalize_f32(const float* x, float* y, int64_t planes, int h, int w, void* workspace, int64_t workspace_bytes,
                    void* stream);
int mv_equalize_u8(const uint8_t* x, uint8_t* y, int64_t planes, int h, int w, void* workspace, int64_t workspace_bytes,
                   void* stream);

/* ---- RandomResizedCrop's hot path: F.resized_crop = resize_image(crop_image(x, top, left, wh, ww), (oh, ow)) without a copy of
 * the crop.  x is (planes, h, w); the source window [top, top + wh) x [left, left + ww) is in input coordinates and may reach
 * outside the image (crop_image's zero padding: such pixels read as 0); the interpolation axes are those of a (wh, ww) image.
 * flip_h / flip_v mirror the OUTPUT (the reference flips after the resize; flipping the input first runs the fma chains in the
 * other order and is not bit-identical).  Workspace: mv_resize_workspace_bytes(planes, wh, ww, oh, ow, 0, 0, oh, ow).  The
 * *_preset_* forms add the tail of mv_preset_classification_*: uint8 `/ 255` (v2_scale = 0, v1's convert_image_dtype) or
 * uint8 `* (1 / 255)` (v2_scale = 1, v2's to_dtype(scale=True)), then `(v - mean[c]) / std[c]` into fp32; float32 input is
 * not rescaled. */
int mv_resized_crop_u8(const uint8_t* x, uint8_t* y, int64_t planes, int h, int wdt, int top, int left, int wh, int ww, int oh,
                       int ow, int flip_h, int flip_v, void* workspace, int64_t workspace_bytes, void* stream);
int mv_resized_crop_f32(const float* x, float* y, int64_t planes, int h, int wdt, int top, int left, int wh, int ww, int oh,
                        int ow, int flip_h, int flip_v, void* workspace, int64_t workspace_bytes, void* stream);
int mv_resized_crop_preset_u8(const uint8_t* x, float* y, int64_t n, int c, int h, int wdt, int top, int left, int wh, int ww,
                              int oh, int ow, int flip_h, int flip_v, int v2_scale, const float* mean, const float* stdv,
                              void* workspace, int64_t workspace_bytes, void* stream);
int mv_resized_crop_preset_f32(const float* x, float* y, int64_t n, int c, int h, int wdt, int top, int left, int wh, int ww,
                               int oh, int ow, int flip_h, int flip_v, int v2_scale, const float* mean, const float* stdv,
                               void* workspace, int64_t workspace_bytes, void* stream);
/* ---- F.pad / F.crop / F.horizontal_flip / F.vertical_flip / F.erase: one gather kernel that moves elements of elem_bytes
 * (1, 2, 4 or 8) bytes, whatever their dtype.  x is (planes, ih, iw), y is (planes, oh, ow).  Output pixel (oy, ox) takes source
 * pixel (map(oy), map(ox)), per axis: p = (flip ? out - 1 - o : o) + offset with offset = `top` / `left` (negative: padding,
 * positive: cropping); 0 <= p < in is p itself, otherwise the border mode decides: MV_PAD_CONSTANT the fill, MV_PAD_EDGE
 * clamp(p), MV_PAD_REFLECT -p or 2 (in - 1) - p (each padding must be smaller than the side, as ATen requires),
 * MV_PAD_SYMMETRIC -1 - p or 2 in - 1 - p (each padding at most the side).  `fill` is NULL (zeros)
 * or a HOST array of `channels` (1..4) elements of elem_bytes each, already in the image's dtype; plane p takes
 * fill[p % channels].  One launch, no workspace. */
#define MV_PAD_CONSTANT 0
#define MV_PAD_EDGE 1
#define MV_PAD_REFLECT 2
#define MV_PAD_SYMMETRIC 3
int mv_pad_crop_flip(const void* x, void* y, int64_t planes, int channels, int elem_bytes, int ih, int iw, int oh, int ow, int top,
                     int left, int mode, int flip_h, int flip_v, const void* fill, void* stream);
/* erase: y = x with the box [i, i + eh) x [j, j + ew) (inside the image) replaced by v, a DEVICE array in the image's dtype of
 * `channels` elements (v_is_per_pixel = 0) or channels x eh x ew elements (1); plane p takes channel p % channels.  Out of
 * place it is one launch of the gather kernel and the source pixels under the box are not read; with y == x only the box is
 * written. */
int mv_erase(const void* x, void* y, int64_t planes, int channels, int elem_bytes, int h, int w, int i, int j, int eh, int ew,
             const void* v, int v_is_per_pixel, void* stream);
/* ---- MixUp / CutMix (transforms/v2/_augment.py) over a contiguous batch x of `batch` samples: sample b is paired with sample
 * (b - 1 + batch) % batch, the reference's roll(1, 0).  x and y must not alias; batch == 0 or empty samples are a no-op.
 * mixup: y[b] = fl(fl(x[b - 1] * wp) + fl(x[b] * ws)) with wp = 1 - lam and ws = lam narrowed from double to the compute type
 * (float for _f32 and _f16, double for _f64): two separately rounded products and one rounded sum, never an fma; _f16 rounds
 * each of the three results to float16.  Probability labels (batch, num_classes) go through the same entries. */
int mv_mixup_f32(const float* x, float* y, int64_t batch, int64_t sample_elems, double lam, void* stream);
int mv_mixup_f16(const void* x, void* y, int64_t batch, int64_t sample_elems, double lam, void* stream);
int mv_mixup_f64(const double* x, double* y, int64_t batch, int64_t sample_elems, double lam, void* stream);
/* cutmix: a sample is planes_per_sample planes of (h, w) elements of elem_bytes (1, 2, 4 or 8) bytes, whatever their dtype; inside
 * the box [y1, y2) x [x1, x2) (0 <= x1 <= x2 <= w, 0 <= y1 <= y2 <= h) y[b] takes x[b - 1], outside it x[b].  An empty box is a
 * copy, the whole image a roll. */
int mv_cutmix(const void* x, void* y, int64_t batch, int64_t planes_per_sample, int elem_bytes, int h, int w, int x1, int y1, int x2,
              int y2, void* stream);
/* index labels: y (batch, num_classes) float32 = the mixup of one_hot(labels, num_classes).float(), in one launch and with the
 * same three roundings (a row whose neighbour has the same label holds fl(fl(1 - lam) + fl(lam)) there, not a literal 1).  A label
 * outside [0, num_classes) is not reported (that would need a read-back): it matches no column, its row's own share is zeros and
 * nothing is written outside y.  labels needs 8-byte and y 4-byte alignment; a 16-byte aligned y is written with 16-byte stores
 * (k_mixup_labels<vec>), any other element by element (k_mixup_labels<scalar>): the same values. */
int mv_mixup_labels_i64(const int64_t* labels, float* y, int64_t batch, int num_classes, double lam, void* stream);

/* ---- torchvision.ops.nms (forward), the arithmetic of the reference's CPU kernel.  boxes (n, 4) float32 as x1, y1, x2, y2 and
 * scores (n) float32, both DEVICE arrays that need 4-byte alignment only; n <= 262144.  The boxes are taken in descending score
 * order, equal scores in index order (the stable sort of the reference; -0 == +0, a NaN score ranks first as in torch.sort), and a
 * box j is dropped when a box i kept before it has  inter / ((area_i + area_j) - inter) > iou_threshold  with
 * area = (x2 - x1) * (y2 - y1), inter = max(0, min(x2) - max(x1)) * max(0, min(y2) - max(y1)): every operation rounded once to
 * float32, the division correctly rounded, the quotient compared with the threshold as a double.  keep_out (n int64, DEVICE)
 * receives the kept indices in that order -- only its first *keep_count_out (one int64, DEVICE) elements are written.  Three
 * launches (order, 64 x 64 suppression-mask tiles on and above the diagonal, one workgroup that walks the mask rows with the
 * "removed" bitset in LDS); nothing is read back and nothing is allocated: the sorted boxes, the order and the mask words live in
 * `workspace`, a 16-byte aligned DEVICE buffer of mv_nms_workspace_bytes(n) bytes (16 n + 8 n ceil(n / 64) + 4 n, rounded up to
 * 16; 0 for n <= 0 or an unsupported n) with any content.  n == 0 is a no-op: nothing is launched and not even the count is
 * written. */
int64_t mv_nms_workspace_bytes(int64_t n);
int mv_nms_f32(const float* boxes, const float* scores, int64_t n, double iou_threshold, int64_t* keep_out, int64_t* keep_count_out,
               void* workspace, int64_t workspace_bytes, void* stream);
/* ---- torchvision.ops.roi_align (forward), the arithmetic of the reference's CPU kernel.  x (n, c, h, w) float32, rois (k, 5)
 * float32 rows [batch_idx, x1, y1, x2, y2], y (k, c, pooled_h, pooled_w) float32; h * w < 2^31.  Per roi: the corners times
 * (float)spatial_scale minus 0.5 when `aligned`; without `aligned` the roi's width and height are clamped to at least 1; bin =
 * size / pooled; grid = sampling_ratio when positive, else ceil(size / pooled) per axis.  Output (ph, pw) is the sum over the
 * grid_h x grid_w samples at  start + p * bin + (i + 0.5) * bin / grid  (ascending iy, then ix) of the bilinear value
 * ((w1 v1 + w2 v2) + w3 v3) + w4 v4, divided by max(grid_h * grid_w, 1).  A sample outside [-1, h] x [-1, w] adds zero; inside,
 * coordinates below 0 clamp to 0 and the last row / column has no upper neighbour (bilinear_interpolate of the reference).
 * Every product, sum and quotient is rounded once to float32 -- nothing is fused.  One lane per output element, one launch, no
 * workspace.  rois stay on the device and are not read back, so a batch index that does not truncate into [0, n) cannot be
 * reported: that roi's outputs are zeros and x is not read for it.  k == 0 (or an empty output) is a no-op. */
int mv_roi_align_f32(const float* x, const float* rois, float* y, int64_t n, int c, int h, int w, int64_t k, int pooled_h, int pooled_w,
                     double spatial_scale, int sampling_ratio, int aligned, void* stream);
/* ---- torchvision.ops.roi_pool, ps_roi_pool and ps_roi_align (forward), the arithmetic of the reference's CPU kernels.  x (n, c, h,
 * w) float32, rois (k, 5) float32 rows [batch_idx, x1, y1, x2, y2], h * w < 2^31, as for mv_roi_align_f32.  Each op writes two
 * outputs of one shape, y float32 and a second one of 32-bit ints (`int` is 32 bits on every supported target), which must not be
 * NULL and must not overlap y or an input.  Every float product, sum, difference and quotient is rounded once to float32 --
 * nothing is fused.  One lane per output element, one launch, no workspace.  A roi whose batch index does not truncate into
 * [0, n) (or is NaN) cannot be reported without a read-back: its elements of y are 0, those of the second output -1 (roi_pool) or
 * the input channel (the position-sensitive ops, where it does not depend on data), and x is not read for it.  k == 0, c == 0 or
 * a zero output side is a no-op.
 *
 * Rounded corners (roi_pool, ps_roi_pool): start_w = (int)roundf(x1 * (float)spatial_scale), roundf half away from zero, and
 * likewise start_h (y1), end_w (x2), end_h (y2).  The rounded float is clamped to +-2^29 and a NaN becomes 0 before the
 * conversion: inside that range this is the reference; outside it the reference's conversion is undefined.
 *
 * mv_roi_pool_f32: y and argmax are (k, c, pooled_h, pooled_w).  roi_w = max(end_w - start_w + 1, 1), roi_h likewise; bin =
 * (float)roi / (float)pooled; bin (ph, pw) covers rows [floor(ph * bin_h) + start_h, ceil((ph + 1) * bin_h) + start_h) and the
 * columns likewise, each bound clamped to [0, h] resp. [0, w].  y is the window's maximum, found with a strict `>` from -FLT_MAX in
 * row-major order (the first of equal values wins, a NaN is never taken), argmax its index hh * w + ww in the plane; an empty
 * window gives 0 and -1, a window of NaNs -FLT_MAX and -1.
 *
 * mv_ps_roi_pool_f32: c must be a multiple of pooled_h * pooled_w (MV_ERR_INVALID_ARGUMENT otherwise); y and channel_mapping are
 * (k, c / (pooled_h * pooled_w), pooled_h, pooled_w).  roi_w = max(end_w - start_w, 1) (no + 1), roi_h likewise; rows
 * [floor(ph * bin_h + (float)start_h), ceil((ph + 1) * bin_h + (float)start_h)), columns likewise, clamped as above.  Output
 * (c_out, ph, pw) reads input channel c_in = (c_out * pooled_h + ph) * pooled_w + pw: y is the sum of the window (rows ascending,
 * columns ascending, from 0) divided by its element count, 0 for an empty window; channel_mapping is c_in.
 *
 * mv_ps_roi_align_f32: shapes and channel mapping of mv_ps_roi_pool_f32.  The corners are x * (float)spatial_scale - 0.5 (the
 * half-pixel shift is always applied; there is no `aligned` flag) and the roi's size is NOT clamped to 1.  bin = size / pooled;
 * grid = sampling_ratio when positive, else (int)ceil(size / pooled) per axis.  y is the sum over the grid_h x grid_w samples at
 * (p * bin + start) + ((i + 0.5) * bin) / grid (ascending iy, then ix) of the bilinear value of mv_roi_align_f32, divided by
 * (float)(grid_h * grid_w) -- NOT by max(.., 1).  This differs from mv_roi_align_f32: a roi of zero size (and one of negative
 * size whenever ceil(size / pooled) is 0 on an axis) has an adaptive grid whose product is 0, and its outputs are 0 / 0 = NaN, as
 * the reference's loop computes; a roi with a negative grid whose product is not 0 adds no sample and gives 0 / product, a
 * signed zero.  With sampling_ratio > 0 the outputs of such rois are finite.
 *
 * Loops a roi can size: a pooling window is at most h x w elements.  The adaptive grid of ps_roi_align grows with the roi's size
 * exactly as that of mv_roi_align_f32 does and has no cap that roi_align does not have. */
int mv_roi_pool_f32(const float* x, const float* rois, float* y, int* argmax, int64_t n, int c, int h, int w, int64_t k, int pooled_h,
                    int pooled_w, double spatial_scale, void* stream);
int mv_ps_roi_pool_f32(const float* x, const float* rois, float* y, int* channel_mapping, int64_t n, int c, int h, int w, int64_t k,
                       int pooled_h, int pooled_w, double spatial_scale, void* stream);
int mv_ps_roi_align_f32(const float* x, const float* rois, float* y, int* channel_mapping, int64_t n, int c, int h, int w, int64_t k,
                        int pooled_h, int pooled_w, double spatial_scale, int sampling_ratio, void* stream);

/* ---- torchvision.ops.MultiScaleRoIAlign (ops/poolers.py, forward): mv_roi_align_f32 over up to 8 feature maps in ONE launch.
 * xs, hs, ws and scales are HOST tables of `levels` entries (as the pointer tables of the mv_*_v entry points; they are copied
 * into the kernel arguments): xs[l] a DEVICE map (n, c, hs[l], ws[l]) float32 with spatial scale (float)scales[l].  rois (k, 5)
 * float32 and roi_levels (k) int64 (8-byte aligned) are DEVICE arrays; y (k, c, pooled_h, pooled_w) float32.  Roi i is pooled from
 * the map xs[roi_levels[i]] with exactly the arithmetic of mv_roi_align_f32 (one device function serves both kernels), so the
 * result equals, bit for bit, a roi_align per level scattered into y.  A level outside [0, levels) cannot be reported without a
 * read-back: that roi's outputs are zeros and nothing is read for it, as for a batch index outside [0, n).  The checks are those
 * of mv_roi_align_f32 for every level; levels > 8 is MV_ERR_UNSUPPORTED; k == 0 (or an empty output) is a no-op that touches no
 * pointer. */
int mv_multiscale_roi_align_f32(const float* const* xs, const int* hs, const int* ws, const double* scales, int levels, const float* rois,
                                const int64_t* roi_levels, float* y, int64_t n, int c, int64_t k, int pooled_h, int pooled_w,
                                int sampling_ratio, int aligned, void* stream);

/* ---- torchvision.ops.box_iou / generalized_box_iou / distance_box_iou (ops/boxes.py, forward).  boxes1 (n, 4) and boxes2 (m, 4)
 * float32 rows x1, y1, x2, y2 that need 4-byte alignment only; out (n, m) float32 row-major.  mode 0 iou, 1 generalized, 2
 * distance; any other mode is MV_ERR_INVALID_ARGUMENT.  The values are the reference's chain of broadcast torch ops evaluated in
 * float32, every operation rounded once and nothing fused:
 *   area = (x2 - x1) * (y2 - y1);  wh = clamp(min(x2, y2 corners) - max(x1, y1 corners), min = 0);  inter = w * h;
 *   union = (area1 + area2) - inter;  iou = inter / union                     (0 / 0 = NaN, as the reference);
 *   enclosing box: whi = clamp(max(x2, y2 corners) - min(x1, y1 corners), min = 0);
 *   generalized: iou - (wi * hi - union) / (wi * hi);
 *   distance:    iou - (dx * dx + dy * dy) / ((wi * wi + hi * hi) + (float)1e-7), dx, dy the differences of the centres (a + b) / 2.
 * min, max and clamp give NaN for a NaN operand, as torch.min / torch.max / torch.clamp do.  One launch, no workspace: a wave
 * keeps 4 columns per lane in registers over a strip of rows and writes a row with one 16-byte store per lane when m % 4 == 0 and
 * out is 16-byte aligned (k_box_iou<.., vec16>), with 4-byte stores otherwise (k_box_iou<.., scalar>): the same values.  n == 0 or
 * m == 0 is a no-op that touches no pointer; a grid that n * m exceeds is MV_ERR_UNSUPPORTED. */
int mv_box_iou_f32(const float* boxes1, const float* boxes2, float* out, int64_t n, int64_t m, int mode, void* stream);

/* ---- torchvision.ops.masks_to_boxes.  masks (n, h, w) of bytes (_u8: uint8 or bool storage) or float32 (_f32); boxes (n, 4)
 * float32 = [min x, min y, max x, max y] over the elements `!= 0` of each mask (the C operator: a NaN is set, -0.0 is clear).
 * Masks are split into chunks of rows over several workgroups, which combine with integer atomicMin / atomicMax in `workspace`: a
 * 16-byte aligned DEVICE buffer of mv_masks_to_boxes_workspace_bytes(n) = 16 n bytes (0 for n <= 0) with any content; the result
 * is exact and does not depend on the order.  Rows are read with 16-byte loads between the 16-byte boundaries and element by
 * element outside them, at any w and any alignment of masks.  A mask without a set element (h * w == 0 included) cannot be
 * reported without a read-back: its box is zeros and 1 is ORed into *empty_flag (one int, DEVICE, 4-byte aligned), which the caller
 * clears beforehand and reads afterwards; the flag is not written otherwise.  n == 0 is a no-op that touches no pointer. */
int64_t mv_masks_to_boxes_workspace_bytes(int64_t n);
int mv_masks_to_boxes_u8(const unsigned char* masks, float* boxes, int* empty_flag, int64_t n, int h, int w, void* workspace,
                         int64_t workspace_bytes, void* stream);
int mv_masks_to_boxes_f32(const float* masks, float* boxes, int* empty_flag, int64_t n, int h, int w, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* ---- RegionProposalNetwork inference (models/detection/rpn.py filter_proposals up to the nms, anchor_utils.py, _utils.py
 * BoxCoder.decode_single): select first, on the head's own NCHW maps, then decode only what was selected.
 *
 * The level tables (logits, deltas, hs, ws, as, the strides) are HOST arrays of 1 <= levels <= 8 entries, copied into the kernel
 * arguments as those of mv_multiscale_roi_align_f32; logits[l] is a DEVICE map (n, as[l], hs[l], ws[l]) float32 and deltas[l] one of
 * (n, 4 as[l], hs[l], ws[l]), image i of a map starting img_strides[l] * i ELEMENTS after image 0 (>= the map's own size: a channel
 * slice of a wider tensor can be passed).  Anchor (y, x, a) of level l has the flat index  start_l + (y ws[l] + x) as[l] + a,
 * start_l the anchors of the levels before it -- the reference's permute(0, 3, 4, 1, 2) and concatenation; its logit is channel
 * a and its delta q channel 4 a + q.  The anchors of all levels number less than 2^31 (MV_ERR_UNSUPPORTED otherwise).
 *
 * mv_rpn_topk_f32: idx (n, K) int32, K = sum_l min(k, as[l] hs[l] ws[l]), receives for every image, level after level, the flat
 * indices of the level's min(k, n_l) greatest logits in STABLE DESCENDING order: greater logit first, equal logits by ascending flat
 * index, -0 equal to +0, every NaN the one greatest value (the keys of mv_nms_f32; the first k of torch.sort(stable=True,
 * descending=True) and one of torch.topk's valid answers).  One workgroup per (level, image): a four-pass radix select of the k-th
 * key with the histograms in LDS, a compaction that takes the ties in ascending flat index, a pairwise rank of the <= k candidates.
 * k <= 4096 (MV_ERR_UNSUPPORTED above), n <= 65535.  The candidates pass through `workspace`: a 16-byte aligned DEVICE buffer of
 * mv_rpn_topk_workspace_bytes(n, hs, ws, as, levels, k) = 8 n K bytes rounded up to 16 (0 for arguments the entry refuses), any
 * content.  Nothing is allocated or read back.
 *
 * mv_rpn_decode_f32: one lane per candidate idx[i, j] (idx (n, k) int32; k is any count per image, for the pair of calls the K
 * above).  The lane finds the level from the index, reads the logit and the four deltas, builds the anchor
 *   (x sw + b[a][0], y sh + b[a][1], x sw + b[a][2], y sh + b[a][3]),  sh = strides_h[l], sw = strides_w[l],
 * from base_anchors (a DEVICE (sum_l as[l], 4) float32 array, level after level: AnchorGenerator.cell_anchors concatenated),
 * applies decode_single (below) with the weights and clip given, clamps x to [0, width] and y to [0, height] of its image
 * (image_sizes: DEVICE (n, 2) float32 rows (height, width); a NaN stays) and writes
 *   boxes (n, k, 4) float32;  scores (n, k) = 1 / (1 + E(-logit));  levels (n, k) int64 (8-byte aligned);
 *   valid (n, k) uint8 = (x2 - x1 >= (float)min_size) & (y2 - y1 >= (float)min_size) & (score >= (float)score_thresh).
 * An index outside [0, anchors) cannot be reported without a read-back: zeros, level -1, valid 0, and nothing is read for it.
 *
 * mv_box_decode_f32 (BoxCoder.decode): boxes (m, 4), rel_codes (m, 4 classes) -> out (m, 4 classes), decode_single per (box, class).
 *
 * decode_single, every operation rounded once to float32, nothing fused, the divisions correctly rounded:
 *   w = x2 - x1; h = y2 - y1; cx = x1 + 0.5 w; cy = y1 + 0.5 h;  dx = c0 / wx; dy = c1 / wy; dw = min(c2 / ww, clip); dh likewise
 *   (a NaN stays); pcx = dx w + cx; pcy = dy h + cy; pw = E(dw) w; ph = E(dh) h;  box = (pcx - 0.5 pw, pcy - 0.5 ph, pcx + 0.5 pw,
 *   pcy + 0.5 ph); the weights and clip are taken as (float).
 * E is the CORRECTLY ROUNDED float32 exponential, (float)exp((double)v) -- not torch's CPU exp, a 1-ulp vector routine that
 * differs from it in about 1 % of arguments and that no other implementation reproduces bit for bit.
 *
 * Refused before any launch (MV_ERR_INVALID_ARGUMENT unless said): a null pointer or table, levels outside 1 .. 8 (above 8:
 * MV_ERR_UNSUPPORTED), a non-positive h, w or a, k < 1 (topk), an image stride below the map's size, a negative stride_h / stride_w,
 * an output that overlaps an input or another output, a workspace that is missing, too small or misaligned.  n == 0 (k == 0 for
 * decode, m == 0 for box_decode) is a no-op. */
int64_t mv_rpn_topk_workspace_bytes(int64_t n, const int* hs, const int* ws, const int* as, int levels, int k);
int mv_rpn_topk_f32(const float* const* logits, const int* hs, const int* ws, const int* as, const int64_t* img_strides, int levels,
                    int64_t n, int k, int* idx, void* workspace, int64_t workspace_bytes, void* stream);
int mv_rpn_decode_f32(const float* const* logits, const float* const* deltas, const int* hs, const int* ws, const int* as,
                      const int64_t* logit_strides, const int64_t* delta_strides, const int* strides_h, const int* strides_w, int levels,
                      const float* base_anchors, const float* image_sizes, const int* idx, int64_t n, int64_t k, double wx, double wy,
                      double ww, double wh, double clip, double min_size, double score_thresh, float* boxes, float* scores,
                      int64_t* levels_out, unsigned char* valid, void* stream);
int mv_box_decode_f32(const float* boxes, const float* rel_codes, float* out, int64_t m, int classes, double wx, double wy, double ww,
                      double wh, double clip, void* stream);

/* ---- RoIHeads.postprocess_detections up to the per-image filters (models/detection/roi_heads.py): softmax over the classes,
 * BoxCoder.decode of every class, clip_boxes_to_image, the background column dropped, the score and small-box tests -- ONE launch,
 * one wave64 per roi, lanes striding over the classes.
 *
 * All tensors are DEVICE float32.  class_logits (r, classes) and box_regression (r, 4 classes): row i starts logits_stride /
 * regression_stride ELEMENTS after row 0 (>= the row's width: a column slice of a wider tensor can be passed, as img_strides in
 * mv_rpn_topk_f32).  rois (r, 5) rows (image index, x1, y1, x2, y2), the layout of mv_roi_align_f32; image_sizes (n, 2) rows
 * (height, width) as in mv_rpn_decode_f32.  2 <= classes <= 2048 (MV_ERR_UNSUPPORTED above); r * classes < 2^31
 * (MV_ERR_UNSUPPORTED otherwise).  The outputs are dense, the background class 0 dropped; cell (i, j - 1) belongs to class j >= 1:
 *   boxes (r, classes - 1, 4) float32;  scores (r, classes - 1) float32;  labels (r, classes - 1) int64 = j (8-byte aligned);
 *   valid (r, classes - 1) uint8 = (score > (float)score_thresh) & (x2 - x1 >= (float)min_size) & (y2 - y1 >= (float)min_size)
 * -- the score test is STRICT, as torch.where(scores > score_thresh) of the reference (mv_rpn_decode_f32's is not).
 *
 * Numerics: every operation rounded once to float32, nothing fused, the divisions correctly rounded.
 *   softmax of row i:  m = max_j x_j (a NaN wins);  e_j = E(x_j - m), E the correctly rounded float32 exponential of
 *     mv_rpn_decode_f32;  s = ((e_0 + e_1) + e_2) + ... , ONE float32 chain in ascending class order, the background included;
 *     score_j = e_j / s.  NaN and +-inf behave as these formulas say: a row of all -inf, or a row that contains +inf or a NaN, gives
 *     NaN scores (and valid 0).  torch's CPU softmax uses a 1-ulp vector exp and a summation order that depends on the vector width,
 *     which no kernel reproduces bit for bit; this is the library's statement of the value.
 *   box (i, j):  decode_single (above) of rois[i, 1:5] with the codes box_regression[i, 4 j .. 4 j + 3], weights and clip as (float);
 *     then x clamped to [0, width] and y to [0, height] of image (int)rois[i, 0] (a NaN stays).
 * An image index outside [0, n) cannot be reported without a read-back: the row's boxes, scores and labels are zeros, valid 0, and
 * nothing is read through the index.
 *
 * Refused before any launch (MV_ERR_INVALID_ARGUMENT unless said): a null pointer, classes < 2, a row stride below the row's width,
 * n < 1 with r > 0, a negative r or n, an output that overlaps an input or another output (byte ranges), a misaligned labels.
 * r == 0 is a no-op that touches no pointer.  Nothing is allocated or read back. */
int mv_roi_detections_f32(const float* class_logits, int64_t logits_stride, const float* box_regression, int64_t regression_stride,
                          const float* rois, const float* image_sizes, int64_t r, int classes, int64_t n, double wx, double wy, double ww,
                          double wh, double clip, double score_thresh, double min_size, float* boxes, float* scores, int64_t* labels,
                          unsigned char* valid, void* stream);

/* ---- RetinaNet inference (models/detection/retinanet.py postprocess_detections up to the nms): sigmoid, `> score_thresh`, the top k
 * per (image, level) over every (anchor, class) pair, then the decoding of what was selected -- on the head's own NCHW maps.
 *
 * The level tables are those of mv_rpn_topk_f32 (HOST arrays, 1 <= levels <= 8) with `classes` = K >= 1 more: logits[l] is a DEVICE
 * map (n, as[l] K, hs[l], ws[l]) float32, deltas[l] one of (n, 4 as[l], hs[l], ws[l]), the image strides in ELEMENTS (64-bit, >= the
 * map's size).  The logit of anchor (y, x, a) and class c is channel a K + c; the candidate's flat index is
 *   f = (start_l + (y ws[l] + x) as[l] + a) K + c,   start_l the anchors of the levels before it
 * -- the reference's view(N, -1, K, H, W).permute(0, 3, 4, 1, 2).reshape(N, -1, K) and the concatenation over levels.  The anchors of
 * all levels times K number less than 2^31 (MV_ERR_UNSUPPORTED otherwise).
 *
 * The score of both entries is  s = 1 / (1 + E(-x)),  E the correctly rounded float32 exponential of mv_rpn_decode_f32, every
 * operation rounded once to float32, the division correctly rounded.
 *
 * mv_retinanet_topk_f32: idx (n, Ktot) int32, Ktot = sum_l min(k, as[l] hs[l] ws[l] K).  For every (image, level) the candidates with
 * s > (float)score_thresh pass (strict, in float32; a NaN score does not pass); the level's segment of idx receives the flat indices
 * of its min(k, passing) greatest scores in STABLE DESCENDING order -- greater score first, equal SCORES (not logits: every logit
 * above about 17 has the score 1) by ascending flat index -- and -1 in the rest of the segment.  This is the first k of
 * torch.sort(stable=True, descending=True) of the passing scores and one of torch.topk's valid answers.  k <= 4096
 * (MV_ERR_UNSUPPORTED above), n <= 65535.
 *   Stage 1: one workgroup per chunk of mv_retinanet_topk_chunk() consecutive elements of an (image, level) map, read once and in
 *   memory order; the chunk's own min(k, passing) greatest (score, index) keys go to the level's pool in `workspace`.  Stage 2: one
 *   workgroup per (image, level) selects the k greatest keys of the pool and ranks them.  The keys of distinct candidates differ, so
 *   the result is exact and the same on every run for every input; a pool holds min(k, chunk) keys per chunk, so nothing is dropped.
 * `workspace`: a 16-byte aligned DEVICE buffer of mv_retinanet_topk_workspace_bytes(n, hs, ws, as, levels, classes, k) bytes (0 for
 * arguments the entry refuses), any content.  Nothing is allocated or read back.
 *
 * mv_retinanet_decode_f32: one lane per idx[i, j] (idx (n, k) int32, k any count per image).  An index outside [0, anchors K) -- the
 * -1 padding -- gives a zero box, score 0, label 0 and valid 0, and nothing is read through it.  Otherwise anchor f / K, label f % K,
 * the anchor built as in mv_rpn_decode_f32 from base_anchors and the strides, decode_single with the weights and clip given
 * (RetinaNet: 1, 1, 1, 1 and log(1000 / 16)) on the deltas of channels 4 a + q, x clamped to [0, width] and y to [0, height] of the
 * image (a NaN stays), the score recomputed from the logit:
 *   boxes (n, k, 4) float32;  scores (n, k) float32;  labels (n, k) int64 (8-byte aligned);  valid (n, k) uint8 = 1.
 * There is no small-box test: the reference's RetinaNet has none.
 *
 * Refused before any launch (MV_ERR_INVALID_ARGUMENT unless said): a null pointer or table, levels outside 1 .. 8 (above 8:
 * MV_ERR_UNSUPPORTED), a non-positive h, w, a or classes, k < 1 (topk), an image stride below the map's size, a negative stride_h /
 * stride_w, an output that overlaps an input or another output, a workspace that is missing, too small or misaligned, a misaligned
 * labels.  n == 0 (k == 0 for decode) is a no-op that touches no pointer. */
int mv_retinanet_topk_chunk(void);
int64_t mv_retinanet_topk_workspace_bytes(int64_t n, const int* hs, const int* ws, const int* as, int levels, int classes, int k);
int mv_retinanet_topk_f32(const float* const* logits, const int* hs, const int* ws, const int* as, const int64_t* img_strides, int levels,
                          int classes, int64_t n, int k, double score_thresh, int* idx, void* workspace, int64_t workspace_bytes,
                          void* stream);
int mv_retinanet_decode_f32(const float* const* logits, const float* const* deltas, const int* hs, const int* ws, const int* as,
                            const int64_t* logit_strides, const int64_t* delta_strides, const int* strides_h, const int* strides_w,
                            int levels, int classes, const float* base_anchors, const float* image_sizes, const int* idx, int64_t n,
                            int64_t k, double wx, double wy, double ww, double wh, double clip, float* boxes, float* scores,
                            int64_t* labels, unsigned char* valid, void* stream);

/* ---- FCOS inference (models/detection/fcos.py postprocess_detections up to the nms) on the head's own NCHW maps: RetinaNet's two
 * entries above with another score and another box coder.  FCOS has ONE anchor per location: every as[l] is 1 (refused otherwise),
 * logits[l] is (n, K, hs[l], ws[l]), ctrness[l] (n, 1, hs[l], ws[l]), deltas[l] (n, 4, hs[l], ws[l]), each with its image stride in
 * elements; the flat index of position pos = y ws[l] + x and class c is f = (start_l + pos) K + c.
 *
 * The score of both entries is  s = sqrt(fl(sig(cls) * sig(ctr))),  sig the sigmoid of mv_retinanet_topk_f32, ctr the centerness at the
 * candidate's position, the product and the correctly rounded square root each rounded once to float32.
 *
 * mv_fcos_topk_f32: mv_retinanet_topk_f32 with that score -- s > (float)score_thresh passes (a NaN in either map does not), stable
 * descending order, -1 in the rest of a segment, the same two stages, exact and the same on every run.  `workspace`:
 * mv_retinanet_topk_workspace_bytes(n, hs, ws, as, levels, classes, k) bytes; the stage-1 chunk is mv_retinanet_topk_chunk().
 *
 * mv_fcos_decode_f32: one lane per idx[i, j]; outside the pyramid: zeros and valid 0, as above.  Otherwise the anchor (x1, y1, x2, y2)
 * of position f / K built as in mv_rpn_decode_f32, label f % K, r_q = max(deltas channel q, 0) (the head's ReLU; a NaN stays) and
 * BoxLinearCoder(normalize_by_size=True).decode, every operation rounded once to float32:
 *   cx = 0.5 (x1 + x2), cy = 0.5 (y1 + y2), w = x2 - x1, h = y2 - y1
 *   box = (cx - r0 w, cy - r1 h, cx + r2 w, cy + r3 h)
 * clamped to the image as in mv_retinanet_decode_f32, the score recomputed.  The outputs and the refusals are RetinaNet's, the
 * centerness maps checked like the logits. */
int mv_fcos_topk_f32(const float* const* logits, const float* const* ctrness, const int* hs, const int* ws, const int* as,
                     const int64_t* img_strides, const int64_t* ctr_strides, int levels, int classes, int64_t n, int k, double score_thresh,
                     int* idx, void* workspace, int64_t workspace_bytes, void* stream);
int mv_fcos_decode_f32(const float* const* logits, const float* const* ctrness, const float* const* deltas, const int* hs, const int* ws,
                       const int* as, const int64_t* logit_strides, const int64_t* ctr_strides, const int64_t* delta_strides,
                       const int* strides_h, const int* strides_w, int levels, int classes, const float* base_anchors,
                       const float* image_sizes, const int* idx, int64_t n, int64_t k, float* boxes, float* scores, int64_t* labels,
                       unsigned char* valid, void* stream);

/* ---- SSD.postprocess_detections (models/detection/ssd.py) up to the nms, on the head's own NCHW maps.  The level tables are HOST arrays
 * of `levels` <= 8 entries as for mv_rpn_topk_f32: map l holds as[l] anchors per location on an hs[l] x ws[l] grid, anchor
 * v = start_l + (y ws[l] + x) as[l] + a (start_l: the anchors of the levels before, V their total), class c of anchor a in logit
 * channel a classes + c, delta channels 4 a .. 4 a + 3; image i of map l at pointer[l] + i stride[l] (elements).
 *
 * mv_ssd_scores_f32: scores (n, classes, V), CLASS-MAJOR and dense: scores[i][c][v] = softmax over the classes of anchor v, in
 *   m = the maximum of the classes' logits (any NaN makes it NaN);  e_j = E(fl(x_j - m)) in float32, E the correctly rounded float32
 *   exp;  S = ((0 + e_0) + e_1) + e_2 + ..., one chain in ascending class order in FLOAT64 (a float32 chain over 91 classes is less
 *   accurate than torch's softmax);  p_c = (float)((double)e_c / S), the IEEE float64 division rounded to float32.  A row with a NaN
 *   or with +inf is NaN throughout, as torch's.  ONE launch for all levels and images.
 * mv_ssd_topk_f32: scores (n, classes, v) as above -> idx (n, (classes - 1) k) int32.  For image i and class c >= 1 (the background is
 *   skipped) the candidates are the anchors with scores[i][c][v] > (float)score_thresh (a NaN fails); the min(k, candidates) greatest
 *   by the key (score bits << 32 | ~v) -- the greater score first, the smaller v first among equal scores; scores are >= +0 -- are
 *   written in descending key order to idx[i][(c - 1) k ...] as f = v classes + c, the rest of the segment is -1.  Exact and
 *   deterministic for any input; nothing is read back.  k <= 4096.
 * mv_ssd_decode_f32: one candidate per idx[i][j] (n rows of k): anchor f / classes, label f % classes.  Its default box, with (w, h)
 *   = wh_pairs[pair_l + a] (a DEVICE (sum of as, 2) table, level after level, already clamped to [0, 1] where the generator clips),
 *   x_f[l], y_f[l] the level's grid divisors (HOST floats) and batch_w, batch_h the sides of the batch tensor:
 *     cx = fl(fl(x + 0.5) / x_f[l]),  x1 = fl(fl(cx - fl(0.5 w)) batch_w),  x2 = fl(fl(cx + fl(0.5 w)) batch_w),  y likewise;
 *   then BoxCoder.decode_single with the weights and `clip` as for mv_rpn_decode_f32, the clamp to image_sizes[i] = (h, w) (DEVICE,
 *   n rows), scores_out = scores[i][label][anchor], labels int64, valid 1.  f < 0 or an anchor outside the pyramid: zeros,
 *   valid 0, and nothing is read through it.
 * Refused before any launch (MV_ERR_INVALID_ARGUMENT unless said): a negative n, v or k (mv_ssd_topk_f32: k < 1), bad level tables,
 * classes < 2, an image stride below the map, a null or misaligned pointer, an output overlapping an input or another output,
 * non-positive grid divisors or batch sides; more than 8 levels, anchors x classes beyond 2^31 - 1, k > 4096, n beyond the launch
 * grid (MV_ERR_UNSUPPORTED).  n == 0 (and k == 0 for the decode) is a no-op that touches no pointer. */
int mv_ssd_scores_f32(const float* const* logits, const int* hs, const int* ws, const int* as, const int64_t* img_strides, int levels,
                      int classes, int64_t n, float* scores, void* stream);
int mv_ssd_topk_f32(const float* scores, int64_t n, int classes, int64_t v, int k, double score_thresh, int* idx, void* stream);
int mv_ssd_decode_f32(const float* scores, const float* const* deltas, const int* hs, const int* ws, const int* as,
                      const int64_t* delta_strides, int levels, int classes, const float* wh_pairs, const float* x_f, const float* y_f,
                      int batch_h, int batch_w, const float* image_sizes, const int* idx, int64_t n, int64_t k, double wx, double wy,
                      double ww, double wh, double clip, float* boxes, float* scores_out, int64_t* labels, unsigned char* valid,
                      void* stream);

/* ---- torch.nn.GroupNorm (+ ReLU) on float32 NCHW: x (n, c, h, w) -> y of the same shape, image i at x + i x_stride / y + i y_stride
 * (elements, >= c h w: a channel slice of a wider tensor is passed as it is), each image dense.  The slab of (image, group g) is the
 * contiguous span of m = (c / groups) h w elements at channel g c / groups.  Two launches, nothing read back:
 *
 *   statistics  per chunk of mv_group_norm_chunk() = 4096 consecutive elements of a slab (the last one shorter), in float64:
 *               thread t of 256 adds its 16 elements  e = 1024 u + 4 t + q  (u = 0 .. 3 outer, q = 0 .. 3 inner; an element past the
 *               slab's end counts as +0), one after the other, to (s, s2) = (0, 0): s += x, s2 += x x (exact in float64);  the 64
 *               threads 64 v .. 64 v + 63 are folded by halves, a[l] += a[l ^ 32], then ^ 16, 8, 4, 2, 1;  the four folds are
 *               added in ascending v.
 *   apply       S, S2 = the chunks' sums added in ascending chunk order to 0;  in float64  mean = S / m,
 *               var = max(S2 / m - mean mean, 0) (a NaN stays),  rstd = 1 / sqrt(var + (double)(float)eps);  mean32, rstd32 their
 *               roundings to float32;  y = fl(fl(fl(fl(x - mean32) rstd32) weight[ch]) + bias[ch])  -- the multiplication is left
 *               out when weight is null, the addition when bias is null, never an fma -- and then, when relu != 0,
 *               y < 0 ? 0 : y (a NaN stays).
 * The result of a slab is a function of the slab's values, m, weight, bias, eps and relu alone: not of n, of the slab's place or
 * alignment, or of the launch.  A NaN or an infinity in a slab makes the whole slab NaN and touches no other slab.
 * Domain: the sums carry 53 bits for 24-bit data, so S2 / m - mean^2 keeps about 29 - 2 log2(|mean| / std) bits; the statistics
 * are good to float32 for |mean| / std up to about 2^12 (tests/_fcos_ref.py measures against torch's float64 GroupNorm).
 *
 * `workspace`: a 16-byte aligned DEVICE buffer of mv_group_norm_workspace_bytes(n, c, h, w, groups) bytes (16 per chunk of every slab;
 * 0 for arguments the entry refuses or for empty work), any content.  y may be x itself with the same stride (in place).
 * Refused before any launch (MV_ERR_INVALID_ARGUMENT unless said): a negative size, groups < 1, c not divisible by groups, eps that is
 * not positive and finite as a float32, an image stride below c h w, a null or misaligned x / y, y overlapping x other than exactly, a
 * workspace that is missing, too small, misaligned or overlaps a tensor; a slab or a grid beyond 2^31 - 1 (MV_ERR_UNSUPPORTED).
 * n c h w == 0 is a no-op that touches no pointer. */
int mv_group_norm_chunk(void);
int64_t mv_group_norm_workspace_bytes(int64_t n, int c, int h, int w, int groups);
int mv_group_norm_act_f32(const float* x, float* y, const float* weight, const float* bias, int64_t n, int c, int h, int w, int groups,
                          int64_t x_stride, int64_t y_stride, double eps, int relu, void* workspace, int64_t workspace_bytes,
                          void* stream);

/* ---- weight.view(1, -1, 1, 1) * torch.nn.functional.normalize(x) (p = 2, dim = 1) on float32 NCHW: SSD's rescaling of conv4_3
 * (models/detection/ssd.py).  x (n, c, h, w) -> y of the same shape, image i at x + i x_stride / y + i y_stride (elements, >= c h w:
 * a channel slice of a wider tensor is passed as it is), each image dense; weight: c device floats.  ONE launch, nothing read back.
 * Per pixel, with x_c its value in channel c:
 *
 *   sum    for g = 0 .. 15:  S_g = the sum of (double)x_c (double)x_c (exact) over c = g, g + 16, g + 32, ... < c, added one
 *          after the other in ascending c to 0 in float64 (a group without a channel is 0);
 *          S = S_0 + S_1 + ... + S_15 added in ascending g to 0 in float64;
 *   apply  nrm = (float)sqrt(S) (the float64 square root rounded to float32);  d = nrm < eps32 ? eps32 : nrm  with
 *          eps32 = (float)eps -- clamp_min, a NaN nrm stays;  y_c = fl(weight[c] fl(x_c / d)): an IEEE division and an IEEE
 *          multiplication, never an fma, never a reciprocal.
 * The result of a pixel is a function of its c values, weight and eps alone: not of n, h, w, of the pixel's place or alignment, or
 * of the launch.  An all-zero pixel gives weight[c] 0; a NaN or an infinity makes its own pixel NaN (x / inf = 0 for a finite x) and
 * touches no other.  x is read twice, the second time out of L2.
 *
 * y may be x itself with the same stride (in place).  Refused before any launch (MV_ERR_INVALID_ARGUMENT unless said): a negative
 * size, eps that is not positive and finite as a float32, an image stride below c h w, a null or misaligned x / y / weight, y
 * overlapping x other than exactly or overlapping weight; an image or a grid beyond 2^31 - 1 (MV_ERR_UNSUPPORTED).
 * n c h w == 0 is a no-op that touches no pointer. */
int mv_l2_normalize_scale_f32(const float* x, float* y, const float* weight, int64_t n, int c, int h, int w, int64_t x_stride,
                              int64_t y_stride, double eps, void* stream);

/* ---- torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=False) and the front end of a detection model
 * (models/detection/transform.py: normalize -> resize -> batch_images) on planar float32.
 *
 * mv_interpolate_bilinear_f32: x (planes, h, w) -> y (planes, oh, ow).  Per axis, with `in` and `out` its two sizes:
 *   s   = float32(in) / float32(out)
 *   src = max(fma(s, d + 0.5f, -0.5f), 0)                     for output index d
 *   i0  = min((int)floor(src), in - 1),  i1 = min(i0 + 1, in - 1)
 *   lam = clamp(src - (float)i0, 0, 1),  w0 = 1 - lam,  w1 = lam
 * and with a, b the taps (y0, x0), (y0, x1) of the top row and c, d those of the bottom row
 *   t = fma(wx0, a, wx1 * b),  u = fma(wx0, c, wx1 * d),  out = fma(wy0, t, wy1 * u)
 * every product and every fma rounded once to float32.  NaN and +-inf follow from the formula (a zero weight times inf is NaN); with
 * out == in, src == d exactly and the result is a + 0 * b per row, the input itself for finite values.
 * This is bit for bit what torch 2.10's CPU kernel computes where it takes its vectorised channels-first loop (outputs of more than
 * 3 264 elements, and not the channels-last kernel it picks for 3 channels on one thread); its other loops differ from it by a few
 * 2^-24 max|x|.  The statement above is the library's own.
 *
 * mv_detection_batch_f32: ONE pass from n separately allocated images to the padded batch y (n, c, hp, wp).  xs is a HOST table of n
 * DEVICE pointers, image i is (c, hs[i], ws[i]) and is resized to (ohs[i], ows[i]) <= (hp, wp) (hs, ws, ohs, ows HOST tables); mean and
 * stdv are HOST arrays of c <= 16 floats (MV_ERR_UNSUPPORTED above).  Every element of y is written: inside (ohs[i], ows[i]) of image i
 * the formula above on the NORMALISED taps, each (x - mean[ch]) / stdv[ch] with the subtraction rounded and the division correctly
 * rounded (mv_normalize_f32's arithmetic); outside it +0.0.  The result has the bits of mv_normalize_f32 -> mv_interpolate_bilinear_f32
 * -> new_full(0) + copy_.  ohs[i] == hs[i] and ows[i] == ws[i] (no resize) is normalise + pad.  The tables travel in the kernel
 * arguments, 64 images per launch (longer lists take several launches); nothing is allocated or read back.
 *
 * y is stored 16 bytes at a time when its row pitch (ow, wp) is a multiple of 4 and y is 16-byte aligned, else element by element;
 * x may start at any 4-byte address.  Element offsets are 64-bit.
 * Refused before any launch (MV_ERR_INVALID_ARGUMENT unless said): a null pointer or table, a non-positive size or channel count, a
 * negative plane / image count, a resized size that exceeds the batch, a zero stdv, an output that overlaps an input, more workgroups
 * than one launch grid holds (MV_ERR_UNSUPPORTED).  planes == 0 / n == 0 is a no-op that touches no pointer. */
int mv_interpolate_bilinear_f32(const float* x, float* y, int64_t planes, int h, int w, int oh, int ow, void* stream);
int mv_detection_batch_f32(const float* const* xs, const int* hs, const int* ws, const int* ohs, const int* ows, int64_t n, int c,
                           const float* mean, const float* stdv, float* y, int hp, int wp, void* stream);

/* ---- The labels of a segmentation model (models/segmentation/_utils.py: the head's logits resized to the input with
 * F.interpolate(mode="bilinear", align_corners=False), then the argmax over the classes that users take of it) as ONE pass.
 *
 * mv_interpolate_argmax_f32: x (n, c, h, w) DEVICE float32 -> y (n, oh, ow) DEVICE labels of out_bytes 1 (uint8) or 8 (int64):
 *   y[b, Y, X] = argmax over k of v_k,   v_k = element (Y, X) of mv_interpolate_bilinear_f32's (h, w) -> (oh, ow) resize of plane (b, k)
 * The v_k are exactly that entry's float32 values (its per-axis taps and its three-step blend, every product and fma rounded once);
 * the upsampled planes never reach memory.  The taps and weights of a pixel are computed once for its c planes.  The order is
 * torch.argmax's: the lowest index among equal maxima (-0.0 == +0.0 is a tie); a NaN is greater than every number and the first NaN
 * wins.  A NaN or an infinity in a source pixel therefore reaches exactly the output pixels whose taps read it, zero-weight taps
 * included (0 * inf is NaN).  c == 1 gives all zeros.
 *
 * y is stored as one dword (uint8) or two 16-byte stores (int64) per four labels when ow is a multiple of 4 and y is 4-byte resp.
 * 16-byte aligned, else element by element (mv_last_kernel says which: k_interp_argmax<u8|i64,vec|scalar>); x may start at any 4-byte
 * address.  Element and byte offsets are 64-bit (n oh ow 8 may pass 2^32).
 * Refused before any launch (MV_ERR_INVALID_ARGUMENT unless said), writing nothing: n < 0, c < 1, a size below 1, out_bytes other
 * than 1 or 8, c > 256 with out_bytes 1, a null pointer, int64 labels that are not 8-byte aligned, an output that overlaps the input,
 * sizes that exceed the address space; a source plane of 2^30 elements or more, or more workgroups than one launch grid holds
 * (MV_ERR_UNSUPPORTED).  n == 0 is a no-op that touches no pointer. */
int mv_interpolate_argmax_f32(const float* x, void* y, int64_t n, int c, int h, int w, int oh, int ow, int out_bytes, void* stream);

/* ---- The mask branch of Mask R-CNN (models/detection/roi_heads.py maskrcnn_inference, paste_masks_in_image; mask_rcnn.py's
 * ConvTranspose2d(kernel 2, stride 2)).  All tensors DEVICE float32 unless said.
 *
 * mv_paste_masks_f32: masks (r, m, m), boxes (r, 4) rows (x1, y1, x2, y2) -> y (r, h, w), ONE launch that writes every element of y
 * once.  Everything is float32 and every operation is rounded once.  Per roi (expand_boxes, in registers):
 *   wh = (x2 - x1) * 0.5f,  hh = (y2 - y1) * 0.5f,  xc = (x2 + x1) * 0.5f,  yc = (y2 + y1) * 0.5f
 *   wh = wh * scale,  hh = hh * scale,   scale = float32((double)(m + 2 padding) / m)      (m = 28, padding = 1: 1.0714285373687744)
 *   (bx0, by0, bx1, by1) = trunc(xc - wh), trunc(yc - hh), trunc(xc + wh), trunc(yc + hh)   (toward zero, the reference's .to(int64))
 *   bw = max(bx1 - bx0 + 1, 1),  bh = max(by1 - by0 + 1, 1)
 * and y[r, Y, X] is element (Y - by0, X - bx0) of the bilinear resize of the zero-padded mask (m + 2 padding)^2 -> (bh, bw) when
 * max(bx0, 0) <= X < min(bx1 + 1, w) and max(by0, 0) <= Y < min(by1 + 1, h), and +0.0 everywhere else.  The resize is exactly the
 * formula of mv_interpolate_bilinear_f32 with s = float32(m + 2 padding) / float32(bw) (and bh), a correctly rounded division on the
 * device.  The padded mask is never materialised: a tap in the padding ring reads as +0.0.  The boxes are read on the device; nothing
 * is allocated, read back or synchronised, and r is only a grid extent.
 *   Domain.  A roi with an expanded coordinate that is not finite or whose magnitude reaches 2^30 gives a zero plane (the reference's
 *   conversion is undefined there).  The rule equals the reference's paste_mask_in_image wherever its slice bounds are non-negative and
 *   inside the image; for a box wholly outside the image (bx1 < -1, bx0 > w, ...) the reference raises on a shape mismatch or applies
 *   Python's negative-index slicing, and this entry writes what the rule says (zeros).  RoIHeads clips its boxes to the image, so the
 *   model never meets that case.
 * y is stored 16 bytes at a time when w is a multiple of 4 and y is 16-byte aligned, else element by element (mv_last_kernel says
 * which); masks and boxes may start at any 4-byte address.  Element offsets are 64-bit.
 *
 * mv_mask_probs_f32: logits (r, classes, mh, mw), labels (r) int64 -> y (r, mh, mw) = s(logits[i, labels[i]]), s the sigmoid of
 * mv_retinanet_topk_f32 (1 / (1 + E(-x)), E the correctly rounded float32 exponential, the division correctly rounded).  Only the
 * selected plane of a roi is read.  A label outside [0, classes) gives a zero plane and nothing is read through it (the reference
 * would raise; the library does not read labels back).
 *
 * mv_conv_transpose2x2_bias_act_f32: ConvTranspose2d(kernel_size 2, stride 2, padding 0, output_padding 0, groups 1, dilation 1) +
 * bias + activation, x (n, cin, h, w) -> y (n, cout, 2 h, 2 w):
 *   y[b, co, 2 i + dy, 2 j + dx] = act(bias4[q] + sum_ci x[b, ci, i, j] * w4[q, ci]),   q = 4 co + 2 dy + dx
 * `w4` is the RELAID weight (4 cout, cin), row q = torch's weight[:, co, dy, dx]; `bias4` (4 cout) the bias with every entry
 * repeated four times, or NULL.  It is the pointwise kernel of mv_conv_norm_act_f32 (MV_CONV_PW1X1) on 4 cout channels with the same
 * plan, tiles, K chunks and K slices, whose store is the pixel shuffle: the summation order is, by construction, exactly the one
 * mv_conv1x1_k_slices(n, cin, h, w, 4 cout) states, then `+ bias`, then the activation (MV_ACT_NONE / RELU / RELU6).  The
 * (n, 4 cout, h, w) intermediate never reaches memory and y is written once, 16 bytes at a time when w is even and y is 16-byte
 * aligned, else element by element (mv_last_kernel says which).
 *
 * Refused before any launch (MV_ERR_INVALID_ARGUMENT unless said), writing nothing: a null pointer (bias4 may be null), a non-positive
 * m / h / w / classes / cin / cout, a negative r, n or padding, an activation code other than the three, an output that overlaps an
 * input (byte ranges), sizes that exceed the address space, more workgroups than one launch grid holds (MV_ERR_UNSUPPORTED).
 * r == 0 / n == 0 is a no-op that touches no pointer. */
int mv_paste_masks_f32(const float* masks, const float* boxes, float* y, int64_t r, int m, int padding, int h, int w, void* stream);
int mv_mask_probs_f32(const float* logits, const int64_t* labels, float* y, int64_t r, int classes, int mh, int mw, void* stream);
int mv_conv_transpose2x2_bias_act_f32(const float* x, const float* w4, const float* bias4, float* y, int64_t n, int cin, int h, int w,
                                      int cout, int act, void* stream);

/* ---- The keypoint branch of Keypoint R-CNN (models/detection/keypoint_rcnn.py's ConvTranspose2d(kernel 4, stride 2, padding 1);
 * roi_heads.py heatmaps_to_keypoints).  All tensors DEVICE float32.
 *
 * mv_conv_transpose4x4s2_bias_act_f32: ConvTranspose2d(kernel_size 4, stride 2, padding 1, output_padding 0, groups 1, dilation 1) +
 * bias + activation, x (n, cin, h, w) -> y (n, cout, 2 h, 2 w).  With xp the input zero-padded by one pixel on every side:
 *   y[b, co, 2 m + py, 2 n + px] = act(bias4[q] + sum_ci sum_ty sum_tx xp[b, ci, m + py + ty, n + px + tx] * w2[q, ci, ty, tx])
 *   q = 4 co + 2 py + px,   py, px, ty, tx in {0, 1}
 * `w2` is the RELAID weight (4 cout, cin, 2, 2), w2[q, ci, ty, tx] = torch's weight[ci, co, 3 - py - 2 ty, 3 - px - 2 tx]; `bias4`
 * (4 cout) the bias with every entry repeated four times, or NULL.  This is the 2x2 convolution with padding 1 of w2, evaluated on
 * the (h + 1) x (w + 1) grid of window positions, of which phase (py, px) keeps position (m + py, n + px).  The summation order is
 * mv_conv2d_bias_act_f32's: one accumulator per output, ascending (ci, ty, tx) from +0, then `+ bias`, then the activation
 * (MV_ACT_NONE / RELU / RELU6) -- bit for bit mv_conv2d_bias_act_f32(x, w2, bias4, padding 1) followed by that strided gather.  ONE
 * launch of the implicit-GEMM kernel with a transposed store: the (n, 4 cout, h + 1, w + 1) intermediate never reaches memory and y is
 * written once, element by element; x, w2 and y may start at any 4-byte address.  Element offsets are 64-bit.
 * MV_ERR_UNSUPPORTED beyond the kernel's index range: cin >= 16384, w + 1 >= 4096, (h + 1) (w + 1) >= 2^20, cin h w >= 2^30,
 * cout > (2^31 - 1) / 4 or n > 65535.
 *
 * mv_heatmaps_to_keypoints_f32: maps (r, k, mh, mw), rois (r, 4) rows (x1, y1, x2, y2) -> xy (r, k, 3) rows (x, y, visibility) and
 * scores (r, k), ONE launch, one workgroup per (roi, keypoint).  Every operation is rounded once to float32 and never contracted,
 * except the one fma named below.  Per roi:
 *   w  = max(x2 - x1, 1),  h = max(y2 - y1, 1),   rw = (int)ceil(w),  rh = (int)ceil(h)
 *   cx = w / float32(rw),  cy = h / float32(rh)                                    (correctly rounded divisions)
 *   roi_map[k] = bicubic(maps[r, k]; (mh, mw) -> (rh, rw))                          (never materialised)
 *   pos = the first row-major index of the maximum of roi_map[k]; a NaN counts as larger than every number and the first NaN wins
 *         (torch's CPU argmax); -0.0 and +0.0 are equal;  yi = pos / rw,  xi = pos % rw
 *   xy[r, k] = ((float)xi + 0.5f) * cx + x1,  ((float)yi + 0.5f) * cy + y1,  1.0f;    scores[r, k] = roi_map[k][yi, xi]
 * The bicubic resize is the library's own statement of interpolate(mode="bicubic", align_corners=False, antialias=False), A = -0.75.
 * Per axis, with `in` and `out` its two sizes and d the output index:
 *   s    = float32(in) / float32(out)
 *   real = fma(s, d + 0.5f, -0.5f)                        (the one fma, as in mv_interpolate_bilinear_f32; NOT clamped at 0)
 *   i0   = min((int)floor(real), in - 1),   t = clamp(real - (float)i0, 0, 1)
 *   taps clamp(i0 - 1 + j, 0, in - 1), j = 0 .. 3, with the weights c2(t + 1), c1(t), c1(1 - t), c2((1 - t) + 1)
 *   c1(x) = ((A + 2) x - (A + 3)) x x + 1,   c2(x) = ((A x - 5 A) x + 8 A) x - 4 A      (left to right, every operation rounded)
 * and the value is sum_i wy_i * (sum_j wx_j * src[y_i, x_j]): the inner sum first, each sum from its first product with the next three
 * added in order, every product and every sum rounded.  With out == in, real == d, t == 0 and the weights are 0, 1, 0, 0: the map
 * itself for finite values.  NaN and +-inf follow from the formula.  torch's CPU kernel differs from this statement by a few
 * 2^-24 max|x| (DESIGN.md 3.29 has the bound).
 *   Domain.  A roi with a coordinate that is not finite, or with rw or rh above 2^15, gives the row +0.0 (x, y, visibility and score)
 *   and nothing is read through it (the reference would fail or try to allocate the resized map).  mh * mw > 16384 (the heatmap is
 *   staged in LDS) is MV_ERR_UNSUPPORTED.
 * The rois are read on the device; nothing is allocated, read back or synchronised, and r is only a grid extent.
 *
 * Refused before any launch (MV_ERR_INVALID_ARGUMENT unless said), writing nothing: a null pointer (bias4 may be null), a non-positive
 * k / mh / mw / cin / cout / h / w, a negative r or n, an activation code other than the three, an output that overlaps an input or
 * the other output (byte ranges), sizes that exceed the address space, more workgroups than one launch grid holds.
 * r == 0 / n == 0 is a no-op that touches no pointer. */
int mv_conv_transpose4x4s2_bias_act_f32(const float* x, const float* w2, const float* bias4, float* y, int64_t n, int cin, int h, int w,
                                        int cout, int act, void* stream);
int mv_heatmaps_to_keypoints_f32(const float* maps, const float* rois, float* xy, float* scores, int64_t r, int k, int mh, int mw,
                                 void* stream);

/* ---- MobileNetV3 (models/mobilenetv3.py): depthwise 5x5 blocks, squeeze-excitation (ops/misc.py SqueezeExcitation), the dense layer
 * with Hardswish of the classifier.  All DEVICE pointers, float32, 4-byte aligned; every entry is ONE launch, nothing read back.
 *
 * mv_dwconv_norm_act_f32: depthwise conv, a k x k kernel per channel, w (c, 1, k, k), zero padding (k - 1) / 2, stride 1 | 2,
 *   x (n, c, h, w) -> y (n, c, (h - 1) / stride + 1, (w - 1) / stride + 1), then the epilogue of mv_conv_norm_act_f32 in its order:
 *   `+ bias` -> folded norm (affine) -> `residual + v` -> activation (MV_ACT_NONE .. MV_ACT_SILU).  k == 3 IS
 *   mv_conv_norm_act_f32(MV_CONV_DW3X3): the same kernels, the same bits.  k == 5 (k_dwpc5x5): one float32 accumulator per output,
 *   acc = fmaf(w[ky][kx], x[iy][ix], acc) in ascending (ky, kx) order from +0, a tap in the padding entering the chain as +0 --
 *   oracle/oracle.c::orc_conv2d_affine_act_f32 with groups = c.  The bits do not depend on the alignment of x or on the launch.
 *   Any other k is MV_ERR_UNSUPPORTED; the other refusals are those of mv_conv_norm_act_f32.  It is the dilation == 1 call of:
 *
 * mv_dwconv_dilated_norm_act_f32: the same with a dilation.  dilation == 1 IS mv_dwconv_norm_act_f32: the same kernels, the same bits,
 *   the same refusals in the same order.  dilation == 2 needs k == 5 and stride == 1 (the dilated blocks of MobileNetV3 as a segmentation
 *   backbone; zero padding 4, y (n, c, h, w)); every other dilated geometry is MV_ERR_UNSUPPORTED, dilation < 1 MV_ERR_INVALID_ARGUMENT.
 *   Arithmetic (k_dwpc5x5<1, 2>): one float32 accumulator per output, acc = fmaf(w[ky][kx], x[oy - 4 + 2 ky][ox - 4 + 2 kx], acc) in
 *   ascending (ky, kx) order from +0, a tap in the padding entering the chain as +0, then the epilogue above -- orc_conv2d_affine_act_f32
 *   with groups = c on the kernel zero-stuffed to 9 x 9.  The bits do not depend on the alignment of x, on the launch or on n.
 *
 * mv_global_avgpool_f64sum_f32: y[i][c] = the mean of plane (i, c) of x (n, c, h, w), image i at x + i x_stride (elements, >= c h w: a
 *   channel slice of a wider tensor is passed as it is), y (n, c) dense.  With P = h w and p the index inside the plane:
 *     lane   element p belongs to lane l = (p / 4) mod 64;  S[l] = the sum of (double)x[p] over the lane's elements, added one after
 *            the other in ascending p to 0.0 in float64 (a lane without an element is 0.0);
 *     tree   for off = 32, 16, 8, 4, 2, 1:  S[l] = S[l] + S[l + off] for every l < off;
 *     mean   y = (float)(S[0] / (double)P): a float64 division, rounded once to float32.
 *   The result of a plane is a function of its P values alone: not of n, c, the plane's place or alignment, or the width of the loads.
 *   NaN / +-inf in a plane reach that plane's mean only.  (mv_adaptive_avgpool_f32 keeps its float32 chain.)
 *
 * mv_linear_act_f32: y (n, m) = act(x (n, k) w (m, k)^T + b (m, or NULL)).  Per output (i, j):
 *     lane   S[l] = the sum of the exact float64 products (double)x[i][q] (double)w[j][q] over q = l, l + 64, l + 128, ... < k, added
 *            in ascending q to 0.0 in float64;  the tree above;
 *     v      (float)(S[0] + (double)b[j]), without the addend when b is NULL;
 *     act    MV_ACT_NONE: v;  MV_ACT_RELU: v < 0 ? 0 : v;  with t = clamp(fl(v + 3), 0, 6) (torch.clamp: a NaN stays)
 *            MV_ACT_HARDSWISH: fl(fl(v t) / 6),  MV_ACT_HARDSIGMOID: fl(t / 6), IEEE divisions;  MV_ACT_SIGMOID:
 *            fl(1 / fl(1 + E(-v))) with E the correctly rounded float32 exp (mv_rpn_decode_f32's sigmoid).
 *   A NaN v gives NaN under every activation; hardswish(-inf) is NaN (-inf * 0), as torch's.  An output depends on its row of x, its
 *   row of w and b[j] alone: not on n, m or its indices.  Other activation codes are MV_ERR_INVALID_ARGUMENT; n <= 65535.
 *
 * mv_se_scale_f32: y[i][c][p] = fl(gate[i][c] x[i][c][p]) on dense (n, c, h, w), gate (n, c).  y may be x itself (in place).
 *
 * mv_conv1x1_scaled_f32: the pointwise conv of mv_conv_norm_act_f32 (MV_CONV_PW1X1) on x[i][q][p] scaled by gate[i][q] (n, cin), the
 *   gate multiplied into the kernel's loads (k_conv1x1_sc): the same tiles, plan and summation order (mv_conv1x1_k_slices(n, cin, h, w,
 *   cout)), the same epilogue.  Bit for bit mv_conv_norm_act_f32(MV_CONV_PW1X1) on the output of mv_se_scale_f32(x, gate), without that
 *   tensor in memory.  n <= 65535 as there.
 *
 * mv_conv1x1_gated_upsample_f32 (LRASPP's head, models/segmentation/lraspp.py: high_classifier over the resized gated map, plus
 *   low_classifier's output): y (n, cout, oh, ow) = residual + (w (cout, cin) . U + bias), U (n, cin, oh, ow) = mv_interpolate_bilinear_f32's
 *   (h, w) -> (oh, ow) resize of mv_se_scale_f32(x, gate), x (n, cin, h, w), gate (n, cin).  U is computed in the kernel's loads
 *   (k_conv1x1_gu): each of the four taps is fl(gate[i][q] x[i][q][tap]), taps and weights per axis and the three-step blend are those
 *   stated for mv_interpolate_bilinear_f32, every product and fma rounded once; then the pointwise chain in the summation order
 *   mv_conv1x1_k_slices(n, cin, oh, ow, cout) states, `+ bias`, `residual + v`.  No norm, no activation.  Bit for bit, NaN included,
 *   mv_conv_norm_act_f32(MV_CONV_PW1X1) on mv_interpolate_bilinear_f32 of mv_se_scale_f32(x, gate), with neither tensor in memory.
 *   bias and residual may be null; the residual may be y itself (each element is read before it is written) but must not otherwise
 *   overlap it.  n <= 65535; cin h w < 2^31.
 *
 * Refused before any launch (MV_ERR_INVALID_ARGUMENT unless said), writing nothing: a null pointer (bias, residual and b may be null), a
 * non-positive c / cin / cout / h / w / oh / ow / k / m, a negative n, an unknown affine or activation code, an image stride below c h w, a
 * misaligned pointer (pool, scale), y overlapping an input (mv_se_scale_f32: other than y == x), a plane, an image or a grid beyond
 * what one launch indexes (MV_ERR_UNSUPPORTED).  n == 0 is a no-op that touches no pointer. */
#define MV_ACT_HARDSIGMOID 5 /* mv_linear_act_f32 only */
#define MV_ACT_SIGMOID 6     /* mv_linear_act_f32 only */
int mv_dwconv_norm_act_f32(const float* x, const float* w, const float* bias, const float* alpha, const float* beta, const float* residual,
                           float* y, int64_t n, int c, int h, int wdt, int k, int stride, int affine, int act, void* stream);
int mv_dwconv_dilated_norm_act_f32(const float* x, const float* w, const float* bias, const float* alpha, const float* beta,
                                   const float* residual, float* y, int64_t n, int c, int h, int wdt, int k, int stride, int dilation,
                                   int affine, int act, void* stream);
int mv_global_avgpool_f64sum_f32(const float* x, float* y, int64_t n, int c, int h, int wdt, int64_t x_stride, void* stream);
int mv_linear_act_f32(const float* x, const float* w, const float* b, float* y, int64_t n, int k, int m, int act, void* stream);
int mv_se_scale_f32(const float* x, const float* gate, float* y, int64_t n, int c, int h, int wdt, void* stream);
int mv_conv1x1_scaled_f32(const float* x, const float* gate, const float* w, const float* bias, const float* alpha, const float* beta,
                          const float* residual, float* y, int64_t n, int cin, int h, int wdt, int cout, int affine, int act,
                          void* stream);
int mv_conv1x1_gated_upsample_f32(const float* x, const float* gate, const float* w, const float* bias, const float* residual, float* y,
                                  int64_t n, int cin, int h, int wdt, int oh, int ow, int cout, void* stream);

/* ---- SSDlite's depthwise-separable block (models/detection/ssdlite.py _prediction_block, the back half of _extra_block) ----------------
 * mv_dwconv3x3_conv1x1_f32: y (n, cout, oh, ow) = the pointwise conv w (cout, cin) of mv_conv_norm_act_f32 (MV_CONV_PW1X1) with its whole
 *   epilogue (bias, alpha / beta under `affine`, residual (n, cout, oh, ow), `act`) over H (n, cin, oh, ow) = mv_conv_norm_act_f32
 *   (MV_CONV_DW3X3) of x (n, cin, h, w): depthwise 3 x 3, zero padding 1, stride 1 | 2 (oh = (h - 1) / stride + 1), w_dw (cin, 3, 3), with
 *   the depthwise epilogue bias_dw / alpha_dw / beta_dw (cin each) under `affine_dw`, then `act_dw`.  H is computed in the kernel's loads
 *   (k_conv1x1_dw) and never reaches memory: per element one float32 accumulator, acc = fmaf(w_dw[ky][kx], x[oy s - 1 + ky][ox s - 1 + kx],
 *   acc) in ascending (ky, kx) order from +0, a tap in the padding entering the chain as fmaf(w_dw, +0, acc) (a NaN or infinite weight
 *   reaches the border pixels), then `+ bias_dw`, the affine and the activation as stated for mv_conv_norm_act_f32; then the pointwise
 *   chain in the summation order mv_conv1x1_k_slices(n, cin, oh, ow, cout) states.  Bit for bit, NaN included, mv_conv_norm_act_f32
 *   (MV_CONV_PW1X1) on the output of mv_conv_norm_act_f32(MV_CONV_DW3X3), in ONE launch.  Any epilogue pointer may be null as its affine
 *   code allows.  n <= 65535; cin h w < 2^31.
 * Refused before any launch (MV_ERR_INVALID_ARGUMENT unless said), writing nothing: null x / w_dw / w / y, a non-positive cin / cout / h /
 * w, a negative n, a stride other than 1 or 2, an unknown affine or activation code of either stage, an affine code without its alpha and
 * beta, y overlapping any input, cin h w beyond the int range of the tap offsets, a plane or a batch beyond what one launch indexes
 * (MV_ERR_UNSUPPORTED).  n == 0 is a no-op that touches no pointer. */
int mv_dwconv3x3_conv1x1_f32(const float* x, const float* w_dw, const float* bias_dw, const float* alpha_dw, const float* beta_dw,
                             const float* w, const float* bias, const float* alpha, const float* beta, const float* residual, float* y,
                             int64_t n, int cin, int h, int wdt, int cout, int stride, int affine_dw, int act_dw, int affine, int act,
                             void* stream);

/* ---- ConvNeXt (models/convnext.py): depthwise 7x7, LayerNorm over the channels of an NCHW map, the per-pixel Linear + GELU ------------
 * All DEVICE pointers, float32, 4-byte aligned, dense NCHW; every entry is ONE launch, nothing read back.
 *
 * mv_dwconv7x7_bias_f32: depthwise conv, a 7 x 7 kernel per channel, w (c, 1, 7, 7), zero padding 3, stride 1, x (n, c, h, w) -> y of the
 *   same shape (k_dwpc7x7).  One float32 accumulator per output, acc = fmaf(w[ky][kx], x[oy - 3 + ky][ox - 3 + kx], acc) in ascending
 *   (ky, kx) order from +0, a tap in the padding entering the chain as +0 (never skipped: a NaN or infinite weight reaches the border
 *   pixels), then `+ bias[c]` (bias may be null: no addition) -- oracle/oracle.c::orc_conv2d_affine_act_f32 with groups = c.  The bits do
 *   not depend on the alignment of x, on the launch or on n.  mv_conv_norm_act_f32 and mv_dwconv_norm_act_f32 keep refusing k == 7.
 *
 * mv_layer_norm2d_stats_f32: mean, rstd (n, h, w) of every pixel's c values of x (n, c, h, w).  With e = (double)(float)eps:
 *     part   for g = 0 .. 15:  P[g] = the sum of (double)x[q] over the channels q = g, g + 16, g + 32, ... < c, added one after the
 *            other in ascending q to 0.0 in float64 (a group without a channel is 0.0);
 *     S      = P[0] + P[1] + ... + P[15], added in ascending g to 0.0;      m = S / (double)c
 *     Q      the same two steps over d d with d = (double)x[q] - m: the subtraction, the square and every add one float64 rounding
 *            each, never an fma
 *     mean   = (float)m,      rstd = (float)(1.0 / sqrt(Q / (double)c + e)), IEEE float64 divisions and square root.
 *   The order is the same for every shape: a pixel's pair is a function of its c values, c and eps alone -- not of n, h, w, the pixel's
 *   place or the launch.  c == 1 gives mean = x, rstd = (float)(1 / sqrt(e)); eps == 0 with a constant pixel gives rstd = +inf.
 * mv_layer_norm2d_f32 (LayerNorm2d: permute, F.layer_norm over C, permute back): with the pixel's mean and rstd as above,
 *     y[q] = fl(fl(fl(fl(x[q] - mean) rstd) weight[q]) + bias[q]),
 *   four float32 roundings, never an fma; a null weight / bias drops its step.  NaN and +-inf follow from the formula (a constant pixel
 *   at eps == 0 is 0 * inf = NaN).  torch's CPU layer_norm sums in float32 and multiplies by another association: it differs by a few
 *   float32 ulps of the result's scale, and this statement is the closer one to the float64 evaluation.
 *
 * mv_conv1x1_ln_gelu_f32: y (n, cout, h, w) = act(w (cout, cin) . Z + bias), the pointwise kernel of mv_conv_norm_act_f32 (MV_CONV_PW1X1)
 *   (k_conv1x1_ln): the same tiles, plan and summation order (mv_conv1x1_k_slices(n, cin, h, w, cout)), then `+ bias[j]` (null: no addition),
 *   then, with gelu == 1, GELU in its erf form: t = fl(v * 0.70710678118654752440f), E = (float)erf((double)t) -- the correctly rounded
 *   float32 erf, through float64 as the exp of mv_rpn_decode_f32 --, y = fl(fl(0.5f v) fl(1 + E)).  NaN gives NaN, +inf gives +inf and -inf
 *   gives NaN (-inf * 0): what the formula gives, not what another library's vector routine gives.  gelu == 0: no activation.
 *   Z = x (n, cin, h, w) when mean is null.  Otherwise Z = mv_layer_norm2d_f32's value on x, computed in the kernel's loads from mean, rstd
 *   (n, h, w) -- the outputs of mv_layer_norm2d_stats_f32 -- and ln_w, ln_b (cin each, either may be null) with the four roundings above:
 *   bit for bit, NaN included, mv_conv1x1_ln_gelu_f32(mean = NULL) on the output of mv_layer_norm2d_f32, without that tensor in memory.
 *   GELU is reachable through this entry point only: every other entry keeps refusing activation codes beyond its own.  n <= 65535.
 *
 * Refused before any launch (MV_ERR_INVALID_ARGUMENT unless said), writing nothing: a null x / w / y / mean / rstd where it is required
 * (bias, weight, ln_w, ln_b may be null; mean and rstd are both null or both set, and ln_w / ln_b need them), a negative size, cin or
 * cout or (for the norms) c of 0 on a non-empty map, eps negative, NaN or beyond float32, gelu other than 0 / 1, a misaligned pointer,
 * an output that overlaps an input or the other output, a plane, an image or a grid beyond what one launch indexes
 * (MV_ERR_UNSUPPORTED).  n == 0 or an empty plane is a no-op that touches no pointer. */
int mv_dwconv7x7_bias_f32(const float* x, const float* w, const float* bias, float* y, int64_t n, int c, int h, int wdt, void* stream);
int mv_layer_norm2d_stats_f32(const float* x, float* mean, float* rstd, int64_t n, int c, int h, int w, double eps, void* stream);
int mv_layer_norm2d_f32(const float* x, const float* weight, const float* bias, float* y, int64_t n, int c, int h, int w, double eps,
                        void* stream);
int mv_conv1x1_ln_gelu_f32(const float* x, const float* mean, const float* rstd, const float* ln_w, const float* ln_b, const float* w,
                           const float* bias, float* y, int64_t n, int cin, int h, int wdt, int cout, int gelu, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355VISION_H */
