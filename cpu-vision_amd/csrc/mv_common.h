// mv_common.h -- shared by the gfx950 kernels and the C-ABI shim.  gfx950 (CDNA4) only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/mi355vision.h"

// Tuning knobs (MV_FORCE_*, MV_*_ROWS, ...) exist only in -DMV_TUNING builds: the hook that reads the environment lives
// outside the product sources (tools/tuning/mv_tuning.h, on the include path of those builds only).  The product library
// performs no environment lookup: tune_env() is a constant there and every `if (tune_env(..))` folds away.
#ifdef MV_TUNING
#include "mv_tuning.h"
#else
namespace mv {
constexpr const char* tune_env(const char*) { return nullptr; }
}  // namespace mv
#endif

namespace mv {

constexpr int kWave = 64;          // CDNA wavefront width
constexpr int kXcds = 8;           // MI355X: 8 XCDs, each with a private 4 MiB L2
constexpr int kMaxTaps2D = MV_MAX_HOST_TAPS_2D;
constexpr int kMaxTaps1D = MV_MAX_TAPS_1D;

// ---- error plumbing (thread-local message, integer status across the ABI) --------------------
int set_error(int code, const char* fmt, ...);
// check_launch also records `what` as the calling thread's last launched kernel (mv_last_kernel()); launchers with
// template variants describe the instantiation ("k_dwtile<f32,3x3,rpt4,vec16,tw256>").
int check_launch(const char* what);
int check_launchf(const char* fmt, ...);

// ---- by-value filter taps (kernel arguments live in SGPRs: every tap is a scalar operand) ----
struct Taps2D {
  float w[kMaxTaps2D];
};
struct Taps1D {
  float x[kMaxTaps1D];
  float y[kMaxTaps1D];
};

// ---- separately allocated frames in ONE launch (mv_*_v entry points) ------------------------------
// A DataLoader hands over frames that were allocated one by one; a launch per 1080p frame is launch-bound (14 us = 44 % of HBM
// peak).  The *_v entries pass a table of per-frame base pointers BY VALUE in the kernel arguments (no device allocation, no
// host-to-device copy): plane p belongs to frame p / ppf and starts (p % ppf) planes into it.  n == 0: the contiguous layout.
constexpr int kMaxFrames = 112;  // 112 x 16 B = 1792 B of the 4 KB kernel-argument segment; longer lists go in several launches
struct FramePtrs {
  const void* x[kMaxFrames];
  void* y[kMaxFrames];
  int ppf;  // planes per frame
  int n;    // frames in the table (0 = unused)
};
// The table of the *_v call in progress on this thread (nullptr outside one); launchers copy it into their kernel arguments.
const FramePtrs* call_frames();
inline void fill_frames(FramePtrs& dst) {
  if (const FramePtrs* f = call_frames()) dst = *f; else dst.n = 0, dst.ppf = 1;
}
template <typename T>
__device__ inline const T* frame_in(const FramePtrs& fp, const void* x, long long plane, size_t plane_elems) {
  if (fp.n == 0) return static_cast<const T*>(x) + (size_t)plane * plane_elems;
  const long long f = plane / fp.ppf;
  return static_cast<const T*>(fp.x[f]) + (size_t)(plane - f * fp.ppf) * plane_elems;
}
template <typename T>
__device__ inline T* frame_out(const FramePtrs& fp, void* y, long long plane, size_t plane_elems) {
  if (fp.n == 0) return static_cast<T*>(y) + (size_t)plane * plane_elems;
  const long long f = plane / fp.ppf;
  return static_cast<T*>(fp.y[f]) + (size_t)(plane - f * fp.ppf) * plane_elems;
}

// ---- index helpers ---------------------------------------------------------------------------
// ATen reflection_pad2d index map, made total by a final clamp (positions that no valid output
// needs may land outside one reflection).
__host__ __device__ inline int reflect_clamp(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  i = i < 0 ? 0 : i;
  return i >= n ? n - 1 : i;
}

// XCD-aware block remap (T1 in the CDNA guide): blocks are dealt round-robin over the 8 XCDs, so
// block b and b+8 share an L2.  Give every XCD one contiguous chunk of the work list, so that
// vertically adjacent strips (which share halo rows) meet in the same L2.  Bijective for any grid.
__device__ inline unsigned xcd_remap(unsigned bid, unsigned nblocks) {
  unsigned per = nblocks / kXcds, rem = nblocks % kXcds;
  unsigned xcd = bid % kXcds, idx = bid / kXcds;
  // XCDs [0, rem) own per+1 blocks, the rest own per blocks
  unsigned start = xcd * per + (xcd < rem ? xcd : rem);
  return start + idx;
}

// round-half-to-even to uint8, as torch.round_() followed by .to(torch.uint8) on in-range values
__device__ inline unsigned char round_u8(float v) { return (unsigned char)(int)__builtin_rintf(v); }

// ---- centred zero-padding of host taps to a larger odd size that has a specialised kernel ------------------------------------
// A zero tap is an exact no-op of the fma chain: the padded kernel gives the same bits.
inline void center_pad(const float* src, int k, float* dst, int n) {
  for (int i = 0; i < n; ++i) dst[i] = 0.f;
  for (int i = 0; i < k; ++i) dst[(n - k) / 2 + i] = src[i];
}
// row-major ky x kx taps into ty x tx
inline void center_pad2d(const float* src, int ky, int kx, float* dst, int ty, int tx) {
  const int top = (ty - ky) / 2;
  for (int j = 0; j < ty; ++j) {
    if (j >= top && j < top + ky) center_pad(src + (j - top) * kx, kx, dst + j * tx, tx);
    else for (int i = 0; i < tx; ++i) dst[j * tx + i] = 0.f;
  }
}

// ---- exact uint8 Gaussian blur at separable cost (tiefix_u8.hip) --------------------------------------------------------------
// The reference rounds ONE 2-D fp32 chain per pixel (V2); the separable pair (V1) is another association of the same sum and
// differs from it by at most M = (kx * ky + kx + ky + 2) * 2^-17 (proof in tiefix_u8.hip), so round(V1) == round(V2) whenever V1
// is farther than M from every rounding tie n + 0.5.  The separable kernels therefore flag the few lane-rows that hold a value
// within M of a tie and append them here; k_u8_tie_fixup recomputes exactly those pixels with the reference's 2-D chain.
// The list is kTieSegs independent segments, each with its own counter: every wave publishes its strip's batch with ONE atomic
// add, and ~10 k of those to a single address serialised in L2 (9 x 9 on 32 x 4K: 0.83 ms against 0.60 ms with the atomic
// compiled out).  A wave picks its segment from its workgroup id, so 64 counters see 1 / 64 of the adds each.
constexpr int kTieSegs = 64;
struct TieList {
  unsigned count;      // total lane-rows appended (written by k_u8_tie_fixup: a diagnostic, tools/dbg_ties.py)
  unsigned capacity;   // entries that fit PER SEGMENT
  unsigned npx;        // pixels per entry (16: k_dwk_u8, 4 or 2: k_sepstream)
  unsigned pad;        // non-zero: some wave's LDS batch overflowed -> the fix-up recomputes every pixel
  unsigned seg_count[kTieSegs];  // lane-rows appended to each segment (may exceed capacity: then the fix-up recomputes EVERY pixel)
  unsigned long long idx[1];     // segment s at idx[s * capacity]: linear index (plane * h + y) * w + x of an entry's first pixel
};
// Flagged lane-rows are collected per WAVE in LDS and published ONCE, after the wave's strip: no global memory operation sits
// inside the row loop.  (A global atomic per flagged wave-row -- 475 k adds to one counter for 5x5 on 32 x 4K -- serialised in
// L2 and cost 12 ms; a flush inside the loop, however rare, made the compiler wait with vmcnt(0) for the prefetch ring on
// every row and doubled the kernel's time.)  A wave whose buffer fills up (an image built on rounding ties) drops the rest and
// raises TieList::pad: the fix-up then recomputes every pixel.  Every lane of the wave calls tie_push / tie_flush.
struct TieWave {
  unsigned long long* buf;  // wave-private LDS: `cap` entries + 64 dump slots (tie_push)
  int n, cap, over;         // wave-uniform
};
// BRANCH-FREE on purpose: tie_push sits in the row loop of kernels whose prefetch ring depends on that loop being one basic block
// (the compiler counts the loads in flight only across straight-line code).  With `if (no lane flagged) return;` in front, the 9 x 9
// pair + tie check ran 0.86 ms against 0.51 ms with the push compiled out.  Lanes without a flag (and every lane once the buffer
// is full) store into a dump area of 64 entries behind the `cap` usable ones: the buffer holds cap + 64.
__device__ inline void tie_push(TieWave& W, bool flag, unsigned long long first_pixel, int lane) {
  const unsigned long long m = __ballot(flag);
  const int add = __popcll(m);
  const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
  const bool fits = W.n + add <= W.cap;  // wave-uniform
  W.buf[(flag && fits) ? W.n + rank : W.cap + lane] = first_pixel;
  W.over |= fits ? 0 : 1;
  W.n += fits ? add : 0;
}
__device__ inline void tie_flush(TieList* T, const TieWave& W, int lane, unsigned seg) {
  if (W.over && lane == 0) atomicOr(&T->pad, 1u);
  if (W.n == 0) return;
  seg &= kTieSegs - 1;
  unsigned base = 0;
  if (lane == 0) base = atomicAdd(&T->seg_count[seg], (unsigned)W.n);
  base = __builtin_amdgcn_readfirstlane(base);
  const unsigned cap = T->capacity;
  for (int i = lane; i < W.n; i += kWave)
    if (base + i < cap) T->idx[(size_t)seg * cap + base + i] = W.buf[i];
}
// flag threshold on |v - rint(v)|: a value is "near a tie" when that distance exceeds 0.5 - M (with a little slack)
inline float tie_threshold(int kx, int ky) {
  const float m = (float)(kx * ky + kx + ky + 2) * (1.0f / 131072.0f);
  return 0.5f - (m * 1.0625f + 1e-6f);
}
int64_t u8_tie_workspace_bytes(int64_t planes, int h, int w, int npx);
int hybrid_npx(int kx, int ky);  // pixels per tie-list entry: 16 on k_dwk_u8's separable form, else k_sepstream's
bool gaussian_blur_u8_hybrid_supported(int h, int w, int kx, int ky);
int launch_gaussian_blur_u8_hybrid(const uint8_t* x, uint8_t* y, int64_t planes, int h, int w, const float* k1d_x, int kx,
                                   const float* k1d_y, int ky, void* workspace, int64_t workspace_bytes, hipStream_t s);

// ---- launchers implemented in the .hip files -------------------------------------------------
// 3x3 family (dw3x3.hip).  mode: 0 = single filter, 1 = sobel (two outputs), 2 = sharpness v2, 3 = sharpness v1
int launch_dw3x3_f32(const float* x, float* y0, float* y1, const float* w9a, const float* w9b, int64_t planes, int h,
                     int w, int border, hipStream_t s);
int launch_dw3x3_u8(const uint8_t* x, uint8_t* y, const float* w9, int64_t planes, int h, int w, int border,
                    hipStream_t s);
int launch_sharpness(const void* x, void* y, bool u8, int64_t planes, int h, int w, double factor, int v1,
                     float bound, int round_blur, hipStream_t s);
// uint8 KY x KX in {3,5,7}^2 \ {3x3}, 16 pixels per lane (dwk_u8.hip)
bool dwk_u8x16_supported(const uint8_t* x, const uint8_t* y, int h, int w, int ky, int kx, int border);
int launch_dwk_u8x16(const uint8_t* x, uint8_t* y, const float* w2d, const float* k1d_x, const float* k1d_y,
                     int64_t planes, int h, int w, int ky, int kx, int border, hipStream_t s);
// the same lane layout, separable form (row pass then systolic column chain), reflect border.  Sides of 1 count as 3 (the
// launcher zero-pads them); the side pairs built are {3, 5, 7}^2 and 9 x 7, 7 x 9, 9 x 9.
bool sep_u8x16_sides(int ky, int kx);
bool sep_u8x16_supported(int h, int w, int ky, int kx);
bool sep_u8x16_ties_supported(int h, int w, int ky, int kx);  // the instantiation with the tie check: full 64-lane rows, no byte path
int launch_sep_u8x16(const uint8_t* x, uint8_t* y, const float* k1d_x, const float* k1d_y, int64_t planes, int h, int w, int ky,
                     int kx, hipStream_t s, TieList* ties = nullptr, float tie_thresh = 0.f);
// generic LDS-tiled depthwise (dwtile.hip)
// storage types of the tile kernel
enum { kDtF32 = 0, kDtU8 = 1, kDtF16 = 2, kDtBF16 = 3 };
int launch_dwtile(const void* x, void* y, int dtype, const float* w2d_host, const float* w_dev, const float* k1d_x,
                  const float* k1d_y, int64_t planes, int h, int w, int ky, int kx, int border, hipStream_t s);
// float64 images (dwf64.hip): taps as fp64 1-D pairs (outer product formed in-kernel) or a device (ky, kx) array
int launch_dwf64(const double* x, double* y, const double* w2d_dev, const double* k1d_x, const double* k1d_y, int64_t planes,
                 int h, int w, int ky, int kx, int border, hipStream_t s);
int launch_sharpness_f64(const double* x, double* y, int64_t planes, int h, int w, double factor, int v1, hipStream_t s);
// separable blur and blur+sobel (separable.hip)
int launch_separable(const float* x, float* y, float* gx, float* gy, bool sobel, int64_t planes, int h, int w,
                     const float* k1d_x, int kx, const float* k1d_y, int ky, hipStream_t s);
// register-streaming separable / fused sobel for K in {3,5,7}, aligned rows (sepfast.hip)
bool sepfast_supported(const float* x, const float* o1, const float* o2, int h, int w, int kx, int ky, bool sobel);
int launch_sepfast(const float* x, float* y, float* gx, float* gy, bool sobel, int64_t planes, int h, int w,
                   const float* k1d_x, const float* k1d_y, int k, hipStream_t s);
// row-streaming separable blur for large kernels, 8 < K <= 63 (sepstream.hip)
bool sepstream_supported(const void* x, const void* y, bool u8, int h, int w, int kx, int ky);
int launch_sepstream(const void* x, void* y, bool u8, int64_t planes, int h, int w, const float* k1d_x, int kx,
                     const float* k1d_y, int ky, hipStream_t s, TieList* ties = nullptr, float tie_thresh = 0.f);
int sepstream_u8_pixels_per_lane(int kx, int ky);
// implicit-GEMM conv3x3 + bias + relu on the fp32 MFMA (conv3x3_mfma.hip)
int launch_conv3x3(const float* x, const float* w, const float* b, float* y, int64_t n, int cin, int h, int wdt,
                   int cout, int relu, hipStream_t s);

// uint8 3x3 with 16 pixels per lane (dw3x3_u8.hip): epi 0 = filter, 2 = sharpness v2, 3 = sharpness v1
bool dw3x3_u8x16_supported(const uint8_t* x, const uint8_t* y, int h, int w);
int launch_dw3x3_u8x16(const uint8_t* x, uint8_t* y, const float* w9, int64_t planes, int h, int w, int border, int epi,
                       double factor, hipStream_t s);
// first-layer specialisation: cin = 3, cout <= 64, 16-byte stores (conv3x3_c3.hip)
bool conv3x3_c3_supported(const float* x, const float* y, int cin, int cout, int h, int w);
int launch_conv3x3_c3(const void* x, bool in_u8, const float* mean3, const float* std3, const float* w, const float* b,
                      float* y, int64_t n, int h, int wdt, int cout, int relu, hipStream_t s);
int launch_to_float_normalize(const void* x, float* y, bool u8, int64_t n, int c, int64_t hw, const float* mean,
                              const float* stdv, hipStream_t s);

// general-cin conv3x3 (K-chunked MFMA, conv3x3_gen.hip) and the pooling layers (cnn_ops.hip)
bool conv3x3_gen_supported(int cin, int cout, int h, int w);
int launch_conv3x3_gen(const float* x, const float* w, const float* b, float* y, int64_t n, int cin, int h, int wdt,
                       int cout, int relu, hipStream_t s);
int launch_maxpool2x2(const float* x, float* y, int64_t planes, int h, int w, hipStream_t s);
int launch_linear(const float* x, const float* w, const float* b, float* y, int64_t n, int k, int m, int relu,
                  hipStream_t s);
void linear_plan(int64_t n, int k, int m, int* slices, int* slice_len);
int launch_linear_sliced(const float* x, const float* w, const float* b, float* y, int64_t n, int k, int m, int relu,
                         float* ws, hipStream_t s);
int launch_adaptive_avgpool(const float* x, float* y, int64_t planes, int h, int w, int oh, int ow, hipStream_t s);

// Conv2dNormActivation family (convnorm.hip): conv -> [+bias] -> folded norm -> [+residual] -> activation
struct Epilogue {
  const float* bias;   // [cout] or null
  const float* alpha;  // [cout] (affine != 0)
  const float* beta;
  const float* res;    // same shape as y, or null
  int affine, act;     // affine: 0 none, 1 x*a then +b (FrozenBatchNorm2d), 2 fma(x, a, b) (BatchNorm2d eval)
};
int launch_dwpc3x3(const float* x, const float* w, float* y, int64_t n, int c, int h, int wd, int stride, const Epilogue& e,
                   hipStream_t s);
int launch_conv3x3_smallcin(const float* x, const float* w, float* y, int64_t n, int cin, int h, int wd, int cout, int stride,
                            const Epilogue& e, hipStream_t s);
// x_img_stride / y_img_stride: floats between consecutive images (0 = dense: cin*hw / cout*hw); a channel slice of a
// wider tensor passes the full tensor's strides (the weight groups of the columns form, launch_conv2d_columns)
int launch_conv1x1(const float* x, const float* w, float* y, int64_t n, int cin, int64_t hw, int cout, const Epilogue& e,
                   hipStream_t s, int64_t x_img_stride = 0, int64_t y_img_stride = 0, bool allow_k_slices = true);
// the K slicing launch_conv1x1 applies to this shape: slices == 1 -> one ascending-k chain per output; otherwise `slices`
// chains over `slice_len` channels each (the last may be shorter), added in ascending slice order
void conv1x1_plan(int64_t n, int cin, int64_t hw, int cout, int* slices, int* slice_len);
// FPN's top-down merge: launch_conv1x1 on (n, cin, h, wd) whose residual is top (n, cout, top_h, top_w) read at ATen's nearest
// source index of each output pixel (k_conv1x1_up: the same plan, tiles and summation order; e.res must be null)
int launch_conv1x1_upsample_add(const float* x, const float* w, const float* top, float* y, int64_t n, int cin, int h, int wd, int cout,
                                int top_h, int top_w, const Epilogue& e, hipStream_t s);
// the pointwise kernel with a per-(image, input channel) gate multiplied into its X loads (k_conv1x1_sc: the same plan, tiles and
// summation order): bit for bit launch_conv1x1 on x[i][k][p] * gate[i * cin + k], rounded once, without that tensor in memory
int launch_conv1x1_scaled(const float* x, const float* gate, const float* w, float* y, int64_t n, int cin, int64_t hw, int cout,
                          const Epilogue& e, hipStream_t s);
// the pointwise kernel over U = the bilinear (align_corners = False) resize to (oh, ow) of fl(gate[i][k] * x[i][k]) (n, cin, h, wd), the
// product and the four-tap blend computed in its X loads (k_conv1x1_gu: the plan, tiles and summation order of launch_conv1x1 on
// (n, cin, oh * ow, cout)); neither the gated nor the resized tensor reaches memory.  LRASPP's head
int launch_conv1x1_gated_upsample(const float* x, const float* gate, const float* w, float* y, int64_t n, int cin, int h, int wd, int oh,
                                  int ow, int cout, const Epilogue& e, hipStream_t s);
// the pointwise kernel over H = the depthwise 3x3 conv (padding 1, stride 1 | 2) of x (n, cin, h, wd) through the depthwise epilogue e_dw
// (its res is ignored), computed in its X loads (k_conv1x1_dw: the plan, tiles and summation order of launch_conv1x1 on
// (n, cin, oh * ow, cout)); H never reaches memory.  Bit for bit launch_dwpc3x3 followed by launch_conv1x1.  SSDlite's prediction blocks
int launch_dwconv3x3_conv1x1(const float* x, const float* w_dw, const Epilogue& e_dw, const float* w, float* y, int64_t n, int cin, int h,
                             int wd, int cout, int stride, const Epilogue& e, hipStream_t s);
// depthwise 5x5, a kernel per channel, stride 1 | 2 with zero padding 2, or dilation 2 at stride 1 with zero padding 4 (dw5x5.hip).  A
// thread's strip is kDw5Rows output rows (of one parity at dilation 2), half of that when the launch has fewer than kDw5ShortLaunch threads
constexpr int kDw5Rows = 8;
constexpr int kDw5ShortLaunch = 16384;
int launch_dwpc5x5(const float* x, const float* w, float* y, int64_t n, int c, int h, int wd, int stride, int dilation, const Epilogue& e,
                   hipStream_t s);
// depthwise 7x7, a kernel per channel, stride 1 with zero padding 3, `+ bias` (dw7x7.hip: ConvNeXt's blocks).  A thread's strip is
// kDw7Rows output rows, half of that when the launch has fewer than kDw7ShortLaunch threads
constexpr int kDw7Rows = 8;
constexpr int kDw7ShortLaunch = 16384;
int launch_dwpc7x7(const float* x, const float* w, const float* bias, float* y, int64_t n, int c, int h, int wd, hipStream_t s);
// LayerNorm over the channels of dense NCHW images (layernorm.hip; semantics in mi355vision.h mv_layer_norm2d_f32).  y non-null: the
// normalised map (mean / rstd unused); y null: the statistics alone into mean / rstd (n, hw).  The entry points have checked the
// arguments, the extents and the grid; n, c, hw are positive and c hw < 2^31.
constexpr int kLnPixels = 16, kLnGroups = 16;  // a workgroup: 16 consecutive pixels x 16 channel groups
inline int64_t layer_norm_blocks(int64_t hw) { return (hw + kLnPixels - 1) / kLnPixels; }
int launch_layer_norm2d(const float* x, const float* weight, const float* bias, float* y, float* mean, float* rstd, int64_t n, int c,
                        int64_t hw, float eps, hipStream_t s);
// the pointwise kernel of a ConvNeXt block (k_conv1x1_ln: the plan, tiles and summation order of launch_conv1x1): with mean / rstd
// (n, hw) the X chunk's element (k, p) is fl(fl(fl(fl(x - mean[p]) rstd[p]) ln_w[k]) + ln_b[k]) (ln_w / ln_b may be null: their step is
// dropped), computed in the loads; with mean null the plain loads.  Epilogue: `+ bias`, then the erf GELU (gelu != 0) or nothing.
// kActGelu is this family's activation code inside Epilogue::act; no public entry point accepts it.
constexpr int kActGelu = 7;
int launch_conv1x1_ln_gelu(const float* x, const float* mean, const float* rstd, const float* ln_w, const float* ln_b, const float* w,
                           const float* bias, float* y, int64_t n, int cin, int64_t hw, int cout, int gelu, hipStream_t s);
// squeeze-excitation and the dense layer with an activation (se.hip; the orders are stated in mi355vision.h).  The entry points have
// checked every argument
int launch_global_avgpool(const float* x, float* y, int64_t n, int c, int hw, int64_t x_stride, hipStream_t s);
int launch_linear_act(const float* x, const float* w, const float* b, float* y, int64_t n, int k, int m, int act, hipStream_t s);
int launch_se_scale(const float* x, const float* gate, float* y, int64_t planes, int hw, hipStream_t s);
// nn.Conv2d of any geometry and deform_conv2d: mv_conv.h, mv_deform.h
int launch_maxpool2d(const float* x, float* y, int64_t planes, int h, int w, int k, int stride, hipStream_t s);
int launch_maxpool2d_pad(const float* x, float* y, int64_t planes, int h, int w, int k, int stride, int pad, hipStream_t s);
// ceil_mode=True: the output side of one axis (torch's pooling_output_shape) and the launch; 0 <= pad <= k / 2, in + 2 pad >= k
inline int maxpool_ceil_out(int in, int k, int stride, int pad) {
  int o = (int)(((long long)in + 2 * pad - k + stride - 1) / stride) + 1;
  if ((long long)(o - 1) * stride >= (long long)in + pad) --o;  // the last window would start in the right padding
  return o;
}
int launch_maxpool2d_ceil(const float* x, float* y, int64_t planes, int h, int w, int k, int stride, int pad, hipStream_t s);

// F.resize(bilinear, antialias) [+ center_crop] [+ preset tail] (resize.hip)
int64_t resize_workspace_bytes(int64_t planes, int h, int w, int oh, int ow, int ct, int cl, int ch, int cw);
// win: nullptr (the whole image), or the source window of F.resized_crop and the flips of the output; (h, w) is then the
// window's size, which is what the interpolation axes and the workspace are made from
struct ResizeWindow {
  int top, left;        // the window's corner in the (ih, iw) image; the window may reach outside it (zeros)
  int ih, iw;           // the image's own size
  int flip_h, flip_v;   // mirror the output
};
int launch_resize(const void* x, void* y, bool u8, int64_t planes, int channels, int h, int w, int oh, int ow, int ct,
                  int cl, int ch, int cw, int preset, const float* mean, const float* stdv, void* workspace,
                  int64_t workspace_bytes, hipStream_t s, const ResizeWindow* win = nullptr);

// F.pad / F.crop / F.*_flip / F.erase (crop.hip; the index maps in mi355vision.h mv_pad_crop_flip).  The entry points have
// checked the arguments (gather_axis_ok per axis) and the grid (gather_grid_fits).
bool gather_axis_ok(int in, int out, int off, int mode);
bool gather_grid_fits(int64_t planes, int oh, int ow, int elem_bytes);
int launch_gather(const void* x, void* y, int64_t planes, int channels, int elem_bytes, int ih, int iw, int oh, int ow, int top,
                  int left, int mode, int flip_h, int flip_v, const unsigned long long* fill, const void* v, int bi, int bj,
                  int bh, int bw, int v_per_pixel, hipStream_t s);
int launch_erase_box(void* y, int64_t planes, int channels, int elem_bytes, int h, int w, int bi, int bj, int bh, int bw,
                     const void* v, int v_per_pixel, hipStream_t s);

// MixUp / CutMix over a contiguous (batch, elems) batch (batchmix.hip; arithmetic in mi355vision.h mv_mixup_f32).  The entry
// points have checked the arguments and the grid (mix_grid_fits); elem_bytes of launch_mixup: 4 float32, 2 float16, 8 float64.
bool mix_grid_fits(int64_t batch, int64_t elems, int elem_bytes);
int launch_mixup(const void* x, void* y, int elem_bytes, int64_t batch, int64_t elems, double lam, hipStream_t s);
int launch_cutmix(const void* x, void* y, int64_t batch, int64_t elems, int elem_bytes, int h, int w, int x1, int y1, int x2, int y2,
                  hipStream_t s);
int launch_mixup_labels(const int64_t* labels, float* y, int64_t batch, int classes, double lam, hipStream_t s);

// ops.nms / ops.roi_align (detect.hip; semantics in mi355vision.h mv_nms_f32, mv_roi_align_f32).  The entry points have checked
// the arguments, the workspace (nms_workspace_bytes, 16-byte aligned) and the grids; n and k are positive here.
constexpr int kNmsMaxBoxes = 64 * 4096;  // the reduce phase keeps one bit per box in LDS (32 KiB at this size)
int64_t nms_workspace_bytes(int64_t n);
int launch_nms(const float* boxes, const float* scores, int n, double iou_threshold, int64_t* keep, int64_t* keep_count, void* workspace,
               hipStream_t s);
int launch_roi_align(const float* x, const float* rois, float* y, int n, int c, int h, int w, int64_t k, int pooled_h, int pooled_w,
                     float spatial_scale, int sampling_ratio, int aligned, hipStream_t s);
// ops.MultiScaleRoIAlign (detect.hip; mv_multiscale_roi_align_f32): xs / hs / ws / scales are HOST tables of `levels` <= kMaxRoiLevels
// entries, copied into the kernel arguments; checked per level as for launch_roi_align.
constexpr int kMaxRoiLevels = 8;
int launch_multiscale_roi_align(const float* const* xs, const int* hs, const int* ws, const double* scales, int levels, const float* rois,
                                const int64_t* roi_levels, float* y, int n, int c, int64_t k, int pooled_h, int pooled_w, int sampling_ratio,
                                int aligned, hipStream_t s);
// ops.box_iou / generalized_box_iou / distance_box_iou and ops.masks_to_boxes (boxes.hip; semantics in mi355vision.h).  The entry
// points have checked the arguments, the workspace and the grids (*_grid_fits); n, m (and for the masks h, w >= 0) are positive.
bool box_iou_grid_fits(int64_t n, int64_t m);
int launch_box_iou(const float* boxes1, const float* boxes2, float* out, int64_t n, int64_t m, int mode, hipStream_t s);
bool masks_to_boxes_grid_fits(int64_t n, int h);
int launch_masks_to_boxes(const void* masks, bool f32, float* boxes, int* empty_flag, int64_t n, int h, int w, void* workspace,
                          hipStream_t s);
// RegionProposalNetwork's top-k and decode, BoxCoder.decode (rpn.hip; semantics in mi355vision.h mv_rpn_topk_f32 and below).  The
// entry points have checked the arguments, the extents, the workspace and the grids.
constexpr int kMaxRpnLevels = 8;
constexpr int kRpnMaxK = 4096;  // the candidates of a level are ranked pairwise: k^2 comparisons per (image, level)
// A head's per-level NCHW maps as the rpn and retinanet entry points receive them: HOST arrays of `levels` <= kMaxRpnLevels
// entries, copied into the kernel arguments.  The top-k launchers read logits, hs, ws, as and logit_strides; the rest is null there.
struct PyramidMaps {
  const float* const* logits;
  const float* const* deltas;
  const int *hs, *ws, *as;
  const int64_t *logit_strides, *delta_strides;  // elements between the images of a level's map
  const int *strides_h, *strides_w;              // the anchor grid's steps
  int levels;
  const float* base_anchors;  // DEVICE: the (sum of as, 4) cell anchors, level after level
  // FCOS only (null elsewhere): the per-level centerness maps (n, 1, hs[l], ws[l]) and their image strides
  const float* const* ctrness;
  const int64_t* ctr_strides;
};
// BoxCoder's weights and clip as the kernels take them (decode_single, mv_boxcoder.h)
struct DecodeCoef {
  float wx, wy, ww, wh, clip;
};
inline DecodeCoef decode_coef(double wx, double wy, double ww, double wh, double clip) {
  return {(float)wx, (float)wy, (float)ww, (float)wh, (float)clip};
}
int launch_rpn_topk(const PyramidMaps& m, int n, int k, int* idx, void* workspace, hipStream_t s);
int launch_rpn_decode(const PyramidMaps& m, const float* image_sizes, const int* idx, int64_t n, int64_t k, const DecodeCoef& coef, float min_size,
                      float score_thresh, float* boxes, float* scores, int64_t* levels_out, unsigned char* valid, hipStream_t s);
int launch_box_decode(const float* boxes, const float* rel_codes, float* out, int64_t m, int classes, const DecodeCoef& coef, hipStream_t s);
// RoIHeads.postprocess_detections up to the per-image filters (roi_heads.hip; semantics in mi355vision.h mv_roi_detections_f32).  The
// entry point has checked the arguments, the extents and the grid; r and n are positive, 2 <= classes <= kRoiMaxClasses.
constexpr int kRoiMaxClasses = 2048;  // a workgroup parks four rows of exponentials in LDS: 32 KiB at this size
int launch_roi_detections(const float* logits, int64_t logit_stride, const float* deltas, int64_t delta_stride, const float* rois,
                          const float* image_sizes, int64_t r, int classes, int64_t n, const DecodeCoef& coef, float score_thresh, float min_size,
                          float* boxes, float* scores, int64_t* labels, unsigned char* valid, hipStream_t s);
// RetinaNet's threshold + top-k and decode (retinanet.hip; semantics in mi355vision.h mv_retinanet_topk_f32 and below).  The entry
// points have checked the arguments, the extents, the workspace and the grids; PyramidMaps is as for the rpn launchers.
constexpr int kRetChunk = 16384;  // elements of an (image, level) map per stage-1 workgroup: 16 per thread, in registers
struct RetinanetPlan {           // the workspace of launch_retinanet_topk: counts, then per image the pools of its levels
  int64_t chunks[kMaxRpnLevels], pool_start[kMaxRpnLevels];
  int64_t total_chunks, pool_per_image, counts_bytes, bytes;
};
RetinanetPlan retinanet_plan(int64_t n, const int* hs, const int* ws, const int* as, int levels, int classes, int k);
int launch_retinanet_topk(const PyramidMaps& m, int classes, int n, int k, float score_thresh, int* idx, void* workspace, hipStream_t s);
int launch_retinanet_decode(const PyramidMaps& m, int classes, const float* image_sizes, const int* idx, int64_t n, int64_t k,
                            const DecodeCoef& coef, float* boxes, float* scores, int64_t* labels, unsigned char* valid, hipStream_t s);
// FCOS's threshold + top-k and decode (retinanet.hip: the select / rank body of RetinaNet's with the centerness map read at the
// candidate's position; semantics in mi355vision.h mv_fcos_topk_f32 and below).  m.ctrness / m.ctr_strides are set, every as[l] is 1;
// the workspace is retinanet_plan's.
int launch_fcos_topk(const PyramidMaps& m, int classes, int n, int k, float score_thresh, int* idx, void* workspace, hipStream_t s);
int launch_fcos_decode(const PyramidMaps& m, int classes, const float* image_sizes, const int* idx, int64_t n, int64_t k, float* boxes,
                       float* scores, int64_t* labels, unsigned char* valid, hipStream_t s);
// SSD's softmax, per-class threshold + top-k and decode (ssd.hip; semantics in mi355vision.h mv_ssd_scores_f32 and below).  The entry
// points have checked the arguments, the extents and the grids.  scores: the (n, classes, V) class-major matrix, V the anchors of
// all levels; x_f, y_f: HOST arrays of `levels` floats; wh_pairs: DEVICE (sum of as, 2).
int launch_ssd_scores(const PyramidMaps& m, int classes, int n, float* scores, hipStream_t s);
int launch_ssd_topk(const float* scores, int n, int classes, int v, int k, float score_thresh, int* idx, hipStream_t s);
int launch_ssd_decode(const float* scores, const PyramidMaps& m, int classes, const float* wh_pairs, const float* x_f, const float* y_f,
                      int batch_h, int batch_w, const float* image_sizes, const int* idx, int64_t n, int64_t k, const DecodeCoef& coef,
                      float* boxes, float* scores_out, int64_t* labels, unsigned char* valid, hipStream_t s);
// GroupNorm (+ ReLU) (groupnorm.hip; semantics in mi355vision.h mv_group_norm_act_f32).  The entry point has checked the arguments,
// the extents, the workspace and the grid; n, c, h, w are positive and m = (c / groups) h w < 2^31.
constexpr int kGnChunk = 4096;  // elements of a slab per workgroup of the statistics and of the apply launch: 16 per thread
inline int64_t group_norm_chunks(int64_t m) { return (m + kGnChunk - 1) / kGnChunk; }
int launch_group_norm_act(const float* x, float* y, const float* gamma, const float* beta, int64_t n, int c, int h, int w, int groups,
                          int64_t x_stride, int64_t y_stride, float eps, int relu, void* workspace, hipStream_t s);
// weight * F.normalize(x, dim=1) (l2norm.hip; semantics in mi355vision.h mv_l2_normalize_scale_f32).  The entry point has checked
// the arguments, the extents and the grid; n, c, h, w are positive and c h w < 2^31.
constexpr int kL2Pixels = 16, kL2Groups = 16;  // a workgroup: 16 consecutive pixels x 16 channel groups
inline int64_t l2_normalize_blocks(int64_t hw) { return (hw + kL2Pixels - 1) / kL2Pixels; }
int launch_l2_normalize_scale(const float* x, float* y, const float* weight, int64_t n, int c, int h, int w, int64_t x_stride,
                              int64_t y_stride, float eps, hipStream_t s);
// F.interpolate(bilinear) and the detection transform's fused normalize + resize + batch (interp.hip; semantics in mi355vision.h
// mv_interpolate_bilinear_f32, mv_detection_batch_f32).  The tables are HOST arrays of n <= kMaxDetImages entries, copied into the kernel
// arguments; mean / stdv: c <= 16 host floats, or both null (no normalisation).  The entry points have checked the arguments, the
// extents and the grid (interp_grid_fits).
constexpr int kMaxDetImages = 64;  // 64 x 32 B = 2 KiB of the 4 KiB kernel-argument segment; longer lists go in several launches
bool interp_grid_fits(int64_t planes, int hp, int wp);
int launch_interp_batch(const float* const* xs, const int* hs, const int* ws, const int* ohs, const int* ows, int n, int c,
                        const float* mean, const float* stdv, float* y, int hp, int wp, hipStream_t s);
// F.interpolate(bilinear) + argmax over the channels, the labels of a segmentation model (segment.hip; semantics in mi355vision.h
// mv_interpolate_argmax_f32).  out_bytes 1 (uint8) or 8 (int64).  The entry point has checked the arguments, the extents and the
// grid (interp_argmax_grid_fits); n is positive.
bool interp_argmax_grid_fits(int64_t n, int oh, int ow);
int launch_interp_argmax(const float* x, void* y, int64_t n, int c, int h, int w, int oh, int ow, int out_bytes, hipStream_t s);
// Mask R-CNN's paste_masks_in_image and maskrcnn_inference (mask.hip; semantics in mi355vision.h mv_paste_masks_f32,
// mv_mask_probs_f32).  The entry points have checked the arguments, the extents and the grids (*_grid_fits); r is positive.
bool paste_masks_grid_fits(int64_t r, int h, int w);
int launch_paste_masks(const float* masks, const float* boxes, float* y, int64_t r, int m, int padding, int h, int w, hipStream_t s);
bool mask_probs_grid_fits(int64_t r, int64_t plane);
int launch_mask_probs(const float* logits, const int64_t* labels, float* y, int64_t r, int classes, int64_t plane, hipStream_t s);
// ConvTranspose2d(kernel 2, stride 2) + bias + activation: launch_conv1x1 on the relaid (4 cout, cin) weight whose store is the pixel
// shuffle (convnorm.hip, k_conv1x1_ct: the same plan, tiles and summation order; e.res must be null, e.affine 0)
int launch_conv_transpose2x2(const float* x, const float* w4, float* y, int64_t n, int cin, int h, int wd, int cout, const Epilogue& e,
                             hipStream_t s);
// ConvTranspose2d(kernel 4, stride 2, padding 1) + bias + activation: the implicit-GEMM kernel on the relaid (4 cout, cin, 2, 2) weight
// whose store keeps, per phase, the window positions of that phase (conv_igemm.hip, k_conv_igemm<.., TR>: the summation order of
// mv_conv2d_bias_act_f32; only e.bias and e.act are used).  The entry point has checked the extents the kernel's indices cover.
int launch_conv_transpose4x4s2(const float* x, const float* w2, float* y, int64_t n, int cin, int h, int wd, int cout, const Epilogue& e,
                               hipStream_t s);
// Keypoint R-CNN's heatmaps_to_keypoints (keypoint.hip; semantics in mi355vision.h mv_heatmaps_to_keypoints_f32).  The entry point has
// checked the arguments, the extents and the grid; r is positive and mh * mw <= kKpMaxPlane.
constexpr int kKpMaxPlane = 16384;  // the heatmap is staged in LDS: 64 KiB
bool heatmaps_to_keypoints_grid_fits(int64_t r, int k);
int launch_heatmaps_to_keypoints(const float* maps, const float* rois, float* xy, float* scores, int64_t r, int k, int mh, int mw,
                                 hipStream_t s);
// ops.roi_pool / ps_roi_pool / ps_roi_align (roi_pool.hip; semantics in mi355vision.h).  Checked by the entry points as for
// launch_roi_align; for the two position-sensitive ops c is a multiple of pooled_h * pooled_w.
int launch_roi_pool(const float* x, const float* rois, float* y, int* argmax, int n, int c, int h, int w, int64_t k, int pooled_h,
                    int pooled_w, float spatial_scale, hipStream_t s);
int launch_ps_roi_pool(const float* x, const float* rois, float* y, int* channel_mapping, int n, int c, int h, int w, int64_t k,
                       int pooled_h, int pooled_w, float spatial_scale, hipStream_t s);
int launch_ps_roi_align(const float* x, const float* rois, float* y, int* channel_mapping, int n, int c, int h, int w, int64_t k,
                        int pooled_h, int pooled_w, float spatial_scale, int sampling_ratio, hipStream_t s);

// F.elastic: grid_sample of every plane at identity grid + displacement (elastic.hip).  base_x / base_y: the reference's
// linspace vectors (W and H floats, device); disp (1, H, W, 2) fp32 by strides; mode 0 bilinear, 1 nearest; fill: NULL or
// `channels` host floats (plane p takes fill[p % channels]).
int launch_elastic(const void* x, void* y, bool u8, int64_t planes, int channels, int h, int w, const float* base_x,
                   const float* base_y, const float* disp, int64_t disp_sh, int64_t disp_sw, int64_t disp_sc, int mode,
                   const float* fill, hipStream_t s);

// F.affine / F.rotate / F.perspective: grid_sample of every (ih, iw) plane at a grid computed per (oh, ow) output pixel from 8
// host floats (warp.hip; layout and arithmetic in mi355vision.h mv_warp_f32).  kind 0 affine, 1 perspective; order 1 the fma
// chain, 0 the plain sum (the rounding of the reference's CPU bmm); mode 0 bilinear, 1 nearest; fill as launch_elastic.
int launch_warp(const void* x, void* y, bool u8, int64_t planes, int channels, int ih, int iw, int oh, int ow, const float* coeffs,
                int kind, int order, int mode, const float* fill, hipStream_t s);

// The v2 colour ops (color.hip; layout and arithmetic in mi355vision.h mv_color_chain_f32).  The entry points have checked
// the arguments, the workspace size (color_workspace_bytes) and the grid (color_grid_fits).
int64_t color_workspace_bytes(int64_t images, int h, int w, bool u8);
bool color_grid_fits(int64_t images, int h, int w, bool u8);
int launch_color_chain(const void* x, void* y, bool u8, int64_t images, int channels, int h, int w, const int* ops,
                       const double* factors, int n_ops, int form, void* ws, hipStream_t s);
int launch_rgb_to_grayscale(const void* x, void* y, bool u8, int64_t images, int h, int w, int out_channels, int form,
                            hipStream_t s);

// The automatic-augmentation colour ops (autoaug.hip; arithmetic in mi355vision.h mv_pointwise_f32 and below).  The entry
// points have checked the arguments, the workspace size and the grid (autoaug_grid_fits).
bool autoaug_grid_fits(int64_t planes, int64_t plane_elems, bool u8);
int64_t autocontrast_workspace_bytes(int64_t planes, int64_t plane_elems, bool u8);
int64_t equalize_workspace_bytes(int64_t planes);
int launch_pointwise(const void* x, void* y, bool u8, int64_t n, int op, double param, hipStream_t s);
int launch_autocontrast(const void* x, void* y, bool u8, int64_t planes, int64_t plane_elems, void* ws, hipStream_t s);
int launch_equalize(const void* x, void* y, bool u8, int64_t planes, int64_t plane_elems, void* ws, hipStream_t s);

}  // namespace mv
