// abi.hip -- the extern "C" surface declared in include/mi355vision.h: argument validation (the same
// conditions the reference / ATen reject, reported as status codes instead of exceptions) and dispatch
// to the gfx950 kernels.  No allocation, no synchronisation, no environment lookups, no global state but the
// thread-local error / last-kernel strings.
#include <cstdlib>
#include <cstring>

#include "mv_common.h"
#include "mv_conv.h"
#include "mv_invres.h"
#include "mv_deform.h"

namespace mv {

static thread_local char g_err[512] = "";

int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

static thread_local char g_kernel[160] = "";

int check_launch(const char* what) {
  snprintf(g_kernel, sizeof(g_kernel), "%s", what);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(MV_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return MV_OK;
}

int check_launchf(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_kernel, sizeof(g_kernel), fmt, ap);
  va_end(ap);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(MV_ERR_LAUNCH, "%s: %s", g_kernel, hipGetErrorString(e));
  return MV_OK;
}

// The frame table of the *_v call in progress on this thread: set for the duration of one dispatch, read by the launchers
// (mv_common.h: fill_frames), cleared before the entry point returns.  Call-scoped, never visible to another call.
static thread_local const FramePtrs* g_call_frames = nullptr;
const FramePtrs* call_frames() { return g_call_frames; }

// 3x3 single-output filters run on the LDS-halo-tile kernel (k_dwtile<3,3>): interleaved A/B on MI355X puts it
// 1.5-6 % ahead of the register-window kernel (k_dw3x3) and its HBM traffic is 1.000x algorithmic (vs 1.13x on
// the read side), profiles/r01_tune_dw3x3_5*.log.  MV_FORCE_REG3X3=1 selects the register kernel for A/B runs;
// the Sobel pair and adjust_sharpness always use k_dw3x3 (fused epilogues).
// Images up to 128 pixels wide (thumbnails) always take the register kernel: it packs 64 / lanes-per-row strips into a
// wave, where the 256-pixel tile would idle most of its lanes (4096x3x32x32: 101 -> 3x us).
static bool use_reg3x3(int wdt) {
  if (wdt <= 128) return true;
  const char* v = tune_env("MV_FORCE_REG3X3");
  return v && *v && *v != '0';
}

static int check_image(const void* x, const void* y, int64_t planes, int h, int w) {
  if (planes < 0 || h < 0 || w < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "negative size (planes=%lld h=%d w=%d)", (long long)planes, h, w);
  if (planes > 0 && h > 0 && w > 0 && (!x || !y)) return set_error(MV_ERR_INVALID_ARGUMENT, "null image pointer");
  if (x && x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  return MV_OK;
}

static int check_kernel_size(int ky, int kx, int h, int w, int border) {
  if (ky <= 0 || kx <= 0 || (ky & 1) == 0 || (kx & 1) == 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "kernel size must be odd and positive, got (%d, %d)", ky, kx);
  if (border != MV_BORDER_VALID && border != MV_BORDER_REFLECT && border != MV_BORDER_ZERO)
    return set_error(MV_ERR_INVALID_ARGUMENT, "unknown border mode %d", border);
  if (border == MV_BORDER_REFLECT && (ky / 2 >= h || kx / 2 >= w))
    return set_error(MV_ERR_INVALID_ARGUMENT,
                     "reflect padding (%d, %d) must be smaller than the image (%d, %d)", ky / 2, kx / 2, h, w);
  if (border == MV_BORDER_VALID && (ky > h || kx > w))
    return set_error(MV_ERR_INVALID_ARGUMENT, "valid conv: kernel (%d, %d) larger than image (%d, %d)", ky, kx, h, w);
  return MV_OK;
}

// hint: appended to the tap-count message
static int check_taps1d(const void* k1d_x, int kx, const void* k1d_y, int ky, const char* hint = "") {
  if (!k1d_x || !k1d_y) return set_error(MV_ERR_INVALID_ARGUMENT, "null tap pointer");
  if (kx > kMaxTaps1D || ky > kMaxTaps1D)
    return set_error(MV_ERR_UNSUPPORTED, "1-D kernels up to %d taps are supported, got (%d, %d)%s", kMaxTaps1D, ky, kx, hint);
  return MV_OK;
}

// The argument checks of the single-output entry points that take a pair of 1-D kernels (reflect border), in the order the
// ABI reports them.  An empty image passes: the caller returns MV_OK before dispatching.
static int check_blur1d(const void* x, const void* y, int64_t planes, int h, int w, const void* k1d_x, int kx, const void* k1d_y,
                        int ky, const char* hint = "") {
  if (int rc = check_image(x, y, planes, h, w)) return rc;
  if (planes == 0 || h == 0 || w == 0) return MV_OK;
  if (int rc = check_kernel_size(ky, kx, h, w, MV_BORDER_REFLECT)) return rc;
  return check_taps1d(k1d_x, kx, k1d_y, ky, hint);
}

// Kernel sides up to 11 of a size no specialised tile kernel is built for (1x5, 7x3, 9x1, ...) are zero-padded (centred) to
// one that is: a zero tap is an exact no-op of the fma chain, and static fmas beat taps read from LDS one by one by 3x (7x5 on
// 32 x 4K: 3.1 -> 1.5 ms).  Each side rounds up to 3 / 5 / 7 / 9 / 11.
static int tile_side(int k) { return k <= 3 ? 3 : (k <= 5 ? 5 : (k <= 7 ? 7 : (k <= 9 ? 9 : 11))); }

// The padded sides (ty, tx) of a ky x kx kernel: the tile kernels are built for equal sides and 5x3 / 3x5, the uint8 16-pixel
// kernels for any mix of 3 / 5 / 7; any other pair is squared up to its larger side.  False when the kernel stays as it is:
// a side above 11, a size that is built already, or a padded half-size that would reach past the image.
static bool fit_tile(int ky, int kx, bool u8, int h, int w, int& ty, int& tx) {
  if (ky > 11 || kx > 11) return false;
  ty = tile_side(ky), tx = tile_side(kx);
  const bool pair_ok = ty == tx || (ty <= 5 && tx <= 5) || (u8 && ty <= 7 && tx <= 7);
  if (!pair_ok) ty = tx = (ty > tx ? ty : tx);
  return (ty != ky || tx != kx) && ty / 2 < h && tx / 2 < w;
}

// fit_tile for a pair of 1-D kernels: on a fit, k1d_x / k1d_y point at the padded copies in pad_x / pad_y
static void fit_taps1d(bool u8, int h, int w, const float*& k1d_x, int& kx, const float*& k1d_y, int& ky, float (&pad_x)[11],
                       float (&pad_y)[11]) {
  int ty, tx;
  if (!fit_tile(ky, kx, u8, h, w, ty, tx)) return;
  center_pad(k1d_x, kx, pad_x, tx);
  center_pad(k1d_y, ky, pad_y, ty);
  k1d_x = pad_x, k1d_y = pad_y, kx = tx, ky = ty;
}

template <typename T>
static int depthwise(const T* x, T* y, const float* w, int w_on_device, int64_t planes, int h, int wdt, int ky, int kx,
                     int border, hipStream_t s) {
  if (int rc = check_image(x, y, planes, h, wdt)) return rc;
  if (planes == 0 || h == 0 || wdt == 0) return MV_OK;
  if (int rc = check_kernel_size(ky, kx, h, wdt, border)) return rc;
  if (!w) return set_error(MV_ERR_INVALID_ARGUMENT, "null tap pointer");
  if (!w_on_device && ky * kx > kMaxTaps2D)
    return set_error(MV_ERR_UNSUPPORTED, "%d host taps exceed MV_MAX_HOST_TAPS_2D=%d: pass a device pointer", ky * kx,
                     kMaxTaps2D);
  constexpr bool u8 = sizeof(T) == 1;
  // host taps are zero-padded to a specialised size (fit_tile); not for VALID borders (the output size follows the kernel size)
  float padded[121];
  int ty, tx;
  if (!w_on_device && border != MV_BORDER_VALID && fit_tile(ky, kx, u8, h, wdt, ty, tx)) {
    center_pad2d(w, ky, kx, padded, ty, tx);
    w = padded, ky = ty, kx = tx;
  }
  if constexpr (u8) {
    // the 16-pixel kernels narrow with a saturating pack; the reference's .to(uint8) of an out-of-range float is not
    // defined, so they only take averaging kernels (taps >= 0, sum <= 1), whose results lie in [0, 255] like a blur's
    bool averaging = !w_on_device;
    if (averaging) {
      double sum = 0.0;
      for (int i = 0; i < ky * kx; ++i) averaging = averaging && w[i] >= 0.f, sum += w[i];
      averaging = averaging && sum <= 1.0 + 1e-4;
    }
    if (averaging && ky == 3 && kx == 3 && border != MV_BORDER_VALID && dw3x3_u8x16_supported(x, y, h, wdt))
      return launch_dw3x3_u8x16(x, y, w, planes, h, wdt, border, 0, 0.0, s);
    if (averaging && dwk_u8x16_supported(x, y, h, wdt, ky, kx, border))
      return launch_dwk_u8x16(x, y, w, nullptr, nullptr, planes, h, wdt, ky, kx, border, s);
  }
  if (ky == 3 && kx == 3 && !w_on_device && border != MV_BORDER_VALID && use_reg3x3(wdt)) {
    if constexpr (u8)
      return launch_dw3x3_u8(x, y, w, planes, h, wdt, border, s);
    else
      return launch_dw3x3_f32(x, y, nullptr, w, nullptr, planes, h, wdt, border, s);
  }
  return launch_dwtile(x, y, u8, w_on_device ? nullptr : w, w_on_device ? w : nullptr, nullptr, nullptr, planes, h,
                       wdt, ky, kx, border, s);
}

template <typename T>
static int gaussian(const T* x, T* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx, const float* k1d_y,
                    int ky, hipStream_t s) {
  if (int rc = check_blur1d(x, y, planes, h, wdt, k1d_x, kx, k1d_y, ky)) return rc;
  if (planes == 0 || h == 0 || wdt == 0) return MV_OK;
  constexpr bool u8 = sizeof(T) == 1;
  // the padded outer product has exact zeros, so e.g. kernel_size = (1, 5) runs on the 3x5 kernel with the same bits
  float pad_x[11], pad_y[11];
  fit_taps1d(u8, h, wdt, k1d_x, kx, k1d_y, ky, pad_x, pad_y);
  bool u8x16 = false;
  if constexpr (u8) u8x16 = (ky == 3 && kx == 3) && dw3x3_u8x16_supported(x, y, h, wdt);
  if (ky == 3 && kx == 3 && (use_reg3x3(wdt) || u8x16)) {
    float w9[9];  // kernel2d = k1d_y[:, None] * k1d_x  (_misc.py:97): one fp32 product per tap
    for (int j = 0; j < 3; ++j)
      for (int i = 0; i < 3; ++i) w9[j * 3 + i] = k1d_y[j] * k1d_x[i];
    if constexpr (u8) {
      if (u8x16) return launch_dw3x3_u8x16(x, y, w9, planes, h, wdt, MV_BORDER_REFLECT, 0, 0.0, s);
    }
    if constexpr (u8)
      return launch_dw3x3_u8(x, y, w9, planes, h, wdt, MV_BORDER_REFLECT, s);
    else
      return launch_dw3x3_f32(x, y, nullptr, w9, nullptr, planes, h, wdt, MV_BORDER_REFLECT, s);
  }
  if constexpr (u8) {
    if (dwk_u8x16_supported(x, y, h, wdt, ky, kx, MV_BORDER_REFLECT))
      return launch_dwk_u8x16(x, y, nullptr, k1d_x, k1d_y, planes, h, wdt, ky, kx, MV_BORDER_REFLECT, s);
  }
  return launch_dwtile(x, y, u8, nullptr, nullptr, k1d_x, k1d_y, planes, h, wdt, ky, kx, MV_BORDER_REFLECT, s);
}

// ---- separately allocated frames, one launch per <= kMaxFrames frames --------------------------------------------------
// `dispatch(x0, y0, planes)` is the ordinary contiguous-batch dispatcher; it runs with the frame table in scope, so the
// kernels it launches take each plane's base from the table.  Frames whose pointers are not 16-byte aligned (the vector
// paths check the base pointer's alignment once per launch) go one launch per frame instead.
template <typename T, typename F>
static int for_frames(const T* const* xs, T* const* ys, int nframes, int64_t planes_per_frame, int h, int wdt, F dispatch) {
  if (nframes < 0 || planes_per_frame < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "negative frame count / planes per frame");
  if (nframes == 0 || planes_per_frame == 0 || h == 0 || wdt == 0) return MV_OK;
  if (!xs || !ys) return set_error(MV_ERR_INVALID_ARGUMENT, "null frame pointer table");
  bool aligned = planes_per_frame <= 0x7fffffff;
  for (int i = 0; i < nframes; ++i) {
    if (!xs[i] || !ys[i]) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer for frame %d", i);
    if ((const void*)xs[i] == (const void*)ys[i]) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input (frame %d)", i);
    aligned = aligned && (uintptr_t)xs[i] % 16 == 0 && (uintptr_t)ys[i] % 16 == 0;
  }
  if (!aligned) {
    for (int i = 0; i < nframes; ++i)
      if (int rc = dispatch(xs[i], ys[i], planes_per_frame)) return rc;
    return MV_OK;
  }
  FramePtrs fp;
  fp.ppf = (int)planes_per_frame;
  for (int i0 = 0; i0 < nframes; i0 += kMaxFrames) {
    fp.n = nframes - i0 < kMaxFrames ? nframes - i0 : kMaxFrames;
    for (int i = 0; i < fp.n; ++i) fp.x[i] = xs[i0 + i], fp.y[i] = ys[i0 + i];
    g_call_frames = &fp;
    const int rc = dispatch(xs[i0], ys[i0], (int64_t)fp.n * planes_per_frame);
    g_call_frames = nullptr;
    if (rc) return rc;
  }
  return MV_OK;
}

}  // namespace mv

using namespace mv;

extern "C" {

int mv_abi_version(void) { return MV_ABI_VERSION; }

const char* mv_last_error(void) { return g_err; }

const char* mv_last_kernel(void) { return g_kernel; }

#ifndef MV_BUILD_ID
#define MV_BUILD_ID "unknown"
#endif
#ifdef MV_TUNING
const char* mv_build_id(void) { return MV_BUILD_ID "+tuning"; }
#else
const char* mv_build_id(void) { return MV_BUILD_ID; }
#endif

int mv_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int mv_depthwise_conv2d_f32(const float* x, float* y, const float* w, int w_on_device, int64_t planes, int h, int wdt,
                            int ky, int kx, int border, void* stream) {
  return depthwise<float>(x, y, w, w_on_device, planes, h, wdt, ky, kx, border, (hipStream_t)stream);
}

int mv_depthwise_conv2d_u8(const uint8_t* x, uint8_t* y, const float* w, int w_on_device, int64_t planes, int h,
                           int wdt, int ky, int kx, int border, void* stream) {
  return depthwise<uint8_t>(x, y, w, w_on_device, planes, h, wdt, ky, kx, border, (hipStream_t)stream);
}

int mv_gaussian_blur_f32(const float* x, float* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx,
                         const float* k1d_y, int ky, void* stream) {
  return gaussian<float>(x, y, planes, h, wdt, k1d_x, kx, k1d_y, ky, (hipStream_t)stream);
}

int mv_gaussian_blur_u8(const uint8_t* x, uint8_t* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx,
                        const float* k1d_y, int ky, void* stream) {
  return gaussian<uint8_t>(x, y, planes, h, wdt, k1d_x, kx, k1d_y, ky, (hipStream_t)stream);
}

// The same result as mv_gaussian_blur_u8 (the reference's single 2-D pass), bit for bit, at the cost of the separable pair:
// tiefix_u8.hip.  Taps must be what a Gaussian is -- non-negative, sum <= 1 -- for its error bound; anything else, and every
// size / width outside the separable kernels, takes the 2-D pass.
static bool taps_are_an_average(const float* k, int n) {
  double sum = 0.0;
  for (int i = 0; i < n; ++i) {
    if (!(k[i] >= 0.f)) return false;
    sum += k[i];
  }
  return sum <= 1.0 + 1e-5;
}

int64_t mv_gaussian_blur_u8_workspace_bytes(int64_t planes, int h, int wdt, int kx, int ky) {
  if (planes <= 0 || h <= 0 || wdt <= 0 || kx < 1 || ky < 1 || !(kx & 1) || !(ky & 1)) return 0;
  if (kx / 2 >= wdt || ky / 2 >= h || !gaussian_blur_u8_hybrid_supported(h, wdt, kx, ky)) return 0;
  return u8_tie_workspace_bytes(planes, h, wdt, hybrid_npx(kx, ky));
}

int mv_gaussian_blur_u8_ws(const uint8_t* x, uint8_t* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx,
                           const float* k1d_y, int ky, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_blur1d(x, y, planes, h, wdt, k1d_x, kx, k1d_y, ky)) return rc;
  if (planes == 0 || h == 0 || wdt == 0) return MV_OK;
  const bool fast = workspace != nullptr && workspace_bytes > 0 && gaussian_blur_u8_hybrid_supported(h, wdt, kx, ky) &&
                    taps_are_an_average(k1d_x, kx) && taps_are_an_average(k1d_y, ky);
  if (!fast) return gaussian<uint8_t>(x, y, planes, h, wdt, k1d_x, kx, k1d_y, ky, (hipStream_t)stream);
  return launch_gaussian_blur_u8_hybrid(x, y, planes, h, wdt, k1d_x, kx, k1d_y, ky, workspace, workspace_bytes, (hipStream_t)stream);
}

int mv_gaussian_blur_f32_v(const float* const* xs, float* const* ys, int nframes, int64_t planes_per_frame, int h, int wdt,
                           const float* k1d_x, int kx, const float* k1d_y, int ky, void* stream) {
  return for_frames<float>(xs, ys, nframes, planes_per_frame, h, wdt, [&](const float* x, float* y, int64_t planes) {
    return gaussian<float>(x, y, planes, h, wdt, k1d_x, kx, k1d_y, ky, (hipStream_t)stream);
  });
}

int mv_gaussian_blur_u8_v(const uint8_t* const* xs, uint8_t* const* ys, int nframes, int64_t planes_per_frame, int h, int wdt,
                          const float* k1d_x, int kx, const float* k1d_y, int ky, void* stream) {
  return for_frames<uint8_t>(xs, ys, nframes, planes_per_frame, h, wdt, [&](const uint8_t* x, uint8_t* y, int64_t planes) {
    return gaussian<uint8_t>(x, y, planes, h, wdt, k1d_x, kx, k1d_y, ky, (hipStream_t)stream);
  });
}

// float64 images: the reference computes them in float64 (taps, padding and conv2d all in the image dtype)
int mv_gaussian_blur_f64(const double* x, double* y, int64_t planes, int h, int wdt, const double* k1d_x, int kx,
                         const double* k1d_y, int ky, void* stream) {
  if (int rc = check_blur1d(x, y, planes, h, wdt, k1d_x, kx, k1d_y, ky,
                            ": pass the 2-D kernel to mv_depthwise_conv2d_f64 as a device array"))
    return rc;
  if (planes == 0 || h == 0 || wdt == 0) return MV_OK;
  return launch_dwf64(x, y, nullptr, k1d_x, k1d_y, planes, h, wdt, ky, kx, MV_BORDER_REFLECT, (hipStream_t)stream);
}

int mv_depthwise_conv2d_f64(const double* x, double* y, const double* w_dev, int64_t planes, int h, int wdt, int ky, int kx,
                            int border, void* stream) {
  if (int rc = check_image(x, y, planes, h, wdt)) return rc;
  if (planes == 0 || h == 0 || wdt == 0) return MV_OK;
  if (int rc = check_kernel_size(ky, kx, h, wdt, border)) return rc;
  if (!w_dev) return set_error(MV_ERR_INVALID_ARGUMENT, "null tap pointer");
  if ((size_t)(64 + kx - 1) * (16 + ky - 1) * sizeof(double) > 160 * 1024)
    return set_error(MV_ERR_UNSUPPORTED, "fp64 filter: kernel (%d, %d) does not fit the LDS tile", ky, kx);
  return launch_dwf64(x, y, w_dev, nullptr, nullptr, planes, h, wdt, ky, kx, border, (hipStream_t)stream);
}

int mv_sharpness_f64(const double* x, double* y, int64_t planes, int h, int wdt, double sharpness_factor, int v1, void* stream) {
  if (int rc = check_image(x, y, planes, h, wdt)) return rc;
  if (!(sharpness_factor >= 0.0)) return set_error(MV_ERR_INVALID_ARGUMENT, "sharpness_factor (%g) is not non-negative.", sharpness_factor);
  if (planes == 0 || h == 0 || wdt == 0) return MV_OK;
  if (h <= 2 || wdt <= 2) {  // _color.py:240 returns the input unchanged
    if (hipMemcpyAsync(y, x, (size_t)planes * h * wdt * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
      return set_error(MV_ERR_LAUNCH, "sharpness: device copy failed");
    return MV_OK;
  }
  return launch_sharpness_f64(x, y, planes, h, wdt, sharpness_factor, v1, (hipStream_t)stream);
}

// fp16 / bf16 storage: the 2-D pass on the LDS tile kernel with fp32 arithmetic and one rounding on store.  Kernel sides up
// to 11 (zero-padded to the templated sizes like the fp32 path); larger ones return MV_ERR_UNSUPPORTED and the caller
// converts to fp32 around mv_separable_blur_f32.
static int gaussian_half(const void* x, void* y, int dtype, int64_t planes, int h, int wdt, const float* k1d_x, int kx,
                         const float* k1d_y, int ky, hipStream_t s) {
  if (int rc = check_blur1d(x, y, planes, h, wdt, k1d_x, kx, k1d_y, ky)) return rc;
  if (planes == 0 || h == 0 || wdt == 0) return MV_OK;
  if (kx > 11 || ky > 11) return set_error(MV_ERR_UNSUPPORTED, "half-precision storage: kernel sides up to 11, got (%d, %d)", ky, kx);
  float pad_x[11], pad_y[11];
  fit_taps1d(false, h, wdt, k1d_x, kx, k1d_y, ky, pad_x, pad_y);
  return launch_dwtile(x, y, dtype, nullptr, nullptr, k1d_x, k1d_y, planes, h, wdt, ky, kx, MV_BORDER_REFLECT, s);
}

int mv_gaussian_blur_f16(const void* x, void* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx, const float* k1d_y,
                         int ky, void* stream) {
  return gaussian_half(x, y, kDtF16, planes, h, wdt, k1d_x, kx, k1d_y, ky, (hipStream_t)stream);
}

int mv_gaussian_blur_bf16(const void* x, void* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx, const float* k1d_y,
                          int ky, void* stream) {
  return gaussian_half(x, y, kDtBF16, planes, h, wdt, k1d_x, kx, k1d_y, ky, (hipStream_t)stream);
}

// Unequal small kernels, e.g. GaussianBlur(kernel_size=(7, 3)): both 1-D kernels zero-padded (centred) to K = max(kx, ky, 3)
// in {3, 5, 7} run on the register-streaming k_sepfast<K>; a zero tap is an exact no-op of the fma chain, so the result
// equals the unpadded separable pair bit for bit (finite pixels).
struct PaddedTaps {
  float x[7], y[7];
  int k;
};
static bool pad_small_taps(const float* k1d_x, int kx, const float* k1d_y, int ky, PaddedTaps& p) {
  if (kx > 7 || ky > 7 || kx < 1 || ky < 1) return false;
  p.k = kx > ky ? kx : ky;
  if (p.k < 3) p.k = 3;
  center_pad(k1d_x, kx, p.x, p.k);
  center_pad(k1d_y, ky, p.y, p.k);
  return true;
}

int mv_separable_blur_f32(const float* x, float* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx,
                          const float* k1d_y, int ky, void* stream) {
  if (int rc = check_blur1d(x, y, planes, h, wdt, k1d_x, kx, k1d_y, ky)) return rc;
  if (planes == 0 || h == 0 || wdt == 0) return MV_OK;
  PaddedTaps pt;
  if (pad_small_taps(k1d_x, kx, k1d_y, ky, pt) && sepfast_supported(x, y, nullptr, h, wdt, pt.k, pt.k, false))
    return launch_sepfast(x, y, nullptr, nullptr, false, planes, h, wdt, pt.x, pt.y, pt.k, (hipStream_t)stream);
  if (sepstream_supported(x, y, false, h, wdt, kx, ky))
    return launch_sepstream(x, y, false, planes, h, wdt, k1d_x, kx, k1d_y, ky, (hipStream_t)stream);
  return launch_separable(x, y, nullptr, nullptr, false, planes, h, wdt, k1d_x, kx, k1d_y, ky, (hipStream_t)stream);
}

int mv_separable_blur_u8(const uint8_t* x, uint8_t* y, int64_t planes, int h, int wdt, const float* k1d_x, int kx,
                         const float* k1d_y, int ky, void* stream) {
  if (int rc = check_blur1d(x, y, planes, h, wdt, k1d_x, kx, k1d_y, ky)) return rc;
  if (planes == 0 || h == 0 || wdt == 0) return MV_OK;
  // small kernels: the 16-pixel-per-lane register kernel in its separable form; 9-tap sides below W = 16 take k_sepstream
  if (sep_u8x16_supported(h, wdt, ky, kx)) return launch_sep_u8x16(x, y, k1d_x, k1d_y, planes, h, wdt, ky, kx, (hipStream_t)stream);
  if (kx <= 7 && ky <= 7)
    return set_error(MV_ERR_UNSUPPORTED, "separable uint8 blur with kernel sides <= 7 needs W >= 16 (got %d): use mv_gaussian_blur_u8", wdt);
  if (!sepstream_supported(x, y, true, h, wdt, kx, ky))
    return set_error(MV_ERR_UNSUPPORTED, "separable uint8 blur with a kernel side above 7 needs K <= 63 and W >= 8");
  return launch_sepstream(x, y, true, planes, h, wdt, k1d_x, kx, k1d_y, ky, (hipStream_t)stream);
}

static const float kSobelGX[9] = {-1.f, 0.f, 1.f, -2.f, 0.f, 2.f, -1.f, 0.f, 1.f};
static const float kSobelGY[9] = {-1.f, -2.f, -1.f, 0.f, 0.f, 0.f, 1.f, 2.f, 1.f};

int mv_sobel_f32(const float* x, float* gx, float* gy, int64_t planes, int h, int wdt, int border, void* stream) {
  if (int rc = check_image(x, gx, planes, h, wdt)) return rc;
  if (int rc = check_image(x, gy, planes, h, wdt)) return rc;
  if (gx && gx == gy) return set_error(MV_ERR_INVALID_ARGUMENT, "gx and gy must be distinct buffers");
  if (planes == 0 || h == 0 || wdt == 0) return MV_OK;
  if (int rc = check_kernel_size(3, 3, h, wdt, border)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (border == MV_BORDER_VALID) {
    if (int rc = launch_dwtile(x, gx, false, kSobelGX, nullptr, nullptr, nullptr, planes, h, wdt, 3, 3, border, s)) return rc;
    return launch_dwtile(x, gy, false, kSobelGY, nullptr, nullptr, nullptr, planes, h, wdt, 3, 3, border, s);
  }
  return launch_dw3x3_f32(x, gx, gy, kSobelGX, kSobelGY, planes, h, wdt, border, s);
}

int mv_gaussian_sobel_f32(const float* x, float* gx, float* gy, int64_t planes, int h, int wdt, const float* k1d_x,
                          int kx, const float* k1d_y, int ky, void* stream) {
  if (int rc = check_image(x, gx, planes, h, wdt)) return rc;
  if (int rc = check_image(x, gy, planes, h, wdt)) return rc;
  if (gx && gx == gy) return set_error(MV_ERR_INVALID_ARGUMENT, "gx and gy must be distinct buffers");
  if (planes == 0 || h == 0 || wdt == 0) return MV_OK;
  if (int rc = check_kernel_size(ky, kx, h, wdt, MV_BORDER_REFLECT)) return rc;
  if (int rc = check_kernel_size(3, 3, h, wdt, MV_BORDER_REFLECT)) return rc;
  if (int rc = check_taps1d(k1d_x, kx, k1d_y, ky)) return rc;
  PaddedTaps pt;
  if (pad_small_taps(k1d_x, kx, k1d_y, ky, pt) && sepfast_supported(x, gx, gy, h, wdt, pt.k, pt.k, true))
    return launch_sepfast(x, nullptr, gx, gy, true, planes, h, wdt, pt.x, pt.y, pt.k, (hipStream_t)stream);
  return launch_separable(x, nullptr, gx, gy, true, planes, h, wdt, k1d_x, kx, k1d_y, ky, (hipStream_t)stream);
}

static int sharpness(const void* x, void* y, bool u8, int64_t planes, int h, int wdt, double f, int v1, float bound,
                     int round_blur, hipStream_t s) {
  if (int rc = check_image(x, y, planes, h, wdt)) return rc;
  if (!(f >= 0.0)) return set_error(MV_ERR_INVALID_ARGUMENT, "sharpness_factor (%g) is not non-negative.", f);
  if (planes == 0 || h == 0 || wdt == 0) return MV_OK;
  if (h <= 2 || wdt <= 2) {  // _color.py:240 returns the input unchanged
    const size_t bytes = (size_t)planes * h * wdt * (u8 ? 1 : 4);
    if (hipMemcpyAsync(y, x, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return set_error(MV_ERR_LAUNCH, "sharpness: device copy failed");
    return MV_OK;
  }
  if (u8 && dw3x3_u8x16_supported((const uint8_t*)x, (const uint8_t*)y, h, wdt))
    return launch_dw3x3_u8x16((const uint8_t*)x, (uint8_t*)y, nullptr, planes, h, wdt, MV_BORDER_ZERO, v1 ? 3 : 2, f, s);
  return launch_sharpness(x, y, u8, planes, h, wdt, f, v1, bound, round_blur, s);
}

int mv_sharpness_f32(const float* x, float* y, int64_t planes, int h, int wdt, double sharpness_factor, int v1,
                     float bound, int integer_semantics, void* stream) {
  if (!(bound > 0.f)) return set_error(MV_ERR_INVALID_ARGUMENT, "sharpness: bound must be positive");
  return sharpness(x, y, false, planes, h, wdt, sharpness_factor, v1, bound, integer_semantics, (hipStream_t)stream);
}

int mv_sharpness_u8(const uint8_t* x, uint8_t* y, int64_t planes, int h, int wdt, double sharpness_factor, int v1,
                    void* stream) {
  return sharpness(x, y, true, planes, h, wdt, sharpness_factor, v1, 255.f, 1, (hipStream_t)stream);
}

int mv_separable_blur_f32_v(const float* const* xs, float* const* ys, int nframes, int64_t planes_per_frame, int h, int wdt,
                            const float* k1d_x, int kx, const float* k1d_y, int ky, void* stream) {
  return for_frames<float>(xs, ys, nframes, planes_per_frame, h, wdt, [&](const float* x, float* y, int64_t planes) {
    return mv_separable_blur_f32(x, y, planes, h, wdt, k1d_x, kx, k1d_y, ky, stream);
  });
}

int mv_separable_blur_u8_v(const uint8_t* const* xs, uint8_t* const* ys, int nframes, int64_t planes_per_frame, int h, int wdt,
                           const float* k1d_x, int kx, const float* k1d_y, int ky, void* stream) {
  return for_frames<uint8_t>(xs, ys, nframes, planes_per_frame, h, wdt, [&](const uint8_t* x, uint8_t* y, int64_t planes) {
    return mv_separable_blur_u8(x, y, planes, h, wdt, k1d_x, kx, k1d_y, ky, stream);
  });
}

int mv_sharpness_f32_v(const float* const* xs, float* const* ys, int nframes, int64_t planes_per_frame, int h, int wdt,
                       double sharpness_factor, int v1, float bound, int integer_semantics, void* stream) {
  if (!(bound > 0.f)) return set_error(MV_ERR_INVALID_ARGUMENT, "sharpness: bound must be positive");
  if ((h <= 2 || wdt <= 2) && xs && ys) {  // the input is returned unchanged: one device copy per frame
    for (int i = 0; i < nframes; ++i)
      if (int rc = sharpness(xs[i], ys[i], false, planes_per_frame, h, wdt, sharpness_factor, v1, bound, integer_semantics, (hipStream_t)stream)) return rc;
    return MV_OK;
  }
  return for_frames<float>(xs, ys, nframes, planes_per_frame, h, wdt, [&](const float* x, float* y, int64_t planes) {
    return sharpness(x, y, false, planes, h, wdt, sharpness_factor, v1, bound, integer_semantics, (hipStream_t)stream);
  });
}

int mv_sharpness_u8_v(const uint8_t* const* xs, uint8_t* const* ys, int nframes, int64_t planes_per_frame, int h, int wdt,
                      double sharpness_factor, int v1, void* stream) {
  if ((h <= 2 || wdt <= 2) && xs && ys) {
    for (int i = 0; i < nframes; ++i)
      if (int rc = sharpness(xs[i], ys[i], true, planes_per_frame, h, wdt, sharpness_factor, v1, 255.f, 1, (hipStream_t)stream)) return rc;
    return MV_OK;
  }
  return for_frames<uint8_t>(xs, ys, nframes, planes_per_frame, h, wdt, [&](const uint8_t* x, uint8_t* y, int64_t planes) {
    return sharpness(x, y, true, planes, h, wdt, sharpness_factor, v1, 255.f, 1, (hipStream_t)stream);
  });
}

int mv_conv3x3_bias_relu_f32(const float* x, const float* w, const float* b, float* y, int64_t n, int cin, int h,
                             int wdt, int cout, int relu, void* stream) {
  if (n < 0 || cin <= 0 || cout <= 0 || h < 0 || wdt < 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad conv shape n=%lld cin=%d cout=%d h=%d w=%d", (long long)n, cin, cout, h, wdt);
  if (n == 0 || h == 0 || wdt == 0) return MV_OK;
  if (!x || !w || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  if (conv3x3_c3_supported(x, y, cin, cout, h, wdt))
    return launch_conv3x3_c3(x, false, nullptr, nullptr, w, b, y, n, h, wdt, cout, relu, (hipStream_t)stream);
  if (conv3x3_gen_supported(cin, cout, h, wdt))
    return launch_conv3x3_gen(x, w, b, y, n, cin, h, wdt, cout, relu, (hipStream_t)stream);
  return launch_conv3x3(x, w, b, y, n, cin, h, wdt, cout, relu, (hipStream_t)stream);
}

int mv_conv3x3_k_slices(int64_t n, int cin, int h, int wdt, int cout, int* slice_channels) {
  int slices = 1, sc = cin;
  if (n > 0 && cin > 4 && cout > 0 && h > 0 && wdt > 0) conv3x3_gen_plan(n, cin, h, wdt, cout, &slices, &sc);
  if (slice_channels) *slice_channels = sc;
  return slices;
}

int64_t mv_conv3x3_workspace_bytes(int64_t n, int cin, int h, int wdt, int cout) {
  if (n <= 0 || cin <= 4 || cout <= 0 || h <= 0 || wdt <= 0) return 0;
  return conv3x3_gen_workspace_bytes(n, cin, h, wdt, cout);
}

int mv_conv3x3_bias_relu_ws_f32(const float* x, const float* w, const float* b, float* y, int64_t n, int cin, int h, int wdt, int cout,
                                int relu, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n < 0 || cin <= 0 || cout <= 0 || h < 0 || wdt < 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad conv shape n=%lld cin=%d cout=%d h=%d w=%d", (long long)n, cin, cout, h, wdt);
  if (n == 0 || h == 0 || wdt == 0) return MV_OK;
  if (!x || !w || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  const int64_t need = mv_conv3x3_workspace_bytes(n, cin, h, wdt, cout);
  if (need == 0 || conv3x3_c3_supported(x, y, cin, cout, h, wdt) || !conv3x3_gen_supported(cin, cout, h, wdt))
    return mv_conv3x3_bias_relu_f32(x, w, b, y, n, cin, h, wdt, cout, relu, stream);  // this shape runs its single chain
  if (workspace == nullptr || workspace_bytes < need)
    return set_error(MV_ERR_INVALID_ARGUMENT, "conv3x3: workspace of %lld bytes needed (mv_conv3x3_workspace_bytes), got %lld",
                     (long long)need, (long long)workspace_bytes);
  return launch_conv3x3_gen_ws(x, w, b, y, n, cin, h, wdt, cout, relu, (hipStream_t)stream, workspace, workspace_bytes);
}

int mv_conv3x3_bias_relu_u8norm_f32(const uint8_t* x, const float* mean3, const float* std3, const float* w, const float* b,
                                    float* y, int64_t n, int h, int wdt, int cout, int relu, void* stream) {
  if (n < 0 || cout <= 0 || h < 0 || wdt < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "bad conv shape");
  if (n == 0 || h == 0 || wdt == 0) return MV_OK;
  if (!x || !w || !y || !mean3 || !std3) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  for (int i = 0; i < 3; ++i)
    if (std3[i] == 0.f) return set_error(MV_ERR_INVALID_ARGUMENT, "std evaluated to zero, leading to division by zero.");
  if (cout > 64 || wdt % 4 != 0 || (uintptr_t)y % 16 != 0 || (size_t)cout * h * wdt * sizeof(float) >= (1ull << 32))
    return set_error(MV_ERR_UNSUPPORTED, "fused uint8 first layer needs cout <= 64, W %% 4 == 0 and a 16-byte aligned output");
  return launch_conv3x3_c3(x, true, mean3, std3, w, b, y, n, h, wdt, cout, relu, (hipStream_t)stream);
}

int mv_to_float_normalize_u8(const uint8_t* x, float* y, int64_t n, int c, int64_t hw, const float* mean, const float* stdv,
                             void* stream) {
  if (n < 0 || c <= 0 || hw < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "bad shape");
  if (n == 0 || hw == 0) return MV_OK;
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if ((mean == nullptr) != (stdv == nullptr)) return set_error(MV_ERR_INVALID_ARGUMENT, "mean and std go together");
  if (stdv)
    for (int i = 0; i < c && i < 16; ++i)
      if (stdv[i] == 0.f) return set_error(MV_ERR_INVALID_ARGUMENT, "std evaluated to zero, leading to division by zero.");
  return launch_to_float_normalize(x, y, true, n, c, hw, mean, stdv, (hipStream_t)stream);
}

int mv_normalize_f32(const float* x, float* y, int64_t n, int c, int64_t hw, const float* mean, const float* stdv,
                     void* stream) {
  if (n < 0 || c <= 0 || hw < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "bad shape");
  if (n == 0 || hw == 0) return MV_OK;
  if (!x || !y || !mean || !stdv) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  for (int i = 0; i < c && i < 16; ++i)
    if (stdv[i] == 0.f) return set_error(MV_ERR_INVALID_ARGUMENT, "std evaluated to zero, leading to division by zero.");
  return launch_to_float_normalize(x, y, false, n, c, hw, mean, stdv, (hipStream_t)stream);
}

int mv_maxpool2x2_f32(const float* x, float* y, int64_t planes, int h, int wdt, void* stream) {
  if (planes < 0 || h < 0 || wdt < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "negative size");
  if (planes == 0 || h < 2 || wdt < 2) return MV_OK;
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  return launch_maxpool2x2(x, y, planes, h, wdt, (hipStream_t)stream);
}

int mv_linear_bias_relu_f32(const float* x, const float* w, const float* b, float* y, int64_t n, int k, int m, int relu,
                            void* stream) {
  if (n < 0 || k <= 0 || m <= 0) return set_error(MV_ERR_INVALID_ARGUMENT, "bad linear shape n=%lld k=%d m=%d", (long long)n, k, m);
  if (n == 0) return MV_OK;
  if (!x || !w || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  return launch_linear(x, w, b, y, n, k, m, relu, (hipStream_t)stream);
}

int mv_linear_k_slices(int64_t n, int k, int m, int* slice_len) {
  int slices = 1, len = k;
  if (n >= 0 && k > 0 && m > 0) linear_plan(n, k, m, &slices, &len);
  if (slice_len) *slice_len = len;
  return slices;
}

int64_t mv_linear_workspace_bytes(int64_t n, int k, int m) {
  if (n <= 0 || k <= 0 || m <= 0) return 0;
  int slices, len;
  linear_plan(n, k, m, &slices, &len);
  return slices > 1 ? (int64_t)slices * n * m * (int64_t)sizeof(float) : 0;
}

int mv_linear_bias_relu_ws_f32(const float* x, const float* w, const float* b, float* y, int64_t n, int k, int m, int relu,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  if (n < 0 || k <= 0 || m <= 0) return set_error(MV_ERR_INVALID_ARGUMENT, "bad linear shape n=%lld k=%d m=%d", (long long)n, k, m);
  if (n == 0) return MV_OK;
  if (!x || !w || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  if (n > 0x7fffffffLL) return set_error(MV_ERR_UNSUPPORTED, "linear: problem too large for one launch");
  const int64_t need = mv_linear_workspace_bytes(n, k, m);
  if (need == 0) return launch_linear(x, w, b, y, n, k, m, relu, (hipStream_t)stream);
  if (!workspace || workspace_bytes < need)
    return set_error(MV_ERR_INVALID_ARGUMENT, "linear: workspace of %lld bytes needed (mv_linear_workspace_bytes), got %lld",
                     (long long)need, (long long)workspace_bytes);
  if ((uintptr_t)workspace % 4 != 0) return set_error(MV_ERR_INVALID_ARGUMENT, "linear: workspace must be 4-byte aligned");
  return launch_linear_sliced(x, w, b, y, n, k, m, relu, static_cast<float*>(workspace), (hipStream_t)stream);
}

int mv_adaptive_avgpool_f32(const float* x, float* y, int64_t planes, int h, int wdt, int oh, int ow, void* stream) {
  if (planes < 0 || h <= 0 || wdt <= 0 || oh <= 0 || ow <= 0) return set_error(MV_ERR_INVALID_ARGUMENT, "bad pooling shape");
  if (planes == 0) return MV_OK;
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  return launch_adaptive_avgpool(x, y, planes, h, wdt, oh, ow, (hipStream_t)stream);
}

int mv_conv_norm_act_f32(int kind, const float* x, const float* w, const float* bias, const float* alpha, const float* beta,
                         const float* residual, float* y, int64_t n, int cin, int h, int wdt, int cout, int stride,
                         int affine, int act, void* stream) {
  if (n < 0 || cin <= 0 || cout <= 0 || h <= 0 || wdt <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad conv shape n=%lld cin=%d cout=%d h=%d w=%d", (long long)n, cin, cout, h, wdt);
  if (stride != 1 && stride != 2) return set_error(MV_ERR_INVALID_ARGUMENT, "stride should be 1 or 2 instead of %d", stride);
  if (affine < MV_AFFINE_NONE || affine > MV_AFFINE_FMA || act < MV_ACT_NONE || act > MV_ACT_SILU)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad affine (%d) / activation (%d) code", affine, act);
  if (n == 0) return MV_OK;
  if (!x || !w || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (affine != MV_AFFINE_NONE && (!alpha || !beta)) return set_error(MV_ERR_INVALID_ARGUMENT, "affine without alpha / beta");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  Epilogue e = {bias, alpha, beta, residual, affine, act};
  switch (kind) {
    case MV_CONV_DENSE3X3:
      if (cin > 4) return set_error(MV_ERR_UNSUPPORTED, "dense 3x3 with norm: cin <= 4 (the stem); got %d", cin);
      return launch_conv3x3_smallcin(x, w, y, n, cin, h, wdt, cout, stride, e, (hipStream_t)stream);
    case MV_CONV_DW3X3:
      if (cin != cout) return set_error(MV_ERR_INVALID_ARGUMENT, "depthwise: cin (%d) != cout (%d)", cin, cout);
      return launch_dwpc3x3(x, w, y, n, cin, h, wdt, stride, e, (hipStream_t)stream);
    case MV_CONV_PW1X1:
      if (stride != 1) return set_error(MV_ERR_UNSUPPORTED, "pointwise conv: stride 1 only");
      return launch_conv1x1(x, w, y, n, cin, (int64_t)h * wdt, cout, e, (hipStream_t)stream);
  }
  return set_error(MV_ERR_INVALID_ARGUMENT, "unknown conv kind %d", kind);
}

// [a, a + an) and [b, b + bn) floats share an element
static bool overlaps(const float* a, long long an, const float* b, long long bn) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bn * sizeof(float) && b0 < a0 + (uintptr_t)an * sizeof(float);
}

int mv_conv1x1_upsample_add_f32(const float* x, const float* w, const float* bias, const float* alpha, const float* beta,
                                const float* top, float* y, int64_t n, int cin, int h, int wdt, int cout, int top_h, int top_w,
                                int affine, int act, void* stream) {
  if (n < 0 || cin <= 0 || cout <= 0 || h <= 0 || wdt <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad conv shape n=%lld cin=%d cout=%d h=%d w=%d", (long long)n, cin, cout, h, wdt);
  if (top_h < 1 || top_w < 1) return set_error(MV_ERR_INVALID_ARGUMENT, "bad top size (%d, %d)", top_h, top_w);
  if (affine < MV_AFFINE_NONE || affine > MV_AFFINE_FMA || act < MV_ACT_NONE || act > MV_ACT_SILU)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad affine (%d) / activation (%d) code", affine, act);
  if (n == 0) return MV_OK;
  if (!x || !w || !y || !top) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (affine != MV_AFFINE_NONE && (!alpha || !beta)) return set_error(MV_ERR_INVALID_ARGUMENT, "affine without alpha / beta");
  const long long hw = (long long)h * wdt, ny = n * cout * hw;
  if (overlaps(y, ny, x, n * cin * hw) || overlaps(y, ny, w, (long long)cout * cin) || overlaps(y, ny, top, n * cout * (long long)top_h * top_w))
    return set_error(MV_ERR_INVALID_ARGUMENT, "output must not overlap input, weight or top");
  const Epilogue e = {bias, affine ? alpha : nullptr, affine ? beta : nullptr, nullptr, affine, act};
  return launch_conv1x1_upsample_add(x, w, top, y, n, cin, h, wdt, cout, top_h, top_w, e, (hipStream_t)stream);
}

int mv_conv1x1_k_slices(int64_t n, int cin, int h, int wdt, int cout, int* slice_len) {
  int slices = 1, len = cin;
  if (n > 0 && cin > 0 && cout > 0 && h > 0 && wdt > 0) conv1x1_plan(n, cin, (int64_t)h * wdt, cout, &slices, &len);
  if (slice_len) *slice_len = len;
  return slices;
}

// ---- MobileNetV3: depthwise 3x3 | 5x5, squeeze-excitation, the gated projection (dw5x5.hip, se.hip, convnorm.hip) -------------------
int mv_dwconv_dilated_norm_act_f32(const float* x, const float* w, const float* bias, const float* alpha, const float* beta,
                                   const float* residual, float* y, int64_t n, int c, int h, int wdt, int k, int stride, int dilation,
                                   int affine, int act, void* stream) {
  if (dilation < 1) return set_error(MV_ERR_INVALID_ARGUMENT, "dilation should be at least 1 instead of %d", dilation);
  if (k == 3 && dilation == 1)
    return mv_conv_norm_act_f32(MV_CONV_DW3X3, x, w, bias, alpha, beta, residual, y, n, c, h, wdt, c, stride, affine, act, stream);
  // the refusals of mv_conv_norm_act_f32, in its order
  if (n < 0 || c <= 0 || h <= 0 || wdt <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad conv shape n=%lld cin=%d cout=%d h=%d w=%d", (long long)n, c, c, h, wdt);
  if (stride != 1 && stride != 2) return set_error(MV_ERR_INVALID_ARGUMENT, "stride should be 1 or 2 instead of %d", stride);
  if (affine < MV_AFFINE_NONE || affine > MV_AFFINE_FMA || act < MV_ACT_NONE || act > MV_ACT_SILU)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad affine (%d) / activation (%d) code", affine, act);
  if (dilation == 1 && k != 5) return set_error(MV_ERR_UNSUPPORTED, "depthwise conv with norm: kernel 3 or 5; got %d", k);
  if (dilation != 1 && !(dilation == 2 && k == 5 && stride == 1))
    return set_error(MV_ERR_UNSUPPORTED, "dilated depthwise conv with norm: kernel 5, dilation 2, stride 1; got kernel %d, dilation %d, stride %d",
                     k, dilation, stride);
  if (n == 0) return MV_OK;
  if (!x || !w || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (affine != MV_AFFINE_NONE && (!alpha || !beta)) return set_error(MV_ERR_INVALID_ARGUMENT, "affine without alpha / beta");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  const Epilogue e = {bias, alpha, beta, residual, affine, act};
  return launch_dwpc5x5(x, w, y, n, c, h, wdt, stride, dilation, e, (hipStream_t)stream);
}

int mv_dwconv_norm_act_f32(const float* x, const float* w, const float* bias, const float* alpha, const float* beta, const float* residual,
                           float* y, int64_t n, int c, int h, int wdt, int k, int stride, int affine, int act, void* stream) {
  return mv_dwconv_dilated_norm_act_f32(x, w, bias, alpha, beta, residual, y, n, c, h, wdt, k, stride, 1, affine, act, stream);
}

int mv_conv1x1_scaled_f32(const float* x, const float* gate, const float* w, const float* bias, const float* alpha, const float* beta,
                          const float* residual, float* y, int64_t n, int cin, int h, int wdt, int cout, int affine, int act,
                          void* stream) {
  if (n < 0 || cin <= 0 || cout <= 0 || h <= 0 || wdt <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad conv shape n=%lld cin=%d cout=%d h=%d w=%d", (long long)n, cin, cout, h, wdt);
  if (affine < MV_AFFINE_NONE || affine > MV_AFFINE_FMA || act < MV_ACT_NONE || act > MV_ACT_SILU)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad affine (%d) / activation (%d) code", affine, act);
  if (n == 0) return MV_OK;
  if (!x || !gate || !w || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (affine != MV_AFFINE_NONE && (!alpha || !beta)) return set_error(MV_ERR_INVALID_ARGUMENT, "affine without alpha / beta");
  const long long hw = (long long)h * wdt, ny = n * cout * hw;
  if (overlaps(y, ny, x, n * cin * hw) || overlaps(y, ny, w, (long long)cout * cin) || overlaps(y, ny, gate, n * cin) ||
      (residual && overlaps(y, ny, residual, ny)))
    return set_error(MV_ERR_INVALID_ARGUMENT, "output must not overlap input, gate, weight or residual");
  const Epilogue e = {bias, affine ? alpha : nullptr, affine ? beta : nullptr, residual, affine, act};
  return launch_conv1x1_scaled(x, gate, w, y, n, cin, hw, cout, e, (hipStream_t)stream);
}

// ---- LRASPP's head: high_classifier over the resized gated map, low_classifier's output as the residual (convnorm.hip, k_conv1x1_gu) ---
int mv_conv1x1_gated_upsample_f32(const float* x, const float* gate, const float* w, const float* bias, const float* residual, float* y,
                                  int64_t n, int cin, int h, int wdt, int oh, int ow, int cout, void* stream) {
  if (n < 0 || cin <= 0 || cout <= 0 || h <= 0 || wdt <= 0 || oh <= 0 || ow <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad conv shape n=%lld cin=%d cout=%d (%d, %d) -> (%d, %d)", (long long)n, cin, cout, h, wdt, oh, ow);
  if (n == 0) return MV_OK;
  if (!x || !gate || !w || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  const long long hw = (long long)h * wdt, ohw = (long long)oh * ow, ny = n * cout * ohw;
  if (overlaps(y, ny, x, n * cin * hw) || overlaps(y, ny, w, (long long)cout * cin) || overlaps(y, ny, gate, n * cin) ||
      (residual && residual != y && overlaps(y, ny, residual, ny)))
    return set_error(MV_ERR_INVALID_ARGUMENT, "output must not overlap input, gate or weight, nor a residual other than itself");
  const Epilogue e = {bias, nullptr, nullptr, residual, MV_AFFINE_NONE, MV_ACT_NONE};
  return launch_conv1x1_gated_upsample(x, gate, w, y, n, cin, h, wdt, oh, ow, cout, e, (hipStream_t)stream);
}

// ---- SSDlite's depthwise-separable block: depthwise 3x3 + norm + activation in the loads of the pointwise conv (convnorm.hip, k_conv1x1_dw)
int mv_dwconv3x3_conv1x1_f32(const float* x, const float* w_dw, const float* bias_dw, const float* alpha_dw, const float* beta_dw,
                             const float* w, const float* bias, const float* alpha, const float* beta, const float* residual, float* y,
                             int64_t n, int cin, int h, int wdt, int cout, int stride, int affine_dw, int act_dw, int affine, int act,
                             void* stream) {
  if (n < 0 || cin <= 0 || cout <= 0 || h <= 0 || wdt <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad conv shape n=%lld cin=%d cout=%d h=%d w=%d", (long long)n, cin, cout, h, wdt);
  if (stride != 1 && stride != 2) return set_error(MV_ERR_INVALID_ARGUMENT, "stride should be 1 or 2 instead of %d", stride);
  if (affine_dw < MV_AFFINE_NONE || affine_dw > MV_AFFINE_FMA || act_dw < MV_ACT_NONE || act_dw > MV_ACT_SILU)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad depthwise affine (%d) / activation (%d) code", affine_dw, act_dw);
  if (affine < MV_AFFINE_NONE || affine > MV_AFFINE_FMA || act < MV_ACT_NONE || act > MV_ACT_SILU)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad affine (%d) / activation (%d) code", affine, act);
  if (n == 0) return MV_OK;
  if (!x || !w_dw || !w || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (affine_dw != MV_AFFINE_NONE && (!alpha_dw || !beta_dw))
    return set_error(MV_ERR_INVALID_ARGUMENT, "depthwise affine without alpha / beta");
  if (affine != MV_AFFINE_NONE && (!alpha || !beta)) return set_error(MV_ERR_INVALID_ARGUMENT, "affine without alpha / beta");
  // tap offsets inside a source plane and a channel's plane offset are ints
  if ((long long)cin * h * wdt > 0x7fffffffLL)
    return set_error(MV_ERR_UNSUPPORTED, "dwconv3x3_conv1x1: an image of %d x %d x %d elements exceeds the 32-bit index", cin, h, wdt);
  const long long oh = (h - 1) / stride + 1, ow = (wdt - 1) / stride + 1, ny = n * cout * oh * ow;
  const bool adw = affine_dw != MV_AFFINE_NONE, apw = affine != MV_AFFINE_NONE;
  if (overlaps(y, ny, x, n * cin * (long long)h * wdt) || overlaps(y, ny, w_dw, 9LL * cin) || overlaps(y, ny, w, (long long)cout * cin) ||
      (bias_dw && overlaps(y, ny, bias_dw, cin)) || (adw && (overlaps(y, ny, alpha_dw, cin) || overlaps(y, ny, beta_dw, cin))) ||
      (bias && overlaps(y, ny, bias, cout)) || (apw && (overlaps(y, ny, alpha, cout) || overlaps(y, ny, beta, cout))) ||
      (residual && overlaps(y, ny, residual, ny)))
    return set_error(MV_ERR_INVALID_ARGUMENT, "output must not overlap an input, weight, epilogue term or residual");
  const Epilogue e_dw = {bias_dw, adw ? alpha_dw : nullptr, adw ? beta_dw : nullptr, nullptr, affine_dw, act_dw};
  const Epilogue e = {bias, apw ? alpha : nullptr, apw ? beta : nullptr, residual, affine, act};
  return launch_dwconv3x3_conv1x1(x, w_dw, e_dw, w, y, n, cin, h, wdt, cout, stride, e, (hipStream_t)stream);
}

// ---- ConvNeXt: depthwise 7x7 + bias, LayerNorm over the channels, the pointwise conv with the norm in its loads and GELU in its
//      epilogue (dw7x7.hip, layernorm.hip, convnorm.hip k_conv1x1_ln) ------------------------------------------------------------------
int mv_dwconv7x7_bias_f32(const float* x, const float* w, const float* bias, float* y, int64_t n, int c, int h, int wdt, void* stream) {
  if (n < 0 || c < 0 || h < 0 || wdt < 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "dwconv7x7: negative size (n=%lld c=%d h=%d w=%d)", (long long)n, c, h, wdt);
  const long long hw = (long long)h * wdt;
  if (hw > 0x7fffffffLL) return set_error(MV_ERR_UNSUPPORTED, "dwconv7x7: a plane of %d x %d elements exceeds the 32-bit index", h, wdt);
  if (n == 0 || c == 0 || hw == 0) return MV_OK;
  if (n * c > (1LL << 40) / hw) return set_error(MV_ERR_UNSUPPORTED, "dwconv7x7: %lld planes of %lld elements exceed the launch grid", (long long)(n * c), hw);
  if (!x || !w || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "dwconv7x7: null pointer");
  if ((uintptr_t)x % 4 || (uintptr_t)y % 4 || (uintptr_t)w % 4 || (uintptr_t)bias % 4)
    return set_error(MV_ERR_INVALID_ARGUMENT, "dwconv7x7: x, w, bias and y must be 4-byte aligned");
  const long long ny = n * c * hw;
  if (overlaps(y, ny, x, ny) || overlaps(y, ny, w, 49LL * c) || (bias && overlaps(y, ny, bias, c)))
    return set_error(MV_ERR_INVALID_ARGUMENT, "dwconv7x7: y must not overlap x, w or bias");
  return launch_dwpc7x7(x, w, bias, y, n, c, h, wdt, (hipStream_t)stream);
}

// apply: mv_layer_norm2d_f32 (y); otherwise mv_layer_norm2d_stats_f32 (mean / rstd)
static int layer_norm2d(const char* op, bool apply, const float* x, const float* weight, const float* bias, float* y, float* mean, float* rstd, int64_t n,
                        int c, int h, int w, double eps, void* stream) {
  if (n < 0 || c < 0 || h < 0 || w < 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: negative size (n=%lld c=%d h=%d w=%d)", op, (long long)n, c, h, w);
  if (!(eps >= 0) || eps > 3.0e38) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: eps must be non-negative and finite in float32, got %g", op, eps);
  const int64_t hw = (int64_t)h * w, image = (int64_t)c * hw;
  if (hw > 0x7fffffffLL || image > 0x7fffffffLL)
    return set_error(MV_ERR_UNSUPPORTED, "%s: an image of %d x %d x %d elements exceeds the 32-bit index", op, c, h, w);
  if (n == 0 || hw == 0) return MV_OK;
  if (c == 0) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: no channels to normalise over", op);
  const int64_t blocks = n * layer_norm_blocks(hw);
  if (n > 0x7fffffffLL || blocks > 0x7fffffffLL) return set_error(MV_ERR_UNSUPPORTED, "%s: %lld workgroups exceed the launch grid", op, (long long)blocks);
  if (!x || (apply ? !y : (!mean || !rstd))) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: null pointer", op);
  if ((uintptr_t)x % 4 || (uintptr_t)y % 4 || (uintptr_t)weight % 4 || (uintptr_t)bias % 4 || (uintptr_t)mean % 4 || (uintptr_t)rstd % 4)
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: every pointer must be 4-byte aligned", op);
  const long long nx = n * image, ns = n * hw;
  if (apply) {
    if (overlaps(y, nx, x, nx) || (weight && overlaps(y, nx, weight, c)) || (bias && overlaps(y, nx, bias, c)))
      return set_error(MV_ERR_INVALID_ARGUMENT, "%s: y must not overlap x, weight or bias", op);
  } else if (overlaps(mean, ns, x, nx) || overlaps(rstd, ns, x, nx) || overlaps(mean, ns, rstd, ns)) {
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: mean and rstd must not overlap x or each other", op);
  }
  return launch_layer_norm2d(x, weight, bias, y, mean, rstd, n, c, hw, (float)eps, (hipStream_t)stream);
}

int mv_layer_norm2d_stats_f32(const float* x, float* mean, float* rstd, int64_t n, int c, int h, int w, double eps, void* stream) {
  return layer_norm2d("layer_norm2d_stats", false, x, nullptr, nullptr, nullptr, mean, rstd, n, c, h, w, eps, stream);
}

int mv_layer_norm2d_f32(const float* x, const float* weight, const float* bias, float* y, int64_t n, int c, int h, int w, double eps,
                        void* stream) {
  return layer_norm2d("layer_norm2d", true, x, weight, bias, y, nullptr, nullptr, n, c, h, w, eps, stream);
}

int mv_conv1x1_ln_gelu_f32(const float* x, const float* mean, const float* rstd, const float* ln_w, const float* ln_b, const float* w,
                           const float* bias, float* y, int64_t n, int cin, int h, int wdt, int cout, int gelu, void* stream) {
  if (n < 0 || cin <= 0 || cout <= 0 || h < 0 || wdt < 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad conv shape n=%lld cin=%d cout=%d h=%d w=%d", (long long)n, cin, cout, h, wdt);
  if (gelu != 0 && gelu != 1) return set_error(MV_ERR_INVALID_ARGUMENT, "conv1x1_ln_gelu: gelu should be 0 or 1 instead of %d", gelu);
  if ((mean == nullptr) != (rstd == nullptr)) return set_error(MV_ERR_INVALID_ARGUMENT, "conv1x1_ln_gelu: mean and rstd come together");
  if (!mean && (ln_w || ln_b)) return set_error(MV_ERR_INVALID_ARGUMENT, "conv1x1_ln_gelu: LayerNorm terms without mean and rstd");
  if (n == 0 || h == 0 || wdt == 0) return MV_OK;
  if (!x || !w || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if ((uintptr_t)x % 4 || (uintptr_t)y % 4 || (uintptr_t)w % 4 || (uintptr_t)bias % 4 || (uintptr_t)mean % 4 || (uintptr_t)rstd % 4 ||
      (uintptr_t)ln_w % 4 || (uintptr_t)ln_b % 4)
    return set_error(MV_ERR_INVALID_ARGUMENT, "conv1x1_ln_gelu: every pointer must be 4-byte aligned");
  const long long hw = (long long)h * wdt, ny = n * cout * hw, ns = n * hw;
  if (overlaps(y, ny, x, n * cin * hw) || overlaps(y, ny, w, (long long)cout * cin) || (bias && overlaps(y, ny, bias, cout)) ||
      (mean && (overlaps(y, ny, mean, ns) || overlaps(y, ny, rstd, ns))) || (ln_w && overlaps(y, ny, ln_w, cin)) ||
      (ln_b && overlaps(y, ny, ln_b, cin)))
    return set_error(MV_ERR_INVALID_ARGUMENT, "output must not overlap input, statistics, LayerNorm terms, weight or bias");
  return launch_conv1x1_ln_gelu(x, mean, rstd, ln_w, ln_b, w, bias, y, n, cin, hw, cout, gelu, (hipStream_t)stream);
}

int mv_global_avgpool_f64sum_f32(const float* x, float* y, int64_t n, int c, int h, int wdt, int64_t x_stride, void* stream) {
  if (n < 0 || c <= 0 || h <= 0 || wdt <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "global_avgpool: bad shape n=%lld c=%d h=%d w=%d", (long long)n, c, h, wdt);
  const long long hw = (long long)h * wdt;
  if (hw > 0x7fffffffLL || c * hw > 0x7fffffffLL)
    return set_error(MV_ERR_UNSUPPORTED, "global_avgpool: an image of %d x %d x %d elements exceeds the 32-bit index", c, h, wdt);
  if (x_stride < c * hw)
    return set_error(MV_ERR_INVALID_ARGUMENT, "global_avgpool: image stride %lld, an image has %lld elements", (long long)x_stride, c * hw);
  if (n == 0) return MV_OK;
  if (n * c > 4LL * 0x7fffffffLL) return set_error(MV_ERR_UNSUPPORTED, "global_avgpool: %lld planes exceed the launch grid", (long long)(n * c));
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "global_avgpool: null pointer");
  if ((uintptr_t)x % 4 || (uintptr_t)y % 4) return set_error(MV_ERR_INVALID_ARGUMENT, "global_avgpool: x and y must be 4-byte aligned");
  if (overlaps(y, n * c, x, (n - 1) * x_stride + c * hw)) return set_error(MV_ERR_INVALID_ARGUMENT, "global_avgpool: y must not overlap x");
  return launch_global_avgpool(x, y, n, c, (int)hw, x_stride, (hipStream_t)stream);
}

int mv_linear_act_f32(const float* x, const float* w, const float* b, float* y, int64_t n, int k, int m, int act, void* stream) {
  if (n < 0 || k <= 0 || m <= 0) return set_error(MV_ERR_INVALID_ARGUMENT, "bad linear shape n=%lld k=%d m=%d", (long long)n, k, m);
  if (act != MV_ACT_NONE && act != MV_ACT_RELU && act != MV_ACT_HARDSWISH && act != MV_ACT_HARDSIGMOID && act != MV_ACT_SIGMOID)
    return set_error(MV_ERR_INVALID_ARGUMENT, "linear_act: activation code %d (none, ReLU, Hardswish, Hardsigmoid, Sigmoid)", act);
  if (n == 0) return MV_OK;
  if (n > 65535) return set_error(MV_ERR_UNSUPPORTED, "linear_act: n = %lld rows exceed the launch grid (65535)", (long long)n);
  if (!x || !w || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  const long long ny = n * m;
  if (overlaps(y, ny, x, n * k) || overlaps(y, ny, w, (long long)m * k) || (b && overlaps(y, ny, b, m)))
    return set_error(MV_ERR_INVALID_ARGUMENT, "linear_act: y must not overlap x, w or b");
  return launch_linear_act(x, w, b, y, n, k, m, act, (hipStream_t)stream);
}

int mv_se_scale_f32(const float* x, const float* gate, float* y, int64_t n, int c, int h, int wdt, void* stream) {
  if (n < 0 || c <= 0 || h <= 0 || wdt <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "se_scale: bad shape n=%lld c=%d h=%d w=%d", (long long)n, c, h, wdt);
  const long long hw = (long long)h * wdt;
  if (hw > 0x7fffffffLL) return set_error(MV_ERR_UNSUPPORTED, "se_scale: a plane of %d x %d elements exceeds the 32-bit index", h, wdt);
  if (n == 0) return MV_OK;
  const long long planes = n * c;
  if (planes > (1LL << 40) / hw) return set_error(MV_ERR_UNSUPPORTED, "se_scale: %lld planes of %lld elements exceed the launch grid", planes, hw);
  if (!x || !gate || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "se_scale: null pointer");
  if ((uintptr_t)x % 4 || (uintptr_t)y % 4 || (uintptr_t)gate % 4) return set_error(MV_ERR_INVALID_ARGUMENT, "se_scale: x, gate and y must be 4-byte aligned");
  if (x != y && overlaps(y, planes * hw, x, planes * hw))
    return set_error(MV_ERR_INVALID_ARGUMENT, "se_scale: y must be x itself (in place) or must not overlap it");
  if (overlaps(y, planes * hw, gate, planes)) return set_error(MV_ERR_INVALID_ARGUMENT, "se_scale: y must not overlap gate");
  return launch_se_scale(x, gate, y, planes, (int)hw, (hipStream_t)stream);
}

int mv_inverted_residual_k_slices(int64_t n, int cin, int hidden, int cout, int h, int wdt, int stride, int* slice_len) {
  int slices = 0, len = hidden;
  if (!invres_plan(n, cin, hidden, cout, h, wdt, stride, &slices, &len)) slices = 0, len = hidden;
  if (slice_len) *slice_len = len;
  return slices;
}

int64_t mv_inverted_residual_workspace_bytes(int64_t n, int cin, int hidden, int cout, int h, int wdt, int stride) {
  return invres_workspace_bytes(n, cin, hidden, cout, h, wdt, stride);
}

int mv_inverted_residual_f32(const float* x, const float* w_expand, const float* a1, const float* b1, const float* w_dw,
                             const float* a2, const float* b2, const float* w_project, const float* a3, const float* b3,
                             int residual, float* y, int64_t n, int cin, int hidden, int cout, int h, int wdt, int stride,
                             int affine, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n < 0 || cin <= 0 || hidden <= 0 || cout <= 0 || h <= 0 || wdt <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad inverted_residual shape n=%lld %d -> %d -> %d on %d x %d", (long long)n, cin, hidden, cout, h, wdt);
  if (stride != 1 && stride != 2) return set_error(MV_ERR_INVALID_ARGUMENT, "stride should be 1 or 2 instead of %d", stride);
  if (affine != MV_AFFINE_MUL_ADD && affine != MV_AFFINE_FMA)
    return set_error(MV_ERR_INVALID_ARGUMENT, "inverted_residual: affine must be MV_AFFINE_MUL_ADD or MV_AFFINE_FMA (every conv of the block is followed by a norm)");
  if (n == 0) return MV_OK;
  // a block without expansion (expand_ratio 1: hidden == cin) has no w_expand / a1 / b1
  if (!x || !w_dw || !a2 || !b2 || !w_project || !a3 || !b3 || !y || (hidden != cin && (!w_expand || !a1 || !b1))) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  return launch_invres(x, w_expand, a1, b1, w_dw, a2, b2, w_project, a3, b3, residual, y, n, cin, hidden, cout, h, wdt, stride, affine,
                       workspace, workspace_bytes, (hipStream_t)stream);
}

void mv_fold_batchnorm(const float* weight, const float* bias, const float* mean, const float* var, double eps, int c,
                       float* alpha, float* beta) {
  for (int i = 0; i < c; ++i) {
    const float invstd = 1.0f / sqrtf(var[i] + (float)eps);
    const float a = invstd * (weight ? weight[i] : 1.0f);
    alpha[i] = a;
    beta[i] = fmaf(-mean[i], a, bias ? bias[i] : 0.0f);
  }
}

// Validates a convolution's kernel, stride, padding and dilation on its image (the reference's checks and messages,
// deform_conv2d_kernel.cpp:1004-1045, for the ordinary convolutions as well) and sets g->oh / g->ow
static int conv2d_geometry(Conv2dGeom* g) {
  if (g->h <= 0 || g->w <= 0 || g->kh <= 0 || g->kw <= 0) return set_error(MV_ERR_INVALID_ARGUMENT, "bad deform_conv2d shape (%d, %d) kernel (%d, %d)", g->h, g->w, g->kh, g->kw);
  if (g->sh <= 0 || g->sw <= 0) return set_error(MV_ERR_INVALID_ARGUMENT, "stride_h: %d stride_w: %d", g->sh, g->sw);  // :1004-1006
  if (g->ph < 0 || g->pw < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "pad_h: %d pad_w: %d", g->ph, g->pw);
  if (g->dh <= 0 || g->dw <= 0) return set_error(MV_ERR_INVALID_ARGUMENT, "dil_h: %d dil_w: %d", g->dh, g->dw);
  g->oh = (g->h + 2 * g->ph - (g->dh * (g->kh - 1) + 1)) / g->sh + 1;
  g->ow = (g->w + 2 * g->pw - (g->dw * (g->kw - 1) + 1)) / g->sw + 1;
  if (g->oh <= 0 || g->ow <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "Calculated output size too small - out_h: %d out_w: %d", g->oh, g->ow);  // :1040-1045
  return MV_OK;
}

static bool channels_divide(const Conv2dGeom& g, int offset_groups) {
  return g.cin > 0 && g.cout > 0 && g.groups > 0 && offset_groups > 0 && g.cin % g.groups == 0 && g.cout % g.groups == 0 && g.cin % offset_groups == 0;
}

// What the three convolution entries check first, in the order they report it: batch and channel counts, geometry, groups.
// offset_groups == nullptr: an ordinary convolution
static int check_conv2d(int64_t n, Conv2dGeom* g, const int* offset_groups) {
  if (n < 0 || g->cin <= 0 || g->cout <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad %s shape n=%lld cin=%d cout=%d", offset_groups ? "deform_conv2d" : "conv2d", (long long)n, g->cin, g->cout);
  if (int rc = conv2d_geometry(g)) return rc;
  if (channels_divide(*g, offset_groups ? *offset_groups : 1)) return MV_OK;
  if (offset_groups)
    return set_error(MV_ERR_INVALID_ARGUMENT, "channels (%d -> %d) must divide into %d weight groups and %d offset groups", g->cin, g->cout,
                     g->groups, *offset_groups);
  return set_error(MV_ERR_INVALID_ARGUMENT, "channels (%d -> %d) must divide into %d groups", g->cin, g->cout, g->groups);
}

int64_t mv_deform_conv2d_workspace_bytes(int64_t images, int cin, int h, int wdt, int kh, int kw, int stride_h, int stride_w,
                                         int pad_h, int pad_w, int dilation_h, int dilation_w) {
  Conv2dGeom g = {cin, h, wdt, /*cout=*/0, kh, kw, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, /*groups=*/1};
  if (images <= 0 || cin <= 0 || conv2d_geometry(&g)) return 0;
  return images * columns_bytes_per_image(g);
}

int mv_deform_conv2d_needs_workspace(int64_t images, int cin, int cout, int h, int wdt, int kh, int kw, int stride_h, int stride_w,
                                     int pad_h, int pad_w, int dilation_h, int dilation_w, int groups, int offset_groups) {
  Conv2dGeom g = {cin, h, wdt, cout, kh, kw, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, groups};
  if (images <= 0 || !channels_divide(g, offset_groups) || conv2d_geometry(&g)) return kFormColumns;
  return deform_conv2d_form(images, g, offset_groups);
}

int mv_deform_conv2d_f32(const float* x, const float* weight, const float* offset, const float* mask, const float* bias, float* y,
                         int64_t n, int cin, int h, int wdt, int cout, int kh, int kw, int stride_h, int stride_w, int pad_h,
                         int pad_w, int dilation_h, int dilation_w, int groups, int offset_groups, int use_mask, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  Conv2dGeom g = {cin, h, wdt, cout, kh, kw, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, groups};
  if (int rc = check_conv2d(n, &g, &offset_groups)) return rc;
  if (n == 0) return MV_OK;
  if (!x || !weight || !offset || !y || (use_mask && !mask)) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  return launch_deform_conv2d(x, weight, offset, use_mask ? mask : nullptr, bias, y, n, g, offset_groups, workspace, workspace_bytes,
                              (hipStream_t)stream);
}

int mv_conv2d_needs_workspace(int64_t n, int cin, int cout, int h, int wdt, int kh, int kw, int stride_h, int stride_w, int pad_h,
                              int pad_w, int dilation_h, int dilation_w, int groups) {
  Conv2dGeom g = {cin, h, wdt, cout, kh, kw, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, groups};
  if (!channels_divide(g, 1) || conv2d_geometry(&g)) return kFormColumns;
  return conv2d_form(n, g);
}

// the rest of the two ordinary entries' checks; check_overlap: mv_conv2d_affine_act_f32 only (host dispatch: a known gap)
static int launch_checked_conv2d(const float* x, const float* weight, float* y, int64_t n, const Conv2dGeom& g, const Epilogue& e,
                                 bool check_overlap, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n == 0) return MV_OK;
  if (!x || !weight || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (e.affine != MV_AFFINE_NONE && (!e.alpha || !e.beta)) return set_error(MV_ERR_INVALID_ARGUMENT, "affine without alpha / beta");
  const long long ny = (long long)n * g.cout * g.oh * g.ow;
  if (check_overlap && (overlaps(y, ny, x, (long long)n * g.cin * g.h * g.w) ||
                        overlaps(y, ny, weight, (long long)g.cout * (g.cin / g.groups) * g.kh * g.kw) || (e.res && overlaps(y, ny, e.res, ny))))
    return set_error(MV_ERR_INVALID_ARGUMENT, "output must not overlap input, weight or residual");
  return launch_conv2d(x, weight, y, n, g, e, workspace, workspace_bytes, (hipStream_t)stream);
}

int mv_conv2d_bias_act_f32(const float* x, const float* weight, const float* bias, float* y, int64_t n, int cin, int h, int wdt,
                           int cout, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h,
                           int dilation_w, int groups, int act, void* workspace, int64_t workspace_bytes, void* stream) {
  Conv2dGeom g = {cin, h, wdt, cout, kh, kw, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, groups};
  if (int rc = check_conv2d(n, &g, nullptr)) return rc;
  if (act < MV_ACT_NONE || act > MV_ACT_SILU) return set_error(MV_ERR_INVALID_ARGUMENT, "bad activation code %d", act);
  return launch_checked_conv2d(x, weight, y, n, g, {bias, nullptr, nullptr, nullptr, MV_AFFINE_NONE, act}, false, workspace,
                               workspace_bytes, stream);
}

int mv_conv2d_affine_act_f32(const float* x, const float* weight, const float* bias, const float* alpha, const float* beta,
                             const float* residual, float* y, int64_t n, int cin, int h, int wdt, int cout, int kh, int kw,
                             int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w, int groups,
                             int affine, int act, void* workspace, int64_t workspace_bytes, void* stream) {
  Conv2dGeom g = {cin, h, wdt, cout, kh, kw, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, groups};
  if (int rc = check_conv2d(n, &g, nullptr)) return rc;
  if (affine < MV_AFFINE_NONE || affine > MV_AFFINE_FMA || act < MV_ACT_NONE || act > MV_ACT_SILU)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad affine (%d) / activation (%d) code", affine, act);
  return launch_checked_conv2d(x, weight, y, n, g, {bias, affine ? alpha : nullptr, affine ? beta : nullptr, residual, affine, act}, true,
                               workspace, workspace_bytes, stream);
}

int mv_maxpool2d_pad_f32(const float* x, float* y, int64_t planes, int h, int wdt, int k, int stride, int pad, void* stream) {
  if (planes < 0 || h <= 0 || wdt <= 0 || k <= 0 || stride <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad pooling shape planes=%lld (%d, %d) k=%d stride=%d", (long long)planes, h, wdt, k, stride);
  if (pad < 0 || pad > k / 2) return set_error(MV_ERR_INVALID_ARGUMENT, "pad should be at most half of effective kernel size, but got pad=%d, kernel_size=%d", pad, k);
  if ((long long)h + 2 * pad < k || (long long)wdt + 2 * pad < k)
    return set_error(MV_ERR_INVALID_ARGUMENT, "Output size is too small: (%d, %d) with k=%d pad=%d", h, wdt, k, pad);
  if (planes == 0) return MV_OK;
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  return launch_maxpool2d_pad(x, y, planes, h, wdt, k, stride, pad, (hipStream_t)stream);
}

int mv_maxpool2d_ceil_f32(const float* x, float* y, int64_t planes, int h, int wdt, int k, int stride, int pad, void* stream) {
  if (planes < 0 || h <= 0 || wdt <= 0 || k <= 0 || stride <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad pooling shape planes=%lld (%d, %d) k=%d stride=%d", (long long)planes, h, wdt, k, stride);
  if (pad < 0 || pad > k / 2) return set_error(MV_ERR_INVALID_ARGUMENT, "pad should be at most half of effective kernel size, but got pad=%d, kernel_size=%d", pad, k);
  if ((long long)h + 2 * pad < k || (long long)wdt + 2 * pad < k)
    return set_error(MV_ERR_INVALID_ARGUMENT, "Output size is too small: (%d, %d) with k=%d pad=%d", h, wdt, k, pad);
  if (planes == 0) return MV_OK;
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  return launch_maxpool2d_ceil(x, y, planes, h, wdt, k, stride, pad, (hipStream_t)stream);
}

int mv_maxpool2d_f32(const float* x, float* y, int64_t planes, int h, int wdt, int k, int stride, void* stream) {
  if (planes < 0 || h <= 0 || wdt <= 0 || k <= 0 || stride <= 0 || k > h || k > wdt)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad pooling shape planes=%lld (%d, %d) k=%d stride=%d", (long long)planes, h, wdt, k, stride);
  if (planes == 0) return MV_OK;
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  return launch_maxpool2d(x, y, planes, h, wdt, k, stride, (hipStream_t)stream);
}

static int check_resize(const void* x, const void* y, int64_t planes, int h, int wdt, int oh, int ow, int ch, int cw) {
  if (planes < 0 || h <= 0 || wdt <= 0 || oh <= 0 || ow <= 0 || ch <= 0 || cw <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "bad resize shape planes=%lld (%d, %d) -> (%d, %d), window (%d, %d)",
                     (long long)planes, h, wdt, oh, ow, ch, cw);
  if (planes > 0 && (!x || !y)) return set_error(MV_ERR_INVALID_ARGUMENT, "null pointer");
  if (x == y && planes > 0) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  return MV_OK;
}

int64_t mv_resize_workspace_bytes(int64_t planes, int h, int wdt, int oh, int ow, int crop_top, int crop_left, int crop_h,
                                  int crop_w) {
  if (planes <= 0 || h <= 0 || wdt <= 0 || oh <= 0 || ow <= 0 || crop_h <= 0 || crop_w <= 0) return 0;
  return resize_workspace_bytes(planes, h, wdt, oh, ow, crop_top, crop_left, crop_h, crop_w);
}

int mv_resize_bilinear_aa_u8(const uint8_t* x, uint8_t* y, int64_t planes, int h, int wdt, int oh, int ow, int crop_top,
                             int crop_left, int crop_h, int crop_w, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_resize(x, y, planes, h, wdt, oh, ow, crop_h, crop_w)) return rc;
  if (planes == 0) return MV_OK;
  return launch_resize(x, y, true, planes, 1, h, wdt, oh, ow, crop_top, crop_left, crop_h, crop_w, 0, nullptr, nullptr,
                       workspace, workspace_bytes, (hipStream_t)stream);
}

int mv_resize_bilinear_aa_f32(const float* x, float* y, int64_t planes, int h, int wdt, int oh, int ow, int crop_top,
                              int crop_left, int crop_h, int crop_w, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_resize(x, y, planes, h, wdt, oh, ow, crop_h, crop_w)) return rc;
  if (planes == 0) return MV_OK;
  return launch_resize(x, y, false, planes, 1, h, wdt, oh, ow, crop_top, crop_left, crop_h, crop_w, 0, nullptr, nullptr,
                       workspace, workspace_bytes, (hipStream_t)stream);
}

static int preset(const void* x, float* y, bool u8, int64_t n, int c, int h, int wdt, int oh, int ow, int ct, int cl, int ch,
                  int cw, const float* mean, const float* stdv, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n < 0 || c <= 0 || c > 4) return set_error(MV_ERR_INVALID_ARGUMENT, "preset: n=%lld, c=%d (1..4 channels)", (long long)n, c);
  if (int rc = check_resize(x, y, n * c, h, wdt, oh, ow, ch, cw)) return rc;
  if (n == 0) return MV_OK;
  if (!mean || !stdv) return set_error(MV_ERR_INVALID_ARGUMENT, "preset: null mean / std");
  for (int i = 0; i < c; ++i)
    if (stdv[i] == 0.f) return set_error(MV_ERR_INVALID_ARGUMENT, "std evaluated to zero, leading to division by zero.");
  return launch_resize(x, y, u8, n * c, c, h, wdt, oh, ow, ct, cl, ch, cw, 1, mean, stdv, workspace, workspace_bytes,
                       (hipStream_t)stream);
}

int mv_preset_classification_u8(const uint8_t* x, float* y, int64_t n, int c, int h, int wdt, int oh, int ow, int crop_top,
                                int crop_left, int crop_h, int crop_w, const float* mean, const float* stdv,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  return preset(x, y, true, n, c, h, wdt, oh, ow, crop_top, crop_left, crop_h, crop_w, mean, stdv, workspace,
                workspace_bytes, stream);
}

int mv_preset_classification_f32(const float* x, float* y, int64_t n, int c, int h, int wdt, int oh, int ow, int crop_top,
                                 int crop_left, int crop_h, int crop_w, const float* mean, const float* stdv,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  return preset(x, y, false, n, c, h, wdt, oh, ow, crop_top, crop_left, crop_h, crop_w, mean, stdv, workspace,
                workspace_bytes, stream);
}

// F.resized_crop: the window's size takes the place of the input size; the window itself and the flips ride in ResizeWindow
static int resized_crop(const void* x, void* y, bool u8, int64_t planes, int channels, int h, int wdt, int top, int left, int wh,
                        int ww, int oh, int ow, int flip_h, int flip_v, int preset, const float* mean, const float* stdv,
                        void* workspace, int64_t workspace_bytes, void* stream) {
  if (h <= 0 || wdt <= 0) return set_error(MV_ERR_INVALID_ARGUMENT, "resized_crop: bad image size (%d, %d)", h, wdt);
  if (int rc = check_resize(x, y, planes, wh, ww, oh, ow, oh, ow)) return rc;
  // the window's corner plus its size must stay an int
  if (top < -0x3fffffff || top > 0x3fffffff || left < -0x3fffffff || left > 0x3fffffff || wh > 0x3fffffff || ww > 0x3fffffff)
    return set_error(MV_ERR_INVALID_ARGUMENT, "resized_crop: window (%d, %d, %d, %d) out of range", top, left, wh, ww);
  if (planes == 0) return MV_OK;
  if (preset) {
    if (!mean || !stdv) return set_error(MV_ERR_INVALID_ARGUMENT, "preset: null mean / std");
    for (int i = 0; i < channels; ++i)
      if (stdv[i] == 0.f) return set_error(MV_ERR_INVALID_ARGUMENT, "std evaluated to zero, leading to division by zero.");
  }
  const ResizeWindow win = {top, left, h, wdt, flip_h ? 1 : 0, flip_v ? 1 : 0};
  return launch_resize(x, y, u8, planes, channels, wh, ww, oh, ow, 0, 0, oh, ow, preset, mean, stdv, workspace, workspace_bytes,
                       (hipStream_t)stream, &win);
}

int mv_resized_crop_u8(const uint8_t* x, uint8_t* y, int64_t planes, int h, int wdt, int top, int left, int wh, int ww, int oh,
                       int ow, int flip_h, int flip_v, void* workspace, int64_t workspace_bytes, void* stream) {
  return resized_crop(x, y, true, planes, 1, h, wdt, top, left, wh, ww, oh, ow, flip_h, flip_v, 0, nullptr, nullptr, workspace,
                      workspace_bytes, stream);
}

int mv_resized_crop_f32(const float* x, float* y, int64_t planes, int h, int wdt, int top, int left, int wh, int ww, int oh,
                        int ow, int flip_h, int flip_v, void* workspace, int64_t workspace_bytes, void* stream) {
  return resized_crop(x, y, false, planes, 1, h, wdt, top, left, wh, ww, oh, ow, flip_h, flip_v, 0, nullptr, nullptr, workspace,
                      workspace_bytes, stream);
}

int mv_resized_crop_preset_u8(const uint8_t* x, float* y, int64_t n, int c, int h, int wdt, int top, int left, int wh, int ww,
                              int oh, int ow, int flip_h, int flip_v, int v2_scale, const float* mean, const float* stdv,
                              void* workspace, int64_t workspace_bytes, void* stream) {
  if (n < 0 || c <= 0 || c > 4) return set_error(MV_ERR_INVALID_ARGUMENT, "preset: n=%lld, c=%d (1..4 channels)", (long long)n, c);
  return resized_crop(x, y, true, n * c, c, h, wdt, top, left, wh, ww, oh, ow, flip_h, flip_v, v2_scale ? 2 : 1, mean, stdv, workspace,
                      workspace_bytes, stream);
}

int mv_resized_crop_preset_f32(const float* x, float* y, int64_t n, int c, int h, int wdt, int top, int left, int wh, int ww,
                               int oh, int ow, int flip_h, int flip_v, int v2_scale, const float* mean, const float* stdv,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  if (n < 0 || c <= 0 || c > 4) return set_error(MV_ERR_INVALID_ARGUMENT, "preset: n=%lld, c=%d (1..4 channels)", (long long)n, c);
  return resized_crop(x, y, false, n * c, c, h, wdt, top, left, wh, ww, oh, ow, flip_h, flip_v, 1, mean, stdv, workspace,
                      workspace_bytes, stream);
}

// ---- pad / crop / flip / erase: the gather kernel of crop.hip -------------------------------------------------------------------
static int check_elem_bytes(const char* what, int elem_bytes) {
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: elem_bytes must be 1, 2, 4 or 8, got %d", what, elem_bytes);
  return MV_OK;
}

int mv_pad_crop_flip(const void* x, void* y, int64_t planes, int channels, int elem_bytes, int ih, int iw, int oh, int ow, int top,
                     int left, int mode, int flip_h, int flip_v, const void* fill, void* stream) {
  if (int rc = check_elem_bytes("pad_crop_flip", elem_bytes)) return rc;
  if (planes < 0 || ih < 0 || iw < 0 || oh < 0 || ow < 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "pad_crop_flip: bad shape planes=%lld (%d, %d) -> (%d, %d)", (long long)planes, ih, iw,
                     oh, ow);
  if (mode < MV_PAD_CONSTANT || mode > MV_PAD_SYMMETRIC)
    return set_error(MV_ERR_INVALID_ARGUMENT, "pad_crop_flip: unknown padding mode %d (0 constant, 1 edge, 2 reflect, 3 symmetric)", mode);
  if (channels < 1 || channels > 4)
    return set_error(MV_ERR_INVALID_ARGUMENT, "pad_crop_flip: a fill has 1 to 4 channels, got %d", channels);
  if (planes % channels != 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "pad_crop_flip: planes (%lld) must be a multiple of channels (%d)", (long long)planes, channels);
  if (top < -0x3fffffff || top > 0x3fffffff || left < -0x3fffffff || left > 0x3fffffff || ih > 0x3fffffff || iw > 0x3fffffff ||
      oh > 0x3fffffff || ow > 0x3fffffff)
    return set_error(MV_ERR_INVALID_ARGUMENT, "pad_crop_flip: offsets (%d, %d) out of range", top, left);
  if (planes == 0 || oh == 0 || ow == 0) return MV_OK;
  if (mode != MV_PAD_CONSTANT && (ih == 0 || iw == 0))
    return set_error(MV_ERR_INVALID_ARGUMENT, "pad_crop_flip: an empty image has no border to repeat");
  if (ih > 0 && iw > 0 && (!gather_axis_ok(ih, oh, top, mode) || !gather_axis_ok(iw, ow, left, mode))) {
    if (mode == MV_PAD_REFLECT)
      return set_error(MV_ERR_INVALID_ARGUMENT, "pad_crop_flip: reflect padding (%d, %d, %d, %d) must be smaller than the image side (%d, %d)",
                       -left, ow - iw + left, -top, oh - ih + top, ih, iw);
    return set_error(MV_ERR_INVALID_ARGUMENT, "pad_crop_flip: symmetric padding (%d, %d, %d, %d) exceeds the image side (%d, %d)",
                     -left, ow - iw + left, -top, oh - ih + top, ih, iw);
  }
  if (!y || (!x && ih > 0 && iw > 0)) return set_error(MV_ERR_INVALID_ARGUMENT, "pad_crop_flip: null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  if (!gather_grid_fits(planes, oh, ow, elem_bytes))
    return set_error(MV_ERR_UNSUPPORTED, "pad_crop_flip: %lld planes of %d x %d exceed the launch grid", (long long)planes, oh, ow);
  unsigned long long bits[4] = {0, 0, 0, 0};
  if (fill)
    for (int c = 0; c < channels; ++c) __builtin_memcpy(&bits[c], static_cast<const char*>(fill) + (size_t)c * elem_bytes, elem_bytes);
  if (ih == 0 || iw == 0) ih = iw = 1, top = left = 0x3fffffff;  // constant mode on an empty image: every pixel is fill
  return launch_gather(x, y, planes, channels, elem_bytes, ih, iw, oh, ow, top, left, mode, flip_h ? 1 : 0, flip_v ? 1 : 0, bits,
                       nullptr, 0, 0, 0, 0, 0, (hipStream_t)stream);
}

int mv_erase(const void* x, void* y, int64_t planes, int channels, int elem_bytes, int h, int w, int i, int j, int eh, int ew,
             const void* v, int v_is_per_pixel, void* stream) {
  if (int rc = check_elem_bytes("erase", elem_bytes)) return rc;
  if (planes < 0 || h < 0 || w < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "erase: bad shape planes=%lld (%d, %d)", (long long)planes, h, w);
  if (channels < 1 || planes % channels != 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "erase: planes (%lld) must be a multiple of channels (%d)", (long long)planes, channels);
  if (eh < 0 || ew < 0 || i < 0 || j < 0 || i > h - eh || j > w - ew)
    return set_error(MV_ERR_INVALID_ARGUMENT, "erase: the box (%d, %d, %d, %d) must lie inside the (%d, %d) image", i, j, eh, ew, h, w);
  if (planes == 0 || h == 0 || w == 0) return MV_OK;
  if (!x || !y || (!v && eh > 0 && ew > 0)) return set_error(MV_ERR_INVALID_ARGUMENT, "erase: null pointer");
  if (eh == 0 || ew == 0) eh = ew = 0;
  if (x == y) {
    if (planes * (long long)eh * ew > 256LL * 0x7fffffffLL) return set_error(MV_ERR_UNSUPPORTED, "erase: box too large for one launch");
    return launch_erase_box(y, planes, channels, elem_bytes, h, w, i, j, eh, ew, v, v_is_per_pixel ? 1 : 0, (hipStream_t)stream);
  }
  if (!gather_grid_fits(planes, h, w, elem_bytes))
    return set_error(MV_ERR_UNSUPPORTED, "erase: %lld planes of %d x %d exceed the launch grid", (long long)planes, h, w);
  return launch_gather(x, y, planes, channels, elem_bytes, h, w, h, w, 0, 0, MV_PAD_CONSTANT, 0, 0, nullptr, v, i, j, eh, ew,
                       v_is_per_pixel ? 1 : 0, (hipStream_t)stream);
}

// ---- MixUp / CutMix: batchmix.hip ------------------------------------------------------------------------------------------------
static int mixup(const void* x, void* y, int elem_bytes, int64_t batch, int64_t sample_elems, double lam, void* stream) {
  if (batch < 0 || sample_elems < 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "mixup: bad shape batch=%lld, sample_elems=%lld", (long long)batch, (long long)sample_elems);
  if (lam != lam) return set_error(MV_ERR_INVALID_ARGUMENT, "mixup: lam is NaN");
  if (batch == 0 || sample_elems == 0) return MV_OK;
  if (sample_elems > 0x7fffffffffffLL / batch)
    return set_error(MV_ERR_UNSUPPORTED, "mixup: %lld samples of %lld elements are too many", (long long)batch, (long long)sample_elems);
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "mixup: null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  if (!mix_grid_fits(batch, sample_elems, elem_bytes))
    return set_error(MV_ERR_UNSUPPORTED, "mixup: %lld samples of %lld elements exceed the launch grid", (long long)batch,
                     (long long)sample_elems);
  return launch_mixup(x, y, elem_bytes, batch, sample_elems, lam, (hipStream_t)stream);
}

int mv_mixup_f32(const float* x, float* y, int64_t batch, int64_t sample_elems, double lam, void* stream) {
  return mixup(x, y, 4, batch, sample_elems, lam, stream);
}

int mv_mixup_f16(const void* x, void* y, int64_t batch, int64_t sample_elems, double lam, void* stream) {
  return mixup(x, y, 2, batch, sample_elems, lam, stream);
}

int mv_mixup_f64(const double* x, double* y, int64_t batch, int64_t sample_elems, double lam, void* stream) {
  return mixup(x, y, 8, batch, sample_elems, lam, stream);
}

int mv_cutmix(const void* x, void* y, int64_t batch, int64_t planes_per_sample, int elem_bytes, int h, int w, int x1, int y1, int x2,
              int y2, void* stream) {
  if (int rc = check_elem_bytes("cutmix", elem_bytes)) return rc;
  if (batch < 0 || planes_per_sample < 0 || h < 0 || w < 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "cutmix: bad shape batch=%lld, planes_per_sample=%lld (%d, %d)", (long long)batch,
                     (long long)planes_per_sample, h, w);
  if (x1 < 0 || y1 < 0 || x2 < x1 || y2 < y1 || x2 > w || y2 > h)
    return set_error(MV_ERR_INVALID_ARGUMENT, "cutmix: the box x [%d, %d) y [%d, %d) must lie inside the (%d, %d) image", x1, x2, y1, y2,
                     h, w);
  if (batch == 0 || planes_per_sample == 0 || h == 0 || w == 0) return MV_OK;
  if (planes_per_sample > 0x7fffffffffffLL / batch / h / w)
    return set_error(MV_ERR_UNSUPPORTED, "cutmix: %lld samples of %lld planes of %d x %d are too many", (long long)batch,
                     (long long)planes_per_sample, h, w);
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "cutmix: null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  const int64_t elems = planes_per_sample * h * w;
  if (!mix_grid_fits(batch, elems, elem_bytes))
    return set_error(MV_ERR_UNSUPPORTED, "cutmix: %lld samples of %lld elements exceed the launch grid", (long long)batch,
                     (long long)elems);
  return launch_cutmix(x, y, batch, elems, elem_bytes, h, w, x1, y1, x2, y2, (hipStream_t)stream);
}

int mv_mixup_labels_i64(const int64_t* labels, float* y, int64_t batch, int num_classes, double lam, void* stream) {
  if (batch < 0 || num_classes <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "mixup_labels: bad shape batch=%lld, num_classes=%d", (long long)batch, num_classes);
  if (lam != lam) return set_error(MV_ERR_INVALID_ARGUMENT, "mixup_labels: lam is NaN");
  if (batch == 0) return MV_OK;
  if (batch > (0x7fffffffLL * 1024) / num_classes)
    return set_error(MV_ERR_UNSUPPORTED, "mixup_labels: %lld x %d outputs exceed the launch grid", (long long)batch, num_classes);
  if (!labels || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "mixup_labels: null pointer");
  if ((const void*)labels == (const void*)y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  return launch_mixup_labels(labels, y, batch, num_classes, lam, (hipStream_t)stream);
}

// ---- nms / roi_align: detect.hip -----------------------------------------------------------------------------------------------
int64_t mv_nms_workspace_bytes(int64_t n) {
  if (n <= 0 || n > kNmsMaxBoxes) return 0;
  return nms_workspace_bytes(n);
}

int mv_nms_f32(const float* boxes, const float* scores, int64_t n, double iou_threshold, int64_t* keep_out, int64_t* keep_count_out,
               void* workspace, int64_t workspace_bytes, void* stream) {
  if (n < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "nms: bad box count %lld", (long long)n);
  if (n == 0) return MV_OK;
  if (n > kNmsMaxBoxes) return set_error(MV_ERR_UNSUPPORTED, "nms: up to %d boxes per call, got %lld", kNmsMaxBoxes, (long long)n);
  if (!boxes || !scores || !keep_out || !keep_count_out) return set_error(MV_ERR_INVALID_ARGUMENT, "nms: null pointer");
  if ((uintptr_t)keep_out % 8 || (uintptr_t)keep_count_out % 8)
    return set_error(MV_ERR_INVALID_ARGUMENT, "nms: keep_out and keep_count_out must be 8-byte aligned");
  if (!workspace) return set_error(MV_ERR_INVALID_ARGUMENT, "nms: needs a workspace");
  if (workspace_bytes < nms_workspace_bytes(n))
    return set_error(MV_ERR_INVALID_ARGUMENT, "nms: workspace of %lld bytes, need %lld (mv_nms_workspace_bytes)", (long long)workspace_bytes,
                     (long long)nms_workspace_bytes(n));
  if ((uintptr_t)workspace % 16) return set_error(MV_ERR_INVALID_ARGUMENT, "nms: the workspace must be 16-byte aligned");
  return launch_nms(boxes, scores, (int)n, iou_threshold, keep_out, keep_count_out, workspace, (hipStream_t)stream);
}

// One lane per output element in workgroups of 256: k rois x c_out channels x (pooled_h, pooled_w) must fit the launch grid.
static int roi_grid_check(const char* op, int64_t k, int c_out, int pooled_h, int pooled_w) {
  if (k > ((0x7fffffffLL * 256) / c_out) / pooled_h / pooled_w)
    return set_error(MV_ERR_UNSUPPORTED, "%s: %lld rois x %d channels x (%d, %d) outputs exceed the launch grid", op, (long long)k, c_out,
                     pooled_h, pooled_w);
  return 0;
}

// The checks roi_align, roi_pool, ps_roi_pool and ps_roi_align share: 0 launch, 1 nothing to do, < 0 the error.  has_second:
// the op writes a second output (argmax or channel_mapping), which must be there and alias nothing.
static int roi_check(const char* op, bool position_sensitive, const float* x, const float* rois, const float* y, bool has_second,
                     const int* second, int64_t n, int c, int h, int w, int64_t k, int pooled_h, int pooled_w) {
  if (n < 0 || c < 0 || h < 0 || w < 0 || k < 0 || pooled_h < 0 || pooled_w < 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: bad shape n=%lld c=%d (%d, %d), k=%lld, output (%d, %d)", op, (long long)n, c, h, w,
                     (long long)k, pooled_h, pooled_w);
  if (k == 0 || c == 0 || pooled_h == 0 || pooled_w == 0) return 1;
  if (position_sensitive && c % ((int64_t)pooled_h * pooled_w))
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: input channels must be a multiple of pooling height * pooling width, got %d for (%d, %d)",
                     op, c, pooled_h, pooled_w);
  if (n > 0 && (h == 0 || w == 0)) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: empty (%d, %d) feature map", op, h, w);
  if (n > 0x7fffffffLL || (int64_t)h * w > 0x7fffffffLL)
    return set_error(MV_ERR_UNSUPPORTED, "%s: %lld images of %d x %d exceed the 32-bit plane index", op, (long long)n, h, w);
  if (int rc = roi_grid_check(op, k, position_sensitive ? c / (pooled_h * pooled_w) : c, pooled_h, pooled_w)) return rc;
  if (!rois || !y || (has_second && !second) || (n > 0 && !x)) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: null pointer", op);
  const void* const s = second;
  if (x == y || rois == y || (has_second && (x == s || rois == s || y == s)))
    return set_error(MV_ERR_INVALID_ARGUMENT,
                     has_second ? "output must not alias input or the other output" : "output must not alias input");
  return 0;
}

int mv_roi_align_f32(const float* x, const float* rois, float* y, int64_t n, int c, int h, int w, int64_t k, int pooled_h, int pooled_w,
                     double spatial_scale, int sampling_ratio, int aligned, void* stream) {
  if (int rc = roi_check("roi_align", false, x, rois, y, false, nullptr, n, c, h, w, k, pooled_h, pooled_w)) return rc < 0 ? rc : MV_OK;
  return launch_roi_align(x, rois, y, (int)n, c, h, w, k, pooled_h, pooled_w, (float)spatial_scale, sampling_ratio, aligned ? 1 : 0,
                          (hipStream_t)stream);
}

int mv_multiscale_roi_align_f32(const float* const* xs, const int* hs, const int* ws, const double* scales, int levels, const float* rois,
                                const int64_t* roi_levels, float* y, int64_t n, int c, int64_t k, int pooled_h, int pooled_w,
                                int sampling_ratio, int aligned, void* stream) {
  if (levels < 0 || n < 0 || c < 0 || k < 0 || pooled_h < 0 || pooled_w < 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "multiscale_roi_align: bad shape levels=%d n=%lld c=%d, k=%lld, output (%d, %d)", levels,
                     (long long)n, c, (long long)k, pooled_h, pooled_w);
  if (levels > kMaxRoiLevels)
    return set_error(MV_ERR_UNSUPPORTED, "multiscale_roi_align: up to %d feature maps per call, got %d", kMaxRoiLevels, levels);
  if (k == 0 || c == 0 || pooled_h == 0 || pooled_w == 0) return MV_OK;
  if (levels > 0 && (!xs || !hs || !ws || !scales)) return set_error(MV_ERR_INVALID_ARGUMENT, "multiscale_roi_align: null level table");
  for (int l = 0; l < levels; ++l) {
    if (hs[l] < 0 || ws[l] < 0)
      return set_error(MV_ERR_INVALID_ARGUMENT, "multiscale_roi_align: bad shape (%d, %d) of feature map %d", hs[l], ws[l], l);
    if (n > 0 && (hs[l] == 0 || ws[l] == 0))
      return set_error(MV_ERR_INVALID_ARGUMENT, "multiscale_roi_align: empty (%d, %d) feature map %d", hs[l], ws[l], l);
    if ((int64_t)hs[l] * ws[l] > 0x7fffffffLL)
      return set_error(MV_ERR_UNSUPPORTED, "multiscale_roi_align: feature map %d of %d x %d exceeds the 32-bit plane index", l, hs[l], ws[l]);
  }
  if (n > 0x7fffffffLL) return set_error(MV_ERR_UNSUPPORTED, "multiscale_roi_align: %lld images exceed the 32-bit plane index", (long long)n);
  if (int rc = roi_grid_check("multiscale_roi_align", k, c, pooled_h, pooled_w)) return rc;
  if (!rois || !roi_levels || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "multiscale_roi_align: null pointer");
  if (rois == y || (const void*)roi_levels == (const void*)y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  if ((uintptr_t)roi_levels % 8) return set_error(MV_ERR_INVALID_ARGUMENT, "multiscale_roi_align: roi_levels must be 8-byte aligned");
  for (int l = 0; l < levels; ++l) {
    if (n > 0 && !xs[l]) return set_error(MV_ERR_INVALID_ARGUMENT, "multiscale_roi_align: null pointer (feature map %d)", l);
    if (xs[l] == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  }
  return launch_multiscale_roi_align(xs, hs, ws, scales, levels, rois, roi_levels, y, (int)n, c, k, pooled_h, pooled_w, sampling_ratio,
                                     aligned ? 1 : 0, (hipStream_t)stream);
}

// ---- box_iou family / masks_to_boxes: boxes.hip -------------------------------------------------------------------------------------
int mv_box_iou_f32(const float* boxes1, const float* boxes2, float* out, int64_t n, int64_t m, int mode, void* stream) {
  if (n < 0 || m < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "box_iou: bad shape n=%lld, m=%lld", (long long)n, (long long)m);
  if (mode < 0 || mode > 2)
    return set_error(MV_ERR_INVALID_ARGUMENT, "box_iou: unknown mode %d (0 iou, 1 generalized, 2 distance)", mode);
  if (n == 0 || m == 0) return MV_OK;
  if (!boxes1 || !boxes2 || !out) return set_error(MV_ERR_INVALID_ARGUMENT, "box_iou: null pointer");
  if (boxes1 == out || boxes2 == out) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  if (n > 0x7fffffffffffLL / m || !box_iou_grid_fits(n, m))
    return set_error(MV_ERR_UNSUPPORTED, "box_iou: %lld x %lld pairs exceed the launch grid", (long long)n, (long long)m);
  return launch_box_iou(boxes1, boxes2, out, n, m, mode, (hipStream_t)stream);
}

int64_t mv_masks_to_boxes_workspace_bytes(int64_t n) {
  if (n <= 0 || n > 0x7fffffffLL) return 0;
  return 16 * n;
}

static int masks_to_boxes(const void* masks, bool f32, float* boxes, int* empty_flag, int64_t n, int h, int w, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  if (n < 0 || h < 0 || w < 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "masks_to_boxes: bad shape n=%lld (%d, %d)", (long long)n, h, w);
  if (n == 0) return MV_OK;
  if (n > 0x7fffffffLL || !masks_to_boxes_grid_fits(n, h))
    return set_error(MV_ERR_UNSUPPORTED, "masks_to_boxes: %lld masks of %d rows exceed the launch grid", (long long)n, h);
  if (!boxes || !empty_flag || (h > 0 && w > 0 && !masks)) return set_error(MV_ERR_INVALID_ARGUMENT, "masks_to_boxes: null pointer");
  if (masks == (const void*)boxes || masks == (const void*)empty_flag || (const void*)boxes == (const void*)empty_flag)
    return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input or the other output");
  if ((uintptr_t)empty_flag % 4) return set_error(MV_ERR_INVALID_ARGUMENT, "masks_to_boxes: empty_flag must be 4-byte aligned");
  if (!workspace) return set_error(MV_ERR_INVALID_ARGUMENT, "masks_to_boxes: needs a workspace");
  if (workspace_bytes < 16 * n)
    return set_error(MV_ERR_INVALID_ARGUMENT, "masks_to_boxes: workspace of %lld bytes, need %lld (mv_masks_to_boxes_workspace_bytes)",
                     (long long)workspace_bytes, (long long)(16 * n));
  if ((uintptr_t)workspace % 16) return set_error(MV_ERR_INVALID_ARGUMENT, "masks_to_boxes: the workspace must be 16-byte aligned");
  return launch_masks_to_boxes(masks, f32, boxes, empty_flag, n, h, w, workspace, (hipStream_t)stream);
}

int mv_masks_to_boxes_u8(const unsigned char* masks, float* boxes, int* empty_flag, int64_t n, int h, int w, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  return masks_to_boxes(masks, false, boxes, empty_flag, n, h, w, workspace, workspace_bytes, stream);
}

int mv_masks_to_boxes_f32(const float* masks, float* boxes, int* empty_flag, int64_t n, int h, int w, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  return masks_to_boxes(masks, true, boxes, empty_flag, n, h, w, workspace, workspace_bytes, stream);
}

// ---- RPN top-k / decode, BoxCoder.decode: rpn.hip; the pyramid checks shared with the RetinaNet entries below ------------------------
struct ByteRange {
  const void* p;
  long long bytes;
};
static bool ranges_overlap(const ByteRange& a, const ByteRange& b) {
  const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
  return a0 < b0 + (uintptr_t)b.bytes && b0 < a0 + (uintptr_t)a.bytes;
}
// no output shares a byte with an input or with another output
static bool outputs_clear(const ByteRange* outs, int n_out, const ByteRange* ins, int n_in) {
  for (int i = 0; i < n_out; ++i) {
    for (int j = 0; j < n_in; ++j)
      if (ranges_overlap(outs[i], ins[j])) return false;
    for (int j = i + 1; j < n_out; ++j)
      if (ranges_overlap(outs[i], outs[j])) return false;
  }
  return true;
}

// The rpn and retinanet entries are one set of checks: a pyramid of per-level maps with `classes` logit channels per anchor, the
// rpn's with one (the two refusals that name the classes cannot fire then).  `op` names the entry in the messages.
//
// The level tables: 0 and taken = sum of min(k, a * h * w * classes) (k < 1: not computed), or the error.  The anchors of all
// levels, sum of a * h * w, times the classes stay below 2^31.
static int levels_check(const char* op, const int* hs, const int* ws, const int* as, int levels, int classes, int k, int64_t* taken) {
  if (levels < 1 || levels > kMaxRpnLevels)
    return set_error(levels > kMaxRpnLevels ? MV_ERR_UNSUPPORTED : MV_ERR_INVALID_ARGUMENT, "%s: 1 to %d levels per call, got %d", op,
                     kMaxRpnLevels, levels);
  if (!hs || !ws || !as) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: null level table", op);
  int64_t anchors = 0;
  for (int l = 0; l < levels; ++l) {
    if (hs[l] < 1 || ws[l] < 1 || as[l] < 1)
      return set_error(MV_ERR_INVALID_ARGUMENT, "%s: bad shape (%d anchors, %d, %d) of level %d", op, as[l], hs[l], ws[l], l);
    const int64_t hw = (int64_t)hs[l] * ws[l];
    if (hw > 0x7fffffffLL || hw * as[l] > 0x7fffffffLL || (anchors += hw * as[l]) > 0x7fffffffLL)
      return set_error(MV_ERR_UNSUPPORTED, "%s: the anchors of all levels exceed the 32-bit index", op);
  }
  if (classes < 1) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: classes must be positive, got %d", op, classes);
  if (anchors * classes > 0x7fffffffLL)
    return set_error(MV_ERR_UNSUPPORTED, "%s: %lld anchors x %d classes exceed the 32-bit index", op, (long long)anchors, classes);
  *taken = 0;
  for (int l = 0; l < levels; ++l) {
    const int64_t nl = (int64_t)as[l] * hs[l] * ws[l] * classes;
    *taken += nl < k ? nl : k;
  }
  return MV_OK;
}

// The bytes of a top-k entry's workspace, the level tables checked (taken: levels_check's).  The rpn's: a 64-bit candidate per
// index taken; retinanet's: retinanet_plan's.
typedef int64_t (*TopkBytes)(int64_t n, const int* hs, const int* ws, const int* as, int levels, int classes, int k, int64_t taken);
static int64_t rpn_topk_bytes(int64_t n, const int*, const int*, const int*, int, int, int, int64_t taken) { return (n * taken * 8 + 15) / 16 * 16; }
static int64_t retinanet_topk_bytes(int64_t n, const int* hs, const int* ws, const int* as, int levels, int classes, int k, int64_t) {
  return retinanet_plan(n, hs, ws, as, levels, classes, k).bytes;
}
// what the two *_topk_workspace_bytes entries answer: 0 for a call the launch entry refuses
static int64_t topk_workspace_bytes(const char* op, TopkBytes bytes, int64_t n, const int* hs, const int* ws, const int* as, int levels, int classes,
                                    int k) {
  int64_t taken;
  if (n <= 0 || n > 65535 || k < 1 || k > kRpnMaxK || levels_check(op, hs, ws, as, levels, classes, k, &taken)) return 0;
  return bytes(n, hs, ws, as, levels, classes, k, taken);
}

// The arguments of a top-k entry (m: topk_maps), in the order of the refusals: 0 launch, 1 nothing to do, < 0 the error.
static PyramidMaps topk_maps(const float* const* logits, const int* hs, const int* ws, const int* as, const int64_t* img_strides, int levels) {
  PyramidMaps m = {};
  m.logits = logits, m.hs = hs, m.ws = ws, m.as = as, m.logit_strides = img_strides, m.levels = levels;
  return m;
}
// Level l's map p, n images of `elems` elements, `stride` elements apart: kMapOk and *r, the bytes they span, or the first refusal
// (unaligned only where `aligned` asks for 4-byte pointers: the SSD entries do, the RPN family's do not), for the entry's words.
enum LevelMap { kMapOk = 0, kMapNull, kMapUnaligned, kMapStride };
static LevelMap level_map(const float* p, int64_t stride, int64_t elems, int64_t n, bool aligned, ByteRange* r) {
  if (!p) return kMapNull;
  if (aligned && (uintptr_t)p % 4) return kMapUnaligned;
  if (stride < elems || stride > 0x7fffffffffffLL / n) return kMapStride;
  *r = {p, ((n - 1) * stride + elems) * 4};
  return kMapOk;
}
// level_map with the words that the entries with one map per level share
static int level_map_check(const char* op, const char* of_what, int l, const float* p, int64_t stride, int64_t elems, int64_t n, bool aligned,
                           ByteRange* r) {
  const LevelMap rc = level_map(p, stride, elems, n, aligned, r);
  if (rc == kMapNull) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: null pointer (level %d)", op, l);
  if (rc == kMapUnaligned) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: the maps must be 4-byte aligned (level %d)", op, l);
  if (rc == kMapOk) return MV_OK;
  return set_error(MV_ERR_INVALID_ARGUMENT, "%s: image stride %lld of %slevel %d, its map has %lld elements", op, (long long)stride, of_what, l,
                   (long long)elems);
}
// ctr: the entry takes centerness maps too (FCOS): one anchor per location, m.ctrness[l] a map (n, 1, hs[l], ws[l]).
static int one_anchor_check(const char* op, const PyramidMaps& m) {
  for (int l = 0; l < m.levels; ++l)
    if (m.as[l] != 1) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: one anchor per location, level %d has %d", op, l, m.as[l]);
  return MV_OK;
}
static int ctr_check(const char* op, const PyramidMaps& m, int64_t n, ByteRange* ins) {
  if (!m.ctrness || !m.ctr_strides) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: null pointer", op);
  for (int l = 0; l < m.levels; ++l)
    if (int rc = level_map_check(op, "the centerness of ", l, m.ctrness[l], m.ctr_strides[l], (int64_t)m.hs[l] * m.ws[l], n, false, ins + l))
      return rc;
  return MV_OK;
}
static int topk_check(const char* op, TopkBytes bytes, const PyramidMaps& m, int classes, int64_t n, int k, const int* idx, const void* workspace,
                      int64_t workspace_bytes, bool ctr = false) {
  if (n < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: bad image count %lld", op, (long long)n);
  if (k < 1) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: k must be positive, got %d", op, k);
  int64_t taken;
  if (int rc = levels_check(op, m.hs, m.ws, m.as, m.levels, classes, k, &taken)) return rc;
  if (ctr)
    if (int rc = one_anchor_check(op, m)) return rc;
  if (k > kRpnMaxK) return set_error(MV_ERR_UNSUPPORTED, "%s: k up to %d, got %d", op, kRpnMaxK, k);
  if (n == 0) return 1;
  if (n > 65535) return set_error(MV_ERR_UNSUPPORTED, "%s: %lld images exceed the launch grid", op, (long long)n);
  if (!m.logits || !m.logit_strides || !idx) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: null pointer", op);
  const int64_t need = bytes(n, m.hs, m.ws, m.as, m.levels, classes, k, taken);
  ByteRange ins[2 * kMaxRpnLevels];
  if (ctr)
    if (int rc = ctr_check(op, m, n, ins + m.levels)) return rc;
  for (int l = 0; l < m.levels; ++l)
    if (int rc = level_map_check(op, "", l, m.logits[l], m.logit_strides[l], (int64_t)m.as[l] * m.hs[l] * m.ws[l] * classes, n, false, ins + l))
      return rc;
  if (!workspace) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: needs a workspace", op);
  if (workspace_bytes < need)
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: workspace of %lld bytes, need %lld (mv_%s_workspace_bytes)", op, (long long)workspace_bytes,
                     (long long)need, op);
  if ((uintptr_t)workspace % 16) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: the workspace must be 16-byte aligned", op);
  if ((uintptr_t)idx % 4) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: idx must be 4-byte aligned", op);
  const ByteRange outs[2] = {{idx, n * taken * 4}, {workspace, need}};
  if (!outputs_clear(outs, 2, ins, ctr ? 2 * m.levels : m.levels))
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: idx and the workspace must not overlap an input or each other", op);
  return 0;
}

// The arguments of a decode entry, in the order of the refusals: 0 launch, 1 nothing to do, < 0 the error.  out64 is the int64
// output, `out64_name` its word in the alignment message.
static int decode_check(const char* op, const char* out64_name, const PyramidMaps& m, int classes, const float* image_sizes, const int* idx,
                        int64_t n, int64_t k, const float* boxes, const float* scores, const int64_t* out64, const unsigned char* valid,
                        bool ctr = false) {
  if (n < 0 || k < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: bad shape n=%lld, k=%lld", op, (long long)n, (long long)k);
  int64_t taken;
  if (int rc = levels_check(op, m.hs, m.ws, m.as, m.levels, classes, 1, &taken)) return rc;
  if (ctr)
    if (int rc = one_anchor_check(op, m)) return rc;
  if (!m.strides_h || !m.strides_w) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: null level table", op);
  for (int l = 0; l < m.levels; ++l)
    if (m.strides_h[l] < 0 || m.strides_w[l] < 0 || (int64_t)m.strides_h[l] * m.hs[l] > 0x7fffffffLL ||
        (int64_t)m.strides_w[l] * m.ws[l] > 0x7fffffffLL)
      return set_error(MV_ERR_INVALID_ARGUMENT, "%s: bad strides (%d, %d) of level %d", op, m.strides_h[l], m.strides_w[l], l);
  if (n == 0 || k == 0) return 1;
  if (n > 0x7fffffffLL || k > (0x7fffffffLL * 256) / n)
    return set_error(MV_ERR_UNSUPPORTED, "%s: %lld x %lld candidates exceed the launch grid", op, (long long)n, (long long)k);
  if (!m.logits || !m.deltas || !m.logit_strides || !m.delta_strides || !m.base_anchors || !image_sizes || !idx || !boxes || !scores || !out64 ||
      !valid)
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: null pointer", op);
  if ((uintptr_t)out64 % 8) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: %s must be 8-byte aligned", op, out64_name);
  if ((uintptr_t)idx % 4) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: idx must be 4-byte aligned", op);
  ByteRange ins[3 * kMaxRpnLevels + 3];
  int n_in = 2 * m.levels + 3;
  if (ctr) {
    if (int rc = ctr_check(op, m, n, ins + n_in)) return rc;
    n_in += m.levels;
  }
  int64_t base_rows = 0;
  for (int l = 0; l < m.levels; ++l) {
    const int64_t al = (int64_t)m.as[l] * m.hs[l] * m.ws[l], nl = al * classes;
    const int64_t ls = m.logit_strides[l], ds = m.delta_strides[l];
    const LevelMap lg = level_map(m.logits[l], ls, nl, n, false, ins + 2 * l), dl = level_map(m.deltas[l], ds, 4 * al, n, false, ins + 2 * l + 1);
    if (lg == kMapNull || dl == kMapNull) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: null pointer (level %d)", op, l);
    if (lg || dl)  // the two maps of a level are refused in one message
      return set_error(MV_ERR_INVALID_ARGUMENT, "%s: image strides (%lld, %lld) of level %d, its maps have %lld and %lld elements", op,
                       (long long)ls, (long long)ds, l, (long long)nl, (long long)(4 * al));
    base_rows += m.as[l];
  }
  ins[2 * m.levels] = {m.base_anchors, base_rows * 16}, ins[2 * m.levels + 1] = {image_sizes, n * 8}, ins[2 * m.levels + 2] = {idx, n * k * 4};
  const ByteRange outs[4] = {{boxes, n * k * 16}, {scores, n * k * 4}, {out64, n * k * 8}, {valid, n * k}};
  if (!outputs_clear(outs, 4, ins, n_in))
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: the outputs must not overlap an input or each other", op);
  return 0;
}

int64_t mv_rpn_topk_workspace_bytes(int64_t n, const int* hs, const int* ws, const int* as, int levels, int k) {
  return topk_workspace_bytes("rpn_topk", rpn_topk_bytes, n, hs, ws, as, levels, 1, k);
}

int mv_rpn_topk_f32(const float* const* logits, const int* hs, const int* ws, const int* as, const int64_t* img_strides, int levels,
                    int64_t n, int k, int* idx, void* workspace, int64_t workspace_bytes, void* stream) {
  const PyramidMaps m = topk_maps(logits, hs, ws, as, img_strides, levels);
  if (int rc = topk_check("rpn_topk", rpn_topk_bytes, m, 1, n, k, idx, workspace, workspace_bytes)) return rc < 0 ? rc : MV_OK;
  return launch_rpn_topk(m, (int)n, k, idx, workspace, (hipStream_t)stream);
}

int mv_rpn_decode_f32(const float* const* logits, const float* const* deltas, const int* hs, const int* ws, const int* as,
                      const int64_t* logit_strides, const int64_t* delta_strides, const int* strides_h, const int* strides_w, int levels,
                      const float* base_anchors, const float* image_sizes, const int* idx, int64_t n, int64_t k, double wx, double wy,
                      double ww, double wh, double clip, double min_size, double score_thresh, float* boxes, float* scores,
                      int64_t* levels_out, unsigned char* valid, void* stream) {
  const PyramidMaps m = {logits, deltas, hs, ws, as, logit_strides, delta_strides, strides_h, strides_w, levels, base_anchors};
  if (int rc = decode_check("rpn_decode", "levels", m, 1, image_sizes, idx, n, k, boxes, scores, levels_out, valid)) return rc < 0 ? rc : MV_OK;
  return launch_rpn_decode(m, image_sizes, idx, n, k, decode_coef(wx, wy, ww, wh, clip), (float)min_size, (float)score_thresh, boxes, scores,
                           levels_out, valid, (hipStream_t)stream);
}

int mv_box_decode_f32(const float* boxes, const float* rel_codes, float* out, int64_t m, int classes, double wx, double wy, double ww,
                      double wh, double clip, void* stream) {
  if (m < 0 || classes < 1) return set_error(MV_ERR_INVALID_ARGUMENT, "box_decode: bad shape m=%lld, classes=%d", (long long)m, classes);
  if (m == 0) return MV_OK;
  if (m > (0x7fffffffLL * 256) / classes)
    return set_error(MV_ERR_UNSUPPORTED, "box_decode: %lld boxes x %d classes exceed the launch grid", (long long)m, classes);
  if (!boxes || !rel_codes || !out) return set_error(MV_ERR_INVALID_ARGUMENT, "box_decode: null pointer");
  const ByteRange ins[2] = {{boxes, m * 16}, {rel_codes, m * classes * 16}}, outs[1] = {{out, m * classes * 16}};
  if (!outputs_clear(outs, 1, ins, 2)) return set_error(MV_ERR_INVALID_ARGUMENT, "box_decode: the output must not overlap an input");
  return launch_box_decode(boxes, rel_codes, out, m, classes, decode_coef(wx, wy, ww, wh, clip), (hipStream_t)stream);
}

// ---- RoIHeads.postprocess_detections: roi_heads.hip -----------------------------------------------------------------------------------
int mv_roi_detections_f32(const float* class_logits, int64_t logits_stride, const float* box_regression, int64_t regression_stride,
                          const float* rois, const float* image_sizes, int64_t r, int classes, int64_t n, double wx, double wy, double ww,
                          double wh, double clip, double score_thresh, double min_size, float* boxes, float* scores, int64_t* labels,
                          unsigned char* valid, void* stream) {
  if (r < 0 || n < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "roi_detections: bad shape r=%lld, n=%lld", (long long)r, (long long)n);
  if (classes < 2)
    return set_error(MV_ERR_INVALID_ARGUMENT, "roi_detections: at least 2 classes (the background and one more), got %d", classes);
  if (classes > kRoiMaxClasses) return set_error(MV_ERR_UNSUPPORTED, "roi_detections: up to %d classes, got %d", kRoiMaxClasses, classes);
  if (logits_stride < classes || regression_stride < 4LL * classes)
    return set_error(MV_ERR_INVALID_ARGUMENT, "roi_detections: row strides (%lld, %lld), the rows have %d and %d elements",
                     (long long)logits_stride, (long long)regression_stride, classes, 4 * classes);
  if (r > 0x7fffffffLL / classes)
    return set_error(MV_ERR_UNSUPPORTED, "roi_detections: %lld rois x %d classes exceed the 32-bit index", (long long)r, classes);
  if (r == 0) return MV_OK;
  if (n < 1) return set_error(MV_ERR_INVALID_ARGUMENT, "roi_detections: %lld rois and no image", (long long)r);
  if (logits_stride > 0x7fffffffffffLL / r || regression_stride > 0x7fffffffffffLL / r)
    return set_error(MV_ERR_INVALID_ARGUMENT, "roi_detections: row strides (%lld, %lld) of %lld rows exceed the address space",
                     (long long)logits_stride, (long long)regression_stride, (long long)r);
  if (!class_logits || !box_regression || !rois || !image_sizes || !boxes || !scores || !labels || !valid)
    return set_error(MV_ERR_INVALID_ARGUMENT, "roi_detections: null pointer");
  if ((uintptr_t)labels % 8) return set_error(MV_ERR_INVALID_ARGUMENT, "roi_detections: labels must be 8-byte aligned");
  const int64_t cells = r * (classes - 1);
  const ByteRange ins[4] = {{class_logits, ((r - 1) * logits_stride + classes) * 4},
                            {box_regression, ((r - 1) * regression_stride + 4LL * classes) * 4},
                            {rois, r * 20},
                            {image_sizes, n * 8}};
  const ByteRange outs[4] = {{boxes, cells * 16}, {scores, cells * 4}, {labels, cells * 8}, {valid, cells}};
  if (!outputs_clear(outs, 4, ins, 4))
    return set_error(MV_ERR_INVALID_ARGUMENT, "roi_detections: the outputs must not overlap an input or each other");
  return launch_roi_detections(class_logits, logits_stride, box_regression, regression_stride, rois, image_sizes, r, classes, n,
                               decode_coef(wx, wy, ww, wh, clip), (float)score_thresh, (float)min_size, boxes, scores, labels, valid,
                               (hipStream_t)stream);
}

// ---- RetinaNet threshold + top-k / decode: retinanet.hip -------------------------------------------------------------------------------
// The checks are the rpn's, above (levels_check, topk_check, decode_check), with the class count.
int mv_retinanet_topk_chunk(void) { return kRetChunk; }

int64_t mv_retinanet_topk_workspace_bytes(int64_t n, const int* hs, const int* ws, const int* as, int levels, int classes, int k) {
  return topk_workspace_bytes("retinanet_topk", retinanet_topk_bytes, n, hs, ws, as, levels, classes, k);
}

int mv_retinanet_topk_f32(const float* const* logits, const int* hs, const int* ws, const int* as, const int64_t* img_strides, int levels,
                          int classes, int64_t n, int k, double score_thresh, int* idx, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  const PyramidMaps m = topk_maps(logits, hs, ws, as, img_strides, levels);
  if (int rc = topk_check("retinanet_topk", retinanet_topk_bytes, m, classes, n, k, idx, workspace, workspace_bytes))
    return rc < 0 ? rc : MV_OK;
  return launch_retinanet_topk(m, classes, (int)n, k, (float)score_thresh, idx, workspace, (hipStream_t)stream);
}

int mv_retinanet_decode_f32(const float* const* logits, const float* const* deltas, const int* hs, const int* ws, const int* as,
                            const int64_t* logit_strides, const int64_t* delta_strides, const int* strides_h, const int* strides_w,
                            int levels, int classes, const float* base_anchors, const float* image_sizes, const int* idx, int64_t n,
                            int64_t k, double wx, double wy, double ww, double wh, double clip, float* boxes, float* scores,
                            int64_t* labels, unsigned char* valid, void* stream) {
  const PyramidMaps m = {logits, deltas, hs, ws, as, logit_strides, delta_strides, strides_h, strides_w, levels, base_anchors};
  if (int rc = decode_check("retinanet_decode", "labels", m, classes, image_sizes, idx, n, k, boxes, scores, labels, valid))
    return rc < 0 ? rc : MV_OK;
  return launch_retinanet_decode(m, classes, image_sizes, idx, n, k, decode_coef(wx, wy, ww, wh, clip), boxes, scores, labels, valid,
                                 (hipStream_t)stream);
}

// ---- FCOS threshold + top-k / decode: retinanet.hip ------------------------------------------------------------------------------------
// RetinaNet's checks with the centerness maps (topk_check / decode_check with ctr); the workspace is
// mv_retinanet_topk_workspace_bytes'.
int mv_fcos_topk_f32(const float* const* logits, const float* const* ctrness, const int* hs, const int* ws, const int* as,
                     const int64_t* img_strides, const int64_t* ctr_strides, int levels, int classes, int64_t n, int k, double score_thresh,
                     int* idx, void* workspace, int64_t workspace_bytes, void* stream) {
  PyramidMaps m = topk_maps(logits, hs, ws, as, img_strides, levels);
  m.ctrness = ctrness, m.ctr_strides = ctr_strides;
  if (int rc = topk_check("fcos_topk", retinanet_topk_bytes, m, classes, n, k, idx, workspace, workspace_bytes, true)) return rc < 0 ? rc : MV_OK;
  return launch_fcos_topk(m, classes, (int)n, k, (float)score_thresh, idx, workspace, (hipStream_t)stream);
}

int mv_fcos_decode_f32(const float* const* logits, const float* const* ctrness, const float* const* deltas, const int* hs, const int* ws,
                       const int* as, const int64_t* logit_strides, const int64_t* ctr_strides, const int64_t* delta_strides,
                       const int* strides_h, const int* strides_w, int levels, int classes, const float* base_anchors,
                       const float* image_sizes, const int* idx, int64_t n, int64_t k, float* boxes, float* scores, int64_t* labels,
                       unsigned char* valid, void* stream) {
  const PyramidMaps m = {logits, deltas, hs, ws, as, logit_strides, delta_strides, strides_h, strides_w, levels, base_anchors, ctrness, ctr_strides};
  if (int rc = decode_check("fcos_decode", "labels", m, classes, image_sizes, idx, n, k, boxes, scores, labels, valid, true))
    return rc < 0 ? rc : MV_OK;
  return launch_fcos_decode(m, classes, image_sizes, idx, n, k, boxes, scores, labels, valid, (hipStream_t)stream);
}

// ---- SSD: ssd.hip ------------------------------------------------------------------------------------------------------------------
int mv_ssd_scores_f32(const float* const* logits, const int* hs, const int* ws, const int* as, const int64_t* img_strides, int levels,
                      int classes, int64_t n, float* scores, void* stream) {
  const char* const op = "ssd_scores";
  if (n < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: bad image count %lld", op, (long long)n);
  int64_t taken;
  if (int rc = levels_check(op, hs, ws, as, levels, classes, 1, &taken)) return rc;
  if (classes < 2) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: at least 2 classes (the background and one more), got %d", op, classes);
  if (n == 0) return MV_OK;
  if (n > 65535) return set_error(MV_ERR_UNSUPPORTED, "%s: %lld images exceed the launch grid", op, (long long)n);
  if (!logits || !img_strides || !scores) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: null pointer", op);
  if ((uintptr_t)scores % 4) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: scores must be 4-byte aligned", op);
  ByteRange ins[kMaxRpnLevels];
  int64_t anchors = 0;
  for (int l = 0; l < levels; ++l) {
    const int64_t al = (int64_t)as[l] * hs[l] * ws[l];
    if (int rc = level_map_check(op, "", l, logits[l], img_strides[l], al * classes, n, true, ins + l)) return rc;
    anchors += al;
  }
  const ByteRange out = {scores, n * anchors * classes * 4};
  if (!outputs_clear(&out, 1, ins, levels)) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: scores must not overlap an input", op);
  const PyramidMaps m = topk_maps(logits, hs, ws, as, img_strides, levels);
  return launch_ssd_scores(m, classes, (int)n, scores, (hipStream_t)stream);
}

int mv_ssd_topk_f32(const float* scores, int64_t n, int classes, int64_t v, int k, double score_thresh, int* idx, void* stream) {
  const char* const op = "ssd_topk";
  if (n < 0 || v < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: bad shape n=%lld, v=%lld", op, (long long)n, (long long)v);
  if (k < 1) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: k must be positive, got %d", op, k);
  if (classes < 2) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: at least 2 classes (the background and one more), got %d", op, classes);
  if (v > 0x7fffffffLL / classes)
    return set_error(MV_ERR_UNSUPPORTED, "%s: %lld anchors x %d classes exceed the 32-bit index", op, (long long)v, classes);
  if (k > kRpnMaxK) return set_error(MV_ERR_UNSUPPORTED, "%s: k up to %d, got %d", op, kRpnMaxK, k);
  if (n == 0) return MV_OK;
  if (n > 65535) return set_error(MV_ERR_UNSUPPORTED, "%s: %lld images exceed the launch grid", op, (long long)n);
  if (!idx || (v > 0 && !scores)) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: null pointer", op);
  if ((uintptr_t)scores % 4 || (uintptr_t)idx % 4) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: scores and idx must be 4-byte aligned", op);
  const ByteRange in = {scores, n * classes * v * 4}, out = {idx, n * (classes - 1) * (int64_t)k * 4};
  if (!outputs_clear(&out, 1, &in, 1)) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: idx must not overlap scores", op);
  return launch_ssd_topk(scores, (int)n, classes, (int)v, k, (float)score_thresh, idx, (hipStream_t)stream);
}

int mv_ssd_decode_f32(const float* scores, const float* const* deltas, const int* hs, const int* ws, const int* as,
                      const int64_t* delta_strides, int levels, int classes, const float* wh_pairs, const float* x_f, const float* y_f,
                      int batch_h, int batch_w, const float* image_sizes, const int* idx, int64_t n, int64_t k, double wx, double wy,
                      double ww, double wh, double clip, float* boxes, float* scores_out, int64_t* labels, unsigned char* valid,
                      void* stream) {
  const char* const op = "ssd_decode";
  if (n < 0 || k < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: bad shape n=%lld, k=%lld", op, (long long)n, (long long)k);
  int64_t taken;
  if (int rc = levels_check(op, hs, ws, as, levels, classes, 1, &taken)) return rc;
  if (classes < 2) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: at least 2 classes (the background and one more), got %d", op, classes);
  if (!x_f || !y_f) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: null level table", op);
  for (int l = 0; l < levels; ++l)
    if (!(x_f[l] > 0.f) || !(y_f[l] > 0.f) || x_f[l] > 3.0e38f || y_f[l] > 3.0e38f)
      return set_error(MV_ERR_INVALID_ARGUMENT, "%s: bad grid divisors (%g, %g) of level %d", op, (double)x_f[l], (double)y_f[l], l);
  if (batch_h < 1 || batch_w < 1) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: bad batch size (%d, %d)", op, batch_h, batch_w);
  if (n == 0 || k == 0) return MV_OK;
  if (n > 0x7fffffffLL || k > (0x7fffffffLL * 256) / n)
    return set_error(MV_ERR_UNSUPPORTED, "%s: %lld x %lld candidates exceed the launch grid", op, (long long)n, (long long)k);
  if (!scores || !deltas || !delta_strides || !wh_pairs || !image_sizes || !idx || !boxes || !scores_out || !labels || !valid)
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: null pointer", op);
  if ((uintptr_t)labels % 8) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: labels must be 8-byte aligned", op);
  if ((uintptr_t)idx % 4) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: idx must be 4-byte aligned", op);
  if ((uintptr_t)scores % 4 || (uintptr_t)wh_pairs % 4 || (uintptr_t)image_sizes % 4 || (uintptr_t)boxes % 4 || (uintptr_t)scores_out % 4)
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: the float tensors must be 4-byte aligned", op);
  ByteRange ins[kMaxRpnLevels + 4];
  int64_t anchors = 0, pairs = 0;
  for (int l = 0; l < levels; ++l) {
    const int64_t al = (int64_t)as[l] * hs[l] * ws[l];
    if (int rc = level_map_check(op, "", l, deltas[l], delta_strides[l], 4 * al, n, true, ins + l)) return rc;
    anchors += al, pairs += as[l];
  }
  ins[levels] = {scores, n * anchors * classes * 4}, ins[levels + 1] = {wh_pairs, pairs * 8}, ins[levels + 2] = {image_sizes, n * 8};
  ins[levels + 3] = {idx, n * k * 4};
  const ByteRange outs[4] = {{boxes, n * k * 16}, {scores_out, n * k * 4}, {labels, n * k * 8}, {valid, n * k}};
  if (!outputs_clear(outs, 4, ins, levels + 4))
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: the outputs must not overlap an input or each other", op);
  PyramidMaps m = {};
  m.deltas = deltas, m.hs = hs, m.ws = ws, m.as = as, m.delta_strides = delta_strides, m.levels = levels;
  return launch_ssd_decode(scores, m, classes, wh_pairs, x_f, y_f, batch_h, batch_w, image_sizes, idx, n, k, decode_coef(wx, wy, ww, wh, clip),
                           boxes, scores_out, labels, valid, (hipStream_t)stream);
}

// ---- GroupNorm (+ ReLU): groupnorm.hip ---------------------------------------------------------------------------------------------
int mv_group_norm_chunk(void) { return kGnChunk; }

// 0 and the slabs' extent, or the error: the shape, the groups and the launch grid
static int group_norm_shape(int64_t n, int c, int h, int w, int groups, int64_t* m, int64_t* blocks) {
  if (n < 0 || c < 0 || h < 0 || w < 0) return set_error(MV_ERR_INVALID_ARGUMENT, "group_norm_act: negative size (n=%lld c=%d h=%d w=%d)", (long long)n, c, h, w);
  if (groups < 1) return set_error(MV_ERR_INVALID_ARGUMENT, "group_norm_act: groups must be positive, got %d", groups);
  if (c % groups) return set_error(MV_ERR_INVALID_ARGUMENT, "group_norm_act: %d channels are not divisible by %d groups", c, groups);
  *m = (int64_t)(c / groups) * h * w;
  if ((int64_t)h * w > 0x7fffffffLL || *m > 0x7fffffffLL)
    return set_error(MV_ERR_UNSUPPORTED, "group_norm_act: a group of %lld elements exceeds the 32-bit index", (long long)*m);
  *blocks = *m ? n * groups * group_norm_chunks(*m) : 0;
  if (n > 0x7fffffffLL || *blocks > 0x7fffffffLL)
    return set_error(MV_ERR_UNSUPPORTED, "group_norm_act: %lld workgroups exceed the launch grid", (long long)*blocks);
  return MV_OK;
}

int64_t mv_group_norm_workspace_bytes(int64_t n, int c, int h, int w, int groups) {
  int64_t m, blocks;
  if (group_norm_shape(n, c, h, w, groups, &m, &blocks)) return 0;
  return blocks * 16;
}

int mv_group_norm_act_f32(const float* x, float* y, const float* weight, const float* bias, int64_t n, int c, int h, int w, int groups,
                          int64_t x_stride, int64_t y_stride, double eps, int relu, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  int64_t m, blocks;
  if (int rc = group_norm_shape(n, c, h, w, groups, &m, &blocks)) return rc;
  if (!(eps > 0) || eps > 3.0e38 || !((float)eps > 0.f))
    return set_error(MV_ERR_INVALID_ARGUMENT, "group_norm_act: eps must be positive and finite in float32, got %g", eps);
  if (blocks == 0) return MV_OK;
  const int64_t image = (int64_t)c * h * w;
  if (x_stride < image || y_stride < image || x_stride > 0x7fffffffffffLL / n || y_stride > 0x7fffffffffffLL / n)
    return set_error(MV_ERR_INVALID_ARGUMENT, "group_norm_act: image strides (%lld, %lld), an image has %lld elements", (long long)x_stride,
                     (long long)y_stride, (long long)image);
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "group_norm_act: null pointer");
  if ((uintptr_t)x % 4 || (uintptr_t)y % 4) return set_error(MV_ERR_INVALID_ARGUMENT, "group_norm_act: x and y must be 4-byte aligned");
  const ByteRange xr = {x, ((n - 1) * x_stride + image) * 4}, yr = {y, ((n - 1) * y_stride + image) * 4};
  // in place exactly (the same pointer and stride) or apart
  if (!(x == y && x_stride == y_stride) && ranges_overlap(xr, yr))
    return set_error(MV_ERR_INVALID_ARGUMENT, "group_norm_act: y must be x itself (in place) or must not overlap it");
  if (!workspace) return set_error(MV_ERR_INVALID_ARGUMENT, "group_norm_act: needs a workspace");
  if (workspace_bytes < blocks * 16)
    return set_error(MV_ERR_INVALID_ARGUMENT, "group_norm_act: workspace of %lld bytes, need %lld (mv_group_norm_workspace_bytes)",
                     (long long)workspace_bytes, (long long)(blocks * 16));
  if ((uintptr_t)workspace % 16) return set_error(MV_ERR_INVALID_ARGUMENT, "group_norm_act: the workspace must be 16-byte aligned");
  const ByteRange wr = {workspace, blocks * 16};
  const ByteRange params[2] = {{weight, weight ? c * 4LL : 0}, {bias, bias ? c * 4LL : 0}};
  if (ranges_overlap(wr, xr) || ranges_overlap(wr, yr) || ranges_overlap(wr, params[0]) || ranges_overlap(wr, params[1]) ||
      ranges_overlap(yr, params[0]) || ranges_overlap(yr, params[1]))
    return set_error(MV_ERR_INVALID_ARGUMENT, "group_norm_act: the workspace and y must not overlap an input or each other");
  return launch_group_norm_act(x, y, weight, bias, n, c, h, w, groups, x_stride, y_stride, (float)eps, relu != 0, workspace,
                               (hipStream_t)stream);
}

// ---- weight * F.normalize(x, dim=1): l2norm.hip ------------------------------------------------------------------------------------
int mv_l2_normalize_scale_f32(const float* x, float* y, const float* weight, int64_t n, int c, int h, int w, int64_t x_stride,
                              int64_t y_stride, double eps, void* stream) {
  if (n < 0 || c < 0 || h < 0 || w < 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "l2_normalize_scale: negative size (n=%lld c=%d h=%d w=%d)", (long long)n, c, h, w);
  const int64_t hw = (int64_t)h * w, image = (int64_t)c * hw;
  if (hw > 0x7fffffffLL || image > 0x7fffffffLL)
    return set_error(MV_ERR_UNSUPPORTED, "l2_normalize_scale: an image of %d x %d x %d elements exceeds the 32-bit index", c, h, w);
  const int64_t blocks = n * l2_normalize_blocks(hw);
  if (n > 0x7fffffffLL || blocks > 0x7fffffffLL)
    return set_error(MV_ERR_UNSUPPORTED, "l2_normalize_scale: %lld workgroups exceed the launch grid", (long long)blocks);
  if (!(eps > 0) || eps > 3.0e38 || !((float)eps > 0.f))
    return set_error(MV_ERR_INVALID_ARGUMENT, "l2_normalize_scale: eps must be positive and finite in float32, got %g", eps);
  if (n == 0 || image == 0) return MV_OK;
  if (x_stride < image || y_stride < image || x_stride > 0x7fffffffffffLL / n || y_stride > 0x7fffffffffffLL / n)
    return set_error(MV_ERR_INVALID_ARGUMENT, "l2_normalize_scale: image strides (%lld, %lld), an image has %lld elements",
                     (long long)x_stride, (long long)y_stride, (long long)image);
  if (!x || !y || !weight) return set_error(MV_ERR_INVALID_ARGUMENT, "l2_normalize_scale: null pointer");
  if ((uintptr_t)x % 4 || (uintptr_t)y % 4 || (uintptr_t)weight % 4)
    return set_error(MV_ERR_INVALID_ARGUMENT, "l2_normalize_scale: x, y and weight must be 4-byte aligned");
  const ByteRange xr = {x, ((n - 1) * x_stride + image) * 4}, yr = {y, ((n - 1) * y_stride + image) * 4}, wr = {weight, c * 4LL};
  // in place exactly (the same pointer and stride) or apart
  if (!(x == y && x_stride == y_stride) && ranges_overlap(xr, yr))
    return set_error(MV_ERR_INVALID_ARGUMENT, "l2_normalize_scale: y must be x itself (in place) or must not overlap it");
  if (ranges_overlap(yr, wr)) return set_error(MV_ERR_INVALID_ARGUMENT, "l2_normalize_scale: y must not overlap weight");
  return launch_l2_normalize_scale(x, y, weight, n, c, h, w, x_stride, y_stride, (float)eps, (hipStream_t)stream);
}

// ---- roi_pool / ps_roi_pool / ps_roi_align: roi_pool.hip ---------------------------------------------------------------------------
// (the checks: roi_check, with mv_roi_align_f32)
int mv_roi_pool_f32(const float* x, const float* rois, float* y, int* argmax, int64_t n, int c, int h, int w, int64_t k, int pooled_h,
                    int pooled_w, double spatial_scale, void* stream) {
  if (int rc = roi_check("roi_pool", false, x, rois, y, true, argmax, n, c, h, w, k, pooled_h, pooled_w)) return rc < 0 ? rc : MV_OK;
  return launch_roi_pool(x, rois, y, argmax, (int)n, c, h, w, k, pooled_h, pooled_w, (float)spatial_scale, (hipStream_t)stream);
}

int mv_ps_roi_pool_f32(const float* x, const float* rois, float* y, int* channel_mapping, int64_t n, int c, int h, int w, int64_t k,
                       int pooled_h, int pooled_w, double spatial_scale, void* stream) {
  if (int rc = roi_check("ps_roi_pool", true, x, rois, y, true, channel_mapping, n, c, h, w, k, pooled_h, pooled_w))
    return rc < 0 ? rc : MV_OK;
  return launch_ps_roi_pool(x, rois, y, channel_mapping, (int)n, c, h, w, k, pooled_h, pooled_w, (float)spatial_scale, (hipStream_t)stream);
}

int mv_ps_roi_align_f32(const float* x, const float* rois, float* y, int* channel_mapping, int64_t n, int c, int h, int w, int64_t k,
                        int pooled_h, int pooled_w, double spatial_scale, int sampling_ratio, void* stream) {
  if (int rc = roi_check("ps_roi_align", true, x, rois, y, true, channel_mapping, n, c, h, w, k, pooled_h, pooled_w))
    return rc < 0 ? rc : MV_OK;
  return launch_ps_roi_align(x, rois, y, channel_mapping, (int)n, c, h, w, k, pooled_h, pooled_w, (float)spatial_scale, sampling_ratio,
                             (hipStream_t)stream);
}

static int elastic(const void* x, void* y, bool u8, int64_t planes, int channels, int h, int wdt, const float* base_x,
                   const float* base_y, const float* disp, int64_t disp_sh, int64_t disp_sw, int64_t disp_sc, int mode,
                   const float* fill, void* stream) {
  if (planes <= 0 || h <= 0 || wdt <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "elastic: bad shape planes=%lld (%d, %d)", (long long)planes, h, wdt);
  if (channels <= 0 || planes % channels)
    return set_error(MV_ERR_INVALID_ARGUMENT, "elastic: planes (%lld) must be a multiple of channels (%d)", (long long)planes, channels);
  if (mode != 0 && mode != 1) return set_error(MV_ERR_INVALID_ARGUMENT, "elastic: unknown mode %d (0 bilinear, 1 nearest)", mode);
  if (!x || !y || !base_x || !base_y || !disp) return set_error(MV_ERR_INVALID_ARGUMENT, "elastic: null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  if ((int64_t)h * wdt > 0x7fffffffLL)
    return set_error(MV_ERR_UNSUPPORTED, "elastic: planes of %d x %d pixels exceed 2^31 - 1", h, wdt);
  return launch_elastic(x, y, u8, planes, channels, h, wdt, base_x, base_y, disp, disp_sh, disp_sw, disp_sc, mode, fill,
                        (hipStream_t)stream);
}

int mv_elastic_f32(const float* x, float* y, int64_t planes, int channels, int h, int wdt, const float* base_x,
                   const float* base_y, const float* disp, int64_t disp_sh, int64_t disp_sw, int64_t disp_sc, int mode,
                   const float* fill, void* stream) {
  return elastic(x, y, false, planes, channels, h, wdt, base_x, base_y, disp, disp_sh, disp_sw, disp_sc, mode, fill, stream);
}

int mv_elastic_u8(const uint8_t* x, uint8_t* y, int64_t planes, int channels, int h, int wdt, const float* base_x,
                  const float* base_y, const float* disp, int64_t disp_sh, int64_t disp_sw, int64_t disp_sc, int mode,
                  const float* fill, void* stream) {
  return elastic(x, y, true, planes, channels, h, wdt, base_x, base_y, disp, disp_sh, disp_sw, disp_sc, mode, fill, stream);
}

static int warp(const void* x, void* y, bool u8, int64_t planes, int channels, int ih, int iw, int oh, int ow,
                const float* coeffs, int kind, int order, int mode, const float* fill, void* stream) {
  if (planes <= 0 || ih <= 0 || iw <= 0 || oh <= 0 || ow <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "warp: bad shape planes=%lld (%d, %d) -> (%d, %d)", (long long)planes, ih, iw, oh,
                     ow);
  if (channels <= 0 || planes % channels)
    return set_error(MV_ERR_INVALID_ARGUMENT, "warp: planes (%lld) must be a multiple of channels (%d)", (long long)planes, channels);
  if (kind != 0 && kind != 1) return set_error(MV_ERR_INVALID_ARGUMENT, "warp: unknown kind %d (0 affine, 1 perspective)", kind);
  if (order != 0 && order != 1)
    return set_error(MV_ERR_INVALID_ARGUMENT, "warp: unknown grid order %d (0 plain sum, 1 fma chain)", order);
  if (mode != 0 && mode != 1) return set_error(MV_ERR_INVALID_ARGUMENT, "warp: unknown mode %d (0 bilinear, 1 nearest)", mode);
  if (!x || !y || !coeffs) return set_error(MV_ERR_INVALID_ARGUMENT, "warp: null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  if ((int64_t)ih * iw > 0x7fffffffLL || (int64_t)oh * ow > 0x7fffffffLL)
    return set_error(MV_ERR_UNSUPPORTED, "warp: planes of %d x %d -> %d x %d pixels exceed 2^31 - 1", ih, iw, oh, ow);
  return launch_warp(x, y, u8, planes, channels, ih, iw, oh, ow, coeffs, kind, order, mode, fill, (hipStream_t)stream);
}

int mv_warp_f32(const float* x, float* y, int64_t planes, int channels, int ih, int iw, int oh, int ow, const float* coeffs,
                int kind, int order, int mode, const float* fill, void* stream) {
  return warp(x, y, false, planes, channels, ih, iw, oh, ow, coeffs, kind, order, mode, fill, stream);
}

int mv_warp_u8(const uint8_t* x, uint8_t* y, int64_t planes, int channels, int ih, int iw, int oh, int ow, const float* coeffs,
               int kind, int order, int mode, const float* fill, void* stream) {
  return warp(x, y, true, planes, channels, ih, iw, oh, ow, coeffs, kind, order, mode, fill, stream);
}

int64_t mv_color_workspace_bytes(int64_t images, int h, int w, int u8) {
  if (images <= 0 || h <= 0 || w <= 0) return 0;
  return color_workspace_bytes(images, h, w, u8 != 0);
}

static int color_chain(const void* x, void* y, bool u8, int64_t images, int channels, int h, int w, const int* ops,
                       const double* factors, int n_ops, int form, void* ws, int64_t ws_bytes, void* stream) {
  if (images <= 0 || h <= 0 || w <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "color: bad shape images=%lld (%d, %d)", (long long)images, h, w);
  if (channels != 1 && channels != 3)
    return set_error(MV_ERR_INVALID_ARGUMENT, "color: channels must be 1 or 3, got %d", channels);
  if (n_ops < 1 || n_ops > 4) return set_error(MV_ERR_INVALID_ARGUMENT, "color: a chain has 1 to 4 ops, got %d", n_ops);
  if (!x || !y || !ops || !factors) return set_error(MV_ERR_INVALID_ARGUMENT, "color: null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  if (form != 0 && form != 1) return set_error(MV_ERR_INVALID_ARGUMENT, "color: unknown blend form %d (0 plain, 1 fma)", form);
  int contrasts = 0;
  for (int k = 0; k < n_ops; ++k) {
    if (ops[k] < MV_COLOR_BRIGHTNESS || ops[k] > MV_COLOR_HUE)
      return set_error(MV_ERR_INVALID_ARGUMENT, "color: unknown op code %d at position %d", ops[k], k);
    const double f = factors[k];
    if (ops[k] == MV_COLOR_HUE ? !(f >= -0.5 && f <= 0.5) : !(f >= 0.0))
      return set_error(MV_ERR_INVALID_ARGUMENT, "color: factor %g of op %d is out of range", f, ops[k]);
    contrasts += ops[k] == MV_COLOR_CONTRAST;
  }
  if (contrasts > 1) return set_error(MV_ERR_INVALID_ARGUMENT, "color: a chain holds at most one contrast op, got %d", contrasts);
  if (contrasts) {
    const int64_t need = color_workspace_bytes(images, h, w, u8);
    if (!ws) return set_error(MV_ERR_INVALID_ARGUMENT, "color: a chain with contrast needs a workspace");
    if (ws_bytes < need)
      return set_error(MV_ERR_INVALID_ARGUMENT, "color: workspace of %lld bytes, need %lld", (long long)ws_bytes, (long long)need);
    if ((uintptr_t)ws % 16)
      return set_error(MV_ERR_INVALID_ARGUMENT, "color: the workspace must be 16-byte aligned");
  }
  if (!color_grid_fits(images, h, w, u8))
    return set_error(MV_ERR_UNSUPPORTED, "color: %lld images of %d x %d pixels exceed the launch grid", (long long)images, h, w);
  return launch_color_chain(x, y, u8, images, channels, h, w, ops, factors, n_ops, form, ws, (hipStream_t)stream);
}

int mv_color_chain_f32(const float* x, float* y, int64_t images, int channels, int h, int w, const int* ops,
                       const double* factors, int n_ops, int form, void* workspace, int64_t workspace_bytes, void* stream) {
  return color_chain(x, y, false, images, channels, h, w, ops, factors, n_ops, form, workspace, workspace_bytes, stream);
}

int mv_color_chain_u8(const uint8_t* x, uint8_t* y, int64_t images, int channels, int h, int w, const int* ops,
                      const double* factors, int n_ops, int form, void* workspace, int64_t workspace_bytes, void* stream) {
  return color_chain(x, y, true, images, channels, h, w, ops, factors, n_ops, form, workspace, workspace_bytes, stream);
}

static int rgb_to_grayscale(const void* x, void* y, bool u8, int64_t images, int h, int w, int out_channels, int form,
                            void* stream) {
  if (images <= 0 || h <= 0 || w <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "rgb_to_grayscale: bad shape images=%lld (%d, %d)", (long long)images, h, w);
  if (out_channels != 1 && out_channels != 3)
    return set_error(MV_ERR_INVALID_ARGUMENT, "rgb_to_grayscale: out_channels must be 1 or 3, got %d", out_channels);
  if (form != 0 && form != 1)
    return set_error(MV_ERR_INVALID_ARGUMENT, "rgb_to_grayscale: unknown form %d (0 plain, 1 fma)", form);
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "rgb_to_grayscale: null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  if (!color_grid_fits(images, h, w, u8))
    return set_error(MV_ERR_UNSUPPORTED, "rgb_to_grayscale: %lld images of %d x %d pixels exceed the launch grid",
                     (long long)images, h, w);
  return launch_rgb_to_grayscale(x, y, u8, images, h, w, out_channels, form, (hipStream_t)stream);
}

int mv_rgb_to_grayscale_f32(const float* x, float* y, int64_t images, int h, int w, int out_channels, int form, void* stream) {
  return rgb_to_grayscale(x, y, false, images, h, w, out_channels, form, stream);
}

int mv_rgb_to_grayscale_u8(const uint8_t* x, uint8_t* y, int64_t images, int h, int w, int out_channels, int form,
                           void* stream) {
  return rgb_to_grayscale(x, y, true, images, h, w, out_channels, form, stream);
}

static int pointwise(const void* x, void* y, bool u8, int64_t n, int op, double param, void* stream) {
  if (n <= 0) return set_error(MV_ERR_INVALID_ARGUMENT, "pointwise: bad element count %lld", (long long)n);
  if (op < MV_POINT_INVERT || op > MV_POINT_SOLARIZE) return set_error(MV_ERR_INVALID_ARGUMENT, "pointwise: unknown op code %d", op);
  if (op == MV_POINT_POSTERIZE && !(param >= 0.0 && param <= 8.0 && param == (double)(int)param))
    return set_error(MV_ERR_INVALID_ARGUMENT, "pointwise: posterize bits must be an integer in [0, 8], got %g", param);
  if (op == MV_POINT_SOLARIZE && param != param) return set_error(MV_ERR_INVALID_ARGUMENT, "pointwise: solarize threshold is NaN");
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "pointwise: null pointer");
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  return launch_pointwise(x, y, u8, n, op, param, (hipStream_t)stream);
}

int mv_pointwise_f32(const float* x, float* y, int64_t n, int op, double param, void* stream) {
  return pointwise(x, y, false, n, op, param, stream);
}

int mv_pointwise_u8(const uint8_t* x, uint8_t* y, int64_t n, int op, double param, void* stream) {
  return pointwise(x, y, true, n, op, param, stream);
}

int64_t mv_autocontrast_workspace_bytes(int64_t planes, int h, int w, int u8) {
  if (planes <= 0 || h <= 0 || w <= 0) return 0;
  return autocontrast_workspace_bytes(planes, (int64_t)h * w, u8 != 0);
}

int64_t mv_equalize_workspace_bytes(int64_t planes, int h, int w, int u8) {
  (void)u8;
  if (planes <= 0 || h <= 0 || w <= 0) return 0;
  return equalize_workspace_bytes(planes);
}

// the checks autocontrast and equalize share; need: the op's workspace size
static int plane_op_args(const char* what, const void* x, void* y, bool u8, int64_t planes, int h, int w, const void* ws,
                         int64_t ws_bytes, int64_t need) {
  if (planes <= 0 || h <= 0 || w <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: bad shape planes=%lld (%d, %d)", what, (long long)planes, h, w);
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
  if (x == y) return set_error(MV_ERR_INVALID_ARGUMENT, "output must not alias input");
  if (!ws) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: needs a workspace", what);
  if (ws_bytes < need)
    return set_error(MV_ERR_INVALID_ARGUMENT, "%s: workspace of %lld bytes, need %lld", what, (long long)ws_bytes, (long long)need);
  if ((uintptr_t)ws % 16) return set_error(MV_ERR_INVALID_ARGUMENT, "%s: the workspace must be 16-byte aligned", what);
  if (!autoaug_grid_fits(planes, (int64_t)h * w, u8))
    return set_error(MV_ERR_UNSUPPORTED, "%s: %lld planes of %d x %d pixels exceed the launch grid", what, (long long)planes, h, w);
  return MV_OK;
}

static int autocontrast(const void* x, void* y, bool u8, int64_t planes, int h, int w, void* ws, int64_t ws_bytes,
                        void* stream) {
  const int64_t need = planes > 0 && h > 0 && w > 0 ? autocontrast_workspace_bytes(planes, (int64_t)h * w, u8) : 0;
  if (int rc = plane_op_args("autocontrast", x, y, u8, planes, h, w, ws, ws_bytes, need)) return rc;
  return launch_autocontrast(x, y, u8, planes, (int64_t)h * w, ws, (hipStream_t)stream);
}

int mv_autocontrast_f32(const float* x, float* y, int64_t planes, int h, int w, void* workspace, int64_t workspace_bytes,
                        void* stream) {
  return autocontrast(x, y, false, planes, h, w, workspace, workspace_bytes, stream);
}

int mv_autocontrast_u8(const uint8_t* x, uint8_t* y, int64_t planes, int h, int w, void* workspace, int64_t workspace_bytes,
                       void* stream) {
  return autocontrast(x, y, true, planes, h, w, workspace, workspace_bytes, stream);
}

static int equalize(const void* x, void* y, bool u8, int64_t planes, int h, int w, void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = plane_op_args("equalize", x, y, u8, planes, h, w, ws, ws_bytes, equalize_workspace_bytes(planes))) return rc;
  if ((int64_t)h * w >= (int64_t)1 << 31)
    return set_error(MV_ERR_UNSUPPORTED, "equalize: planes of %d x %d pixels overflow the 32-bit histogram", h, w);
  return launch_equalize(x, y, u8, planes, (int64_t)h * w, ws, (hipStream_t)stream);
}

int mv_equalize_f32(const float* x, float* y, int64_t planes, int h, int w, void* workspace, int64_t workspace_bytes,
                    void* stream) {
  return equalize(x, y, false, planes, h, w, workspace, workspace_bytes, stream);
}

int mv_equalize_u8(const uint8_t* x, uint8_t* y, int64_t planes, int h, int w, void* workspace, int64_t workspace_bytes,
                   void* stream) {
  return equalize(x, y, true, planes, h, w, workspace, workspace_bytes, stream);
}

// ---- F.interpolate(bilinear) and the detection transform's front end: interp.hip --------------------------------------------------------
int mv_interpolate_bilinear_f32(const float* x, float* y, int64_t planes, int h, int w, int oh, int ow, void* stream) {
  if (planes < 0 || h < 1 || w < 1 || oh < 1 || ow < 1)
    return set_error(MV_ERR_INVALID_ARGUMENT, "interpolate: bad shape planes=%lld, (%d, %d) -> (%d, %d)", (long long)planes, h, w, oh, ow);
  if (planes == 0) return MV_OK;
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "interpolate: null pointer");
  if (planes > 0x7fffffffffffLL / ((int64_t)h * w) || planes > 0x7fffffffffffLL / ((int64_t)oh * ow))
    return set_error(MV_ERR_INVALID_ARGUMENT, "interpolate: %lld planes exceed the address space", (long long)planes);
  const ByteRange in = {x, planes * h * w * 4}, out = {y, planes * oh * ow * 4};
  if (!outputs_clear(&out, 1, &in, 1)) return set_error(MV_ERR_INVALID_ARGUMENT, "interpolate: the output must not overlap the input");
  if (!interp_grid_fits(planes, oh, ow))
    return set_error(MV_ERR_UNSUPPORTED, "interpolate: %lld planes of (%d, %d) exceed the launch grid", (long long)planes, oh, ow);
  return launch_interp_batch(&x, &h, &w, &oh, &ow, 1, (int)planes, nullptr, nullptr, y, oh, ow, (hipStream_t)stream);
}

int mv_detection_batch_f32(const float* const* xs, const int* hs, const int* ws, const int* ohs, const int* ows, int64_t n, int c,
                           const float* mean, const float* stdv, float* y, int hp, int wp, void* stream) {
  if (n < 0 || c < 1 || hp < 1 || wp < 1)
    return set_error(MV_ERR_INVALID_ARGUMENT, "detection_batch: bad shape n=%lld, c=%d, batch (%d, %d)", (long long)n, c, hp, wp);
  if (c > 16) return set_error(MV_ERR_UNSUPPORTED, "detection_batch: up to 16 channels, got %d", c);
  if (n == 0) return MV_OK;
  if (!xs || !hs || !ws || !ohs || !ows || !mean || !stdv || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "detection_batch: null pointer");
  for (int i = 0; i < c; ++i)
    if (stdv[i] == 0.f) return set_error(MV_ERR_INVALID_ARGUMENT, "std evaluated to zero, leading to division by zero.");
  const int64_t plane = (int64_t)hp * wp;
  if (n > 0x7fffffffffffLL / (plane * c)) return set_error(MV_ERR_INVALID_ARGUMENT, "detection_batch: %lld images exceed the address space", (long long)n);
  const ByteRange out = {y, n * c * plane * 4};
  for (int64_t i = 0; i < n; ++i) {
    if (!xs[i]) return set_error(MV_ERR_INVALID_ARGUMENT, "detection_batch: null pointer (image %lld)", (long long)i);
    if (hs[i] < 1 || ws[i] < 1 || ohs[i] < 1 || ows[i] < 1)
      return set_error(MV_ERR_INVALID_ARGUMENT, "detection_batch: bad size (%d, %d) -> (%d, %d) of image %lld", hs[i], ws[i], ohs[i], ows[i],
                       (long long)i);
    if (ohs[i] > hp || ows[i] > wp)
      return set_error(MV_ERR_INVALID_ARGUMENT, "detection_batch: image %lld resized to (%d, %d) does not fit the batch (%d, %d)", (long long)i,
                       ohs[i], ows[i], hp, wp);
    const ByteRange in = {xs[i], (int64_t)c * hs[i] * ws[i] * 4};
    if (!outputs_clear(&out, 1, &in, 1))
      return set_error(MV_ERR_INVALID_ARGUMENT, "detection_batch: the output must not overlap an input (image %lld)", (long long)i);
  }
  if (!interp_grid_fits((int64_t)kMaxDetImages * c, hp, wp))
    return set_error(MV_ERR_UNSUPPORTED, "detection_batch: a batch of (%d, %d) exceeds the launch grid", hp, wp);
  for (int64_t i = 0; i < n; i += kMaxDetImages) {  // one launch per kMaxDetImages images: the table is a kernel argument
    const int m = (int)(n - i < kMaxDetImages ? n - i : kMaxDetImages);
    if (int rc = launch_interp_batch(xs + i, hs + i, ws + i, ohs + i, ows + i, m, c, mean, stdv, y + i * c * plane, hp, wp, (hipStream_t)stream))
      return rc;
  }
  return MV_OK;
}

// ---- F.interpolate(bilinear) + argmax over the channels, the labels of a segmentation model: segment.hip --------------------------------
int mv_interpolate_argmax_f32(const float* x, void* y, int64_t n, int c, int h, int w, int oh, int ow, int out_bytes, void* stream) {
  if (n < 0 || c < 1 || h < 1 || w < 1 || oh < 1 || ow < 1)
    return set_error(MV_ERR_INVALID_ARGUMENT, "interpolate_argmax: bad shape n=%lld, c=%d, (%d, %d) -> (%d, %d)", (long long)n, c, h, w, oh, ow);
  if (out_bytes != 1 && out_bytes != 8)
    return set_error(MV_ERR_INVALID_ARGUMENT, "interpolate_argmax: out_bytes is 1 (uint8) or 8 (int64), got %d", out_bytes);
  if (out_bytes == 1 && c > 256)
    return set_error(MV_ERR_INVALID_ARGUMENT, "interpolate_argmax: %d classes do not fit a uint8 label (up to 256 do)", c);
  if (n == 0) return MV_OK;
  if (!x || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "interpolate_argmax: null pointer");
  if (out_bytes == 8 && (uintptr_t)y % 8) return set_error(MV_ERR_INVALID_ARGUMENT, "interpolate_argmax: int64 labels must be 8-byte aligned");
  if (n > 0x7fffffffffffLL / ((int64_t)h * w) / c || n > 0x7fffffffffffLL / ((int64_t)oh * ow) / 8)
    return set_error(MV_ERR_INVALID_ARGUMENT, "interpolate_argmax: %lld images exceed the address space", (long long)n);
  const ByteRange in = {x, n * c * h * w * 4}, out = {y, n * oh * ow * out_bytes};
  if (!outputs_clear(&out, 1, &in, 1)) return set_error(MV_ERR_INVALID_ARGUMENT, "interpolate_argmax: the output must not overlap the input");
  if ((int64_t)h * w > 0x3fffffffLL)  // a tap's byte offset in its plane is 32-bit
    return set_error(MV_ERR_UNSUPPORTED, "interpolate_argmax: a source plane of %d x %d elements exceeds the 32-bit byte offset", h, w);
  if (!interp_argmax_grid_fits(n, oh, ow))
    return set_error(MV_ERR_UNSUPPORTED, "interpolate_argmax: %lld images of (%d, %d) exceed the launch grid", (long long)n, oh, ow);
  return launch_interp_argmax(x, y, n, c, h, w, oh, ow, out_bytes, (hipStream_t)stream);
}

// ---- the mask branch of Mask R-CNN: mask.hip, and convnorm.hip's pixel-shuffle instance of the pointwise kernel --------------------------
int mv_paste_masks_f32(const float* masks, const float* boxes, float* y, int64_t r, int m, int padding, int h, int w, void* stream) {
  if (r < 0 || m < 1 || padding < 0 || h < 1 || w < 1)
    return set_error(MV_ERR_INVALID_ARGUMENT, "paste_masks: bad shape r=%lld, m=%d, padding=%d, image (%d, %d)", (long long)r, m, padding, h, w);
  if (padding > (0x7fffffff - m) / 2) return set_error(MV_ERR_INVALID_ARGUMENT, "paste_masks: padding=%d exceeds the index range", padding);
  if (r == 0) return MV_OK;
  if (!masks || !boxes || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "paste_masks: null pointer");
  if (r > 0x7fffffffffffLL / ((int64_t)h * w) || r > 0x7fffffffffffLL / ((int64_t)m * m))
    return set_error(MV_ERR_INVALID_ARGUMENT, "paste_masks: %lld masks exceed the address space", (long long)r);
  const ByteRange ins[2] = {{masks, r * m * m * 4}, {boxes, r * 16}}, out = {y, r * h * w * 4};
  if (!outputs_clear(&out, 1, ins, 2)) return set_error(MV_ERR_INVALID_ARGUMENT, "paste_masks: the output must not overlap an input");
  if (!paste_masks_grid_fits(r, h, w))
    return set_error(MV_ERR_UNSUPPORTED, "paste_masks: %lld masks into (%d, %d) exceed the launch grid", (long long)r, h, w);
  return launch_paste_masks(masks, boxes, y, r, m, padding, h, w, (hipStream_t)stream);
}

int mv_mask_probs_f32(const float* logits, const int64_t* labels, float* y, int64_t r, int classes, int mh, int mw, void* stream) {
  if (r < 0 || classes < 1 || mh < 1 || mw < 1)
    return set_error(MV_ERR_INVALID_ARGUMENT, "mask_probs: bad shape r=%lld, classes=%d, (%d, %d)", (long long)r, classes, mh, mw);
  if (r == 0) return MV_OK;
  if (!logits || !labels || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "mask_probs: null pointer");
  const int64_t plane = (int64_t)mh * mw;
  if (r > 0x7fffffffffffLL / plane / classes) return set_error(MV_ERR_INVALID_ARGUMENT, "mask_probs: %lld rois exceed the address space", (long long)r);
  if ((uintptr_t)labels % 8) return set_error(MV_ERR_INVALID_ARGUMENT, "mask_probs: labels must be 8-byte aligned");
  const ByteRange ins[2] = {{logits, r * classes * plane * 4}, {labels, r * 8}}, out = {y, r * plane * 4};
  if (!outputs_clear(&out, 1, ins, 2)) return set_error(MV_ERR_INVALID_ARGUMENT, "mask_probs: the output must not overlap an input");
  if (!mask_probs_grid_fits(r, plane))
    return set_error(MV_ERR_UNSUPPORTED, "mask_probs: %lld rois of (%d, %d) exceed the launch grid", (long long)r, mh, mw);
  return launch_mask_probs(logits, labels, y, r, classes, plane, (hipStream_t)stream);
}

int mv_conv_transpose2x2_bias_act_f32(const float* x, const float* w4, const float* bias4, float* y, int64_t n, int cin, int h, int w,
                                      int cout, int act, void* stream) {
  if (n < 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "conv_transpose2x2: bad shape n=%lld cin=%d cout=%d h=%d w=%d", (long long)n, cin, cout, h, w);
  if (act != MV_ACT_NONE && act != MV_ACT_RELU && act != MV_ACT_RELU6)
    return set_error(MV_ERR_INVALID_ARGUMENT, "conv_transpose2x2: bad activation code %d (none, ReLU and ReLU6 are supported)", act);
  if (cout > 0x7fffffff / 4) return set_error(MV_ERR_UNSUPPORTED, "conv_transpose2x2: cout=%d exceeds the index range", cout);
  if (n == 0) return MV_OK;
  if (!x || !w4 || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "conv_transpose2x2: null pointer");
  const int64_t hw = (int64_t)h * w;
  if (n > 0x7fffffffffffLL / hw / cin || n > 0x7fffffffffffLL / hw / 4 / cout)
    return set_error(MV_ERR_INVALID_ARGUMENT, "conv_transpose2x2: %lld images exceed the address space", (long long)n);
  const ByteRange ins[3] = {{x, n * cin * hw * 4}, {w4, (int64_t)cout * 16 * cin}, {bias4, bias4 ? (int64_t)cout * 16 : 0}};
  const ByteRange out = {y, n * cout * hw * 16};
  if (!outputs_clear(&out, 1, ins, 3)) return set_error(MV_ERR_INVALID_ARGUMENT, "conv_transpose2x2: the output must not overlap an input");
  const Epilogue e = {bias4, nullptr, nullptr, nullptr, MV_AFFINE_NONE, act};
  return launch_conv_transpose2x2(x, w4, y, n, cin, h, w, cout, e, (hipStream_t)stream);
}

// ---- the keypoint branch of Keypoint R-CNN: conv_igemm.hip's transposed store, keypoint.hip ---------------------------------------------
int mv_conv_transpose4x4s2_bias_act_f32(const float* x, const float* w2, const float* bias4, float* y, int64_t n, int cin, int h, int w,
                                        int cout, int act, void* stream) {
  if (n < 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0)
    return set_error(MV_ERR_INVALID_ARGUMENT, "conv_transpose4x4s2: bad shape n=%lld cin=%d cout=%d h=%d w=%d", (long long)n, cin, cout, h, w);
  if (act != MV_ACT_NONE && act != MV_ACT_RELU && act != MV_ACT_RELU6)
    return set_error(MV_ERR_INVALID_ARGUMENT, "conv_transpose4x4s2: bad activation code %d (none, ReLU and ReLU6 are supported)", act);
  // what the implicit-GEMM kernel's 32-bit indices cover: K = 4 cin, the (h + 1) x (w + 1) window positions, one image of x and of y
  const int64_t hw = (int64_t)h * w, positions = ((int64_t)h + 1) * ((int64_t)w + 1);
  if (cout > 0x7fffffff / 4 || cin >= 65536 / 4 || w + 1 >= 4096 || positions >= (1 << 20) || cin * hw >= (1LL << 30) || n > 65535)
    return set_error(MV_ERR_UNSUPPORTED, "conv_transpose4x4s2: n=%lld cin=%d cout=%d h=%d w=%d exceeds the kernel's index range",
                     (long long)n, cin, cout, h, w);
  if (n == 0) return MV_OK;
  if (!x || !w2 || !y) return set_error(MV_ERR_INVALID_ARGUMENT, "conv_transpose4x4s2: null pointer");
  if (n > 0x7fffffffffffLL / hw / cin || n > 0x7fffffffffffLL / hw / 4 / cout)
    return set_error(MV_ERR_INVALID_ARGUMENT, "conv_transpose4x4s2: %lld images exceed the address space", (long long)n);
  const ByteRange ins[3] = {{x, n * cin * hw * 4}, {w2, (int64_t)cout * 64 * cin}, {bias4, bias4 ? (int64_t)cout * 16 : 0}};
  const ByteRange out = {y, n * cout * hw * 16};
  if (!outputs_clear(&out, 1, ins, 3)) return set_error(MV_ERR_INVALID_ARGUMENT, "conv_transpose4x4s2: the output must not overlap an input");
  const Epilogue e = {bias4, nullptr, nullptr, nullptr, MV_AFFINE_NONE, act};
  return launch_conv_transpose4x4s2(x, w2, y, n, cin, h, w, cout, e, (hipStream_t)stream);
}

int mv_heatmaps_to_keypoints_f32(const float* maps, const float* rois, float* xy, float* scores, int64_t r, int k, int mh, int mw,
                                 void* stream) {
  if (r < 0 || k < 1 || mh < 1 || mw < 1)
    return set_error(MV_ERR_INVALID_ARGUMENT, "heatmaps_to_keypoints: bad shape r=%lld, k=%d, (%d, %d)", (long long)r, k, mh, mw);
  const int64_t plane = (int64_t)mh * mw;
  if (plane > kKpMaxPlane)
    return set_error(MV_ERR_UNSUPPORTED, "heatmaps_to_keypoints: heatmaps of (%d, %d) exceed %d elements", mh, mw, kKpMaxPlane);
  if (r == 0) return MV_OK;
  if (!maps || !rois || !xy || !scores) return set_error(MV_ERR_INVALID_ARGUMENT, "heatmaps_to_keypoints: null pointer");
  if (r > 0x7fffffffffffLL / plane / k) return set_error(MV_ERR_INVALID_ARGUMENT, "heatmaps_to_keypoints: %lld rois exceed the address space", (long long)r);
  const ByteRange ins[2] = {{maps, r * k * plane * 4}, {rois, r * 16}}, outs[2] = {{xy, r * k * 12}, {scores, r * k * 4}};
  if (!outputs_clear(outs, 2, ins, 2))
    return set_error(MV_ERR_INVALID_ARGUMENT, "heatmaps_to_keypoints: the outputs must not overlap an input or each other");
  if (!heatmaps_to_keypoints_grid_fits(r, k))
    return set_error(MV_ERR_INVALID_ARGUMENT, "heatmaps_to_keypoints: %lld rois of %d keypoints exceed the launch grid", (long long)r, k);
  return launch_heatmaps_to_keypoints(maps, rois, xy, scores, r, k, mh, mw, (hipStream_t)stream);
}

}  // extern "C"
