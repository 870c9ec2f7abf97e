// roi_pool.hip -- torchvision.ops.roi_pool, ps_roi_pool and ps_roi_align (forward) on gfx950, with the arithmetic of the
// reference's CPU kernels (csrc/ops/cpu/roi_pool_kernel.cpp, ps_roi_pool_kernel.cpp, ps_roi_align_kernel.cpp) as
// mi355vision.h states it.  As in detect.hip every float operation is written with __fmul_rn / __fadd_rn / __fsub_rn /
// __fdiv_rn: one IEEE rounding each, never an fma.
//
// One lane per output element (k, c_out, ph, pw), pw fastest, 256 threads per workgroup, no workspace; the lane recomputes its
// roi's geometry and writes both outputs of its element.  The element index, the batch-index rule and ps_roi_align's grid size
// and sampling loop are mv_roi.h's, shared with k_roi_align (detect.hip).  A batch index that does not truncate into [0, n) (or
// NaN): the element is 0, the second output -1 (roi_pool) or the input channel (the two position-sensitive ops), and nothing of
// x is read.
//
// Loops a roi can size: a pooling window is clamped to the map, at most h x w elements.  The adaptive grid of ps_roi_align
// (sampling_ratio <= 0) is roi_align's (roi_grid) and grows with the roi; it has no cap that roi_align does not have.
#include <cfloat>

#include "mv_common.h"
#include "mv_roi.h"

namespace mv {
namespace {

struct RoiPoolArgs {
  const float* x;
  const float* rois;
  float* y;
  int* second;      // argmax (roi_pool) or channel_mapping (ps_roi_pool, ps_roi_align)
  long long total;  // k * c_out * pooled_h * pooled_w
  int n, c, c_out, h, w, pooled_h, pooled_w, sampling_ratio;
  float spatial_scale;
};

// (int)roundf(v * scale), roundf half away from zero.  The rounded float is clamped to +-2^29 and a NaN becomes 0 before the
// conversion: inside that range this is the reference, outside it the reference's conversion is undefined, and with the clamp
// no later int expression (end - start + 1, window start + corner) overflows.
__device__ inline int rounded_corner(float v, float scale) {
  constexpr float kLimit = 536870912.f;  // 2^29
  float r = roundf(__fmul_rn(v, scale));
  if (r != r) r = 0.f;
  r = r < -kLimit ? -kLimit : (r > kLimit ? kLimit : r);
  return (int)r;
}

__device__ inline int clamp_to(int v, int hi) { return min(max(v, 0), hi); }

__global__ __launch_bounds__(256) void k_roi_pool(const RoiPoolArgs A) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= A.total) return;
  const RoiElem e = roi_elem(idx, A.pooled_h, A.pooled_w, A.c_out);
  const float* const roi = A.rois + e.k * 5;
  int b;
  if (!roi_image(roi[0], A.n, &b)) {
    A.y[idx] = 0.f;
    A.second[idx] = -1;
    return;
  }
  const int start_w = rounded_corner(roi[1], A.spatial_scale), start_h = rounded_corner(roi[2], A.spatial_scale);
  const int end_w = rounded_corner(roi[3], A.spatial_scale), end_h = rounded_corner(roi[4], A.spatial_scale);
  const int roi_w = max(end_w - start_w + 1, 1), roi_h = max(end_h - start_h + 1, 1);
  const float bin_h = __fdiv_rn((float)roi_h, (float)A.pooled_h), bin_w = __fdiv_rn((float)roi_w, (float)A.pooled_w);
  const int hstart = clamp_to((int)floorf(__fmul_rn((float)e.ph, bin_h)) + start_h, A.h);
  const int hend = clamp_to((int)ceilf(__fmul_rn((float)(e.ph + 1), bin_h)) + start_h, A.h);
  const int wstart = clamp_to((int)floorf(__fmul_rn((float)e.pw, bin_w)) + start_w, A.w);
  const int wend = clamp_to((int)ceilf(__fmul_rn((float)(e.pw + 1), bin_w)) + start_w, A.w);
  const bool empty = hend <= hstart || wend <= wstart;
  const float* const plane = A.x + ((size_t)b * A.c + e.ch) * ((size_t)A.h * A.w);
  float maxval = empty ? 0.f : -FLT_MAX;
  int maxidx = -1;
  for (int hh = hstart; hh < hend; ++hh)
    for (int ww = wstart; ww < wend; ++ww) {
      const float v = plane[hh * A.w + ww];
      if (v > maxval) maxval = v, maxidx = hh * A.w + ww;  // strict: the first of equal values wins, a NaN is never taken
    }
  A.y[idx] = maxval;
  A.second[idx] = maxidx;
}

__global__ __launch_bounds__(256) void k_ps_roi_pool(const RoiPoolArgs A) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= A.total) return;
  const RoiElem e = roi_elem(idx, A.pooled_h, A.pooled_w, A.c_out);
  const float* const roi = A.rois + e.k * 5;
  const int c_in = (e.ch * A.pooled_h + e.ph) * A.pooled_w + e.pw;
  A.second[idx] = c_in;
  int b;
  if (!roi_image(roi[0], A.n, &b)) {
    A.y[idx] = 0.f;
    return;
  }
  const int start_w = rounded_corner(roi[1], A.spatial_scale), start_h = rounded_corner(roi[2], A.spatial_scale);
  const int end_w = rounded_corner(roi[3], A.spatial_scale), end_h = rounded_corner(roi[4], A.spatial_scale);
  const int roi_w = max(end_w - start_w, 1), roi_h = max(end_h - start_h, 1);
  const float bin_h = __fdiv_rn((float)roi_h, (float)A.pooled_h), bin_w = __fdiv_rn((float)roi_w, (float)A.pooled_w);
  const int hstart = clamp_to((int)floorf(__fadd_rn(__fmul_rn((float)e.ph, bin_h), (float)start_h)), A.h);
  const int hend = clamp_to((int)ceilf(__fadd_rn(__fmul_rn((float)(e.ph + 1), bin_h), (float)start_h)), A.h);
  const int wstart = clamp_to((int)floorf(__fadd_rn(__fmul_rn((float)e.pw, bin_w), (float)start_w)), A.w);
  const int wend = clamp_to((int)ceilf(__fadd_rn(__fmul_rn((float)(e.pw + 1), bin_w), (float)start_w)), A.w);
  const bool empty = hend <= hstart || wend <= wstart;
  const float* const plane = A.x + ((size_t)b * A.c + c_in) * ((size_t)A.h * A.w);
  float sum = 0.f;
  for (int hh = hstart; hh < hend; ++hh)
    for (int ww = wstart; ww < wend; ++ww) sum = __fadd_rn(sum, plane[hh * A.w + ww]);
  // (hend - hstart) * (wend - wstart) <= h * w < 2^31 (checked by the entry point)
  A.y[idx] = empty ? 0.f : __fdiv_rn(sum, (float)((hend - hstart) * (wend - wstart)));
}

__global__ __launch_bounds__(256) void k_ps_roi_align(const RoiPoolArgs A) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= A.total) return;
  const RoiElem e = roi_elem(idx, A.pooled_h, A.pooled_w, A.c_out);
  const float* const roi = A.rois + e.k * 5;
  const int c_in = (e.ch * A.pooled_h + e.ph) * A.pooled_w + e.pw;
  A.second[idx] = c_in;
  int b;
  if (!roi_image(roi[0], A.n, &b)) {
    A.y[idx] = 0.f;
    return;
  }
  // the half-pixel shift is always applied, and the roi's size is NOT clamped to 1
  const float start_w = __fsub_rn(__fmul_rn(roi[1], A.spatial_scale), .5f);
  const float start_h = __fsub_rn(__fmul_rn(roi[2], A.spatial_scale), .5f);
  const float end_w = __fsub_rn(__fmul_rn(roi[3], A.spatial_scale), .5f);
  const float end_h = __fsub_rn(__fmul_rn(roi[4], A.spatial_scale), .5f);
  const float roi_w = __fsub_rn(end_w, start_w), roi_h = __fsub_rn(end_h, start_h);
  const float bin_h = __fdiv_rn(roi_h, (float)A.pooled_h), bin_w = __fdiv_rn(roi_w, (float)A.pooled_w);
  const float base_y = __fadd_rn(__fmul_rn((float)e.ph, bin_h), start_h), base_x = __fadd_rn(__fmul_rn((float)e.pw, bin_w), start_w);
  const int grid_h = roi_grid(A.sampling_ratio, roi_h, A.pooled_h), grid_w = roi_grid(A.sampling_ratio, roi_w, A.pooled_w);
  const float count = (float)(grid_h * grid_w);  // not max(.., 1): an empty adaptive grid gives 0 / 0 = NaN, as the reference's loop
  const float* const plane = A.x + ((size_t)b * A.c + c_in) * ((size_t)A.h * A.w);
  A.y[idx] = __fdiv_rn(roi_bin_sum(plane, A.h, A.w, base_y, base_x, bin_h, bin_w, grid_h, grid_w), count);
}

RoiPoolArgs roi_pool_args(const float* x, const float* rois, float* y, int* second, int n, int c, int c_out, int h, int w, int64_t k,
                          int pooled_h, int pooled_w, float spatial_scale, int sampling_ratio) {
  return {x, rois, y, second, (long long)k * c_out * pooled_h * pooled_w, n, c, c_out, h, w, pooled_h, pooled_w, sampling_ratio,
          spatial_scale};
}

dim3 roi_pool_grid(const RoiPoolArgs& a) { return dim3((unsigned)((a.total + 255) / 256)); }

}  // namespace

int launch_roi_pool(const float* x, const float* rois, float* y, int* argmax, int n, int c, int h, int w, int64_t k, int pooled_h,
                    int pooled_w, float spatial_scale, hipStream_t s) {
  const RoiPoolArgs a = roi_pool_args(x, rois, y, argmax, n, c, c, h, w, k, pooled_h, pooled_w, spatial_scale, 0);
  hipLaunchKernelGGL(k_roi_pool, roi_pool_grid(a), dim3(256), 0, s, a);
  return check_launch("k_roi_pool");
}

int launch_ps_roi_pool(const float* x, const float* rois, float* y, int* channel_mapping, int n, int c, int h, int w, int64_t k,
                       int pooled_h, int pooled_w, float spatial_scale, hipStream_t s) {
  const RoiPoolArgs a = roi_pool_args(x, rois, y, channel_mapping, n, c, c / (pooled_h * pooled_w), h, w, k, pooled_h, pooled_w,
                                      spatial_scale, 0);
  hipLaunchKernelGGL(k_ps_roi_pool, roi_pool_grid(a), dim3(256), 0, s, a);
  return check_launch("k_ps_roi_pool");
}

int launch_ps_roi_align(const float* x, const float* rois, float* y, int* channel_mapping, int n, int c, int h, int w, int64_t k,
                        int pooled_h, int pooled_w, float spatial_scale, int sampling_ratio, hipStream_t s) {
  const RoiPoolArgs a = roi_pool_args(x, rois, y, channel_mapping, n, c, c / (pooled_h * pooled_w), h, w, k, pooled_h, pooled_w,
                                      spatial_scale, sampling_ratio);
  hipLaunchKernelGGL(k_ps_roi_align, roi_pool_grid(a), dim3(256), 0, s, a);
  return check_launchf("k_ps_roi_align<%s>", sampling_ratio > 0 ? "fixed" : "adaptive");
}

}  // namespace mv
