// roi_pool.hip -- torchvision.ops.roi_pool, ps_roi_pool and ps_roi_align (forward) on gfx950, with the arithmetic of the
// reference's CPU kernels (csrc/ops/cpu/roi_pool_kernel.cpp, ps_roi_pool_kernel.cpp, ps_roi_align_kernel.cpp) as
// mi355vision.h states it.  As in detect.hip every float operation is written with __fmul_rn / __fadd_rn / __fsub_rn /
// __fdiv_rn: one IEEE rounding each, never an fma.
//
// One lane per output element (k, c_out, ph, pw), pw fastest, 256 threads per workgroup, no workspace; the lane recomputes its
// roi's geometry and writes both outputs of its element.  A batch index that does not truncate into [0, n) (or NaN) is
// handled as k_roi_align handles it: the element is 0, the second output -1 (roi_pool) or the input channel (the two
// position-sensitive ops), and nothing of x is read.
//
// Loops a roi can size: a pooling window is clamped to the map, at most h x w elements.  The adaptive grid of ps_roi_align
// (sampling_ratio <= 0) is ceil(roi size / pooled size) per axis and grows with the roi exactly as k_roi_align's does; it has no
// cap that roi_align does not have.
#include <cfloat>

#include "mv_common.h"

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

// the output element of a lane
struct Elem {
  int pw, ph, ch;  // ch: the OUTPUT channel
  const float* roi;
};

__device__ inline Elem elem_of(const RoiPoolArgs& A, long long idx) {
  Elem e;
  e.pw = (int)(idx % A.pooled_w);
  e.ph = (int)((idx / A.pooled_w) % A.pooled_h);
  const long long kc = idx / ((long long)A.pooled_w * A.pooled_h);
  e.ch = (int)(kc % A.c_out);
  e.roi = A.rois + (kc / A.c_out) * 5;
  return e;
}

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
  const Elem e = elem_of(A, idx);
  const float bf = e.roi[0];
  if (!(bf > -1.f && bf < (float)A.n)) {
    A.y[idx] = 0.f;
    A.second[idx] = -1;
    return;
  }
  const int b = (int)bf;
  const int start_w = rounded_corner(e.roi[1], A.spatial_scale), start_h = rounded_corner(e.roi[2], A.spatial_scale);
  const int end_w = rounded_corner(e.roi[3], A.spatial_scale), end_h = rounded_corner(e.roi[4], A.spatial_scale);
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
  const Elem e = elem_of(A, idx);
  const int c_in = (e.ch * A.pooled_h + e.ph) * A.pooled_w + e.pw;
  A.second[idx] = c_in;
  const float bf = e.roi[0];
  if (!(bf > -1.f && bf < (float)A.n)) {
    A.y[idx] = 0.f;
    return;
  }
  const int b = (int)bf;
  const int start_w = rounded_corner(e.roi[1], A.spatial_scale), start_h = rounded_corner(e.roi[2], A.spatial_scale);
  const int end_w = rounded_corner(e.roi[3], A.spatial_scale), end_h = rounded_corner(e.roi[4], A.spatial_scale);
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
  const Elem e = elem_of(A, idx);
  const int c_in = (e.ch * A.pooled_h + e.ph) * A.pooled_w + e.pw;
  A.second[idx] = c_in;
  const float bf = e.roi[0];
  if (!(bf > -1.f && bf < (float)A.n)) {
    A.y[idx] = 0.f;
    return;
  }
  const int b = (int)bf;
  // the half-pixel shift is always applied, and the roi's size is NOT clamped to 1
  const float start_w = __fsub_rn(__fmul_rn(e.roi[1], A.spatial_scale), .5f);
  const float start_h = __fsub_rn(__fmul_rn(e.roi[2], A.spatial_scale), .5f);
  const float end_w = __fsub_rn(__fmul_rn(e.roi[3], A.spatial_scale), .5f);
  const float end_h = __fsub_rn(__fmul_rn(e.roi[4], A.spatial_scale), .5f);
  const float roi_w = __fsub_rn(end_w, start_w), roi_h = __fsub_rn(end_h, start_h);
  const float bin_h = __fdiv_rn(roi_h, (float)A.pooled_h), bin_w = __fdiv_rn(roi_w, (float)A.pooled_w);
  const float base_y = __fadd_rn(__fmul_rn((float)e.ph, bin_h), start_h), base_x = __fadd_rn(__fmul_rn((float)e.pw, bin_w), start_w);
  const int grid_h = A.sampling_ratio > 0 ? A.sampling_ratio : (int)ceilf(__fdiv_rn(roi_h, (float)A.pooled_h));
  const int grid_w = A.sampling_ratio > 0 ? A.sampling_ratio : (int)ceilf(__fdiv_rn(roi_w, (float)A.pooled_w));
  const float count = (float)(grid_h * grid_w);  // not max(.., 1): an empty adaptive grid gives 0 / 0 = NaN, as the reference's loop
  const float* const plane = A.x + ((size_t)b * A.c + c_in) * ((size_t)A.h * A.w);
  const float fh = (float)A.h, fw = (float)A.w;
  float out = 0.f;
  // the sample of k_roi_align: 0 outside [-1, h] x [-1, w], clamped at 0, the high index collapsing onto the last row / column
  for (int iy = 0; iy < grid_h; ++iy) {
    float yy = __fadd_rn(base_y, __fdiv_rn(__fmul_rn(__fadd_rn((float)iy, .5f), bin_h), (float)grid_h));
    const bool y_out = yy < -1.f || yy > fh;
    if (y_out || yy <= 0.f) yy = 0.f;  // (an outside row's weights are not used)
    int y_low = (int)yy, y_high;
    if (y_low >= A.h - 1) {
      y_high = y_low = A.h - 1;
      yy = (float)y_low;
    } else {
      y_high = y_low + 1;
    }
    const float ly = __fsub_rn(yy, (float)y_low), hy = __fsub_rn(1.f, ly);
    for (int ix = 0; ix < grid_w; ++ix) {
      float xx = __fadd_rn(base_x, __fdiv_rn(__fmul_rn(__fadd_rn((float)ix, .5f), bin_w), (float)grid_w));
      float w1 = 0.f, w2 = 0.f, w3 = 0.f, w4 = 0.f;
      int p1 = 0, p2 = 0, p3 = 0, p4 = 0;  // an outside sample: zero weights on element 0
      if (!(y_out || xx < -1.f || xx > fw)) {
        if (xx <= 0.f) xx = 0.f;
        int x_low = (int)xx, x_high;
        if (x_low >= A.w - 1) {
          x_high = x_low = A.w - 1;
          xx = (float)x_low;
        } else {
          x_high = x_low + 1;
        }
        const float lx = __fsub_rn(xx, (float)x_low), hx = __fsub_rn(1.f, lx);
        w1 = __fmul_rn(hy, hx), w2 = __fmul_rn(hy, lx), w3 = __fmul_rn(ly, hx), w4 = __fmul_rn(ly, lx);
        p1 = y_low * A.w + x_low, p2 = y_low * A.w + x_high, p3 = y_high * A.w + x_low, p4 = y_high * A.w + x_high;
      }
      const float s = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w1, plane[p1]), __fmul_rn(w2, plane[p2])), __fmul_rn(w3, plane[p3])),
                                __fmul_rn(w4, plane[p4]));
      out = __fadd_rn(out, s);
    }
  }
  A.y[idx] = __fdiv_rn(out, count);
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
