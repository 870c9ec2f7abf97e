// mv_roi.h -- what the five RoI kernels share, as device functions: detect.hip (k_roi_align, k_multiscale_roi_align) and
// roi_pool.hip (k_roi_pool, k_ps_roi_pool, k_ps_roi_align).  Every float operation is one __f*_rn intrinsic, one IEEE rounding
// each and never an fma: the results are bit-equal to the reference's CPU kernels, so this arithmetic exists here and nowhere
// else.
#pragma once

#include "mv_common.h"

namespace mv {

// Output element idx of a (K, channels, pooled_h, pooled_w) tensor, pw fastest.
struct RoiElem {
  int pw, ph, ch;  // ch: the OUTPUT channel
  long long k;     // the roi: row k of rois[K, 5]
};

__device__ inline RoiElem roi_elem(long long idx, int pooled_h, int pooled_w, int channels) {
  RoiElem e;
  e.pw = (int)(idx % pooled_w);
  e.ph = (int)((idx / pooled_w) % pooled_h);
  const long long kc = idx / ((long long)pooled_w * pooled_h);
  e.ch = (int)(kc % channels);
  e.k = kc / channels;
  return e;
}

// The image a roi names: false when its batch index bf does not truncate into [0, n) (or is NaN) -- the kernels then write zeros
// and read nothing of x -- else true and the index in *b.
__device__ inline bool roi_image(float bf, int n, int* b) {
  if (!(bf > -1.f && bf < (float)n)) return false;
  *b = (int)bf;
  return true;
}

// Samples per bin along one axis: sampling_ratio if positive, else ceil(roi size / pooled size), which grows with the roi.
__device__ inline int roi_grid(int sampling_ratio, float roi_size, int pooled) {
  return sampling_ratio > 0 ? sampling_ratio : (int)ceilf(__fdiv_rn(roi_size, (float)pooled));
}

// The rounded sum of the grid_h x grid_w bilinear samples of one bin of `plane` (h x w), in ascending (iy, ix) order; sample
// (iy, ix) lies at (base_y + (iy + .5) bin_h / grid_h, base_x + (ix + .5) bin_w / grid_w).  A sample outside [-1, h] x [-1, w]
// is 0; inside, a coordinate is clamped at 0 and the high index collapses onto the last row / column.  The caller divides by its
// own count.
__device__ inline float roi_bin_sum(const float* plane, int h, int w, float base_y, float base_x, float bin_h, float bin_w, int grid_h,
                                    int grid_w) {
  const float fh = (float)h, fw = (float)w;
  float out = 0.f;
  for (int iy = 0; iy < grid_h; ++iy) {
    float yy = __fadd_rn(base_y, __fdiv_rn(__fmul_rn(__fadd_rn((float)iy, .5f), bin_h), (float)grid_h));
    const bool y_out = yy < -1.f || yy > fh;
    if (y_out || yy <= 0.f) yy = 0.f;  // (an outside row's weights are not used)
    int y_low = (int)yy, y_high;
    if (y_low >= h - 1) {
      y_high = y_low = h - 1;
      yy = (float)y_low;
    } else {
      y_high = y_low + 1;
    }
    const float ly = __fsub_rn(yy, (float)y_low), hy = __fsub_rn(1.f, ly);
    for (int ix = 0; ix < grid_w; ++ix) {
      float xx = __fadd_rn(base_x, __fdiv_rn(__fmul_rn(__fadd_rn((float)ix, .5f), bin_w), (float)grid_w));
      float w1 = 0.f, w2 = 0.f, w3 = 0.f, w4 = 0.f;
      int p1 = 0, p2 = 0, p3 = 0, p4 = 0;  // an outside sample: zero weights on element 0, as the reference's pre_calc does
      if (!(y_out || xx < -1.f || xx > fw)) {
        if (xx <= 0.f) xx = 0.f;
        int x_low = (int)xx, x_high;
        if (x_low >= w - 1) {
          x_high = x_low = w - 1;
          xx = (float)x_low;
        } else {
          x_high = x_low + 1;
        }
        const float lx = __fsub_rn(xx, (float)x_low), hx = __fsub_rn(1.f, lx);
        w1 = __fmul_rn(hy, hx), w2 = __fmul_rn(hy, lx), w3 = __fmul_rn(ly, hx), w4 = __fmul_rn(ly, lx);
        p1 = y_low * w + x_low, p2 = y_low * w + x_high, p3 = y_high * w + x_low, p4 = y_high * w + x_high;
      }
      const float s = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w1, plane[p1]), __fmul_rn(w2, plane[p2])), __fmul_rn(w3, plane[p3])),
                                __fmul_rn(w4, plane[p4]));
      out = __fadd_rn(out, s);
    }
  }
  return out;
}

}  // namespace mv
