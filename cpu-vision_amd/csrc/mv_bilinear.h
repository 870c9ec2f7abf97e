// mv_bilinear.h -- one axis of torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=False) as a device
// function, shared by interp.hip (k_interp_batch) and mask.hip (k_paste_masks); the formula is stated in mi355vision.h,
// mv_interpolate_bilinear_f32.
#pragma once

#include "mv_common.h"

namespace mv {

// source index pair and weights of output index d: src = max(fma(s, d + 0.5, -0.5), 0), s = float32(in) / float32(out)
struct BilinearTap {
  int i0, i1;
  float w0, w1;
};
__device__ inline BilinearTap bilinear_tap(int d, float s, int in) {
  const float src = fmaxf(__fmaf_rn(s, (float)d + 0.5f, -0.5f), 0.f);
  BilinearTap t;
  t.i0 = min((int)src, in - 1);  // src >= 0: the conversion truncates to the floor
  t.i1 = min(t.i0 + 1, in - 1);
  t.w1 = fminf(fmaxf(__fsub_rn(src, (float)t.i0), 0.f), 1.f);
  t.w0 = __fsub_rn(1.f, t.w1);
  return t;
}

}  // namespace mv
