// mv_bilinear.h -- one axis of torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=False) as a device
// function, shared by interp.hip (k_interp_batch), mask.hip (k_paste_masks) and segment.hip (k_interp_argmax, which also takes the
// blend of the four taps from here); the formula is stated in mi355vision.h, mv_interpolate_bilinear_f32.
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

// the three-step blend of the four taps a, b (top row, x0 and x1) and c, d (bottom row): every product and every fma rounded once
__device__ inline float bilinear_blend(const BilinearTap& ty, const BilinearTap& tx, float a, float b, float c, float d) {
  const float top = __fmaf_rn(tx.w0, a, __fmul_rn(tx.w1, b));
  const float bot = __fmaf_rn(tx.w0, c, __fmul_rn(tx.w1, d));
  return __fmaf_rn(ty.w0, top, __fmul_rn(ty.w1, bot));
}

}  // namespace mv
