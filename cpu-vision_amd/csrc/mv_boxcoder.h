// mv_boxcoder.h -- BoxCoder.decode_single (_utils.py) as one device function, shared by rpn.hip (k_rpn_decode, k_box_decode) and
// roi_heads.hip (k_roi_detections).  Every float operation is written with __f*_rn: the reference is a chain of float32 torch ops,
// one rounding each, never an fma.  exp is the CORRECTLY ROUNDED float32 exp, (float)exp((double)v): torch's CPU exp is a 1-ulp
// vector routine whose bits no other implementation reproduces, so the library states the one value that does not depend on an
// implementation (mi355vision.h, mv_rpn_decode_f32).
#pragma once

#include "mv_common.h"

namespace mv {

struct DecodeCoef {
  float wx, wy, ww, wh, clip;
};

__device__ inline float exp_cr(float v) { return (float)exp((double)v); }

// One box (x1, y1, x2, y2) and its four codes -> the decoded box, operation by operation as the reference's float32 tensor ops.
__device__ inline void decode_single(float x1, float y1, float x2, float y2, float c0, float c1, float c2, float c3, const DecodeCoef& K,
                                     float (&out)[4]) {
  const float widths = __fsub_rn(x2, x1), heights = __fsub_rn(y2, y1);
  const float ctr_x = __fadd_rn(x1, __fmul_rn(0.5f, widths)), ctr_y = __fadd_rn(y1, __fmul_rn(0.5f, heights));
  const float dx = __fdiv_rn(c0, K.wx), dy = __fdiv_rn(c1, K.wy);
  float dw = __fdiv_rn(c2, K.ww), dh = __fdiv_rn(c3, K.wh);
  dw = dw > K.clip ? K.clip : dw;  // torch.clamp(max=): a NaN stays
  dh = dh > K.clip ? K.clip : dh;
  const float pcx = __fadd_rn(__fmul_rn(dx, widths), ctr_x), pcy = __fadd_rn(__fmul_rn(dy, heights), ctr_y);
  const float pw = __fmul_rn(exp_cr(dw), widths), ph = __fmul_rn(exp_cr(dh), heights);
  const float half_w = __fmul_rn(0.5f, pw), half_h = __fmul_rn(0.5f, ph);
  out[0] = __fsub_rn(pcx, half_w), out[1] = __fsub_rn(pcy, half_h), out[2] = __fadd_rn(pcx, half_w), out[3] = __fadd_rn(pcy, half_h);
}

// torch.clamp(v, min=0, max=hi): a NaN stays
__device__ inline float clamp0(float v, float hi) { return v != v ? v : (v < 0.f ? 0.f : (v > hi ? hi : v)); }

}  // namespace mv
