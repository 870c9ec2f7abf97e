// mv_boxcoder.h -- BoxCoder.decode_single (_utils.py) as one device function, shared by rpn.hip (k_rpn_decode, k_box_decode),
// roi_heads.hip (k_roi_detections) and retinanet.hip (k_retinanet_decode); the anchor of a flat index, built in registers from the
// level tables (anchor_at), and the sigmoid (sigmoid_cr), shared by k_rpn_decode and k_retinanet_decode.  Every float operation is written with __f*_rn: the reference is a chain of float32 torch ops,
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

// 1 / (1 + E(-x)), every operation rounded once to float32, the division correctly rounded
__device__ inline float sigmoid_cr(float x) { return __fdiv_rn(1.f, __fadd_rn(1.f, exp_cr(-x))); }

// The pyramid of an anchor generator, by value in the kernel arguments (kMaxRpnLevels entries, `levels` used).
struct AnchorLevels {
  int h[kMaxRpnLevels], w[kMaxRpnLevels], a[kMaxRpnLevels];
  int start[kMaxRpnLevels];     // flat index of the level's first anchor
  int base_off[kMaxRpnLevels];  // row of the level's first base anchor
  int stride_h[kMaxRpnLevels], stride_w[kMaxRpnLevels];
  int levels, total;            // total: anchors of all levels
  const float* base_anchors;
};
inline void fill_anchor_levels(AnchorLevels& t, const int* hs, const int* ws, const int* as, const int* strides_h, const int* strides_w,
                               int levels, const float* base_anchors) {
  int start = 0, base = 0;
  for (int l = 0; l < levels; ++l) {
    t.h[l] = hs[l], t.w[l] = ws[l], t.a[l] = as[l], t.start[l] = start, t.base_off[l] = base;
    t.stride_h[l] = strides_h[l], t.stride_w[l] = strides_w[l];
    start += as[l] * hs[l] * ws[l], base += as[l];
  }
  t.levels = levels, t.total = start, t.base_anchors = base_anchors;
}

// Anchor v (0 <= v < T.total) of the concatenated (y, x, a) layout: its level, its anchor a and position s = y W + x in the level's
// map of hw = H W elements, and the box (x sw + b[a][0], y sh + b[a][1], x sw + b[a][2], y sh + b[a][3]).
struct AnchorAt {
  int level, a, s;
  size_t hw;
  float x1, y1, x2, y2;
};
__device__ inline AnchorAt anchor_at(const AnchorLevels& T, int v) {
  int level = 0;
#pragma unroll
  for (int l = 1; l < kMaxRpnLevels; ++l)
    if (l < T.levels && v >= T.start[l]) level = l;
  int H = 1, W = 1, A = 1, start = 0, base_off = 0, sh = 0, sw = 0;
#pragma unroll
  for (int l = 0; l < kMaxRpnLevels; ++l)
    if (l == level)
      H = T.h[l], W = T.w[l], A = T.a[l], start = T.start[l], base_off = T.base_off[l], sh = T.stride_h[l], sw = T.stride_w[l];
  const int flat = v - start, a = flat % A, s = flat / A, y = s / W, x = s % W;
  const float* const b = T.base_anchors + (size_t)(base_off + a) * 4;
  const float fx = (float)(x * sw), fy = (float)(y * sh);  // the reference's int32 shifts, converted as its int + float add does
  return {level, a, s, (size_t)H * W, __fadd_rn(fx, b[0]), __fadd_rn(fy, b[1]), __fadd_rn(fx, b[2]), __fadd_rn(fy, b[3])};
}

}  // namespace mv
