// mv_boxcoder.h -- BoxCoder.decode_single (_utils.py) as one device function, shared by rpn.hip (k_rpn_decode, k_box_decode),
// roi_heads.hip (k_roi_detections), retinanet.hip (k_retinanet_decode) and ssd.hip (k_ssd_decode); the level, anchor and position of
// a flat index from the level tables (PyramidLevels, level_at: k_ssd_scores, k_ssd_decode) and, with an anchor generator's tables,
// the anchor built in registers (AnchorLevels, anchor_at: decode_candidate, k_fcos_decode); the sigmoid (sigmoid_cr); the decode of
// one candidate of a pyramid (PyramidDecode, decode_candidate: k_rpn_decode, k_retinanet_decode); the outputs of an index that is no
// candidate (store_no_candidate: k_rpn_decode, k_retinanet_decode, k_ssd_decode).  Every float operation is written with __f*_rn:
// the reference is a chain of float32 torch ops, one rounding each, never an fma.  exp is the CORRECTLY ROUNDED float32 exp,
// (float)exp((double)v): torch's CPU exp is a 1-ulp vector routine whose bits no other implementation reproduces, so the library
// states the one value that does not depend on an implementation (mi355vision.h, mv_rpn_decode_f32).
#pragma once

#include "mv_common.h"

namespace mv {

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

// torch.max over a row: any NaN makes the result NaN
__device__ inline float nan_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// 1 / (1 + E(-x)), every operation rounded once to float32, the division correctly rounded
__device__ inline float sigmoid_cr(float x) { return __fdiv_rn(1.f, __fadd_rn(1.f, exp_cr(-x))); }

// The correctly rounded float32 square root, through float64 as exp_cr (53 >= 2 * 24 + 2 bits: the second rounding is innocuous).
// __fsqrt_rn is the native 1-ulp instruction unless the headers are built with rounded operations.
__device__ inline float sqrt_cr(float v) { return (float)__builtin_sqrt((double)v); }

// FCOS's score of a candidate (fcos.py postprocess_detections): sqrt(sigmoid(cls) * sigmoid(centerness)), each operation rounded once
__device__ inline float fcos_score(float cls, float ctr) { return sqrt_cr(__fmul_rn(sigmoid_cr(cls), sigmoid_cr(ctr))); }

// BoxLinearCoder(normalize_by_size=True).decode (_utils.py) of one anchor with the four distances r (left, top, right, bottom in
// units of the anchor's sides): linear in the anchor's size, no exp.  max(r, 0) first -- the head's ReLU, the same bits on a map
// that is rectified already (a NaN stays).
__device__ inline void decode_linear(float x1, float y1, float x2, float y2, float r0, float r1, float r2, float r3, float (&out)[4]) {
  r0 = r0 < 0.f ? 0.f : r0, r1 = r1 < 0.f ? 0.f : r1, r2 = r2 < 0.f ? 0.f : r2, r3 = r3 < 0.f ? 0.f : r3;
  const float ctr_x = __fmul_rn(0.5f, __fadd_rn(x1, x2)), ctr_y = __fmul_rn(0.5f, __fadd_rn(y1, y2));
  const float w = __fsub_rn(x2, x1), h = __fsub_rn(y2, y1);
  out[0] = __fsub_rn(ctr_x, __fmul_rn(r0, w)), out[1] = __fsub_rn(ctr_y, __fmul_rn(r1, h));
  out[2] = __fadd_rn(ctr_x, __fmul_rn(r2, w)), out[3] = __fadd_rn(ctr_y, __fmul_rn(r3, h));
}

// The levels of a pyramid, by value in the kernel arguments (kMaxRpnLevels entries, `levels` used): what a kernel needs to find the
// level, the anchor and the position of a flat index.  ssd.hip's kernels take this alone (their boxes come from other tables, and
// tables a kernel does not read still cost it SGPRs); AnchorLevels adds an anchor generator's base anchors and strides.
struct PyramidLevels {
  int h[kMaxRpnLevels], w[kMaxRpnLevels], a[kMaxRpnLevels];
  int start[kMaxRpnLevels];  // flat index of the level's first anchor
  int levels, total;         // total: anchors of all levels
};
struct AnchorLevels {
  PyramidLevels py;
  int base_off[kMaxRpnLevels];  // row of the level's first base anchor
  int stride_h[kMaxRpnLevels], stride_w[kMaxRpnLevels];
  const float* base_anchors;
};
inline void fill_pyramid_levels(PyramidLevels& t, const PyramidMaps& m) {
  int start = 0;
  for (int l = 0; l < m.levels; ++l) {
    t.h[l] = m.hs[l], t.w[l] = m.ws[l], t.a[l] = m.as[l], t.start[l] = start;
    start += m.as[l] * m.hs[l] * m.ws[l];
  }
  t.levels = m.levels, t.total = start;
}
inline void fill_anchor_levels(AnchorLevels& t, const PyramidMaps& m) {
  fill_pyramid_levels(t.py, m);
  int base = 0;
  for (int l = 0; l < m.levels; ++l) {
    t.base_off[l] = base, t.stride_h[l] = m.strides_h[l], t.stride_w[l] = m.strides_w[l];
    base += m.as[l];
  }
  t.base_anchors = m.base_anchors;
}

// What k_rpn_decode, k_retinanet_decode and k_fcos_decode take alike, by value in the kernel arguments: the head's maps (logit
// channel a * classes + c, delta channels 4 a .. 4 a + 3 of anchor a), the pyramid, the n * k candidates and the outputs all write.
struct PyramidDecode {
  const float* logits[kMaxRpnLevels];
  const float* deltas[kMaxRpnLevels];
  long long logit_stride[kMaxRpnLevels], delta_stride[kMaxRpnLevels];
  AnchorLevels lv;
  int classes;  // the rpn: 1
  const float* image_sizes;
  const int* idx;
  long long count, k;  // n * k candidates
  DecodeCoef coef;
  float* boxes;
  float* scores;
  unsigned char* valid;
};
inline void fill_pyramid_decode(PyramidDecode& p, const PyramidMaps& m, int classes, const float* image_sizes, const int* idx, int64_t n,
                                int64_t k, const DecodeCoef& coef, float* boxes, float* scores, unsigned char* valid) {
  for (int l = 0; l < m.levels; ++l)
    p.logits[l] = m.logits[l], p.deltas[l] = m.deltas[l], p.logit_stride[l] = m.logit_strides[l], p.delta_stride[l] = m.delta_strides[l];
  fill_anchor_levels(p.lv, m);
  p.classes = classes, p.image_sizes = image_sizes, p.idx = idx, p.count = n * k, p.k = k, p.coef = coef;
  p.boxes = boxes, p.scores = scores, p.valid = valid;
}

// Anchor v (0 <= v < T.total) of the concatenated (y, x, a) layout: its level, its anchor a and position s = y W + x in the level's
// map of width W and hw = H W elements.  more(l): the caller's own picks from tables of level l, in the same pass over the levels
// -- anchor_at's: picked in a second pass they cost k_rpn_decode 8 more SGPRs (106) and left a SIMD 7 waves for 8.
struct LevelAt {
  int level, a, s, W;
  size_t hw;
};
template <typename More>
__device__ inline LevelAt level_at(const PyramidLevels& T, int v, const More& more) {
  int level = 0;
#pragma unroll
  for (int l = 1; l < kMaxRpnLevels; ++l)
    if (l < T.levels && v >= T.start[l]) level = l;
  int H = 1, W = 1, A = 1, start = 0;
#pragma unroll
  for (int l = 0; l < kMaxRpnLevels; ++l)
    if (l == level) H = T.h[l], W = T.w[l], A = T.a[l], start = T.start[l], more(l);
  const int flat = v - start;
  return {level, flat % A, flat / A, W, (size_t)H * W};
}
__device__ inline LevelAt level_at(const PyramidLevels& T, int v) {
  return level_at(T, v, [](int) {});
}

// level_at, and the anchor's box (x sw + b[a][0], y sh + b[a][1], x sw + b[a][2], y sh + b[a][3]).
struct AnchorAt {
  int level, a, s;
  size_t hw;
  float x1, y1, x2, y2;
};
__device__ inline AnchorAt anchor_at(const AnchorLevels& T, int v) {
  int base_off = 0, sh = 0, sw = 0;
  const LevelAt at = level_at(T.py, v, [&](int l) { base_off = T.base_off[l], sh = T.stride_h[l], sw = T.stride_w[l]; });
  const int y = at.s / at.W, x = at.s % at.W;
  const float* const b = T.base_anchors + (size_t)(base_off + at.a) * 4;
  const float fx = (float)(x * sw), fy = (float)(y * sh);  // the reference's int32 shifts, converted as its int + float add does
  return {at.level, at.a, at.s, at.hw, __fadd_rn(fx, b[0]), __fadd_rn(fy, b[1]), __fadd_rn(fx, b[2]), __fadd_rn(fy, b[3])};
}

// What a decode kernel writes at t for an index that is no candidate of its pyramid: zeros, `fill` in the int64 output, valid = 0
// (k_fcos_decode writes the same itself: see there).
__device__ inline void store_no_candidate(float* boxes, float* scores, long long* out64, unsigned char* valid, long long t, long long fill) {
  for (int q = 0; q < 4; ++q) boxes[t * 4 + q] = 0.f;
  scores[t] = 0.f, out64[t] = fill, valid[t] = 0;
}

// Candidate t of P (0 <= t < P.count), flat index f = P.idx[t] = anchor * classes + class.  in_pyramid: f is a candidate of this
// pyramid (f >= 0 and its anchor not past the last); a kernel reads nothing but the index for one that is not.  decode_candidate,
// for one that is: its level, its class, its logit and decode_single of its anchor with its four deltas, clipped to its image.
// CLASSES: the class count where the kernel knows it (the rpn's 1: no division is left), 0 = P.classes.
struct Candidate {
  int level, label;
  float logit, box[4];
};
template <int CLASSES>
__device__ inline bool in_pyramid(const PyramidDecode& P, long long t) {
  const int K = CLASSES ? CLASSES : P.classes;
  const int f = P.idx[t];
  return f >= 0 && f / K < P.lv.py.total;
}
template <int CLASSES>
__device__ inline Candidate decode_candidate(const PyramidDecode& P, long long t) {
  Candidate out;
  const int K = CLASSES ? CLASSES : P.classes;
  const long long img = t / P.k;
  const int f = P.idx[t];
  const int v = f / K, c = f - v * K;
  const AnchorAt an = anchor_at(P.lv, v);
  const float* lg = nullptr;
  const float* dl = nullptr;
  long long ls = 0, ds = 0;
#pragma unroll
  for (int l = 0; l < kMaxRpnLevels; ++l)
    if (l == an.level) lg = P.logits[l], dl = P.deltas[l], ls = P.logit_stride[l], ds = P.delta_stride[l];
  const size_t hw = an.hw;
  out.level = an.level, out.label = c;
  out.logit = lg[(size_t)img * ls + ((size_t)an.a * K + c) * hw + an.s];
  const float* const d = dl + (size_t)img * ds + (size_t)(4 * an.a) * hw + an.s;
  decode_single(an.x1, an.y1, an.x2, an.y2, d[0], d[hw], d[2 * hw], d[3 * hw], P.coef, out.box);
  const float ih = P.image_sizes[img * 2], iw = P.image_sizes[img * 2 + 1];
  out.box[0] = clamp0(out.box[0], iw), out.box[1] = clamp0(out.box[1], ih);
  out.box[2] = clamp0(out.box[2], iw), out.box[3] = clamp0(out.box[3], ih);
  return out;
}

}  // namespace mv
