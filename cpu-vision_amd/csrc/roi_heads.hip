// roi_heads.hip -- RoIHeads.postprocess_detections (models/detection/roi_heads.py) up to the per-image filters, on gfx950, in ONE
// launch.  The reference runs a softmax over the classes, BoxCoder.decode over every class, clip_boxes_to_image, three slices that drop
// the background column, three reshapes and three filter passes (score, small boxes) per image; here one wave64 owns one roi and
// writes the dense (R, C - 1) boxes / scores / labels with a validity flag, as k_rpn_decode does for the RPN.
//
// k_roi_detections  four waves per workgroup, one roi each; lanes stride over the classes.
//                     1. the row of logits goes to LDS, its maximum through a wave reduction (a NaN wins, as torch's max);
//                     2. e_j = E(x_j - m) per lane, in parallel: double precision, straight-line code, parked in LDS;
//                     3. s = ((e_0 + e_1) + e_2) + ... is ONE float32 chain in ascending class order (background included), run by
//                        every lane on the same LDS words (broadcast reads): the order is part of the stated numerics;
//                     4. class j >= 1 per lane: score e_j / s, decode_single of the roi with deltas 4 j .. 4 j + 3, the clamp to the
//                        roi's image, the flag.
//                   A roi whose image index is outside [0, n) reads nothing through it: zeros, valid 0.
//
// Every float operation is written with __f*_rn, as in rpn.hip; E is mv_boxcoder.h's correctly rounded float32 exp.
#include "mv_boxcoder.h"
#include "mv_common.h"

namespace mv {
namespace {

constexpr int kRoiWaves = 4;  // rois per workgroup

struct RoiDetArgs {
  const float* logits;
  const float* deltas;
  const float* rois;
  const float* image_sizes;
  long long logit_stride, delta_stride;  // elements between rows
  long long r, n;
  int classes;
  DecodeCoef coef;
  float score_thresh, min_size;
  float* boxes;
  float* scores;
  long long* labels;
  unsigned char* valid;
};

__global__ __launch_bounds__(kRoiWaves* kWave) void k_roi_detections(const RoiDetArgs A) {
  extern __shared__ float row_all[];  // kRoiWaves rows of `classes` floats: the logits, then the exponentials
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int C = A.classes;
  const long long r = (long long)blockIdx.x * kRoiWaves + wave;
  float* const row = row_all + (size_t)wave * C;

  // the roi and its image: uniform over the wave.  `live` rows compute; the others only keep the workgroup's barriers company
  bool live = r < A.r;
  float roi[4] = {0.f, 0.f, 0.f, 0.f};
  long long img = 0;
  if (live) {
    const float* const q = A.rois + r * 5;
    const float fi = q[0];
    if (fi > -1.f && fi < (float)A.n) img = (long long)fi;  // the conversion truncates: (-1, 0) is image 0
    else img = -1;                                        // a NaN index included
    if (img >= A.n) img = -1;                             // (float)n rounded up
    roi[0] = q[1], roi[1] = q[2], roi[2] = q[3], roi[3] = q[4];
  }
  const bool bad = live && img < 0;
  live = live && !bad;

  // 1. the logits into LDS, their maximum
  float m = -INFINITY;
  if (live) {
    const float* const x = A.logits + (size_t)r * A.logit_stride;
    for (int j = lane; j < C; j += kWave) {
      const float v = x[j];
      row[j] = v;
      m = nan_max(m, v);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = nan_max(m, __shfl_xor(m, d, kWave));
  // 2. the exponentials, each lane on the words it wrote
  if (live)
    for (int j = lane; j < C; j += kWave) row[j] = exp_cr(__fsub_rn(row[j], m));
  __syncthreads();
  // 3. the ascending chain, the same in every lane
  float s = 0.f;
  if (live) {
    s = row[0];
    for (int j = 1; j < C; ++j) s = __fadd_rn(s, row[j]);
  }

  // 4. the classes after the background
  const size_t out0 = (size_t)(r < A.r ? r : 0) * (size_t)(C - 1);
  if (bad) {
    for (int j = 1 + lane; j < C; j += kWave) {
      const size_t o = out0 + (size_t)(j - 1);
      for (int q = 0; q < 4; ++q) A.boxes[o * 4 + q] = 0.f;
      A.scores[o] = 0.f, A.labels[o] = 0, A.valid[o] = 0;
    }
    return;
  }
  if (!live) return;
  const float ih = A.image_sizes[img * 2], iw = A.image_sizes[img * 2 + 1];
  const float* const d = A.deltas + (size_t)r * A.delta_stride;
  for (int j = 1 + lane; j < C; j += kWave) {
    const size_t o = out0 + (size_t)(j - 1);
    const float score = __fdiv_rn(row[j], s);
    float box[4];
    decode_single(roi[0], roi[1], roi[2], roi[3], d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3], A.coef, box);
    box[0] = clamp0(box[0], iw), box[1] = clamp0(box[1], ih), box[2] = clamp0(box[2], iw), box[3] = clamp0(box[3], ih);
    const float bw = __fsub_rn(box[2], box[0]), bh = __fsub_rn(box[3], box[1]);
    for (int q = 0; q < 4; ++q) A.boxes[o * 4 + q] = box[q];
    A.scores[o] = score;
    A.labels[o] = j;
    A.valid[o] = (score > A.score_thresh && bw >= A.min_size && bh >= A.min_size) ? 1 : 0;
  }
}

}  // namespace

int launch_roi_detections(const float* logits, int64_t logit_stride, const float* deltas, int64_t delta_stride, const float* rois,
                          const float* image_sizes, int64_t r, int classes, int64_t n, const DecodeCoef& coef, float score_thresh, float min_size,
                          float* boxes, float* scores, int64_t* labels, unsigned char* valid, hipStream_t s) {
  RoiDetArgs a = {};
  a.logits = logits, a.deltas = deltas, a.rois = rois, a.image_sizes = image_sizes;
  a.logit_stride = logit_stride, a.delta_stride = delta_stride, a.r = r, a.n = n, a.classes = classes, a.coef = coef;
  a.score_thresh = score_thresh, a.min_size = min_size;
  a.boxes = boxes, a.scores = scores, a.labels = reinterpret_cast<long long*>(labels), a.valid = valid;
  const unsigned blocks = (unsigned)((r + kRoiWaves - 1) / kRoiWaves);
  const size_t lds = (size_t)kRoiWaves * classes * sizeof(float);  // <= 4 * kRoiMaxClasses * 4 = 32 KiB
  hipLaunchKernelGGL(k_roi_detections, dim3(blocks), dim3(kRoiWaves * kWave), lds, s, a);
  return check_launchf("k_roi_detections<classes%d>", classes);
}

}  // namespace mv
