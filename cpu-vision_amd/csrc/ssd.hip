// ssd.hip -- the inference half of torchvision's SSD.postprocess_detections (models/detection/ssd.py) up to the nms on gfx950.  Per
// image the reference takes a softmax over the K classes of every one of V anchors, decodes and clips all V boxes, and then loops
// over the labels 1 .. K - 1: mask `> score_thresh`, topk(min(k, count)), gather -- K - 1 rounds with a read-back each.  Here:
//
// k_ssd_scores   ONE launch for all levels and images, one thread per anchor v = start_l + (y W + x) A + a of the reference's
//                concatenated layout: the K logits of channel a K + c at (y, x) are read where they lie, in the head's NCHW maps,
//                and the softmax goes to the CLASS-MAJOR matrix scores[i][c][v].  Consecutive lanes are consecutive v, so every
//                store of a wave is 64 consecutive floats of a row; its loads are A runs of 64 / A consecutive positions of A
//                channel planes.  Three passes over the K classes: the maximum (a NaN wins, as torch's max); e_j = E(x_j - m),
//                parked in scores[i][j][v] -- the thread's own word -- and summed as ONE chain in ascending class order, in
//                FLOAT64 (S += (double)e_j): a float32 chain of 91 terms is measurably less accurate than torch's softmax
//                (DESIGN 3.31), so the sum follows the GroupNorm / L2-norm precedent; p_j = (float)((double)e_j / S) over the
//                parked words.  Maximum and exponentials are k_roi_detections' (roi_heads.hip).
// k_ssd_topk     one workgroup per (image, class >= 1) walks its contiguous row of V scores: key (score bits << 32 | ~v), 0 when
//                `score > thresh` fails (a NaN fails); select_keys (mv_topk.h) picks the k greatest, which go to LDS and are ranked
//                pairwise there (rank_selected, shared with k_retinanet_rank); idx[i][(c - 1) k + rank] = v K + c, the rest -1.  Keys of
//                distinct anchors differ, so the result is one set in one order whatever the order of the visits; nothing is read
//                back and no atomic touches global memory.
// k_ssd_decode   one lane per idx[i, j]: anchor f / K and label f % K, the default box built in registers (DefaultBoxGenerator's
//                float32 chain, anchor_utils.py), decode_single with delta channels 4 a .. 4 a + 3, the clamp to the image, the score
//                read from the matrix.  The level tables and the (level, a, position) of an anchor are PyramidLevels / level_at of
//                mv_boxcoder.h (k_ssd_scores too), the outputs of the padding its store_no_candidate.
//
// Every float operation is written with __f*_rn and exp is the correctly rounded float32 exp, as in rpn.hip.
#include "mv_boxcoder.h"
#include "mv_common.h"
#include "mv_topk.h"

namespace mv {
namespace {

typedef unsigned long long u64;

constexpr int kSsdTopkThreads = 1024;
constexpr int kSsdTopkLoads = 4;  // scores a thread loads before it works on them

struct SsdScoresArgs {
  const float* logits[kMaxRpnLevels];
  long long img_stride[kMaxRpnLevels];
  PyramidLevels lv;
  int classes;
  float* scores;  // (n, classes, total)
};

__global__ __launch_bounds__(256) void k_ssd_scores(const SsdScoresArgs S) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= S.lv.total) return;
  const int img = blockIdx.y, K = S.classes;
  const LevelAt at = level_at(S.lv, (int)v);
  const float* p = nullptr;
  long long stride = 0;
#pragma unroll
  for (int l = 0; l < kMaxRpnLevels; ++l)
    if (l == at.level) p = S.logits[l], stride = S.img_stride[l];
  const size_t hw = at.hw;
  const float* const x = p + (size_t)img * stride + (size_t)at.a * K * hw + at.s;  // class c at x[c hw]
  float* const out = S.scores + (size_t)img * K * S.lv.total + v;                  // class c at out[c total]
  const size_t V = (size_t)S.lv.total;

  float m = x[0];
  for (int c = 1; c < K; ++c) m = nan_max(m, x[c * hw]);
  double s = 0.0;
  for (int c = 0; c < K; ++c) {
    const float e = exp_cr(__fsub_rn(x[c * hw], m));
    out[c * V] = e;
    s = __dadd_rn(s, (double)e);
  }
  for (int c = 0; c < K; ++c) out[c * V] = __double2float_rn(__ddiv_rn((double)out[c * V], s));
}

struct SsdTopkArgs {
  const float* scores;  // (n, classes, v)
  int classes, v, k;
  float thresh;
  int* idx;  // (n, (classes - 1) k)
};

__global__ __launch_bounds__(kSsdTopkThreads) void k_ssd_topk(const SsdTopkArgs T) {
  const int c = blockIdx.x + 1, img = blockIdx.y, K = T.classes;
  const float* const row = T.scores + ((size_t)img * K + c) * (size_t)T.v;
  const int total = T.v;

  __shared__ unsigned hist[256];
  __shared__ unsigned sel[4];
  __shared__ unsigned n_out;
  __shared__ u64 cand[kRpnMaxK];
  const int tid = threadIdx.x, lane = tid & 63;

  const auto key_at = [&](int i) -> u64 {
    if (i >= total) return 0ull;
    const float s = row[i];
    return s > T.thresh ? ((u64)__float_as_uint(s) << 32) | (unsigned)~(unsigned)i : 0ull;
  };
  const auto each = [&](auto f) {
    // no overflow: v <= 2^30, as v classes < 2^31 with classes >= 2 (checked at the entry)
    for (int b = 0; b < total; b += kSsdTopkThreads * kSsdTopkLoads) {
      u64 key[kSsdTopkLoads];
#pragma unroll
      for (int u = 0; u < kSsdTopkLoads; ++u) key[u] = key_at(b + u * kSsdTopkThreads + tid);
#pragma unroll
      for (int u = 0; u < kSsdTopkLoads; ++u) f(key[u]);
    }
  };
  unsigned take_u;
  const u64 thr = select_keys(each, (unsigned)T.k, hist, sel, tid, lane, &take_u);
  rank_selected<kSsdTopkThreads>(key_at, total, thr, take_u, cand, &n_out, T.idx + ((size_t)img * (K - 1) + (c - 1)) * (size_t)T.k, T.k,
                                 [&](u64 key) { return (int)(~(unsigned)key) * K + c; });
}

struct SsdDecodeArgs {
  const float* scores;  // (n, classes, total)
  const float* deltas[kMaxRpnLevels];
  long long delta_stride[kMaxRpnLevels];
  PyramidLevels lv;
  int pair_off[kMaxRpnLevels];              // row of the level's first (w, h) pair
  float x_f[kMaxRpnLevels], y_f[kMaxRpnLevels];
  float img_w, img_h;                       // the batch tensor's sides
  const float* wh_pairs;                    // (sum of a, 2), clamped already where the generator clips
  int classes;
  const float* image_sizes;
  const int* idx;
  long long count, k;
  DecodeCoef coef;
  float* boxes;
  float* scores_out;
  long long* labels;
  unsigned char* valid;
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_ssd_decode(const SsdDecodeArgs D) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= D.count) return;
  const int K = D.classes;
  const int f = D.idx[t];
  // not a candidate of this pyramid (the -1 padding): nothing is read for it
  if (f < 0 || f / K >= D.lv.total) return store_no_candidate(D.boxes, D.scores_out, D.labels, D.valid, t, 0);
  const long long img = t / D.k;
  const int v = f / K, c = f - v * K;
  const LevelAt at = level_at(D.lv, v);
  const float* dl = nullptr;
  long long ds = 0;
  int pair_off = 0;
  float x_f = 1.f, y_f = 1.f;
#pragma unroll
  for (int l = 0; l < kMaxRpnLevels; ++l)
    if (l == at.level) dl = D.deltas[l], ds = D.delta_stride[l], pair_off = D.pair_off[l], x_f = D.x_f[l], y_f = D.y_f[l];
  // the default box: DefaultBoxGenerator's float32 chain
  const int y = at.s / at.W, x = at.s - y * at.W;
  const float cx = __fdiv_rn(__fadd_rn((float)x, 0.5f), x_f), cy = __fdiv_rn(__fadd_rn((float)y, 0.5f), y_f);
  const float* const wh = D.wh_pairs + (size_t)(pair_off + at.a) * 2;
  const float hw_ = __fmul_rn(0.5f, wh[0]), hh_ = __fmul_rn(0.5f, wh[1]);
  const float x1 = __fmul_rn(__fsub_rn(cx, hw_), D.img_w), y1 = __fmul_rn(__fsub_rn(cy, hh_), D.img_h);
  const float x2 = __fmul_rn(__fadd_rn(cx, hw_), D.img_w), y2 = __fmul_rn(__fadd_rn(cy, hh_), D.img_h);
  const size_t hw = at.hw;
  const float* const d = dl + (size_t)img * ds + (size_t)(4 * at.a) * hw + at.s;
  float box[4];
  decode_single(x1, y1, x2, y2, d[0], d[hw], d[2 * hw], d[3 * hw], D.coef, box);
  const float ih = D.image_sizes[img * 2], iw = D.image_sizes[img * 2 + 1];
  D.boxes[t * 4 + 0] = clamp0(box[0], iw), D.boxes[t * 4 + 1] = clamp0(box[1], ih);
  D.boxes[t * 4 + 2] = clamp0(box[2], iw), D.boxes[t * 4 + 3] = clamp0(box[3], ih);
  D.scores_out[t] = D.scores[((size_t)img * K + c) * (size_t)D.lv.total + v];
  D.labels[t] = c;
  D.valid[t] = 1;
}

}  // namespace

int launch_ssd_scores(const PyramidMaps& m, int classes, int n, float* scores, hipStream_t s) {
  SsdScoresArgs a = {};
  for (int l = 0; l < m.levels; ++l) a.logits[l] = m.logits[l], a.img_stride[l] = m.logit_strides[l];
  fill_pyramid_levels(a.lv, m);
  a.classes = classes, a.scores = scores;
  hipLaunchKernelGGL(k_ssd_scores, dim3((unsigned)((a.lv.total + 255) / 256), n), dim3(256), 0, s, a);
  return check_launchf("k_ssd_scores<levels%d,classes%d>", m.levels, classes);
}

int launch_ssd_topk(const float* scores, int n, int classes, int v, int k, float score_thresh, int* idx, hipStream_t s) {
  const SsdTopkArgs t = {scores, classes, v, k, score_thresh, idx};
  hipLaunchKernelGGL(k_ssd_topk, dim3(classes - 1, n), dim3(kSsdTopkThreads), 0, s, t);
  return check_launchf("k_ssd_topk<classes%d,k%d>", classes, k);
}

int launch_ssd_decode(const float* scores, const PyramidMaps& m, int classes, const float* wh_pairs, const float* x_f, const float* y_f,
                      int batch_h, int batch_w, const float* image_sizes, const int* idx, int64_t n, int64_t k, const DecodeCoef& coef,
                      float* boxes, float* scores_out, int64_t* labels, unsigned char* valid, hipStream_t s) {
  SsdDecodeArgs d = {};
  d.scores = scores;
  int pairs = 0;
  for (int l = 0; l < m.levels; ++l) {
    d.deltas[l] = m.deltas[l], d.delta_stride[l] = m.delta_strides[l], d.pair_off[l] = pairs, d.x_f[l] = x_f[l], d.y_f[l] = y_f[l];
    pairs += m.as[l];
  }
  fill_pyramid_levels(d.lv, m);
  d.img_w = (float)batch_w, d.img_h = (float)batch_h, d.wh_pairs = wh_pairs, d.classes = classes, d.image_sizes = image_sizes, d.idx = idx;
  d.count = n * k, d.k = k, d.coef = coef, d.boxes = boxes, d.scores_out = scores_out, d.labels = reinterpret_cast<long long*>(labels);
  d.valid = valid;
  hipLaunchKernelGGL(k_ssd_decode, dim3((unsigned)((d.count + 255) / 256)), dim3(256), 0, s, d);
  return check_launchf("k_ssd_decode<levels%d>", m.levels);
}

}  // namespace mv
