// rpn.hip -- the inference half of torchvision's RegionProposalNetwork (models/detection/rpn.py filter_proposals up to the nms, with
// anchor_utils.py and _utils.py BoxCoder.decode_single folded in) on gfx950.  The reference materialises every anchor, permutes and
// concatenates every logit and delta, decodes every anchor and only then takes the top k per level; here the selection comes first,
// on the head's own NCHW maps, and only the selected candidates are decoded, each anchor built in registers.
//
// k_rpn_topk    one workgroup per (level, image).  The flat index of the reference's permuted layout is f = (y W + x) A + a, the
//               element sits at a H W + y W + x of the map; keys are the monotonic 32-bit image of the logit that k_nms_rank uses
//               (-0 == +0, every NaN the one greatest key).
//                 1. radix select: four passes of 8 bits from the top, a 256-bin histogram in LDS per pass (read in memory order,
//                    coalesced; a wave adds each distinct digit once) -> the k-th key T and how many keys are greater.
//                 2. compaction in ascending flat index: keys > T go to the candidate list in any order (an LDS counter), keys == T
//                    in flat order up to the count still missing (a ballot per wave, the wave totals through LDS, one barrier per
//                    1024 elements; a thread loads four elements ahead).  The candidates are (key << 32 | ~f), in the workspace.
//                 3. the <= k candidates are ranked pairwise, 1024 at a time through LDS, as k_nms_rank ranks scores: position =
//                    #{greater (key, ~f)}, which is the stable descending order; idx[rank] = level start + f.
// k_rpn_decode  one lane per selected candidate: (level, y, x, a) from the index, the logit and four deltas from the NCHW maps, the
//               anchor from the level's strides and base anchors, decode_single, clip to the image, sigmoid, the validity flag.
// k_box_decode  decode_single on explicit boxes (BoxCoder.decode), one lane per (box, class).
//
// Every float operation is written with __f*_rn: the reference is a chain of float32 torch ops, one rounding each, never an fma.
// exp is the CORRECTLY ROUNDED float32 exp, (float)exp((double)v): torch's CPU exp is a 1-ulp vector routine whose bits no other
// implementation reproduces, so the library states the one value that does not depend on an implementation.
#include "mv_boxcoder.h"
#include "mv_common.h"
#include "mv_topk.h"

namespace mv {
namespace {

typedef unsigned long long u64;

constexpr int kTopkThreads = 1024;
constexpr int kTopkWaves = kTopkThreads / kWave;
constexpr int kTopkLoads = 4;  // elements a thread loads before it works on them

// score_key of detect.hip, the high word: negative floats inverted, the sign bit set on the others, -0 as +0, NaN greatest
__device__ inline unsigned logit_key(float s) {
  const unsigned u = __float_as_uint(s);
  if (s != s) return 0xffffffffu;
  if (u == 0x80000000u) return 0x80000000u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct TopkArgs {
  const float* logits[kMaxRpnLevels];
  long long img_stride[kMaxRpnLevels];
  int hw[kMaxRpnLevels], a[kMaxRpnLevels];
  int level_start[kMaxRpnLevels];  // flat index of the level's first anchor in the concatenation
  int out_start[kMaxRpnLevels];    // position of the level's first candidate in a row of idx
  int take[kMaxRpnLevels];         // min(k, a * hw)
  int* idx;
  u64* cand;  // (n, k_total)
  int k_total;
};

__global__ __launch_bounds__(kTopkThreads) void k_rpn_topk(const TopkArgs T) {
  const int level = blockIdx.x, img = blockIdx.y;
  const float* p = nullptr;
  long long img_stride = 0;
  int hw = 0, A = 1, level_start = 0, out_start = 0, take = 0;
#pragma unroll
  for (int l = 0; l < kMaxRpnLevels; ++l)
    if (l == level)
      p = T.logits[l], img_stride = T.img_stride[l], hw = T.hw[l], A = T.a[l], level_start = T.level_start[l], out_start = T.out_start[l],
      take = T.take[l];
  p += (size_t)img * img_stride;
  const int nl = A * hw;

  __shared__ unsigned hist[256];
  __shared__ unsigned sel[2];
  __shared__ unsigned wave_cnt[2][kTopkWaves];
  __shared__ unsigned n_gt;
  __shared__ u64 tile[kTopkThreads];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  // 1. the k-th greatest key, 8 bits per pass
  unsigned prefix = 0, rem = (unsigned)take;  // rem: how many of the keys that share `prefix` are taken
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int base = 0; base < nl; base += kTopkThreads * kTopkLoads) {
      unsigned key[kTopkLoads];
      bool on[kTopkLoads];
#pragma unroll
      for (int u = 0; u < kTopkLoads; ++u) {
        const int o = base + u * kTopkThreads + tid;
        on[u] = o < nl;
        key[u] = on[u] ? logit_key(p[o]) : 0u;
      }
#pragma unroll
      for (int u = 0; u < kTopkLoads; ++u)
        hist_add(hist, on[u] && (pass == 0 || (key[u] >> (shift + 8)) == prefix), (key[u] >> shift) & 255u, lane);
    }
    __syncthreads();
    if (tid < 256) {
      unsigned above = 0;
      for (int j = tid + 1; j < 256; ++j) above += hist[j];
      if (above < rem && above + hist[tid] >= rem) sel[0] = (unsigned)tid, sel[1] = rem - above;  // exactly one digit
    }
    __syncthreads();
    prefix = (prefix << 8) | sel[0];
    rem = sel[1];
  }
  const unsigned thr = prefix, need_eq = rem, gt_total = (unsigned)take - rem;

  // 2. candidates: every key > thr, and the first need_eq keys == thr in ascending flat index
  u64* const cand = T.cand + (size_t)img * T.k_total + out_start;
  if (tid == 0) n_gt = 0;
  __syncthreads();
  unsigned eq_base = 0;
  int buf = 0;
  for (int base4 = 0; base4 < nl; base4 += kTopkThreads * kTopkLoads) {
    unsigned keys[kTopkLoads];
#pragma unroll
    for (int u = 0; u < kTopkLoads; ++u) {
      const int f = base4 + u * kTopkThreads + tid;
      keys[u] = f < nl ? logit_key(p[(size_t)(f % A) * hw + f / A]) : 0u;
    }
#pragma unroll
    for (int u = 0; u < kTopkLoads; ++u, buf ^= 1) {  // ascending flat index: step u is the 1024 elements from base4 + 1024 u
      const int f = base4 + u * kTopkThreads + tid;
      const bool on = f < nl;
      const unsigned key = keys[u];
      const bool gt = on && key > thr, eq = on && key == thr;
      const u64 m = __ballot(eq);
      if (lane == 0) wave_cnt[buf][wave] = (unsigned)__popcll(m);
      if (gt) {
        const unsigned slot = atomicAdd(&n_gt, 1u);
        if (slot < gt_total) cand[slot] = ((u64)key << 32) | (unsigned)~f;
      }
      __syncthreads();  // wave_cnt[buf] is next written two steps on, behind the barrier of the step between
      unsigned before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kTopkWaves; ++w) {
        const unsigned c = wave_cnt[buf][w];
        total += c;
        before += w < wave ? c : 0u;
      }
      if (eq) {
        const unsigned r = eq_base + before + (unsigned)__popcll(m & ((1ull << lane) - 1));
        if (r < need_eq) cand[gt_total + r] = ((u64)key << 32) | (unsigned)~f;
      }
      eq_base += total;
    }
  }

  // 3. the stable descending order of the `take` candidates (their keys are pairwise distinct and not 0)
  int* const out = T.idx + (size_t)img * T.k_total + out_start;
  for (int i0 = 0; i0 < take; i0 += kTopkThreads) {
    const int i = i0 + tid;
    u64 ki = ~0ull;
    int rank = 0;
    for (int j0 = 0; j0 < take; j0 += kTopkThreads) {
      __syncthreads();  // the first one also orders step 2's stores to cand before the loads below
      if (j0 == 0 && i < take) ki = cand[i];
      tile[tid] = j0 + tid < take ? cand[j0 + tid] : 0ull;
      __syncthreads();
      const int lim = min(kTopkThreads, take - j0);
      for (int t = 0; t < lim; ++t) rank += tile[t] > ki ? 1 : 0;
    }
    if (i < take) out[rank] = level_start + (int)~(unsigned)ki;
  }
}

// ---- the decode of a candidate: decode_candidate and store_no_candidate of mv_boxcoder.h (shared with retinanet.hip), one class ----
__global__ __launch_bounds__(256) void k_rpn_decode(const PyramidDecode P, long long* levels_out, float min_size, float score_thresh) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= P.count) return;
  if (!in_pyramid<1>(P, t)) return store_no_candidate(P.boxes, P.scores, levels_out, P.valid, t, -1);  // nothing is read for it
  const Candidate c = decode_candidate<1>(P, t);
  const float score = sigmoid_cr(c.logit);
  const float bw = __fsub_rn(c.box[2], c.box[0]), bh = __fsub_rn(c.box[3], c.box[1]);
  for (int q = 0; q < 4; ++q) P.boxes[t * 4 + q] = c.box[q];
  P.scores[t] = score;
  levels_out[t] = c.level;
  P.valid[t] = (bw >= min_size && bh >= min_size && score >= score_thresh) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_box_decode(const float* __restrict__ boxes, const float* __restrict__ codes, float* __restrict__ out,
                                                    long long count, int classes, const DecodeCoef K) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= count) return;
  const long long i = t / classes;
  const float* const b = boxes + i * 4;
  const float* const c = codes + t * 4;  // row i, columns 4 c .. 4 c + 3 of (m, 4 classes)
  float box[4];
  decode_single(b[0], b[1], b[2], b[3], c[0], c[1], c[2], c[3], K, box);
  for (int q = 0; q < 4; ++q) out[t * 4 + q] = box[q];
}

}  // namespace

int launch_rpn_topk(const PyramidMaps& m, int n, int k, int* idx, void* workspace, hipStream_t s) {
  TopkArgs t = {};
  int start = 0, out = 0;
  for (int l = 0; l < m.levels; ++l) {
    const int nl = m.as[l] * m.hs[l] * m.ws[l];
    t.logits[l] = m.logits[l], t.img_stride[l] = m.logit_strides[l], t.hw[l] = m.hs[l] * m.ws[l], t.a[l] = m.as[l];
    t.level_start[l] = start, t.out_start[l] = out, t.take[l] = nl < k ? nl : k;
    start += nl, out += t.take[l];
  }
  t.idx = idx, t.cand = static_cast<u64*>(workspace), t.k_total = out;
  hipLaunchKernelGGL(k_rpn_topk, dim3(m.levels, n), dim3(kTopkThreads), 0, s, t);
  return check_launchf("k_rpn_topk<levels%d,k%d>", m.levels, k);
}

int launch_rpn_decode(const PyramidMaps& m, const float* image_sizes, const int* idx, int64_t n, int64_t k, const DecodeCoef& coef, float min_size,
                      float score_thresh, float* boxes, float* scores, int64_t* levels_out, unsigned char* valid, hipStream_t s) {
  PyramidDecode p = {};
  fill_pyramid_decode(p, m, 1, image_sizes, idx, n, k, coef, boxes, scores, valid);
  hipLaunchKernelGGL(k_rpn_decode, dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, s, p, reinterpret_cast<long long*>(levels_out), min_size,
                     score_thresh);
  return check_launchf("k_rpn_decode<levels%d>", m.levels);
}

int launch_box_decode(const float* boxes, const float* rel_codes, float* out, int64_t m, int classes, const DecodeCoef& coef, hipStream_t s) {
  const long long count = (long long)m * classes;
  hipLaunchKernelGGL(k_box_decode, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, boxes, rel_codes, out, count, classes, coef);
  return check_launch("k_box_decode");
}

}  // namespace mv
