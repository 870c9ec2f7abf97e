// retinanet.hip -- the inference half of torchvision's RetinaNet.postprocess_detections (models/detection/retinanet.py) up to the nms
// on gfx950.  Per image and level the reference applies a sigmoid to every (anchor, class) logit of a permuted copy, masks
// `> score_thresh`, torch.where, topk, divides and gathers, decodes and clips; here the selection runs on the head's own NCHW maps,
// spread over many workgroups, and only the selected candidates are decoded.
//
// A candidate is (anchor, class): logit channel a K + c at (y, x), flat index f = (start_l + (y W + x) A + a) K + c.  Its key is
// the 64-bit (score bits << 32 | ~f): scores are in [0, 1], so their bit patterns order as the scores do, and ~f puts the smaller
// flat index first among equal SCORES.  Keys of distinct candidates differ, so "the k greatest keys" is ONE set whatever the order
// in which the candidates are visited, and the stable descending order is the descending order of the keys.  A candidate that fails
// `score > thresh` (a NaN fails) has the key 0, which no passing candidate has (f < 2^31: ~f != 0).
//
// k_retinanet_chunks   stage 1, one workgroup per chunk of kRetChunk consecutive ELEMENTS of an (image, level) map, read in memory
//                      order (coalesced) and once: score, threshold, key, all in registers.  The chunk's own min(k, passing) greatest
//                      keys (select_keys below) are appended to the (image, level)'s pool in the workspace: one global atomicAdd per
//                      chunk reserves the room, so the pool's ORDER varies from run to run and its content does not.  A pool has room
//                      for min(k, kRetChunk) keys of every chunk: nothing is dropped, whatever passes.
// k_retinanet_rank     stage 2, one workgroup per (image, level): select_keys over the pool, the <= k <= 4096 selected keys into
//                      LDS, ranked pairwise there (position = #{greater keys}); idx[rank] = f, the rest of the segment -1
//                      (rank_selected of mv_topk.h, shared with k_ssd_topk).
// select_keys          (mv_topk.h, shared with ssd.hip) radix select of the k-th greatest key, 8 bits per pass from the top, a
//                      256-bin histogram in LDS per pass (hist_add of k_rpn_topk).  It stops as soon as the answer is known: after the first pass when at most k
//                      keys pass at all, after any pass when the bin of the k-th key is taken whole; at most 8 passes.
// k_retinanet_decode   one lane per idx[i, j]: anchor f / K and label f % K, the anchor in registers, decode_single, clip to the
//                      image (decode_candidate of mv_boxcoder.h, shared with k_rpn_decode), the score recomputed.  An index that
//                      is no candidate gets store_no_candidate's outputs, as in k_rpn_decode and k_ssd_decode.
//
// FCOS (models/detection/fcos.py postprocess_detections) is the same selection with another score, sqrt(sigmoid(cls) *
// sigmoid(centerness)), the centerness map read at the candidate's position: the chunk and rank kernels are instantiated with
// FCOS = true, where only candidate_key differs, and k_fcos_decode decodes with BoxLinearCoder's decode_linear.  It shares
// anchor_at (mv_boxcoder.h) with decode_candidate and keeps its own pick of the level's maps, clamp and not-a-candidate branch:
// with the shared helpers it compiles to other registers than before.
//
// Every float operation is written with __f*_rn and exp is the correctly rounded float32 exp, as in rpn.hip.
#include "mv_boxcoder.h"
#include "mv_common.h"
#include "mv_topk.h"

namespace mv {
namespace {

typedef unsigned long long u64;

constexpr int kRetThreads = 1024;
constexpr int kRetLoads = kRetChunk / kRetThreads;  // elements of a chunk per thread, in registers
constexpr int kRankLoads = 4;                       // pool keys a thread loads before it works on them
static_assert(kRetChunk % kRetThreads == 0, "a chunk is a whole number of elements per thread");

// The key of element e (memory order: channel a K + c, position pos) of a level's map with the logit x: 0 when it does not pass.
// FCOS: the score takes the centerness map's value at the same pos (one anchor per location: ctr has one channel).
template <bool FCOS>
__device__ inline u64 candidate_key(unsigned e, float x, const float* ctr, int hw, int A, int K, int level_start, float thresh) {
  const unsigned ch = e / (unsigned)hw, pos = e - ch * (unsigned)hw, a = ch / (unsigned)K, c = ch - a * (unsigned)K;
  const float s = FCOS ? fcos_score(x, ctr[pos]) : sigmoid_cr(x);
  const unsigned f = ((unsigned)level_start + pos * (unsigned)A + a) * (unsigned)K + c;
  return s > thresh ? ((u64)__float_as_uint(s) << 32) | (unsigned)~f : 0ull;
}

struct RetTopkArgs {
  const float* logits[kMaxRpnLevels];
  const float* ctr[kMaxRpnLevels];  // FCOS: the centerness maps (n, 1, h, w)
  long long img_stride[kMaxRpnLevels], ctr_stride[kMaxRpnLevels];
  int hw[kMaxRpnLevels], a[kMaxRpnLevels];
  int level_start[kMaxRpnLevels];   // anchors of the levels before
  int chunk_start[kMaxRpnLevels];   // first stage-1 block of the level
  long long pool_start[kMaxRpnLevels];  // first pool entry of the level within an image's pools
  int out_start[kMaxRpnLevels];     // position of the level's segment in a row of idx
  int seg[kMaxRpnLevels];           // min(k, a * hw * classes)
  int levels, classes, k, k_total;
  long long pool_per_image;
  float thresh;
  unsigned* counts;  // (n, levels): keys in the pool
  u64* pool;
  int* idx;
};

__global__ __launch_bounds__(256) void k_retinanet_zero(unsigned* __restrict__ counts, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) counts[i] = 0;
}

template <bool FCOS>
__global__ __launch_bounds__(kRetThreads) void k_retinanet_chunks(const RetTopkArgs T) {
  const int img = blockIdx.y;
  int level = 0;
#pragma unroll
  for (int l = 1; l < kMaxRpnLevels; ++l)
    if (l < T.levels && (int)blockIdx.x >= T.chunk_start[l]) level = l;
  const float* p = nullptr;
  const float* ctr = nullptr;
  long long img_stride = 0, pool_start = 0, ctr_stride = 0;
  int hw = 1, A = 1, level_start = 0, chunk_start = 0;
#pragma unroll
  for (int l = 0; l < kMaxRpnLevels; ++l)
    if (l == level) {
      p = T.logits[l], img_stride = T.img_stride[l], pool_start = T.pool_start[l], hw = T.hw[l], A = T.a[l], level_start = T.level_start[l],
      chunk_start = T.chunk_start[l];
      if (FCOS) ctr = T.ctr[l], ctr_stride = T.ctr_stride[l];
    }
  p += (size_t)img * img_stride;
  if (FCOS) ctr += (size_t)img * ctr_stride;
  const int K = T.classes;
  const long long nl = (long long)A * K * hw;  // < 2^31
  const long long base = (long long)((int)blockIdx.x - chunk_start) * kRetChunk;

  __shared__ unsigned hist[256];
  __shared__ unsigned sel[4];
  __shared__ unsigned n_out, room;
  const int tid = threadIdx.x, lane = tid & 63;

  float x[kRetLoads];
#pragma unroll
  for (int u = 0; u < kRetLoads; ++u) {
    const long long o = base + u * kRetThreads + tid;
    x[u] = o < nl ? p[o] : 0.f;
  }
  u64 key[kRetLoads];
#pragma unroll
  for (int u = 0; u < kRetLoads; ++u) {
    const long long o = base + u * kRetThreads + tid;
    key[u] = o < nl ? candidate_key<FCOS>((unsigned)o, x[u], ctr, hw, A, K, level_start, T.thresh) : 0ull;
  }

  unsigned take;
  const u64 thr = select_keys(
      [&](auto f) {
#pragma unroll
        for (int u = 0; u < kRetLoads; ++u) f(key[u]);
      },
      (unsigned)T.k, hist, sel, tid, lane, &take);
  if (take == 0) return;  // the same in every thread
  if (tid == 0) n_out = 0, room = atomicAdd(&T.counts[img * T.levels + level], take);
  __syncthreads();
  u64* const pool = T.pool + (size_t)img * T.pool_per_image + pool_start + room;
#pragma unroll
  for (int u = 0; u < kRetLoads; ++u)
    if (key[u] >= thr && key[u] != 0) {  // exactly `take` keys
      const unsigned slot = atomicAdd(&n_out, 1u);
      if (slot < take) pool[slot] = key[u];
    }
}

// DIRECT: the keys come from the level's map itself, computed anew in every pass, in place of the pool -- the whole (image, level)
// in ONE workgroup, without stage 1.  Instantiated in -DMV_TUNING builds only, for tools/perf_retinanet.py to measure what stage 1 buys.
// FCOS matters to the DIRECT form only: the pool holds keys, whatever made them.
template <bool DIRECT, bool FCOS = false>
__global__ __launch_bounds__(kRetThreads) void k_retinanet_rank(const RetTopkArgs T) {
  const int level = blockIdx.x, img = blockIdx.y;
  const float* p = nullptr;
  const float* ctr = nullptr;
  long long pool_start = 0, img_stride = 0, ctr_stride = 0;
  int out_start = 0, seg = 0, hw = 1, A = 1, level_start = 0;
#pragma unroll
  for (int l = 0; l < kMaxRpnLevels; ++l)
    if (l == level) {
      pool_start = T.pool_start[l], out_start = T.out_start[l], seg = T.seg[l], p = T.logits[l], img_stride = T.img_stride[l], hw = T.hw[l],
      A = T.a[l], level_start = T.level_start[l];
      if (FCOS) ctr = T.ctr[l], ctr_stride = T.ctr_stride[l];
    }
  const u64* const pool = T.pool + (size_t)img * T.pool_per_image + pool_start;
  p += (size_t)img * img_stride;
  if (FCOS) ctr += (size_t)img * ctr_stride;
  const int K = T.classes;
  const long long total = DIRECT ? (long long)A * K * hw : (long long)T.counts[img * T.levels + level];

  __shared__ unsigned hist[256];
  __shared__ unsigned sel[4];
  __shared__ unsigned n_out;
  __shared__ u64 cand[kRpnMaxK];
  const int tid = threadIdx.x, lane = tid & 63;

  const auto key_at = [&](long long i) -> u64 {
    if (i >= total) return 0ull;
    if (DIRECT) return candidate_key<FCOS>((unsigned)i, p[i], ctr, hw, A, K, level_start, T.thresh);
    return pool[i];
  };
  const auto each = [&](auto f) {
    for (long long b = 0; b < total; b += kRetThreads * kRankLoads) {
      u64 key[kRankLoads];
#pragma unroll
      for (int u = 0; u < kRankLoads; ++u) key[u] = key_at(b + u * kRetThreads + tid);
#pragma unroll
      for (int u = 0; u < kRankLoads; ++u) f(key[u]);
    }
  };
  unsigned take_u;
  const u64 thr = select_keys(each, (unsigned)T.k, hist, sel, tid, lane, &take_u);
  // every key >= thr is a candidate's, != 0, so rank_selected's `key != 0` selects the same set
  rank_selected<kRetThreads>(key_at, total, thr, take_u, cand, &n_out, T.idx + (size_t)img * T.k_total + out_start, seg,
                             [](u64 key) { return (int)~(unsigned)key; });
}

// amdgpu_waves_per_eu(8): left alone the compiler keeps the tables of all eight levels in 102 SGPRs, which leaves a SIMD 7 waves
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_retinanet_decode(const PyramidDecode P, long long* labels) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= P.count) return;
  if (!in_pyramid<0>(P, t)) return store_no_candidate(P.boxes, P.scores, labels, P.valid, t, 0);  // the -1 padding: nothing is read for it
  const Candidate c = decode_candidate<0>(P, t);
  for (int q = 0; q < 4; ++q) P.boxes[t * 4 + q] = c.box[q];
  P.scores[t] = sigmoid_cr(c.logit);
  labels[t] = c.label;
  P.valid[t] = 1;
}

// FCOS: PyramidDecode (one anchor per location, coef unused) and the centerness maps.  The score is fcos_score of the class logit and
// the centerness at the anchor's position, the box decode_linear of the anchor with the four distances, clipped to the image.
struct FcosDecode {
  PyramidDecode P;
  const float* ctr[kMaxRpnLevels];
  long long ctr_stride[kMaxRpnLevels];
};
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_fcos_decode(const FcosDecode F, long long* labels) {
  const PyramidDecode& P = F.P;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= P.count) return;
  if (!in_pyramid<0>(P, t)) {
    for (int q = 0; q < 4; ++q) P.boxes[t * 4 + q] = 0.f;
    P.scores[t] = 0.f, labels[t] = 0, P.valid[t] = 0;
    return;
  }
  const int K = P.classes;
  const long long img = t / P.k;
  const int f = P.idx[t];
  const int v = f / K, c = f - v * K;
  const AnchorAt an = anchor_at(P.lv, v);  // a = 0
  const float* lg = nullptr;
  const float* dl = nullptr;
  const float* ct = nullptr;
  long long ls = 0, ds = 0, cs = 0;
#pragma unroll
  for (int l = 0; l < kMaxRpnLevels; ++l)
    if (l == an.level) lg = P.logits[l], dl = P.deltas[l], ct = F.ctr[l], ls = P.logit_stride[l], ds = P.delta_stride[l], cs = F.ctr_stride[l];
  const size_t hw = an.hw;
  const float logit = lg[(size_t)img * ls + (size_t)c * hw + an.s];
  const float ctr = ct[(size_t)img * cs + an.s];
  const float* const d = dl + (size_t)img * ds + an.s;
  float box[4];
  decode_linear(an.x1, an.y1, an.x2, an.y2, d[0], d[hw], d[2 * hw], d[3 * hw], box);
  const float ih = P.image_sizes[img * 2], iw = P.image_sizes[img * 2 + 1];
  P.boxes[t * 4 + 0] = clamp0(box[0], iw), P.boxes[t * 4 + 1] = clamp0(box[1], ih);
  P.boxes[t * 4 + 2] = clamp0(box[2], iw), P.boxes[t * 4 + 3] = clamp0(box[3], ih);
  P.scores[t] = fcos_score(logit, ctr);
  labels[t] = c;
  P.valid[t] = 1;
}

}  // namespace

// The layout of the workspace of mv_retinanet_topk_f32: counts (n, levels) uint32 rounded up to 16 bytes, then per image the pools
// of its levels, chunks_l * min(k, kRetChunk) keys of 8 bytes each.
RetinanetPlan retinanet_plan(int64_t n, const int* hs, const int* ws, const int* as, int levels, int classes, int k) {
  RetinanetPlan p = {};
  const int64_t per_chunk = k < kRetChunk ? k : kRetChunk;
  for (int l = 0; l < levels; ++l) {
    const int64_t nl = (int64_t)as[l] * hs[l] * ws[l] * classes;
    p.chunks[l] = (nl + kRetChunk - 1) / kRetChunk;
    p.pool_start[l] = p.pool_per_image;
    p.pool_per_image += p.chunks[l] * per_chunk;
    p.total_chunks += p.chunks[l];
  }
  p.counts_bytes = (n * levels * 4 + 15) / 16 * 16;
  p.bytes = p.counts_bytes + n * p.pool_per_image * 8;
  return p;
}

template <bool FCOS>
static int launch_topk(const PyramidMaps& m, int classes, int n, int k, float score_thresh, int* idx, void* workspace, hipStream_t s) {
  const int *const hs = m.hs, *const ws = m.ws, *const as = m.as, levels = m.levels;
  const RetinanetPlan plan = retinanet_plan(n, hs, ws, as, levels, classes, k);
  RetTopkArgs t = {};
  int start = 0, out = 0, chunk = 0;
  for (int l = 0; l < levels; ++l) {
    const int64_t nl = (int64_t)as[l] * hs[l] * ws[l] * classes;
    t.logits[l] = m.logits[l], t.img_stride[l] = m.logit_strides[l], t.hw[l] = hs[l] * ws[l], t.a[l] = as[l];
    if (FCOS) t.ctr[l] = m.ctrness[l], t.ctr_stride[l] = m.ctr_strides[l];
    t.level_start[l] = start, t.chunk_start[l] = chunk, t.pool_start[l] = plan.pool_start[l], t.out_start[l] = out;
    t.seg[l] = nl < k ? (int)nl : k;
    start += as[l] * hs[l] * ws[l], out += t.seg[l], chunk += (int)plan.chunks[l];
  }
  t.levels = levels, t.classes = classes, t.k = k, t.k_total = out, t.pool_per_image = plan.pool_per_image, t.thresh = score_thresh;
  t.counts = static_cast<unsigned*>(workspace);
  t.pool = reinterpret_cast<u64*>(static_cast<char*>(workspace) + plan.counts_bytes);
  t.idx = idx;
#ifdef MV_TUNING
  if (tune_env("MV_RETINANET_ONE_WORKGROUP")) {  // tools/perf_retinanet.py: stage 2 alone, on the maps (not in the product library)
    hipLaunchKernelGGL((k_retinanet_rank<true, FCOS>), dim3(levels, n), dim3(kRetThreads), 0, s, t);
    return check_launchf("k_retinanet_rank<%sdirect,levels%d,k%d>", FCOS ? "fcos," : "", levels, k);
  }
#endif
  // a kernel rather than hipMemsetAsync: see k_zero_hist (autoaug.hip)
  hipLaunchKernelGGL(k_retinanet_zero, dim3((unsigned)((n * levels + 255) / 256)), dim3(256), 0, s, t.counts, n * levels);
  if (int rc = check_launch("k_retinanet_zero")) return rc;
  hipLaunchKernelGGL(k_retinanet_chunks<FCOS>, dim3((unsigned)plan.total_chunks, n), dim3(kRetThreads), 0, s, t);
  if (int rc = check_launchf("k_retinanet_chunks<%slevels%d,k%d>", FCOS ? "fcos," : "", levels, k)) return rc;
  hipLaunchKernelGGL(k_retinanet_rank<false>, dim3(levels, n), dim3(kRetThreads), 0, s, t);
  return check_launchf("k_retinanet_rank<%slevels%d,k%d>", FCOS ? "fcos," : "", levels, k);
}

int launch_retinanet_topk(const PyramidMaps& m, int classes, int n, int k, float score_thresh, int* idx, void* workspace, hipStream_t s) {
  return launch_topk<false>(m, classes, n, k, score_thresh, idx, workspace, s);
}
int launch_fcos_topk(const PyramidMaps& m, int classes, int n, int k, float score_thresh, int* idx, void* workspace, hipStream_t s) {
  return launch_topk<true>(m, classes, n, k, score_thresh, idx, workspace, s);
}

int launch_retinanet_decode(const PyramidMaps& m, int classes, const float* image_sizes, const int* idx, int64_t n, int64_t k,
                            const DecodeCoef& coef, float* boxes, float* scores, int64_t* labels, unsigned char* valid, hipStream_t s) {
  PyramidDecode p = {};
  fill_pyramid_decode(p, m, classes, image_sizes, idx, n, k, coef, boxes, scores, valid);
  hipLaunchKernelGGL(k_retinanet_decode, dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, s, p, reinterpret_cast<long long*>(labels));
  return check_launchf("k_retinanet_decode<levels%d>", m.levels);
}

int launch_fcos_decode(const PyramidMaps& m, int classes, const float* image_sizes, const int* idx, int64_t n, int64_t k, float* boxes,
                       float* scores, int64_t* labels, unsigned char* valid, hipStream_t s) {
  FcosDecode f = {};
  fill_pyramid_decode(f.P, m, classes, image_sizes, idx, n, k, DecodeCoef{}, boxes, scores, valid);
  for (int l = 0; l < m.levels; ++l) f.ctr[l] = m.ctrness[l], f.ctr_stride[l] = m.ctr_strides[l];
  hipLaunchKernelGGL(k_fcos_decode, dim3((unsigned)((f.P.count + 255) / 256)), dim3(256), 0, s, f, reinterpret_cast<long long*>(labels));
  return check_launchf("k_fcos_decode<levels%d>", m.levels);
}

}  // namespace mv
