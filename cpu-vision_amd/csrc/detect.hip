// detect.hip -- torchvision.ops.nms and torchvision.ops.roi_align (forward) on gfx950, with the arithmetic of the reference's CPU
// kernels (csrc/ops/cpu/nms_kernel.cpp, roi_align_kernel.cpp + roi_align_common.h).  Every float operation below is written with
// __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn: one IEEE rounding each, never an fma, which is what those scalar loops compute.
//
// nms, three launches on one stream, nothing read back (workspace layout in NmsWorkspace):
//   k_nms_rank   the stable descending order of the scores without a sort: box i goes to position
//                #{j : s_j > s_i or (s_j == s_i and j < i)} (NaN counts as the greatest score, as torch.sort does).  n^2 comparisons,
//                which is what the mask phase costs anyway; the keys stream through LDS 1024 at a time.  Writes order[] and the boxes in
//                score order.
//   k_nms_mask   one wavefront per 64 x 64 tile (row tile r, column tile c >= r) of the sorted boxes: lane t owns row box 64 r + t and
//                sets bit j of its word when column box 64 c + j comes later in the order and IoU > threshold.  One uint64 per
//                (box, column tile); tiles below the diagonal are never written and never read.
//   k_nms_reduce one workgroup walks the row tiles in order with the "removed" bitset in LDS.  Per tile, wave 0 resolves the 64
//                boxes against each other in registers (lane t holds the diagonal word of box t; 64 uniform steps), emits the kept
//                indices at count + rank and publishes the kept mask; then every thread ORs the rows of the kept boxes into its
//                words of the bitset -- those loads do not depend on each other, unlike a walk box by box.
//
// roi_align: one lane per output element (k, c, ph, pw), pw fastest; the lane recomputes its roi's geometry (a few dozen flops)
// and sums its bin's samples (roi_align_element; the element index, the batch-index rule, the grid size and the sampling loop are
// mv_roi.h's, shared with roi_pool.hip).  k_multiscale_roi_align (ops/poolers.py MultiScaleRoIAlign) is the same element function
// on the feature map of the roi's level: one launch over all levels, no read-back.
#include "mv_common.h"
#include "mv_roi.h"

namespace mv {
namespace {

typedef unsigned long long u64;

constexpr int kRankBlock = 128;
constexpr int kRankTile = 1024;  // keys staged in LDS per step
constexpr int kReduceThreads = 1024;

// The stable descending order as ONE unsigned comparison: the score's bits made monotonic (negative floats inverted, the sign bit
// set on the others; -0 counts as +0 and every NaN as the single greatest key, which is how torch.sort compares) in the high
// word, ~index in the low word, so that of two equal scores the lower index has the greater key.
__device__ inline u64 score_key(float s, int i) {
  unsigned u = __float_as_uint(s);
  if (s != s) u = 0xffffffffu;
  else if (u == 0x80000000u) u = 0x80000000u;  // -0: its bits already are the key of +0 (0 | sign bit)
  else u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((u64)u << 32) | (unsigned)~i;
}

__global__ __launch_bounds__(kRankBlock) void k_nms_rank(const float* __restrict__ boxes, const float* __restrict__ scores, int n,
                                                         float* __restrict__ sorted, int* __restrict__ order) {
  __shared__ u64 tile[kRankTile];
  const int i = blockIdx.x * kRankBlock + threadIdx.x;
  const u64 ki = i < n ? score_key(scores[i], i) : 0ull;
  int rank = 0;  // keys greater than this box's: the boxes in front of it
  for (int j0 = 0; j0 < n; j0 += kRankTile) {
    __syncthreads();
    for (int t = threadIdx.x; t < kRankTile; t += kRankBlock) tile[t] = j0 + t < n ? score_key(scores[j0 + t], j0 + t) : 0ull;
    __syncthreads();
#pragma unroll 8
    for (int t = 0; t < kRankTile; ++t) rank += tile[t] > ki ? 1 : 0;  // a padding key of 0 is greater than no box's key
  }
  if (i >= n) return;
  order[rank] = i;  // a permutation: every slot of order[] and sorted[] is written exactly once
  for (int q = 0; q < 4; ++q) sorted[(size_t)rank * 4 + q] = boxes[(size_t)i * 4 + q];
}

// std::max / std::min as the reference's scalar code evaluates them (which operand a NaN or a signed zero yields)
__device__ inline float ref_max(float a, float b) { return a < b ? b : a; }
__device__ inline float ref_min(float a, float b) { return b < a ? b : a; }

__global__ __launch_bounds__(kWave) void k_nms_mask(const float* __restrict__ sorted, int n, int tiles, double thr,
                                                    u64* __restrict__ mask) {
  const int r = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
  if (c < r) return;
  __shared__ float col[kWave][4];
  __shared__ float col_area[kWave];
  const int cj = c * kWave + t;
  if (cj < n) {
    const float x1 = sorted[(size_t)cj * 4], y1 = sorted[(size_t)cj * 4 + 1], x2 = sorted[(size_t)cj * 4 + 2], y2 = sorted[(size_t)cj * 4 + 3];
    col[t][0] = x1, col[t][1] = y1, col[t][2] = x2, col[t][3] = y2;
    col_area[t] = __fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1));
  }
  __syncthreads();
  const int i = r * kWave + t;
  if (i >= n) return;
  const float ix1 = sorted[(size_t)i * 4], iy1 = sorted[(size_t)i * 4 + 1], ix2 = sorted[(size_t)i * 4 + 2], iy2 = sorted[(size_t)i * 4 + 3];
  const float iarea = __fmul_rn(__fsub_rn(ix2, ix1), __fsub_rn(iy2, iy1));
  const int cols = min(kWave, n - c * kWave);
  u64 word = 0;
  for (int j = (c == r ? t + 1 : 0); j < cols; ++j) {
    const float xx1 = ref_max(ix1, col[j][0]), yy1 = ref_max(iy1, col[j][1]);
    const float xx2 = ref_min(ix2, col[j][2]), yy2 = ref_min(iy2, col[j][3]);
    const float w = ref_max(0.f, __fsub_rn(xx2, xx1)), h = ref_max(0.f, __fsub_rn(yy2, yy1));
    const float inter = __fmul_rn(w, h);
    const float ovr = __fdiv_rn(inter, __fsub_rn(__fadd_rn(iarea, col_area[j]), inter));
    if ((double)ovr > thr) word |= 1ull << j;  // the reference compares its float with the double threshold
  }
  mask[(size_t)i * tiles + c] = word;
}

__device__ inline u64 uniform64(u64 v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((u64)hi << 32) | lo;
}

__global__ __launch_bounds__(kReduceThreads) void k_nms_reduce(const u64* __restrict__ mask, const int* __restrict__ order, int n,
                                                               int tiles, long long* __restrict__ keep, long long* __restrict__ keep_count) {
  extern __shared__ u64 removed[];  // tiles words, then the kept mask of the tile in hand
  u64* const kept_slot = removed + tiles;
  const int tid = threadIdx.x;
  for (int w = tid; w < tiles; w += kReduceThreads) removed[w] = 0;
  long long count = 0;  // wave 0's running total (uniform)
  __syncthreads();
  for (int r = 0; r < tiles; ++r) {
    if (tid < kWave) {
      const int i = r * kWave + tid;
      const int valid_n = min(kWave, n - r * kWave);
      const u64 diag = i < n ? mask[(size_t)i * tiles + r] : 0ull;
      u64 rem = uniform64(removed[r]) | (valid_n < kWave ? ~0ull << valid_n : 0ull);
#pragma unroll
      for (int t = 0; t < kWave; ++t) {
        const u64 d = ((u64)(unsigned)__builtin_amdgcn_readlane((int)(diag >> 32), t) << 32) |
                      (unsigned)__builtin_amdgcn_readlane((int)diag, t);
        if (!((rem >> t) & 1)) rem |= d;  // box t is kept: it removes the later boxes of its diagonal word
      }
      const u64 kept = ~rem;  // bit t of rem was final before step t: the diagonal words only hold later bits
      if ((kept >> tid) & 1) keep[count + __popcll(kept & ((1ull << tid) - 1))] = order[i];
      count += __popcll(kept);
      if (tid == 0) *kept_slot = kept;
    }
    __syncthreads();
    const u64 kept = uniform64(*kept_slot);
    if (kept) {
      for (int w = r + 1 + tid; w < tiles; w += kReduceThreads) {
        const u64* const rows = mask + (size_t)r * kWave * tiles + w;
        u64 acc = removed[w], m = kept;
        while (m) {  // four independent loads in flight per step
          u64 v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            v[u] = 0;
            if (m) {
              v[u] = rows[(size_t)__builtin_ctzll(m) * tiles];
              m &= m - 1;
            }
          }
          acc |= (v[0] | v[1]) | (v[2] | v[3]);
        }
        removed[w] = acc;
      }
    }
    __syncthreads();
  }
  if (tid == 0) *keep_count = count;
}

struct RoiAlignArgs {
  const float* x;
  const float* rois;
  float* y;
  long long total;  // k * c * pooled_h * pooled_w
  int n, c, h, w, pooled_h, pooled_w, sampling_ratio, aligned;
  float spatial_scale;
};

// Output element idx of roi_align on the map A.x (A.h x A.w, A.spatial_scale): k_roi_align hands over its arguments as they are,
// k_multiscale_roi_align the map of the roi's level.
__device__ inline void roi_align_element(const RoiAlignArgs& A, long long idx) {
  const RoiElem e = roi_elem(idx, A.pooled_h, A.pooled_w, A.c);
  const float* const roi = A.rois + e.k * 5;
  int b;
  if (!roi_image(roi[0], A.n, &b)) {
    A.y[idx] = 0.f;
    return;
  }
  const float offset = A.aligned ? 0.5f : 0.f;
  const float start_w = __fsub_rn(__fmul_rn(roi[1], A.spatial_scale), offset);
  const float start_h = __fsub_rn(__fmul_rn(roi[2], A.spatial_scale), offset);
  const float end_w = __fsub_rn(__fmul_rn(roi[3], A.spatial_scale), offset);
  const float end_h = __fsub_rn(__fmul_rn(roi[4], A.spatial_scale), offset);
  float roi_w = __fsub_rn(end_w, start_w), roi_h = __fsub_rn(end_h, start_h);
  if (!A.aligned) roi_w = ref_max(roi_w, 1.f), roi_h = ref_max(roi_h, 1.f);
  const float bin_h = __fdiv_rn(roi_h, (float)A.pooled_h), bin_w = __fdiv_rn(roi_w, (float)A.pooled_w);
  const int grid_h = roi_grid(A.sampling_ratio, roi_h, A.pooled_h), grid_w = roi_grid(A.sampling_ratio, roi_w, A.pooled_w);
  const float count = (float)max(grid_h * grid_w, 1);  // an empty adaptive grid: 0 / 1 = 0
  const float* const plane = A.x + ((size_t)b * A.c + e.ch) * ((size_t)A.h * A.w);
  const float base_y = __fadd_rn(start_h, __fmul_rn((float)e.ph, bin_h)), base_x = __fadd_rn(start_w, __fmul_rn((float)e.pw, bin_w));
  A.y[idx] = __fdiv_rn(roi_bin_sum(plane, A.h, A.w, base_y, base_x, bin_h, bin_w, grid_h, grid_w), count);
}

__global__ __launch_bounds__(256) void k_roi_align(const RoiAlignArgs A) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= A.total) return;
  roi_align_element(A, idx);
}

// MultiScaleRoIAlign in one launch: the per-level maps travel by value (host tables copied into the arguments); a lane reads its
// roi's level, picks that level's map with a chain of selects (no indexed access to the argument arrays, which would move them to
// scratch) and computes roi_align_element on it.  A level outside [0, levels): zeros, nothing is read.
struct MultiScaleArgs {
  const float* xs[kMaxRoiLevels];
  int hs[kMaxRoiLevels], ws[kMaxRoiLevels];
  float scales[kMaxRoiLevels];
  const long long* roi_levels;
  int levels;
  RoiAlignArgs roi;  // x, h, w and spatial_scale are set per lane
};

__global__ __launch_bounds__(256) void k_multiscale_roi_align(const MultiScaleArgs M) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M.roi.total) return;
  const long long level = M.roi_levels[roi_elem(idx, M.roi.pooled_h, M.roi.pooled_w, M.roi.c).k];
  if (level < 0 || level >= M.levels) {
    M.roi.y[idx] = 0.f;
    return;
  }
  RoiAlignArgs A = M.roi;
#pragma unroll
  for (int l = 0; l < kMaxRoiLevels; ++l)
    if (l == (int)level) A.x = M.xs[l], A.h = M.hs[l], A.w = M.ws[l], A.spatial_scale = M.scales[l];
  roi_align_element(A, idx);
}

}  // namespace

// ---- nms workspace: [sorted boxes: n x 4 float][mask: n x tiles uint64][order: n int32], rounded up to 16 bytes ----------------
struct NmsWorkspace {
  float* sorted;
  u64* mask;
  int* order;
};

static NmsWorkspace nms_carve(void* ws, int64_t n) {
  const int64_t tiles = (n + kWave - 1) / kWave;
  char* p = static_cast<char*>(ws);
  NmsWorkspace w;
  w.sorted = reinterpret_cast<float*>(p);
  w.mask = reinterpret_cast<u64*>(p + 16 * n);
  w.order = reinterpret_cast<int*>(p + 16 * n + 8 * n * tiles);
  return w;
}

int64_t nms_workspace_bytes(int64_t n) {
  const int64_t tiles = (n + kWave - 1) / kWave;
  return (16 * n + 8 * n * tiles + 4 * n + 15) / 16 * 16;
}

int launch_nms(const float* boxes, const float* scores, int n, double iou_threshold, int64_t* keep, int64_t* keep_count, void* workspace,
               hipStream_t s) {
  const NmsWorkspace w = nms_carve(workspace, n);
  const int tiles = (n + kWave - 1) / kWave;
  hipLaunchKernelGGL(k_nms_rank, dim3((n + kRankBlock - 1) / kRankBlock), dim3(kRankBlock), 0, s, boxes, scores, n, w.sorted, w.order);
  if (int rc = check_launch("k_nms_rank")) return rc;
  hipLaunchKernelGGL(k_nms_mask, dim3(tiles, tiles), dim3(kWave), 0, s, w.sorted, n, tiles, iou_threshold, w.mask);
  if (int rc = check_launch("k_nms_mask")) return rc;
  hipLaunchKernelGGL(k_nms_reduce, dim3(1), dim3(kReduceThreads), (size_t)(tiles + 1) * sizeof(u64), s, w.mask, w.order, n, tiles,
                     reinterpret_cast<long long*>(keep), reinterpret_cast<long long*>(keep_count));
  return check_launchf("k_nms_rank+k_nms_mask<64x64>+k_nms_reduce<tiles%d>", tiles);
}

int launch_roi_align(const float* x, const float* rois, float* y, int n, int c, int h, int w, int64_t k, int pooled_h, int pooled_w,
                     float spatial_scale, int sampling_ratio, int aligned, hipStream_t s) {
  RoiAlignArgs a = {x, rois, y, (long long)k * c * pooled_h * pooled_w, n, c, h, w, pooled_h, pooled_w, sampling_ratio, aligned, spatial_scale};
  hipLaunchKernelGGL(k_roi_align, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, s, a);
  return check_launchf("k_roi_align<%s,%s>", aligned ? "aligned" : "legacy", sampling_ratio > 0 ? "fixed" : "adaptive");
}

int launch_multiscale_roi_align(const float* const* xs, const int* hs, const int* ws, const double* scales, int levels, const float* rois,
                                const int64_t* roi_levels, float* y, int n, int c, int64_t k, int pooled_h, int pooled_w, int sampling_ratio,
                                int aligned, hipStream_t s) {
  MultiScaleArgs m = {};
  for (int l = 0; l < levels; ++l) m.xs[l] = xs[l], m.hs[l] = hs[l], m.ws[l] = ws[l], m.scales[l] = (float)scales[l];
  m.roi_levels = reinterpret_cast<const long long*>(roi_levels);
  m.levels = levels;
  m.roi = {nullptr, rois, y, (long long)k * c * pooled_h * pooled_w, n, c, 0, 0, pooled_h, pooled_w, sampling_ratio, aligned, 0.f};
  hipLaunchKernelGGL(k_multiscale_roi_align, dim3((unsigned)((m.roi.total + 255) / 256)), dim3(256), 0, s, m);
  return check_launchf("k_multiscale_roi_align<levels%d,%s,%s>", levels, aligned ? "aligned" : "legacy",
                       sampling_ratio > 0 ? "fixed" : "adaptive");
}

}  // namespace mv
