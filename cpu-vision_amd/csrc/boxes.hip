// boxes.hip -- torchvision.ops.box_iou / generalized_box_iou / distance_box_iou and masks_to_boxes on gfx950 (ops/boxes.py of the
// reference, which is Python over broadcast torch ops).  The float arithmetic is that chain of torch ops evaluated in float32: every
// difference, product, sum and quotient below is one __fsub_rn / __fmul_rn / __fadd_rn / __fdiv_rn (one IEEE rounding, never an
// fma), and min / max / clamp propagate NaN as torch.min / torch.max / torch.clamp do.
//
// k_box_iou<mode, vec>: the op writes 4 bytes per pair and reads next to nothing, so it is laid out for its stores.  A wave owns
//   kIouCols = 256 columns (4 per lane) and holds its four boxes2 rows, their areas and (distance) centres in registers while it
//   walks kIouWaveRows rows; the 4 waves of a workgroup take consecutive row groups of one kIouStrip-row strip.  A row's boxes1
//   values are wave-uniform (scalar loads), so a row costs each lane 4 results and
//     vec     one 16-byte store of columns 4 lane .. 4 lane + 3: 1 KB contiguous per wave (m % 4 == 0 and out 16-byte aligned);
//     scalar  four 4-byte stores of columns lane, lane + 64, lane + 128, lane + 192: 256 contiguous bytes per wave each (any m,
//             any alignment).  Same arithmetic per pair.
//   row * m is a 64-bit product.
//
// masks_to_boxes, three launches on one stream, nothing read back by the library:
//   k_mtb_init    4 ints per mask in the workspace: [INT_MAX, INT_MAX, -1, -1] (min x, min y, max x, max y)
//   k_mtb_reduce  one workgroup per (mask, chunk of kMtbChunkRows rows); a wave takes a row at a time: the elements before the
//                 first 16-byte boundary one per lane, then 16-byte loads, then the remainder one per lane, so any w and any
//                 alignment are read correctly.  Lane -> wave -> workgroup reduction, then four integer atomicMin / atomicMax per
//                 workgroup that found a set element: order cannot change a min or a max.
//   k_mtb_final   per mask: the ints as float32 into boxes; an empty mask writes zeros and ORs 1 into *empty_flag.
#include <climits>

#include "mv_common.h"

namespace mv {
namespace {

constexpr int kIouBlock = 256;                              // 4 waves
constexpr int kIouCols = 256;                               // columns of one tile: 4 per lane
constexpr int kIouWaveRows = 32;                            // rows a wave walks with its columns in registers
constexpr int kIouStrip = 128;                              // rows of one workgroup: its 4 waves take kIouWaveRows each
static_assert(kIouStrip == kIouWaveRows * (kIouBlock / kWave) && kIouCols == 4 * kWave, "a strip is the waves' row groups");

// torch.max / torch.min / clamp(min=0) on floats: a NaN operand gives NaN
__device__ inline float t_max(float a, float b) { return (b != b || a < b) ? b : a; }
__device__ inline float t_min(float a, float b) { return (b != b || b < a) ? b : a; }
__device__ inline float clamp0(float v) { return v < 0.f ? 0.f : v; }

struct Box {
  float x1, y1, x2, y2;
};

template <int MODE>
__device__ inline float pair_value(const Box a, float a_area, float a_cx, float a_cy, const Box b, float b_area, float b_cx, float b_cy) {
  const float w = clamp0(__fsub_rn(t_min(a.x2, b.x2), t_max(a.x1, b.x1)));
  const float h = clamp0(__fsub_rn(t_min(a.y2, b.y2), t_max(a.y1, b.y1)));
  const float inter = __fmul_rn(w, h);
  const float uni = __fsub_rn(__fadd_rn(a_area, b_area), inter);
  const float iou = __fdiv_rn(inter, uni);
  if (MODE == 0) return iou;
  const float wi = clamp0(__fsub_rn(t_max(a.x2, b.x2), t_min(a.x1, b.x1)));  // the smallest enclosing box
  const float hi = clamp0(__fsub_rn(t_max(a.y2, b.y2), t_min(a.y1, b.y1)));
  if (MODE == 1) {
    const float areai = __fmul_rn(wi, hi);
    return __fsub_rn(iou, __fdiv_rn(__fsub_rn(areai, uni), areai));
  }
  const float diag = __fadd_rn(__fadd_rn(__fmul_rn(wi, wi), __fmul_rn(hi, hi)), 1e-7f);
  const float dx = __fsub_rn(a_cx, b_cx), dy = __fsub_rn(a_cy, b_cy);
  return __fsub_rn(iou, __fdiv_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), diag));
}

__device__ inline float box_area(const Box b) { return __fmul_rn(__fsub_rn(b.x2, b.x1), __fsub_rn(b.y2, b.y1)); }
__device__ inline float half_sum(float p, float q) { return __fmul_rn(__fadd_rn(p, q), 0.5f); }  // (p + q) / 2: halving is exact

template <int MODE, bool VEC>
__global__ __launch_bounds__(kIouBlock) void k_box_iou(const float* __restrict__ boxes1, const float* __restrict__ boxes2,
                                                       float* __restrict__ out, long long n, long long m, unsigned col_tiles) {
  const unsigned tile = blockIdx.x % col_tiles, strip = blockIdx.x / col_tiles;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  long long col[4];
  Box b[4];
  float b_area[4], b_cx[4], b_cy[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    col[q] = (long long)tile * kIouCols + (VEC ? lane * 4 + q : q * kWave + lane);
    b[q] = Box{0.f, 0.f, 0.f, 0.f};  // a column past m: computed on zeros, never stored
    if (col[q] < m) {
      const float* const p = boxes2 + col[q] * 4;
      b[q] = Box{p[0], p[1], p[2], p[3]};
    }
    b_area[q] = box_area(b[q]);
    b_cx[q] = half_sum(b[q].x1, b[q].x2), b_cy[q] = half_sum(b[q].y1, b[q].y2);
  }
  const long long row0 = (long long)strip * kIouStrip + (long long)wave * kIouWaveRows;
  const long long row1 = row0 + kIouWaveRows < n ? row0 + kIouWaveRows : n;
  for (long long row = row0; row < row1; ++row) {
    const float* const p = boxes1 + row * 4;  // wave-uniform
    const Box a = {p[0], p[1], p[2], p[3]};
    const float a_area = box_area(a), a_cx = half_sum(a.x1, a.x2), a_cy = half_sum(a.y1, a.y2);
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = pair_value<MODE>(a, a_area, a_cx, a_cy, b[q], b_area[q], b_cx[q], b_cy[q]);
    float* const o = out + row * m;
    if (VEC) {
      if (col[0] < m) *reinterpret_cast<float4*>(o + col[0]) = make_float4(v[0], v[1], v[2], v[3]);  // m % 4 == 0: all four lie inside
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (col[q] < m) o[col[q]] = v[q];
    }
  }
}

template <int MODE>
int launch_box_iou_mode(const float* b1, const float* b2, float* out, int64_t n, int64_t m, bool vec, unsigned col_tiles, unsigned blocks,
                        hipStream_t s) {
  if (vec)
    hipLaunchKernelGGL((k_box_iou<MODE, true>), dim3(blocks), dim3(kIouBlock), 0, s, b1, b2, out, (long long)n, (long long)m, col_tiles);
  else
    hipLaunchKernelGGL((k_box_iou<MODE, false>), dim3(blocks), dim3(kIouBlock), 0, s, b1, b2, out, (long long)n, (long long)m, col_tiles);
  static const char* const names[3] = {"iou", "giou", "diou"};
  return check_launchf("k_box_iou<%s,%s>", names[MODE], vec ? "vec16" : "scalar");
}

// ---- masks_to_boxes ----------------------------------------------------------------------------------------------------------------
constexpr int kMtbBlock = 256;
constexpr int kMtbChunkRows = 32;  // rows of one mask that one workgroup reduces

__global__ __launch_bounds__(256) void k_mtb_init(int* __restrict__ ws, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  ws[i * 4] = INT_MAX, ws[i * 4 + 1] = INT_MAX, ws[i * 4 + 2] = -1, ws[i * 4 + 3] = -1;
}

// the set elements among the 16 bytes at p (16-byte aligned), whose first element is column x0: lo / hi take the least / greatest
__device__ inline void scan16(const unsigned char* p, int x0, int& lo, int& hi) {
  const uint4 q = *reinterpret_cast<const uint4*>(p);
  const unsigned d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!d[i]) continue;
    const unsigned nz = (d[i] | ((d[i] & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;  // bit 7 of every byte that is not 0
    lo = min(lo, x0 + 4 * i + (__builtin_ctz(nz) >> 3));
    hi = max(hi, x0 + 4 * i + ((31 - __builtin_clz(nz)) >> 3));
  }
}

__device__ inline void scan16(const float* p, int x0, int& lo, int& hi) {
  const float4 q = *reinterpret_cast<const float4*>(p);
  const float d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (d[i] != 0.f) lo = min(lo, x0 + i), hi = max(hi, x0 + i);  // the C `!=`: NaN is set, -0 is clear
}

template <typename T>
__global__ __launch_bounds__(kMtbBlock) void k_mtb_reduce(const T* __restrict__ masks, int* __restrict__ ws, int h, int w, int chunks) {
  constexpr int E = 16 / (int)sizeof(T);  // elements of one 16-byte load
  const long long mask = blockIdx.x / chunks;
  const int chunk = blockIdx.x % chunks;
  const int y_end = (int)min((long long)h, ((long long)chunk + 1) * kMtbChunkRows);  // the product passes 2^31 for h within 32 of it
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int min_x = INT_MAX, min_y = INT_MAX, max_x = -1, max_y = -1;
  for (int y = chunk * kMtbChunkRows + wave; y < y_end; y += kMtbBlock / kWave) {
    const T* const row = masks + ((size_t)mask * h + y) * (size_t)w;
    const int to_boundary = (int)(((16 - ((uintptr_t)row & 15)) & 15) / sizeof(T));  // < E <= 16 lanes
    const int head = min(w, to_boundary);
    const int nvec = (w - head) / E;
    int lo = INT_MAX, hi = -1;
    if (lane < head && row[lane] != (T)0) lo = hi = lane;
    for (int v = lane; v < nvec; v += kWave) scan16(row + head + v * E, head + v * E, lo, hi);
    const int t = head + nvec * E + lane;  // fewer than E elements remain
    if (t < w && row[t] != (T)0) lo = min(lo, t), hi = max(hi, t);
    if (hi >= 0) min_x = min(min_x, lo), max_x = max(max_x, hi), min_y = min(min_y, y), max_y = max(max_y, y);
  }
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    min_x = min(min_x, __shfl_xor(min_x, d)), min_y = min(min_y, __shfl_xor(min_y, d));
    max_x = max(max_x, __shfl_xor(max_x, d)), max_y = max(max_y, __shfl_xor(max_y, d));
  }
  __shared__ int part[kMtbBlock / kWave][4];
  if (lane == 0) part[wave][0] = min_x, part[wave][1] = min_y, part[wave][2] = max_x, part[wave][3] = max_y;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int i = 1; i < kMtbBlock / kWave; ++i)
    min_x = min(min_x, part[i][0]), min_y = min(min_y, part[i][1]), max_x = max(max_x, part[i][2]), max_y = max(max_y, part[i][3]);
  if (max_x < 0) return;  // nothing set in this chunk
  int* const r = ws + mask * 4;
  atomicMin(r, min_x), atomicMin(r + 1, min_y), atomicMax(r + 2, max_x), atomicMax(r + 3, max_y);
}

__global__ __launch_bounds__(256) void k_mtb_final(const int* __restrict__ ws, float* __restrict__ boxes, int* __restrict__ empty_flag,
                                                   long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int min_x = ws[i * 4], min_y = ws[i * 4 + 1], max_x = ws[i * 4 + 2], max_y = ws[i * 4 + 3];
  const bool empty = max_x < 0;
  boxes[i * 4] = empty ? 0.f : (float)min_x, boxes[i * 4 + 1] = empty ? 0.f : (float)min_y;
  boxes[i * 4 + 2] = empty ? 0.f : (float)max_x, boxes[i * 4 + 3] = empty ? 0.f : (float)max_y;
  if (empty) atomicOr(empty_flag, 1);
}

}  // namespace

bool box_iou_grid_fits(int64_t n, int64_t m) {
  const int64_t col_tiles = (m + kIouCols - 1) / kIouCols, strips = (n + kIouStrip - 1) / kIouStrip;
  return col_tiles <= 0x7fffffffLL / strips;
}

int launch_box_iou(const float* boxes1, const float* boxes2, float* out, int64_t n, int64_t m, int mode, hipStream_t s) {
  const unsigned col_tiles = (unsigned)((m + kIouCols - 1) / kIouCols);
  const unsigned blocks = (unsigned)(col_tiles * ((n + kIouStrip - 1) / kIouStrip));
  const bool vec = m % 4 == 0 && (uintptr_t)out % 16 == 0;
  if (mode == 0) return launch_box_iou_mode<0>(boxes1, boxes2, out, n, m, vec, col_tiles, blocks, s);
  if (mode == 1) return launch_box_iou_mode<1>(boxes1, boxes2, out, n, m, vec, col_tiles, blocks, s);
  return launch_box_iou_mode<2>(boxes1, boxes2, out, n, m, vec, col_tiles, blocks, s);
}

bool masks_to_boxes_grid_fits(int64_t n, int h) {
  const int64_t chunks = ((int64_t)h + kMtbChunkRows - 1) / kMtbChunkRows;
  // one workgroup of kMtbBlock threads per (mask, chunk); the runtime takes a grid of fewer than 2^32 threads in all (a launch of
  // 2^26 workgroups of 256 -- one mask of nearly 2^31 rows -- fails with "invalid configuration argument")
  return n <= ((1LL << 32) / kMtbBlock - 1) / (chunks > 0 ? chunks : 1);
}

int launch_masks_to_boxes(const void* masks, bool f32, float* boxes, int* empty_flag, int64_t n, int h, int w, void* workspace,
                          hipStream_t s) {
  int* const ws = static_cast<int*>(workspace);
  const unsigned per_mask_blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_mtb_init, dim3(per_mask_blocks), dim3(256), 0, s, ws, (long long)n);
  if (int rc = check_launch("k_mtb_init")) return rc;
  const int chunks = (int)(((int64_t)h + kMtbChunkRows - 1) / kMtbChunkRows);
  if (chunks > 0 && w > 0) {
    const unsigned blocks = (unsigned)(n * chunks);
    if (f32)
      hipLaunchKernelGGL(k_mtb_reduce<float>, dim3(blocks), dim3(kMtbBlock), 0, s, static_cast<const float*>(masks), ws, h, w, chunks);
    else
      hipLaunchKernelGGL(k_mtb_reduce<unsigned char>, dim3(blocks), dim3(kMtbBlock), 0, s, static_cast<const unsigned char*>(masks), ws, h,
                         w, chunks);
    if (int rc = check_launch("k_mtb_reduce")) return rc;
  }
  hipLaunchKernelGGL(k_mtb_final, dim3(per_mask_blocks), dim3(256), 0, s, ws, boxes, empty_flag, (long long)n);
  return check_launchf("k_mtb_init+k_mtb_reduce<%s,chunks%d>+k_mtb_final", f32 ? "f32" : "u8", chunks);
}

}  // namespace mv
