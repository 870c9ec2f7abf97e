// batchmix.hip -- MixUp / CutMix (v2/_augment.py) over a contiguous (B, S) batch on gfx950: y[b] = mix(x[b], x[(b - 1 + B) % B]).
//
// MixUp     y = fl(fl(prev * wp) + fl(self * ws)), wp = 1 - lam, ws = lam narrowed to the compute type: two rounded products and
//           one rounded sum, the reference's roll(1, 0).mul_(1 - lam).add_(x.mul(lam)).  float16 computes in float32 and rounds
//           each of the three results to float16, as ATen's CPU kernels do.  Never an fma (__fmul_rn / __fadd_rn).
// CutMix    y = prev inside the box [y1, y2) x [x1, x2) of every (h, w) plane, self outside: a byte mover over elements of 1, 2, 4
//           or 8 bytes.
// labels    one_hot(labels, K).float() mixed as above, without the one-hot tensor: every output is computed from the two indices.
//
// A lane owns 16 bytes of a sample.  gfx950 global memory takes 16-byte accesses at any byte address, so samples
// need no alignment; the ragged last group of a sample is anchored at S - V (it overlaps its left neighbour and writes the same
// bytes), and samples narrower than 16 bytes go element by element.
//
// Traffic.  MixUp needs every sample twice, as itself and as the partner of the next one.
//   k_mixup_roll  a lane keeps its 16-byte slice and walks b upwards over a segment of the batch with x[b - 1]'s slice in
//                 registers: every input byte is read once (plus one sample per segment), 2 x bytes in all.  Four b in flight.
//   k_mixup_flat  one lane per (b, slice), two loads: 3 x bytes from the lane's point of view.  Rows narrower than 64 groups
//                 (label rows) take it, where a walk would leave most of a wave idle.
// CutMix needs no walk: a group wholly outside the box loads only x[b], one wholly inside only x[b - 1], so k_cutmix already
// reads every output byte once; only groups that straddle a box edge load both.
#include <cstdlib>

#include "mv_common.h"

namespace mv {
namespace {

typedef unsigned int u32x4u __attribute__((ext_vector_type(4), aligned(1)));

template <typename T>
union Group {
  u32x4u q;
  T e[16 / sizeof(T)];
};

template <typename T>
__device__ inline Group<T> load16(const T* p) {
  Group<T> g;
  g.q = *reinterpret_cast<const u32x4u*>(p);
  return g;
}
template <typename T>
__device__ inline void store16(T* p, const Group<T>& g) {
  *reinterpret_cast<u32x4u*>(p) = g.q;
}

// ---- the three arithmetic types ------------------------------------------------------------------------------------------------
struct MixF32 {
  typedef float T;
  float wp, ws;
  __device__ float operator()(float prev, float self) const { return __fadd_rn(__fmul_rn(prev, wp), __fmul_rn(self, ws)); }
};
struct MixF16 {
  typedef _Float16 T;
  float wp, ws;
  __device__ _Float16 operator()(_Float16 prev, _Float16 self) const {
    const _Float16 a = (_Float16)__fmul_rn((float)prev, wp), b = (_Float16)__fmul_rn((float)self, ws);
    return (_Float16)__fadd_rn((float)a, (float)b);
  }
};
struct MixF64 {
  typedef double T;
  double wp, ws;
  __device__ double operator()(double prev, double self) const { return __dadd_rn(__dmul_rn(prev, wp), __dmul_rn(self, ws)); }
};

template <typename Op>
__device__ inline Group<typename Op::T> mix16(const Op& op, const Group<typename Op::T>& prev, const Group<typename Op::T>& self) {
  Group<typename Op::T> r;
#pragma unroll
  for (int j = 0; j < (int)(16 / sizeof(typename Op::T)); ++j) r.e[j] = op(prev.e[j], self.e[j]);
  return r;
}

// ---- (b, slice) per lane: rows of up to 256 groups share a workgroup -------------------------------------------------------------
struct FlatGrid {
  long long batch, elems;  // B, S
  long long groups;        // 16-byte groups per sample (1 when the sample is narrower than 16 bytes)
  int tpr_log2;            // lanes per sample segment (a power of two, 4..256)
};

// -> false when this lane has nothing to do; b, e0: the sample and the first element of the lane's group
__device__ inline bool flat_position(const FlatGrid& G, int v, long long& b, long long& e0) {
  const int tpr = 1 << G.tpr_log2;
  const unsigned tiles = (unsigned)((G.groups + tpr - 1) >> G.tpr_log2);
  const unsigned rb = blockIdx.x / tiles, tile = blockIdx.x - rb * tiles;
  b = (long long)rb * (256 >> G.tpr_log2) + (threadIdx.x >> G.tpr_log2);
  const long long g = (long long)tile * tpr + (threadIdx.x & (tpr - 1));
  if (b >= G.batch || g >= G.groups) return false;
  e0 = G.elems >= v ? min(g * v, G.elems - v) : 0;
  return true;
}

template <typename Op>
__global__ __launch_bounds__(256) void k_mixup_flat(const typename Op::T* __restrict__ x, typename Op::T* __restrict__ y,
                                                    const FlatGrid G, const Op op) {
  typedef typename Op::T T;
  constexpr int V = 16 / (int)sizeof(T);
  long long b, e0;
  if (!flat_position(G, V, b, e0)) return;
  const T* const self = x + b * G.elems + e0;
  const T* const prev = x + (b == 0 ? G.batch - 1 : b - 1) * G.elems + e0;
  T* const dst = y + b * G.elems + e0;
  if (G.elems >= V) {
    store16(dst, mix16(op, load16(prev), load16(self)));
    return;
  }
  for (int j = 0; j < (int)G.elems; ++j) dst[j] = op(prev[j], self[j]);
}

// ---- the walk: a lane keeps its slice and carries x[b - 1] in registers ------------------------------------------------------------
template <typename Op>
__global__ __launch_bounds__(256) void k_mixup_roll(const typename Op::T* __restrict__ x, typename Op::T* __restrict__ y,
                                                    const long long batch, const long long elems, const long long groups,
                                                    const int seg_len, const Op op) {
  typedef typename Op::T T;
  constexpr int V = 16 / (int)sizeof(T);
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= groups) return;
  const long long e0 = min(g * V, elems - V);  // the launcher sends samples of at least one group here
  const long long b0 = (long long)blockIdx.y * seg_len;
  const long long b1 = min(b0 + seg_len, batch);
  const T* src = x + b0 * elems + e0;
  T* dst = y + b0 * elems + e0;
  Group<T> prev = load16(x + (b0 == 0 ? batch - 1 : b0 - 1) * elems + e0);
  long long b = b0;
  for (; b + 4 <= b1; b += 4) {
    const Group<T> c0 = load16(src), c1 = load16(src + elems), c2 = load16(src + 2 * elems), c3 = load16(src + 3 * elems);
    store16(dst, mix16(op, prev, c0));
    store16(dst + elems, mix16(op, c0, c1));
    store16(dst + 2 * elems, mix16(op, c1, c2));
    store16(dst + 3 * elems, mix16(op, c2, c3));
    prev = c3;
    src += 4 * elems, dst += 4 * elems;
  }
  for (; b < b1; ++b) {
    const Group<T> c = load16(src);
    store16(dst, mix16(op, prev, c));
    prev = c;
    src += elems, dst += elems;
  }
}

// ---- CutMix ------------------------------------------------------------------------------------------------------------------------
struct Box {
  int h, w, x1, y1, x2, y2;
};

template <typename U>
__global__ __launch_bounds__(256) void k_cutmix(const U* __restrict__ x, U* __restrict__ y, const FlatGrid G, const Box B) {
  constexpr int V = 16 / (int)sizeof(U);
  long long b, e0;
  if (!flat_position(G, V, b, e0)) return;
  const int n = G.elems >= V ? V : (int)G.elems;
  // which of the group's elements lie in the box: the pixel of the first one, then a walk along the row
  const unsigned long long hw = (unsigned long long)B.h * B.w;
  int row, col;
  if (G.elems <= 0x7fffffffLL) {  // 32-bit division when the sample fits
    const unsigned pix = (unsigned)e0 % (unsigned)hw;
    row = (int)(pix / (unsigned)B.w), col = (int)(pix - (unsigned)row * (unsigned)B.w);
  } else {
    const unsigned long long pix = (unsigned long long)e0 % hw;
    row = (int)(pix / (unsigned)B.w), col = (int)(pix - (unsigned long long)row * (unsigned)B.w);
  }
  unsigned mask = 0;
  if (col + n <= B.w) {  // the group lies in one row: the box covers elements [lo, hi) of it
    const int lo = min(max(B.x1 - col, 0), n), hi = min(max(B.x2 - col, 0), n);
    if (row >= B.y1 && row < B.y2 && hi > lo) mask = (unsigned)((1ull << hi) - (1ull << lo));
  } else {
    for (int j = 0; j < n; ++j) {
      if (row >= B.y1 && row < B.y2 && col >= B.x1 && col < B.x2) mask |= 1u << j;
      if (++col == B.w) {
        col = 0;
        if (++row == B.h) row = 0;
      }
    }
  }
  const U* const self = x + b * G.elems + e0;
  const U* const prev = x + (b == 0 ? G.batch - 1 : b - 1) * G.elems + e0;
  U* const dst = y + b * G.elems + e0;
  if (G.elems >= V) {
    if (mask == 0) {
      store16(dst, load16(self));
    } else if (mask == (1u << V) - 1u) {
      store16(dst, load16(prev));
    } else {
      const Group<U> s = load16(self), p = load16(prev);
      Group<U> r;
#pragma unroll
      for (int j = 0; j < V; ++j) r.e[j] = (mask >> j) & 1u ? p.e[j] : s.e[j];
      store16(dst, r);
    }
    return;
  }
  for (int j = 0; j < n; ++j) dst[j] = (mask >> j) & 1u ? prev[j] : self[j];
}

// ---- index labels: one_hot, float, roll and the mix in one pass over the outputs ---------------------------------------------------
// Four consecutive outputs of the flat (B, K) result per lane.  A label outside [0, K) matches no column: its row's own
// contribution is all zeros and nothing is written out of bounds (there is no scatter).
template <bool VEC>
__global__ __launch_bounds__(256) void k_mixup_labels(const long long* __restrict__ labels, float* __restrict__ y,
                                                      const long long batch, const int classes, const MixF32 op) {
  const long long total = batch * classes;
  const long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (base >= total) return;
  const bool small = total <= 0x7fffffffLL;
  float out[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long i = min(base + j, total - 1);
    const long long b = small ? (long long)((unsigned)i / (unsigned)classes) : i / classes;
    const long long c = i - b * classes;
    const long long self = labels[b], prev = labels[b == 0 ? batch - 1 : b - 1];
    out[j] = op(prev == c ? 1.f : 0.f, self == c ? 1.f : 0.f);
  }
  if (VEC && base + 4 <= total) {
    *reinterpret_cast<float4*>(y + base) = make_float4(out[0], out[1], out[2], out[3]);
    return;
  }
  for (int j = 0; j < 4 && base + j < total; ++j) y[base + j] = out[j];
}

FlatGrid flat_grid(long long batch, long long elems, int elem_bytes, long long* blocks) {
  const int v = 16 / elem_bytes;
  FlatGrid g;
  g.batch = batch, g.elems = elems;
  g.groups = elems >= v ? (elems + v - 1) / v : 1;
  g.tpr_log2 = 2;
  while (g.tpr_log2 < 8 && (1LL << g.tpr_log2) < g.groups) ++g.tpr_log2;
  const int tpr = 1 << g.tpr_log2, rpb = 256 / tpr;
  *blocks = ((batch + rpb - 1) / rpb) * ((g.groups + tpr - 1) / tpr);
  return g;
}

// The walk's launch: ceil(groups / 256) workgroups along a sample, times the segments of the batch.
struct RollPlan {
  long long blocks_x;
  int segments, seg_len;
};

// Enough workgroups to keep 256 CUs x 8 in flight; a segment re-reads one sample, so it is at least kMinSegment samples long
// (at most 1 / kMinSegment extra input traffic).  Measured (the segment-length table): segments of 8 to 32
// samples are the fastest at 256 x 3 x 224^2 and 4096 x 3 x 32^2; at 32^2 a minimum of 16 is 8 % faster than one of 4 although it
// launches 768 workgroups.  kRollMinGroups has only the 256 x 1000 label row behind it.
constexpr long long kRollTargetBlocks = 2048;
constexpr long long kMinSegment = 16;
constexpr long long kRollMinGroups = 64;

RollPlan roll_plan(long long batch, long long groups) {
  RollPlan p;
  p.blocks_x = (groups + 255) / 256;
  long long segs = (kRollTargetBlocks + p.blocks_x - 1) / p.blocks_x;
  long long len = (batch + segs - 1) / segs;
  if (len < kMinSegment) len = kMinSegment;
  if (const char* e = tune_env("MV_MIX_SEG_LEN")) len = atoll(e) > 0 ? atoll(e) : len;  // tools/perf_mix.py --segments
  if (len > batch) len = batch;
  if (len > 0x7fffffffLL) len = 0x7fffffffLL;
  p.seg_len = (int)len;
  p.segments = (int)((batch + len - 1) / len > 65535 ? 0 : (batch + len - 1) / len);
  return p;
}

bool use_roll(long long batch, long long elems, int elem_bytes) {
  const int v = 16 / elem_bytes;
  if (elems < v) return false;
  const long long groups = (elems + v - 1) / v;
  if (const char* e = tune_env("MV_MIX_KERNEL")) return e[0] == 'r';  // tools/perf_mix.py: "roll" / "flat"
  return batch > 1 && groups >= kRollMinGroups;
}

template <typename Op>
int launch_mixup_t(const void* x, void* y, long long batch, long long elems, const Op& op, const char* name, hipStream_t s) {
  typedef typename Op::T T;
  constexpr int V = 16 / (int)sizeof(T);
  if (use_roll(batch, elems, (int)sizeof(T))) {
    const long long groups = (elems + V - 1) / V;
    const RollPlan p = roll_plan(batch, groups);
    if (p.segments > 0 && p.blocks_x <= 0x7fffffffLL) {
      hipLaunchKernelGGL(k_mixup_roll<Op>, dim3((unsigned)p.blocks_x, (unsigned)p.segments), dim3(256), 0, s, static_cast<const T*>(x),
                         static_cast<T*>(y), batch, elems, groups, p.seg_len, op);
      return check_launchf("k_mixup_roll<%s,seg%d>", name, p.seg_len);
    }
  }
  long long blocks;
  const FlatGrid g = flat_grid(batch, elems, (int)sizeof(T), &blocks);
  hipLaunchKernelGGL(k_mixup_flat<Op>, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const T*>(x), static_cast<T*>(y), g, op);
  return check_launchf("k_mixup_flat<%s>", name);
}

}  // namespace

bool mix_grid_fits(int64_t batch, int64_t elems, int elem_bytes) {
  long long blocks;
  flat_grid(batch, elems, elem_bytes, &blocks);
  return blocks <= 0x7fffffffLL;
}

int launch_mixup(const void* x, void* y, int elem_bytes, int64_t batch, int64_t elems, double lam, hipStream_t s) {
  const double wp = 1.0 - lam;
  if (elem_bytes == 4) return launch_mixup_t(x, y, batch, elems, MixF32{(float)wp, (float)lam}, "f32", s);
  if (elem_bytes == 2) return launch_mixup_t(x, y, batch, elems, MixF16{(float)wp, (float)lam}, "f16", s);
  return launch_mixup_t(x, y, batch, elems, MixF64{wp, lam}, "f64", s);
}

int launch_cutmix(const void* x, void* y, int64_t batch, int64_t elems, int elem_bytes, int h, int w, int x1, int y1, int x2, int y2,
                  hipStream_t s) {
  long long blocks;
  const FlatGrid g = flat_grid(batch, elems, elem_bytes, &blocks);
  const Box box = {h, w, x1, y1, x2, y2};
  auto go = [&](auto* px, auto* py, auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, s, px, py, g, box); };
  switch (elem_bytes) {
    case 1: go((const uint8_t*)x, (uint8_t*)y, k_cutmix<uint8_t>); break;
    case 2: go((const uint16_t*)x, (uint16_t*)y, k_cutmix<uint16_t>); break;
    case 4: go((const uint32_t*)x, (uint32_t*)y, k_cutmix<uint32_t>); break;
    default: go((const uint64_t*)x, (uint64_t*)y, k_cutmix<uint64_t>); break;
  }
  return check_launchf("k_cutmix<b%d>", elem_bytes);
}

int launch_mixup_labels(const int64_t* labels, float* y, int64_t batch, int classes, double lam, hipStream_t s) {
  const MixF32 op{(float)(1.0 - lam), (float)lam};
  const long long quads = (batch * (long long)classes + 3) / 4;
  const unsigned nb = (unsigned)((quads + 255) / 256);
  const bool vec = ((uintptr_t)y % 16) == 0;
  if (vec)
    hipLaunchKernelGGL(k_mixup_labels<true>, dim3(nb), dim3(256), 0, s, (const long long*)labels, y, (long long)batch, classes, op);
  else
    hipLaunchKernelGGL(k_mixup_labels<false>, dim3(nb), dim3(256), 0, s, (const long long*)labels, y, (long long)batch, classes, op);
  return check_launchf("k_mixup_labels<%s>", vec ? "vec" : "scalar");
}

}  // namespace mv
