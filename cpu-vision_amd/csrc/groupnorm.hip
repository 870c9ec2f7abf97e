// groupnorm.hip -- torch.nn.GroupNorm (+ ReLU) of float32 NCHW images on gfx950: the block `GroupNorm(G, C) -> ReLU` of the FCOS
// towers (models/detection/fcos.py) and of the v2 detection heads.
//
// The slab of (image i, group g) is ONE contiguous span of m = (C / G) H W floats at x + i x_stride + g m.  A slab runs from a
// hundred elements (P7) to half a MiB (P3 of an 800 x 1344 input), more than LDS holds, and at batch 1 there are 32 slabs for 256
// CUs, so a slab is cut into chunks of kGnChunk elements and the call is two launches over (slab, chunk):
//
// k_gn_stats   one workgroup per (slab, chunk): the chunk's sum of x and of x^2 in float64 -> partials[slab][chunk] = (S, S2) in
//              the workspace.  No atomics: every partial has one writer.
// k_gn_apply   one workgroup per (slab, chunk): the slab's partials summed in ASCENDING chunk order (one thread, from LDS), mean
//              and rstd, then x -> y over the chunk.
//
// The float64 sums are reproducible because the order is fixed and stated (mi355vision.h, mv_group_norm_act_f32):
//   thread t of 256 adds its kGnChunk / 256 = 16 elements  e = u 1024 + 4 t + q  (u = 0 .. 3 outer, q = 0 .. 3 inner; an element
//   past the slab's end counts as +0) one after the other to (s, s2) = (0, 0): s += (double)x, s2 += (double)x (double)x (exact);
//   the 64 lanes of a wave are folded by halves, v[l] += v[l ^ 32], then ^ 16, 8, 4, 2, 1;  the four waves are added in order.
// The element -> thread mapping is relative to the SLAB's start, so the result of a slab does not depend on where it lies or on
// how it is aligned: VEC (every slab 16-byte aligned and m % 4 == 0) only replaces four dword loads by one dwordx4 load of the same
// four elements.  Every float operation is written with __f*_rn / __d*_rn: never an fma.
#include "mv_common.h"

namespace mv {
namespace {

constexpr int kGnThreads = 256;
constexpr int kGnPerThread = kGnChunk / kGnThreads;  // 16
constexpr int kGnRounds = kGnPerThread / 4;          // 4 groups of 4 consecutive elements per thread
static_assert(kGnChunk == kGnThreads * 16, "the stated order: 4 rounds of 4 consecutive elements per thread");

struct GnArgs {
  const float* x;
  float* y;
  const float* gamma;  // null: no scale
  const float* beta;   // null: no shift
  long long x_stride, y_stride;  // elements between images
  long long m;                   // elements of a slab, < 2^31
  int groups, cpg, hw;           // cpg: channels per group
  long long chunks;              // per slab
  float eps;
  int relu;
  double* partials;  // (slabs, chunks, 2)
};

// the four elements e .. e + 3 of a slab of m elements at p; past the end: +0
template <bool VEC>
__device__ inline void load4(const float* p, long long e, long long m, float (&v)[4]) {
  if (VEC) {
    if (e < m) {  // m % 4 == 0 and e % 4 == 0: all four or none
      const float4 f = *reinterpret_cast<const float4*>(p + e);
      v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
    } else {
      v[0] = v[1] = v[2] = v[3] = 0.f;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = e + q < m ? p[e + q] : 0.f;
  }
}

__device__ inline double lane_xor(double v, int mask) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __shfl_xor(lo, mask), hi = __shfl_xor(hi, mask);
  return __hiloint2double(hi, lo);
}

template <bool VEC>
__global__ __launch_bounds__(kGnThreads) void k_gn_stats(const GnArgs G) {
  const long long slab = (long long)blockIdx.x / G.chunks, chunk = (long long)blockIdx.x - slab * G.chunks;
  const long long img = slab / G.groups;
  const int g = (int)(slab - img * G.groups);
  const float* const p = G.x + (size_t)img * G.x_stride + (size_t)g * G.m;
  const int tid = threadIdx.x;
  const long long base = chunk * kGnChunk + 4 * tid;

  float v[kGnRounds][4];
#pragma unroll
  for (int u = 0; u < kGnRounds; ++u) load4<VEC>(p, base + u * (4 * kGnThreads), G.m, v[u]);
  double s = 0.0, s2 = 0.0;
#pragma unroll
  for (int u = 0; u < kGnRounds; ++u)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double d = (double)v[u][q];
      s = __dadd_rn(s, d), s2 = __dadd_rn(s2, __dmul_rn(d, d));
    }
#pragma unroll
  for (int mask = 32; mask >= 1; mask >>= 1) s = __dadd_rn(s, lane_xor(s, mask)), s2 = __dadd_rn(s2, lane_xor(s2, mask));

  __shared__ double part[kGnThreads / kWave][2];
  if ((tid & 63) == 0) part[tid >> 6][0] = s, part[tid >> 6][1] = s2;
  __syncthreads();
  if (tid == 0) {
    double a = part[0][0], b = part[0][1];
#pragma unroll
    for (int w = 1; w < kGnThreads / kWave; ++w) a = __dadd_rn(a, part[w][0]), b = __dadd_rn(b, part[w][1]);
    double* const out = G.partials + ((size_t)slab * G.chunks + chunk) * 2;
    out[0] = a, out[1] = b;
  }
}

template <bool VEC>
__global__ __launch_bounds__(kGnThreads) void k_gn_apply(const GnArgs G) {
  const long long slab = (long long)blockIdx.x / G.chunks, chunk = (long long)blockIdx.x - slab * G.chunks;
  const long long img = slab / G.groups;
  const int g = (int)(slab - img * G.groups);
  const float* const p = G.x + (size_t)img * G.x_stride + (size_t)g * G.m;
  float* const o = G.y + (size_t)img * G.y_stride + (size_t)g * G.m;
  const int tid = threadIdx.x;

  // the slab's sums: its partials in ascending chunk order, kGnThreads at a time through LDS
  __shared__ double tile[kGnThreads][2];
  __shared__ float stat[2];
  const double* const parts = G.partials + (size_t)slab * G.chunks * 2;
  double S = 0.0, S2 = 0.0;
  for (long long c0 = 0; c0 < G.chunks; c0 += kGnThreads) {
    const long long left = G.chunks - c0;
    const int cnt = left < kGnThreads ? (int)left : kGnThreads;
    if (tid < cnt) tile[tid][0] = parts[(c0 + tid) * 2], tile[tid][1] = parts[(c0 + tid) * 2 + 1];
    __syncthreads();
    if (tid == 0)
      for (int j = 0; j < cnt; ++j) S = __dadd_rn(S, tile[j][0]), S2 = __dadd_rn(S2, tile[j][1]);
    __syncthreads();
  }
  if (tid == 0) {
    const double dm = (double)G.m;
    const double mean = __ddiv_rn(S, dm);
    double var = __dsub_rn(__ddiv_rn(S2, dm), __dmul_rn(mean, mean));
    var = var < 0.0 ? 0.0 : var;  // a NaN stays
    const double rstd = __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(var, (double)G.eps)));
    stat[0] = (float)mean, stat[1] = (float)rstd;
  }
  __syncthreads();
  const float mean = stat[0], rstd = stat[1];

  const long long base = chunk * kGnChunk + 4 * tid;
  const unsigned hw = (unsigned)G.hw;
  const int c_first = g * G.cpg;
#pragma unroll
  for (int u = 0; u < kGnRounds; ++u) {
    const long long e = base + u * (4 * kGnThreads);
    if (e >= G.m) continue;
    float v[4];
    load4<VEC>(p, e, G.m, v);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c_first + (int)((unsigned)(e + q) / hw);  // past the end (not stored): any channel of the group or the next
      float r = __fmul_rn(__fsub_rn(v[q], mean), rstd);
      if (e + q < G.m) {
        if (G.gamma) r = __fmul_rn(r, G.gamma[c]);
        if (G.beta) r = __fadd_rn(r, G.beta[c]);
      }
      if (G.relu) r = r < 0.f ? 0.f : r;  // a NaN stays
      v[q] = r;
    }
    if (VEC) {
      *reinterpret_cast<float4*>(o + e) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (e + q < G.m) o[e + q] = v[q];
    }
  }
}

}  // namespace

int launch_group_norm_act(const float* x, float* y, const float* gamma, const float* beta, int64_t n, int c, int h, int w, int groups,
                          int64_t x_stride, int64_t y_stride, float eps, int relu, void* workspace, hipStream_t s) {
  GnArgs g = {};
  g.x = x, g.y = y, g.gamma = gamma, g.beta = beta, g.x_stride = x_stride, g.y_stride = y_stride;
  g.groups = groups, g.cpg = c / groups, g.hw = h * w, g.m = (int64_t)g.cpg * g.hw;
  g.chunks = group_norm_chunks(g.m);
  g.eps = eps, g.relu = relu, g.partials = static_cast<double*>(workspace);
  const unsigned blocks = (unsigned)(n * groups * g.chunks);
  // one dwordx4 per four elements where every slab of x and of y starts on 16 bytes
  const bool vec = g.m % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0 && (n == 1 || (x_stride % 4 == 0 && y_stride % 4 == 0));
  if (vec) {
    hipLaunchKernelGGL(k_gn_stats<true>, dim3(blocks), dim3(kGnThreads), 0, s, g);
    if (int rc = check_launch("k_gn_stats<vec>")) return rc;
    hipLaunchKernelGGL(k_gn_apply<true>, dim3(blocks), dim3(kGnThreads), 0, s, g);
    return check_launchf("k_gn_apply<vec,relu%d>", relu);
  }
  hipLaunchKernelGGL(k_gn_stats<false>, dim3(blocks), dim3(kGnThreads), 0, s, g);
  if (int rc = check_launch("k_gn_stats<scalar>")) return rc;
  hipLaunchKernelGGL(k_gn_apply<false>, dim3(blocks), dim3(kGnThreads), 0, s, g);
  return check_launchf("k_gn_apply<scalar,relu%d>", relu);
}

}  // namespace mv
