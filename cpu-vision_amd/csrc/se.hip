// se.hip -- the squeeze-excitation layer (ops/misc.py SqueezeExcitation: scale_activation(fc2(activation(fc1(avgpool(x))))) * x) of
// MobileNetV3 and the dense layer of its classifier on gfx950, as three small kernels whose summation orders are stated in
// mi355vision.h and do not depend on the launch:
//
//   k_se_pool      one WAVE per (image, channel) plane of H W elements.  Element p belongs to lane (p / 4) mod 64; a lane adds
//                  (double)x[p] for its elements in ascending p to 0.0; the 64 lane sums go through the fixed tree
//                  S[l] += S[l + off] for l < off, off = 32, 16, 8, 4, 2, 1; m = (float)(S[0] / (double)(H W)).  A lane's
//                  elements come as whole quads 4 q .. 4 q + 3, q = lane, lane + 64, ...: one 16-byte load where the plane starts on a
//                  16-byte boundary, four 4-byte loads where it does not, the same values in the same order either way.
//   k_linear_act   one WAVE per output (i, j).  Lane l adds the exact products (double)x[i][k] (double)w[j][k] for k = l, l + 64, ...
//                  in ascending k to 0.0; the same tree; v = (float)(S + (double)b[j]); then the activation.  The four waves of a
//                  workgroup are four consecutive j of one image i (x[i] comes from L1 for three of them).
//   k_se_scale     y[i][c][p] = fl(gate[i][c] x[i][c][p]), four consecutive elements per thread.
//
// Every float64 operation is written with __d*_rn and every float32 one with __f*_rn: never an fma.
#include "mv_boxcoder.h"
#include "mv_common.h"

namespace mv {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// S[l] += S[l + off] for l < off, off = 32 .. 1: lane 0 ends with the tree's root (the other lanes' values are not used)
__device__ __forceinline__ double wave_tree_sum(double s) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s = __dadd_rn(s, __shfl_down(s, off, kWave));
  return s;
}

struct PoolArgs {
  const float* x;
  float* y;
  long long planes, x_stride;  // n * c; elements between images
  int c, hw;
};

__global__ __launch_bounds__(256) void k_se_pool(const PoolArgs A) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long plane = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (plane >= A.planes) return;
  const long long img = plane / A.c;
  const int ch = (int)(plane - img * A.c);
  const float* xp = A.x + (size_t)img * A.x_stride + (size_t)ch * A.hw;
  const int HW = A.hw;
  const bool vec = (reinterpret_cast<uintptr_t>(xp) & 15) == 0;  // wave-uniform
  double s = 0.0;
  for (long long p = 4LL * lane; p < HW; p += 4 * kWave) {
    if (vec && p + 3 < HW) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(xp + p);
      s = __dadd_rn(s, (double)a.x), s = __dadd_rn(s, (double)a.y), s = __dadd_rn(s, (double)a.z), s = __dadd_rn(s, (double)a.w);
    } else {
      for (int i = 0; i < 4; ++i)
        if (p + i < HW) s = __dadd_rn(s, (double)xp[p + i]);
    }
  }
  s = wave_tree_sum(s);
  if (lane == 0) A.y[plane] = __double2float_rn(__ddiv_rn(s, (double)HW));
}

__device__ __forceinline__ float linear_activation(float v, int act) {
  if (act == MV_ACT_RELU) return v < 0.f ? 0.f : v;  // a NaN stays
  if (act == MV_ACT_SIGMOID) return sigmoid_cr(v);
  if (act == MV_ACT_HARDSWISH || act == MV_ACT_HARDSIGMOID) {
    const float t = clamp0(__fadd_rn(v, 3.f), 6.f);  // torch.clamp: a NaN stays
    return act == MV_ACT_HARDSIGMOID ? __fdiv_rn(t, 6.f) : __fdiv_rn(__fmul_rn(v, t), 6.f);
  }
  return v;
}

struct LinActArgs {
  const float* x;  // [n][k]
  const float* w;  // [m][k]
  const float* b;  // [m] or null
  float* y;        // [n][m]
  int k, m, act;
};

__global__ __launch_bounds__(256) void k_linear_act(const LinActArgs A) {
  const int lane = threadIdx.x & (kWave - 1);
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  const int i = blockIdx.y;
  if (j >= A.m) return;
  const float* xr = A.x + (size_t)i * A.k;
  const float* wr = A.w + (size_t)j * A.k;
  double s = 0.0;
  for (int k = lane; k < A.k; k += kWave) s = __dadd_rn(s, __dmul_rn((double)xr[k], (double)wr[k]));
  s = wave_tree_sum(s);
  if (lane == 0) {
    if (A.b) s = __dadd_rn(s, (double)A.b[j]);
    A.y[(size_t)i * A.m + j] = linear_activation(__double2float_rn(s), A.act);
  }
}

struct ScaleArgs {
  const float* x;
  const float* gate;  // [planes]
  float* y;
  long long total;  // planes * hw
  int hw, vec;      // vec: hw % 4 == 0 and x, y 16-byte aligned -- a thread's four elements are one quad of one plane
};

__global__ __launch_bounds__(256) void k_se_scale(const ScaleArgs A) {
  const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e >= A.total) return;
  if (A.vec) {
    const float g = A.gate[e / A.hw];
    const f32x4 a = *reinterpret_cast<const f32x4*>(A.x + e);
    *reinterpret_cast<f32x4*>(A.y + e) = (f32x4){__fmul_rn(g, a.x), __fmul_rn(g, a.y), __fmul_rn(g, a.z), __fmul_rn(g, a.w)};
  } else {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (e + i < A.total) v[i] = __fmul_rn(A.gate[(e + i) / A.hw], A.x[e + i]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (e + i < A.total) A.y[e + i] = v[i];
  }
}

}  // namespace

int launch_global_avgpool(const float* x, float* y, int64_t n, int c, int hw, int64_t x_stride, hipStream_t s) {
  PoolArgs a = {x, y, (long long)n * c, (long long)x_stride, c, hw};
  hipLaunchKernelGGL(k_se_pool, dim3((unsigned)((a.planes + 3) / 4)), dim3(256), 0, s, a);
  return check_launch("k_se_pool");
}

int launch_linear_act(const float* x, const float* w, const float* b, float* y, int64_t n, int k, int m, int act, hipStream_t s) {
  LinActArgs a = {x, w, b, y, k, m, act};
  hipLaunchKernelGGL(k_linear_act, dim3((unsigned)((m + 3) / 4), (unsigned)n), dim3(256), 0, s, a);
  return check_launch("k_linear_act");
}

int launch_se_scale(const float* x, const float* gate, float* y, int64_t planes, int hw, hipStream_t s) {
  ScaleArgs a = {x, gate, y, (long long)planes * hw, hw, 0};
  a.vec = hw % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0;
  hipLaunchKernelGGL(k_se_scale, dim3((unsigned)((a.total + 1023) / 1024)), dim3(256), 0, s, a);
  return check_launchf("k_se_scale<%s>", a.vec ? "vec16" : "scalar");
}

}  // namespace mv
