// layernorm.hip -- LayerNorm over the channels of float32 NCHW images on gfx950: models/convnext.py LayerNorm2d (permute to NHWC,
// F.layer_norm over C, permute back) as ONE launch, and its statistics alone for the pointwise conv that normalises in its loads
// (convnorm.hip, k_conv1x1_ln).
//
// A pixel's C values lie H W elements apart, so -- as in l2norm.hip -- the lanes run along the pixels and the channels are cut over the
// threads of a workgroup: 256 threads = kLnPixels (16) consecutive pixels x kLnGroups (16) channel groups, thread t = 16 g + p.
// The summation order is fixed, the same for every shape, and does not involve the pixel's index, N, H or W:
//
//   sum     group g adds (double)x_c for c = g, g + 16, g + 32, ... in ascending order to 0.0;
//   fold    the 16 partial sums go through LDS and every thread of the pixel adds them in ascending g to 0.0: S;  m = S / C;
//   square  group g adds d d, d = (double)x_c - m, over the same channels in the same order to 0.0 (the subtraction, the square and the
//           add are one float64 rounding each: never an fma); the same fold: Q;
//   stats   mean = (float)m, rstd = (float)(1.0 / sqrt(Q / C + (double)eps)), IEEE float64 division and square root;
//   apply   the group's channels a third time: y_c = fl(fl(fl(fl(x_c - mean) rstd) w_c) + b_c), four float32 roundings; the last two
//           steps are dropped when w / b are null.
//
// The second and third read of x come from L2 (the 16 x C floats of a workgroup were loaded by the same workgroup just before).
// Every operation is written with __f*_rn / __d*_rn.
#include "mv_common.h"

namespace mv {
namespace {

constexpr int kLnThreads = kLnPixels * kLnGroups;
static_assert(kLnThreads == 256 && kLnPixels == 16, "thread t = 16 g + p");

struct LnArgs {
  const float* x;
  float* y;                // APPLY
  float *mean, *rstd;      // !APPLY: (n, hw)
  const float *weight, *bias;
  int c, hw;
  int blocks_per_image;    // ceil(hw / kLnPixels)
  float eps;
};

__device__ inline double ln_fold(double (&part)[kLnGroups][kLnPixels], double s, int g, int p) {
  __syncthreads();  // the previous fold's reads
  part[g][p] = s;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int j = 0; j < kLnGroups; ++j) t = __dadd_rn(t, part[j][p]);
  return t;
}

template <bool APPLY>
__global__ __launch_bounds__(kLnThreads) void k_layer_norm2d(const LnArgs A) {
  const int img = (int)(blockIdx.x / (unsigned)A.blocks_per_image);
  const int blk = (int)(blockIdx.x - (unsigned)img * (unsigned)A.blocks_per_image);
  const int p = threadIdx.x & (kLnPixels - 1), g = threadIdx.x >> 4;
  const long long pix = (long long)blk * kLnPixels + p;
  const bool live = pix < A.hw;
  const size_t image = (size_t)A.c * A.hw;
  const float* const xp = A.x + (size_t)img * image + pix;  // channel c at xp[c hw]; c hw + pix < 2^31
  __shared__ double part[kLnGroups][kLnPixels];

  double s = 0.0;
  if (live) {
#pragma unroll 4
    for (int c = g; c < A.c; c += kLnGroups) s = __dadd_rn(s, (double)xp[(size_t)c * A.hw]);
  }
  const double m = __ddiv_rn(ln_fold(part, s, g, p), (double)A.c);
  double q = 0.0;
  if (live) {
#pragma unroll 4
    for (int c = g; c < A.c; c += kLnGroups) {
      const double d = __dsub_rn((double)xp[(size_t)c * A.hw], m);
      q = __dadd_rn(q, __dmul_rn(d, d));
    }
  }
  const double Q = ln_fold(part, q, g, p);
  if (!live) return;
  const float mean = __double2float_rn(m);
  const float rstd = __double2float_rn(__ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(__ddiv_rn(Q, (double)A.c), (double)A.eps))));
  if constexpr (APPLY) {
    float* const yp = A.y + (size_t)img * image + pix;
#pragma unroll 4
    for (int c = g; c < A.c; c += kLnGroups) {
      const size_t e = (size_t)c * A.hw;
      float v = __fmul_rn(__fsub_rn(xp[e], mean), rstd);
      if (A.weight) v = __fmul_rn(v, A.weight[c]);
      if (A.bias) v = __fadd_rn(v, A.bias[c]);
      yp[e] = v;
    }
  } else if (g == 0) {
    A.mean[(size_t)img * A.hw + pix] = mean;
    A.rstd[(size_t)img * A.hw + pix] = rstd;
  }
}

}  // namespace

int launch_layer_norm2d(const float* x, const float* weight, const float* bias, float* y, float* mean, float* rstd, int64_t n, int c,
                        int64_t hw, float eps, hipStream_t s) {
  LnArgs a = {};
  a.x = x, a.y = y, a.mean = mean, a.rstd = rstd, a.weight = weight, a.bias = bias;
  a.c = c, a.hw = (int)hw, a.blocks_per_image = (int)layer_norm_blocks(hw), a.eps = eps;
  const dim3 grid((unsigned)(n * a.blocks_per_image));
  if (y) {
    hipLaunchKernelGGL(k_layer_norm2d<true>, grid, dim3(kLnThreads), 0, s, a);
    return check_launch("k_layer_norm2d<apply>");
  }
  hipLaunchKernelGGL(k_layer_norm2d<false>, grid, dim3(kLnThreads), 0, s, a);
  return check_launch("k_layer_norm2d<stats>");
}

}  // namespace mv
