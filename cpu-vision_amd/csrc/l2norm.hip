// l2norm.hip -- scale_weight.view(1, -1, 1, 1) * torch.nn.functional.normalize(x) (p = 2, dim = 1) of float32 NCHW images on gfx950:
// the rescaling of conv4_3 in front of SSD's first head (models/detection/ssd.py, SSDFeatureExtractorVGG.forward).
//
// A pixel's C values lie H W elements apart, so the lanes run along the pixels and the channels are cut over the threads of a
// workgroup: 256 threads = kL2Pixels (16) consecutive pixels x kL2Groups (16) channel groups, thread t = 16 g + p.  A wave reads four
// spans of 16 consecutive floats per channel step; at 38 x 38 x 512 that is 91 workgroups per image with 32 channels per thread
// instead of 23 waves with a 512-channel chain each.  ONE launch:
//
//   sum     group g adds (double)x_c (double)x_c (exact) for c = g, g + 16, g + 32, ... in ascending order to 0 in float64;
//   fold    the 16 partial sums go through LDS and every thread of the pixel adds them in ascending g to 0: S;
//   apply   nrm = (float)sqrt(S), d = nrm < eps ? eps : nrm (a NaN stays), and the group's channels again:
//           y_c = fl(w_c fl(x_c / d)).
//
// The second read of x comes from L2: the 16 x C floats of a workgroup (32 KiB at C = 512) were loaded by the same workgroup a few
// microseconds before, and C is not bounded, so neither registers nor LDS hold them in general.  The traffic counts as 3 x 4 B
// per element.  In place (y == x): a thread's second read and its store are of the same element, after the barrier behind the sums.
// The channel -> group mapping does not involve the pixel's index, so a pixel's result is a function of its C values, the weights
// and eps alone.  Every float operation is written with __f*_rn / __d*_rn: never an fma, never a reciprocal.
#include "mv_common.h"

namespace mv {
namespace {

constexpr int kL2Threads = kL2Pixels * kL2Groups;
static_assert(kL2Threads == 256 && kL2Pixels == 16, "thread t = 16 g + p");

struct L2Args {
  const float* x;
  float* y;
  const float* weight;
  long long x_stride, y_stride;  // elements between images
  int c, hw;
  int blocks_per_image;          // ceil(hw / kL2Pixels)
  float eps;
};

__global__ __launch_bounds__(kL2Threads) void k_l2_normalize_scale(const L2Args A) {
  const int img = (int)(blockIdx.x / (unsigned)A.blocks_per_image);
  const int blk = (int)(blockIdx.x - (unsigned)img * (unsigned)A.blocks_per_image);
  const int p = threadIdx.x & (kL2Pixels - 1), g = threadIdx.x >> 4;
  const long long pix = (long long)blk * kL2Pixels + p;
  const bool live = pix < A.hw;
  const float* const xp = A.x + (size_t)img * A.x_stride + pix;  // channel c at xp[c hw]; c hw + pix < 2^31
  float* const yp = A.y + (size_t)img * A.y_stride + pix;

  double s = 0.0;
  if (live) {
#pragma unroll 4
    for (int c = g; c < A.c; c += kL2Groups) {
      const double d = (double)xp[(size_t)c * A.hw];
      s = __dadd_rn(s, __dmul_rn(d, d));
    }
  }
  __shared__ double part[kL2Groups][kL2Pixels];
  part[g][p] = s;
  __syncthreads();
  if (!live) return;
  double S = 0.0;
#pragma unroll
  for (int j = 0; j < kL2Groups; ++j) S = __dadd_rn(S, part[j][p]);
  const float nrm = __double2float_rn(__dsqrt_rn(S));
  const float d = nrm < A.eps ? A.eps : nrm;  // clamp_min: a NaN stays
#pragma unroll 4
  for (int c = g; c < A.c; c += kL2Groups) {
    const size_t e = (size_t)c * A.hw;
    yp[e] = __fmul_rn(A.weight[c], __fdiv_rn(xp[e], d));
  }
}

}  // namespace

int launch_l2_normalize_scale(const float* x, float* y, const float* weight, int64_t n, int c, int h, int w, int64_t x_stride,
                              int64_t y_stride, float eps, hipStream_t s) {
  L2Args a = {};
  a.x = x, a.y = y, a.weight = weight, a.x_stride = x_stride, a.y_stride = y_stride;
  a.c = c, a.hw = h * w, a.blocks_per_image = (int)l2_normalize_blocks(a.hw), a.eps = eps;
  hipLaunchKernelGGL(k_l2_normalize_scale, dim3((unsigned)(n * a.blocks_per_image)), dim3(kL2Threads), 0, s, a);
  return check_launch("k_l2_normalize_scale");
}

}  // namespace mv
