// keypoint.hip -- the keypoint branch of Keypoint R-CNN after the predictor (models/detection/roi_heads.py heatmaps_to_keypoints) as
// ONE launch.  The reference loops over the detections in Python: per roi two .item() read-backs, a bicubic interpolate of the
// (K, Mh, Mw) heatmaps to the roi's (ceil(h), ceil(w)) -- as large as the image --, an argmax, index arithmetic and a gather.  Here
// the resized map is never materialised: a workgroup owns one (roi, keypoint) pair, evaluates the resize where it needs it and keeps
// only the running maximum.
//
// k_heatmaps_to_keypoints   one workgroup of 4 waves per (roi, keypoint).  The roi's four floats are read through the uniform index;
//                a roi outside the domain stores its zero row and reads nothing else.  The heatmap (56 x 56: 12.25 KiB) is staged
//                once in LDS.  Wave v sweeps the output rows [v * ceil(rh / 4), ...); a lane owns the output columns lane, lane + 64,
//                ... and walks its wave's rows.  The interpolation is separable with identical bits -- u[r][x] = sum_j wx_j *
//                src[r, x_j] depends only on the source row r and the output column x --, so the lane keeps the four u of the
//                current row window and computes one new u (4 LDS reads, 4 multiplies) when the window moves down by one source row,
//                all four when it jumps (downsampling).  The row taps and weights are wave-uniform.  Every lane keeps its (value,
//                flat index) maximum; the pairs are reduced with cross-lane shuffles, then across the waves through LDS.  The pair
//                order is total -- a NaN beats every number, equal values (and two NaNs) go to the smaller index --, so the result
//                does not depend on how rows and columns were dealt to waves and lanes.
//
// Arithmetic (mi355vision.h, mv_heatmaps_to_keypoints_f32): every operation is written with __f*_rn, one rounding each; the only fma
// is the source coordinate's, as in mv_bilinear.h.
#include <cfloat>

#include "mv_common.h"

namespace mv {
namespace {

constexpr int kKpWaves = 4;
constexpr int kKpMaxRoiSide = 1 << 15;  // a roi's resized map is at most 2^15 on a side: the flat index stays below 2^30

struct KpArgs {
  const float* maps;  // (r, k, mh, mw)
  const float* rois;  // (r, 4)
  float* xy;          // (r, k, 3)
  float* scores;      // (r, k)
  int k, mh, mw;
};

// one axis of interpolate(mode="bicubic", align_corners=False), A = -0.75: the first of the four taps is i0 - 1
struct CubicTap {
  int i0;
  float w[4];
};
__device__ inline float cubic_c1(float x) {  // ((A + 2) x - (A + 3)) x x + 1
  return __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(1.25f, x), 2.25f), x), x), 1.f);
}
__device__ inline float cubic_c2(float x) {  // ((A x - 5 A) x + 8 A) x - 4 A
  return __fsub_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(-0.75f, x), -3.75f), x), -6.f), x), -3.f);
}
__device__ inline CubicTap cubic_tap(int d, float s, int in) {
  const float real = __fmaf_rn(s, (float)d + 0.5f, -0.5f);  // not clamped at 0: i0 = -1 for the first outputs of an upsampling
  CubicTap t;
  t.i0 = min((int)floorf(real), in - 1);
  const float lam = fminf(fmaxf(__fsub_rn(real, (float)t.i0), 0.f), 1.f);
  const float one_lam = __fsub_rn(1.f, lam);
  t.w[0] = cubic_c2(__fadd_rn(lam, 1.f));
  t.w[1] = cubic_c1(lam);
  t.w[2] = cubic_c1(one_lam);
  t.w[3] = cubic_c2(__fadd_rn(one_lam, 1.f));
  return t;
}

// sum_j w_j * v_j: from the first product, the next three added in order
__device__ inline float dot4(const float (&w)[4], float v0, float v1, float v2, float v3) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w[0], v0), __fmul_rn(w[1], v1)), __fmul_rn(w[2], v2)), __fmul_rn(w[3], v3));
}

// the total order of the (value, flat index) pairs: does (v, i) come before (bv, bi)?
__device__ inline bool kp_before(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

__device__ inline bool kp_finite(float v) { return fabsf(v) <= FLT_MAX; }  // false for a NaN

__global__ __launch_bounds__(kWave * kKpWaves) void k_heatmaps_to_keypoints(const KpArgs A) {
  extern __shared__ __attribute__((aligned(16))) float hm[];  // the heatmap; afterwards the waves' (value, index) pairs
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const size_t item = blockIdx.x;  // roi * k + keypoint
  const size_t roi = item / (unsigned)A.k;
  const float* const b = A.rois + roi * 4;
  const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
  const float bw = fmaxf(__fsub_rn(x2, x1), 1.f), bh = fmaxf(__fsub_rn(y2, y1), 1.f);
  float* const xy = A.xy + item * 3;
  if (!(kp_finite(x1) && kp_finite(y1) && kp_finite(x2) && kp_finite(y2) && bw <= (float)kKpMaxRoiSide && bh <= (float)kKpMaxRoiSide)) {
    if (tid == 0) xy[0] = 0.f, xy[1] = 0.f, xy[2] = 0.f, A.scores[item] = 0.f;  // uniform over the workgroup: nothing else is read
    return;
  }
  const int rw = (int)ceilf(bw), rh = (int)ceilf(bh);
  const int mh = A.mh, mw = A.mw, plane = mh * mw;
  const float* const src = A.maps + item * (size_t)plane;
  for (int i = tid; i < plane; i += kWave * kKpWaves) hm[i] = src[i];
  __syncthreads();

  const float sx = __fdiv_rn((float)mw, (float)rw), sy = __fdiv_rn((float)mh, (float)rh);
  const int rows_per_wave = (rh + kKpWaves - 1) / kKpWaves;
  const int ya = wave * rows_per_wave, yb = min(rh, ya + rows_per_wave);
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int x = lane; x < rw; x += kWave) {
    const CubicTap tx = cubic_tap(x, sx, mw);
    const int c0 = min(max(tx.i0 - 1, 0), mw - 1), c1 = min(max(tx.i0, 0), mw - 1);
    const int c2 = min(max(tx.i0 + 1, 0), mw - 1), c3 = min(max(tx.i0 + 2, 0), mw - 1);
    auto urow = [&](int r) {  // u[r][x], r the first-tap-relative row index before clamping
      const float* const row = hm + min(max(r, 0), mh - 1) * mw;
      return dot4(tx.w, row[c0], row[c1], row[c2], row[c3]);
    };
    int cur = -8;  // i0 of the window u[] holds (i0 >= -1)
    float u[4] = {0.f, 0.f, 0.f, 0.f};
    for (int y = ya; y < yb; ++y) {
      const CubicTap ty = cubic_tap(y, sy, mh);  // wave-uniform
      if (ty.i0 != cur) {
        if (ty.i0 == cur + 1) {  // clamp(i0 - 1 + j) of the new window = clamp(i0 + j) of the old one, j < 3
          u[0] = u[1], u[1] = u[2], u[2] = u[3];
        } else {
          u[0] = urow(ty.i0 - 1), u[1] = urow(ty.i0), u[2] = urow(ty.i0 + 1);
        }
        u[3] = urow(ty.i0 + 2);
        cur = ty.i0;
      }
      const float v = dot4(ty.w, u[0], u[1], u[2], u[3]);
      const int idx = y * rw + x;
      if (kp_before(v, idx, bv, bi)) bv = v, bi = idx;
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, kWave);
    const int oi = __shfl_xor(bi, off, kWave);
    if (kp_before(ov, oi, bv, bi)) bv = ov, bi = oi;
  }
  __syncthreads();  // every wave is done with the heatmap
  int* const hmi = reinterpret_cast<int*>(hm);
  if (lane == 0) hm[2 * wave] = bv, hmi[2 * wave + 1] = bi;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int v = 1; v < kKpWaves; ++v)
      if (kp_before(hm[2 * v], hmi[2 * v + 1], bv, bi)) bv = hm[2 * v], bi = hmi[2 * v + 1];
    const int yi = bi / rw, xi = bi - yi * rw;
    const float cx = __fdiv_rn(bw, (float)rw), cy = __fdiv_rn(bh, (float)rh);
    xy[0] = __fadd_rn(__fmul_rn(__fadd_rn((float)xi, 0.5f), cx), x1);
    xy[1] = __fadd_rn(__fmul_rn(__fadd_rn((float)yi, 0.5f), cy), y1);
    xy[2] = 1.f;
    A.scores[item] = bv;
  }
}

}  // namespace

bool heatmaps_to_keypoints_grid_fits(int64_t r, int k) { return r <= 0x7fffffffLL / k; }

int launch_heatmaps_to_keypoints(const float* maps, const float* rois, float* xy, float* scores, int64_t r, int k, int mh, int mw,
                                 hipStream_t s) {
  KpArgs a = {};
  a.maps = maps, a.rois = rois, a.xy = xy, a.scores = scores, a.k = k, a.mh = mh, a.mw = mw;
  const int floats = mh * mw > 2 * kKpWaves ? mh * mw : 2 * kKpWaves;  // at most kKpMaxPlane: 64 KiB
  hipLaunchKernelGGL(k_heatmaps_to_keypoints, dim3((unsigned)(r * k)), dim3(kWave * kKpWaves), (size_t)floats * sizeof(float), s, a);
  return check_launch("k_heatmaps_to_keypoints");
}

}  // namespace mv
