// mask.hip -- the mask branch of Mask R-CNN after the predictor (models/detection/roi_heads.py): maskrcnn_inference as one gather +
// sigmoid, and paste_masks_in_image as ONE pass that writes the (R, 1, H, W) result once, zeros included.  The reference loops over
// the detections in Python: per mask an expand, an interpolate, a zeros((H, W)), a slice assignment with the box read back to the
// host, then a stack -- the output is written twice and read once.
//
// k_paste_masks  a workgroup is 4 waves, each owning kPasteRowsPerWave consecutive output rows; a lane owns 4 consecutive output x.
//                The flat workgroup index gives (roi, row block, column block) with scalar divisions.  The roi's four floats are read
//                through that uniform index and expand_boxes and the truncation run in registers.  A wave whose columns, or a row
//                that, lies wholly outside the box stores zeros and computes nothing (most of the output); inside, the taps of the
//                zero-padded mask are plain global loads of the unpadded one (3 KB per roi: it stays in the caches), a tap in the
//                padding ring is +0.0.  16-byte stores when the row pitch is a multiple of 4 and the base is 16-byte aligned, else
//                element by element.  Element offsets are 64-bit.
// k_mask_probs   one lane per output element: the roi's label through its index, the selected plane's logit, sigmoid_cr.
//
// Arithmetic (mi355vision.h, mv_paste_masks_f32 / mv_mask_probs_f32): every operation is written with __f*_rn, one rounding each;
// the interpolation is k_interp_batch's (mv_bilinear.h).
#include "mv_bilinear.h"
#include "mv_boxcoder.h"
#include "mv_common.h"

namespace mv {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPasteRowsPerWave = 4;
constexpr int kPasteRowsPerBlock = 4 * kPasteRowsPerWave;  // 4 waves
constexpr int kPasteColsPerBlock = kWave * 4;              // 256 output x per wave

struct PasteArgs {
  const float* masks;  // (r, m, m)
  const float* boxes;  // (r, 4)
  float* y;            // (r, h, w)
  int m, pad, h, w;
  float scale;         // float32((double)(m + 2 pad) / m)
  unsigned xblocks, rblocks;
};

template <bool VEC>
__device__ inline void store4(float* out, const float (&v)[4], int x0, int w) {
  if (VEC) {  // w % 4 == 0: x0 + 3 < w
    *reinterpret_cast<f32x4*>(out) = (f32x4){v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < w) out[j] = v[j];
  }
}

template <bool VEC>
__global__ __launch_bounds__(kWave * 4) void k_paste_masks(const PasteArgs A) {
  const unsigned xb = blockIdx.x % A.xblocks, t = blockIdx.x / A.xblocks;
  const unsigned rb = t % A.rblocks, roi = t / A.rblocks;
  const int x0 = (int)(xb * kPasteColsPerBlock + threadIdx.x * 4);
  const int yw = (int)(rb * kPasteRowsPerBlock + threadIdx.y * kPasteRowsPerWave);  // the wave's first row
  if (x0 >= A.w || yw >= A.h) return;

  // expand_boxes and .to(int64) of this roi, in registers (uniform over the workgroup)
  const float* const b = A.boxes + (size_t)roi * 4;
  const float bx1f = b[0], by1f = b[1], bx2f = b[2], by2f = b[3];
  const float wh = __fmul_rn(__fmul_rn(__fsub_rn(bx2f, bx1f), 0.5f), A.scale);
  const float hh = __fmul_rn(__fmul_rn(__fsub_rn(by2f, by1f), 0.5f), A.scale);
  const float xc = __fmul_rn(__fadd_rn(bx2f, bx1f), 0.5f), yc = __fmul_rn(__fadd_rn(by2f, by1f), 0.5f);
  const float e0 = __fsub_rn(xc, wh), e1 = __fsub_rn(yc, hh), e2 = __fadd_rn(xc, wh), e3 = __fadd_rn(yc, hh);
  const float lim = 1073741824.f;  // 2^30; a NaN fails every comparison
  const bool ok = fabsf(e0) < lim && fabsf(e1) < lim && fabsf(e2) < lim && fabsf(e3) < lim;
  const int bx0 = ok ? (int)e0 : 0, by0 = ok ? (int)e1 : 0, bx1 = ok ? (int)e2 : -1, by1 = ok ? (int)e3 : -1;
  const int bw = max(bx1 - bx0 + 1, 1), bh = max(by1 - by0 + 1, 1);
  const int cx0 = max(bx0, 0), cx1 = ok ? min(bx1 + 1, A.w) : 0;  // the columns and rows the roi writes: [cx0, cx1) x [cy0, cy1)
  const int cy0 = max(by0, 0), cy1 = ok ? min(by1 + 1, A.h) : 0;

  float* const plane = A.y + (size_t)roi * A.h * A.w;
  const float zero[4] = {0.f, 0.f, 0.f, 0.f};
  const int xw = (int)(xb * kPasteColsPerBlock);  // the wave's first column
  const bool wave_cols_in = xw < cx1 && xw + kPasteColsPerBlock > cx0;
  const bool lane_cols_in = x0 < cx1 && x0 + 4 > cx0;
  const int in = A.m + 2 * A.pad;
  float sy = 0.f, sx = 0.f;
  BilinearTap tx[4] = {};
  if (wave_cols_in && yw < cy1 && yw + kPasteRowsPerWave > cy0) {  // wave-uniform: some row of the wave meets the box
    sy = __fdiv_rn((float)in, (float)bh), sx = __fdiv_rn((float)in, (float)bw);
    if (lane_cols_in) {
#pragma unroll
      for (int j = 0; j < 4; ++j) tx[j] = bilinear_tap(x0 + j - bx0, sx, in);
    }
  }
  const float* const mk = A.masks + (size_t)roi * A.m * A.m;
  const int M = A.m, P = A.pad;
  for (int i = 0; i < kPasteRowsPerWave; ++i) {
    const int y = yw + i;
    if (y >= A.h) break;
    float* const out = plane + (size_t)y * A.w + x0;
    if (!(wave_cols_in && y >= cy0 && y < cy1)) {  // wave-uniform: store only
      store4<VEC>(out, zero, x0, A.w);
      continue;
    }
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (lane_cols_in) {
      const BilinearTap ty = bilinear_tap(y - by0, sy, in);
      const int r0 = ty.i0 - P, r1 = ty.i1 - P;  // rows of the unpadded mask
      const bool r0in = r0 >= 0 && r0 < M, r1in = r1 >= 0 && r1 < M;
      const float* const m0 = mk + (size_t)(r0in ? r0 : 0) * M;
      const float* const m1 = mk + (size_t)(r1in ? r1 : 0) * M;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        if (x >= cx0 && x < cx1) {
          const int c0 = tx[j].i0 - P, c1 = tx[j].i1 - P;
          const bool c0in = c0 >= 0 && c0 < M, c1in = c1 >= 0 && c1 < M;
          const int k0 = c0in ? c0 : 0, k1 = c1in ? c1 : 0;
          const float a = (r0in && c0in) ? m0[k0] : 0.f, bb = (r0in && c1in) ? m0[k1] : 0.f;
          const float c = (r1in && c0in) ? m1[k0] : 0.f, d = (r1in && c1in) ? m1[k1] : 0.f;
          const float top = __fmaf_rn(tx[j].w0, a, __fmul_rn(tx[j].w1, bb));
          const float bot = __fmaf_rn(tx[j].w0, c, __fmul_rn(tx[j].w1, d));
          v[j] = __fmaf_rn(ty.w0, top, __fmul_rn(ty.w1, bot));
        }
      }
    }
    store4<VEC>(out, v, x0, A.w);
  }
}

struct ProbsArgs {
  const float* logits;    // (r, classes, plane)
  const int64_t* labels;  // (r)
  float* y;               // (r, plane)
  long long total, plane;
  int classes;
};

__global__ __launch_bounds__(256) void k_mask_probs(const ProbsArgs A) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= A.total) return;
  const long long roi = idx / A.plane, p = idx - roi * A.plane;
  const long long label = A.labels[roi];
  float v = 0.f;
  if (label >= 0 && label < A.classes) v = sigmoid_cr(A.logits[((size_t)roi * A.classes + (size_t)label) * A.plane + p]);
  A.y[idx] = v;
}

}  // namespace

bool paste_masks_grid_fits(int64_t r, int h, int w) {
  const int64_t xblocks = ((int64_t)w + kPasteColsPerBlock - 1) / kPasteColsPerBlock;
  const int64_t rblocks = ((int64_t)h + kPasteRowsPerBlock - 1) / kPasteRowsPerBlock;
  return r <= 0x7fffffffLL / (xblocks * rblocks);
}

int launch_paste_masks(const float* masks, const float* boxes, float* y, int64_t r, int m, int padding, int h, int w, hipStream_t s) {
  PasteArgs a = {};
  a.masks = masks, a.boxes = boxes, a.y = y, a.m = m, a.pad = padding, a.h = h, a.w = w;
  a.scale = (float)((double)(m + 2 * padding) / (double)m);
  a.xblocks = (unsigned)((w + kPasteColsPerBlock - 1) / kPasteColsPerBlock);
  a.rblocks = (unsigned)((h + kPasteRowsPerBlock - 1) / kPasteRowsPerBlock);
  const bool vec = w % 4 == 0 && (uintptr_t)y % 16 == 0;
  const dim3 grid((unsigned)(r * a.rblocks * a.xblocks)), block(kWave, 4);
  if (vec) hipLaunchKernelGGL(k_paste_masks<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_paste_masks<false>, grid, block, 0, s, a);
  return check_launchf("k_paste_masks<%s>", vec ? "vec16" : "scalar");
}

bool mask_probs_grid_fits(int64_t r, int64_t plane) { return r <= (256LL * 0x7fffffffLL) / plane; }

int launch_mask_probs(const float* logits, const int64_t* labels, float* y, int64_t r, int classes, int64_t plane, hipStream_t s) {
  ProbsArgs a = {};
  a.logits = logits, a.labels = labels, a.y = y, a.total = r * plane, a.plane = plane, a.classes = classes;
  hipLaunchKernelGGL(k_mask_probs, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, s, a);
  return check_launch("k_mask_probs");
}

}  // namespace mv
