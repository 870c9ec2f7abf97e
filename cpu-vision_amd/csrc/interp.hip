// interp.hip -- torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=False) on planar float32, and the
// front end of a detection model (models/detection/transform.py: normalize -> resize -> batch_images) as ONE pass: every source image
// is read once and the padded batch tensor is written once, padding included.  The reference makes four passes over the pixels
// (sub / div, interpolate, new_full, a copy_ per image).
//
// k_interp_batch  a workgroup is 4 waves, one output row each; a lane owns 4 consecutive output x of its row.  The flat workgroup
//                 index gives (plane, row block, column block) with scalar divisions; plane = image * channels + channel, and the
//                 image's entry of the by-value table (pointer, sizes, scales) is read through that uniform index.  The vertical
//                 index and weight are computed once per lane, the four horizontal ones in registers; the taps are plain global
//                 loads (neighbouring lanes share them, the caches serve an upscale).  Outside the image's (oh, ow) the lane
//                 writes +0.0.  The four values go out as one 16-byte store when the row pitch is a multiple of 4 and the base is
//                 16-byte aligned, else element by element.  Element offsets are 64-bit.
//
// Arithmetic (mi355vision.h, mv_interpolate_bilinear_f32): every product and every fma is written with __fmul_rn / __fmaf_rn, one
// rounding each; NORM normalises each tap first as (x - mean[c]) / std[c], the subtraction rounded, the division correctly rounded
// (k_to_float_normalize's arithmetic), so the fused result has the bits of normalize -> interpolate -> batch_images.
#include "mv_bilinear.h"
#include "mv_common.h"

namespace mv {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRowsPerBlock = 4;                 // one wave per row
constexpr int kColsPerBlock = kWave * 4;         // 256 output x per wave

struct DetImage {
  const float* x;  // (c, h, w)
  int h, w, oh, ow;
  float sy, sx;    // float32(h) / float32(oh), float32(w) / float32(ow)
};

struct InterpArgs {
  DetImage img[kMaxDetImages];
  float* y;             // (n, c, hp, wp)
  unsigned c;           // channels per image
  int hp, wp;
  unsigned xblocks, rblocks;
  int vec;              // 16-byte stores
  float mean[16], stdv[16];
};

template <bool NORM>
__global__ __launch_bounds__(kWave * kRowsPerBlock) void k_interp_batch(const InterpArgs A) {
  const unsigned xb = blockIdx.x % A.xblocks, t = blockIdx.x / A.xblocks;
  const unsigned rb = t % A.rblocks, plane = t / A.rblocks;
  const unsigned n = plane / A.c, ch = plane - n * A.c;
  const int y = (int)(rb * kRowsPerBlock + threadIdx.y), x0 = (int)(xb * kColsPerBlock + threadIdx.x * 4);
  if (y >= A.hp || x0 >= A.wp) return;
  const DetImage I = A.img[n];
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (y < I.oh && x0 < I.ow) {
    const BilinearTap ty = bilinear_tap(y, I.sy, I.h);
    const float* const r0 = I.x + ((size_t)ch * I.h + ty.i0) * I.w;
    const float* const r1 = I.x + ((size_t)ch * I.h + ty.i1) * I.w;
    const float m = NORM ? A.mean[ch] : 0.f, sd = NORM ? A.stdv[ch] : 1.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (x0 + j < I.ow) {
        const BilinearTap tx = bilinear_tap(x0 + j, I.sx, I.w);
        float a = r0[tx.i0], b = r0[tx.i1], c = r1[tx.i0], d = r1[tx.i1];
        if (NORM) {
          a = __fdiv_rn(__fsub_rn(a, m), sd), b = __fdiv_rn(__fsub_rn(b, m), sd);
          c = __fdiv_rn(__fsub_rn(c, m), sd), d = __fdiv_rn(__fsub_rn(d, m), sd);
        }
        const float top = __fmaf_rn(tx.w0, a, __fmul_rn(tx.w1, b));
        const float bot = __fmaf_rn(tx.w0, c, __fmul_rn(tx.w1, d));
        v[j] = __fmaf_rn(ty.w0, top, __fmul_rn(ty.w1, bot));
      }
    }
  }
  float* const out = A.y + ((size_t)plane * A.hp + y) * A.wp + x0;
  if (A.vec) {  // wp % 4 == 0: x0 + 3 < wp
    *reinterpret_cast<f32x4*>(out) = (f32x4){v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < A.wp) out[j] = v[j];
  }
}

}  // namespace

bool interp_grid_fits(int64_t planes, int hp, int wp) {
  const int64_t xblocks = ((int64_t)wp + kColsPerBlock - 1) / kColsPerBlock, rblocks = ((int64_t)hp + kRowsPerBlock - 1) / kRowsPerBlock;
  return planes <= 0x7fffffffLL / (xblocks * rblocks);
}

int launch_interp_batch(const float* const* xs, const int* hs, const int* ws, const int* ohs, const int* ows, int n, int c,
                        const float* mean, const float* stdv, float* y, int hp, int wp, hipStream_t s) {
  InterpArgs a = {};
  for (int i = 0; i < n; ++i) {
    DetImage& d = a.img[i];
    d.x = xs[i], d.h = hs[i], d.w = ws[i], d.oh = ohs[i], d.ow = ows[i];
    d.sy = (float)hs[i] / (float)ohs[i], d.sx = (float)ws[i] / (float)ows[i];
  }
  const bool norm = mean != nullptr;
  for (int i = 0; norm && i < c; ++i) a.mean[i] = mean[i], a.stdv[i] = stdv[i];
  a.y = y, a.c = (unsigned)c, a.hp = hp, a.wp = wp;
  a.xblocks = (unsigned)((wp + kColsPerBlock - 1) / kColsPerBlock), a.rblocks = (unsigned)((hp + kRowsPerBlock - 1) / kRowsPerBlock);
  a.vec = wp % 4 == 0 && (uintptr_t)y % 16 == 0;
  const dim3 grid((unsigned)((int64_t)n * c * a.rblocks * a.xblocks)), block(kWave, kRowsPerBlock);
  if (norm) hipLaunchKernelGGL(k_interp_batch<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_interp_batch<false>, grid, block, 0, s, a);
  return check_launchf("k_interp_batch<%s,%s>", norm ? "norm" : "plain", a.vec ? "vec16" : "scalar");
}

}  // namespace mv
