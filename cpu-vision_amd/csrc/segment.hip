// segment.hip -- the last step of a segmentation model, F.interpolate(mode="bilinear", align_corners=False) of the (n, c, h, w) logits
// followed by argmax over the classes, as ONE pass that writes only the (n, oh, ow) labels.  The composition writes and reads c
// upsampled planes (84 + 84 bytes per pixel at 21 classes) for an 8-byte or 1-byte label, and computes the taps and weights of a
// pixel, which its c planes share, c times.
//
// k_interp_argmax  k_interp_batch's shape: a workgroup is 4 waves, one output row each; a lane owns 4 consecutive output x of its
//                  row.  The flat workgroup index gives (image, row block, column block) with scalar divisions.  The vertical tap
//                  and the four horizontal taps are computed once per lane and stay in registers; the lane then walks the c planes
//                  in ascending order, 16 plain global loads per plane (neighbouring lanes share them; the source of all planes is
//                  small next to the output and is served by the caches), and keeps (best value, best index) per pixel.  A lane
//                  past the ragged end of a row computes the row's last pixel again and stores nothing for it, so the plane loop
//                  has no bounds test.  The four labels go out as one dword (uint8) or two 16-byte stores (int64) when ow is a
//                  multiple of 4 and the base is aligned for them, else element by element.  Element offsets are 64-bit.
//
// Arithmetic (mi355vision.h, mv_interpolate_argmax_f32): the compared values are mv_interpolate_bilinear_f32's (bilinear_tap per
// axis, bilinear_blend); the order is torch.argmax's -- a NaN is greater than every number, equal values (-0.0 and +0.0 among them)
// and later NaNs leave the earlier index in place.
#include "mv_bilinear.h"
#include "mv_common.h"

namespace mv {
namespace {

typedef long long i64x2 __attribute__((ext_vector_type(2)));

constexpr int kRowsPerBlock = 4;          // one wave per row
constexpr int kColsPerBlock = kWave * 4;  // 256 output x per wave

struct ArgmaxArgs {
  const float* x;  // (n, c, h, w)
  void* y;         // (n, oh, ow) of OUT
  int c, h, w, oh, ow;
  float sy, sx;    // float32(h) / float32(oh), float32(w) / float32(ow)
  unsigned xblocks, rblocks;
  int vec;         // one dword / two 16-byte stores per lane
};

template <typename OUT>
__global__ __launch_bounds__(kWave * kRowsPerBlock) void k_interp_argmax(const ArgmaxArgs A) {
  const unsigned xb = blockIdx.x % A.xblocks, t = blockIdx.x / A.xblocks;
  const unsigned rb = t % A.rblocks, n = t / A.rblocks;
  const int y = (int)(rb * kRowsPerBlock + threadIdx.y), x0 = (int)(xb * kColsPerBlock + threadIdx.x * 4);
  if (y >= A.oh || x0 >= A.ow) return;
  const BilinearTap ty = bilinear_tap(y, A.sy, A.h);
  BilinearTap tx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) tx[j] = bilinear_tap(min(x0 + j, A.ow - 1), A.sx, A.w);
  // the 16 taps as byte offsets into a plane (h w 4 < 2^32, checked by the entry point): the plane's base is wave-uniform and
  // advances by one plane per step, the offsets never change
  const unsigned row0 = (unsigned)ty.i0 * (unsigned)A.w, row1 = (unsigned)ty.i1 * (unsigned)A.w;
  unsigned o[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[j][0] = (row0 + (unsigned)tx[j].i0) * 4u, o[j][1] = (row0 + (unsigned)tx[j].i1) * 4u;
    o[j][2] = (row1 + (unsigned)tx[j].i0) * 4u, o[j][3] = (row1 + (unsigned)tx[j].i1) * 4u;
  }
  const size_t plane_bytes = (size_t)A.h * A.w * 4;
  const char* p = reinterpret_cast<const char*>(A.x) + (size_t)n * A.c * plane_bytes;
  const auto tap = [&p](unsigned off) { return *reinterpret_cast<const float*>(p + off); };
  float best[4];
  int arg[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) best[j] = bilinear_blend(ty, tx[j], tap(o[j][0]), tap(o[j][1]), tap(o[j][2]), tap(o[j][3]));
#pragma unroll 3  // 48 loads in flight per lane at 162 VGPRs, 3 waves per SIMD, no scratch (4: 194 VGPRs and 2 waves)
  for (int ch = 1; ch < A.c; ++ch) {
    p += plane_bytes;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = bilinear_blend(ty, tx[j], tap(o[j][0]), tap(o[j][1]), tap(o[j][2]), tap(o[j][3]));
      if (v > best[j] || (v != v && best[j] == best[j])) best[j] = v, arg[j] = ch;  // ascending ch: the first maximum, the first NaN
    }
  }
  OUT* const out = static_cast<OUT*>(A.y) + ((size_t)n * A.oh + y) * A.ow + x0;
  if (A.vec) {  // ow % 4 == 0: x0 + 3 < ow
    if (sizeof(OUT) == 1) {
      *reinterpret_cast<unsigned*>(out) = (unsigned)arg[0] | (unsigned)arg[1] << 8 | (unsigned)arg[2] << 16 | (unsigned)arg[3] << 24;
    } else {
      reinterpret_cast<i64x2*>(out)[0] = (i64x2){arg[0], arg[1]};
      reinterpret_cast<i64x2*>(out)[1] = (i64x2){arg[2], arg[3]};
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < A.ow) out[j] = (OUT)arg[j];
  }
}

}  // namespace

bool interp_argmax_grid_fits(int64_t n, int oh, int ow) {
  const int64_t xblocks = ((int64_t)ow + kColsPerBlock - 1) / kColsPerBlock, rblocks = ((int64_t)oh + kRowsPerBlock - 1) / kRowsPerBlock;
  return n <= 0x7fffffffLL / (xblocks * rblocks);
}

int launch_interp_argmax(const float* x, void* y, int64_t n, int c, int h, int w, int oh, int ow, int out_bytes, hipStream_t s) {
  ArgmaxArgs a = {};
  a.x = x, a.y = y, a.c = c, a.h = h, a.w = w, a.oh = oh, a.ow = ow;
  a.sy = (float)h / (float)oh, a.sx = (float)w / (float)ow;
  a.xblocks = (unsigned)((ow + kColsPerBlock - 1) / kColsPerBlock), a.rblocks = (unsigned)((oh + kRowsPerBlock - 1) / kRowsPerBlock);
  a.vec = ow % 4 == 0 && (uintptr_t)y % (out_bytes == 1 ? 4 : 16) == 0;
  const dim3 grid((unsigned)(n * a.rblocks * a.xblocks)), block(kWave, kRowsPerBlock);
  if (out_bytes == 1) hipLaunchKernelGGL(k_interp_argmax<uint8_t>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_interp_argmax<int64_t>, grid, block, 0, s, a);
  return check_launchf("k_interp_argmax<%s,%s>", out_bytes == 1 ? "u8" : "i64", a.vec ? "vec" : "scalar");
}

}  // namespace mv
