// dw7x7.hip -- depthwise 7x7 + bias for ConvNeXt's blocks (models/convnext.py CNBlock: Conv2d(dim, dim, 7, padding=3, groups=dim,
// bias=True)) on gfx950, in the shape of dw5x5.hip's k_dwpc5x5:
//   thread = 4 consecutive output pixels x a strip of `rows` output rows of one plane.  The seven input rows of the window roll
//   through registers, one new row per output row, as 12 columns each: 84 row registers beside the 49 weights.
// Arithmetic = oracle/oracle.c::orc_conv2d_affine_act_f32 with groups = c, bit for bit: one float32 accumulator per output fed by fmaf
// in ascending (ky, kx) order from +0, the padding taps through the same chain as zeros (never skipped: a NaN or Inf weight reaches
// the border pixels), then `+ bias`.  No norm, no residual, no activation: the block's LayerNorm follows.
//
// Loads: the columns a thread needs, ox0 - 3 .. ox0 + 6, lie inside the three quads that start at column ox0 - 4, a multiple of 4.
// A quad that lies inside the row is ONE 16-byte load -- gfx950's global loads need dword alignment only, so the same instruction
// serves rows that are 16-byte aligned and rows that are not (7- and 14-pixel maps, an x at a 4-byte offset); a quad that crosses an
// end of the row is read element by element under its bounds.  Either way a register holds x[iy][ix] or +0: the two ways cannot
// differ in a bit.
//
// Registers: 7 x 12 row registers + 49 weights + addresses = 168 VGPRs, no scratch, three waves per SIMD -- compiled with
// -fno-slp-vectorize (_build.SOURCE_FLAGS): left to the SLP vectoriser the chains of neighbouring outputs become v_pk_fma_f32 pairs
// whose operands need aligned register pairs, and the allocation grows to 256 VGPRs + 10 AGPRs, one wave per SIMD.
#include "mv_common.h"

namespace mv {
namespace {

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));  // dword-aligned 16-byte access

struct Dw7Args {
  const float* x;
  const float* w;     // [c][7][7]
  const float* bias;  // [c] or null
  float* y;
  long long total;  // planes * strips * groups_x
  int c, h, wd;
  int rows, strips, groups_x;
};

constexpr int kDw7Cols = 12;  // r[i] holds column ox0 - 4 + i; output j, tap kx reads r[1 + j + kx]

__global__ __launch_bounds__(256) void k_dwpc7x7(const Dw7Args A) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= A.total) return;
  const int gx = (int)(idx % A.groups_x);
  const long long t = idx / A.groups_x;
  const int st = (int)(t % A.strips);
  const long long plane = t / A.strips;
  const int ch = (int)(plane % A.c);
  const int H = A.h, W = A.wd;
  const float* xp = A.x + (size_t)plane * H * W;
  float* yp = A.y + (size_t)plane * H * W;
  const int ox0 = 4 * gx, c0 = ox0 - 4;
  const int oy0 = st * A.rows, oy1 = min(oy0 + A.rows, H);

  float wk[49];
#pragma unroll
  for (int i = 0; i < 49; ++i) wk[i] = A.w[(size_t)ch * 49 + i];
  const float bias = A.bias ? A.bias[ch] : 0.f;

  auto load_row = [&](int iy, float (&r)[kDw7Cols]) {
#pragma unroll
    for (int i = 0; i < kDw7Cols; ++i) r[i] = 0.f;
    if (iy < 0 || iy >= H) return;
    const float* row = xp + (size_t)iy * W;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int col = c0 + 4 * q;
      if (col >= 0 && col + 3 < W) {
        const f32x4u a = *reinterpret_cast<const f32x4u*>(row + col);
        r[4 * q] = a.x, r[4 * q + 1] = a.y, r[4 * q + 2] = a.z, r[4 * q + 3] = a.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (col + i >= 0 && col + i < W) r[4 * q + i] = row[col + i];
      }
    }
  };

  float r0[kDw7Cols], r1[kDw7Cols], r2[kDw7Cols], r3[kDw7Cols], r4[kDw7Cols], r5[kDw7Cols], r6[kDw7Cols];
  load_row(oy0 - 3, r0);
  load_row(oy0 - 2, r1);
  load_row(oy0 - 1, r2);
  load_row(oy0, r3);
  load_row(oy0 + 1, r4);
  load_row(oy0 + 2, r5);
  for (int oy = oy0; oy < oy1; ++oy) {
    load_row(oy + 3, r6);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float acc = 0.f;
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) acc = fmaf(wk[kx], r0[1 + j + kx], acc);
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) acc = fmaf(wk[7 + kx], r1[1 + j + kx], acc);
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) acc = fmaf(wk[14 + kx], r2[1 + j + kx], acc);
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) acc = fmaf(wk[21 + kx], r3[1 + j + kx], acc);
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) acc = fmaf(wk[28 + kx], r4[1 + j + kx], acc);
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) acc = fmaf(wk[35 + kx], r5[1 + j + kx], acc);
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) acc = fmaf(wk[42 + kx], r6[1 + j + kx], acc);
      v[j] = A.bias ? acc + bias : acc;
    }
    const size_t o = (size_t)oy * W + ox0;
    if (ox0 + 3 < W) {
      *reinterpret_cast<f32x4u*>(yp + o) = (f32x4u){v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (ox0 + j < W) yp[o + j] = v[j];
    }
#pragma unroll
    for (int i = 0; i < kDw7Cols; ++i) r0[i] = r1[i], r1[i] = r2[i], r2[i] = r3[i], r3[i] = r4[i], r4[i] = r5[i], r5[i] = r6[i];
  }
}

}  // namespace

int launch_dwpc7x7(const float* x, const float* w, const float* bias, float* y, int64_t n, int c, int h, int wd, hipStream_t s) {
  Dw7Args a = {};
  a.x = x, a.w = w, a.bias = bias, a.y = y;
  a.c = c, a.h = h, a.wd = wd;
  a.groups_x = (wd + 3) / 4;
  // strip height: kDw7Rows rows amortise the six halo rows (14 row loads for 8 output rows); launches that would leave the chip
  // short of threads (the 14- and 7-pixel maps at batch 1) take half
  const long long planes = (long long)n * c;
  a.rows = kDw7Rows;
  if (planes * ((h + a.rows - 1) / a.rows) * a.groups_x < kDw7ShortLaunch) a.rows = kDw7Rows / 2;
  a.strips = (h + a.rows - 1) / a.rows;
  a.total = planes * a.strips * a.groups_x;
  if (a.total > 256LL * 0x7fffffffLL) return set_error(MV_ERR_UNSUPPORTED, "depthwise 7x7: batch too large for one launch");
  if (a.total == 0) return MV_OK;
  const unsigned nb = (unsigned)((a.total + 255) / 256);
  hipLaunchKernelGGL(k_dwpc7x7, dim3(nb), dim3(256), 0, s, a);
  return check_launchf("k_dwpc7x7<rows%d>", a.rows);
}

}  // namespace mv
