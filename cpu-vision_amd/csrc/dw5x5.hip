// dw5x5.hip -- depthwise 5x5 + folded norm + activation for MobileNetV3's blocks (models/mobilenetv3.py: 11 of large's 15 blocks and
// 8 of small's 11 use kernel 5) on gfx950, in the shape of convnorm.hip's k_dwpc3x3:
//   thread = 4 consecutive output pixels x a strip of `rows` output rows of one plane.  The five input rows of the window roll through
//   registers -- one new row per output row at stride 1, two at stride 2 -- as 8 (stride 1) or 11 (stride 2) columns each.
// Arithmetic = oracle/oracle.c::orc_conv2d_affine_act_f32 with groups = c, bit for bit: one float32 accumulator per output fed by fmaf
// in ascending (ky, kx) order from +0, the padding taps through the same chain as zeros, then mv_epilogue.h's `+ bias` -> folded
// norm -> `residual + v` -> activation.
//
// Loads: the columns a thread needs, ox0 * STRIDE - 2 .. + 7 | 10, lie inside the three (stride 1) or four (stride 2) quads that
// start at column ox0 * STRIDE - 4, a multiple of 4.  A quad that lies inside the row is ONE 16-byte load -- gfx950's global loads
// need dword alignment only, so the same instruction serves rows that are 16-byte aligned (W a multiple of 4 on an aligned x) and
// rows that are not (7- and 14-pixel maps, an x at a 4-byte offset); a quad that crosses an end of the row is read element by
// element under its bounds.  Either way a register holds x[iy][ix] or +0: the two ways cannot differ in a bit.
//
// DIL = 2 (the dilated blocks of MobileNetV3 as a segmentation backbone: kernel 5, dilation 2, stride 1, padding 4 -- the one dilated
// geometry): acc = fmaf(w[ky][kx], x[oy - 4 + 2 ky][ox - 4 + 2 kx], acc) in the same order.  The columns of a thread's 4 outputs,
// ox0 - 4 .. ox0 + 7, are exactly the three quads of stride 1; output j, tap kx reads register j + 2 kx.  A strip walks the output
// rows of ONE PARITY of a block of 2 * rows rows (oy0, oy0 + 2, ...), so that the five input rows oy - 4, oy - 2, .., oy + 4 roll
// through the registers as at dilation 1: a strip is a (row block, parity) pair, strip index 2 * block + parity.
#include "mv_common.h"
#include "mv_epilogue.h"

namespace mv {
namespace {

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));  // dword-aligned 16-byte access

struct Dw5Args {
  const float* x;
  const float* w;  // [c][5][5]
  float* y;
  Epilogue e;
  long long total;  // planes * strips * groups_x
  int c, h, wd, oh, ow;
  int rows, strips, groups_x;  // DIL = 2: rows per parity of a row block; strips = 2 * row blocks
};

// DIL = 2 asks for 4 workgroups per CU (4 waves per SIMD): left alone the instance takes 130 VGPRs, two above that occupancy; the
// dilation-1 instances keep the allocation they had (125 and 142 VGPRs)
template <int STRIDE, int DIL = 1>
__global__ __launch_bounds__(256, DIL == 2 ? 4 : 1) void k_dwpc5x5(const Dw5Args A) {
  static_assert(DIL == 1 || (DIL == 2 && STRIDE == 1), "the dilated geometry is kernel 5, dilation 2, stride 1");
  constexpr int NQ = 2 + STRIDE;  // quads per row: columns ox0 * STRIDE - 4 .. + 4 NQ - 1
  constexpr int NC = 4 * NQ;
  constexpr int B0 = DIL == 1 ? 2 : 0;  // output j, tap kx reads r[B0 + j * STRIDE + kx * DIL]
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= A.total) return;
  const int gx = (int)(idx % A.groups_x);
  const long long t = idx / A.groups_x;
  const int st = (int)(t % A.strips);
  const long long plane = t / A.strips;
  const int ch = (int)(plane % A.c);
  const int H = A.h, W = A.wd, OW = A.ow;
  const float* xp = A.x + (size_t)plane * H * W;
  float* yp = A.y + (size_t)plane * A.oh * OW;
  const float* rp = A.e.res ? A.e.res + (size_t)plane * A.oh * OW : nullptr;
  const int ox0 = 4 * gx, c0 = ox0 * STRIDE - 4;  // r[i] holds column c0 + i
  const int blk0 = (DIL == 1 ? st : st >> 1) * (A.rows * DIL);  // first row of the strip's row block
  const int oy0 = blk0 + (DIL == 1 ? 0 : st & 1), oy1 = min(blk0 + A.rows * DIL, A.oh);
  if (DIL > 1 && oy0 >= oy1) return;  // the odd-parity strip of a last block of one row

  float wk[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) wk[i] = A.w[(size_t)ch * 25 + i];
  const ChannelTerms ct = channel_terms(A.e, ch);
  const Clamp cl = make_clamp(A.e.act);

  auto load_row = [&](int iy, float (&r)[NC]) {
#pragma unroll
    for (int i = 0; i < NC; ++i) r[i] = 0.f;
    if (iy < 0 || iy >= H) return;
    const float* row = xp + (size_t)iy * W;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
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

  float r0[NC], r1[NC], r2[NC], r3[NC], r4[NC];
  load_row(oy0 * STRIDE - 2 * DIL, r0);
  load_row(oy0 * STRIDE - DIL, r1);
  load_row(oy0 * STRIDE, r2);
  load_row(oy0 * STRIDE + DIL, r3);
  for (int oy = oy0; oy < oy1; oy += DIL) {
    load_row(oy * STRIDE + 2 * DIL, r4);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = B0 + j * STRIDE;
      float acc = 0.f;
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) acc = fmaf(wk[kx], r0[b + kx * DIL], acc);
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) acc = fmaf(wk[5 + kx], r1[b + kx * DIL], acc);
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) acc = fmaf(wk[10 + kx], r2[b + kx * DIL], acc);
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) acc = fmaf(wk[15 + kx], r3[b + kx * DIL], acc);
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) acc = fmaf(wk[20 + kx], r4[b + kx * DIL], acc);
      v[j] = epi_norm(acc, ct, A.e);
    }
    const size_t o = (size_t)oy * OW + ox0;
    if (rp) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (ox0 + j < OW) v[j] = rp[o + j] + v[j];
    }
    if (A.e.act >= 3) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (A.e.act == 3) ? epi_act<1>(v[j], cl) : epi_act<2>(v[j], cl);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = epi_act<0>(v[j], cl);
    }
    if (ox0 + 3 < OW) {
      *reinterpret_cast<f32x4u*>(yp + o) = (f32x4u){v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (ox0 + j < OW) yp[o + j] = v[j];
    }
    if (STRIDE == 1) {
#pragma unroll
      for (int i = 0; i < NC; ++i) r0[i] = r1[i], r1[i] = r2[i], r2[i] = r3[i], r3[i] = r4[i];
    } else {
#pragma unroll
      for (int i = 0; i < NC; ++i) r0[i] = r2[i], r1[i] = r3[i], r2[i] = r4[i];
      load_row(oy * STRIDE + 3, r3);
    }
  }
}

}  // namespace

int launch_dwpc5x5(const float* x, const float* w, float* y, int64_t n, int c, int h, int wd, int stride, int dilation,
                   const Epilogue& e, hipStream_t s) {
  Dw5Args a = {};
  a.x = x, a.w = w, a.y = y, a.e = e;
  a.c = c, a.h = h, a.wd = wd;
  a.oh = (h - 1) / stride + 1, a.ow = (wd - 1) / stride + 1;
  a.groups_x = (a.ow + 3) / 4;
  // strip height: kDw5Rows rows amortise the four halo rows (12 row loads for 8 outputs rows at stride 1); launches that would leave
  // the chip short of threads (the 14- and 7-pixel maps at batch 1) take half
  const long long planes = (long long)n * c;
  // dilation 2 (stride 1): a row block is 2 * rows output rows, one strip per parity -- the same rule on its strip count
  auto strips_of = [&](int rows) { return dilation * ((a.oh + dilation * rows - 1) / (dilation * rows)); };
  a.rows = kDw5Rows;
  if (planes * strips_of(a.rows) * a.groups_x < kDw5ShortLaunch) a.rows = kDw5Rows / 2;
  a.strips = strips_of(a.rows);
  a.total = planes * a.strips * a.groups_x;
  if (a.total > 256LL * 0x7fffffffLL) return set_error(MV_ERR_UNSUPPORTED, "depthwise 5x5: batch too large for one launch");
  if (a.total == 0) return MV_OK;
  const unsigned nb = (unsigned)((a.total + 255) / 256);
  if (dilation == 2) {
    hipLaunchKernelGGL((k_dwpc5x5<1, 2>), dim3(nb), dim3(256), 0, s, a);
    return check_launchf("k_dwpc5x5<s1,d2,rows%d>", a.rows);
  }
  if (stride == 1)
    hipLaunchKernelGGL((k_dwpc5x5<1>), dim3(nb), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((k_dwpc5x5<2>), dim3(nb), dim3(256), 0, s, a);
  return check_launchf("k_dwpc5x5<s%d,rows%d>", stride, a.rows);
}

}  // namespace mv
