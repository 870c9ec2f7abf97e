// mv_gridsample.h -- the per-pixel core of grid_sample(mode, padding_mode="zeros", align_corners=False) and the v2 fill
// blend of `_apply_grid_transform` (transforms/v2/functional/_geometry.py), shared by k_elastic (elastic.hip) and k_warp
// (warp.hip).  The arithmetic is ATen's vectorised CPU grid_sampler per pixel, so the results are its bits (DESIGN.md
// sections 3.13 / 3.14).  The caller supplies the sample position in input pixels, xs = fma(gx + 1, W / 2, -0.5) (the same
// for ys), and walks the planes; this header turns the position into corner offsets, weights and in-bounds bits once per
// pixel (`setup`), the fill mask (`fill_mask`), and one plane's value (`sample`):
//   bilinear  x0 = floor(x), w = x - x0, e = 1 - w (n, s for y);  nw = s*e, ne = s*w, sw = n*e, se = n*w
//             acc = v_nw*nw; acc = fma(v_ne, ne, acc); acc = fma(v_sw, sw, acc); acc = fma(v_se, se, acc)
//             (a corner outside the image has value 0 and is never loaded: clamped address, selected 0)
//             fill: m = the same chain over the in-bounds indicators; out = ((acc - fill) * m) + fill
//   nearest   the corner at (rint(y), rint(x)) (half to even) or 0; fill: an out-of-frame sample is fill
//   uint8     computed in fp32, rounded half to even, narrowed (narrow<T>).
// PAIR (bilinear, w >= 2): each corner row is ONE 2-element load (columns x0, x0 + 1, clamped into the row), 2 gathers per
// pixel and plane instead of 4.
#pragma once

#include "mv_common.h"

namespace mv {
namespace gs {

constexpr int kMaxFill = 16;  // fill values by value in the kernel arguments (per channel; a scalar fill is 1 channel)

struct Fill {
  float v[kMaxFill];
};

template <typename T>
__device__ inline float load_f(const T* p) { return (float)*p; }

template <typename T>
__device__ inline T narrow(float v);
template <>
__device__ inline float narrow<float>(float v) { return v; }
template <>
__device__ inline uint8_t narrow<uint8_t>(float v) { return round_u8(v); }

// the 2-element corner pair at p[0], p[1] (x0 and x0 + 1 of one row) as one load where the target allows it
template <typename T>
__device__ inline void load_pair(const T* p, float& a, float& b) {
  struct alignas(sizeof(T)) Pair { T v[2]; } q;
  __builtin_memcpy(&q, p, sizeof(q));
  a = (float)q.v[0], b = (float)q.v[1];
}

// One pixel's sample position (xs, ys) in an h x w plane -> corner offsets in the plane (clamped: always a legal address)
// and weights, with the out-of-bounds corners zeroed through the in-bounds bits (bit 0..3 = nw, ne, sw, se; nearest: bit 0;
// PAIR: bits 4 / 5 take the pair's first element for nw / ne).
template <bool NEAREST, bool PAIR>
__device__ inline void setup(float xs, float ys, int h, int w, int off[4], float wt[4], unsigned& inb) {
  const float fw = (float)w, fh = (float)h;
  if (NEAREST) {
    // clamp before the int conversion: far-out samples (and NaN) become out-of-bounds indices, never UB
    const int ix = (int)__builtin_fminf(__builtin_fmaxf(__builtin_rintf(xs), -1.f), fw);
    const int iy = (int)__builtin_fminf(__builtin_fmaxf(__builtin_rintf(ys), -1.f), fh);
    inb = (ix >= 0 && ix < w && iy >= 0 && iy < h) ? 1u : 0u;
    const int cx = ix < 0 ? 0 : (ix >= w ? w - 1 : ix), cy = iy < 0 ? 0 : (iy >= h ? h - 1 : iy);
    off[0] = cy * w + cx;
  } else {
    const float x0 = __builtin_floorf(xs), y0 = __builtin_floorf(ys);
    const float ww = xs - x0, ee = 1.f - ww, nn = ys - y0, ss = 1.f - nn;
    wt[0] = ss * ee, wt[1] = ss * ww, wt[2] = nn * ee, wt[3] = nn * ww;
    const int ix = (int)__builtin_fminf(__builtin_fmaxf(x0, -2.f), fw);
    const int iy = (int)__builtin_fminf(__builtin_fmaxf(y0, -2.f), fh);
    const bool in_x0 = ix >= 0 && ix < w, in_x1 = ix + 1 >= 0 && ix + 1 < w;
    const bool in_y0 = iy >= 0 && iy < h, in_y1 = iy + 1 >= 0 && iy + 1 < h;
    inb = (in_y0 && in_x0 ? 1u : 0u) | (in_y0 && in_x1 ? 2u : 0u) | (in_y1 && in_x0 ? 4u : 0u) | (in_y1 && in_x1 ? 8u : 0u);
    const int cx0 = ix < 0 ? 0 : (ix >= w ? w - 1 : ix), cx1 = ix + 1 < 0 ? 0 : (ix + 1 >= w ? w - 1 : ix + 1);
    const int cy0 = iy < 0 ? 0 : (iy >= h ? h - 1 : iy), cy1 = iy + 1 < 0 ? 0 : (iy + 1 >= h ? h - 1 : iy + 1);
    if (PAIR) {
      // pair start px in [0, w - 2]: ix == px -> (nw, ne) = (a, b); ix == -1 -> ne = a; ix == w - 1 -> nw = b (the corner
      // outside the row is masked out anyway)
      const int px = ix < 0 ? 0 : (ix > w - 2 ? w - 2 : ix);
      inb |= (ix == px ? 16u : 0u) | (ix + 1 == px ? 32u : 0u);
      off[0] = cy0 * w + px, off[2] = cy1 * w + px;
    } else {
      off[0] = cy0 * w + cx0, off[1] = cy0 * w + cx1, off[2] = cy1 * w + cx0, off[3] = cy1 * w + cx1;
    }
  }
}

// the fill mask of a bilinear pixel: the resampled ones-channel of the reference (independent of the plane)
__device__ inline float fill_mask(const float wt[4], unsigned inb) {
  float m = (inb & 1u ? 1.f : 0.f) * wt[0];
  m = __builtin_fmaf(inb & 2u ? 1.f : 0.f, wt[1], m);
  m = __builtin_fmaf(inb & 4u ? 1.f : 0.f, wt[2], m);
  return __builtin_fmaf(inb & 8u ? 1.f : 0.f, wt[3], m);
}

// one plane's output value of the pixel (before narrowing); f = the plane's fill value, msk = fill_mask (FILL && !NEAREST)
template <typename T, bool NEAREST, bool FILL, bool PAIR>
__device__ inline float sample(const T* src, const int off[4], const float wt[4], unsigned inb, float msk, float f) {
  if (NEAREST) {
    const float v = load_f(src + off[0]);
    return FILL ? (inb ? v : f) : (inb ? v : 0.f);
  }
  float v0, v1, v2, v3;
  if (PAIR) {
    float a0, b0, a1, b1;
    load_pair(src + off[0], a0, b0);
    load_pair(src + off[2], a1, b1);
    v0 = inb & 16u ? a0 : b0, v1 = inb & 32u ? a0 : b0;
    v2 = inb & 16u ? a1 : b1, v3 = inb & 32u ? a1 : b1;
  } else {
    v0 = load_f(src + off[0]), v1 = load_f(src + off[1]);
    v2 = load_f(src + off[2]), v3 = load_f(src + off[3]);
  }
  float acc = (inb & 1u ? v0 : 0.f) * wt[0];
  acc = __builtin_fmaf(inb & 2u ? v1 : 0.f, wt[1], acc);
  acc = __builtin_fmaf(inb & 4u ? v2 : 0.f, wt[2], acc);
  acc = __builtin_fmaf(inb & 8u ? v3 : 0.f, wt[3], acc);
  if (FILL) acc = ((acc - f) * msk) + f;  // three roundings (sub_, mul_, add_): -ffp-contract=off keeps them apart
  return acc;
}

// Plane chunks for a launch of `tiles` workgroup tiles: at least ~2048 workgroups (8 per CU) when the frame alone gives
// fewer, so the planes go to several workgroups per tile.  false: the grid does not fit the launch limits.
inline bool plan_chunks(long long tiles, long long planes, long long& chunks, long long& chunk_planes) {
  chunks = (2048 + tiles - 1) / tiles;
  if (chunks > planes) chunks = planes;
  if (chunks < 1) chunks = 1;
  chunk_planes = (planes + chunks - 1) / chunks;
  chunks = (planes + chunk_planes - 1) / chunk_planes;
  return tiles * chunks <= 0x7fffffffLL && chunk_planes <= 0x7fffffffLL;
}

}  // namespace gs
}  // namespace mv
