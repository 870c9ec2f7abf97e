// warp.hip -- F.affine / F.rotate / F.perspective (transforms/v2/functional/_geometry.py `affine_image`, `rotate_image`,
// `perspective_image`): grid_sample(mode, padding_mode="zeros", align_corners=False) of every plane at a grid that is a 2 x 3
// (affine) or 3 x 3 (perspective) matrix applied to the output pixel's coordinates, with the v2 fill blend.  The reference builds
// the grid with `base_grid.view(1, oh * ow, 3).bmm(theta)` on the CPU; here each lane computes its pixels' grid values in
// registers with that bmm's rounding sequence and hands them to the sampling core elastic uses (mv_gridsample.h), so the results
// are the reference's bits:
//   affine       x = j - (ow - 1) / 2, y = i - (oh - 1) / 2   (the `_affine_grid` linspace vectors: step exactly 1)
//                g = fma(y, b, x * a) + c  per axis (order 1); (a, b, c) = one column of theta^T / (0.5 * iw, 0.5 * ih)
//   perspective  x = j + 0.5, y = i + 0.5                      (`_perspective_grid`)
//                g = (fma(y, b, x * a) + c) / (fma(y, c7, x * c6) + 1) - 1   (correctly rounded division, -fno-fast-math)
//   order 0      the plain sum (x * a + y * b) + c instead: ATen's naive small-bmm loop (oh * ow * 3 * 2 < 400), and the
//                blocked bmm of hosts whose BLAS kernel does not fuse (the host probes its own bmm: functional.py)
//   then         xs = fma(g + 1, iw / 2, -0.5) (ys likewise) -> gs::setup / gs::sample / the fill blend
//
// Layout (template BLOCK, picked on the host from the dtype and the matrix: pick_block): ROW = elastic's, one 256-pixel row
// segment per wave and a 256 x 4 workgroup tile (float: pixel k of lane l at column 64k + l; uint8: 4 adjacent pixels per
// lane, one dword store);
// BLOCK = a 2-D footprint per wave so that one gather instruction's 64 samples land in a few source rows at any angle: float
// 16 x 16 pixels per wave (8 x 8 lanes, pixel k at (+8 (k >> 1), +8 (k & 1))), uint8 32 x 8 (8 x 8 lanes of 4 adjacent
// pixels); both make a 32 x 32 workgroup tile.  Each lane computes its pixels' offsets, weights and in-bounds bits once and walks
// all N*C planes; tiles go to the XCDs in contiguous runs (xcd_remap); small outputs split the planes over several workgroups.
#include "mv_gridsample.h"

namespace mv {

namespace {

struct Coeffs {
  float ax, bx, cx, ay, by, cy, c6, c7;  // column x of the (rescaled) theta, column y, the perspective denominator's x and y
};

template <bool BLOCK>
struct Tile;
template <>
struct Tile<false> {
  static constexpr int kW = 256, kH = 4;
};
template <>
struct Tile<true> {
  static constexpr int kW = 32, kH = 32;
};

// (row, column) of pixel k of the calling lane in the workgroup tile
template <typename T, bool BLOCK>
__device__ inline void pixel_of(int k, int& r, int& c) {
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  if (!BLOCK) {
    r = wave;
    c = sizeof(T) == 4 ? lane + 64 * k : 4 * lane + k;
  } else if (sizeof(T) == 4) {
    r = (wave >> 1) * 16 + (lane >> 3) + 8 * (k >> 1);
    c = (wave & 1) * 16 + (lane & 7) + 8 * (k & 1);
  } else {
    r = wave * 8 + (lane >> 3);
    c = 4 * (lane & 7) + k;
  }
}

// T: float or uint8_t.  NEAREST: mode.  FILL: blend with fill.v[plane % channels].  VEC (uint8): the lane's 4 adjacent pixels
// are one aligned dword store.  PAIR (bilinear, iw >= 2): corner pairs.  BLOCK: the layout above.  kind: 0 affine, 1
// perspective; order: 1 the fma chain, 0 the plain sum (both wave-uniform, outside the plane loop).
template <typename T, bool NEAREST, bool FILL, bool VEC, bool PAIR, bool BLOCK>
__global__ __launch_bounds__(256) void k_warp(const T* __restrict__ x, T* __restrict__ y, long long planes, int chunk_planes,
                                              int tiles_x, int tiles, int ih, int iw, int oh, int ow, Coeffs m, int kind,
                                              int order, int channels, gs::Fill fill) {
  const unsigned id = xcd_remap(blockIdx.x, gridDim.x);
  const int chunk = (int)(id / (unsigned)tiles), tile = (int)(id % (unsigned)tiles);
  const int i_t = (tile / tiles_x) * Tile<BLOCK>::kH, j_t = (tile % tiles_x) * Tile<BLOCK>::kW;
  int r0, c0;
  pixel_of<T, BLOCK>(0, r0, c0);
  if (i_t + r0 >= oh || j_t + c0 >= ow) return;  // pixel 0 has the lane's smallest row and column
  const long long p0 = (long long)chunk * chunk_planes;
  const long long p1 = p0 + chunk_planes < planes ? p0 + chunk_planes : planes;

  const float hw_x = (float)iw * 0.5f, hw_y = (float)ih * 0.5f;
  const float ox = kind == 0 ? 0.5f * (float)(ow - 1) : -0.5f, oy = kind == 0 ? 0.5f * (float)(oh - 1) : -0.5f;
  int off[4][4];
  float wt[4][4];
  unsigned inb[4];
  int dof[4];        // the pixel's offset in an output plane
  unsigned live = 0;  // bit k: pixel k is inside the output
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int r, c;
    pixel_of<T, BLOCK>(k, r, c);
    r += i_t, c += j_t;
    live |= (r < oh && c < ow) ? 1u << k : 0u;
    r = r < oh ? r : oh - 1, c = c < ow ? c : ow - 1;
    dof[k] = r * ow + c;
    const float bx = (float)c - ox, by = (float)r - oy;  // exact: the reference's linspace values (step 1)
    float gx, gy;
    if (order) {
      gx = __builtin_fmaf(by, m.bx, bx * m.ax) + m.cx;
      gy = __builtin_fmaf(by, m.by, bx * m.ay) + m.cy;
    } else {
      gx = (bx * m.ax + by * m.bx) + m.cx;
      gy = (bx * m.ay + by * m.by) + m.cy;
    }
    if (kind == 1) {
      const float d = order ? __builtin_fmaf(by, m.c7, bx * m.c6) + 1.f : (bx * m.c6 + by * m.c7) + 1.f;
      gx = gx / d - 1.f;
      gy = gy / d - 1.f;
    }
    const float xs = __builtin_fmaf(gx + 1.f, hw_x, -0.5f);
    const float ys = __builtin_fmaf(gy + 1.f, hw_y, -0.5f);
    gs::setup<NEAREST, PAIR>(xs, ys, ih, iw, off[k], wt[k], inb[k]);
  }
  float msk[4] = {};
  if (FILL && !NEAREST) {
#pragma unroll
    for (int k = 0; k < 4; ++k) msk[k] = gs::fill_mask(wt[k], inb[k]);
  }

  const size_t in_elems = (size_t)ih * iw, out_elems = (size_t)oh * ow;
  int c = FILL ? (int)(p0 % channels) : 0;
#pragma unroll 2
  for (long long p = p0; p < p1; ++p) {
    const T* src = x + (size_t)p * in_elems;
    float out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      out[k] = gs::sample<T, NEAREST, FILL, PAIR>(src, off[k], wt[k], inb[k], msk[k], FILL ? fill.v[c] : 0.f);
    T* dst = y + (size_t)p * out_elems;
    if (VEC && sizeof(T) == 1) {
      const unsigned o = (unsigned)gs::narrow<T>(out[0]) | ((unsigned)gs::narrow<T>(out[1]) << 8) |
                         ((unsigned)gs::narrow<T>(out[2]) << 16) | ((unsigned)gs::narrow<T>(out[3]) << 24);
      *reinterpret_cast<unsigned*>(dst + dof[0]) = o;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (live & (1u << k)) dst[dof[k]] = gs::narrow<T>(out[k]);
    }
    if (FILL) c = c + 1 == channels ? 0 : c + 1;
  }
}

struct Args {
  long long planes;
  int chunk_planes, tiles_x, tiles, ih, iw, oh, ow;
  Coeffs m;
  int kind, order, channels;
  gs::Fill fill;
};

template <typename T, bool NEAREST, bool FILL, bool VEC, bool PAIR, bool BLOCK>
void go(dim3 grid, hipStream_t s, const T* x, T* y, const Args& a) {
  hipLaunchKernelGGL((k_warp<T, NEAREST, FILL, VEC, PAIR, BLOCK>), grid, dim3(256), 0, s, x, y, a.planes, a.chunk_planes,
                     a.tiles_x, a.tiles, a.ih, a.iw, a.oh, a.ow, a.m, a.kind, a.order, a.channels, a.fill);
}

template <typename T, bool NEAREST, bool FILL, bool VEC, bool BLOCK>
void launch_pair(bool pair, dim3 grid, hipStream_t s, const T* x, T* y, const Args& a) {
  if (pair && !NEAREST) go<T, NEAREST, FILL, VEC, true, BLOCK>(grid, s, x, y, a);
  else go<T, NEAREST, FILL, VEC, false, BLOCK>(grid, s, x, y, a);
}

template <typename T, bool NEAREST, bool FILL, bool BLOCK>
void launch_vec(bool vec, bool pair, dim3 grid, hipStream_t s, const T* x, T* y, const Args& a) {
  if (sizeof(T) == 1 && vec) launch_pair<T, NEAREST, FILL, true, BLOCK>(pair, grid, s, x, y, a);
  else launch_pair<T, NEAREST, FILL, false, BLOCK>(pair, grid, s, x, y, a);
}

template <typename T, bool BLOCK>
void launch_mode(bool nearest, bool with_fill, bool vec, bool pair, dim3 grid, hipStream_t s, const T* x, T* y, const Args& a) {
  if (nearest && with_fill) launch_vec<T, true, true, BLOCK>(vec, pair, grid, s, x, y, a);
  else if (nearest) launch_vec<T, true, false, BLOCK>(vec, pair, grid, s, x, y, a);
  else if (with_fill) launch_vec<T, false, true, BLOCK>(vec, pair, grid, s, x, y, a);
  else launch_vec<T, false, false, BLOCK>(vec, pair, grid, s, x, y, a);
}

// ROW only for float32 grids that run along the output rows: a row segment's 256 pixels then read few source rows.  |ay| /
// |by| is the number of source rows an output row crosses per output row the column crosses; up to 1/4, ROW's coalesced
// 256-pixel segments win (0 degrees, small rotations and shears, mild perspectives), above it BLOCK does (30 degrees: 0.77
// against 1.19 ms).  uint8 takes BLOCK always: never slower, 2.3x faster at 30 degrees (DESIGN.md section 3.14 has the table).
bool pick_block(const Coeffs& m, bool u8) {
  if (const char* v = tune_env("MV_WARP_LAYOUT")) return v[0] == 'b';  // tools/perf_warp.py --layouts: "block" / "row"
  return u8 || __builtin_fabsf(m.ay) * 4.f > __builtin_fabsf(m.by);
}

template <typename T>
int launch(const T* x, T* y, int64_t planes, int channels, int ih, int iw, int oh, int ow, const float* coeffs, int kind, int order,
           int mode, const float* fill_host, hipStream_t s) {
  if (fill_host && channels > gs::kMaxFill)
    return set_error(MV_ERR_UNSUPPORTED, "warp: a per-channel fill covers up to %d channels, got %d", gs::kMaxFill, channels);
  Args a{};
  if (fill_host)
    for (int k = 0; k < channels; ++k) a.fill.v[k] = fill_host[k];
  a.m = Coeffs{coeffs[0], coeffs[1], coeffs[2], coeffs[3], coeffs[4], coeffs[5], coeffs[6], coeffs[7]};
  const bool block = pick_block(a.m, sizeof(T) == 1);
  const int tw = block ? Tile<true>::kW : Tile<false>::kW, th = block ? Tile<true>::kH : Tile<false>::kH;
  const int tiles_x = (ow + tw - 1) / tw, tiles_y = (oh + th - 1) / th;
  const long long tiles = (long long)tiles_x * tiles_y;
  long long chunks, chunk_planes;
  if (!gs::plan_chunks(tiles, planes, chunks, chunk_planes))
    return set_error(MV_ERR_UNSUPPORTED, "warp: grid of %lld tiles x %lld plane chunks is too large", tiles, chunks);
  const dim3 grid((unsigned)(tiles * chunks));
  a.planes = planes, a.chunk_planes = (int)chunk_planes, a.tiles_x = tiles_x, a.tiles = (int)tiles;
  a.ih = ih, a.iw = iw, a.oh = oh, a.ow = ow, a.kind = kind, a.order = order, a.channels = channels;
  const bool vec = sizeof(T) == 1 && ow % 4 == 0 && ((uintptr_t)y % 4) == 0;  // float stores are per pixel (coalesced)
  const bool pair = iw >= 2;
  const bool nearest = mode == 1, with_fill = fill_host != nullptr;
  if (block) launch_mode<T, true>(nearest, with_fill, vec, pair, grid, s, x, y, a);
  else launch_mode<T, false>(nearest, with_fill, vec, pair, grid, s, x, y, a);
  return check_launchf("k_warp<%s,%s,%s,%s,%s%s,%s>", sizeof(T) == 4 ? "f32" : "u8", kind ? "perspective" : "affine",
                       nearest ? "nearest" : "bilinear", with_fill ? "fill" : "nofill", vec ? "vec" : "px",
                       pair && !nearest ? ",pair" : "", block ? "block" : "row");
}

}  // namespace

int launch_warp(const void* x, void* y, bool u8, int64_t planes, int channels, int ih, int iw, int oh, int ow, const float* coeffs,
                int kind, int order, int mode, const float* fill, hipStream_t s) {
  if (u8)
    return launch((const uint8_t*)x, (uint8_t*)y, planes, channels, ih, iw, oh, ow, coeffs, kind, order, mode, fill, s);
  return launch((const float*)x, (float*)y, planes, channels, ih, iw, oh, ow, coeffs, kind, order, mode, fill, s);
}

}  // namespace mv
