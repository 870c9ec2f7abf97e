// elastic.hip -- F.elastic: the displacement field of ElasticTransform applied to an image (transforms/v2/functional/
// _geometry.py `elastic_image` / `_apply_grid_transform`): grid = identity grid + displacement, then grid_sample(mode,
// padding_mode="zeros", align_corners=False), with the optional fill blended through a resampled ones-mask.  The reference
// runs these ops on torch-CPU; the arithmetic below is ATen's vectorised CPU grid_sampler per pixel, so the results are its
// bits (the per-pixel sampling core lives in mv_gridsample.h, shared with warp.hip):
//   gx = base_x[j] + dx,  x = fma(gx + 1, W / 2, -0.5)        (the same for y; base_* = the reference's own linspace)
//   bilinear  x0 = floor(x), w = x - x0, e = 1 - w (n, s for y);  nw = s*e, ne = s*w, sw = n*e, se = n*w
//             acc = v_nw*nw; acc = fma(v_ne, ne, acc); acc = fma(v_sw, sw, acc); acc = fma(v_se, se, acc)
//             (a corner outside the image has value 0 and is never loaded: clamped address, selected 0)
//             fill: m = the same chain over the in-bounds indicators; out = ((acc - fill) * m) + fill
//   nearest   the corner at (rint(y), rint(x)) (half to even) or 0; fill: an out-of-frame sample is fill
//   uint8     computed in fp32, rounded half to even, narrowed.
//
// One lane owns 4 output pixels of a row: it reads the field and the base coordinates ONCE and works out the corner offsets,
// weights and in-bounds masks of its pixels, then walks the planes (all N*C images share the field) with only the gathers and
// the store per plane.  float: the 4 pixels are 64 apart (pixel k of lane l at column 64k + l), so one gather instruction of
// the wave covers 64 neighbouring columns (a few cache lines) and the stores are 256 contiguous bytes; uint8: 4 adjacent
// pixels per lane (64 lanes still span only 256 bytes) stored as one dword.  Bilinear reads each corner row as ONE 2-element
// load (columns x0, x0 + 1, clamped into the row): 2 gathers per pixel and plane instead of 4.  A workgroup is a 256-pixel x
// 4-row tile (one row segment per wave); tiles are dealt to the XCDs in contiguous runs (xcd_remap) so the neighbouring rows
// every bilinear tap reads meet in one L2.  Small frames split the planes over several workgroups per tile (each re-reads the
// 8 B/pixel field) so the grid still fills the chip.
#include "mv_gridsample.h"

namespace mv {

namespace {

constexpr int kElasticMaxFill = gs::kMaxFill;
constexpr int kTileW = 256;          // pixels per wave row segment (64 lanes x 4)
constexpr int kTileH = 4;            // rows per workgroup (one wave each)

using gs::Fill;
using gs::narrow;

// T: float or uint8_t.  NEAREST: mode.  FILL: blend with fill.v[plane % channels].  VEC (uint8): the lane's 4 pixels are one
// aligned dword store; otherwise pixel-wise stores that stop at the end of the row.  PAIR (bilinear, w >= 2): corner pairs.
template <typename T, bool NEAREST, bool FILL, bool VEC, bool PAIR>
__global__ __launch_bounds__(256) void k_elastic(const T* __restrict__ x, T* __restrict__ y, long long planes, int chunk_planes,
                                                 int tiles_x, int tiles, int h, int w, const float* __restrict__ base_x,
                                                 const float* __restrict__ base_y, const float* __restrict__ disp, long long ds_h,
                                                 long long ds_w, long long ds_c, int channels, Fill fill) {
  const unsigned id = xcd_remap(blockIdx.x, gridDim.x);
  const int chunk = (int)(id / (unsigned)tiles), tile = (int)(id % (unsigned)tiles);
  const int i = (tile / tiles_x) * kTileH + (int)(threadIdx.x >> 6);
  constexpr bool kStrided = sizeof(T) == 4;
  const int lane = (int)(threadIdx.x & 63);
  const int j0 = (tile % tiles_x) * kTileW + (kStrided ? lane : 4 * lane);
  constexpr int kStep = kStrided ? 64 : 1;  // column distance between a lane's pixels
  if (i >= h || j0 >= w) return;
  const long long p0 = (long long)chunk * chunk_planes;
  const long long p1 = p0 + chunk_planes < planes ? p0 + chunk_planes : planes;

  const float hw_x = (float)w * 0.5f, hw_y = (float)h * 0.5f;
  const float gy0 = base_y[i];
  // per pixel: corner offsets, weights and in-bounds bits (gs::setup)
  int off[4][4];
  float wt[4][4];
  unsigned inb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = j0 + k * kStep < w ? j0 + k * kStep : w - 1;
    const float* d = disp + (long long)i * ds_h + (long long)j * ds_w;
    const float gx = base_x[j] + d[0];
    const float gy = gy0 + d[ds_c];
    const float xs = __builtin_fmaf(gx + 1.f, hw_x, -0.5f);
    const float ys = __builtin_fmaf(gy + 1.f, hw_y, -0.5f);
    gs::setup<NEAREST, PAIR>(xs, ys, h, w, off[k], wt[k], inb[k]);
  }
  // the fill mask: the resampled ones-channel of the reference, per pixel (independent of the plane)
  float msk[4] = {};
  if (FILL && !NEAREST) {
#pragma unroll
    for (int k = 0; k < 4; ++k) msk[k] = gs::fill_mask(wt[k], inb[k]);
  }

  const size_t plane_elems = (size_t)h * w;
  const size_t row = (size_t)i * w + j0;
  int c = FILL ? (int)(p0 % channels) : 0;
#pragma unroll 2
  for (long long p = p0; p < p1; ++p) {
    const T* src = x + (size_t)p * plane_elems;
    float out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      out[k] = gs::sample<T, NEAREST, FILL, PAIR>(src, off[k], wt[k], inb[k], msk[k], FILL ? fill.v[c] : 0.f);
    T* dst = y + (size_t)p * plane_elems + row;
    if (VEC && !kStrided) {
      const unsigned o = (unsigned)narrow<T>(out[0]) | ((unsigned)narrow<T>(out[1]) << 8) |
                         ((unsigned)narrow<T>(out[2]) << 16) | ((unsigned)narrow<T>(out[3]) << 24);
      *reinterpret_cast<unsigned*>(dst) = o;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j0 + k * kStep < w) dst[k * kStep] = narrow<T>(out[k]);
    }
    if (FILL) c = c + 1 == channels ? 0 : c + 1;
  }
}

template <typename T, bool NEAREST, bool FILL, bool VEC>
void launch_pair(bool pair, dim3 grid, hipStream_t s, const T* x, T* y, long long planes, int chunk_planes, int tiles_x, int tiles,
                 int h, int w, const float* bx, const float* by, const float* disp, long long sh, long long sw, long long sc,
                 int channels, const Fill& fill) {
  if (pair && !NEAREST)
    hipLaunchKernelGGL((k_elastic<T, NEAREST, FILL, VEC, true>), grid, dim3(256), 0, s, x, y, planes, chunk_planes, tiles_x,
                       tiles, h, w, bx, by, disp, sh, sw, sc, channels, fill);
  else
    hipLaunchKernelGGL((k_elastic<T, NEAREST, FILL, VEC, false>), grid, dim3(256), 0, s, x, y, planes, chunk_planes, tiles_x,
                       tiles, h, w, bx, by, disp, sh, sw, sc, channels, fill);
}

template <typename T, bool NEAREST, bool FILL>
void launch_mode(bool vec, bool pair, dim3 grid, hipStream_t s, const T* x, T* y, long long planes, int chunk_planes, int tiles_x,
                 int tiles, int h, int w, const float* bx, const float* by, const float* disp, long long sh, long long sw,
                 long long sc, int channels, const Fill& fill) {
  if (vec)
    launch_pair<T, NEAREST, FILL, true>(pair, grid, s, x, y, planes, chunk_planes, tiles_x, tiles, h, w, bx, by, disp, sh, sw, sc,
                                        channels, fill);
  else
    launch_pair<T, NEAREST, FILL, false>(pair, grid, s, x, y, planes, chunk_planes, tiles_x, tiles, h, w, bx, by, disp, sh, sw, sc,
                                         channels, fill);
}

template <typename T>
int launch(const T* x, T* y, int64_t planes, int channels, int h, int w, const float* bx, const float* by, const float* disp,
           int64_t sh, int64_t sw, int64_t sc, int mode, const float* fill_host, hipStream_t s) {
  if (fill_host && channels > kElasticMaxFill)
    return set_error(MV_ERR_UNSUPPORTED, "elastic: a per-channel fill covers up to %d channels, got %d", kElasticMaxFill, channels);
  Fill fill{};
  if (fill_host)
    for (int k = 0; k < channels; ++k) fill.v[k] = fill_host[k];
  const int tiles_x = (w + kTileW - 1) / kTileW, tiles_y = (h + kTileH - 1) / kTileH;
  const long long tiles = (long long)tiles_x * tiles_y;
  long long chunks, chunk_planes;
  if (!gs::plan_chunks(tiles, planes, chunks, chunk_planes))
    return set_error(MV_ERR_UNSUPPORTED, "elastic: grid of %lld tiles x %lld plane chunks is too large", tiles, chunks);
  const dim3 grid((unsigned)(tiles * chunks));
  const bool vec = sizeof(T) == 1 && w % 4 == 0 && ((uintptr_t)y % 4) == 0;  // float stores are per pixel (coalesced)
  const bool pair = w >= 2;
  const bool nearest = mode == 1, with_fill = fill_host != nullptr;
  const int cp = (int)chunk_planes, tx = tiles_x, nt = (int)tiles;
  if (nearest && with_fill) launch_mode<T, true, true>(vec, pair, grid, s, x, y, planes, cp, tx, nt, h, w, bx, by, disp, sh, sw, sc, channels, fill);
  else if (nearest) launch_mode<T, true, false>(vec, pair, grid, s, x, y, planes, cp, tx, nt, h, w, bx, by, disp, sh, sw, sc, channels, fill);
  else if (with_fill) launch_mode<T, false, true>(vec, pair, grid, s, x, y, planes, cp, tx, nt, h, w, bx, by, disp, sh, sw, sc, channels, fill);
  else launch_mode<T, false, false>(vec, pair, grid, s, x, y, planes, cp, tx, nt, h, w, bx, by, disp, sh, sw, sc, channels, fill);
  return check_launchf("k_elastic<%s,%s,%s,%s%s>", sizeof(T) == 4 ? "f32" : "u8", nearest ? "nearest" : "bilinear",
                       with_fill ? "fill" : "nofill", vec ? "vec" : "px", pair && !nearest ? ",pair" : "");
}

}  // namespace

int launch_elastic(const void* x, void* y, bool u8, int64_t planes, int channels, int h, int w, const float* base_x,
                   const float* base_y, const float* disp, int64_t disp_sh, int64_t disp_sw, int64_t disp_sc, int mode,
                   const float* fill, hipStream_t s) {
  if (u8)
    return launch((const uint8_t*)x, (uint8_t*)y, planes, channels, h, w, base_x, base_y, disp, disp_sh, disp_sw, disp_sc, mode,
                  fill, s);
  return launch((const float*)x, (float*)y, planes, channels, h, w, base_x, base_y, disp, disp_sh, disp_sw, disp_sc, mode, fill, s);
}

}  // namespace mv
