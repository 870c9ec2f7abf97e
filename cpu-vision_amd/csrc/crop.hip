// crop.hip -- F.pad / F.crop / F.horizontal_flip / F.vertical_flip / F.erase (v2/functional/_geometry.py, _augment.py) on gfx950:
// ONE gather kernel, pure data movement, templated on the element width (1, 2, 4, 8 bytes) and not on the dtype.
//
// Per output pixel (y, x) each axis maps independently to a source index or to "fill" (gather_index below; the same map is
// written on the host in _crop.py `axis_index_map`, where it is tested against torch.nn.functional.pad and _pad_symmetric):
//   p = (flip ? out - 1 - o : o) + off          off < 0 extends (padding), off > 0 crops
//   0 <= p < in        -> p
//   constant           -> fill (per channel, by value)
//   edge               -> clamp(p)
//   reflect            -> -p | 2 (in - 1) - p              (ATen reflection_pad2d; one reflection: padding < in is checked)
//   symmetric          -> -1 - p | 2 in - 1 - p            (_functional_tensor.py _pad_symmetric; padding <= in is checked)
// and one optional box [bi, bi + bh) x [bj, bj + bw) of the OUTPUT takes its pixels from `v` (erase) instead of the source, whose
// pixels under the box are never read.
//
// A lane owns 16 bytes of an output row.  gfx950 global memory takes 16-byte accesses at any byte address, so
// rows need no alignment: a group whose 16 bytes map to one ascending (or, flipped, descending) run inside the source row moves
// with one load and one store -- a flipped group is reversed in registers -- and the ragged last group of a row is anchored
// at out - V (it overlaps its left neighbour and writes the same bytes).  Only groups that touch a border column, the box or a
// row narrower than 16 bytes go element by element.  No workspace, one launch, nothing read back.
#include "mv_common.h"

namespace mv {
namespace {

typedef unsigned int u32x4u __attribute__((ext_vector_type(4), aligned(1)));

struct GatherAxis {
  int in, out, off, mode, flip;
};

__host__ __device__ inline int gather_index(const GatherAxis& a, int o) {
  int p = (a.flip ? a.out - 1 - o : o) + a.off;
  if (p >= 0 && p < a.in) return p;
  if (a.mode == MV_PAD_CONSTANT) return -1;
  if (a.mode == MV_PAD_REFLECT)
    p = p < 0 ? -p : 2 * (a.in - 1) - p;
  else if (a.mode == MV_PAD_SYMMETRIC)
    p = p < 0 ? -1 - p : 2 * a.in - 1 - p;
  p = p < 0 ? 0 : p;  // edge; and a total map for the other two (the entry point has checked that one reflection suffices)
  return p >= a.in ? a.in - 1 : p;
}

struct GatherArgs {
  const void* x;
  void* y;
  const void* v;        // erase values in the image's element type: [channels] or [channels][bh][bw]
  GatherAxis ay, ax;
  long long rows;       // planes * ay.out
  int channels;         // plane p belongs to channel p % channels (fill and v)
  unsigned long long fill[4];
  int bi, bj, bh, bw;   // the erase box in output coordinates; bh == 0: none
  int v_per_pixel;
  int tpr_log2;         // lanes per row segment (a power of two <= 256): narrow rows share a workgroup
  int groups;           // 16-byte groups per row
};

__device__ inline void split(long long n, int d, bool small, long long& q, int& r) {
  if (small) {  // 32-bit division when the dividend fits
    const unsigned qq = (unsigned)n / (unsigned)d;
    q = qq, r = (int)((unsigned)n - qq * (unsigned)d);
  } else {
    q = n / d, r = (int)(n - q * d);
  }
}

template <typename U>
__global__ __launch_bounds__(256) void k_gather(const GatherArgs A) {
  constexpr int V = 16 / (int)sizeof(U);
  const int tpr = 1 << A.tpr_log2;
  const unsigned tiles = (unsigned)(A.groups + tpr - 1) >> A.tpr_log2;
  const unsigned rb = blockIdx.x / tiles, tile = blockIdx.x - rb * tiles;
  const long long row = (long long)rb * (256 >> A.tpr_log2) + (threadIdx.x >> A.tpr_log2);
  const int g = (int)tile * tpr + (int)(threadIdx.x & (tpr - 1));
  if (row >= A.rows || g >= A.groups) return;
  const bool small = A.rows <= 0x7fffffffLL;
  long long plane;
  int oy;
  split(row, A.ay.out, small, plane, oy);
  int c = 0;
  if (A.channels > 1) {
    long long q;
    split(plane, A.channels, small, q, c);
  }
  const int ow = A.ax.out;
  U* const dst = static_cast<U*>(A.y) + (size_t)row * ow;
  const int sy = gather_index(A.ay, oy);
  const U* const src = static_cast<const U*>(A.x) + ((size_t)plane * A.ay.in + (sy < 0 ? 0 : sy)) * A.ax.in;
  const bool box_row = A.bh > 0 && oy >= A.bi && oy < A.bi + A.bh;
  const int x0 = ow >= V ? min(g * V, ow - V) : 0;
  const int n = ow >= V ? V : ow;
  bool vec = ow >= V && sy >= 0 && !(box_row && x0 < A.bj + A.bw && x0 + V > A.bj);
  const int s0 = (A.ax.flip ? ow - V - x0 : x0) + A.ax.off;  // the lowest source column of the group
  vec = vec && s0 >= 0 && s0 + V <= A.ax.in;
  if (vec) {
    union {
      u32x4u q;
      U e[V];
    } a, b;
    a.q = *reinterpret_cast<const u32x4u*>(src + s0);
    if (A.ax.flip) {
#pragma unroll
      for (int j = 0; j < V; ++j) b.e[j] = a.e[V - 1 - j];
    } else {
      b.q = a.q;
    }
    *reinterpret_cast<u32x4u*>(dst + x0) = b.q;
    return;
  }
  const U fillv = (U)A.fill[c & 3];
  for (int j = 0; j < n; ++j) {
    const int x = x0 + j;
    U val;
    if (box_row && x >= A.bj && x < A.bj + A.bw) {
      const U* v = static_cast<const U*>(A.v);
      val = A.v_per_pixel ? v[((size_t)c * A.bh + (oy - A.bi)) * A.bw + (x - A.bj)] : v[c];
    } else {
      const int sx = gather_index(A.ax, x);
      val = (sy < 0 || sx < 0) ? fillv : src[sx];
    }
    dst[x] = val;
  }
}

// erase in place: only the box is written
struct EraseArgs {
  void* y;
  const void* v;
  long long planes;
  int channels, h, w, bi, bj, bh, bw, v_per_pixel;
};

template <typename U>
__global__ __launch_bounds__(256) void k_erase_box(const EraseArgs A) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per_plane = (long long)A.bh * A.bw;
  if (idx >= A.planes * per_plane) return;
  const long long plane = idx / per_plane;
  const int rem = (int)(idx - plane * per_plane);
  const int r = rem / A.bw, col = rem - r * A.bw;
  const int c = (int)(plane % A.channels);
  const U* v = static_cast<const U*>(A.v);
  static_cast<U*>(A.y)[((size_t)plane * A.h + (A.bi + r)) * A.w + (A.bj + col)] =
      A.v_per_pixel ? v[((size_t)c * A.bh + r) * A.bw + col] : v[c];
}

template <typename K8, typename K16, typename K32, typename K64>
void by_width(int elem_bytes, K8 k8, K16 k16, K32 k32, K64 k64) {
  switch (elem_bytes) {
    case 1: k8(); break;
    case 2: k16(); break;
    case 4: k32(); break;
    default: k64(); break;
  }
}

}  // namespace

bool gather_axis_ok(int in, int out, int off, int mode) {
  if (in <= 0 || out <= 0) return false;
  const int before = -off, after = out - in + off;  // < 0: crops
  if (mode == MV_PAD_REFLECT) return before < in && after < in;
  if (mode == MV_PAD_SYMMETRIC) return before <= in && after <= in;  // what one mirror image of the side can reach
  return true;
}

bool gather_grid_fits(int64_t planes, int oh, int ow, int elem_bytes) {
  const int v = 16 / elem_bytes;
  const long long groups = ow >= v ? (ow + v - 1) / v : 1;
  int tpr = 4;
  while (tpr < 256 && tpr < groups) tpr *= 2;
  const long long row_blocks = (planes * oh + 256 / tpr - 1) / (256 / tpr);
  return row_blocks * ((groups + tpr - 1) / tpr) <= 0x7fffffffLL;
}

int launch_gather(const void* x, void* y, int64_t planes, int channels, int elem_bytes, int ih, int iw, int oh, int ow, int top,
                  int left, int mode, int flip_h, int flip_v, const unsigned long long* fill, const void* v, int bi, int bj,
                  int bh, int bw, int v_per_pixel, hipStream_t s) {
  GatherArgs a = {};
  a.x = x, a.y = y, a.v = v;
  a.ay = GatherAxis{ih, oh, top, mode, flip_v};
  a.ax = GatherAxis{iw, ow, left, mode, flip_h};
  a.rows = planes * (long long)oh;
  a.channels = channels > 0 ? channels : 1;
  for (int i = 0; i < 4; ++i) a.fill[i] = fill ? fill[i] : 0ull;
  a.bi = bi, a.bj = bj, a.bh = bh, a.bw = bw, a.v_per_pixel = v_per_pixel;
  const int vlen = 16 / elem_bytes;
  a.groups = ow >= vlen ? (ow + vlen - 1) / vlen : 1;
  a.tpr_log2 = 2;
  while (a.tpr_log2 < 8 && (1 << a.tpr_log2) < a.groups) ++a.tpr_log2;
  const int tpr = 1 << a.tpr_log2, rpb = 256 / tpr;
  const long long blocks = ((a.rows + rpb - 1) / rpb) * ((a.groups + tpr - 1) / tpr);
  if (blocks == 0) return MV_OK;
  auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, s, a); };
  by_width(elem_bytes, [&] { go(k_gather<uint8_t>); }, [&] { go(k_gather<uint16_t>); }, [&] { go(k_gather<uint32_t>); },
           [&] { go(k_gather<uint64_t>); });
  return check_launchf("k_gather<b%d,%s%s%s>", elem_bytes, flip_h ? "hflip," : "", flip_v ? "vflip," : "", bh > 0 ? "box" : "map");
}

int launch_erase_box(void* y, int64_t planes, int channels, int elem_bytes, int h, int w, int bi, int bj, int bh, int bw,
                     const void* v, int v_per_pixel, hipStream_t s) {
  EraseArgs a = {y, v, planes, channels, h, w, bi, bj, bh, bw, v_per_pixel};
  const long long n = planes * (long long)bh * bw;
  if (n == 0) return MV_OK;
  const unsigned nb = (unsigned)((n + 255) / 256);
  auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, s, a); };
  by_width(elem_bytes, [&] { go(k_erase_box<uint8_t>); }, [&] { go(k_erase_box<uint16_t>); }, [&] { go(k_erase_box<uint32_t>); },
           [&] { go(k_erase_box<uint64_t>); });
  return check_launchf("k_erase_box<b%d>", elem_bytes);
}

}  // namespace mv
