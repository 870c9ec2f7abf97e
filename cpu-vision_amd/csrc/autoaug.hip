// autoaug.hip -- the colour ops of the automatic augmentation policies that F.adjust_* does not cover
// (transforms/v2/functional/_color.py `invert_image`, `posterize_image`, `solarize_image`, `autocontrast_image`,
// `equalize_image`) on float32 / uint8 images.  Arithmetic per op: include/mi355vision.h.
//
// k_pointwise: invert, posterize and solarize over the flat element range; a lane owns one group of V elements (16 bytes,
// mv_vec16.h), the last partial group goes pixel by pixel.  The op is a template parameter.
//
// autocontrast (two launches) and equalize (three) work on (planes, h, w) single-channel planes and never leave the stream:
//   autocontrast  k_minmax: workgroup b covers chunk b % chunks of plane b / chunks (kItems groups of V pixels per lane) and
//                 writes its (min, max, NaN seen) as one float4 partial; k_autocontrast: every workgroup reduces its plane's
//                 partials (min / max are exact in any order) and maps kMapItems groups per lane.
//   equalize      k_zero_hist zeroes the planes x 256 uint32 histogram; k_hist builds each workgroup's histogram
//                 in LDS -- a lane adds a run of equal bins with one LDS atomic, so a flat image costs one atomic per lane
//                 rather than one per pixel -- and adds its non-zero bins into the plane's histogram with global integer
//                 atomics (order-free); k_equalize: one wave of every workgroup rebuilds the plane's LUT from the 256 bins
//                 with a wave-level scan, the others wait at the barrier, then all map their pixels through the LUT in LDS.
// 64-bit element offsets throughout.  Results are written with vector stores only.
#include "mv_common.h"
#include "mv_vec16.h"

namespace mv {

namespace {

constexpr int kThreads = 256;
constexpr int kItems = 8;     // groups of V pixels per lane in k_minmax / k_hist
constexpr int kMapItems = 4;  // in k_autocontrast / k_equalize
constexpr float kToU8 = 255.999f;          // to_dtype_image float -> uint8: x.mul(255 + 1.0 - 1e-3)
constexpr float kFromU8 = (float)(1.0 / 255.0);  // to_dtype_image uint8 -> float: .mul_(1.0 / 255)

__device__ inline float clamp_to(float v, float hi) {
  // ATen's clamp_(0, hi): NaN stays NaN
  v = v <= 0.f ? 0.f : v;
  return v >= hi ? hi : v;
}

template <bool U8>
__device__ inline float invert(float v) {
  return U8 ? 255.f - v : 1.f - v;
}

// op on one value; p: float posterize 2^bits, solarize the float32 threshold; mask: uint8 posterize's bit mask
template <bool U8, int OP>
__device__ inline float point(float v, float p, unsigned mask) {
  if (OP == MV_POINT_INVERT) return invert<U8>(v);
  if (OP == MV_POINT_POSTERIZE) {
    if (U8) return (float)((unsigned)v & mask);
    return clamp_to(__builtin_floorf(v * p), p - 1.f) * (1.f / p);  // p is a power of two: both products are exact
  }
  return v >= p ? invert<U8>(v) : v;  // MV_POINT_SOLARIZE
}

template <typename T, int OP, bool VEC>
__global__ __launch_bounds__(kThreads) void k_pointwise(const T* __restrict__ x, T* __restrict__ y, long long n, float p,
                                                       unsigned mask) {
  constexpr int V = Vec<T>::V;
  const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * V;
  if (p0 >= n) return;
  float v[1][V];
  if (VEC && p0 + V <= n) {
    load<T, 1, true>(x, n, p0, v);
#pragma unroll
    for (int j = 0; j < V; ++j) v[0][j] = point<sizeof(T) == 1, OP>(v[0][j], p, mask);
    store<T, 1, true>(y, n, p0, v);
  } else {
    load<T, 1, false>(x, n, p0, v);
#pragma unroll
    for (int j = 0; j < V; ++j) v[0][j] = point<sizeof(T) == 1, OP>(v[0][j], p, mask);
    store<T, 1, false>(y, n, p0, v);
  }
}

// ---- autocontrast ----------------------------------------------------------------------------------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void k_minmax(const T* __restrict__ x, long long hw, long long groups, int chunks,
                                                    float4* __restrict__ part) {
  constexpr int V = Vec<T>::V;
  const long long plane = blockIdx.x / (unsigned)chunks;
  const int chunk = (int)(blockIdx.x % (unsigned)chunks);
  const T* base = x + (size_t)plane * hw;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  int nan = 0;
#pragma unroll 1
  for (int it = 0; it < kItems; ++it) {
    const long long g = ((long long)chunk * kItems + it) * kThreads + threadIdx.x;
    if (g >= groups) break;
    const long long p0 = g * V;
    float v[1][V];
    load<T, 1, VEC>(base, hw, p0, v);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (!VEC && p0 + j >= hw) continue;
      const float a = v[0][j];
      mn = a < mn ? a : mn;  // NaN compares false: it only sets the flag
      mx = a > mx ? a : mx;
      nan |= a != a;
    }
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const float omn = __shfl_xor(mn, o), omx = __shfl_xor(mx, o);
    mn = omn < mn ? omn : mn;
    mx = omx > mx ? omx : mx;
    nan |= __shfl_xor(nan, o);
  }
  __shared__ float4 waves[kThreads / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) waves[wave] = make_float4(mn, mx, (float)nan, 0.f);
  __syncthreads();
  if (threadIdx.x == 0) {
    float4 r = waves[0];
    for (int w = 1; w < kThreads / kWave; ++w) {
      r.x = waves[w].x < r.x ? waves[w].x : r.x;
      r.y = waves[w].y > r.y ? waves[w].y : r.y;
      r.z = waves[w].z != 0.f ? 1.f : r.z;
    }
    part[(size_t)plane * chunks + chunk] = r;
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void k_autocontrast(const T* __restrict__ x, T* __restrict__ y, long long hw,
                                                          long long groups, int chunks, int pchunks,
                                                          const float4* __restrict__ part) {
  constexpr int V = Vec<T>::V;
  constexpr bool U8 = sizeof(T) == 1;
  const float bound = U8 ? 255.f : 1.f;
  const long long plane = blockIdx.x / (unsigned)chunks;
  const int chunk = (int)(blockIdx.x % (unsigned)chunks);
  __shared__ float s_lo, s_inv;
  if (threadIdx.x < kWave) {
    float mn = __builtin_inff(), mx = -__builtin_inff();
    int nan = 0;
    for (int k = threadIdx.x; k < pchunks; k += kWave) {
      const float4 r = part[(size_t)plane * pchunks + k];
      mn = r.x < mn ? r.x : mn;
      mx = r.y > mx ? r.y : mx;
      nan |= r.z != 0.f;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      const float omn = __shfl_xor(mn, o), omx = __shfl_xor(mx, o);
      mn = omn < mn ? omn : mn;
      mx = omx > mx ? omx : mx;
      nan |= __shfl_xor(nan, o);
    }
    if (threadIdx.x == 0) {
      float lo = mn, inv = (mx - mn) * (U8 ? (float)(1.0 / 255.0) : 1.f);
      if (nan) lo = inv = __builtin_nanf("");  // amin / amax of the plane are NaN: so is every output
      else if (mx == mn) lo = 0.f, inv = 1.f;
      s_lo = lo, s_inv = inv;
    }
  }
  __syncthreads();
  const float lo = s_lo, inv = s_inv;
  T* out = y + (size_t)plane * hw;
  const T* in = x + (size_t)plane * hw;
#pragma unroll 1
  for (int it = 0; it < kMapItems; ++it) {
    const long long g = ((long long)chunk * kMapItems + it) * kThreads + threadIdx.x;
    if (g >= groups) break;
    const long long p0 = g * V;
    float v[1][V];
    load<T, 1, VEC>(in, hw, p0, v);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float r = clamp_to((v[0][j] - lo) / inv, bound);  // a true division (-fno-fast-math)
      v[0][j] = U8 ? __builtin_truncf(r) : r;                // .to(uint8) of a value in [0, 255]
    }
    store<T, 1, VEC>(out, hw, p0, v);
  }
}

// ---- equalize --------------------------------------------------------------------------------------------------------
// the uint8 value equalize bins a pixel into: to_dtype_image(scale=True) for float in [0, 1]; outside it, saturated
template <bool U8>
__device__ inline int bin_of(float v) {
  if (U8) return (int)v;
  const float s = v * kToU8;
  if (!(s > 0.f)) return 0;  // negative, zero, NaN
  return s >= 255.f ? 255 : (int)s;
}

// the planes x 256 histogram counters to zero, one 16-byte store per lane (a kernel rather than hipMemsetAsync: in a captured
// graph, the memset node did not zero the histograms again on the second replay -- DESIGN.md section 3.16)
__global__ __launch_bounds__(kThreads) void k_zero_hist(unsigned* __restrict__ hist, long long quads) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < quads) reinterpret_cast<uint4*>(hist)[i] = make_uint4(0, 0, 0, 0);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void k_hist(const T* __restrict__ x, long long hw, long long groups, int chunks,
                                                  unsigned* __restrict__ hist) {
  constexpr int V = Vec<T>::V;
  constexpr bool U8 = sizeof(T) == 1;
  __shared__ unsigned bins[256];
  bins[threadIdx.x] = 0;  // kThreads == 256
  __syncthreads();
  const long long plane = blockIdx.x / (unsigned)chunks;
  const int chunk = (int)(blockIdx.x % (unsigned)chunks);
  const T* base = x + (size_t)plane * hw;
  int run_bin = 0;
  unsigned run = 0;
#pragma unroll 1
  for (int it = 0; it < kItems; ++it) {
    const long long g = ((long long)chunk * kItems + it) * kThreads + threadIdx.x;
    if (g >= groups) break;
    const long long p0 = g * V;
    float v[1][V];
    load<T, 1, VEC>(base, hw, p0, v);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (!VEC && p0 + j >= hw) continue;
      const int b = bin_of<U8>(v[0][j]);
      if (b != run_bin) {
        if (run) atomicAdd(&bins[run_bin], run);
        run_bin = b, run = 0;
      }
      ++run;
    }
  }
  if (run) atomicAdd(&bins[run_bin], run);
  __syncthreads();
  const unsigned c = bins[threadIdx.x];
  if (c) atomicAdd(hist + (size_t)plane * 256 + threadIdx.x, c);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void k_equalize(const T* __restrict__ x, T* __restrict__ y, long long hw,
                                                      long long groups, int chunks, const unsigned* __restrict__ hist) {
  constexpr int V = Vec<T>::V;
  constexpr bool U8 = sizeof(T) == 1;
  const long long plane = blockIdx.x / (unsigned)chunks;
  const int chunk = (int)(blockIdx.x % (unsigned)chunks);
  __shared__ float lut[256];
  __shared__ int s_valid;
  if (threadIdx.x < kWave) {
    // lane l owns bins 4l .. 4l + 3
    const int lane = threadIdx.x;
    const uint4 c4 = reinterpret_cast<const uint4*>(hist + (size_t)plane * 256)[lane];
    const unsigned long long c[4] = {c4.x, c4.y, c4.z, c4.w};
    unsigned long long incl[4];
    incl[0] = c[0], incl[1] = incl[0] + c[1], incl[2] = incl[1] + c[2], incl[3] = incl[2] + c[3];
    unsigned long long s = incl[3];
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const unsigned long long t = __shfl_up(s, o);
      if (lane >= o) s += t;
    }
    const unsigned long long excl = s - incl[3];  // cum_hist of bin 4l - 1
    int top = -1;  // the plane's largest value: argmax of the cumulative histogram
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c[k]) top = 4 * lane + k;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      const int t = __shfl_xor(top, o);
      top = t > top ? t : top;
    }
    const unsigned long long mine = c[top & 3];
    const unsigned long long top_count = __shfl(mine, top >> 2);
    const unsigned long long step = ((unsigned long long)hw - top_count) / 255;
    if (step != 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int b = 4 * lane + k;
        const unsigned long long prev = k == 0 ? excl : excl + incl[k - 1];
        const unsigned long long l = (prev + step / 2) / step;
        lut[b] = b == 0 ? 0.f : (float)(l < 255 ? l : 255);
      }
    }
    if (lane == 0) s_valid = step != 0;
  }
  __syncthreads();
  const bool valid = s_valid;
  const T* in = x + (size_t)plane * hw;
  T* out = y + (size_t)plane * hw;
#pragma unroll 1
  for (int it = 0; it < kMapItems; ++it) {
    const long long g = ((long long)chunk * kMapItems + it) * kThreads + threadIdx.x;
    if (g >= groups) break;
    const long long p0 = g * V;
    float v[1][V];
    load<T, 1, VEC>(in, hw, p0, v);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int b = bin_of<U8>(v[0][j]);
      const float q = valid ? lut[b] : (float)b;
      v[0][j] = U8 ? q : q * kFromU8;
    }
    store<T, 1, VEC>(out, hw, p0, v);
  }
}

long long groups_of(long long elems, bool u8) { return (elems + (u8 ? 16 : 4) - 1) / (u8 ? 16 : 4); }
long long reduce_chunks(long long hw, bool u8) {
  return (groups_of(hw, u8) + (long long)kThreads * kItems - 1) / ((long long)kThreads * kItems);
}
long long map_chunks(long long hw, bool u8) {
  return (groups_of(hw, u8) + (long long)kThreads * kMapItems - 1) / ((long long)kThreads * kMapItems);
}

template <typename T, int OP>
int pointwise(const T* x, T* y, long long n, double param, hipStream_t s) {
  constexpr int V = Vec<T>::V;
  const long long blocks = (groups_of(n, V == 16) + kThreads - 1) / kThreads;
  if (blocks > 0xffffffffLL) return set_error(MV_ERR_UNSUPPORTED, "pointwise: %lld elements exceed the launch grid", n);
  float p = 0.f;
  unsigned mask = 0;
  if (OP == MV_POINT_POSTERIZE) {
    const int bits = (int)param;
    p = (float)(1 << bits);
    mask = ((1u << bits) - 1u) << (8 - bits);
  } else if (OP == MV_POINT_SOLARIZE) {
    p = (float)param;
  }
  const bool vec = (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0;
  if (vec) hipLaunchKernelGGL((k_pointwise<T, OP, true>), dim3((unsigned)blocks), dim3(kThreads), 0, s, x, y, n, p, mask);
  else hipLaunchKernelGGL((k_pointwise<T, OP, false>), dim3((unsigned)blocks), dim3(kThreads), 0, s, x, y, n, p, mask);
  return check_launchf("k_pointwise<%s,op%d,%s>", V == 16 ? "u8" : "f32", OP, vec ? "vec16" : "px");
}

template <typename T>
int pointwise_op(const T* x, T* y, long long n, int op, double param, hipStream_t s) {
  if (op == MV_POINT_INVERT) return pointwise<T, MV_POINT_INVERT>(x, y, n, param, s);
  if (op == MV_POINT_POSTERIZE) return pointwise<T, MV_POINT_POSTERIZE>(x, y, n, param, s);
  return pointwise<T, MV_POINT_SOLARIZE>(x, y, n, param, s);
}

template <typename T, bool VEC>
int autocontrast(const T* x, T* y, long long planes, long long hw, void* ws, hipStream_t s) {
  constexpr bool U8 = sizeof(T) == 1;
  const long long groups = groups_of(hw, U8), pchunks = reduce_chunks(hw, U8), chunks = map_chunks(hw, U8);
  auto* part = static_cast<float4*>(ws);
  hipLaunchKernelGGL((k_minmax<T, VEC>), dim3((unsigned)(planes * pchunks)), dim3(kThreads), 0, s, x, hw, groups,
                     (int)pchunks, part);
  if (int rc = check_launch("k_minmax")) return rc;
  hipLaunchKernelGGL((k_autocontrast<T, VEC>), dim3((unsigned)(planes * chunks)), dim3(kThreads), 0, s, x, y, hw, groups,
                     (int)chunks, (int)pchunks, part);
  return check_launchf("k_autocontrast<%s,%s>", U8 ? "u8" : "f32", VEC ? "vec16" : "px");
}

template <typename T, bool VEC>
int equalize(const T* x, T* y, long long planes, long long hw, void* ws, hipStream_t s) {
  constexpr bool U8 = sizeof(T) == 1;
  const long long groups = groups_of(hw, U8), hchunks = reduce_chunks(hw, U8), chunks = map_chunks(hw, U8);
  auto* hist = static_cast<unsigned*>(ws);
  hipLaunchKernelGGL(k_zero_hist, dim3((unsigned)((planes + 3) / 4)), dim3(kThreads), 0, s, hist, planes * 64);
  if (int rc = check_launch("k_zero_hist")) return rc;
  hipLaunchKernelGGL((k_hist<T, VEC>), dim3((unsigned)(planes * hchunks)), dim3(kThreads), 0, s, x, hw, groups, (int)hchunks,
                     hist);
  if (int rc = check_launch("k_hist")) return rc;
  hipLaunchKernelGGL((k_equalize<T, VEC>), dim3((unsigned)(planes * chunks)), dim3(kThreads), 0, s, x, y, hw, groups,
                     (int)chunks, hist);
  return check_launchf("k_equalize<%s,%s>", U8 ? "u8" : "f32", VEC ? "vec16" : "px");
}

}  // namespace

bool autoaug_grid_fits(int64_t planes, int64_t plane_elems, bool u8) {
  return planes * reduce_chunks(plane_elems, u8) <= 0xffffffffLL && planes * map_chunks(plane_elems, u8) <= 0xffffffffLL;
}

int64_t autocontrast_workspace_bytes(int64_t planes, int64_t plane_elems, bool u8) {
  return planes * reduce_chunks(plane_elems, u8) * (int64_t)sizeof(float4);
}

int64_t equalize_workspace_bytes(int64_t planes) { return planes * 256 * (int64_t)sizeof(unsigned); }

int launch_pointwise(const void* x, void* y, bool u8, int64_t n, int op, double param, hipStream_t s) {
  if (u8) return pointwise_op((const uint8_t*)x, (uint8_t*)y, n, op, param, s);
  return pointwise_op((const float*)x, (float*)y, n, op, param, s);
}

int launch_autocontrast(const void* x, void* y, bool u8, int64_t planes, int64_t plane_elems, void* ws, hipStream_t s) {
  const bool vec = vec_ok(x, y, plane_elems, u8 ? 16 : 4);
  if (u8)
    return vec ? autocontrast<uint8_t, true>((const uint8_t*)x, (uint8_t*)y, planes, plane_elems, ws, s)
               : autocontrast<uint8_t, false>((const uint8_t*)x, (uint8_t*)y, planes, plane_elems, ws, s);
  return vec ? autocontrast<float, true>((const float*)x, (float*)y, planes, plane_elems, ws, s)
             : autocontrast<float, false>((const float*)x, (float*)y, planes, plane_elems, ws, s);
}

int launch_equalize(const void* x, void* y, bool u8, int64_t planes, int64_t plane_elems, void* ws, hipStream_t s) {
  const bool vec = vec_ok(x, y, plane_elems, u8 ? 16 : 4);
  if (u8)
    return vec ? equalize<uint8_t, true>((const uint8_t*)x, (uint8_t*)y, planes, plane_elems, ws, s)
               : equalize<uint8_t, false>((const uint8_t*)x, (uint8_t*)y, planes, plane_elems, ws, s);
  return vec ? equalize<float, true>((const float*)x, (float*)y, planes, plane_elems, ws, s)
             : equalize<float, false>((const float*)x, (float*)y, planes, plane_elems, ws, s);
}

}  // namespace mv
