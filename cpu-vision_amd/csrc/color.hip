// color.hip -- the v2 colour ops (transforms/v2/functional/_color.py `adjust_brightness_image`, `adjust_contrast_image`,
// `adjust_saturation_image`, `adjust_hue_image`, `_rgb_to_grayscale_image`) and ColorJitter's chain of them, on planar
// (..., C, H, W) float32 / uint8 images with C = 1 or 3.
//
// k_color applies a chain of 1-4 ops to every pixel in registers, op by op, with the reference's rounding sequence and its
// quantisation between ops (uint8: clamp, then `.to(uint8)`, which truncates).  Per op, with f = float(factor) and
// a = float(1.0 - factor) (the double difference, rounded once):
//   grey        form 1: fma(b, .114, fma(g, .587, r * .2989))   form 0: (r * .2989 + g * .587) + b * .114   (uint8: floored)
//   blend(x, y) form 1: fma(y, a, x * f)                        form 0: x * f + y * a;   clamp to [0, bound]
//   brightness  clamp(x * f, 0, bound)
//   saturation  blend(x, grey)                      (C = 1: identity)
//   contrast    blend(x, mean)                      mean: the image's mean grey of the chain so far (C = 1: of x itself)
//   hue         _rgb_to_hsv, h = remainder(h + f, 1), _hsv_to_rgb  (uint8: in x * float(1/255), out (u8)(y * 255.999))
// `form` is the rounding of the host's `add_(other, alpha=...)` (fused on vectorised ATen; probed in functional.py).  The
// divisions are true, correctly rounded divisions (-fno-fast-math) and every fma is explicit (-ffp-contract=off).
//
// Layout: a lane owns V pixels of one image (16 bytes of each of its C planes: float 4, uint8 16), loads and stores them with
// one 16-byte access per plane when the plane length and both pointers allow it.  A workgroup of 256 lanes stays inside one
// image, so a chain with contrast reads its image's mean once.
//
// Contrast's mean takes two more launches before k_color: k_color_sum recomputes the ops in front of contrast and sums the
// image's grey values per workgroup -- uint8 as an exact integer, one 64-bit atomic add per workgroup into a slot zeroed on the
// stream by k_color_zero (integer addition is order-free); float32 as a double partial per workgroup, reduced in a fixed order -- and
// k_color_mean turns each image's sum into its float32 mean: uint8 (float)S / (float)N, float32 the double sum of the
// partials, in index order, divided by N and rounded once.  Nothing goes back to the host; the results are the same bits on
// every run.
#include "mv_common.h"
#include "mv_vec16.h"

namespace mv {

namespace {

constexpr int kThreads = 256;
constexpr int kSumItems = 8;  // groups of V pixels per lane in k_color_sum

struct Chain {
  int op[4];
  float f[4];  // float(factor)
  float a[4];  // float(1.0 - factor): blend's second weight
  int n;
  int contrast;  // position of contrast in op[], or n when the chain has none
};

__device__ inline float clampf(float v, float hi) {
  // ATen's vectorised clamp_(0, bound): NaN stays NaN
  v = v <= 0.f ? 0.f : v;
  return v >= hi ? hi : v;
}

template <bool U8>
__device__ inline float quantise(float v) {
  return U8 ? __builtin_truncf(v) : v;  // .to(uint8) of a value already clamped to [0, 255]
}

__device__ inline float grey_of(float r, float g, float b, int form) {
  if (form) return __builtin_fmaf(b, 0.114f, __builtin_fmaf(g, 0.587f, r * 0.2989f));
  return (r * 0.2989f + g * 0.587f) + b * 0.114f;
}

template <bool U8>
__device__ inline float blend(float x, float y, float f, float a, int form) {
  const float bound = U8 ? 255.f : 1.f;
  const float t = x * f;
  const float v = form ? __builtin_fmaf(y, a, t) : t + y * a;
  return quantise<U8>(clampf(v, bound));
}

// ATen's float remainder(a, 1): fmod, then + 1 when the result is negative
__device__ inline float remainder1(float a) {
  float m = __builtin_fmodf(a, 1.f);
  if (m != 0.f && m < 0.f) m = m + 1.f;
  return m;
}

// adjust_hue_image on one pixel (float values: uint8 pixels arrive as their integers)
template <bool U8>
__device__ inline void hue_pixel(float& r0, float& g0, float& b0, float hue) {
  float r = r0, g = g0, b = b0;
  if (U8) r = r * (1.f / 255.f), g = g * (1.f / 255.f), b = b * (1.f / 255.f);
  // _rgb_to_hsv
  const float maxc = __builtin_fmaxf(__builtin_fmaxf(r, g), b), minc = __builtin_fminf(__builtin_fminf(r, g), b);
  const bool eqc = maxc == minc;
  const float range = maxc - minc;
  const float s = range / (eqc ? 1.f : maxc);
  const float div = eqc ? 1.f : range;
  const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
  const bool neq_r = maxc != r, eq_g = maxc == g;
  const float hg = ((rc + 2.f) - bc) * (float)(eq_g && neq_r);
  const float hr = (bc - gc) * (float)(!neq_r);
  const float hb = ((gc + 4.f) - rc) * (float)(neq_r && !eq_g);
  float h = (hr + hg) + hb;
  h = __builtin_fmodf(h * (1.f / 6.f) + 1.f, 1.f);
  h = remainder1(h + hue);
  // a NaN channel, or an infinite one (Inf - Inf, Inf / Inf), leaves the hue NaN.  The reference then takes the sector from
  // int(NaN), which is INT_MIN on one host and 0 on another: the library's rule (include/mi355vision.h) is a pixel of three NaNs
  const bool no_hue = h != h;
  const float v = maxc;
  // _hsv_to_rgb
  const float h6 = h * 6.f;
  const float fi = __builtin_floorf(h6);
  const float fr = h6 - fi;
  int i = (int)fi;
  const float sxf = s * fr, oms = 1.f - s;
  const float q = clampf((1.f - sxf) * v, 1.f);
  const float t = clampf((sxf + oms) * v, 1.f);
  const float p = clampf(oms * v, 1.f);
  i = i % 6;
  if (i < 0) i += 6;
  float ro, go, bo;  // the reference's gather table over (v, p, q, t)
  switch (i) {
    case 0: ro = v, go = t, bo = p; break;
    case 1: ro = q, go = v, bo = p; break;
    case 2: ro = p, go = v, bo = t; break;
    case 3: ro = p, go = q, bo = v; break;
    case 4: ro = t, go = p, bo = v; break;
    default: ro = v, go = p, bo = q; break;
  }
  if (!U8 && no_hue) ro = go = bo = h;
  if (U8) {
    ro = (float)(uint8_t)(int)(ro * 255.999f);
    go = (float)(uint8_t)(int)(go * 255.999f);
    bo = (float)(uint8_t)(int)(bo * 255.999f);
  }
  r0 = ro, g0 = go, b0 = bo;
}

// ops [k0, k1) of the chain on the lane's V pixels (op codes are kernel arguments: the branches are wave-uniform)
template <bool U8, int C, int V>
__device__ inline void run_ops(const Chain& ch, int k0, int k1, int form, float mean, float (&v)[C][V]) {
  const float bound = U8 ? 255.f : 1.f;
  for (int k = k0; k < k1; ++k) {
    const int op = ch.op[k];
    const float f = ch.f[k], a = ch.a[k];
    if (op == MV_COLOR_BRIGHTNESS) {
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int j = 0; j < V; ++j) v[c][j] = quantise<U8>(clampf(v[c][j] * f, bound));
    } else if (op == MV_COLOR_CONTRAST) {
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int j = 0; j < V; ++j) v[c][j] = blend<U8>(v[c][j], mean, f, a, form);
    } else if (C == 3 && op == MV_COLOR_SATURATION) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float gr = grey_of(v[0][j], v[1][j], v[C - 1][j], form);
        if (U8) gr = __builtin_floorf(gr);
#pragma unroll
        for (int c = 0; c < C; ++c) v[c][j] = blend<U8>(v[c][j], gr, f, a, form);
      }
    } else if (C == 3 && op == MV_COLOR_HUE) {
#pragma unroll
      for (int j = 0; j < V; ++j) hue_pixel<U8>(v[0][j], v[1][j], v[C - 1][j], f);
    }
  }
}

// Pass 1 of a chain with contrast: the sum over one image of the grey values of the chain in front of contrast.  Workgroup b
// covers chunk b % chunks of image b / chunks, kSumItems groups of V pixels per lane.
template <typename T, int C, bool VEC>
__global__ __launch_bounds__(kThreads) void k_color_sum(const T* __restrict__ x, long long hw, long long groups, int chunks,
                                                       Chain ch, int form, unsigned long long* __restrict__ sums_u8,
                                                       double* __restrict__ partials) {
  constexpr int V = Vec<T>::V;
  constexpr bool U8 = sizeof(T) == 1;
  const long long img = blockIdx.x / (unsigned)chunks;
  const int chunk = (int)(blockIdx.x % (unsigned)chunks);
  const T* base = x + (size_t)img * C * hw;
  unsigned long long isum = 0;
  double fsum = 0.0;
#pragma unroll 1
  for (int it = 0; it < kSumItems; ++it) {
    const long long g = ((long long)chunk * kSumItems + it) * kThreads + threadIdx.x;
    if (g >= groups) break;
    const long long p0 = g * V;
    float v[C][V];
    load<T, C, VEC>(base, hw, p0, v);
    run_ops<U8, C, V>(ch, 0, ch.contrast, form, 0.f, v);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (p0 + j >= hw) continue;
      float gr = C == 3 ? grey_of(v[0][j], v[1][j], v[C - 1][j], form) : v[0][j];
      if (U8) isum += (unsigned long long)__builtin_floorf(gr);
      else fsum += (double)gr;
    }
  }
  __shared__ double part[kThreads / kWave];
  __shared__ unsigned long long ipart[kThreads / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (U8) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) isum += __shfl_xor(isum, o);
    if (lane == 0) ipart[wave] = isum;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long s = 0;
      for (int w = 0; w < kThreads / kWave; ++w) s += ipart[w];
      atomicAdd(sums_u8 + img, s);
    }
  } else {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) fsum += __shfl_xor(fsum, o);  // a fixed tree: the same bits on every run
    if (lane == 0) part[wave] = fsum;
    __syncthreads();
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int w = 0; w < kThreads / kWave; ++w) s += part[w];
      partials[(size_t)img * chunks + chunk] = s;
    }
  }
}

// the images' uint8 sums to zero, one slot per lane (a kernel rather than hipMemsetAsync: in a captured graph the memset node did
// not zero the slots again on the second replay and the sums of the replays added up -- see k_zero_hist, autoaug.hip)
__global__ __launch_bounds__(kThreads) void k_color_zero(unsigned long long* __restrict__ sums_u8, long long images) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < images) sums_u8[i] = 0;
}

// Pass 2: the mean of each image (one workgroup per image)
__global__ __launch_bounds__(kThreads) void k_color_mean(bool u8, long long hw, int chunks,
                                                        const unsigned long long* __restrict__ sums_u8,
                                                        const double* __restrict__ partials, float* __restrict__ means) {
  const long long img = blockIdx.x;
  if (u8) {
    if (threadIdx.x == 0) means[img] = (float)sums_u8[img] / (float)hw;
    return;
  }
  double s = 0.0;
  for (int k = threadIdx.x; k < chunks; k += kThreads) s += partials[(size_t)img * chunks + k];
  __shared__ double part[kThreads];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) means[img] = (float)(part[0] / (double)hw);
}

// The chain on every pixel.  Workgroup b covers chunk b % chunks of image b / chunks, one group of V pixels per lane.
template <typename T, int C, bool VEC>
__global__ __launch_bounds__(kThreads) void k_color(const T* __restrict__ x, T* __restrict__ y, long long hw, long long groups,
                                                   int chunks, Chain ch, int form, const float* __restrict__ means) {
  constexpr int V = Vec<T>::V;
  const long long img = blockIdx.x / (unsigned)chunks;
  const long long g = (long long)(blockIdx.x % (unsigned)chunks) * kThreads + threadIdx.x;
  if (g >= groups) return;
  const float mean = ch.contrast < ch.n ? means[img] : 0.f;
  const size_t off = (size_t)img * C * hw;
  float v[C][V];
  load<T, C, VEC>(x + off, hw, g * V, v);
  run_ops<sizeof(T) == 1, C, V>(ch, 0, ch.n, form, mean, v);
  store<T, C, VEC>(y + off, hw, g * V, v);
}

// rgb_to_grayscale: the grey value (uint8: truncated by .to(uint8)) into `out_c` planes
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void k_grayscale(const T* __restrict__ x, T* __restrict__ y, long long hw,
                                                       long long groups, int chunks, int out_c, int form) {
  constexpr int V = Vec<T>::V;
  const long long img = blockIdx.x / (unsigned)chunks;
  const long long g = (long long)(blockIdx.x % (unsigned)chunks) * kThreads + threadIdx.x;
  if (g >= groups) return;
  float v[3][V];
  load<T, 3, VEC>(x + (size_t)img * 3 * hw, hw, g * V, v);
  float o[1][V];
#pragma unroll
  for (int j = 0; j < V; ++j) o[0][j] = quantise<sizeof(T) == 1>(grey_of(v[0][j], v[1][j], v[2][j], form));
  T* dst = y + (size_t)img * out_c * hw;
  for (int c = 0; c < out_c; ++c) store<T, 1, VEC>(dst + (size_t)c * hw, hw, g * V, o);
}

// workspace: means (images floats, padded to 16 B), then the uint8 sums (images x 8 B) or the float32 partials
// (images x chunks doubles)
long long sum_chunks(long long hw, bool u8) {
  const long long groups = (hw + (u8 ? 16 : 4) - 1) / (u8 ? 16 : 4);
  return (groups + (long long)kThreads * kSumItems - 1) / ((long long)kThreads * kSumItems);
}

long long means_bytes(long long images) { return (images * 4 + 15) / 16 * 16; }

template <typename T, int C, bool VEC>
int launch_chain(const T* x, T* y, long long images, long long hw, const Chain& ch, int form, void* ws, hipStream_t s) {
  constexpr int V = Vec<T>::V;
  constexpr bool U8 = sizeof(T) == 1;
  const long long groups = (hw + V - 1) / V;
  float* means = static_cast<float*>(ws);
  if (ch.contrast < ch.n) {
    char* rest = static_cast<char*>(ws) + means_bytes(images);
    auto* sums = reinterpret_cast<unsigned long long*>(rest);
    auto* partials = reinterpret_cast<double*>(rest);
    const long long chunks = sum_chunks(hw, U8);
    if (U8) {
      hipLaunchKernelGGL(k_color_zero, dim3((unsigned)((images + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, sums, images);
      if (int rc = check_launch("k_color_zero")) return rc;
    }
    hipLaunchKernelGGL((k_color_sum<T, C, VEC>), dim3((unsigned)(images * chunks)), dim3(kThreads), 0, s, x, hw, groups,
                       (int)chunks, ch, form, sums, partials);
    if (int rc = check_launch("k_color_sum")) return rc;
    hipLaunchKernelGGL(k_color_mean, dim3((unsigned)images), dim3(kThreads), 0, s, U8, hw, (int)chunks, sums, partials, means);
    if (int rc = check_launch("k_color_mean")) return rc;
  }
  const long long chunks = (groups + kThreads - 1) / kThreads;
  hipLaunchKernelGGL((k_color<T, C, VEC>), dim3((unsigned)(images * chunks)), dim3(kThreads), 0, s, x, y, hw, groups,
                     (int)chunks, ch, form, means);
  return check_launchf("k_color<%s,c%d,%s,ops%d%s>", U8 ? "u8" : "f32", C, VEC ? "vec16" : "px", ch.n,
                       ch.contrast < ch.n ? ",mean" : "");
}

template <typename T>
int chain(const T* x, T* y, long long images, int channels, long long hw, const Chain& ch, int form, void* ws,
          hipStream_t s) {
  const bool vec = vec_ok(x, y, hw, Vec<T>::V);
  if (channels == 3)
    return vec ? launch_chain<T, 3, true>(x, y, images, hw, ch, form, ws, s)
               : launch_chain<T, 3, false>(x, y, images, hw, ch, form, ws, s);
  return vec ? launch_chain<T, 1, true>(x, y, images, hw, ch, form, ws, s)
             : launch_chain<T, 1, false>(x, y, images, hw, ch, form, ws, s);
}

template <typename T>
int grayscale(const T* x, T* y, long long images, long long hw, int out_c, int form, hipStream_t s) {
  constexpr int V = Vec<T>::V;
  const long long groups = (hw + V - 1) / V, chunks = (groups + kThreads - 1) / kThreads;
  const bool vec = vec_ok(x, y, hw, V);
  const dim3 grid((unsigned)(images * chunks));
  if (vec) hipLaunchKernelGGL((k_grayscale<T, true>), grid, dim3(kThreads), 0, s, x, y, hw, groups, (int)chunks, out_c, form);
  else hipLaunchKernelGGL((k_grayscale<T, false>), grid, dim3(kThreads), 0, s, x, y, hw, groups, (int)chunks, out_c, form);
  return check_launchf("k_grayscale<%s,%s,out%d>", sizeof(T) == 1 ? "u8" : "f32", vec ? "vec16" : "px", out_c);
}

}  // namespace

int64_t color_workspace_bytes(int64_t images, int h, int w, bool u8) {
  const long long hw = (long long)h * w;
  return means_bytes(images) + (u8 ? images * 8 : images * sum_chunks(hw, false) * 8);
}

bool color_grid_fits(int64_t images, int h, int w, bool u8) {
  const long long hw = (long long)h * w, v = u8 ? 16 : 4;
  const long long chunks = ((hw + v - 1) / v + kThreads - 1) / kThreads;
  return images * chunks <= 0xffffffffLL && images * sum_chunks(hw, u8) <= 0xffffffffLL;
}

int launch_color_chain(const void* x, void* y, bool u8, int64_t images, int channels, int h, int w, const int* ops,
                       const double* factors, int n_ops, int form, void* ws, hipStream_t s) {
  Chain ch{};
  ch.n = n_ops;
  ch.contrast = n_ops;
  for (int k = 0; k < n_ops; ++k) {
    ch.op[k] = ops[k];
    ch.f[k] = (float)factors[k];
    ch.a[k] = (float)(1.0 - factors[k]);
    if (ops[k] == MV_COLOR_CONTRAST) ch.contrast = k;
  }
  const long long hw = (long long)h * w;
  if (u8) return chain((const uint8_t*)x, (uint8_t*)y, images, channels, hw, ch, form, ws, s);
  return chain((const float*)x, (float*)y, images, channels, hw, ch, form, ws, s);
}

int launch_rgb_to_grayscale(const void* x, void* y, bool u8, int64_t images, int h, int w, int out_channels, int form,
                            hipStream_t s) {
  const long long hw = (long long)h * w;
  if (u8) return grayscale((const uint8_t*)x, (uint8_t*)y, images, hw, out_channels, form, s);
  return grayscale((const float*)x, (float*)y, images, hw, out_channels, form, s);
}

}  // namespace mv
