// mv_vec16.h -- the 16-byte access layout of the pointwise image kernels (color.hip, autoaug.hip): a lane owns V pixels of a
// plane (float 4, uint8 16) and moves them with one 16-byte load or store when the plane length and both pointers allow it,
// pixel by pixel otherwise.  Values travel as float (uint8 pixels as their integers).
#pragma once

#include "mv_common.h"

namespace mv {
namespace {

template <typename T>
struct Vec;
template <>
struct Vec<float> {
  static constexpr int V = 4;
  using Raw = float4;
  __device__ static void unpack(const Raw& w, float (&o)[V]) { o[0] = w.x, o[1] = w.y, o[2] = w.z, o[3] = w.w; }
  __device__ static Raw pack(const float (&o)[V]) { return make_float4(o[0], o[1], o[2], o[3]); }
};
template <>
struct Vec<uint8_t> {
  static constexpr int V = 16;
  using Raw = uint4;
  __device__ static void unpack(const Raw& w, float (&o)[V]) {
    const unsigned d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = (float)((d[j >> 2] >> (8 * (j & 3))) & 0xffu);
  }
  __device__ static Raw pack(const float (&o)[V]) {
    unsigned d[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < V; ++j) d[j >> 2] |= (unsigned)o[j] << (8 * (j & 3));  // o[j] is an integer in [0, 255]
    return make_uint4(d[0], d[1], d[2], d[3]);
  }
};

// the lane's group of V pixels starting at pixel p0 of each plane (planes of hw elements from base); VEC: one 16-byte load
template <typename T, int C, bool VEC>
__device__ inline void load(const T* __restrict__ base, long long hw, long long p0, float (&v)[C][Vec<T>::V]) {
  constexpr int V = Vec<T>::V;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const T* src = base + (size_t)c * hw + p0;
    if (VEC) {
      Vec<T>::unpack(*reinterpret_cast<const typename Vec<T>::Raw*>(src), v[c]);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) v[c][j] = p0 + j < hw ? (float)src[j] : 0.f;
    }
  }
}

template <typename T, int C, bool VEC>
__device__ inline void store(T* __restrict__ base, long long hw, long long p0, const float (&v)[C][Vec<T>::V]) {
  constexpr int V = Vec<T>::V;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    T* dst = base + (size_t)c * hw + p0;
    if (VEC) {
      *reinterpret_cast<typename Vec<T>::Raw*>(dst) = Vec<T>::pack(v[c]);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (p0 + j < hw) dst[j] = (T)v[c][j];
    }
  }
}

inline bool vec_ok(const void* x, const void* y, long long hw, int v) {
  return hw % v == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0;
}

}  // namespace
}  // namespace mv
