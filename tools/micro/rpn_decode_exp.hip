// What the correctly rounded exp costs in a decode-shaped kernel (tools/perf_rpn.py): BoxCoder.decode_single + clip + sigmoid of
// csrc/rpn.hip on flat arrays, one lane per candidate, with E = (float)exp((double)v) (the library's) or E = expf(v).  A number for
// DESIGN.md 3.24 only: the library has one form.
// hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC -o librpn_decode_exp.so rpn_decode_exp.hip
#include <hip/hip_runtime.h>

template <bool EXPF>
__device__ inline float E(float v) {
  return EXPF ? expf(v) : (float)exp((double)v);
}

template <bool EXPF>
__global__ __launch_bounds__(256) void k_decode_exp(const float* __restrict__ anchors, const float* __restrict__ deltas,
                                                    const float* __restrict__ logits, float* __restrict__ boxes, float* __restrict__ scores,
                                                    long long count, float clip, float ih, float iw) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= count) return;
  const float x1 = anchors[t * 4], y1 = anchors[t * 4 + 1], x2 = anchors[t * 4 + 2], y2 = anchors[t * 4 + 3];
  const float w = __fsub_rn(x2, x1), h = __fsub_rn(y2, y1);
  const float cx = __fadd_rn(x1, __fmul_rn(0.5f, w)), cy = __fadd_rn(y1, __fmul_rn(0.5f, h));
  float dw = deltas[t * 4 + 2], dh = deltas[t * 4 + 3];
  dw = dw > clip ? clip : dw, dh = dh > clip ? clip : dh;
  const float pcx = __fadd_rn(__fmul_rn(deltas[t * 4], w), cx), pcy = __fadd_rn(__fmul_rn(deltas[t * 4 + 1], h), cy);
  const float hw = __fmul_rn(0.5f, __fmul_rn(E<EXPF>(dw), w)), hh = __fmul_rn(0.5f, __fmul_rn(E<EXPF>(dh), h));
  boxes[t * 4] = fminf(fmaxf(__fsub_rn(pcx, hw), 0.f), iw), boxes[t * 4 + 1] = fminf(fmaxf(__fsub_rn(pcy, hh), 0.f), ih);
  boxes[t * 4 + 2] = fminf(fmaxf(__fadd_rn(pcx, hw), 0.f), iw), boxes[t * 4 + 3] = fminf(fmaxf(__fadd_rn(pcy, hh), 0.f), ih);
  scores[t] = __fdiv_rn(1.f, __fadd_rn(1.f, E<EXPF>(-logits[t])));
}

extern "C" int rpn_decode_exp(int use_expf, const float* anchors, const float* deltas, const float* logits, float* boxes, float* scores,
                              long long count, float clip, float ih, float iw, void* stream) {
  if (count <= 0 || !anchors || !deltas || !logits || !boxes || !scores) return -1;
  const dim3 grid((unsigned)((count + 255) / 256));
  if (use_expf)
    hipLaunchKernelGGL(k_decode_exp<true>, grid, dim3(256), 0, (hipStream_t)stream, anchors, deltas, logits, boxes, scores, count, clip, ih, iw);
  else
    hipLaunchKernelGGL(k_decode_exp<false>, grid, dim3(256), 0, (hipStream_t)stream, anchors, deltas, logits, boxes, scores, count, clip, ih, iw);
  return (int)hipGetLastError();
}
