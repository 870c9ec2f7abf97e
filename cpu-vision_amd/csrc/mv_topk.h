// mv_topk.h -- the wave-level histogram step of the radix selects (rpn.hip k_rpn_topk, retinanet.hip, ssd.hip) and the radix select
// of the k greatest 64-bit keys of a workgroup (retinanet.hip, ssd.hip).
#pragma once

#include "mv_common.h"

namespace mv {

// hist[digit] += 1 for every lane with `on`, one LDS atomic per distinct digit of the wave: logits of one map share their top
// byte(s), and 64 adds to one address would serialise.  Called by whole waves.
__device__ inline void hist_add(unsigned* hist, bool on, unsigned digit, int lane) {
  unsigned long long live = __ballot(on);
  while (live) {
    const int leader = __builtin_amdgcn_readfirstlane(__builtin_ctzll(live));
    const unsigned d = (unsigned)__builtin_amdgcn_readlane((int)digit, leader);
    const unsigned long long same = __ballot(on && digit == d);
    if (lane == leader) atomicAdd(&hist[d], (unsigned)__popcll(same));
    live &= ~same;
  }
}

// The k greatest of the non-zero keys that `each` visits (it calls f(key) for every key of this thread, the same number of times
// in every thread of the workgroup; 0 = no key).  Returns T and sets *take = min(k, keys): the selected keys are those >= T.
template <typename Each>
__device__ inline unsigned long long select_keys(const Each& each, unsigned k, unsigned* hist, unsigned* sel, int tid, int lane, unsigned* take) {
  unsigned long long prefix = 0;
  unsigned rem = k;  // how many of the keys that share `prefix` are taken
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    each([&](unsigned long long key) { hist_add(hist, key != 0 && (pass == 0 || ((key >> shift) >> 8) == prefix), (unsigned)(key >> shift) & 255u, lane); });
    __syncthreads();
    if (tid < 256) {
      unsigned above = 0;
      for (int j = tid + 1; j < 256; ++j) above += hist[j];
      const unsigned mine = hist[tid];
      if (tid == 0) sel[3] = above + mine;  // every key counted in this pass
      if (above < rem && above + mine >= rem) sel[0] = (unsigned)tid, sel[1] = rem - above, sel[2] = mine;  // at most one digit
    }
    __syncthreads();  // hist and sel are next written behind the first barrier of the next pass
    if (pass == 0 && sel[3] <= k) {
      *take = sel[3];
      return 1;
    }
    prefix = (prefix << 8) | sel[0];
    rem = sel[1];
    if (sel[2] == rem) return *take = k, prefix << shift;  // the whole bin is taken: no need to look inside it
  }
  *take = k;
  return prefix;
}

}  // namespace mv
