// mv_topk.h -- the wave-level histogram step of the radix selects (rpn.hip k_rpn_topk, retinanet.hip).
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

}  // namespace mv
