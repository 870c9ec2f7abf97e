// mv_topk.h -- the wave-level histogram step of the radix selects (hist_add: rpn.hip k_rpn_topk, and select_keys here), the radix
// select of the k greatest 64-bit keys of a workgroup (select_keys: retinanet.hip k_retinanet_chunks and k_retinanet_rank, ssd.hip
// k_ssd_topk) and the stage behind it, the selected keys gathered into LDS, ranked pairwise and stored (rank_selected:
// k_retinanet_rank and k_ssd_topk).  k_rpn_topk keeps its own compaction and ranking: its equal keys are taken in index order.
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

// The stage behind select_keys, called by the whole workgroup with its results (thr, take): the `take` keys >= thr among
// key_at(0 .. count - 1) go to cand (LDS, room for take <= kRpnMaxK keys; n_out: an LDS counter) in any order and are ranked
// pairwise there, position = #{greater keys} -- the keys are pairwise distinct, so that is their descending order;
// out[rank] = stored(key), and out[take .. seg - 1] = -1.  THREADS: the workgroup's; Index: the type key_at counts in.
template <int THREADS, typename Index, typename KeyAt, typename Stored>
__device__ inline void rank_selected(const KeyAt& key_at, Index count, unsigned long long thr, unsigned take, unsigned long long* cand,
                                     unsigned* n_out, int* out, int seg, const Stored& stored) {
  const int tid = threadIdx.x;
  if (tid == 0) *n_out = 0;
  __syncthreads();
  for (Index i = tid; i < count; i += THREADS) {
    const unsigned long long key = key_at(i);
    if (key >= thr && key != 0) {  // exactly `take` keys
      const unsigned slot = atomicAdd(n_out, 1u);
      if (slot < take) cand[slot] = key;
    }
  }
  __syncthreads();
  for (int i = tid; i < seg; i += THREADS) {
    if (i >= (int)take) {
      out[i] = -1;
      continue;
    }
    const unsigned long long ki = cand[i];
    int rank = 0;
    for (int j = 0; j < (int)take; ++j) rank += cand[j] > ki ? 1 : 0;
    out[rank] = stored(ki);
  }
}

}  // namespace mv
