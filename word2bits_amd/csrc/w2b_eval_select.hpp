// w2b_eval_select.hpp -- the top-k selection state that the evaluator's scan kernels share (w2b_kernels_eval.hip: fp32
// rows, w2b_kernels_evalcodes.hip: 2-bit rows).  Device code; the description of the scheme is in w2b_kernels_eval.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct TopkArgs {
  unsigned long long *keys;   // [nq][nunits][cap]
  unsigned char *cnt;         // [nq][nunits]
  unsigned long long *bkt;    // [nq][k]
  int k, cap, nunits;
};

__device__ __forceinline__ unsigned long long ld_key(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// `key` is the largest candidate of (q, unit)
__device__ inline void topk_note_max(unsigned long long *bkt, int k, unsigned long long *bound, int q, int unit,
                                     unsigned long long key) {
  unsigned long long *b = bkt + (long long)q * k;
  const unsigned long long old = atomicMax(&b[unit % k], key);
  if (old >= key) return;
  const unsigned long long cur = ld_key(&bound[q]);
  if (old > cur) return;                 // the bucket was not the smallest one: the minimum stays
  unsigned long long mn = ~0ull;
#pragma unroll 8
  for (int j = 0; j < k; j++) {
    const unsigned long long v = ld_key(&b[j]);
    mn = v < mn ? v : mn;
  }
  if (mn > cur) atomicMax(&bound[q], mn);
}

}  // namespace
