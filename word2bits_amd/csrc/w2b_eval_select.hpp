// w2b_eval_select.hpp -- the top-k selection state that the evaluator's scan kernels share (w2b_kernels_eval.hip: fp32
// rows, w2b_kernels_evalcodes.hip: 2-bit rows, w2b_kernels_evalbag.hip, w2b_kernels_evalvec.hip).  Device code; the description of the scheme is in w2b_kernels_eval.hip.
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

// The selection of one 32-row unit of an MFMA scan whose rows are the A operand: the unit's scores for question q sit in the
// lane pair (l, l ^ 32), accumulator e of lane half hh being row rbase + 8 (e / 4) + 4 hh + e % 4.  u[e] = the score bits of
// the key (score bits << 32 | ~row), 0 where the row is no answer; `may` = this lane's question is live and its largest u
// reaches the bound `seen` (the caller has found __any(may)); rows >= words are dropped here.  Candidates (keys above
// `seen`) go to the unit's slot, the cap largest of them if there are more; the bound and the buckets are raised as
// w2b_kernels_eval.hip describes.  Every lane of the wavefront must call it.
__device__ __forceinline__ void topk_select_unit32(const unsigned (&u)[16], bool may, int rbase, int h, int words, int q, int unit,
                                                   unsigned long long seen, unsigned long long *bound, const TopkArgs &tk) {
  auto row_of = [&](int e, int hh) { return rbase + 8 * (e >> 2) + 4 * hh + (e & 3); };
  auto key_of = [&](unsigned bits, int c) {
    return ((unsigned long long)bits << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)c);
  };
  unsigned cm = 0u;
  unsigned long long mx = 0ull;
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int c = row_of(e, h);
    const unsigned long long k2 = key_of(u[e], c);
    const bool ok = may && c < words && u[e] > 0u && k2 > seen;
    cm |= ok ? 1u << e : 0u;
    mx = (ok && k2 > mx) ? k2 : mx;
  }
  if (!__any(cm != 0u)) return;
  const int n_me = __builtin_popcount(cm), n_ot = __shfl_xor(n_me, 32, 64), totc = n_me + n_ot;
  const unsigned long long om = __shfl_xor(mx, 32, 64), pm = mx > om ? mx : om;   // the pair's largest candidate
  unsigned long long *slot = tk.keys + ((long long)q * tk.nunits + unit) * tk.cap;   // (used by lanes with candidates only)
  unsigned long long kth = 0ull;
  if (__any(totc > tk.cap)) {
    // more candidates than the slot holds (k < 32 only): a key's place is its rank in the pair, the first cap stay
    const unsigned cmo = __shfl_xor(cm, 32, 64);
    unsigned uq[16];
#pragma unroll
    for (int e = 0; e < 16; e++) uq[e] = __shfl_xor(u[e], 32, 64);
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const unsigned long long mine = key_of(u[e], row_of(e, h));
      int rank = 0;
#pragma unroll
      for (int x = 0; x < 16; x++) {
        const unsigned long long ka = (cm >> x) & 1u ? key_of(u[x], row_of(x, h)) : 0ull;
        const unsigned long long kb = (cmo >> x) & 1u ? key_of(uq[x], row_of(x, h ^ 1)) : 0ull;
        rank += (ka > mine ? 1 : 0) + (kb > mine ? 1 : 0);
      }
      if ((cm >> e) & 1u) {
        if (rank < tk.cap) slot[rank] = mine;
        if (rank == tk.cap - 1) kth = mine;
      }
    }
    const unsigned long long ok2 = __shfl_xor(kth, 32, 64);
    kth = ok2 > kth ? ok2 : kth;              // cap keys of this unit are >= kth
  } else {
    int pos = h ? n_ot : 0;
#pragma unroll
    for (int e = 0; e < 16; e++)
      if ((cm >> e) & 1u) slot[pos++] = key_of(u[e], row_of(e, h));
  }
  if (h == 0 && pm) {
    tk.cnt[(long long)q * tk.nunits + unit] = (unsigned char)(totc < tk.cap ? totc : tk.cap);
    if (kth && tk.cap == tk.k) atomicMax(&bound[q], kth);
    topk_note_max(tk.bkt, tk.k, bound, q, unit, pm);
  }
}

}  // namespace
