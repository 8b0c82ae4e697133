// w2b_kernels_evalbits.hip -- the evaluator's scan on bit-packed 1-bit rows (include/word2bits_eval.h, "bits" mode).
//
// A 1-bit row is D signs, stored as the file stores them: ceil(D/64) 64-bit words, bit set = negative, padding bits
// zero (include/word2bits_corpus.h).  Here a row is 2*ceil(D/64) 32-bit halves, so that popcount-and-add is one
// instruction (v_bcnt_u32_b32).  For a question (b1, b2, b3) the coefficient of column a is
//   t[a] = s_b2[a] - s_b1[a] + s_b3[a]  in {+-1, +-3}
// and two bit planes describe it: sg (t < 0: the majority of s_b2, ~s_b1, s_b3) and m3 (|t| = 3: all three agree).
// With x = sg ^ s_c, a column adds |t| where x is clear and -|t| where it is set:
//   I(c) = (D + 2*n3) - 2*(pop(x) + 2*pop(x & m3)),   n3 = pop(m3)
// i.e. xor, bcnt, and, bcnt per 32 columns.  The kernels rank by acc = pop(x) + 2*pop(x & m3), smaller is better; only
// acc < ceil((D + 2*n3) / 2) has I > 0.  A neighbour query (b1 = b2 = b3 = r) has sg = s_r, m3 = 0: I = D - 2*Hamming.
//
// Shape: one lane = one question, its planes in registers (2 * 2*ceil(D/64) VGPRs; rows longer than 1024 columns read
// the planes from memory instead).  The row index is uniform over the workgroup, so a row is a scalar operand fetched
// through the constant cache, and a lane needs no cross-lane step: it carries its own best (top-1) or its own list of
// the k best (top-k, in LDS).  gridDim.y splits the rows so that the device is full; the partial results meet in a
// 64-bit atomic max (top-1) or in k_bits_merge (top-k).  Rows are visited in ascending order and a later row has to be
// strictly better, so equal scores resolve to the lowest row exactly as the answer list demands.  The rank of a given row
// (k_bits_rank) carries no best and no list: two counts per lane, met in an integer atomic add.
// (BT1, BTK, bits_key and dispatch_nw: w2b_eval_bits.hpp, shared with the scan of signed sums.)
#include "w2b_eval_bits.hpp"

namespace {

// planes of `nq` questions, P[w][nqp] = sg and P[nw + w][nqp] = m3 for the 32-bit half w (question-minor: a wave's loads coalesce)
__global__ void k_bits_planes(const uint32_t *__restrict__ B, int nw, int dim, int nq, long long nqp,
                              const int *__restrict__ b1, const int *__restrict__ b2, const int *__restrict__ b3,
                              uint32_t *__restrict__ P) {
  const long long n = (long long)nq * nw;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int w = (int)(i / nq), q = (int)(i - (long long)w * nq);
    const int cols = dim - 32 * w;                                   // columns of this half that exist
    const uint32_t valid = cols >= 32 ? ~0u : (cols <= 0 ? 0u : (1u << cols) - 1u);
    const uint32_t n1 = ~B[(long long)b1[q] * nw + w], s2 = B[(long long)b2[q] * nw + w], s3 = B[(long long)b3[q] * nw + w];
    P[(long long)w * nqp + q] = ((s2 & n1) | (s2 & s3) | (n1 & s3)) & valid;
    P[(long long)(nw + w) * nqp + q] = ~((s2 ^ n1) | (s2 ^ s3)) & valid;
  }
}

// a workgroup-uniform address, kept apart from the lane's offset so that a load takes it as its scalar base
__device__ __forceinline__ const uint32_t *scalar_base(const uint32_t *u) {
  const unsigned long long a = (unsigned long long)u;
  return (const uint32_t *)(((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                            (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a));
}

// the planes of one lane: NW > 0 in registers, NW == 0 left in memory (any row length)
template <int NW>
struct Planes {
  uint32_t sg[NW > 0 ? NW : 1], m3[NW > 0 ? NW : 1];
  const uint32_t *p;      // P + q
  long long nqp;
  int nw;
  uint32_t n3;

  // SBASE: every load as (uniform address of the half)[q], a scalar base and ONE 32-bit lane offset, instead of (P + q)[uniform
  // offset], a pair of address registers per load in flight
  template <bool SBASE = false>
  __device__ __forceinline__ void load(const uint32_t *__restrict__ P, long long nqp_, int nw_, int q) {
    p = P + q;
    nqp = nqp_;
    nw = NW > 0 ? NW : nw_;
    n3 = 0;
    if constexpr (NW > 0) {
#pragma unroll
      for (int w = 0; w < NW; w++) {
        sg[w] = SBASE ? scalar_base(P + (long long)w * nqp)[(uint32_t)q] : p[(long long)w * nqp];
        m3[w] = SBASE ? scalar_base(P + (long long)(NW + w) * nqp)[(uint32_t)q] : p[(long long)(NW + w) * nqp];
        n3 += __builtin_popcount(m3[w]);
      }
    } else {
      for (int w = 0; w < nw; w++) n3 += __builtin_popcount(p[(long long)(nw + w) * nqp]);
    }
  }
  // pop(x) + 2*pop(x & m3) against the (uniform) row
  __device__ __forceinline__ uint32_t acc(const uint32_t *__restrict__ row) const {
    uint32_t a1 = 0, a3 = 0;
    if constexpr (NW > 0) {
#pragma unroll
      for (int w = 0; w < NW; w++) {
        const uint32_t x = sg[w] ^ row[w];
        a1 += __builtin_popcount(x);
        a3 += __builtin_popcount(x & m3[w]);
      }
    } else {
      for (int w = 0; w < nw; w++) {
        const uint32_t x = p[(long long)w * nqp] ^ row[w];
        a1 += __builtin_popcount(x);
        a3 += __builtin_popcount(x & p[(long long)(nw + w) * nqp]);
      }
    }
    return a1 + 2 * a3;
  }
};

template <int NW>
__global__ void __launch_bounds__(BT1)
k_bits_top1(const uint32_t *__restrict__ B, int words, int nw, int dim, const uint32_t *__restrict__ P, long long nqp, int nq,
            const int *__restrict__ b1, const int *__restrict__ b2, const int *__restrict__ b3, int rpb,
            unsigned long long *__restrict__ best) {
  const int q = blockIdx.x * BT1 + threadIdx.x;
  if (q >= nq) return;
  Planes<NW> pl;
  pl.load(P, nqp, nw, q);
  const uint32_t c = (uint32_t)dim + 2 * pl.n3;
  const int e1 = b1[q], e2 = b2[q], e3 = b3[q];
  uint32_t bacc = (c + 1) >> 1;           // acc must be below: I = c - 2*acc > 0
  int brow = -1;
  const int r0 = blockIdx.y * rpb, r1 = min(words, r0 + rpb);
#pragma unroll 2
  for (int r = r0; r < r1; r++) {
    const uint32_t a = pl.acc(B + (long long)r * pl.nw);
    if (__builtin_amdgcn_ballot_w64(a < bacc) != 0) {                 // rare after the first rows of the range
      if (a < bacc && r != e1 && r != e2 && r != e3) {
        bacc = a;
        brow = r;
      }
    }
  }
  if (brow >= 0) atomicMax(&best[q], bits_key(c, bacc, brow));
}

// The place of a given row (include/word2bits_eval.h, "rank of a given row"): the shape of k_bits_top1 with a count for an
// epilogue.  k_bits_rank_targets, one lane per question with the planes left in memory, runs first: acc of the target row
// (a per-lane address: vector loads), whether the target ranks at all (I = c - 2 acc > 0 and not one of the question's
// rows), and what the rows that the answer list leaves out -- the question's distinct rows and the target itself -- will
// add to the two counts of the scan, which excludes nothing.  The scan's row loop is then acc and two counts: the rows that
// stand before the target (a smaller acc, or the same acc and a lower row: acc < t + (row < g)) and the rows with exactly
// its acc -- three compares and three adds with carry, no ballot, no branch, no LDS.
// The row ranges' counts meet in one 64-bit integer add per lane (low half: before, high half: equal; neither overflows
// 32 bits), so the sum cannot depend on the split.
constexpr uint32_t kNoRank = 0xFFFFFFFFu;     // tacc of a target without a rank (an acc is at most 3 * dim)

__global__ void __launch_bounds__(BT1)
k_bits_rank_targets(const uint32_t *__restrict__ B, int nw, int dim, const uint32_t *__restrict__ P, long long nqp, int nq,
                    const int *__restrict__ b1, const int *__restrict__ b2, const int *__restrict__ b3,
                    const int *__restrict__ target, uint2 *__restrict__ tacc, uint2 *__restrict__ corr, int *__restrict__ tscore) {
  const int q = blockIdx.x * BT1 + threadIdx.x;
  if (q >= nq) return;
  Planes<0> pl;
  pl.load(P, nqp, nw, q);
  const uint32_t c = (uint32_t)dim + 2 * pl.n3;
  const int g = target[q];
  const int own[3] = {b1[q], b2[q], b3[q]};
  const uint32_t ta = pl.acc(B + (long long)g * nw);
  const bool ranked = ta < ((c + 1) >> 1) && g != own[0] && g != own[1] && g != own[2];
  uint32_t before = 0, equal = 1;                        // the target itself has its own acc
#pragma unroll
  for (int i = 0; i < 3; i++) {
    if ((i > 0 && own[i] == own[0]) || (i > 1 && own[i] == own[1])) continue;
    const uint32_t a = pl.acc(B + (long long)own[i] * nw);
    before += a < ta + (own[i] < g ? 1u : 0u) ? 1u : 0u;
    equal += a == ta ? 1u : 0u;
  }
  tacc[q] = make_uint2(ranked ? ta : kNoRank, (uint32_t)g);
  tscore[q] = ranked ? (int)(c - 2 * ta) : 0;
  corr[q] = ranked ? make_uint2(before, equal) : make_uint2(0u, 0u);
}

template <int NW>
__global__ void __launch_bounds__(BT1)
k_bits_rank(const uint32_t *__restrict__ B, int words, int nw, const uint32_t *__restrict__ P, long long nqp, int nq,
            const uint2 *__restrict__ tacc, int rpb, unsigned long long *__restrict__ cnt) {
  const int q = blockIdx.x * BT1 + threadIdx.x;
  if (q >= nq) return;
  Planes<NW> pl;
  pl.template load<true>(P, nqp, nw, q);
  const uint2 tq = tacc[q];                // one load: (acc of the target, the target's row)
  const uint32_t ta = tq.x;
  const int g = (int)tq.y;
  uint32_t before = 0, equal = 0;
  const int r0 = blockIdx.y * rpb, r1 = min(words, r0 + rpb);
  // (one row per trip like top-1: the loop vectoriser would interleave four over a second copy of the planes)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
  for (int r = r0; r < r1; r++) {
    const uint32_t a = pl.acc(B + (long long)r * pl.nw);
    before += a < ta + (r < g ? 1u : 0u) ? 1u : 0u;
    equal += a == ta ? 1u : 0u;
  }
  if (ta != kNoRank && (before | equal) != 0u) atomicAdd(&cnt[q], ((unsigned long long)equal << 32) | before);
}

// Top-k: the lane's k best so far as (acc << 32 | row), unordered, in LDS; `wacc`/`wpos` follow the worst of them (the
// largest entry).  Unused places hold the sentinel (first non-positive acc << 32 | ~0), which is worse than any row.
// A row enters only if its acc is strictly below the worst one's: an equal acc with a higher row loses.
template <int NW>
__global__ void __launch_bounds__(BTK)
k_bits_topk(const uint32_t *__restrict__ B, int words, int nw, int dim, const uint32_t *__restrict__ P, long long nqp, int nq,
            const int *__restrict__ b1, const int *__restrict__ b2, const int *__restrict__ b3, int rpb, int k,
            unsigned long long *__restrict__ slots /* [nq][gridDim.y][k] */) {
  extern __shared__ unsigned long long lst[];     // [k][BTK]
  const int q = blockIdx.x * BTK + threadIdx.x;
  if (q >= nq) return;
  unsigned long long *mine = lst + threadIdx.x;
  Planes<NW> pl;
  pl.load(P, nqp, nw, q);
  const uint32_t c = (uint32_t)dim + 2 * pl.n3;
  const int e1 = b1[q], e2 = b2[q], e3 = b3[q];
  const unsigned long long none = ((unsigned long long)((c + 1) >> 1) << 32) | 0xFFFFFFFFull;
  for (int j = 0; j < k; j++) mine[j * BTK] = none;
  uint32_t wacc = (c + 1) >> 1;
  int wpos = 0;
  const int r0 = blockIdx.y * rpb, r1 = min(words, r0 + rpb);
  for (int r = r0; r < r1; r++) {
    const uint32_t a = pl.acc(B + (long long)r * pl.nw);
    if (__builtin_amdgcn_ballot_w64(a < wacc) != 0) {
      if (a < wacc && r != e1 && r != e2 && r != e3) {
        mine[wpos * BTK] = ((unsigned long long)a << 32) | (uint32_t)r;
        unsigned long long m = 0;
        for (int j = 0; j < k; j++) {
          const unsigned long long v = mine[j * BTK];
          if (v > m) {
            m = v;
            wpos = j;
          }
        }
        wacc = (uint32_t)(m >> 32);
      }
    }
  }
  unsigned long long *out = slots + ((long long)q * gridDim.y + blockIdx.y) * k;
  for (int j = 0; j < k; j++) {
    const unsigned long long v = mine[j * BTK];
    out[j] = v == none ? 0ull : bits_key(c, (uint32_t)(v >> 32), (int)(uint32_t)v);
  }
}

// One wavefront per question: the k largest of its n = splits * k keys, descending.  Round j finds the largest key
// below the one of round j - 1 (keys are unique per row; 0 = no row).
__global__ void __launch_bounds__(64)
k_bits_merge(const unsigned long long *__restrict__ slots, int n, int k, unsigned long long *__restrict__ out) {
  const int q = blockIdx.x, tid = threadIdx.x;
  const unsigned long long *keys = slots + (long long)q * n;
  unsigned long long prev = ~0ull;
  for (int j = 0; j < k; j++) {
    unsigned long long best = 0ull;
    if (prev) {
      for (int i = tid; i < n; i += 64) {
        const unsigned long long v = keys[i];
        best = (v < prev && v > best) ? v : best;
      }
#pragma unroll
      for (int d = 32; d; d >>= 1) {
        const unsigned long long o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
      }
    }
    if (tid == 0) out[(long long)q * k + j] = best;
    prev = best;
  }
}

constexpr int kMaxNW = 32;   // planes in registers up to 32 halves (1024 columns), in memory beyond

}  // namespace

hipError_t w2b_launch_bits_planes(const uint32_t *B, int nw, int dim, int nq, long long nqp, const int *b1, const int *b2,
                                  const int *b3, uint32_t *P, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  const long long n = (long long)nq * nw;
  const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(k_bits_planes, dim3(blocks), dim3(256), 0, s, B, nw, dim, nq, nqp, b1, b2, b3, P);
  return hipGetLastError();
}

// Row ranges of one launch: enough workgroups (question blocks x splits) to fill the device a few times over, never
// fewer than 64 rows per range.  `max_splits` caps it (top-k: the slot scratch grows with the splits).
void w2b_bits_layout(long long words, long long nq, int topk, int max_splits, int *splits, int *rows_per_split) {
  const long long bt = topk ? BTK : BT1, qb = (nq + bt - 1) / bt;
  long long s = 2048 / (qb > 0 ? qb : 1);
  if (s > (words + 63) / 64) s = (words + 63) / 64;
  if (s > 1024) s = 1024;
  if (max_splits > 0 && s > max_splits) s = max_splits;
  if (s < 1) s = 1;
  const long long rpb = words > 0 ? (words + s - 1) / s : 1;
  *rows_per_split = (int)rpb;
  *splits = words > 0 ? (int)((words + rpb - 1) / rpb) : 1;
}

hipError_t w2b_launch_bits_top1(const uint32_t *B, int words, int dim, const uint32_t *P, long long nqp, int nq,
                                const int *b1, const int *b2, const int *b3, unsigned long long *best, hipStream_t s) {
  if (nq <= 0 || words <= 0) return hipSuccess;
  const int nw = (dim + 63) / 64 * 2;
  int splits = 1, rpb = 1;
  w2b_bits_layout(words, nq, 0, 0, &splits, &rpb);
  const dim3 grid((unsigned)((nq + BT1 - 1) / BT1), (unsigned)splits);
  return dispatch_nw<kMaxNW>(nw, [&](auto n) {
    constexpr int NW = decltype(n)::value;
    hipLaunchKernelGGL((k_bits_top1<NW>), grid, dim3(BT1), 0, s, B, words, nw, dim, P, nqp, nq, b1, b2, b3, rpb, best);
    return hipGetLastError();
  });
}

hipError_t w2b_launch_bits_rank(const uint32_t *B, int words, int dim, const uint32_t *P, long long nqp, int nq,
                                const int *b1, const int *b2, const int *b3, const int *target, unsigned long long *cnt,
                                unsigned int *corr, int *tscore, unsigned int *tacc /* [nq][2] */, hipStream_t s) {
  if (nq <= 0 || words <= 0) return hipSuccess;
  const int nw = (dim + 63) / 64 * 2;
  const unsigned qblocks = (unsigned)((nq + BT1 - 1) / BT1);
  hipLaunchKernelGGL(k_bits_rank_targets, dim3(qblocks), dim3(BT1), 0, s, B, nw, dim, P, nqp, nq, b1, b2, b3, target, (uint2 *)tacc,
                     (uint2 *)corr, tscore);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  int splits = 1, rpb = 1;
  w2b_bits_layout(words, nq, 0, 0, &splits, &rpb);
  const dim3 grid(qblocks, (unsigned)splits);
  return dispatch_nw<kMaxNW>(nw, [&](auto n) {
    constexpr int NW = decltype(n)::value;
    hipLaunchKernelGGL((k_bits_rank<NW>), grid, dim3(BT1), 0, s, B, words, nw, P, nqp, nq, (const uint2 *)tacc, rpb, cnt);
    return hipGetLastError();
  });
}

hipError_t w2b_launch_bits_merge(const unsigned long long *slots, int n, int k, int nq, unsigned long long *out,
                                 hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_bits_merge, dim3((unsigned)nq), dim3(64), 0, s, slots, n, k, out);
  return hipGetLastError();
}

hipError_t w2b_launch_bits_topk(const uint32_t *B, int words, int dim, const uint32_t *P, long long nqp, int nq,
                                const int *b1, const int *b2, const int *b3, int k, int splits, int rows_per_split,
                                unsigned long long *slots, unsigned long long *out, hipStream_t s) {
  if (nq <= 0 || words <= 0) return hipSuccess;
  const int nw = (dim + 63) / 64 * 2;
  const dim3 grid((unsigned)((nq + BTK - 1) / BTK), (unsigned)splits);
  const size_t lds = (size_t)k * BTK * sizeof(unsigned long long);
  hipError_t e = dispatch_nw<kMaxNW>(nw, [&](auto n) {
    constexpr int NW = decltype(n)::value;
    hipLaunchKernelGGL((k_bits_topk<NW>), grid, dim3(BTK), lds, s, B, words, nw, dim, P, nqp, nq, b1, b2, b3,
                       rows_per_split, k, slots);
    return hipGetLastError();
  });
  if (e != hipSuccess) return e;
  return w2b_launch_bits_merge(slots, splits * k, k, nq, out, s);
}
