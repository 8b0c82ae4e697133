// w2b_kernels_evalcombine.hip -- the evaluator's signed multi-word question (include/word2bits_eval.h, w2b_eval_combine):
// up to W2B_EVAL_MAX_TERMS = 7 rows per question, each with a sign, instead of the fixed (b2 - b1) + b3.
//
// The questions arrive as rows / signs [nq][W2B_EVAL_XSTRIDE] with the used slots first, in slot order, and row -1 /
// sign 0 in the others; the rows are at the same time the question's exclusion list.
//
// fp32 rows: k_combine_queries builds vec in slot order, one float32 add or subtract per further slot, into the Q that
// the scan kernels of w2b_kernels_eval.hip read; their list-form instantiations do the rest.
//
// 1-bit rows: the coefficient of column a is t[a] = sum over the slots of sign * s_r[a], an integer in [-7, 7], zero
// included.  A question is FOUR bit planes per 32 columns: sg (t < 0) and m0, m1, m2, the binary digits of |t|, all zero
// in the columns past the row's end.  With x = sg ^ s_c a column adds |t| where x is clear and -|t| where it is set:
//   I(c) = C - 2 * acc,   acc = pop(x & m0) + 2 pop(x & m1) + 4 pop(x & m2),   C = pop(m0) + 2 pop(m1) + 4 pop(m2)
// i.e. xor, 3 and, 3 bcnt-and-add per 32 columns, where the three-row scan of w2b_kernels_evalbits.hip needs xor, and,
// 2 bcnt.  Everything else is that scan's shape: one lane = one question, the row a uniform scalar operand, rows in
// ascending order with strict improvement (equal I resolves to the lowest row), a row is an answer only when
// acc < (C + 1) >> 1 (I > 0), gridDim.y splits the rows and the partial lists meet in k_bits_merge through the key
// (I << 32) | ~row.  k_combine_planes builds the planes: it counts the negative effective signs per column in three
// bit-sliced counter planes and turns every count n into t = used - 2 n.
//
// Registers: the planes of a lane take 4 * nw VGPRs (nw = 2 * ceil(D / 64) halves).  Kernel instances keep them in
// registers up to nw = 32 halves = 1024 columns, the same cut-off as the three-row scan: the gfx950 build reports 172
// VGPRs for the top-k and 169 for the top-1 instance at nw = 32 (61 / 56 at D = 200), no scratch and no spill in any
// instance; longer rows use the instance that reads the planes from memory (45 / 32 VGPRs, no scratch).
#include "../../include/word2bits_eval.h"
#include "w2b_eval_bits.hpp"

namespace {

constexpr int XS = W2B_EVAL_XSTRIDE;

// ------------------------------------------------------------------------------------ fp32: the query vector
// vec = +-M[r0], then one add or subtract per further used slot, each rounded on its own (this TU is built
// -ffp-contract=off, and there is nothing to contract).  Slots (+b2, -b1, +b3) give the bits of k_eval_queries.
__global__ void k_combine_queries(const float *__restrict__ M, long long ld, long long nq, const int *__restrict__ rows,
                                  const int *__restrict__ signs, float *__restrict__ Q) {
  const long long n = nq * ld;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const long long q = i / ld, a = i - q * ld;
    const int *r = rows + q * XS, *sg = signs + q * XS;
    float v = M[(long long)r[0] * ld + a];
    v = sg[0] < 0 ? -v : v;
#pragma unroll
    for (int t = 1; t < W2B_EVAL_MAX_TERMS; t++) {
      if (sg[t] == 0) break;                       // used slots come first
      const float m = M[(long long)r[t] * ld + a];
      v = sg[t] < 0 ? v - m : v + m;
    }
    Q[i] = v;
  }
}

// ------------------------------------------------------------------------------------ 1-bit rows: the planes
// P[(plane * nw + w) * nqp + q], plane 0 = sg, 1..3 = m0..m2, for the 32-bit half w (question-minor: a wave's loads coalesce)
__global__ void k_combine_planes(const uint32_t *__restrict__ B, int nw, int dim, int nq, long long nqp,
                                 const int *__restrict__ rows, const int *__restrict__ signs, uint32_t *__restrict__ P) {
  const long long n = (long long)nq * nw;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int w = (int)(i / nq), q = (int)(i - (long long)w * nq);
    const int cols = dim - 32 * w;                                   // columns of this half that exist
    const uint32_t valid = cols >= 32 ? ~0u : (cols <= 0 ? 0u : (1u << cols) - 1u);
    // n[a] = how many used slots have sign * s_r[a] = -1 (a set bit is s = -1), as the bit-sliced counter c2 c1 c0
    uint32_t c0 = 0, c1 = 0, c2 = 0;
    int used = 0;
#pragma unroll
    for (int t = 0; t < W2B_EVAL_MAX_TERMS; t++) {
      const int sg = signs[(long long)q * XS + t];
      if (sg == 0) break;
      const uint32_t s = B[(long long)rows[(long long)q * XS + t] * nw + w];
      const uint32_t neg = sg < 0 ? ~s : s;
      const uint32_t k0 = c0 & neg, k1 = c1 & k0;
      c0 ^= neg;
      c1 ^= k0;
      c2 ^= k1;
      used++;
    }
    uint32_t sgp = 0, m0 = 0, m1 = 0, m2 = 0;
    for (int v = 0; v <= used; v++) {                                // the columns with n == v have t = used - 2 v
      const uint32_t eq = ((v & 1) ? c0 : ~c0) & ((v & 2) ? c1 : ~c1) & ((v & 4) ? c2 : ~c2);
      const int t = used - 2 * v, mag = t < 0 ? -t : t;
      sgp |= t < 0 ? eq : 0u;
      m0 |= (mag & 1) ? eq : 0u;
      m1 |= (mag & 2) ? eq : 0u;
      m2 |= (mag & 4) ? eq : 0u;
    }
    P[(long long)w * nqp + q] = sgp & valid;
    P[(long long)(nw + w) * nqp + q] = m0 & valid;
    P[(long long)(2 * nw + w) * nqp + q] = m1 & valid;
    P[(long long)(3 * nw + w) * nqp + q] = m2 & valid;
  }
}

// the planes of one lane: NW > 0 in registers, NW == 0 left in memory (any row length)
template <int NW>
struct Planes4 {
  uint32_t sg[NW > 0 ? NW : 1], m0[NW > 0 ? NW : 1], m1[NW > 0 ? NW : 1], m2[NW > 0 ? NW : 1];
  const uint32_t *p;      // P + q
  long long nqp;
  int nw;
  uint32_t c;             // C = sum of |t|

  __device__ __forceinline__ void load(const uint32_t *__restrict__ P, long long nqp_, int nw_, int q) {
    p = P + q;
    nqp = nqp_;
    nw = NW > 0 ? NW : nw_;
    uint32_t n0 = 0, n1 = 0, n2 = 0;
    if constexpr (NW > 0) {
#pragma unroll
      for (int w = 0; w < NW; w++) {
        sg[w] = p[(long long)w * nqp];
        m0[w] = p[(long long)(NW + w) * nqp];
        m1[w] = p[(long long)(2 * NW + w) * nqp];
        m2[w] = p[(long long)(3 * NW + w) * nqp];
        n0 += __builtin_popcount(m0[w]);
        n1 += __builtin_popcount(m1[w]);
        n2 += __builtin_popcount(m2[w]);
      }
    } else {
      for (int w = 0; w < nw; w++) {
        n0 += __builtin_popcount(p[(long long)(nw + w) * nqp]);
        n1 += __builtin_popcount(p[(long long)(2 * nw + w) * nqp]);
        n2 += __builtin_popcount(p[(long long)(3 * nw + w) * nqp]);
      }
    }
    c = n0 + 2 * n1 + 4 * n2;
  }
  // pop(x & m0) + 2 pop(x & m1) + 4 pop(x & m2) against the (uniform) row
  __device__ __forceinline__ uint32_t acc(const uint32_t *__restrict__ row) const {
    uint32_t a0 = 0, a1 = 0, a2 = 0;
    if constexpr (NW > 0) {
#pragma unroll
      for (int w = 0; w < NW; w++) {
        const uint32_t x = sg[w] ^ row[w];
        a0 += __builtin_popcount(x & m0[w]);
        a1 += __builtin_popcount(x & m1[w]);
        a2 += __builtin_popcount(x & m2[w]);
      }
    } else {
      for (int w = 0; w < nw; w++) {
        const uint32_t x = p[(long long)w * nqp] ^ row[w];
        a0 += __builtin_popcount(x & p[(long long)(nw + w) * nqp]);
        a1 += __builtin_popcount(x & p[(long long)(2 * nw + w) * nqp]);
        a2 += __builtin_popcount(x & p[(long long)(3 * nw + w) * nqp]);
      }
    }
    return a0 + 2 * a1 + 4 * a2;
  }
};

// the rows a question's answers leave out: its own, -1 in the unused slots
struct Excluded {
  int e[W2B_EVAL_MAX_TERMS];
  __device__ __forceinline__ void load(const int *__restrict__ rows, int q) {
#pragma unroll
    for (int t = 0; t < W2B_EVAL_MAX_TERMS; t++) e[t] = rows[(long long)q * XS + t];
  }
  __device__ __forceinline__ bool hit(int r) const {
    bool h = false;
#pragma unroll
    for (int t = 0; t < W2B_EVAL_MAX_TERMS; t++) h |= r == e[t];
    return h;
  }
};

// The scan.  TOP1 (k = 1): the lane's best row in registers.  Otherwise the lane's k best so far as (acc << 32 | row),
// unordered, in LDS, exactly as k_bits_topk keeps them: `wacc` / `wpos` follow the worst of them, unused places hold a
// sentinel that is worse than any row, and a row enters only if its acc is strictly below the worst one's.  Either way
// (question, row range) writes k keys to `slots`, 0 = no row.
template <int NW, bool TOP1>
__global__ void __launch_bounds__(BTK)
k_combine_bits(const uint32_t *__restrict__ B, int words, int nw, const uint32_t *__restrict__ P, long long nqp, int nq,
               const int *__restrict__ xrows, int rpb, int k, unsigned long long *__restrict__ slots /* [nq][gridDim.y][k] */) {
  extern __shared__ unsigned long long lst[];     // [k][BTK] (none when TOP1)
  const int q = blockIdx.x * BTK + threadIdx.x;
  if (q >= nq) return;
  Planes4<NW> pl;
  pl.load(P, nqp, nw, q);
  const uint32_t c = pl.c;
  Excluded ex;
  ex.load(xrows, q);
  const int r0 = blockIdx.y * rpb, r1 = min(words, r0 + rpb);
  unsigned long long *out = slots + ((long long)q * gridDim.y + blockIdx.y) * k;
  if constexpr (TOP1) {
    uint32_t bacc = (c + 1) >> 1;           // acc must be below: I = c - 2*acc > 0
    int brow = -1;
#pragma unroll 2
    for (int r = r0; r < r1; r++) {
      const uint32_t a = pl.acc(B + (long long)r * pl.nw);
      if (__builtin_amdgcn_ballot_w64(a < bacc) != 0) {                 // rare after the first rows of the range
        if (a < bacc && !ex.hit(r)) {
          bacc = a;
          brow = r;
        }
      }
    }
    out[0] = brow >= 0 ? bits_key(c, bacc, brow) : 0ull;
  } else {
    unsigned long long *mine = lst + threadIdx.x;
    const unsigned long long none = ((unsigned long long)((c + 1) >> 1) << 32) | 0xFFFFFFFFull;
    for (int j = 0; j < k; j++) mine[j * BTK] = none;
    uint32_t wacc = (c + 1) >> 1;
    int wpos = 0;
    for (int r = r0; r < r1; r++) {
      const uint32_t a = pl.acc(B + (long long)r * pl.nw);
      if (__builtin_amdgcn_ballot_w64(a < wacc) != 0) {
        if (a < wacc && !ex.hit(r)) {
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
    for (int j = 0; j < k; j++) {
      const unsigned long long v = mine[j * BTK];
      out[j] = v == none ? 0ull : bits_key(c, (uint32_t)(v >> 32), (int)(uint32_t)v);
    }
  }
}

constexpr int kMaxNW = 32;   // planes in registers up to 32 halves (1024 columns), in memory beyond (see the header comment)

}  // namespace

hipError_t w2b_launch_combine_queries(const float *M, long long ld, long long nq, const int *rows, const int *signs,
                                      float *Q, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_combine_queries, dim3(2048), dim3(256), 0, s, M, ld, nq, rows, signs, Q);
  return hipGetLastError();
}

hipError_t w2b_launch_combine_planes(const uint32_t *B, int nw, int dim, int nq, long long nqp, const int *rows,
                                     const int *signs, uint32_t *P, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  const long long n = (long long)nq * nw;
  const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(k_combine_planes, dim3(blocks), dim3(256), 0, s, B, nw, dim, nq, nqp, rows, signs, P);
  return hipGetLastError();
}

hipError_t w2b_launch_combine_bits(const uint32_t *B, int words, int dim, const uint32_t *P, long long nqp, int nq,
                                   const int *rows, int k, int splits, int rows_per_split, unsigned long long *slots,
                                   unsigned long long *out, hipStream_t s) {
  if (nq <= 0 || words <= 0) return hipSuccess;
  const int nw = (dim + 63) / 64 * 2;
  const dim3 grid((unsigned)((nq + BTK - 1) / BTK), (unsigned)splits);
  hipError_t e = dispatch_nw<kMaxNW>(nw, [&](auto n) {
    constexpr int NW = decltype(n)::value;
    if (k == 1)
      hipLaunchKernelGGL((k_combine_bits<NW, true>), grid, dim3(BTK), 0, s, B, words, nw, P, nqp, nq, rows, rows_per_split,
                         k, slots);
    else
      hipLaunchKernelGGL((k_combine_bits<NW, false>), grid, dim3(BTK), (size_t)k * BTK * sizeof(unsigned long long), s, B,
                         words, nw, P, nqp, nq, rows, rows_per_split, k, slots);
    return hipGetLastError();
  });
  if (e != hipSuccess) return e;
  return w2b_launch_bits_merge(slots, splits * k, k, nq, out, s);
}
