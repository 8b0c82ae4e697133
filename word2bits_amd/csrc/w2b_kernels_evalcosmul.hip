// w2b_kernels_evalcosmul.hip -- the 3CosMul question on bit-packed 1-bit rows (include/word2bits_eval.h, "3CosMul").
// (The 2-bit form is the COSMUL instance of k_codes_scan in w2b_kernels_evalcodes.hip: same scan, another epilogue.)
//
// For a question (b1, b2, b3) and a row c the three agreement counts A_i = D - Hamming(b_i, c) are needed on their own, so
// the two planes of w2b_kernels_evalbits.hip do not serve: a lane keeps the three rows' sign words themselves, 3 * NW
// registers up to 1024 columns, read from the rows in memory beyond.  With u_i = A_i / D (utab, D + 1 floats that the host
// built with one correctly rounded division each)
//   score = (u2 * u3) / (u1 + eps)
// in float32, one rounding per operation (__fmul_rn, __fadd_rn, __fdiv_rn).  The key is the codes key, score bits << 32 |
// ~row, larger is better; rows with score > 0 qualify.
//
// Shape: that of k_bits_topk.  One lane = one question; the row index is uniform over the workgroup, so a row is a scalar
// operand; gridDim.y splits the rows; a lane keeps its k best keys, unordered, in LDS and follows the smallest of them
// (`wkey` at `wpos`; unused places hold 0, which no answer's key is); the partial lists meet in k_bits_merge.  Rows are
// visited in ascending order, so within a lane a later row has the smaller ~row: `key > wkey` lets it in only with a strictly
// larger score.
//
// Prefilter (exact: it never drops a row that would enter).  The score is within 6 roundings, a factor 1 +- 2^-21, of
//   x = A2 * A3 / (D * (A1 + eps * D)),
// so a row can reach the smallest listed score w only if  A2 * A3 >= w * D * (A1 + eps * D) * (1 - 2^-21).  The test below is
// float(A2) * float(A3) >= tm * (float(A1) + es) with es = float(eps * D) and tm = (w * D) * (1 - 2^-18): the conversions are
// exact (D <= 2^24), the two products, the sum, es and the two products in tm are six more roundings, 2^-21 again -- together
// far inside the 2^-18 that tm gives away.  With an empty place in the list w = 0 and every row passes.  Only rows that pass
// in some lane of the wavefront pay for the table reads and the division.
#include "w2b_eval_bits.hpp"

namespace {

constexpr float kCosmulEps = 1e-6f;                 // 0x358637BD
constexpr float kCosmulSlack = 1.0f - 0x1p-18f;     // exact in float

// the three rows of one lane's question: NW > 0 in registers, NW == 0 left in memory (any row length).  The counts index
// utab, so the columns past `dim` are masked here (only the last two halves of a row can hold any) and do not rest on the
// file's padding bits being zero.
template <int NW>
struct Rows3w {
  uint32_t s[3][NW > 0 ? NW : 1];
  const uint32_t *p[3];
  int nw;
  uint32_t m0, m1;        // the columns that exist in halves nw - 2 and nw - 1

  __device__ __forceinline__ uint32_t valid(int w) const { return w == nw - 2 ? m0 : (w == nw - 1 ? m1 : ~0u); }

  __device__ __forceinline__ void load(const uint32_t *__restrict__ B, int nw_, int dim, int e1, int e2, int e3) {
    nw = NW > 0 ? NW : nw_;
    const int c0 = dim - 32 * (nw - 2), c1 = c0 - 32;          // c0 >= 1
    m0 = c0 >= 32 ? ~0u : (1u << c0) - 1u;
    m1 = c1 >= 32 ? ~0u : (c1 <= 0 ? 0u : (1u << c1) - 1u);
    p[0] = B + (long long)e1 * nw;
    p[1] = B + (long long)e2 * nw;
    p[2] = B + (long long)e3 * nw;
    if constexpr (NW > 0) {
#pragma unroll
      for (int t = 0; t < 3; t++)
#pragma unroll
        for (int w = 0; w < NW; w++) s[t][w] = p[t][w] & valid(w);
    }
  }
  // the Hamming distances of the three rows to the (uniform) row over the `dim` columns
  __device__ __forceinline__ void hamming(const uint32_t *__restrict__ row, uint32_t (&h)[3]) const {
    h[0] = h[1] = h[2] = 0;
    if constexpr (NW > 0) {
#pragma unroll
      for (int w = 0; w < NW; w++) {
        const uint32_t x = row[w] & valid(w);
#pragma unroll
        for (int t = 0; t < 3; t++) h[t] += __builtin_popcount(s[t][w] ^ x);
      }
    } else {
      for (int w = 0; w < nw; w++) {
        const uint32_t x = row[w], v = valid(w);
#pragma unroll
        for (int t = 0; t < 3; t++) h[t] += __builtin_popcount((p[t][w] ^ x) & v);
      }
    }
  }
};

template <int NW>
__global__ void __launch_bounds__(BTK)
k_cosmul_bits(const uint32_t *__restrict__ B, int words, int nw, int dim, const float *__restrict__ utab, float es, int nq,
              const int *__restrict__ b1, const int *__restrict__ b2, const int *__restrict__ b3, int rpb, int k,
              unsigned long long *__restrict__ slots /* [nq][gridDim.y][k] */) {
  extern __shared__ unsigned long long lst[];     // [k][BTK]
  const int q = blockIdx.x * BTK + threadIdx.x;
  if (q >= nq) return;
  unsigned long long *mine = lst + threadIdx.x;
  const int e1 = b1[q], e2 = b2[q], e3 = b3[q];
  Rows3w<NW> rw;
  rw.load(B, nw, dim, e1, e2, e3);
  for (int j = 0; j < k; j++) mine[j * BTK] = 0ull;
  unsigned long long wkey = 0ull;
  int wpos = 0;
  float tm = 0.f;
  const float fdim = (float)dim;
  const int r0 = blockIdx.y * rpb, r1 = min(words, r0 + rpb);
  for (int r = r0; r < r1; r++) {
    uint32_t h[3];
    rw.hamming(B + (long long)r * rw.nw, h);
    const float a1 = (float)(dim - (int)h[0]), a2 = (float)(dim - (int)h[1]), a3 = (float)(dim - (int)h[2]);
    const bool pass = __fmul_rn(a2, a3) >= __fmul_rn(tm, __fadd_rn(a1, es));
    if (__builtin_amdgcn_ballot_w64(pass) != 0) {
      if (pass && r != e1 && r != e2 && r != e3) {
        const float u1 = utab[dim - (int)h[0]], u2 = utab[dim - (int)h[1]], u3 = utab[dim - (int)h[2]];
        const float sc = __fdiv_rn(__fmul_rn(u2, u3), __fadd_rn(u1, kCosmulEps));
        const unsigned long long key = ((unsigned long long)__float_as_uint(sc) << 32) | (uint32_t)~r;
        if (sc > 0.f && key > wkey) {
          mine[wpos * BTK] = key;
          unsigned long long m = ~0ull;
          for (int j = 0; j < k; j++) {
            const unsigned long long v = mine[j * BTK];
            if (v < m) {
              m = v;
              wpos = j;
            }
          }
          wkey = m;
          tm = __fmul_rn(__fmul_rn(__uint_as_float((uint32_t)(m >> 32)), fdim), kCosmulSlack);
        }
      }
    }
  }
  unsigned long long *out = slots + ((long long)q * gridDim.y + blockIdx.y) * k;
  for (int j = 0; j < k; j++) out[j] = mine[j * BTK];
}

constexpr int kMaxNW = 32;   // the three rows in registers up to 32 halves (1024 columns), in memory beyond

}  // namespace

hipError_t w2b_launch_cosmul_bits(const uint32_t *B, int words, int dim, const float *utab, int nq, const int *b1,
                                  const int *b2, const int *b3, int k, int splits, int rows_per_split,
                                  unsigned long long *slots, unsigned long long *out, hipStream_t s) {
  if (nq <= 0 || words <= 0) return hipSuccess;
  const int nw = (dim + 63) / 64 * 2;
  const dim3 grid((unsigned)((nq + BTK - 1) / BTK), (unsigned)splits);
  const size_t lds = (size_t)k * BTK * sizeof(unsigned long long);
  const float es = kCosmulEps * (float)dim;
  hipError_t e = dispatch_nw<kMaxNW>(nw, [&](auto n) {
    constexpr int NW = decltype(n)::value;
    hipLaunchKernelGGL((k_cosmul_bits<NW>), grid, dim3(BTK), lds, s, B, words, nw, dim, utab, es, nq, b1, b2, b3,
                       rows_per_split, k, slots);
    return hipGetLastError();
  });
  if (e != hipSuccess) return e;
  return w2b_launch_bits_merge(slots, splits * k, k, nq, out, s);
}
