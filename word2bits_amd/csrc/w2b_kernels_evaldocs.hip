// w2b_kernels_evaldocs.hip -- the document question on both packed forms (include/word2bits_eval.h, "documents"): which
// documents of a corpus of id lists are nearest to a query text by the relaxed word mover's similarity.
//
// A vocabulary row occurs in a corpus many times, so no (query word, document word) pair is ever scored from the packed rows
// while the corpus is walked.  Per chunk of queries there are two phases.
//
// 1. The pair table (k_docs_table, k_docs_rowmax).  The chunk's queries are laid side by side as COLUMNS: query q owns the
//    columns qcol[q] .. qcol[q + 1), a whole number of 64-byte lines, of which the first qm[q] carry its ids >= 0 (colrow[x] =
//    the row of column x) and the rest are pad (colrow = -1).  Tab[c][x] is I(x, c) (bits, int32) or cos(x, c) (codes, float32)
//    of column x against vocabulary row c; a pad column holds kPadI / kPadF, below every real value, and is never summed.
//    One lane = one column with its query row in registers (in memory beyond kMaxNW halves), the vocabulary row is uniform
//    over the workgroup and so a scalar operand: the shape of k_bits_topk.  The codes product is popcounts on the sign and
//    magnitude words (J = sum sgn * (1 + 2 mx)(1 + 2 mc)), the epilogue the neighbours epilogue: ((float)J * w(x)) * w(c),
//    both multiplies rounded on their own.
//    Rmax[c][q] = the largest Tab[c][x] over query q's own columns.  It is what a document position with id c contributes to
//    D -> Q, and it depends on the query alone, not on the document: the walk needs no cross-lane maximum per position.
//
// 2. The walk (k_docs_walk), the hot path.  A workgroup has one query and kDocsPerBlock documents; a wavefront is cut into
//    64 / W groups of W lanes, W = 16, 32 or 64 by the query's width, and a group takes one document at a time.
//      Q -> D: lane = query column.  For every position of the document the group reads the slice Tab[id][columns], one
//        contiguous read, and keeps a per-lane running maximum; four positions are in flight per lane.  A query wider than
//        64 columns walks the document once per 64-column tile.  The maxima of the columns that carry an id are converted
//        (codes: F = (int64)(cos * 2^50), exact) and summed over the group: integers, any order.
//      D -> Q: lane = document position: a gather of Rmax[id][q], converted and summed the same way.
//    The float scores follow the header to the letter (__fdiv_rn, integer -> float conversions round to nearest even).  Every
//    document's key (score bits << 32 | ~index, 0 when the score is not > 0) goes to LDS; wavefront 0 then takes the
//    workgroup's k largest into its slot, and k_bits_merge (w2b_kernels_evalbits.hip) merges the slots of a query.
//
// Only plain vector loads and stores touch the table.
#include "w2b_eval_bits.hpp"
#include "w2b_eval_codes.hpp"

namespace {

constexpr int kDocsPerBlock = W2B_DOCS_PER_BLOCK;
constexpr int kPadI = -0x7FFFFFFF - 1;       // below every I (|I| <= size < 2^21)
constexpr float kPadF = -2.0f;               // below every cos (|cos| <= 1 + a few ulp)
constexpr int kMaxNW = 16;                   // a column's query row in registers up to 16 halves, in memory beyond

// ---------------------------------------------------------------------------------------------- phase 1: the pair table
// One column's query row (NW > 0: registers, NW == 0: memory) against a uniform vocabulary row.  The columns past `dim` are
// masked here (only the halves of the last 64-column block can hold any) and do not rest on the file's padding bits.
template <int BL, int NW>
struct ColRow {
  uint32_t s[NW > 0 ? NW : 1];
  const uint32_t *p;
  int nw, dim;

  // the columns that exist in half `hw` (0 / 1) of 64-column block `b`
  __device__ __forceinline__ uint32_t valid(int b, int hw) const {
    const int c = dim - 64 * b - 32 * hw;
    return c >= 32 ? ~0u : (c <= 0 ? 0u : (1u << c) - 1u);
  }
  __device__ __forceinline__ void load(const uint32_t *__restrict__ B, int nw_, int dim_, int row) {
    nw = NW > 0 ? NW : nw_;
    dim = dim_;
    p = B + (long long)row * nw;
    if constexpr (NW > 0) {
#pragma unroll
      for (int w = 0; w < NW; w++) s[w] = p[w];
    }
  }
  __device__ __forceinline__ uint32_t word(int w) const {
    if constexpr (NW > 0) return s[w];
    else return p[w];
  }
  // bits: the Hamming distance over the `dim` columns.  codes: J
  __device__ __forceinline__ int product(const uint32_t *__restrict__ row) const {
    int acc = 0;
    if constexpr (BL == 1) {
      auto half = [&](int b, int hw) { acc += __builtin_popcount((word(2 * b + hw) ^ row[2 * b + hw]) & valid(b, hw)); };
      if constexpr (NW > 0) {
#pragma unroll
        for (int b = 0; b < NW / 2; b++) half(b, 0), half(b, 1);
      } else {
        for (int b = 0; b < nw / 2; b++) half(b, 0), half(b, 1);
      }
      return acc;
    } else {
      auto half = [&](int b, int hw) {
        const uint32_t v = valid(b, hw);
        const uint32_t neg = (word(4 * b + hw) ^ row[4 * b + hw]) & v, mx = word(4 * b + 2 + hw) & v, mc = row[4 * b + 2 + hw] & v;
        // sum over the half of |t_x t_c| = 1 + 2 mx + 2 mc + 4 mx mc, and of the same over the columns whose signs differ
        const int all = __builtin_popcount(v) + 2 * __builtin_popcount(mx) + 2 * __builtin_popcount(mc) +
                        4 * __builtin_popcount(mx & mc);
        const int ng = __builtin_popcount(neg) + 2 * __builtin_popcount(neg & mx) + 2 * __builtin_popcount(neg & mc) +
                       4 * __builtin_popcount(neg & mx & mc);
        acc += all - 2 * ng;
      };
      if constexpr (NW > 0) {
#pragma unroll
        for (int b = 0; b < NW / 4; b++) half(b, 0), half(b, 1);
      } else {
        for (int b = 0; b < nw / 4; b++) half(b, 0), half(b, 1);
      }
      return acc;
    }
  }
};

template <int BL, int NW>
__global__ void __launch_bounds__(256)
k_docs_table(const uint32_t *__restrict__ B, int words, int nw, int dim, const float *__restrict__ wrow,
             const int *__restrict__ colrow, int tcols, int rpb, uint32_t *__restrict__ Tab /* [words][tcols] */) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= tcols) return;
  const int qr = colrow[x];
  const int r0 = blockIdx.y * rpb, r1 = min(words, r0 + rpb);
  if (qr < 0) {
    const uint32_t pad = BL == 1 ? (uint32_t)kPadI : __float_as_uint(kPadF);
    for (int r = r0; r < r1; r++) Tab[(size_t)r * tcols + x] = pad;
    return;
  }
  ColRow<BL, NW> cr;
  cr.load(B, nw, dim, qr);
  float wx = 0.f;
  if constexpr (BL == 2) wx = wrow[qr];
  for (int r = r0; r < r1; r++) {
    const int v = cr.product(B + (long long)r * cr.nw);
    uint32_t out;
    if constexpr (BL == 1) out = (uint32_t)(dim - 2 * v);
    else out = __float_as_uint(__fmul_rn(__fmul_rn((float)v, wx), wrow[r]));
    Tab[(size_t)r * tcols + x] = out;
  }
}

// Rmax[c][q] = max over query q's columns that carry an id of Tab[c][x] (the pad value when it has none)
template <int BL>
__global__ void __launch_bounds__(256)
k_docs_rowmax(const uint32_t *__restrict__ Tab, int words, int tcols, int nq, const int *__restrict__ qcol,
              const int *__restrict__ qm, uint32_t *__restrict__ Rmax /* [words][nq] */) {
  const long long n = (long long)words * nq, stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int c = (int)(i / nq), q = (int)(i - (long long)c * nq);
    const uint32_t *t = Tab + (size_t)c * tcols + qcol[q];
    const int m = qm[q];
    if constexpr (BL == 1) {
      int mx = kPadI;
      for (int j = 0; j < m; j++) mx = max(mx, (int)t[j]);
      Rmax[i] = (uint32_t)mx;
    } else {
      float mx = kPadF;
      for (int j = 0; j < m; j++) mx = fmaxf(mx, __uint_as_float(t[j]));
      Rmax[i] = __float_as_uint(mx);
    }
  }
}

// ---------------------------------------------------------------------------------------------- phase 2: the walk
template <int BL> struct DocsT;
template <> struct DocsT<1> {
  using val = int;          // a table value
  using sum = int;          // R: |R| <= 1024 * size < 2^31
  static __device__ __forceinline__ val pad() { return kPadI; }
  static __device__ __forceinline__ val of(uint32_t u) { return (int)u; }
  static __device__ __forceinline__ val vmax(val a, val b) { return max(a, b); }
  static __device__ __forceinline__ sum conv(val v) { return v; }
  // (float)R / (float)(m * size): both conversions round to nearest even, one correctly rounded division
  static __device__ __forceinline__ float score(sum r, int m, int dim) { return __fdiv_rn((float)r, (float)(m * dim)); }
};
template <> struct DocsT<2> {
  using val = float;
  using sum = long long;    // A: 1024 values below 2^51
  static __device__ __forceinline__ val pad() { return kPadF; }
  static __device__ __forceinline__ val of(uint32_t u) { return __uint_as_float(u); }
  static __device__ __forceinline__ val vmax(val a, val b) { return fmaxf(a, b); }
  // F = (int64) ldexp(cos, 50): cos is a multiple of 2^-48 below 2 in magnitude, so the product and the conversion are exact
  static __device__ __forceinline__ sum conv(val v) { return (long long)__fmul_rn(v, 0x1p50f); }
  static __device__ __forceinline__ float score(sum a, int m, int) {
    return __fdiv_rn((float)a, __fmul_rn((float)m, 0x1p50f));       // the divisor is exact
  }
};

template <typename T>
__device__ __forceinline__ T group_sum(T v, int W) {
  for (int d = 1; d < W; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

template <int BL>
__global__ void __launch_bounds__(256)
k_docs_walk(const uint32_t *__restrict__ Tab, const uint32_t *__restrict__ Rmax, int tcols, int nq, int dim,
            const int *__restrict__ qcol, const int *__restrict__ qm, const int *__restrict__ ids /* ids >= 0 only */,
            const long long *__restrict__ off /* [n_docs + 1] into ids */, long long n_docs, int symmetric, int k,
            unsigned long long *__restrict__ slots /* [nq][gridDim.x][k] */, float *__restrict__ all /* [nq][n_docs] or null */) {
  using D = DocsT<BL>;
  __shared__ unsigned long long keys[kDocsPerBlock];
  const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long d0 = (long long)blockIdx.x * kDocsPerBlock;
  const int nd = (int)min((long long)kDocsPerBlock, n_docs - d0);
  const int c0 = qcol[q], width = qcol[q + 1] - c0, m = qm[q];
  for (int i = tid; i < kDocsPerBlock; i += 256) keys[i] = 0ull;
  __syncthreads();
  const int W = width <= 16 ? 16 : (width <= 32 ? 32 : 64), G = 64 / W, g = lane / W, x = lane & (W - 1);
  const int ntiles = (width + 63) / 64, per_pass = 4 * G;
  const uint32_t *tq = Tab + c0;
  for (int i0 = 0; i0 < nd; i0 += per_pass) {          // (uniform over the wavefront: the group sums are shuffles)
    const int i = i0 + wave * G + g;
    const bool live = i < nd && m > 0;
    const long long b = live ? off[d0 + i] : 0;
    const int len = live ? (int)(off[d0 + i + 1] - b) : 0;
    const int *di = ids + b;
    // Q -> D: the running maximum of this lane's column over the document's positions, tile by tile
    typename D::sum sq = 0;
    for (int t = 0; t < ntiles; t++) {
      const int col = 64 * t + x;
      if (col < width && len > 0) {
        const uint32_t *tc = tq + col;
        typename D::val mx = D::pad();
        for (int p = 0; p < len; p += 4) {
          // (a position past the end repeats the first one of the four: a maximum does not mind)
          const int id0 = di[p], id1 = p + 1 < len ? di[p + 1] : id0, id2 = p + 2 < len ? di[p + 2] : id0,
                    id3 = p + 3 < len ? di[p + 3] : id0;
          const typename D::val v0 = D::of(tc[(size_t)id0 * tcols]), v1 = D::of(tc[(size_t)id1 * tcols]),
                                v2 = D::of(tc[(size_t)id2 * tcols]), v3 = D::of(tc[(size_t)id3 * tcols]);
          mx = D::vmax(mx, D::vmax(D::vmax(v0, v1), D::vmax(v2, v3)));
        }
        if (col < m) sq += D::conv(mx);
      }
    }
    sq = group_sum(sq, W);
    // D -> Q: lane = document position
    typename D::sum sd = 0;
    if (symmetric) {
      for (int p = x; p < len; p += W) sd += D::conv(D::of(Rmax[(size_t)di[p] * nq + q]));
      sd = group_sum(sd, W);
    }
    if (x == 0 && i < nd) {
      float sc = 0.f;
      if (live && len > 0) {
        sc = D::score(sq, m, dim);
        if (symmetric) {
          const float s2 = D::score(sd, len, dim);
          sc = s2 < sc ? s2 : sc;
        }
      }
      keys[i] = sc > 0.f ? codes_key(sc, (int)(d0 + i)) : 0ull;
      if (all) all[(size_t)q * (size_t)n_docs + (size_t)(d0 + i)] = sc;
    }
  }
  __syncthreads();
  if (wave != 0) return;
  // the workgroup's k largest keys, best first; keys are distinct (~index), so exactly one lane owns each winner
  unsigned long long *out = slots + ((long long)q * gridDim.x + blockIdx.x) * k;
  unsigned long long prev = ~0ull;
  for (int j = 0; j < k; j++) {
    unsigned long long best = 0ull;
    if (prev) {
      for (int i = lane; i < kDocsPerBlock; i += 64) {
        const unsigned long long v = keys[i];
        best = (v < prev && v > best) ? v : best;
      }
#pragma unroll
      for (int d = 32; d; d >>= 1) {
        const unsigned long long o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
      }
    }
    if (lane == 0) out[j] = best;
    prev = best;
  }
}

}  // namespace

hipError_t w2b_launch_docs_table(const uint32_t *B, int words, int dim, int bitlevel, const float *wrow, const int *colrow,
                                 int tcols, const int *qcol, const int *qm, int nq, void *Tab, void *Rmax, hipStream_t s) {
  if (words <= 0 || nq <= 0) return hipSuccess;
  const int nw = (dim + 63) / 64 * 2 * bitlevel;
  if (tcols > 0) {
    const int xb = (tcols + 255) / 256;
    int splits = 2048 / xb;
    if (splits > (words + 63) / 64) splits = (words + 63) / 64;
    if (splits < 1) splits = 1;
    const int rpb = (words + splits - 1) / splits;
    const dim3 grid((unsigned)xb, (unsigned)((words + rpb - 1) / rpb));
    const hipError_t e = dispatch_nw<kMaxNW>(nw, [&](auto n) {
      constexpr int NW = decltype(n)::value;
      if (bitlevel == 1) {
        hipLaunchKernelGGL((k_docs_table<1, NW>), grid, dim3(256), 0, s, B, words, nw, dim, wrow, colrow, tcols, rpb, (uint32_t *)Tab);
      } else if constexpr (NW % 4 == 0) {
        hipLaunchKernelGGL((k_docs_table<2, NW>), grid, dim3(256), 0, s, B, words, nw, dim, wrow, colrow, tcols, rpb, (uint32_t *)Tab);
      }
      return hipGetLastError();
    });
    if (e != hipSuccess) return e;
  }
  const long long n = (long long)words * nq;
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  if (bitlevel == 1)
    hipLaunchKernelGGL((k_docs_rowmax<1>), dim3(blocks), dim3(256), 0, s, (const uint32_t *)Tab, words, tcols, nq, qcol, qm, (uint32_t *)Rmax);
  else
    hipLaunchKernelGGL((k_docs_rowmax<2>), dim3(blocks), dim3(256), 0, s, (const uint32_t *)Tab, words, tcols, nq, qcol, qm, (uint32_t *)Rmax);
  return hipGetLastError();
}

hipError_t w2b_launch_docs_walk(const void *Tab, const void *Rmax, int tcols, int nq, int dim, int bitlevel, const int *qcol,
                                const int *qm, const int *ids, const long long *off, long long n_docs, int symmetric, int k,
                                unsigned long long *slots, unsigned long long *out, float *all_scores, hipStream_t s) {
  if (nq <= 0 || n_docs <= 0) return hipSuccess;
  const long long splits = (n_docs + kDocsPerBlock - 1) / kDocsPerBlock;
  const dim3 grid((unsigned)splits, (unsigned)nq);
  if (bitlevel == 1)
    hipLaunchKernelGGL((k_docs_walk<1>), grid, dim3(256), 0, s, (const uint32_t *)Tab, (const uint32_t *)Rmax, tcols, nq, dim, qcol, qm,
                       ids, off, n_docs, symmetric, k, slots, all_scores);
  else
    hipLaunchKernelGGL((k_docs_walk<2>), grid, dim3(256), 0, s, (const uint32_t *)Tab, (const uint32_t *)Rmax, tcols, nq, dim, qcol, qm,
                       ids, off, n_docs, symmetric, k, slots, all_scores);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return w2b_launch_bits_merge(slots, (int)(splits * k), k, nq, out, s);
}
