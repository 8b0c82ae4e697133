// w2b_kernels_evalbag.hip -- the evaluator's bag question on bit-packed rows (include/word2bits_eval.h, "bag questions").
//
// A question is the unnormalised integer sum T[a] = sum of t_r[a] over a bag of up to 4096 rows (t = +-1 on 1-bit rows,
// +-1 / +-3 on 2-bit rows), so it is ONE integer vector and the scan needs one logical accumulator per (question, row):
//   J(c) = sum_a T[a] * t_c[a],  exact,  |J| <= 9 * 4096 * D < 2^31.
// |T[a]| <= 12288 does not fit an int8 operand, so T goes as two balanced base-256 digits,
//   lo = ((T + 128) mod 256) - 128 in [-128, 127],   hi = (T - lo) / 256 in [-48, 48],
// two accumulator tiles per (question, row) on v_mfma_i32_32x32x32_i8, and J = 256 * J_hi + J_lo in the lane that holds
// both.  Everything else is the shape of k_codes_scan (w2b_kernels_evalcodes.hip): the vocabulary rows are the A operand,
// unpacked once into registers by the wavefront that owns them (2 x 32 rows up to 416 columns, 1 x 32 up to 1216, chunks
// of 38 K steps beyond), the question operands lie in memory in fragment order -- one K step of a 32-question tile is
// 2 x 64 x 16 bytes, two coalesced 16-byte loads per lane, requested one step ahead -- with ZEROS in columns >= D (the
// padding bits of a packed row decode to +1) and one zero step behind the last tile for the last prefetch; the K loop has
// no branch; a lane owns one question; the selection is that of w2b_eval_select.hpp with a 32-row tile as the unit,
// followed by the fp32 scan's merge kernel.
// The key is (score bits << 32 | ~row) in both modes.  1-bit rows: the score bits are (uint32)J for J > 0, which order like
// the float (float)J / (float)D that the host prints.  2-bit rows: the bits of the float ((float)J * wq) * w(c), both
// products rounded on their own, wq = 1 / sqrt(sum_a T[a]^2) built on the host from the integer that k_bag_operands sums.
// The rows of the bag are excluded on the candidate path alone: a score that would enter the list looks its row up in the
// question's sorted list by binary search; the main loop never sees the list.
#include "w2b_internal.h"
#include "w2b_eval_select.hpp"
#include "w2b_eval_codes.hpp"

#include <type_traits>

namespace {

constexpr int BAG_G = 16;      // 16-column groups of one question that a workgroup of k_bag_operands pools
constexpr int BAG_P = 16;      // parts that a bag's ids are dealt to

// columns 32 s + 16 h .. + 15 of a packed row as int8: BL = 1 one sign bit per column (nw = 2 ceil(D / 64) halves per row),
// BL = 2 sign and magnitude (nw = 4 ceil(D / 64))
template <int BL>
__device__ __forceinline__ i32x4 bag_row_frag(const uint32_t *__restrict__ B, long long row, int nw, int s, int h, uint32_t vb) {
  if constexpr (BL == 2) return codes_row_frag(B, row, nw, s, h, vb);
  return codes_unpack16((B[row * nw + s] >> (16 * h)) & 0xFFFFu, 0u, vb);
}

// The question operands in fragment order, T[((qt * ks + s) * 2 + digit) * 64 + lane]: question qt * 32 + lane % 32, columns
// 32 s + 16 (lane / 32) .. + 15 of the pooled vector's digit plane (0 = lo, 1 = hi).  The caller has zeroed T, so columns
// and questions that do not exist and the trailing step stay zero.  One workgroup = one question x BAG_G column groups; its
// ids are dealt to BAG_P parts (integer adds commute).  BL = 2: NT[q] += sum of T[a]^2 over the workgroup's columns.
// ids < 0 are padding; every other id has been validated by the host.
template <int BL>
__global__ void __launch_bounds__(BAG_G *BAG_P)
k_bag_operands(const uint32_t *__restrict__ B, int nw, int dim, int ks, int gtiles, const int *__restrict__ ids,
               const int *__restrict__ off, i32x4 *__restrict__ T, unsigned long long *__restrict__ NT) {
  __shared__ int part[BAG_P][BAG_G][16];
  __shared__ int tot[BAG_G][16];
  const int q = (int)(blockIdx.x / (unsigned)gtiles), g0 = (int)(blockIdx.x % (unsigned)gtiles) * BAG_G;
  const int tid = threadIdx.x, pt = tid / BAG_G, gl = tid % BAG_G, g = g0 + gl;
  const int s = g >> 1, h = g & 1, cols = dim - 16 * g;
  const uint32_t vb = cols >= 16 ? 0xFFFFu : (cols <= 0 ? 0u : (1u << cols) - 1u);
  int acc[16];
#pragma unroll
  for (int j = 0; j < 16; j++) acc[j] = 0;
  if (s < ks) {
    const int lo = off[q], hi = off[q + 1];
    for (int i = lo + pt; i < hi; i += BAG_P) {
      const int row = ids[i];
      if (row < 0) continue;
      const i32x4 o = bag_row_frag<BL>(B, row, nw, s, h, vb);
#pragma unroll
      for (int j = 0; j < 16; j++) acc[j] += (int)(signed char)((unsigned)o[j >> 2] >> (8 * (j & 3)));
    }
  }
#pragma unroll
  for (int j = 0; j < 16; j++) part[pt][gl][j] = acc[j];
  __syncthreads();
  // thread = (group tid / 16, column tid % 16) of the workgroup's 256 columns
  int t = 0;
#pragma unroll
  for (int p = 0; p < BAG_P; p++) t += (&part[p][0][0])[tid];
  (&tot[0][0])[tid] = t;
  if constexpr (BL == 2) {
    unsigned long long n = (unsigned long long)((long long)t * t);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    if ((tid & 63) == 0 && n) atomicAdd(&NT[q], n);
  }
  __syncthreads();
  if (tid < BAG_G && (g0 + tid) < 2 * ks) {
    const int gg = g0 + tid;
    i32x4 lo4 = {0, 0, 0, 0}, hi4 = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int v = tot[tid][j];
      const int l = ((v + 128) & 255) - 128, u = (v - l) >> 8;            // v - l is a multiple of 256
      lo4[j >> 2] |= (int)(((unsigned)l & 255u) << (8 * (j & 3)));
      hi4[j >> 2] |= (int)(((unsigned)u & 255u) << (8 * (j & 3)));
    }
    const long long at = (((long long)(q >> 5) * ks + (gg >> 1)) * 2) * 64 + (gg & 1) * 32 + (q & 31);
    T[at] = lo4;
    T[at + 64] = hi4;
  }
}

// is row c one of the question's own rows?  x[0 .. n) ascending
__device__ __forceinline__ bool bag_owns(const int *__restrict__ x, int n, int c) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (x[mid] < c) lo = mid + 1; else hi = mid;
  }
  return lo < n && x[lo] == c;
}

// xrows / xoff: every question's own rows, ascending and without repeats, and their bounds [nq + 1]; xoff == nullptr: nothing
// is excluded.  Wq (BL = 2): the questions' weights [32 * qtiles], 0 for a question whose vector is zero.
template <int BL, int KS, int R, bool CHUNKED>
__global__ void __launch_bounds__(CT, 1)
k_bag_scan(const uint32_t *__restrict__ B, int nw, int words, const float *__restrict__ wrow, const i32x4 *__restrict__ T,
           const float *__restrict__ Wq, int ks, int nq, int qtiles, int qt_per_y, const int *__restrict__ xrows,
           const int *__restrict__ xoff, unsigned long long *__restrict__ best, const TopkArgs tk) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l32 = lane & 31, h = lane >> 5;
  const int tile0 = ((int)blockIdx.x * 4 + wave) * R, r0 = tile0 * CROWS;
  const int qt0 = (int)blockIdx.y * qt_per_y, qt1 = min(qtiles, qt0 + qt_per_y);
  if (r0 >= words || qt0 >= qt1) return;          // (no barrier in this kernel)

  i32x4 a[R][KS];
  auto unpack_chunk = [&](int c0) {
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int row = r0 + r * CROWS + l32;
#pragma unroll
      for (int s = 0; s < KS; s++) {
        a[r][s] = i32x4{0, 0, 0, 0};
        if (row < words && c0 + s < ks) a[r][s] = bag_row_frag<BL>(B, row, nw, c0 + s, h, 0xFFFFu);
      }
    }
  };
  if (!CHUNKED) unpack_chunk(0);

  const i32x4 *p = T + (long long)qt0 * ks * 128 + lane;
  i32x4 bq[2] = {p[0], p[64]};
  for (int qt = qt0; qt < qt1; qt++) {
    const int q = qt * 32 + l32;
    const bool live = q < nq;
    const unsigned long long seen = live ? ld_key(&best[q]) : ~0ull;     // possibly stale: then it is only lower

    i32x16 acc[2][R];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int r = 0; r < R; r++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[t][r][e] = 0;

    for (int c0 = 0; c0 < ks; c0 += KS) {           // one pass unless CHUNKED
      if (CHUNKED) unpack_chunk(c0);
#pragma unroll
      for (int s = 0; s < KS; s++) {
        // free of branches: a step past the row's last one multiplies by the zero operands that unpack_chunk left there
        // and requests the same (next) step again
        p += c0 + s < ks ? 128 : 0;               // the next step of this stream (after the launch's last one: zeros)
        const i32x4 n0 = p[0], n1 = p[64];
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
          for (int t = 0; t < 2; t++)
            acc[t][r] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[r][s], bq[t], acc[t][r], 0, 0, 0);
        bq[0] = n0;
        bq[1] = n1;
      }
    }

    // Accumulator e of tile r in lane l: row r0 + 32 r + 8 (e / 4) + 4 (l / 32) + e % 4, question l % 32.
    // u = the score bits of the key, 0 where the row is no answer (score <= 0)
    unsigned u[R][16];
    unsigned mr[R];
    float wq = 0.f;
    if constexpr (BL == 2) wq = Wq[q];
#pragma unroll
    for (int r = 0; r < R; r++) {
      mr[r] = 0u;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        cf32x4 wc = {0.f, 0.f, 0.f, 0.f};
        if constexpr (BL == 2) wc = *(const cf32x4 *)(wrow + r0 + r * CROWS + 8 * g + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int e = 4 * g + i;
          const int J = 256 * acc[1][r][e] + acc[0][r][e];
          if constexpr (BL == 2) {
            const float d = __fmul_rn(__fmul_rn((float)J, wq), wc[i]);
            u[r][e] = d > 0.f ? __float_as_uint(d) : 0u;
          } else {
            u[r][e] = J > 0 ? (unsigned)J : 0u;
          }
          mr[r] = u[r][e] > mr[r] ? u[r][e] : mr[r];
        }
      }
    }
    auto row_of = [&](int r, int e, int hh) { return r0 + r * CROWS + 8 * (e >> 2) + 4 * hh + (e & 3); };
    auto key_of = [&](unsigned bits, int c) {
      return ((unsigned long long)bits << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)c);
    };
    const int x0 = (live && xoff) ? xoff[q] : 0, xn = (live && xoff) ? xoff[q + 1] - x0 : 0;

    // unit = one 32-row tile, whose scores for a question sit in the lane pair (l, l ^ 32); `seen` is the bound
#pragma unroll
    for (int r = 0; r < R; r++) {
      const bool may = live && mr[r] > 0u && mr[r] >= (unsigned)(seen >> 32);
      if (!__any(may)) continue;
      unsigned cm = 0u;
      unsigned long long mx = 0ull;
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int c = row_of(r, e, h);
        const unsigned long long k2 = key_of(u[r][e], c);
        bool ok = may && c < words && u[r][e] > 0u && k2 > seen;
        if (ok && xn > 0) ok = !bag_owns(xrows + x0, xn, c);
        cm |= ok ? 1u << e : 0u;
        mx = (ok && k2 > mx) ? k2 : mx;
      }
      if (!__any(cm != 0u)) continue;
      const int n_me = __builtin_popcount(cm), n_ot = __shfl_xor(n_me, 32, 64), totc = n_me + n_ot;
      const unsigned long long om = __shfl_xor(mx, 32, 64), pm = mx > om ? mx : om;   // the pair's largest candidate
      const int unit = tile0 + r;
      unsigned long long *slot = tk.keys + ((long long)q * tk.nunits + unit) * tk.cap;   // (used by lanes with candidates only)
      unsigned long long kth = 0ull;
      if (__any(totc > tk.cap)) {
        // more candidates than the slot holds (k < 32 only): a key's place is its rank in the pair, the first cap stay
        const unsigned cmo = __shfl_xor(cm, 32, 64);
        unsigned uq[16];
#pragma unroll
        for (int e = 0; e < 16; e++) uq[e] = __shfl_xor(u[r][e], 32, 64);
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const unsigned long long mine = key_of(u[r][e], row_of(r, e, h));
          int rank = 0;
#pragma unroll
          for (int x = 0; x < 16; x++) {
            const unsigned long long ka = (cm >> x) & 1u ? key_of(u[r][x], row_of(r, x, h)) : 0ull;
            const unsigned long long kb = (cmo >> x) & 1u ? key_of(uq[x], row_of(r, x, h ^ 1)) : 0ull;
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
          if ((cm >> e) & 1u) slot[pos++] = key_of(u[r][e], row_of(r, e, h));
      }
      if (h == 0 && pm) {
        tk.cnt[(long long)q * tk.nunits + unit] = (unsigned char)(totc < tk.cap ? totc : tk.cap);
        if (kth && tk.cap == tk.k) atomicMax(&best[q], kth);
        topk_note_max(tk.bkt, tk.k, best, q, unit, pm);
      }
    }
  }
}

// the kernel instance for ks K steps: {register-resident steps, row tiles per wavefront, chunked} -- the regimes of k_codes_scan
template <typename F>
hipError_t bag_dispatch_ks(int ks, F &&f) {
#define W2B_KS(n, r) if (ks <= n) return f(std::integral_constant<int, n>(), std::integral_constant<int, r>(), std::false_type());
  W2B_KS(1, 2) W2B_KS(2, 2) W2B_KS(4, 2) W2B_KS(7, 2) W2B_KS(10, 2) W2B_KS(13, 2)
  W2B_KS(16, 1) W2B_KS(20, 1) W2B_KS(26, 1) W2B_KS(32, 1) W2B_KS(W2B_CODES_KS_MAX, 1)
#undef W2B_KS
  return f(std::integral_constant<int, W2B_CODES_KS_MAX>(), std::integral_constant<int, 1>(), std::true_type());
}

template <int BL>
hipError_t bag_scan(const uint32_t *B, int words, int dim, const float *wrow, const void *T, const float *Wq, int nq,
                    const int *xrows, const int *xoff, unsigned long long *bound, const TopkArgs &tk, hipStream_t s) {
  const int ks = (dim + 31) / 32, nw = (dim + 63) / 64 * 2 * BL, qtiles = (nq + 31) / 32;
  return bag_dispatch_ks(ks, [&](auto ksmax, auto tiles, auto chunked) {
    constexpr int KS = decltype(ksmax)::value, R = decltype(tiles)::value;
    constexpr bool CH = decltype(chunked)::value;
    // row groups x ranges of question tiles, as w2b_launch_codes_scan sizes them
    const int gx = (words + 4 * R * CROWS - 1) / (4 * R * CROWS);
    int gy = (1024 + gx - 1) / gx;
    if (gy > qtiles) gy = qtiles;
    const int per_y = (qtiles + gy - 1) / gy;
    gy = (qtiles + per_y - 1) / per_y;
    hipLaunchKernelGGL((k_bag_scan<BL, KS, R, CH>), dim3((unsigned)gx, (unsigned)gy), dim3(CT), 0, s, B, nw, words, wrow,
                       (const i32x4 *)T, Wq, ks, nq, qtiles, per_y, xrows, xoff, bound, tk);
    return hipGetLastError();
  });
}

}  // namespace

size_t w2b_bag_operand_bytes(int dim, long long nq) {
  const long long ks = (dim + 31) / 32, qtiles = (nq + 31) / 32;
  return (size_t)(qtiles * ks * 128 + 128) * 16;
}

hipError_t w2b_launch_bag_operands(const uint32_t *B, int dim, int bitlevel, int nq, const int *ids, const int *off, void *T,
                                   unsigned long long *NT, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  const int ks = (dim + 31) / 32, nw = (dim + 63) / 64 * 2 * bitlevel, gtiles = (2 * ks + BAG_G - 1) / BAG_G;
  const dim3 grid((unsigned)((long long)nq * gtiles)), block(BAG_G * BAG_P);
  if (bitlevel == 2)
    hipLaunchKernelGGL(k_bag_operands<2>, grid, block, 0, s, B, nw, dim, ks, gtiles, ids, off, (i32x4 *)T, NT);
  else
    hipLaunchKernelGGL(k_bag_operands<1>, grid, block, 0, s, B, nw, dim, ks, gtiles, ids, off, (i32x4 *)T, NT);
  return hipGetLastError();
}

hipError_t w2b_launch_bag_scan(const uint32_t *B, int words, int dim, int bitlevel, const float *wrow, const void *T,
                               const float *Wq, int nq, const int *xrows, const int *xoff, int k, unsigned long long *bound,
                               unsigned long long *bkt, unsigned long long *keys, unsigned char *cnt, unsigned long long *out,
                               hipStream_t s) {
  if (nq <= 0 || words <= 0) return hipSuccess;
  TopkArgs tk{};
  tk.keys = keys;
  tk.cnt = cnt;
  tk.bkt = bkt;
  tk.k = k;
  w2b_codes_topk_layout(words, dim, k, &tk.nunits, &tk.cap);
  const hipError_t e = bitlevel == 2 ? bag_scan<2>(B, words, dim, wrow, T, Wq, nq, xrows, xoff, bound, tk, s)
                                     : bag_scan<1>(B, words, dim, wrow, T, Wq, nq, xrows, xoff, bound, tk, s);
  if (e != hipSuccess) return e;
  return w2b_launch_eval_topk_merge(keys, cnt, tk.nunits, tk.cap, k, nq, out, s);
}
