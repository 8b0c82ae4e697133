// w2b_kernels_evalcodes.hip -- the evaluator's scan on bit-packed 2-bit rows (include/word2bits_eval.h, "codes" mode).
//
// A 2-bit row is D values t/4, t in {-1, +1, -3, +3}, stored as the file stores them: per 64 columns one 64-bit word of
// SIGN bits (set = negative) and one of MAGNITUDE bits (set = 3), padding bits zero (include/word2bits_corpus.h).  Here
// a row is 4 * ceil(D / 64) 32-bit halves: per block sign lo, sign hi, magnitude lo, magnitude hi.  For a question
// (b1, b2, b3) and a row c the three integers J(b_i, c) = sum_a t_bi[a] * t_c[a] are exact on the i8 matrix cores, and
//   score = ((J2 * w(b2) - J1 * w(b1)) + J3 * w(b3)) * w(c),   w(r) = 1 / sqrt(D + 8 * n3(r))
// in float32, every operation rounded on its own (__fmul_rn / __fsub_rn / __fadd_rn; the header states the sequence).
//
// Shape: v_mfma_i32_32x32x32_i8 with the vocabulary rows as the A operand and the questions as B, so that a lane owns ONE
// question (column lane % 32) and 16 rows per 32 x 32 tile, and the three terms of a question are three accumulator
// tiles over the same positions: J1, J2, J3 of a (question, row) pair sit in the same lane and register, the combine is
// lane-local, and so is most of the arg-max (one exchange with lane ^ 32 finishes it).
// The ROWS stay in registers: a wavefront unpacks its R x 32 rows once -- sign and magnitude bits to int8 with a few
// integer operations per four columns, no table -- into R * KS operand quads (KS = ceil(D / 32) K steps; D <= 416: R = 2,
// 104 registers; D <= 1216: R = 1, 152 registers) and then walks the question tiles, whose operands k_codes_operands has
// laid out in fragment order: one K step of a 32-question tile is 3 x 64 x 16 bytes, read as three coalesced 16-byte
// loads per lane, the next step requested before the current step's 3 R MFMAs.  No int8 or float copy of the matrix
// exists in memory; per row the device keeps w(c) (4 bytes).  Rows longer than 1216 columns walk K in chunks of 38 steps
// and unpack each chunk again for every question tile (slow, exact, any D).
// Columns >= D: the padding bits of a packed row decode to t = +1, so the QUESTION operands carry zeros there.  Rows past
// the vocabulary are zero operands with w = 0.
// The grid is (row groups of 4 wavefronts) x (ranges of question tiles); a question's partial results meet in the
// 64-bit atomic max on (score bits << 32 | ~row) (top-1), or in the slots, bound and buckets of the fp32 scan's top-k
// selection (w2b_eval_select.hpp; unit = a wavefront's 32-row tile) followed by its merge kernel.
#include "w2b_internal.h"
#include "w2b_eval_select.hpp"
#include "w2b_eval_codes.hpp"

#include <type_traits>

namespace {

// w(c) of every row from its magnitude bits; rows past the vocabulary get 0
__global__ void k_codes_roww(const uint32_t *__restrict__ B, int nw, int dim, long long words, long long rows_padded,
                             const float *__restrict__ wtab, float *__restrict__ wrow) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows_padded) return;
  if (r >= words) {
    wrow[r] = 0.f;
    return;
  }
  const uint32_t *p = B + r * nw;
  int n3 = 0;
  for (int b = 0; 4 * b < nw; b++) {
    const int cols = dim - 64 * b;                                    // >= 1
    const uint32_t lo = cols >= 32 ? ~0u : (1u << cols) - 1u;
    const uint32_t hi = cols >= 64 ? ~0u : (cols <= 32 ? 0u : (1u << (cols - 32)) - 1u);
    n3 += __builtin_popcount(p[4 * b + 2] & lo) + __builtin_popcount(p[4 * b + 3] & hi);
  }
  wrow[r] = wtab[n3];
}

// The question operands in fragment order, T[((qt * ks + s) * 3 + term) * 64 + lane]: question qt * 32 + lane % 32,
// columns 32 s + 16 (lane / 32) .. + 15 of row b_term, zeros where the column or the question does not exist; one more
// (zero) step at the end, which the scan's last prefetch reads.  Wq[term][qtiles * 32] = w(b_term).
__global__ void k_codes_operands(const uint32_t *__restrict__ B, int nw, int dim, int ks, int nq, int qtiles,
                                 const float *__restrict__ wrow, const int *__restrict__ b1, const int *__restrict__ b2,
                                 const int *__restrict__ b3, i32x4 *__restrict__ T, float *__restrict__ Wq) {
  const long long n = (long long)qtiles * ks * 192, stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = i0; i < n + 192; i += stride) {
    i32x4 o = {0, 0, 0, 0};
    if (i < n) {
      const int lane = (int)(i & 63), t = (int)((i >> 6) % 3), s = (int)((i / 192) % ks), qt = (int)(i / (192ll * ks));
      const int q = qt * 32 + (lane & 31), h = lane >> 5;
      if (q < nq) {
        const int row = t == 0 ? b1[q] : (t == 1 ? b2[q] : b3[q]);
        const int cols = dim - (32 * s + 16 * h);
        const uint32_t vb = cols >= 16 ? 0xFFFFu : (cols <= 0 ? 0u : (1u << cols) - 1u);
        o = codes_row_frag(B, row, nw, s, h, vb);
      }
    }
    T[i] = o;
  }
  const int nqp = qtiles * 32;
  for (long long i = i0; i < 3ll * nqp; i += stride) {
    const int t = (int)(i / nqp), q = (int)(i - (long long)t * nqp);
    Wq[i] = q < nq ? wrow[t == 0 ? b1[q] : (t == 1 ? b2[q] : b3[q])] : 0.f;
  }
}

// COSMUL: the 3CosMul question (include/word2bits_eval.h): the same three accumulator tiles, combined as
//   cos_i = (J_i * w(b_i)) * w(c),  u_i = (1 + cos_i) * 0.5,  score = (u2 * u3) / (u1 + eps)
// one rounding per operation.  The scores are positive floats, so the key, the `seen` pruning and the selection stay as
// they are.  (A lane without a question and a row past the vocabulary have w = 0: cos = 0, a finite score that is dropped
// like every other one of theirs.)
constexpr float kCosmulEps = 1e-6f;    // 0x358637BD

// RANK: the place of a given row (include/word2bits_eval.h, "rank of a given row"): the same three accumulator tiles and
// the same float, compared with the question's target score and row instead of selected.  A lane counts the rows that
// stand before the target and the rows with exactly its score in two registers over the workgroup's rows of one question
// tile and adds them to the question's 64-bit counter once (low half: before, high half: equal).  Per score that is one
// compare and one add (score >= target's); which of those tie with the target, and from which side, is worked out again
// from the accumulators in the few tiles where a tie was seen.  Nothing is excluded
// here: the question's own rows and the target itself are counted like any row, and k_codes_rank_targets has put what
// they add into `corr`.  A row past the vocabulary scores 0 and a ranked target's score is > 0, so padding counts nothing.
struct RankArgs {
  const int *target;              // [nq]
  const float *tscore;            // [nq] the target's score, 0 = the target has no rank
  unsigned long long *cnt;        // [nq], zeroed
};

template <int KS, int R, bool CHUNKED, bool TOPK, bool COSMUL = false, bool RANK = false>
__global__ void __launch_bounds__(CT, 1)
k_codes_scan(const uint32_t *__restrict__ B, int nw, int words, const float *__restrict__ wrow, const i32x4 *__restrict__ T,
             const float *__restrict__ Wq, int ks, int nq, int qtiles, int qt_per_y, const int *__restrict__ b1,
             const int *__restrict__ b2, const int *__restrict__ b3, unsigned long long *__restrict__ best, const TopkArgs tk,
             const RankArgs rk) {
  static_assert(!RANK || (!TOPK && !COSMUL), "the rank epilogue belongs to the additive top-1 shape");
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
        if (row < words && c0 + s < ks) a[r][s] = codes_row_frag(B, row, nw, c0 + s, h, 0xFFFFu);
      }
    }
  };
  if (!CHUNKED) unpack_chunk(0);

  const int nqp = qtiles * 32;
  const i32x4 *p = T + (long long)qt0 * ks * 192 + lane;
  i32x4 bq[3] = {p[0], p[64], p[128]};
  for (int qt = qt0; qt < qt1; qt++) {
    const int q = qt * 32 + l32;
    const bool live = q < nq;
    const float w1 = Wq[q], w2 = Wq[nqp + q], w3 = Wq[2 * nqp + q];
    int e1 = -1, e2 = -1, e3 = -1, tg = 0;
    unsigned long long seen = ~0ull;
    float ts = 0.f;
    if constexpr (RANK) {
      ts = live ? rk.tscore[q] : 0.f;
      tg = live ? rk.target[q] : 0;
    } else {
      e1 = live ? b1[q] : -1, e2 = live ? b2[q] : -1, e3 = live ? b3[q] : -1;
      seen = live ? ld_key(&best[q]) : ~0ull;     // possibly stale: then it is only lower
    }

    i32x16 acc[3][R];
#pragma unroll
    for (int t = 0; t < 3; t++)
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
        p += c0 + s < ks ? 192 : 0;               // the next step of this stream (after the launch's last one: zeros)
        const i32x4 n0 = p[0], n1 = p[64], n2 = p[128];
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
          for (int t = 0; t < 3; t++)
            acc[t][r] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[r][s], bq[t], acc[t][r], 0, 0, 0);
        bq[0] = n0;
        bq[1] = n1;
        bq[2] = n2;
      }
    }

    // Accumulator e of tile r in lane l: row r0 + 32 r + 8 (e / 4) + 4 (l / 32) + e % 4, question l % 32.
    auto row_of = [&](int r, int e, int hh) { return r0 + r * CROWS + 8 * (e >> 2) + 4 * hh + (e & 3); };
    float d[R][16];
    float mr[R];
    unsigned before = 0, equal = 0;                 // RANK: this lane's two counts of the question tile
    bool tie = false;                               // RANK: one of this lane's rows has exactly the target's score
#pragma unroll
    for (int r = 0; r < R; r++) {
      mr[r] = 0.f;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const cf32x4 wc = *(const cf32x4 *)(wrow + r0 + r * CROWS + 8 * g + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int e = 4 * g + i;
          const float p1 = codes_term(acc[0][r][e], w1), p2 = codes_term(acc[1][r][e], w2), p3 = codes_term(acc[2][r][e], w3);
          if constexpr (COSMUL) {
            const float u1 = __fmul_rn(__fadd_rn(1.0f, __fmul_rn(p1, wc[i])), 0.5f),
                        u2 = __fmul_rn(__fadd_rn(1.0f, __fmul_rn(p2, wc[i])), 0.5f),
                        u3 = __fmul_rn(__fadd_rn(1.0f, __fmul_rn(p3, wc[i])), 0.5f);
            d[r][e] = __fdiv_rn(__fmul_rn(u2, u3), __fadd_rn(u1, kCosmulEps));
          } else {
            d[r][e] = codes_add_score(p1, p2, p3, wc[i]);
          }
          if constexpr (RANK) {                     // counted as it is made: no score outlives its step
            before += d[r][e] >= ts ? 1u : 0u;      // (the rows that tie with the target are sorted out below)
            tie |= d[r][e] == ts;
          } else {
            mr[r] = __builtin_fmaxf(mr[r], d[r][e]);
          }
        }
      }
    }

    if constexpr (RANK) {
      if (!__any(ts > 0.f)) continue;
      if (__any(tie && ts > 0.f)) {
        // Rare: the tile that holds the target itself, and rows identical to it.  The scores again, from the accumulators:
        // a row with the target's score counts as equal, and stands before the target only from a lower row.
#pragma unroll
        for (int r = 0; r < R; r++) {
          const int trel = tg - (r0 + r * CROWS + 4 * h);      // the target's row relative to this lane's first row of the tile
#pragma unroll
          for (int g = 0; g < 4; g++) {
            const cf32x4 wc = *(const cf32x4 *)(wrow + r0 + r * CROWS + 8 * g + 4 * h);
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const int e = 4 * g + i;
              const float dd = codes_add_score(codes_term(acc[0][r][e], w1), codes_term(acc[1][r][e], w2),
                                               codes_term(acc[2][r][e], w3), wc[i]);
              equal += dd == ts ? 1u : 0u;
              before -= (dd == ts && 8 * g + i >= trel) ? 1u : 0u;   // row_of(r, e, h) >= tg
            }
          }
        }
      }
      before += __shfl_xor(before, 32, 64);
      equal += __shfl_xor(equal, 32, 64);
      if (h == 0 && ts > 0.f && (before | equal) != 0u) atomicAdd(&rk.cnt[q], ((unsigned long long)equal << 32) | before);
    } else if constexpr (!TOPK) {
      // can any of this wavefront's scores still improve its question's key?  (equal scores: a lower row may)
      float m = mr[0];
#pragma unroll
      for (int r = 1; r < R; r++) m = __builtin_fmaxf(m, mr[r]);
      const bool may = live && m > 0.f && __float_as_uint(m) >= (unsigned)(seen >> 32);
      if (!__any(may)) continue;
      unsigned long long key = 0ull;
#pragma unroll
      for (int r = 0; r < R; r++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const int c = row_of(r, e, h);
          const float dd = d[r][e];
          if (may && c < words && c != e1 && c != e2 && c != e3 && dd > 0.f) {
            const unsigned long long k2 = codes_key(dd, c);
            key = k2 > key ? k2 : key;
          }
        }
      const unsigned long long other = __shfl_xor(key, 32, 64);
      key = other > key ? other : key;
      if (h == 0 && key > seen) atomicMax(&best[q], key);
    } else {
      // top-k: unit = one 32-row tile, whose scores for a question sit in the lane pair (l, l ^ 32); `seen` is the bound
#pragma unroll
      for (int r = 0; r < R; r++) {
        const bool may = live && mr[r] > 0.f && __float_as_uint(mr[r]) >= (unsigned)(seen >> 32);
        if (!__any(may)) continue;
        unsigned cm = 0u;
        unsigned long long mx = 0ull;
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const int c = row_of(r, e, h);
          const float dd = d[r][e];
          const unsigned long long k2 = codes_key(dd, c);
          const bool ok = may && c < words && c != e1 && c != e2 && c != e3 && dd > 0.f && k2 > seen;
          cm |= ok ? 1u << e : 0u;
          mx = (ok && k2 > mx) ? k2 : mx;
        }
        if (!__any(cm != 0u)) continue;
        const int n_me = __builtin_popcount(cm), n_ot = __shfl_xor(n_me, 32, 64), tot = n_me + n_ot;
        const unsigned long long om = __shfl_xor(mx, 32, 64), pm = mx > om ? mx : om;   // the pair's largest candidate
        const int unit = tile0 + r;
        unsigned long long *slot = tk.keys + ((long long)q * tk.nunits + unit) * tk.cap;   // (used by lanes with candidates only)
        unsigned long long kth = 0ull;
        if (__any(tot > tk.cap)) {
          // more candidates than the slot holds (k < 32 only): a key's place is its rank in the pair, the first cap stay
          const unsigned cmo = __shfl_xor(cm, 32, 64);
          float dq[16];
#pragma unroll
          for (int e = 0; e < 16; e++) dq[e] = __shfl_xor(d[r][e], 32, 64);
#pragma unroll
          for (int e = 0; e < 16; e++) {
            const unsigned long long mine = codes_key(d[r][e], row_of(r, e, h));
            int rank = 0;
#pragma unroll
            for (int x = 0; x < 16; x++) {
              const unsigned long long ka = (cm >> x) & 1u ? codes_key(d[r][x], row_of(r, x, h)) : 0ull;
              const unsigned long long kb = (cmo >> x) & 1u ? codes_key(dq[x], row_of(r, x, h ^ 1)) : 0ull;
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
            if ((cm >> e) & 1u) slot[pos++] = codes_key(d[r][e], row_of(r, e, h));
        }
        if (h == 0 && pm) {
          tk.cnt[(long long)q * tk.nunits + unit] = (unsigned char)(tot < tk.cap ? tot : tk.cap);
          if (kth && tk.cap == tk.k) atomicMax(&best[q], kth);
          topk_note_max(tk.bkt, tk.k, best, q, unit, pm);
        }
      }
    }
  }
}

// the kernel instance for ks K steps: {register-resident steps, row tiles per wavefront, chunked}
template <typename F>
hipError_t dispatch_ks(int ks, F &&f) {
#define W2B_KS(n, r) if (ks <= n) return f(std::integral_constant<int, n>(), std::integral_constant<int, r>(), std::false_type());
  W2B_KS(1, 2) W2B_KS(2, 2) W2B_KS(4, 2) W2B_KS(7, 2) W2B_KS(10, 2) W2B_KS(13, 2)
  W2B_KS(16, 1) W2B_KS(20, 1) W2B_KS(26, 1) W2B_KS(32, 1) W2B_KS(W2B_CODES_KS_MAX, 1)
#undef W2B_KS
  return f(std::integral_constant<int, W2B_CODES_KS_MAX>(), std::integral_constant<int, 1>(), std::true_type());
}

inline int codes_tiles_per_wave(int dim) { return (dim + 31) / 32 <= 13 ? 2 : 1; }

}  // namespace

size_t w2b_codes_operand_bytes(int dim, long long nq) {
  const long long ks = (dim + 31) / 32, qtiles = (nq + 31) / 32;
  return (size_t)(qtiles * ks * 192 + 192) * 16;
}

void w2b_codes_topk_layout(long long words, int dim, int k, int *nunits, int *cap) {
  const long long per_wg = 4ll * codes_tiles_per_wave(dim);              // 32-row tiles of a workgroup
  const long long tiles = (words + CROWS - 1) / CROWS;
  *nunits = (int)((tiles + per_wg - 1) / per_wg * per_wg);
  *cap = k < CROWS ? k : CROWS;
}

hipError_t w2b_launch_codes_roww(const uint32_t *B, int dim, long long words, long long rows_padded, const float *wtab,
                                 float *wrow, hipStream_t s) {
  const int nw = (dim + 63) / 64 * 4;
  hipLaunchKernelGGL(k_codes_roww, dim3((unsigned)((rows_padded + 255) / 256)), dim3(256), 0, s, B, nw, dim, words, rows_padded,
                     wtab, wrow);
  return hipGetLastError();
}

hipError_t w2b_launch_codes_operands(const uint32_t *B, int dim, int nq, const float *wrow, const int *b1, const int *b2,
                                     const int *b3, void *T, float *Wq, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  const int ks = (dim + 31) / 32, nw = (dim + 63) / 64 * 4, qtiles = (nq + 31) / 32;
  const long long n = (long long)qtiles * ks * 192 + 192;
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(k_codes_operands, dim3(blocks), dim3(256), 0, s, B, nw, dim, ks, nq, qtiles, wrow, b1, b2, b3, (i32x4 *)T, Wq);
  return hipGetLastError();
}

namespace {
template <bool COSMUL>
hipError_t codes_scan(const uint32_t *B, int words, int dim, const float *wrow, const void *T, const float *Wq, int nq,
                      const int *b1, const int *b2, const int *b3, int k, unsigned long long *best, unsigned long long *bkt,
                      unsigned long long *keys, unsigned char *cnt, unsigned long long *out, hipStream_t s) {
  if (nq <= 0 || words <= 0) return hipSuccess;
  const int ks = (dim + 31) / 32, nw = (dim + 63) / 64 * 4, qtiles = (nq + 31) / 32;
  TopkArgs tk{};
  if (k > 0) {
    tk.keys = keys;
    tk.cnt = cnt;
    tk.bkt = bkt;
    tk.k = k;
    w2b_codes_topk_layout(words, dim, k, &tk.nunits, &tk.cap);
  }
  const hipError_t e = dispatch_ks(ks, [&](auto ksmax, auto tiles, auto chunked) {
    constexpr int KS = decltype(ksmax)::value, R = decltype(tiles)::value;
    constexpr bool CH = decltype(chunked)::value;
    // row groups x ranges of question tiles: about a thousand workgroups, so that the device is full and a wavefront's
    // unpacked rows serve many question tiles
    const int gx = (words + 4 * R * CROWS - 1) / (4 * R * CROWS);
    int gy = (1024 + gx - 1) / gx;
    if (gy > qtiles) gy = qtiles;
    const int per_y = (qtiles + gy - 1) / gy;
    gy = (qtiles + per_y - 1) / per_y;
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if constexpr (COSMUL)
      hipLaunchKernelGGL((k_codes_scan<KS, R, CH, true, true>), grid, dim3(CT), 0, s, B, nw, words, wrow, (const i32x4 *)T, Wq, ks,
                         nq, qtiles, per_y, b1, b2, b3, best, tk, RankArgs{});
    else if (k > 0)
      hipLaunchKernelGGL((k_codes_scan<KS, R, CH, true>), grid, dim3(CT), 0, s, B, nw, words, wrow, (const i32x4 *)T, Wq, ks, nq,
                         qtiles, per_y, b1, b2, b3, best, tk, RankArgs{});
    else
      hipLaunchKernelGGL((k_codes_scan<KS, R, CH, false>), grid, dim3(CT), 0, s, B, nw, words, wrow, (const i32x4 *)T, Wq, ks, nq,
                         qtiles, per_y, b1, b2, b3, best, tk, RankArgs{});
    return hipGetLastError();
  });
  if (e != hipSuccess || k <= 0) return e;
  return w2b_launch_eval_topk_merge(keys, cnt, tk.nunits, tk.cap, k, nq, out, s);
}
}  // namespace

hipError_t w2b_launch_codes_scan(const uint32_t *B, int words, int dim, const float *wrow, const void *T, const float *Wq,
                                 int nq, const int *b1, const int *b2, const int *b3, int k, unsigned long long *best,
                                 unsigned long long *bkt, unsigned long long *keys, unsigned char *cnt,
                                 unsigned long long *out, hipStream_t s) {
  return codes_scan<false>(B, words, dim, wrow, T, Wq, nq, b1, b2, b3, k, best, bkt, keys, cnt, out, s);
}

// the 3CosMul form (k >= 1 only): the arguments of the top-k form above
hipError_t w2b_launch_codes_scan_cosmul(const uint32_t *B, int words, int dim, const float *wrow, const void *T,
                                        const float *Wq, int nq, const int *b1, const int *b2, const int *b3, int k,
                                        unsigned long long *bound, unsigned long long *bkt, unsigned long long *keys,
                                        unsigned char *cnt, unsigned long long *out, hipStream_t s) {
  if (k < 1) return hipErrorInvalidValue;
  return codes_scan<true>(B, words, dim, wrow, T, Wq, nq, b1, b2, b3, k, bound, bkt, keys, cnt, out, s);
}

// ---------------------------------------------------------------------------------------------- rank of a given row
namespace {

// J(x, c) = sum_a t_x[a] t_c[a] of two packed rows by popcounts on their 32-bit halves (the one-word path of the pair
// question, w2b_kernels_evalpairs.hip): |t_x t_c| = 1 + 2 m_x + 2 m_c + 4 m_x m_c, its sign that of s_x ^ s_c.
__device__ __forceinline__ int codes_dot(const uint32_t *__restrict__ x, const uint32_t *__restrict__ c, int nw, int dim) {
  int j = 0;
  for (int b = 0; 4 * b < nw; b++) {
    const int cols = dim - 64 * b;                                    // >= 1
    const uint32_t v[2] = {cols >= 32 ? ~0u : (1u << cols) - 1u, cols >= 64 ? ~0u : (cols <= 32 ? 0u : (1u << (cols - 32)) - 1u)};
#pragma unroll
    for (int hh = 0; hh < 2; hh++) {
      const uint32_t s = x[4 * b + hh] ^ c[4 * b + hh], pos = ~s & v[hh], neg = s & v[hh];
      const uint32_t mx = x[4 * b + 2 + hh], mc = c[4 * b + 2 + hh], mm = mx & mc;
      j += (__builtin_popcount(pos) - __builtin_popcount(neg)) + 2 * (__builtin_popcount(pos & mx) - __builtin_popcount(neg & mx)) +
           2 * (__builtin_popcount(pos & mc) - __builtin_popcount(neg & mc)) + 4 * (__builtin_popcount(pos & mm) - __builtin_popcount(neg & mm));
    }
  }
  return j;
}

// One lane per question, ahead of the rank scan: the target's score by the scan's own float sequence (0 when the target is
// one of the question's rows or its score is not > 0), and what the rows that the answer list leaves out -- the question's
// distinct rows and the target itself -- add to the scan's two counts, which excludes nothing.
__global__ void __launch_bounds__(256)
k_codes_rank_targets(const uint32_t *__restrict__ B, int nw, int dim, int nq, const float *__restrict__ wrow,
                     const int *__restrict__ b1, const int *__restrict__ b2, const int *__restrict__ b3,
                     const int *__restrict__ target, float *__restrict__ tscore, uint2 *__restrict__ corr) {
  const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (q >= nq) return;
  const int e1 = b1[q], e2 = b2[q], e3 = b3[q], g = target[q];
  const uint32_t *r1 = B + (long long)e1 * nw, *r2 = B + (long long)e2 * nw, *r3 = B + (long long)e3 * nw;
  const float w1 = wrow[e1], w2 = wrow[e2], w3 = wrow[e3];
  auto score = [&](int c) {
    const uint32_t *rc = B + (long long)c * nw;
    return codes_add_score(codes_term(codes_dot(r1, rc, nw, dim), w1), codes_term(codes_dot(r2, rc, nw, dim), w2),
                           codes_term(codes_dot(r3, rc, nw, dim), w3), wrow[c]);
  };
  const float ts = score(g);
  const bool ranked = g != e1 && g != e2 && g != e3 && ts > 0.f;
  uint32_t before = 0, equal = 1;                        // the target itself has its own score
  const int own[3] = {e1, e2, e3};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    if ((i > 0 && own[i] == own[0]) || (i > 1 && own[i] == own[1])) continue;
    const float so = score(own[i]);
    equal += so == ts ? 1u : 0u;
    before += (so > ts || (so == ts && own[i] < g)) ? 1u : 0u;
  }
  tscore[q] = ranked ? ts : 0.f;
  corr[q] = ranked ? make_uint2(before, equal) : make_uint2(0u, 0u);
}

}  // namespace

// The rank of a given row on 2-bit rows: T / Wq as w2b_launch_codes_operands leaves them; tscore [nq] and corr [nq] are
// written here, cnt [nq] (zeroed by the caller) receives (rows with the target's score << 32 | rows before the target), own
// rows and target included; corr holds their share of both.
hipError_t w2b_launch_codes_rank(const uint32_t *B, int words, int dim, const float *wrow, const void *T, const float *Wq,
                                 int nq, const int *b1, const int *b2, const int *b3, const int *target, float *tscore,
                                 unsigned int *corr, unsigned long long *cnt, hipStream_t s) {
  if (nq <= 0 || words <= 0) return hipSuccess;
  const int ks = (dim + 31) / 32, nw = (dim + 63) / 64 * 4, qtiles = (nq + 31) / 32;
  hipLaunchKernelGGL(k_codes_rank_targets, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, B, nw, dim, nq, wrow, b1, b2, b3,
                     target, tscore, (uint2 *)corr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const RankArgs rk{target, tscore, cnt};
  return dispatch_ks(ks, [&](auto ksmax, auto tiles, auto chunked) {
    constexpr int KS = decltype(ksmax)::value, R = decltype(tiles)::value;
    constexpr bool CH = decltype(chunked)::value;
    const int gx = (words + 4 * R * CROWS - 1) / (4 * R * CROWS);      // the grid of codes_scan
    int gy = (1024 + gx - 1) / gx;
    if (gy > qtiles) gy = qtiles;
    const int per_y = (qtiles + gy - 1) / gy;
    gy = (qtiles + per_y - 1) / per_y;
    hipLaunchKernelGGL((k_codes_scan<KS, R, CH, false, false, true>), dim3((unsigned)gx, (unsigned)gy), dim3(CT), 0, s, B, nw, words,
                       wrow, (const i32x4 *)T, Wq, ks, nq, qtiles, per_y, b1, b2, b3, (unsigned long long *)nullptr, TopkArgs{}, rk);
    return hipGetLastError();
  });
}
