// w2b_kernels_evalvec.hip -- the evaluator's float-vector question on bit-packed rows (include/word2bits_eval.h, "vector
// questions"): which rows are nearest to a float vector that the caller computed itself?
//
// A question is `size` floats x[a]; the row operand is t_c[a] = +-1 (1-bit rows) or +-1 / +-3 (2-bit rows), and
//   S(c) = the float32 chain  acc = +0;  acc = fmaf(x[a], (float)t_c[a], acc)  for a = 0 .. size - 1,
// one accumulator per (question, row), strictly in column order.  That is v_mfma_f32_32x32x2_f32, whose accumulators ARE
// sequential fmaf chains in k order (w2b_kernels_eval.hip relies on it and its parity tests measure it), with one
// difference to k_eval_topk_mfma: the row operand never exists in memory as floats.  A lane keeps its row's PACKED words
// in registers -- per 64 columns two 32-bit halves of sign bits, at 2 bits two more of magnitude bits, both lanes of a
// pair (l, l ^ 32) the same row, each shifted right by its k index l / 32 -- and builds the one float a K step needs with
// integer operations: the sign bit moved to bit 31 and or-ed into 0x3F800000 (1.0f), at 2 bits after a select between
// 0x3F800000 and 0x40400000 (3.0f) on the magnitude bit.  Two or five vector instructions per K step and row tile, under
// MFMAs of 64 matrix cycles each; no decoded float outlives its K step (at size 800 they would be 400 registers per tile).
//
// Shape: the vocabulary rows are the A operand and the questions B, as in k_codes_scan, so a lane owns ONE question
// (column lane % 32) and 16 rows of a 32 x 32 tile.  A wavefront holds VR = 2 row tiles and walks the question tiles VQ = 2
// at a time: four accumulator tiles (64 registers), every decoded float feeds two MFMAs and every question value two.
// The question operands lie in memory in fragment order (k_vec_operands): for a pair of question tiles and a group of 8
// columns, 2 x 64 float4 -- lane l of tile t holds x[question 32 t + l % 32][columns 8 g + 2 i + l / 32], i = 0 .. 3, the B
// operands of four K steps -- one coalesced 16-byte load per lane, tile and group, requested one group ahead.  Columns >=
// size and questions that do not exist are +0 there, and one zero group follows the last pair for the last prefetch.  The
// zeros are REQUIRED: the padding bits of a packed row decode to t = +1, and fmaf(+0, t, acc) == acc for every acc this
// chain can hold (acc starts at +0 and a float sum is -0 only if both terms are).  Rows past the vocabulary decode to
// +1 throughout; the selection drops them by their row number.
//
// Regimes.  VW = 8 blocks of 64 columns are register-resident: 2 x 8 x 2 = 32 registers of packed words at 1 bit, 64 at
// 2 bits, next to 64 accumulators and 16 of question operands -- under 256, so two workgroups share a CU.  There are two
// regimes and ONE border, the same for both bit levels and with VR = 2 on either side of it:
//   size <= 512   the packed words are loaded once per wavefront and serve every question tile of its range;
//   size >= 513   chunks: the K loop walks the row in chunks of 512 columns and loads each chunk's words again for every
//                 pair of question tiles (16 or 32 bytes per lane and chunk under 1024 MFMAs: "unpacking" is a load here,
//                 which is why the border can sit this low).  The accumulators live across the chunks: same chain.
// Inside a chunk the unrolled K loop leaves at the first group of 8 columns at or past `size` (a wavefront-uniform
// branch per 16 MFMAs), so a size costs ceil(size / 8) groups whatever it is; the steps of the last group past `size`
// multiply the +0 operands.
// The two empty asm statements below (on the packed words at the head of a chunk, on the tile's first row number before the
// epilogue) only stop the compiler from hoisting per-pair work out of the loop over question-tile pairs and keeping hundreds
// of values alive across the K loop.  They steer one compiler's optimiser: after a toolchain update check the register
// report again (profiles/eval_vectors_kernel_resources.txt: no scratch access between the first and the last MFMA).
//
// Epilogue: score = (S * wx) * w(c), both products rounded on their own -- wx from the host (1 / sqrt(sum x^2) or 1, 0
// for a zero vector), w(c) the codes table or the constant 1 / sqrt(size) of 1-bit rows -- then the selection of
// w2b_eval_select.hpp with a 32-row tile as the unit, as k_bag_scan has it without the exclusion list, and the fp32 scan's
// merge kernel.  The key is score bits << 32 | ~row in both modes.  The Q x V score matrix never exists in memory.
#include "w2b_internal.h"
#include "w2b_eval_select.hpp"
#include "w2b_eval_codes.hpp"

namespace {

// wavefronts per SIMD that k_vec_scan is built for: 2 = at most 256 registers (the compiler then spills around the selection
// code, never inside the K loop), 1 = 512 registers and no spill; -DW2B_VEC_WAVES=1 builds the other one for a comparison
#ifndef W2B_VEC_WAVES
#define W2B_VEC_WAVES 2
#endif
constexpr int VR = 2;          // 32-row tiles of a wavefront
constexpr int VQ = 2;          // 32-question tiles scored at a time
constexpr int VW = 8;          // 64-column blocks whose packed words a lane keeps in registers
constexpr int VWG = 8192;      // workgroups a launch aims at (a workgroup's rows cost one load: many short ones, a short tail)

typedef float vf32x16 __attribute__((ext_vector_type(16)));

// The question operands in fragment order, X[((pair * ng + g) * VQ + t) * 64 + lane] (float4): question (pair * VQ + t) * 32
// + lane % 32, columns 8 g + 2 i + lane / 32 in element i; +0 where the column or the question does not exist, and in the
// VQ * 64 slots behind the last pair.  Every slot is written: the caller zeroes nothing.
__global__ void k_vec_operands(const float *__restrict__ x, int dim, int ng, int nq, long long n_main,
                               cf32x4 *__restrict__ X) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_main + VQ * 64; i += stride) {
    cf32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (i < n_main) {
      const int lane = (int)(i & 63), t = (int)((i >> 6) % VQ), g = (int)((i / (64 * VQ)) % ng);
      const long long pair = i / (64ll * VQ * ng), q = (pair * VQ + t) * 32 + (lane & 31);
      if (q < nq) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int col = 8 * g + 2 * j + (lane >> 5);
          if (col < dim) o[j] = x[q * dim + col];
        }
      }
    }
    X[i] = o;
  }
}

// B = the packed rows, [words][BL * nb] 64-bit words (nb = ceil(size / 64)); wrow = w(c) per row (BL = 2) or nullptr and
// wconst = the one weight of every 1-bit row; Wx = the questions' weights [32 * VQ * qpairs], 0 = no answers; ng =
// ceil(size / 8).  `best` is the bound of the selection state.
template <int BL>
__global__ void __launch_bounds__(CT, W2B_VEC_WAVES)
k_vec_scan(const uint64_t *__restrict__ B, int nb, int words, const float *__restrict__ wrow, float wconst,
           const cf32x4 *__restrict__ X, const float *__restrict__ Wx, int ng, int nq, int qpairs, int pairs_per_y,
           unsigned long long *__restrict__ best, const TopkArgs tk) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l32 = lane & 31, h = lane >> 5;
  const int tile0 = ((int)blockIdx.x * 4 + wave) * VR, r0 = tile0 * CROWS;
  const int pr0 = (int)blockIdx.y * pairs_per_y, pr1 = min(qpairs, pr0 + pairs_per_y);
  if (r0 >= words || pr0 >= pr1) return;          // (no barrier in this kernel)
  const bool chunked = nb > VW;

  // the packed words of this lane's rows, shifted right by its k index: [tile][block][sign lo, sign hi(, magnitude lo, hi)]
  uint32_t rw[VR][VW][2 * BL];
  auto load_chunk = [&](int c0) {
#pragma unroll
    for (int r = 0; r < VR; r++) {
      // (every address is one of the table's: a row or a block that does not exist reads the last one and keeps zeros)
      const int row = r0 + r * CROWS + l32;
      const uint64_t *pw = B + (long long)min(row, words - 1) * (BL * nb);
#pragma unroll
      for (int b = 0; b < VW; b++)
#pragma unroll
        for (int m = 0; m < BL; m++) {
          const uint64_t got = pw[BL * min(c0 + b, nb - 1) + m];
          const uint64_t v = (row < words && c0 + b < nb) ? got : 0ull;
          rw[r][b][2 * m] = (uint32_t)v >> h;
          rw[r][b][2 * m + 1] = (uint32_t)(v >> 32) >> h;
        }
    }
  };
  if (!chunked) load_chunk(0);

  const cf32x4 *p = X + (long long)pr0 * ng * (VQ * 64) + lane;
  cf32x4 bq[2][VQ];                               // [0]: the group about to be multiplied, [1]: the one requested behind it
#pragma unroll
  for (int t = 0; t < VQ; t++) bq[0][t] = p[64 * t];

  for (int pr = pr0; pr < pr1; pr++) {
    vf32x16 acc[VR][VQ];
#pragma unroll
    for (int r = 0; r < VR; r++)
#pragma unroll
      for (int t = 0; t < VQ; t++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[r][t][e] = 0.f;
    for (int c0 = 0; c0 < nb; c0 += VW) {           // one pass unless chunked
      if (chunked) load_chunk(c0);
      // the packed words are the same for every pair unless chunked; the compiler must not therefore decode them once for
      // all pairs and keep the floats: from here on they are values it knows nothing about
#pragma unroll
      for (int r = 0; r < VR; r++)
#pragma unroll
        for (int b = 0; b < VW; b++)
#pragma unroll
          for (int m = 0; m < 2 * BL; m++) asm volatile("" : "+v"(rw[r][b][m]));
      const int left = ng - 8 * c0;                 // groups of 8 columns from this chunk's first one to the row's end
#pragma unroll
      for (int j = 0; j < 8 * VW; j++) {            // group j of the chunk: block j / 8, half (j / 4) % 2, bits 8 (j % 4) ..
        if (j < left) {
          // the next group of this stream (behind the launch's last one: zeros) into the other half of bq: no copies
#pragma unroll
          for (int t = 0; t < VQ; t++) bq[(j + 1) & 1][t] = p[(j + 1) * (VQ * 64) + 64 * t];
#pragma unroll
          for (int i = 0; i < 4; i++) {               // K step: columns 64 (c0 + j / 8) + 8 (j % 8) + 2 i + h
            const int b = j >> 3, half = (j >> 2) & 1, bit = 8 * (j & 3) + 2 * i;
            float a[VR];
#pragma unroll
            for (int r = 0; r < VR; r++) {
              uint32_t v = 0x3F800000u;
              if constexpr (BL == 2) v = ((rw[r][b][2 + half] >> bit) & 1u) ? 0x40400000u : 0x3F800000u;
              a[r] = __uint_as_float(v | ((rw[r][b][half] << (31 - bit)) & 0x80000000u));
            }
#pragma unroll
            for (int r = 0; r < VR; r++)
#pragma unroll
              for (int t = 0; t < VQ; t++)
                acc[r][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r], bq[j & 1][t][i], acc[r][t], 0, 0, 0);
          }
        }
      }
      const int done = min(left, 8 * VW);
      p += done * (VQ * 64);
      if (done & 1) {                               // (a chunk that is not the row's last one has 8 VW groups: even)
#pragma unroll
        for (int t = 0; t < VQ; t++) {
          const cf32x4 o = bq[0][t];
          bq[0][t] = bq[1][t];
          bq[1][t] = o;
        }
      }
    }

    // Accumulator e of tile (r, t) in lane l: row r0 + 32 r + 8 (e / 4) + 4 (l / 32) + e % 4, question 32 t + l % 32 of the pair.
    // (the row numbers, their keys and their comparisons with `words` are the same for every pair: r0e keeps the compiler
    // from holding 32 of each in registers across the K loop)
    int r0e = r0;
    asm volatile("" : "+v"(r0e));
    // unit = one 32-row tile, whose scores for a question sit in the lane pair (l, l ^ 32); `seen` is the bound
    auto select_tile = [&](const vf32x16 &S, int r, int q, bool live, float wx, unsigned long long seen) {
      // u = the score bits of the key, 0 where the row is no answer (score <= 0)
      unsigned u[16], mr = 0u;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        cf32x4 wc = {wconst, wconst, wconst, wconst};
        if constexpr (BL == 2) wc = *(const cf32x4 *)(wrow + r0 + r * CROWS + 8 * g + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int e = 4 * g + i;
          const float d = __fmul_rn(__fmul_rn(S[e], wx), wc[i]);
          u[e] = d > 0.f ? __float_as_uint(d) : 0u;
          mr = u[e] > mr ? u[e] : mr;
        }
      }
      const bool may = live && mr > 0u && mr >= (unsigned)(seen >> 32);
      if (!__any(may)) return;
      topk_select_unit32(u, may, r0e + r * CROWS, h, words, q, tile0 + r, seen, best, tk);
    };
#pragma unroll
    for (int t = 0; t < VQ; t++) {
      const int q = (pr * VQ + t) * 32 + l32;
      const bool live = q < nq;
      const float wx = Wx[q];
      const unsigned long long seen = live ? ld_key(&best[q]) : ~0ull;   // possibly stale: then it is only lower
#pragma unroll
      for (int r = 0; r < VR; r++) select_tile(acc[r][t], r, q, live, wx, seen);
    }
  }
}

inline long long vec_pairs(long long nq) { return (nq + 32 * VQ - 1) / (32 * VQ); }

}  // namespace

// float4 slots of the operands of nq questions: the pairs' groups and the zero group behind them
static long long vec_operand_slots(int dim, long long nq) { return vec_pairs(nq) * ((dim + 7) / 8) * (VQ * 64) + VQ * 64; }

size_t w2b_vec_operand_bytes(int dim, long long nq) { return (size_t)vec_operand_slots(dim, nq) * 16; }
long long w2b_vec_weight_slots(long long nq) { return vec_pairs(nq) * (32 * VQ); }

void w2b_vec_topk_layout(long long words, int k, int *nunits, int *cap) {
  const long long per_wg = 4ll * VR, tiles = (words + CROWS - 1) / CROWS;    // 32-row tiles of a workgroup, of the table
  *nunits = (int)((tiles + per_wg - 1) / per_wg * per_wg);
  *cap = k < CROWS ? k : CROWS;
}

hipError_t w2b_launch_vec_operands(const float *x, int dim, int nq, void *X, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  const long long n = vec_operand_slots(dim, nq);
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(k_vec_operands, dim3(blocks), dim3(256), 0, s, x, dim, (dim + 7) / 8, nq, n - VQ * 64, (cf32x4 *)X);
  return hipGetLastError();
}

hipError_t w2b_launch_vec_scan(const uint64_t *B, int words, int dim, int bitlevel, const float *wrow, float wconst,
                               const void *X, const float *Wx, int nq, int k, unsigned long long *bound,
                               unsigned long long *bkt, unsigned long long *keys, unsigned char *cnt, unsigned long long *out,
                               hipStream_t s) {
  if (nq <= 0 || words <= 0) return hipSuccess;
  TopkArgs tk{};
  tk.keys = keys;
  tk.cnt = cnt;
  tk.bkt = bkt;
  tk.k = k;
  w2b_vec_topk_layout(words, k, &tk.nunits, &tk.cap);
  const int nb = (dim + 63) / 64, ng = (dim + 7) / 8, qpairs = (int)vec_pairs(nq);
  // row groups x ranges of question-tile pairs
  const int gx = (words + 4 * VR * CROWS - 1) / (4 * VR * CROWS);
  int gy = (VWG + gx - 1) / gx;
  if (gy > qpairs) gy = qpairs;
  const int per_y = (qpairs + gy - 1) / gy;
  gy = (qpairs + per_y - 1) / per_y;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (bitlevel == 2)
    hipLaunchKernelGGL(k_vec_scan<2>, grid, dim3(CT), 0, s, B, nb, words, wrow, wconst, (const cf32x4 *)X, Wx, ng, nq, qpairs,
                       per_y, bound, tk);
  else
    hipLaunchKernelGGL(k_vec_scan<1>, grid, dim3(CT), 0, s, B, nb, words, wrow, wconst, (const cf32x4 *)X, Wx, ng, nq, qpairs,
                       per_y, bound, tk);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return w2b_launch_eval_topk_merge(keys, cnt, tk.nunits, tk.cap, k, nq, out, s);
}
