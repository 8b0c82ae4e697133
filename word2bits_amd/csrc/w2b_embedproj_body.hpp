// w2b_embedproj_body.hpp -- the K loop of the packed embedding's projection, written once for the kernels that need its
// logits: k_embed_project (w2b_kernels_embedproj.hip), which stores them, and the cross-entropy's statistics and gradient
// kernels (w2b_kernels_embedxent.hip), which reduce them or turn them into g.  The comment at the head of
// w2b_kernels_embedproj.hip explains the operand roles, the interleaved candidate tiles, the staging and the two regimes;
// nothing of that differs between the kernels, which is what makes their logits the same bits.  What differs is the
// EPILOGUE, a callable the kernel passes in: it is called once per pair of vector tiles with the finished accumulators.
//
//   epi(acc, pr, j0, l32, h, live, q)
//     acc[r][t][e] in lane l = 32 h + l32: the chain S of vector 32 (PV pr + t) + 8 (e / 4) + 4 h + e % 4 (an index into the
//     launch's operand staging) against candidate j0 + 2 l32 + r; live[r]: that candidate is a row of the table (not padding,
//     not refused, not past m); q: the factor of the one multiply that makes a logit of S.
//
// Epi::kAllWaves says whether the epilogue synchronises the workgroup: then a wavefront whose 64 candidates all lie past m
// stays (every lane dead, zeros in the row operand) instead of leaving before the K loop.
#pragma once
#include "w2b_internal.h"

namespace w2b_proj {

constexpr int PT = 256;        // threads of a workgroup: four wavefronts, each with its own 64 candidates
constexpr int PR = 2;          // interleaved 32-candidate tiles of a wavefront
constexpr int PV = 2;          // 32-vector tiles multiplied at a time: the pairs of k_vec_operands
constexpr int PW = 8;          // 64-column blocks whose packed words a lane keeps in registers
constexpr int PWG = 8192;      // workgroups a launch aims at

typedef float pf32x4 __attribute__((ext_vector_type(4)));
typedef float pf32x16 __attribute__((ext_vector_type(16)));

// T = the packed table [rows][BL * nb] (nb = ceil(dim / 64)); cand = the candidates' rows [m] or nullptr, then candidate j
// is row cand_base + j; X = the vectors' operands in fragment order, ng = ceil(dim / 8); the workgroup takes
// pairs_per_y pairs from pair0 + blockIdx.y * pairs_per_y on, below vpairs.  count_bad: ids >= rows are counted in *bad (once per candidate).
template <int BL, class Epi>
__device__ __forceinline__ void embed_project_body(const uint64_t *__restrict__ T, int nb, long long rows,
                                                   const long long *__restrict__ cand, long long cand_base, int m,
                                                   const pf32x4 *__restrict__ X, int ng, int pair0, int vpairs,
                                                   int pairs_per_y, bool count_bad, unsigned long long *bad, Epi &epi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l32 = lane & 31, h = lane >> 5;
  const int j0 = ((int)blockIdx.x * 4 + wave) * (32 * PR);
  const int pr0 = pair0 + (int)blockIdx.y * pairs_per_y, pr1 = min(vpairs, pr0 + pairs_per_y);
  if ((!Epi::kAllWaves && j0 >= m) || pr0 >= pr1) return;
  const bool chunked = nb > PW;
  const float q = BL == 1 ? __uint_as_float(0x3EAAAAABu) : 0.25f;

  // this lane's two candidates: a row of the table only when 0 <= id < rows
  const uint64_t *pw[PR];
  bool live[PR];
#pragma unroll
  for (int r = 0; r < PR; r++) {
    const int j = j0 + 2 * l32 + r;
    long long id = -1;
    if (j < m) id = cand ? cand[j] : cand_base + j;
    if (count_bad && id >= rows && h == 0 && blockIdx.y == 0) atomicAdd(bad, 1ull);
    live[r] = id >= 0 && id < rows;
    pw[r] = T + (live[r] ? id : 0ll) * (BL * nb);
  }

  // the packed words of this lane's rows, shifted right by its k index: [tile][block][sign lo, sign hi(, magnitude lo, hi)]
  uint32_t rw[PR][PW][2 * BL];
  auto load_chunk = [&](int c0) {
#pragma unroll
    for (int r = 0; r < PR; r++)
#pragma unroll
      for (int b = 0; b < PW; b++)
#pragma unroll
        for (int k = 0; k < BL; k++) {
          // (every address is one of the table's: a block that does not exist reads the last one and keeps zeros)
          uint64_t v = 0ull;
          if (live[r]) v = pw[r][BL * min(c0 + b, nb - 1) + k];
          if (c0 + b >= nb) v = 0ull;
          rw[r][b][2 * k] = (uint32_t)v >> h;
          rw[r][b][2 * k + 1] = (uint32_t)(v >> 32) >> h;
        }
  };
  if (!chunked) load_chunk(0);

  const pf32x4 *p = X + (long long)pr0 * ng * (PV * 64) + lane;
  pf32x4 ax[2][PV];                               // [0]: the group about to be multiplied, [1]: the one requested behind it
#pragma unroll
  for (int t = 0; t < PV; t++) ax[0][t] = p[64 * t];

  for (int pr = pr0; pr < pr1; pr++) {
    pf32x16 acc[PR][PV];
#pragma unroll
    for (int r = 0; r < PR; r++)
#pragma unroll
      for (int t = 0; t < PV; t++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[r][t][e] = 0.f;
    for (int c0 = 0; c0 < nb; c0 += PW) {           // one pass unless chunked
      if (chunked) load_chunk(c0);
      // the packed words are the same for every pair unless chunked; the compiler must not therefore decode them once for
      // all pairs and keep the floats: from here on they are values it knows nothing about
#pragma unroll
      for (int r = 0; r < PR; r++)
#pragma unroll
        for (int b = 0; b < PW; b++)
#pragma unroll
          for (int k = 0; k < 2 * BL; k++) asm volatile("" : "+v"(rw[r][b][k]));
      const int left = ng - 8 * c0;                 // groups of 8 columns from this chunk's first one to the row's end
#pragma unroll
      for (int j = 0; j < 8 * PW; j++) {            // group j of the chunk: block j / 8, half (j / 4) % 2, bits 8 (j % 4) ..
        if (j < left) {
          // the next group of this stream (behind the launch's last one: zeros) into the other half of ax: no copies
#pragma unroll
          for (int t = 0; t < PV; t++) ax[(j + 1) & 1][t] = p[(j + 1) * (PV * 64) + 64 * t];
#pragma unroll
          for (int i = 0; i < 4; i++) {               // K step: columns 64 (c0 + j / 8) + 8 (j % 8) + 2 i + h
            const int b = j >> 3, half = (j >> 2) & 1, bit = 8 * (j & 3) + 2 * i;
            float tr[PR];
#pragma unroll
            for (int r = 0; r < PR; r++) {
              uint32_t v = 0x3F800000u;
              if constexpr (BL == 2) v = ((rw[r][b][2 + half] >> bit) & 1u) ? 0x40400000u : 0x3F800000u;
              tr[r] = __uint_as_float(v | ((rw[r][b][half] << (31 - bit)) & 0x80000000u));
            }
#pragma unroll
            for (int r = 0; r < PR; r++)
#pragma unroll
              for (int t = 0; t < PV; t++)
                acc[r][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ax[j & 1][t][i], tr[r], acc[r][t], 0, 0, 0);
          }
        }
      }
      const int done = min(left, 8 * PW);
      p += done * (PV * 64);
      if (done & 1) {                               // (a chunk that is not the row's last one has 8 PW groups: even)
#pragma unroll
        for (int t = 0; t < PV; t++) {
          const pf32x4 o = ax[0][t];
          ax[0][t] = ax[1][t];
          ax[1][t] = o;
        }
      }
    }
    epi(acc, pr, j0, l32, h, live, q);
  }
}

}  // namespace w2b_proj
