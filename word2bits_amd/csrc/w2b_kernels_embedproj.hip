// w2b_kernels_embedproj.hip -- the packed embedding's output projection (include/word2bits_embed.h, "Projection"):
//   out[i][j] = S * q,   S = the float32 chain  acc = +0;  acc = fmaf(x[i][a], (float)t_r[a], acc)  for a = 0 .. dim - 1,
// for n float vectors x against m candidate rows r = cand[j] of the bit-packed table (or every row), one accumulator per
// (vector, candidate), strictly in column order.  That is v_mfma_f32_32x32x2_f32, whose accumulators ARE sequential fmaf
// chains in k order, with the row operand decoded from the packed bits in registers: the K loop of k_vec_scan
// (w2b_kernels_evalvec.hip), whose comment explains the decode, the operand staging and the two regimes.  What is different
// here is the other end: a dense [n][m] store instead of a selection.
//
// Operand roles.  The VECTORS are the A operand and the table rows B (k_vec_scan has them the other way round; A and B have
// the same lane layout for this instruction, lane l = index l % 32 at k = l / 32, so the chain is the same).  Accumulator e
// of a tile in lane l then belongs to vector 8 (e / 4) + 4 (l / 32) + e % 4 and candidate l % 32: the 32 lanes of a half
// wave hold 32 candidates of ONE vector, which lie side by side in a row-major [n][m] output.  With the rows as A a lane
// would own one vector and 16 rows, and every store of a wavefront would touch 64 different lines.
// A wavefront holds PR = 2 candidate tiles and INTERLEAVES them: lane l of tile r owns candidate j0 + 2 (l % 32) + r (the
// rows are gathered per lane anyway, so the order costs nothing).  The two accumulators acc[0][t][e] and acc[1][t][e] of a
// lane are then ADJACENT output elements: one 8-byte store per lane at float32, 256 contiguous bytes per half wave and
// instruction; at 16 bits the two values are packed into one 4-byte store, 128 contiguous bytes, a full line.  Output row
// i starts at element i * m, which is odd for odd i and odd m: the pair store is used where its first element has an even
// index (the buffer itself is 256-byte aligned) and both candidates exist, two scalar stores otherwise; the tail of m is
// masked per element.
//
// The vector operands are staged in fragment order by k_vec_operands (w2b_launch_vec_operands: tiles in pairs, groups of 8
// columns, +0 where a column or a vector does not exist, one zero group behind the last pair).  The zeros are REQUIRED for
// the same reason as there: padding bits decode to t = +1 and only x = +0 makes a step a no-op.  For the same reason a
// candidate that is padding (id < 0), refused (id >= rows, counted once in *bad) or past m is not "zeroed" in the operand:
// it keeps zero words (all +1, a legal address is never even read for it) and its column is written as +0.0 in the epilogue.
//
// Regimes, as in k_vec_scan: dim <= 512 keeps a lane's packed words in registers for every pair of vector tiles; beyond
// that the K loop walks chunks of 512 columns and loads each chunk's words again per pair, the accumulators living across
// the chunks.  The empty asm statements keep the compiler from hoisting per-pair work (decoded floats, output offsets) out
// of the loop over pairs; profiles/embed_project_kernel_resources.txt is the register report to check after a toolchain
// update: no scratch access between the first and the last MFMA.
#include <hip/hip_fp16.h>

#include "../../include/word2bits_embed.h"
#include "w2b_internal.h"
#include "w2b_embedproj_body.hpp"

namespace {

using namespace w2b_proj;     // PT, PR, PV, PW, PWG, pf32x4, pf32x16 and the K loop (w2b_embedproj_body.hpp)

__device__ __forceinline__ uint32_t to16(float f, int dtype) {
  if (dtype == W2B_EMBED_BF16) {
    const uint32_t u = __float_as_uint(f);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
  }
  return __half_as_ushort(__float2half_rn(f));
}

// The epilogue of k_embed_project: the dense [n][m] store.
struct StoreEpilogue {
  static constexpr bool kAllWaves = false;          // (no barrier in this kernel)
  int m, n, dtype;
  void *__restrict__ out;
  __device__ __forceinline__ void operator()(const pf32x16 (&acc)[PR][PV], int pr, int j0, int l32, int h, const bool (&live)[PR],
                                             float q) const {
    // Accumulator e of tile (r, t) in lane l: vector 32 (PV pr + t) + 8 (e / 4) + 4 (l / 32) + e % 4, candidate j0 + 2 (l % 32) + r.
    // (jl is the same for every pair: the asm keeps the compiler from holding 16 output offsets in registers across the K loop)
    int jl = j0 + 2 * l32;
    asm volatile("" : "+v"(jl));
    const bool have0 = jl < m, have1 = jl + 1 < m;
#pragma unroll
    for (int t = 0; t < PV; t++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int v = (pr * PV + t) * 32 + 8 * (e >> 2) + 4 * h + (e & 3);
        if (v >= n) continue;
        const long long at = (long long)v * m + jl;            // element index of the lane's first candidate
        const float f0 = live[0] ? __fmul_rn(acc[0][t][e], q) : 0.f;
        const float f1 = live[1] ? __fmul_rn(acc[1][t][e], q) : 0.f;
        const bool pair = have1 && (at & 1) == 0;
        if (dtype == W2B_EMBED_F32) {
          float *o = reinterpret_cast<float *>(out) + at;
          if (pair) {
            *reinterpret_cast<float2 *>(o) = make_float2(f0, f1);
          } else {
            if (have0) o[0] = f0;
            if (have1) o[1] = f1;
          }
        } else {
          uint16_t *o = reinterpret_cast<uint16_t *>(out) + at;
          const uint32_t u0 = to16(f0, dtype), u1 = to16(f1, dtype);
          if (pair) {
            *reinterpret_cast<uint32_t *>(o) = u0 | (u1 << 16);
          } else {
            if (have0) o[0] = (uint16_t)u0;
            if (have1) o[1] = (uint16_t)u1;
          }
        }
      }
  }
};

// T = the packed table [rows][BL * nb] (nb = ceil(dim / 64)); cand = the candidates' rows [m] or nullptr, then candidate j
// is row cand_base + j; X = the vectors' operands in fragment order, ng = ceil(dim / 8); out = [n][m] of dtype.
template <int BL>
__global__ void __launch_bounds__(PT, 2)
k_embed_project(const uint64_t *__restrict__ T, int nb, long long rows, const long long *__restrict__ cand, long long cand_base,
                int m, const pf32x4 *__restrict__ X, int ng, int n, int vpairs, int pairs_per_y, int dtype,
                void *__restrict__ out, unsigned long long *bad) {
  StoreEpilogue epi{m, n, dtype, out};
  embed_project_body<BL>(T, nb, rows, cand, cand_base, m, X, ng, 0, vpairs, pairs_per_y, true, bad, epi);
}

}  // namespace

// bytes of the operand staging X for n vectors (the operand kernel writes every byte of it)
size_t w2b_embed_project_operand_bytes(int dim, long long n) { return w2b_vec_operand_bytes(dim, n); }

hipError_t w2b_launch_embed_project(const uint64_t *T, long long rows, int dim, int bitlevel, const float *x, int n,
                                    const long long *cand, long long cand_base, int m, int dtype, void *X, void *out,
                                    unsigned long long *bad, hipStream_t s) {
  if (n <= 0 || m <= 0) return hipSuccess;
  hipError_t e = w2b_launch_vec_operands(x, dim, n, X, s);
  if (e != hipSuccess) return e;
  const int nb = (dim + 63) / 64, ng = (dim + 7) / 8, vpairs = (n + 32 * PV - 1) / (32 * PV);
  // candidate groups x ranges of vector-tile pairs
  const int gx = (int)(((long long)m + 4 * PR * 32 - 1) / (4 * PR * 32));
  int gy = (PWG + gx - 1) / gx;
  if (gy > vpairs) gy = vpairs;
  const int per_y = (vpairs + gy - 1) / gy;
  gy = (vpairs + per_y - 1) / per_y;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (bitlevel == 2)
    hipLaunchKernelGGL(k_embed_project<2>, grid, dim3(PT), 0, s, T, nb, rows, cand, cand_base, m, (const pf32x4 *)X, ng, n, vpairs,
                       per_y, dtype, out, bad);
  else
    hipLaunchKernelGGL(k_embed_project<1>, grid, dim3(PT), 0, s, T, nb, rows, cand, cand_base, m, (const pf32x4 *)X, ng, n, vpairs,
                       per_y, dtype, out, bad);
  return hipGetLastError();
}
