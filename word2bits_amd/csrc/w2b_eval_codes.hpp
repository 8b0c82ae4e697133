// w2b_eval_codes.hpp -- what the evaluator's i8 matrix-core scans share (w2b_kernels_evalcodes.hip: three rows per
// question; w2b_kernels_evalbag.hip: one pooled integer vector per question): the scan workgroup's shape, the unpacking of
// packed 2-bit columns to int8 operands and the key.  Device code; the layout is described in w2b_kernels_evalcodes.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int CT = 256;        // threads of a scan workgroup: 4 wavefronts, each with its own rows
constexpr int CROWS = 32;      // rows of a unit (one MFMA tile)

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef float cf32x4 __attribute__((ext_vector_type(4)));

// bit j of a nibble -> bit 0 of byte j
__device__ __forceinline__ uint32_t spread4(uint32_t x) { return (x * 0x00204081u) & 0x01010101u; }

// 16 columns: sign bits, magnitude bits, valid bits -> 16 int8 (t, or 0 where the column does not exist), column j in byte j
__device__ __forceinline__ i32x4 codes_unpack16(uint32_t sg, uint32_t mg, uint32_t vb) {
  i32x4 o;
#pragma unroll
  for (int d = 0; d < 4; d++) {
    const uint32_t S = spread4((sg >> (4 * d)) & 15u), M = spread4((mg >> (4 * d)) & 15u);
    const uint32_t V = spread4((vb >> (4 * d)) & 15u) * 0xFFu;
    // bytes 1 or 3; negated where the sign is set: ~x + 1 per byte (0xFE + 1, 0xFC + 1: no carry leaves a byte)
    o[d] = (int)((((0x01010101u + 2u * M) ^ (S * 0xFFu)) + S) & V);
  }
  return o;
}

// columns 32 s + 16 h .. + 15 of a packed row (nw halves per row)
__device__ __forceinline__ i32x4 codes_row_frag(const uint32_t *__restrict__ B, long long row, int nw, int s, int h, uint32_t vb) {
  const uint32_t *p = B + row * nw + 4 * (s >> 1) + (s & 1);
  return codes_unpack16((p[0] >> (16 * h)) & 0xFFFFu, (p[2] >> (16 * h)) & 0xFFFFu, vb);
}

// The additive score of a (question, row) pair from the three integers J_i (include/word2bits_eval.h, "codes mode"):
//   p_i = (float)J_i * w(b_i),  score = ((p2 - p1) + p3) * w(c)
// one rounding per operation.  The scan's epilogue and the one-lane-per-question kernel that scores a given row ahead of the
// rank scan both call these two, so that the two floats of one pair are the same bits.
__device__ __forceinline__ float codes_term(int j, float w) { return __fmul_rn((float)j, w); }
__device__ __forceinline__ float codes_add_score(float p1, float p2, float p3, float wc) {
  return __fmul_rn(__fadd_rn(__fsub_rn(p2, p1), p3), wc);
}

__device__ __forceinline__ unsigned long long codes_key(float d, int c) {
  return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)c);
}

}  // namespace
