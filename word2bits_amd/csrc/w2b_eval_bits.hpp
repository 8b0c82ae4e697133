// w2b_eval_bits.hpp -- what the scans on bit-packed 1-bit rows share (w2b_kernels_evalbits.hip: the three-row question,
// w2b_kernels_evalcombine.hip: the signed sum of up to seven rows): the workgroup sizes that w2b_bits_layout plans for,
// the result key and the choice of a kernel instance by row length.  Device code.
#pragma once
#include "w2b_internal.h"

#include <type_traits>

namespace {

constexpr int BT1 = 256;   // lanes (questions) per workgroup, top-1
constexpr int BTK = 128;   // ... top-k: k * BTK keys of 8 bytes in LDS, 64 KiB at k = 64

// c = the score of a row that agrees with the question everywhere, acc = what the disagreements take off (I = c - 2 acc)
__device__ __forceinline__ unsigned long long bits_key(uint32_t c, uint32_t acc, int row) {
  return ((unsigned long long)(c - 2 * acc) << 32) | (uint32_t)~row;      // I > 0: orders like the fp32 path's key
}

// the kernel instance for a row of `nw` 32-bit halves: registers up to MAXNW halves, memory (instance 0) beyond
template <int MAXNW, typename F>
hipError_t dispatch_nw(int nw, F &&f) {
  switch (nw) {
#define W2B_NW(n) case n: if constexpr (n <= MAXNW) return f(std::integral_constant<int, n>()); else break;
    W2B_NW(2) W2B_NW(4) W2B_NW(6) W2B_NW(8) W2B_NW(10) W2B_NW(12) W2B_NW(14) W2B_NW(16)
    W2B_NW(18) W2B_NW(20) W2B_NW(22) W2B_NW(24) W2B_NW(26) W2B_NW(28) W2B_NW(30) W2B_NW(32)
#undef W2B_NW
    default: break;
  }
  return f(std::integral_constant<int, 0>());
}

}  // namespace
