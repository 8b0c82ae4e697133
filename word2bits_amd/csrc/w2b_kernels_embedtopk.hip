// w2b_kernels_embedtopk.hip -- the k largest logits per vector of the packed embedding's tied output layer
// (include/word2bits_embed.h, "Top-k") without the [n][m] logits ever being held: the K loop of k_embed_project
// (w2b_embedproj_body.hpp, the same text, so the same logits bit for bit) with two more epilogues, which select.
//
// Keys.  A live logit at candidate position j becomes the 64-bit key  map(float32 bits) << 32 | ~j,  map the order-preserving
// integer map of the header (w2b_topk_map, w2b_embed_shared.h).  Larger key = larger logit, equal logits = lower position first.
// Keys are unique (the position is in them) and never 0; 0 stands for "no key": a dead lane (padding, refused, past m).
// In the accumulator layout the 32 lanes of a half wave hold the 64 candidates of a wavefront for ONE vector, two per lane.
// That is a UNIT: unit u = candidate positions 64 u .. 64 u + 63.  Four kernels per range of vectors, no race that decides
// anything and no float atomics:
//   1. k_topk_unitmax: the K loop; per (vector, unit) the largest key, by five shuffles within the half wave; one store per
//      (vector, unit), 0 for a unit without a live position.
//   2. k_topk_threshold: one wavefront per vector: T = the k-th largest of its units' maxima, 0 if fewer than k units have one.
//      The k best keys of the vector are all >= T (k keys >= T exist: those maxima), and since keys are unique exactly k units
//      have a maximum >= T: at most 64 k keys are >= T, in those units.  With T = 0 every live key counts: fewer than k units.
//   3. k_topk_collect: the K loop once more -- the same instructions on the same operands, so the same keys --; every key >= T
//      is appended to the vector's list.  A half wave reserves its places with ONE integer atomicAdd on the vector's counter
//      (ballot and prefix counts give each lane its place); the ORDER of a list depends on the order in which units arrive,
//      its CONTENT does not.  The list holds 64 k keys, which is the most there can be; a place beyond it is never written.
//   4. k_topk_merge: one wavefront per vector: every lane walks its share of the list for its largest key, the wavefront takes
//      the maximum of the 64, writes it, and the lane that held it looks for its next one below; k times.  Lists end in
//      pos = -1, val = -inf when the keys run out.  With no unit at all (m == 0) that is the whole output.
// The K loop runs twice.  What that buys: the scratch is ceil(m / 64) maxima and 64 k keys per vector, the lists are short
// (k keys and what ties with or lies among the k-th unit's other candidates), and nothing depends on timing.
#include "../../include/word2bits_embed.h"
#include "w2b_internal.h"
#define W2B_EMBED_SHARED_DEVICE
#include "w2b_embed_shared.h"
#include "w2b_embedproj_body.hpp"

namespace {

using namespace w2b_proj;

static_assert(PR * 32 == W2B_TOPK_UNIT, "a unit is the candidates of one wavefront of the projection");

// this lane's two keys for accumulator (t, e): 0 for a dead lane, whose row operand decoded as +1 throughout and whose
// accumulator is therefore not zero
__device__ __forceinline__ void lane_keys(const pf32x16 (&acc)[PR][PV], int t, int e, const bool (&live)[PR], float q, int jl,
                                          unsigned long long &key0, unsigned long long &key1) {
  key0 = key1 = 0ull;
  if (live[0]) key0 = w2b_topk_key(__float_as_uint(__fmul_rn(acc[0][t][e], q)), (uint32_t)jl);
  if (live[1]) key1 = w2b_topk_key(__float_as_uint(__fmul_rn(acc[1][t][e], q)), (uint32_t)(jl + 1));
}

struct UnitMaxEpilogue {
  static constexpr bool kAllWaves = false;          // no barrier: a wavefront past m has no unit and leaves
  int v0, v1, nunits;                               // the launch's vectors v0 .. v1 (indices into the operand staging)
  unsigned long long *__restrict__ umax;            // [v1 - v0][nunits]
  __device__ __forceinline__ void operator()(const pf32x16 (&acc)[PR][PV], int pr, int j0, int l32, int h, const bool (&live)[PR],
                                             float q) const {
    int jl = j0 + 2 * l32;
    asm volatile("" : "+v"(jl));
    const int unit = j0 / W2B_TOPK_UNIT;
#pragma unroll
    for (int t = 0; t < PV; t++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int v = (pr * PV + t) * 32 + 8 * (e >> 2) + 4 * h + (e & 3);
        unsigned long long key0, key1;
        lane_keys(acc, t, e, live, q, jl, key0, key1);
        unsigned long long top = key0 > key1 ? key0 : key1;
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) {         // within the half wave
          const unsigned long long o = __shfl_xor(top, d);
          top = o > top ? o : top;
        }
        if (l32 == 0 && v >= v0 && v < v1) umax[(long long)(v - v0) * nunits + unit] = top;
      }
  }
};

struct CollectEpilogue {
  static constexpr bool kAllWaves = false;
  int v0, v1, cap;                                  // cap = 64 k: the places of a vector's list
  const unsigned long long *__restrict__ thr;       // [v1 - v0]
  unsigned int *__restrict__ count;                 // [v1 - v0], zeroed by k_topk_threshold
  unsigned long long *__restrict__ list;            // [v1 - v0][cap]
  __device__ __forceinline__ void operator()(const pf32x16 (&acc)[PR][PV], int pr, int j0, int l32, int h, const bool (&live)[PR],
                                             float q) const {
    int jl = j0 + 2 * l32;
    asm volatile("" : "+v"(jl));
    const unsigned int below = (1u << l32) - 1u;
#pragma unroll
    for (int t = 0; t < PV; t++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int v = (pr * PV + t) * 32 + 8 * (e >> 2) + 4 * h + (e & 3);
        const bool mine = v >= v0 && v < v1;
        unsigned long long key0, key1;
        lane_keys(acc, t, e, live, q, jl, key0, key1);
        unsigned long long T = ~0ull;
        if (mine) T = thr[v - v0];
        const bool p0 = mine && key0 != 0ull && key0 >= T, p1 = mine && key1 != 0ull && key1 >= T;
        const unsigned int m0 = (unsigned int)(__ballot(p0) >> (32 * h)), m1 = (unsigned int)(__ballot(p1) >> (32 * h));
        const int passed = __popc(m0) + __popc(m1);
        if (__any(passed > 0)) {                      // (uniform: the whole wavefront takes part in the broadcast)
          unsigned int base = 0u;
          if (l32 == 0 && passed > 0) base = atomicAdd(count + (v - v0), (unsigned int)passed);
          base = __shfl(base, h << 5);
          const unsigned int at = base + __popc(m0 & below) + __popc(m1 & below);
          unsigned long long *mylist = list + (long long)(v - v0) * cap;
          if (p0 && at < (unsigned int)cap) mylist[at] = key0;
          if (p1 && at + (p0 ? 1u : 0u) < (unsigned int)cap) mylist[at + (p0 ? 1u : 0u)] = key1;
        }
      }
  }
};

template <int BL>
__global__ void __launch_bounds__(PT, 2)
k_topk_unitmax(const uint64_t *__restrict__ T, int nb, long long rows, const long long *__restrict__ cand, int m,
               const pf32x4 *__restrict__ X, int ng, int v0, int v1, int pairs_per_y, int nunits,
               unsigned long long *__restrict__ umax) {
  UnitMaxEpilogue epi{v0, v1, nunits, umax};
  embed_project_body<BL>(T, nb, rows, cand, 0ll, m, X, ng, v0 / (32 * PV), (v1 + 32 * PV - 1) / (32 * PV), pairs_per_y, false,
                         nullptr, epi);
}

template <int BL>
__global__ void __launch_bounds__(PT, 2)
k_topk_collect(const uint64_t *__restrict__ T, int nb, long long rows, const long long *__restrict__ cand, int m,
               const pf32x4 *__restrict__ X, int ng, int v0, int v1, int pairs_per_y, int cap,
               const unsigned long long *__restrict__ thr, unsigned int *__restrict__ count, unsigned long long *__restrict__ list) {
  CollectEpilogue epi{v0, v1, cap, thr, count, list};
  embed_project_body<BL>(T, nb, rows, cand, 0ll, m, X, ng, v0 / (32 * PV), (v1 + 32 * PV - 1) / (32 * PV), pairs_per_y, false,
                         nullptr, epi);
}

// the largest key (`first`), or the largest below `under`, among keys[lane], keys[lane + 64], ... below len; 0 if there is none
__device__ __forceinline__ unsigned long long next_key(const unsigned long long *__restrict__ keys, int len, int lane, bool first,
                                                       unsigned long long under) {
  unsigned long long best = 0ull;
  for (int i = lane; i < len; i += 64) {
    const unsigned long long key = keys[i];
    if ((first || key < under) && key > best) best = key;
  }
  return best;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long top) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(top, d);
    top = o > top ? o : top;
  }
  return top;
}

// one wavefront per vector of the range: thr = the k-th largest of its nunits maxima (0: fewer than k are not 0); count = 0
__global__ void __launch_bounds__(64)
k_topk_threshold(int nv, int k, int nunits, const unsigned long long *__restrict__ umax, unsigned long long *__restrict__ thr,
                 unsigned int *__restrict__ count) {
  const int v = (int)blockIdx.x, lane = threadIdx.x;
  if (v >= nv) return;
  umax += (long long)v * nunits;
  unsigned long long own = next_key(umax, nunits, lane, true, 0ull), top = 0ull;
  for (int i = 0; i < k; i++) {
    top = wave_max(own);
    if (top == 0ull) break;                         // (uniform)
    if (own == top && i + 1 < k) own = next_key(umax, nunits, lane, false, top);
  }
  if (lane == 0) {
    thr[v] = top;
    count[v] = 0u;
  }
}

// one wavefront per vector v0 .. v1; vals / pos = [n][k] of the call
__global__ void __launch_bounds__(64)
k_topk_merge(int v0, int v1, int k, int cap, const unsigned int *__restrict__ count, const unsigned long long *__restrict__ list,
             float *__restrict__ vals, long long *__restrict__ pos) {
  const int v = v0 + (int)blockIdx.x, lane = threadIdx.x;
  if (v >= v1) return;
  const int len = min((int)count[v - v0], cap);
  list += (long long)(v - v0) * cap;
  unsigned long long own = next_key(list, len, lane, true, 0ull);
  for (int i = 0; i < k; i++) {
    const unsigned long long top = wave_max(own);
    if (lane == 0) {
      vals[(long long)v * k + i] = __uint_as_float(top ? w2b_topk_unmap((uint32_t)(top >> 32)) : 0xFF800000u);
      pos[(long long)v * k + i] = top ? (long long)(~(uint32_t)top) : -1ll;
    }
    if (top == 0ull) continue;                      // (uniform: the keys have run out, the rest of the list is empty)
    if (own == top) own = next_key(list, len, lane, false, top);
  }
}

// candidate groups x ranges of the pairs that hold vectors v0 .. v1, as w2b_launch_embed_project cuts them
void topk_grid(int m, int v0, int v1, dim3 *grid, int *per_y) {
  const int pairs = (v1 + 32 * PV - 1) / (32 * PV) - v0 / (32 * PV);
  const int gx = (int)(((long long)m + 4 * PR * 32 - 1) / (4 * PR * 32));
  int gy = (PWG + gx - 1) / gx;
  if (gy > pairs) gy = pairs;
  *per_y = (pairs + gy - 1) / gy;
  gy = (pairs + *per_y - 1) / *per_y;
  *grid = dim3((unsigned)gx, (unsigned)gy);
}

}  // namespace

hipError_t w2b_launch_embed_topk(const uint64_t *T, long long rows, int dim, int bitlevel, const void *X, int v0, int v1,
                                 const long long *clean, int m, int k, unsigned long long *umax, unsigned long long *thr,
                                 unsigned int *count, unsigned long long *list, float *vals, long long *pos, hipStream_t s) {
  if (v1 <= v0) return hipSuccess;
  const int nb = (dim + 63) / 64, ng = (dim + 7) / 8, nunits = (int)(((long long)m + W2B_TOPK_UNIT - 1) / W2B_TOPK_UNIT);
  const int cap = W2B_TOPK_UNIT * k;
  dim3 grid;
  int per_y = 1;
  if (m > 0) {
    topk_grid(m, v0, v1, &grid, &per_y);
    if (bitlevel == 2)
      hipLaunchKernelGGL(k_topk_unitmax<2>, grid, dim3(PT), 0, s, T, nb, rows, clean, m, (const pf32x4 *)X, ng, v0, v1, per_y, nunits, umax);
    else
      hipLaunchKernelGGL(k_topk_unitmax<1>, grid, dim3(PT), 0, s, T, nb, rows, clean, m, (const pf32x4 *)X, ng, v0, v1, per_y, nunits, umax);
    if (hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(k_topk_threshold, dim3((unsigned)(v1 - v0)), dim3(64), 0, s, v1 - v0, k, nunits, umax, thr, count);
  if (hipError_t e = hipGetLastError()) return e;
  if (m > 0) {
    if (bitlevel == 2)
      hipLaunchKernelGGL(k_topk_collect<2>, grid, dim3(PT), 0, s, T, nb, rows, clean, m, (const pf32x4 *)X, ng, v0, v1, per_y, cap, thr,
                         count, list);
    else
      hipLaunchKernelGGL(k_topk_collect<1>, grid, dim3(PT), 0, s, T, nb, rows, clean, m, (const pf32x4 *)X, ng, v0, v1, per_y, cap, thr,
                         count, list);
    if (hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)(v1 - v0)), dim3(64), 0, s, v0, v1, k, cap, count, list, vals, pos);
  return hipGetLastError();
}
