// w2b_kernels_evalpairs.hip -- the evaluator's pair question on bit-packed rows (include/word2bits_eval.h, "pair similarity").
//
// A pair is two bags of rows.  Each side is pooled into the unnormalised integer vector T[a] = sum of t_r[a] over its ids >= 0
// (t = +-1 on 1-bit rows, +-1 / +-3 on 2-bit rows, |T[a]| <= 3 * 4096), and the device returns the three exact integers
//   J = sum_a T_A[a] * T_B[a],   N_A = sum_a T_A[a]^2,   N_B = sum_a T_B[a]^2      over the columns a < D,
// as int64 [pair][3].  The host builds the cosine from them; no float exists on the device.  Integer adds commute, so no split
// of the work changes a bit of the result, and every path below must agree with w2b_pairs_host.
//
// The pooling (pool_blocks): lane = column of one 64-column block; an id is wave-uniform, so the packed word of its row for that
// block is one load for the whole wavefront (sign and magnitude word together on 2-bit rows; hipcc proves the address uniform and
// emits scalar loads, so the vector memory path carries the ids alone).  A wavefront reads 64 ids with one coalesced load (a
// bag's first 64 once for all column blocks, the rest per block), takes them back one at a time with v_readlane and keeps
// PAIRS_U = 8 row loads in flight; padding ids (< 0) read row 0 and count nothing.  A lane counts set bits -- sign bits cs,
// magnitude bits cm, both cms -- and the valid ids nv (a scalar):
//   1-bit  T = nv - 2 cs          2-bit  T = nv - 2 cs + 2 cm - 4 cms        (t = (1 + 2 m) * (1 - 2 s))
// At the end of a block the lane adds T_A * T_B, T_A^2, T_B^2 (each below 12288^2 < 2^31) into three int64 accumulators; after
// its last block a wavefront sums them over its lanes with __shfl_xor and one lane stores them with plain stores.
// The padding bits of a row's last word are zero and would read as t = +1: every path zeroes T (or masks the word) in the
// columns >= D.
//
// Paths and their boundaries (w2b_pairs_path, which the host asks for every pair; `ids of a pair` = both bags, padding included):
//   ONE    both bags are exactly one id and that id is >= 0: one LANE per pair, popcounts over the two rows' words (k_pairs_one
//          has the formulas; 1-bit rows: J = D - 2 popcount((A xor B) & valid columns), N_A = N_B = D).  A bag [r, -1] is not on
//          this path.
//   SHORT  every other pair of at most W2B_PAIRS_LONG_IDS = 256 ids: one WAVEFRONT per pair, four pairs per workgroup; the
//          wavefront walks the column blocks in turn.  Pairs with an empty side, or no id at all, are here.
//   LONG   a pair of more than 256 ids: one WORKGROUP per pair; wavefront w pools the block pairs w, w + 4, w + 8, ..., the
//          four partial triples meet in LDS and thread 0 stores their sum.  With fewer than seven blocks (D <= 384) the
//          surplus wavefronts add zeros.
//   column blocks go two at a time: block pair u = the blocks 2 u and 2 u + 1, adjacent words of a row and so one wider load
//          per id; an odd number of blocks leaves a last single block (on the long path with wavefront (blocks / 2) % 4).
//          D = 650 has eleven blocks: wavefront 0 takes two pairs, wavefront 1 a pair and the single block.
//   inside the pooling: ids are taken in batches of 64 (bags of 64 / 65 ids: one / two batches) and in groups of 8.
#include "w2b_internal.h"

namespace {

constexpr int PAIRS_WG = 256;        // threads of a workgroup
constexpr int PAIRS_WAVES = 4;       // its wavefronts
constexpr int PAIRS_U = 8;           // row loads a wavefront keeps in flight

// T[k] of this lane's column in the NK consecutive blocks blk + k for the bag ids[lo .. hi); every argument but `lane` is
// wave-uniform.  `first` = the bag's first 64 ids, one per lane (-1 past its end), which the caller loads once for all blocks
template <int BL, int NK>
__device__ __forceinline__ void pool_blocks(const uint64_t *__restrict__ B, long long wpr, int blk, const int *__restrict__ ids,
                                            int lo, int hi, int first, int lane, int (&T)[NK]) {
  const bool upper = lane >= 32;
  const int sh = lane & 31;
  int nv = 0;
  unsigned cs[NK], cm[NK], cms[NK];
#pragma unroll
  for (int k = 0; k < NK; k++) cs[k] = cm[k] = cms[k] = 0u;
  for (int i0 = lo; i0 < hi; i0 += 64) {
    const int idv = i0 == lo ? first : (i0 + lane < hi ? ids[i0 + lane] : -1);
    const int n = hi - i0 < 64 ? hi - i0 : 64;
    for (int j0 = 0; j0 < n; j0 += PAIRS_U) {      // (lanes n .. 63 hold -1: a group may run past n)
      uint64_t ws[PAIRS_U][NK], wm[PAIRS_U][NK];
      bool ok[PAIRS_U];
#pragma unroll
      for (int u = 0; u < PAIRS_U; u++) {
        const int id = __builtin_amdgcn_readlane(idv, j0 + u);
        ok[u] = id >= 0;
        const uint64_t *r = B + (long long)(ok[u] ? id : 0) * wpr + (long long)blk * BL;
#pragma unroll
        for (int k = 0; k < NK; k++) {             // (adjacent words of the row: one wide load)
          ws[u][k] = r[k * BL];
          wm[u][k] = BL == 2 ? r[k * BL + 1] : 0ull;
        }
      }
#pragma unroll
      for (int u = 0; u < PAIRS_U; u++) {
        nv += ok[u] ? 1 : 0;
#pragma unroll
        for (int k = 0; k < NK; k++) {
          const unsigned s = ((upper ? (unsigned)(ws[u][k] >> 32) : (unsigned)ws[u][k]) >> sh) & (ok[u] ? 1u : 0u);
          cs[k] += s;
          if constexpr (BL == 2) {
            const unsigned m = ((upper ? (unsigned)(wm[u][k] >> 32) : (unsigned)wm[u][k]) >> sh) & (ok[u] ? 1u : 0u);
            cm[k] += m;
            cms[k] += m & s;
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NK; k++) T[k] = nv - 2 * (int)cs[k] + 2 * (int)cm[k] - 4 * (int)cms[k];
}

struct Triple { long long j, na, nb; };
struct Bags { int a0, a1, b1, fa, fb; };   // a pair's bounds in ids and the first 64 ids of either bag

// adds the lane's share of the NK blocks blk + k to t
template <int BL, int NK>
__device__ __forceinline__ void add_blocks(const uint64_t *__restrict__ B, long long wpr, int dim, int blk,
                                           const int *__restrict__ ids, const Bags &g, int lane, Triple &t) {
  int ta[NK], tb[NK];
  pool_blocks<BL, NK>(B, wpr, blk, ids, g.a0, g.a1, g.fa, lane, ta);
  pool_blocks<BL, NK>(B, wpr, blk, ids, g.a1, g.b1, g.fb, lane, tb);
#pragma unroll
  for (int k = 0; k < NK; k++) {
    if ((blk + k) * 64 + lane >= dim) ta[k] = tb[k] = 0;      // the padding bits of the last word are no columns
    t.j += (long long)(ta[k] * tb[k]);
    t.na += (long long)(ta[k] * ta[k]);
    t.nb += (long long)(tb[k] * tb[k]);
  }
}

// the lane's share of (J, N_A, N_B) of pair q over the block pairs u0, u0 + ustep, ... (pair u = the blocks 2 u, 2 u + 1); a
// last odd block belongs to the share that the pair index nb / 2 would belong to
template <int BL>
__device__ __forceinline__ Triple pair_blocks(const uint64_t *__restrict__ B, int dim, const int *__restrict__ ids,
                                              const int *__restrict__ off, int q, int u0, int ustep, int lane) {
  const int nb = (dim + 63) / 64, npair = nb / 2;
  const long long wpr = (long long)nb * BL;
  Bags g;
  g.a0 = off[2 * q], g.a1 = off[2 * q + 1], g.b1 = off[2 * q + 2];
  g.fa = g.a0 + lane < g.a1 ? ids[g.a0 + lane] : -1;
  g.fb = g.a1 + lane < g.b1 ? ids[g.a1 + lane] : -1;
  Triple t{0, 0, 0};
  for (int u = u0; u < npair; u += ustep) add_blocks<BL, 2>(B, wpr, dim, 2 * u, ids, g, lane, t);
  if ((nb & 1) && npair % ustep == u0) add_blocks<BL, 1>(B, wpr, dim, nb - 1, ids, g, lane, t);
  return t;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// SHORT: list[0 .. n) = the pairs of this path; wavefront i takes pair list[i]
template <int BL>
__global__ void __launch_bounds__(PAIRS_WG)
k_pairs_short(const uint64_t *__restrict__ B, int dim, const int *__restrict__ ids, const int *__restrict__ off,
              const int *__restrict__ list, int n, long long *__restrict__ parts) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int i = (int)blockIdx.x * PAIRS_WAVES + wave;
  if (i >= n) return;                               // (no barrier in this kernel)
  const int q = list[i];
  Triple t = pair_blocks<BL>(B, dim, ids, off, q, 0, 1, lane);
  t.j = wave_sum(t.j);
  t.na = wave_sum(t.na);
  t.nb = wave_sum(t.nb);
  if (lane == 0) {
    parts[3ll * q] = t.j;
    parts[3ll * q + 1] = t.na;
    parts[3ll * q + 2] = t.nb;
  }
}

// LONG: workgroup i takes pair list[i]
template <int BL>
__global__ void __launch_bounds__(PAIRS_WG)
k_pairs_long(const uint64_t *__restrict__ B, int dim, const int *__restrict__ ids, const int *__restrict__ off,
             const int *__restrict__ list, long long *__restrict__ parts) {
  __shared__ long long red[PAIRS_WAVES][3];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int q = list[blockIdx.x];
  Triple t = pair_blocks<BL>(B, dim, ids, off, q, wave, PAIRS_WAVES, lane);
  t.j = wave_sum(t.j);
  t.na = wave_sum(t.na);
  t.nb = wave_sum(t.nb);
  if (lane == 0) {
    red[wave][0] = t.j;
    red[wave][1] = t.na;
    red[wave][2] = t.nb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 3; c++) parts[3ll * q + c] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
  }
}

// ONE: thread i takes pair list[i], whose two bags are one id >= 0 each.  Popcounts on whole words, v = the word's columns:
//   1-bit  J = D - 2 popcount((A xor B) & v),  N_A = N_B = D
//   2-bit  with s = sign_A xor sign_B, pos = ~s & v, neg = s & v and the magnitude words mA, mB:  t_A t_B = +-(1 + 2 mA)(1 + 2 mB)
//          J = c(1) + 2 c(mA) + 2 c(mB) + 4 c(mA & mB),  c(x) = popcount(pos & x) - popcount(neg & x);  N = D + 8 popcount(m & v)
template <int BL>
__global__ void __launch_bounds__(PAIRS_WG)
k_pairs_one(const uint64_t *__restrict__ B, int dim, const int *__restrict__ ids, const int *__restrict__ off,
            const int *__restrict__ list, int n, long long *__restrict__ parts) {
  const int i = (int)blockIdx.x * PAIRS_WG + (int)threadIdx.x;
  if (i >= n) return;
  const int q = list[i], nb = (dim + 63) / 64;
  const uint64_t *a = B + (long long)ids[off[2 * q]] * nb * BL, *b = B + (long long)ids[off[2 * q + 1]] * nb * BL;
  const uint64_t last = dim & 63 ? (1ull << (dim & 63)) - 1ull : ~0ull;      // the columns of the last word
  if constexpr (BL == 1) {
    int h = 0;
    for (int w = 0; w < nb; w++) h += __popcll((a[w] ^ b[w]) & (w == nb - 1 ? last : ~0ull));
    parts[3ll * q] = (long long)(dim - 2 * h);
    parts[3ll * q + 1] = (long long)dim;
    parts[3ll * q + 2] = (long long)dim;
  } else {
    int j = 0, ma3 = 0, mb3 = 0;
    for (int w = 0; w < nb; w++) {
      const uint64_t v = w == nb - 1 ? last : ~0ull;
      const uint64_t s = a[2 * w] ^ b[2 * w], pos = ~s & v, neg = s & v, ma = a[2 * w + 1], mb = b[2 * w + 1], mm = ma & mb;
      j += (__popcll(pos) - __popcll(neg)) + 2 * (__popcll(pos & ma) - __popcll(neg & ma)) +
           2 * (__popcll(pos & mb) - __popcll(neg & mb)) + 4 * (__popcll(pos & mm) - __popcll(neg & mm));
      ma3 += __popcll(ma & v);
      mb3 += __popcll(mb & v);
    }
    parts[3ll * q] = (long long)j;
    parts[3ll * q + 1] = (long long)dim + 8ll * ma3;
    parts[3ll * q + 2] = (long long)dim + 8ll * mb3;
  }
}

}  // namespace

int w2b_pairs_path(int bitlevel, const int *ids, long long a0, long long a1, long long b1) {
  if (a1 - a0 == 1 && b1 - a1 == 1 && ids[a0] >= 0 && ids[a1] >= 0) return W2B_PAIRS_PATH_ONE;
  return b1 - a0 > W2B_PAIRS_LONG_IDS ? W2B_PAIRS_PATH_LONG : W2B_PAIRS_PATH_SHORT;
}

hipError_t w2b_launch_pairs(const uint64_t *B, int dim, int bitlevel, const int *ids, const int *off, const int *list,
                            int n_one, int n_short, int n_long, long long *parts, hipStream_t s) {
  const int *l_short = list + n_one, *l_long = l_short + n_short;
  if (n_one > 0) {
    const dim3 grid((unsigned)((n_one + PAIRS_WG - 1) / PAIRS_WG));
    if (bitlevel == 2) hipLaunchKernelGGL(k_pairs_one<2>, grid, dim3(PAIRS_WG), 0, s, B, dim, ids, off, list, n_one, parts);
    else hipLaunchKernelGGL(k_pairs_one<1>, grid, dim3(PAIRS_WG), 0, s, B, dim, ids, off, list, n_one, parts);
    if (hipError_t e = hipGetLastError()) return e;
  }
  if (n_short > 0) {
    const dim3 grid((unsigned)((n_short + PAIRS_WAVES - 1) / PAIRS_WAVES));
    if (bitlevel == 2) hipLaunchKernelGGL(k_pairs_short<2>, grid, dim3(PAIRS_WG), 0, s, B, dim, ids, off, l_short, n_short, parts);
    else hipLaunchKernelGGL(k_pairs_short<1>, grid, dim3(PAIRS_WG), 0, s, B, dim, ids, off, l_short, n_short, parts);
    if (hipError_t e = hipGetLastError()) return e;
  }
  if (n_long > 0) {
    if (bitlevel == 2) hipLaunchKernelGGL(k_pairs_long<2>, dim3((unsigned)n_long), dim3(PAIRS_WG), 0, s, B, dim, ids, off, l_long, parts);
    else hipLaunchKernelGGL(k_pairs_long<1>, dim3((unsigned)n_long), dim3(PAIRS_WG), 0, s, B, dim, ids, off, l_long, parts);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}
