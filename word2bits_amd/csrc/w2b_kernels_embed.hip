// w2b_kernels_embed.hip -- the packed embedding layer (include/word2bits_embed.h): row lookup and bag pooling straight
// from the bit-packed table, [rows][wpr] 64-bit words in the .w2bp layout (per 64 columns a SIGN word and, at bitlevel 2,
// a MAGNITUDE word; include/word2bits_corpus.h).  ids / offsets are int64 in library-owned device buffers; nothing they
// hold makes a kernel touch memory outside its buffers: an id is used as a row only when 0 <= id < rows, a bag's bounds
// are clamped into [0, n_ids], and what had to be ignored or clamped is counted in *bad.
//
// Lookup (k_embed_lookup): bound by its own output -- dim x 4 (x 2) bytes written per id against dim / 8 (dim / 4) read.
// The output [n][dim] is dense, so it is cut into 16-byte chunks of the FLAT element index: one lane = one chunk = 4
// float32 or 8 16-bit columns, one 16-byte store, a wavefront instruction stores 1 KiB whatever dim is.  A chunk that
// lies inside one row and one 64-column block (every chunk when dim is a multiple of 64) loads its id and its packed
// word(s) once and shifts the bits out; a chunk that straddles rows or blocks (dim = 1, 3, 65, 200 x 2 B ...) walks its
// elements one by one; the last chunk of the output may be partial and is stored element by element.  Every value is
// put together from the bits with integer operations: the float patterns are exact by construction.
// Index arithmetic: the chunk number, row x words-per-row and the output offset are 64-bit (both the table and the
// output may exceed 4 GiB); a workgroup divides its first element by dim once, a lane only its small offset (32-bit).
//
// Bag (k_embed_bag, k_embed_bag_long, k_embed_bag_finish): integer accumulators per column.  A wavefront owns 64-column
// blocks (lane = column); the id is wave-uniform, so the lanes of a half wave read the same 32-bit half of the packed
// word (a broadcast) and add its bit: per column the counts A = #sign, B = #magnitude, C = #(sign & magnitude) over the
// m valid ids, and T = m - 2A at bitlevel 1, T = m + 2B - 2A - 4C at bitlevel 2 (t = (1 + 2 mag)(1 - 2 sign)).
// The four waves of a workgroup take different column blocks of the same bag (16 blocks = 1024 columns per pass).
// Bags of at most W2B_EMBED_SPLIT ids are finished by their workgroup.  A longer bag is put on a list instead; its
// segments of W2B_EMBED_SPLIT ids are spread over all workgroups of a second launch, which add their partial T (and m)
// into int32 scratch with integer atomics -- integer adds commute, so the result does not depend on the split -- and a
// third launch converts.  The multiply, the divide and the conversion happen once per output element, after the last add.
// Weighted bags (k_embed_bagw*): float chains in a fixed order instead of counts; see the comment above them.
#include <hip/hip_fp16.h>

#include "../../include/word2bits_embed.h"
#include "w2b_internal.h"

namespace {

constexpr int kLookupThreads = 256, kLookupUnroll = 4;     // chunks per workgroup = 1024
constexpr int kBagThreads = 256, kBagWaves = 4, kBagK = 4; // column blocks per wave and pass; 16 per workgroup

// one value of the table in the output format, from its sign and magnitude bit (integer operations only)
template <int BL, int DT>
__device__ __forceinline__ uint32_t embed_value(uint32_t s, uint32_t m) {
  if constexpr (DT == W2B_EMBED_F32) return (BL == 1 ? 0x3EAAAAABu : 0x3E800000u + m * 0x00C00000u) | (s << 31);
  else if constexpr (DT == W2B_EMBED_BF16) return (BL == 1 ? 0x3EABu : 0x3E80u + m * 0xC0u) | (s << 15);
  else return (BL == 1 ? 0x3555u : 0x3400u + m * 0x600u) | (s << 15);
}

template <int BL, int DT>
__global__ __launch_bounds__(kLookupThreads) void k_embed_lookup(const uint64_t *__restrict__ T, long long rows, int dim,
                                                                 int wpr, const long long *__restrict__ ids, long long n,
                                                                 void *__restrict__ out, unsigned long long *bad) {
  constexpr int E = DT == W2B_EMBED_F32 ? 4 : 8;            // elements of a 16-byte chunk
  constexpr int ES = 16 / E;
  const long long tot = n * dim;                           // elements of the output
  const long long g0 = (long long)blockIdx.x * (kLookupThreads * kLookupUnroll);
  const long long e0 = g0 * E;
  if (e0 >= tot) return;
  const long long row0 = e0 / dim;                         // uniform: once per workgroup
  const unsigned col0 = (unsigned)(e0 - row0 * dim);
#pragma unroll
  for (int u = 0; u < kLookupUnroll; u++) {
    const unsigned local = (unsigned)(threadIdx.x + u * kLookupThreads);
    const long long g = g0 + local;
    const long long e = g * E;
    if (e >= tot) break;
    const unsigned x = col0 + local * E;                    // < 2^24 + 8192
    const unsigned dr = x / (unsigned)dim;
    unsigned col = x - dr * (unsigned)dim;
    long long row = row0 + dr;
    uint32_t v[E];
    const bool whole = e + E <= tot;
    if (whole && col + E <= (unsigned)dim && (col & 63u) + E <= 64u) {
      // the chunk lies in one row and one 64-column block: one id, one sign word (and one magnitude word)
      const long long id = ids[row];
      const bool ok = id >= 0 && id < rows;
      if (col == 0 && id >= rows) atomicAdd(bad, 1ull);
      uint32_t sb = 0, mb = 0;
      if (ok) {
        const uint64_t *w = T + id * (long long)wpr + (long long)(col >> 6) * BL;
        sb = (uint32_t)(w[0] >> (col & 63u));
        if constexpr (BL == 2) mb = (uint32_t)(w[1] >> (col & 63u));
      }
#pragma unroll
      for (int j = 0; j < E; j++) v[j] = ok ? embed_value<BL, DT>((sb >> j) & 1u, (mb >> j) & 1u) : 0u;
    } else {
      // head / tail path: the chunk crosses a row end or a block end, or is the partial last one
      long long id = -1;
      bool have = false;
#pragma unroll
      for (int j = 0; j < E; j++) {
        v[j] = 0u;
        if (e + j < tot) {
          if (col >= (unsigned)dim) { col = 0; row++; have = false; }
          if (!have) {
            id = ids[row];
            have = true;
          }
          if (col == 0 && id >= rows) atomicAdd(bad, 1ull);
          if (id >= 0 && id < rows) {
            const uint64_t *w = T + id * (long long)wpr + (long long)(col >> 6) * BL;
            const uint32_t s = (uint32_t)(w[0] >> (col & 63u)) & 1u;
            uint32_t m = 0;
            if constexpr (BL == 2) m = (uint32_t)(w[1] >> (col & 63u)) & 1u;
            v[j] = embed_value<BL, DT>(s, m);
          }
          col++;
        }
      }
    }
    if (whole) {
      uint4 q;
      if constexpr (E == 4) q = make_uint4(v[0], v[1], v[2], v[3]);
      else q = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
      *reinterpret_cast<uint4 *>(reinterpret_cast<char *>(out) + g * 16) = q;
    } else {
      for (int j = 0; j < E && e + j < tot; j++) {
        if constexpr (ES == 4) reinterpret_cast<uint32_t *>(out)[e + j] = v[j];
        else reinterpret_cast<uint16_t *>(out)[e + j] = (uint16_t)v[j];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- bags
// scratch of one bag launch: header (16 ints, [0] = long bags listed), list[cap] (bag index), cnt[cap] (m), acc[cap][dim]
struct BagScratch {
  int *nlong, *list, *cnt, *acc;
  int cap;
};
__host__ __device__ inline BagScratch bag_scratch(void *p, int cap, int dim) {
  BagScratch s;
  s.nlong = (int *)p;
  s.list = s.nlong + 16;
  s.cnt = s.list + cap;
  s.acc = s.cnt + cap;
  s.cap = cap;
  (void)dim;
  return s;
}

// bounds of bag b as the kernels use them; returns whether they had to be changed
__device__ __forceinline__ bool bag_bounds(const long long *__restrict__ offsets, long long b, long long n_ids, long long *start,
                                           long long *end) {
  const long long o0 = offsets[b], o1 = offsets[b + 1];
  long long s = o0 < 0 ? 0 : (o0 > n_ids ? n_ids : o0);
  long long t = o1 < 0 ? 0 : (o1 > n_ids ? n_ids : o1);
  if (t < s) t = s;
  bool changed = s != o0 || t != o1;
  if (t - s > W2B_EMBED_MAX_BAG) { t = s + W2B_EMBED_MAX_BAG; changed = true; }
  *start = s;
  *end = t;
  return changed;
}

// the column blocks of one wave in one pass, and their counts
template <int BL>
struct BagCols {
  int h[kBagK];            // 32-bit half of the sign word that this lane reads (the magnitude half is 2 further)
  int A[kBagK], B[kBagK], C[kBagK];
  int nk;                  // column blocks in use (uniform)
  int m;                   // valid ids seen
};

// ids[start .. end) of one bag (or segment) into the counts of `c`; count_bad: this wave reports the ids >= rows
template <int BL>
__device__ __forceinline__ void bag_walk(const uint32_t *__restrict__ B32, long long nh, long long rows,
                                         const long long *__restrict__ ids, long long start, long long end, int lane,
                                         BagCols<BL> &c, bool count_bad, unsigned long long *bad) {
  const int bit = lane & 31;
  int nbad = 0;
  for (long long i0 = start; i0 < end; i0 += 64) {
    const long long raw = i0 + lane < end ? ids[i0 + lane] : -1;
    const bool isbad = raw >= rows, ok = raw >= 0 && !isbad;
    c.m += (int)__popcll(__ballot(ok));
    nbad += (int)__popcll(__ballot(isbad));
    const int myid = ok ? (int)raw : -1;
    const int cnt = end - i0 < 64 ? (int)(end - i0) : 64;
    for (int j = 0; j < cnt; j += 4) {                     // j + 3 <= 63; lanes past the end hold -1
      const uint32_t *rowp[4];
      uint32_t msk[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int id = __builtin_amdgcn_readlane(myid, j + u);
        msk[u] = id >= 0 ? ~0u : 0u;
        rowp[u] = B32 + (long long)(id >= 0 ? id : 0) * nh;
      }
#pragma unroll
      for (int k = 0; k < kBagK; k++) {
        if (k < c.nk) {
          uint32_t sw[4], mw[4];
#pragma unroll
          for (int u = 0; u < 4; u++) {
            sw[u] = rowp[u][c.h[k]] & msk[u];
            if constexpr (BL == 2) mw[u] = rowp[u][c.h[k] + 2] & msk[u];
          }
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int s = (int)((sw[u] >> bit) & 1u);
            c.A[k] += s;
            if constexpr (BL == 2) {
              const int g = (int)((mw[u] >> bit) & 1u);
              c.B[k] += g;
              c.C[k] += s & g;
            }
          }
        }
      }
    }
  }
  if (count_bad && nbad > 0 && lane == 0) atomicAdd(bad, (unsigned long long)nbad);
}

// the column blocks cg * 16 + wave + 4 k of this wave, counts zeroed
template <int BL>
__device__ __forceinline__ void bag_cols_init(BagCols<BL> &c, int cg, int wave, int lane, int cbs) {
  c.nk = 0;
  c.m = 0;
#pragma unroll
  for (int k = 0; k < kBagK; k++) {
    const int cb = cg * (kBagWaves * kBagK) + wave + kBagWaves * k;
    if (cb < cbs) c.nk = k + 1;
    c.h[k] = (cb < cbs ? cb : 0) * BL * 2 + (lane >> 5);
    c.A[k] = c.B[k] = c.C[k] = 0;
  }
}
template <int BL>
__device__ __forceinline__ int bag_total(const BagCols<BL> &c, int k) {
  if constexpr (BL == 1) return c.m - 2 * c.A[k];
  else return c.m + 2 * c.B[k] - 2 * c.A[k] - 4 * c.C[k];
}

// T (the integer sum, exact as a float, or the weighted sum S), m -> the output element: one multiply, one division,
// one conversion
__device__ __forceinline__ void bag_store(void *out, long long idx, float T, int m, int bitlevel, int mode, int dtype) {
  const float q = bitlevel == 1 ? __uint_as_float(0x3EAAAAABu) : 0.25f;
  float r = __fmul_rn(T, q);
  if (mode == W2B_EMBED_MEAN) r = m > 0 ? __fdiv_rn(r, (float)m) : 0.f;
  if (dtype == W2B_EMBED_F32) {
    reinterpret_cast<float *>(out)[idx] = r;
  } else if (dtype == W2B_EMBED_BF16) {
    const uint32_t u = __float_as_uint(r);
    reinterpret_cast<uint16_t *>(out)[idx] = (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
  } else {
    reinterpret_cast<uint16_t *>(out)[idx] = __half_as_ushort(__float2half_rn(r));
  }
}

template <int BL>
__global__ __launch_bounds__(kBagThreads) void k_embed_bag(const uint32_t *__restrict__ B32, long long nh, long long rows, int dim,
                                                           const long long *__restrict__ ids, long long n_ids,
                                                           const long long *__restrict__ offsets, long long n_bags, int mode,
                                                           int dtype, void *__restrict__ out, unsigned long long *bad,
                                                           void *scratch, int cap) {
  __shared__ int slot_s;
  const BagScratch S = bag_scratch(scratch, cap, dim);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cbs = (dim + 63) >> 6;
  for (long long b = blockIdx.x; b < n_bags; b += gridDim.x) {
    long long start, end;
    const bool changed = bag_bounds(offsets, b, n_ids, &start, &end);
    if (changed && threadIdx.x == 0) atomicAdd(bad, 1ull);
    if (end - start > W2B_EMBED_SPLIT) {
      __syncthreads();                                       // (the previous bag's readers of slot_s are done)
      if (threadIdx.x == 0) {
        slot_s = atomicAdd(S.nlong, 1);
        if (slot_s < cap) S.list[slot_s] = (int)b;
      }
      __syncthreads();
      if (slot_s < cap) continue;                            // k_embed_bag_long pools it
    }                                                        // (a full list: pooled here, by this workgroup alone)
    for (int cg = 0; cg * (kBagWaves * kBagK) < cbs; cg++) {
      BagCols<BL> c;
      bag_cols_init(c, cg, wave, lane, cbs);
      bag_walk<BL>(B32, nh, rows, ids, start, end, lane, c, wave == 0 && cg == 0, bad);
#pragma unroll
      for (int k = 0; k < kBagK; k++) {
        const int col = (cg * (kBagWaves * kBagK) + wave + kBagWaves * k) * 64 + lane;
        if (k < c.nk && col < dim) bag_store(out, b * (long long)dim + col, (float)bag_total(c, k), c.m, BL, mode, dtype);
      }
    }
  }
}

// the listed long bags: segment s of bag j goes to workgroup (j + s) mod gridDim.x
template <int BL>
__global__ __launch_bounds__(kBagThreads) void k_embed_bag_long(const uint32_t *__restrict__ B32, long long nh, long long rows,
                                                                int dim, const long long *__restrict__ ids, long long n_ids,
                                                                const long long *__restrict__ offsets,
                                                                unsigned long long *bad, void *scratch, int cap) {
  const BagScratch S = bag_scratch(scratch, cap, dim);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cbs = (dim + 63) >> 6;
  const int nl = *S.nlong < cap ? *S.nlong : cap;
  const int G = (int)gridDim.x;
  for (int j = 0; j < nl; j++) {
    long long start, end;
    bag_bounds(offsets, S.list[j], n_ids, &start, &end);
    const long long nseg = (end - start + W2B_EMBED_SPLIT - 1) / W2B_EMBED_SPLIT;
    for (long long s = ((int)blockIdx.x - j % G + G) % G; s < nseg; s += G) {
      const long long s0 = start + s * W2B_EMBED_SPLIT;
      const long long s1 = s0 + W2B_EMBED_SPLIT < end ? s0 + W2B_EMBED_SPLIT : end;
      for (int cg = 0; cg * (kBagWaves * kBagK) < cbs; cg++) {
        BagCols<BL> c;
        bag_cols_init(c, cg, wave, lane, cbs);
        bag_walk<BL>(B32, nh, rows, ids, s0, s1, lane, c, wave == 0 && cg == 0, bad);
#pragma unroll
        for (int k = 0; k < kBagK; k++) {
          const int col = (cg * (kBagWaves * kBagK) + wave + kBagWaves * k) * 64 + lane;
          if (k < c.nk && col < dim) atomicAdd(S.acc + (long long)j * dim + col, bag_total(c, k));
        }
        if (wave == 0 && cg == 0 && lane == 0) atomicAdd(S.cnt + j, c.m);
      }
    }
  }
}

__global__ __launch_bounds__(kBagThreads) void k_embed_bag_finish(int dim, int bitlevel, int mode, int dtype, void *__restrict__ out,
                                                                  void *scratch, int cap) {
  const BagScratch S = bag_scratch(scratch, cap, dim);
  const int nl = *S.nlong < cap ? *S.nlong : cap;
  for (int j = blockIdx.x; j < nl; j += gridDim.x) {
    const long long b = S.list[j];
    const int m = S.cnt[j];
    for (int col = threadIdx.x; col < dim; col += blockDim.x)
      bag_store(out, b * (long long)dim + col, (float)S.acc[(long long)j * dim + col], m, bitlevel, mode, dtype);
  }
}

// ---------------------------------------------------------------------------------------------------- weighted bags
// (k_embed_bagw, k_embed_bagw_long, k_embed_bagw_finish; the semantics are in the header.)  A float sum has an order, so
// these kernels keep ONE chain per (bag, column) where the integer kernels count bits: the layout of bag_walk carries over
// (a wavefront owns 64-column blocks, lane = column, the four waves take different blocks, ids and weights are
// wave-uniform), and per id and column the code t is put together as a float pattern with integer operations and goes
// into one __fmaf_rn -- at bitlevel 1, t = +-1, that is a sign flip of w and one add, the same value.  kBagK column chains
// per lane are independent of each other and hide the latency of the dependent adds.  A padding, ignored or missing id
// takes the weight +0 (and row 0): fmaf(+0, t, P) = P for every P these chains can hold (P is never -0: it starts at +0
// and x + (-x) = +0), so no branch is needed.
// The bag's positions are cut into segments of W2B_EMBED_WSEG; P_s of a segment starts at +0 and the bag's S adds the
// P_s in order.  A bag of at most one segment is finished by its workgroup.  A longer bag is listed with a range of
// rows in the float scratch part[segments][dim]; the second launch spreads the segments over all workgroups, each
// stores its P_s there with plain vector stores (m goes through an integer atomic: integer adds commute), and the
// third adds them in segment order, one thread per column.  There is no float atomic.  A bag that finds the list or
// the scratch full is walked segment by segment by its own workgroup: the same operations in the same order.
struct BagWScratch {
  int *head, *list, *base, *cnt;      // head[0] = long bags listed, head[2..3] = segment rows handed out (64 bits)
  float *part;
  int cap;
  long long segcap;
};
__host__ __device__ inline BagWScratch bagw_scratch(void *p, int cap, long long segcap) {
  BagWScratch s;
  s.head = (int *)p;
  s.list = s.head + 16;
  s.base = s.list + cap;
  s.cnt = s.base + cap;
  s.part = (float *)(s.cnt + cap);
  s.cap = cap;
  s.segcap = segcap;
  return s;
}

// a weight the host form accepts: finite, and 0 or 2^-60 <= |w| <= 2^60 (on the bits: NaN and inf lie above 2^60)
__host__ __device__ inline bool bagw_weight_ok(uint32_t bits) {
  const uint32_t a = bits & 0x7FFFFFFFu;
  return a == 0u || (a >= 0x21800000u && a <= 0x5D800000u);
}

template <int BL>
struct BagWCols {
  int h[kBagK];            // as BagCols
  float P[kBagK];          // the chain of the current segment
  int nk, m;
};
template <int BL>
__device__ __forceinline__ void bagw_cols_init(BagWCols<BL> &c, int cg, int wave, int lane, int cbs) {
  c.nk = 0;
  c.m = 0;
#pragma unroll
  for (int k = 0; k < kBagK; k++) {
    const int cb = cg * (kBagWaves * kBagK) + wave + kBagWaves * k;
    if (cb < cbs) c.nk = k + 1;
    c.h[k] = (cb < cbs ? cb : 0) * BL * 2 + (lane >> 5);
    c.P[k] = 0.f;
  }
}

// positions [start, end) of one segment, in order, onto the chains c.P (which the caller has set to +0)
template <int BL>
__device__ __forceinline__ void bagw_walk(const uint32_t *__restrict__ B32, long long nh, long long rows,
                                          const long long *__restrict__ ids, const float *__restrict__ weights,
                                          long long start, long long end, int lane, BagWCols<BL> &c, bool count_bad,
                                          unsigned long long *bad) {
  const int bit = lane & 31;
  int nbad = 0;
  for (long long i0 = start; i0 < end; i0 += 64) {
    const bool in = i0 + lane < end;
    const long long raw = in ? ids[i0 + lane] : -1;
    const uint32_t wraw = in ? __float_as_uint(weights[i0 + lane]) : 0u;
    const bool isbad = raw >= rows || (raw >= 0 && !bagw_weight_ok(wraw)), ok = raw >= 0 && !isbad;
    c.m += (int)__popcll(__ballot(ok));
    nbad += (int)__popcll(__ballot(isbad));
    const int myid = ok ? (int)raw : 0;
    const int myw = ok ? (int)wraw : 0;
    const int cnt = end - i0 < 64 ? (int)(end - i0) : 64;
    for (int j = 0; j < cnt; j += 4) {                     // j + 3 <= 63; lanes past the end hold row 0, weight +0
      const uint32_t *rowp[4];
      uint32_t w[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        rowp[u] = B32 + (long long)__builtin_amdgcn_readlane(myid, j + u) * nh;
        w[u] = (uint32_t)__builtin_amdgcn_readlane(myw, j + u);
      }
#pragma unroll
      for (int k = 0; k < kBagK; k++) {
        if (k < c.nk) {
          uint32_t sw[4], mw[4];
#pragma unroll
          for (int u = 0; u < 4; u++) {
            sw[u] = rowp[u][c.h[k]];
            if constexpr (BL == 2) mw[u] = rowp[u][c.h[k] + 2];
          }
#pragma unroll
          for (int u = 0; u < 4; u++) {                     // in the order of the ids: one chain
            const uint32_t s = (sw[u] >> bit) & 1u;
            if constexpr (BL == 1) {
              c.P[k] = __fadd_rn(c.P[k], __uint_as_float(w[u] ^ (s << 31)));                    // = fmaf(w, +-1, P)
            } else {
              const uint32_t t = (0x3F800000u + ((mw[u] >> bit) & 1u) * 0x00C00000u) | (s << 31);   // +-1.0f, +-3.0f
              c.P[k] = __fmaf_rn(__uint_as_float(w[u]), __uint_as_float(t), c.P[k]);
            }
          }
        }
      }
    }
  }
  if (count_bad && nbad > 0 && lane == 0) atomicAdd(bad, (unsigned long long)nbad);
}

template <int BL>
__global__ __launch_bounds__(kBagThreads) void k_embed_bagw(const uint32_t *__restrict__ B32, long long nh, long long rows, int dim,
                                                            const long long *__restrict__ ids,
                                                            const float *__restrict__ weights, long long n_ids,
                                                            const long long *__restrict__ offsets, long long n_bags, int mode,
                                                            int dtype, void *__restrict__ out, unsigned long long *bad,
                                                            void *scratch, int cap, long long segcap) {
  __shared__ int listed_s;
  const BagWScratch S = bagw_scratch(scratch, cap, segcap);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cbs = (dim + 63) >> 6;
  for (long long b = blockIdx.x; b < n_bags; b += gridDim.x) {
    long long start, end;
    const bool changed = bag_bounds(offsets, b, n_ids, &start, &end);
    if (changed && threadIdx.x == 0) atomicAdd(bad, 1ull);
    const long long nseg = (end - start + W2B_EMBED_WSEG - 1) / W2B_EMBED_WSEG;     // <= 4096
    if (nseg > 1) {
      __syncthreads();                                       // (the previous bag's readers of listed_s are done)
      if (threadIdx.x == 0) {
        listed_s = 0;
        const int slot = atomicAdd(S.head, 1);
        if (slot < cap) {
          const unsigned long long first = atomicAdd((unsigned long long *)(S.head + 2), (unsigned long long)nseg);
          listed_s = first + (unsigned long long)nseg <= (unsigned long long)segcap;
          S.base[slot] = listed_s ? (int)first : 0;
          S.list[slot] = listed_s ? (int)b : -1;             // -1: no rows left for it; pooled here
        }
      }
      __syncthreads();
      if (listed_s) continue;                                // k_embed_bagw_long pools it
    }
    for (int cg = 0; cg * (kBagWaves * kBagK) < cbs; cg++) {
      BagWCols<BL> c;
      bagw_cols_init(c, cg, wave, lane, cbs);
      float sum[kBagK];
#pragma unroll
      for (int k = 0; k < kBagK; k++) sum[k] = 0.f;
      for (long long s = 0; s < nseg; s++) {
        const long long s0 = start + s * W2B_EMBED_WSEG;
        const long long s1 = s0 + W2B_EMBED_WSEG < end ? s0 + W2B_EMBED_WSEG : end;
        bagw_walk<BL>(B32, nh, rows, ids, weights, s0, s1, lane, c, wave == 0 && cg == 0, bad);
#pragma unroll
        for (int k = 0; k < kBagK; k++) {
          sum[k] = __fadd_rn(sum[k], c.P[k]);
          c.P[k] = 0.f;
        }
      }
#pragma unroll
      for (int k = 0; k < kBagK; k++) {
        const int col = (cg * (kBagWaves * kBagK) + wave + kBagWaves * k) * 64 + lane;
        if (k < c.nk && col < dim) bag_store(out, b * (long long)dim + col, sum[k], c.m, BL, mode, dtype);
      }
    }
  }
}

// the listed long bags: segment s of bag j goes to workgroup (j + s) mod gridDim.x and to row base[j] + s of part
template <int BL>
__global__ __launch_bounds__(kBagThreads) void k_embed_bagw_long(const uint32_t *__restrict__ B32, long long nh, long long rows,
                                                                 int dim, const long long *__restrict__ ids,
                                                                 const float *__restrict__ weights, long long n_ids,
                                                                 const long long *__restrict__ offsets,
                                                                 unsigned long long *bad, void *scratch, int cap,
                                                                 long long segcap) {
  const BagWScratch S = bagw_scratch(scratch, cap, segcap);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cbs = (dim + 63) >> 6;
  const int nl = S.head[0] < cap ? S.head[0] : cap;
  const int G = (int)gridDim.x;
  for (int j = 0; j < nl; j++) {
    if (S.list[j] < 0) continue;
    long long start, end;
    bag_bounds(offsets, S.list[j], n_ids, &start, &end);
    const long long nseg = (end - start + W2B_EMBED_WSEG - 1) / W2B_EMBED_WSEG;
    const long long first = S.base[j];                       // first + nseg <= segcap, or the bag were not listed
    for (long long s = ((int)blockIdx.x - j % G + G) % G; s < nseg; s += G) {
      const long long s0 = start + s * W2B_EMBED_WSEG;
      const long long s1 = s0 + W2B_EMBED_WSEG < end ? s0 + W2B_EMBED_WSEG : end;
      for (int cg = 0; cg * (kBagWaves * kBagK) < cbs; cg++) {
        BagWCols<BL> c;
        bagw_cols_init(c, cg, wave, lane, cbs);
        bagw_walk<BL>(B32, nh, rows, ids, weights, s0, s1, lane, c, wave == 0 && cg == 0, bad);
#pragma unroll
        for (int k = 0; k < kBagK; k++) {
          const int col = (cg * (kBagWaves * kBagK) + wave + kBagWaves * k) * 64 + lane;
          if (k < c.nk && col < dim) S.part[(first + s) * dim + col] = c.P[k];
        }
        if (wave == 0 && cg == 0 && lane == 0) atomicAdd(S.cnt + j, c.m);
      }
    }
  }
}

// S = +0, + P_0, + P_1 ... in segment order, one thread per column; then the multiply, the division and the conversion
__global__ __launch_bounds__(kBagThreads) void k_embed_bagw_finish(int dim, int bitlevel, long long n_ids,
                                                                   const long long *__restrict__ offsets, int mode, int dtype,
                                                                   void *__restrict__ out, void *scratch, int cap,
                                                                   long long segcap) {
  const BagWScratch S = bagw_scratch(scratch, cap, segcap);
  const int nl = S.head[0] < cap ? S.head[0] : cap;
  const int chunks = (dim + kBagThreads - 1) / kBagThreads;
  for (long long w = blockIdx.x; w < (long long)nl * chunks; w += gridDim.x) {
    const int j = (int)(w / chunks), col = (int)(w % chunks) * kBagThreads + (int)threadIdx.x;
    if (S.list[j] < 0 || col >= dim) continue;
    const long long b = S.list[j];
    long long start, end;
    bag_bounds(offsets, b, n_ids, &start, &end);
    const long long nseg = (end - start + W2B_EMBED_WSEG - 1) / W2B_EMBED_WSEG;
    const float *p = S.part + (long long)S.base[j] * dim + col;
    float sum = 0.f;
    for (long long s = 0; s < nseg; s++) sum = __fadd_rn(sum, p[s * dim]);
    bag_store(out, b * (long long)dim + col, sum, S.cnt[j], bitlevel, mode, dtype);
  }
}

}  // namespace

hipError_t w2b_launch_embed_lookup(const uint64_t *T, long long rows, int dim, int bitlevel, const long long *ids, long long n,
                                   int dtype, void *out, unsigned long long *bad, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int E = dtype == W2B_EMBED_F32 ? 4 : 8;
  const long long chunks = (n * dim + E - 1) / E, per = kLookupThreads * kLookupUnroll;
  const long long grid = (chunks + per - 1) / per;
  if (grid > 0x7FFFFFFFll) return hipErrorInvalidValue;
  const int wpr = (dim + 63) / 64 * bitlevel;
#define W2B_LOOKUP(BL, DT) \
  hipLaunchKernelGGL((k_embed_lookup<BL, DT>), dim3((unsigned)grid), dim3(kLookupThreads), 0, s, T, rows, dim, wpr, ids, n, out, bad)
  if (bitlevel == 1) {
    if (dtype == W2B_EMBED_F32) W2B_LOOKUP(1, W2B_EMBED_F32);
    else if (dtype == W2B_EMBED_BF16) W2B_LOOKUP(1, W2B_EMBED_BF16);
    else W2B_LOOKUP(1, W2B_EMBED_F16);
  } else {
    if (dtype == W2B_EMBED_F32) W2B_LOOKUP(2, W2B_EMBED_F32);
    else if (dtype == W2B_EMBED_BF16) W2B_LOOKUP(2, W2B_EMBED_BF16);
    else W2B_LOOKUP(2, W2B_EMBED_F16);
  }
#undef W2B_LOOKUP
  return hipGetLastError();
}

// slots of the long-bag list: every bag longer than W2B_EMBED_SPLIT when the bags do not overlap (overlapping bounds can
// only come from a damaged offsets buffer; what does not fit the list is pooled by one workgroup, still correctly)
long long w2b_embed_bag_scratch(long long n_ids, long long n_bags, int dim, int *cap_out) {
  long long cap = n_ids / W2B_EMBED_SPLIT + 1;
  if (cap > n_bags) cap = n_bags;
  if (cap < 1) cap = 1;
  *cap_out = (int)cap;
  return (16 + 2 * cap + cap * (long long)dim) * 4;
}

hipError_t w2b_launch_embed_bag(const uint64_t *T, long long rows, int dim, int bitlevel, const long long *ids, long long n_ids,
                                const long long *offsets, long long n_bags, int mode, int dtype, void *out,
                                unsigned long long *bad, void *scratch, hipStream_t s) {
  if (n_bags <= 0) return hipSuccess;
  int cap = 0;
  const long long sbytes = w2b_embed_bag_scratch(n_ids, n_bags, dim, &cap);
  hipError_t he = hipMemsetAsync(scratch, 0, (size_t)sbytes, s);
  if (he != hipSuccess) return he;
  const uint32_t *B32 = (const uint32_t *)T;
  const long long nh = (long long)((dim + 63) / 64) * bitlevel * 2;
  const unsigned grid = (unsigned)(n_bags < (1ll << 22) ? n_bags : (1ll << 22));
  const unsigned glong = 2048, gfin = (unsigned)(cap < 4096 ? cap : 4096);
  if (bitlevel == 1) {
    hipLaunchKernelGGL(k_embed_bag<1>, dim3(grid), dim3(kBagThreads), 0, s, B32, nh, rows, dim, ids, n_ids, offsets, n_bags,
                       mode, dtype, out, bad, scratch, cap);
    if (n_ids > W2B_EMBED_SPLIT)
      hipLaunchKernelGGL(k_embed_bag_long<1>, dim3(glong), dim3(kBagThreads), 0, s, B32, nh, rows, dim, ids, n_ids, offsets, bad,
                         scratch, cap);
  } else {
    hipLaunchKernelGGL(k_embed_bag<2>, dim3(grid), dim3(kBagThreads), 0, s, B32, nh, rows, dim, ids, n_ids, offsets, n_bags,
                       mode, dtype, out, bad, scratch, cap);
    if (n_ids > W2B_EMBED_SPLIT)
      hipLaunchKernelGGL(k_embed_bag_long<2>, dim3(glong), dim3(kBagThreads), 0, s, B32, nh, rows, dim, ids, n_ids, offsets, bad,
                         scratch, cap);
  }
  if (n_ids > W2B_EMBED_SPLIT)
    hipLaunchKernelGGL(k_embed_bag_finish, dim3(gfin), dim3(kBagThreads), 0, s, dim, bitlevel, mode, dtype, out, scratch, cap);
  return hipGetLastError();
}

// weighted bags: `cap` list slots as above and `segcap` rows of part -- every segment of every long bag when the bags do
// not overlap (a bag of n ids has at most n / W2B_EMBED_WSEG + 1 segments)
long long w2b_embed_bagw_scratch(long long n_ids, long long n_bags, int dim, int *cap_out, long long *segcap_out,
                                 long long *head_bytes) {
  long long cap = n_ids / W2B_EMBED_WSEG + 1;
  if (cap > n_bags) cap = n_bags;
  if (cap < 1) cap = 1;
  const long long segcap = n_ids / W2B_EMBED_WSEG + cap;    // < 2^31: n_ids <= 2^40
  *cap_out = (int)cap;
  *segcap_out = segcap;
  *head_bytes = (16 + 3 * cap) * 4;
  return *head_bytes + segcap * (long long)dim * 4;
}

hipError_t w2b_launch_embed_bag_weighted(const uint64_t *T, long long rows, int dim, int bitlevel, const long long *ids,
                                         const float *weights, long long n_ids, const long long *offsets, long long n_bags,
                                         int mode, int dtype, void *out, unsigned long long *bad, void *scratch, hipStream_t s) {
  if (n_bags <= 0) return hipSuccess;
  int cap = 0;
  long long segcap = 0, head = 0;
  w2b_embed_bagw_scratch(n_ids, n_bags, dim, &cap, &segcap, &head);
  hipError_t he = hipMemsetAsync(scratch, 0, (size_t)head, s);      // the rows of part are stored whole before they are read
  if (he != hipSuccess) return he;
  const uint32_t *B32 = (const uint32_t *)T;
  const long long nh = (long long)((dim + 63) / 64) * bitlevel * 2;
  const unsigned grid = (unsigned)(n_bags < (1ll << 22) ? n_bags : (1ll << 22));
  const long long fin = (long long)cap * ((dim + kBagThreads - 1) / kBagThreads);
  const unsigned glong = 2048, gfin = (unsigned)(fin < 4096 ? fin : 4096);
  const bool longs = n_ids > W2B_EMBED_WSEG;
  if (bitlevel == 1) {
    hipLaunchKernelGGL(k_embed_bagw<1>, dim3(grid), dim3(kBagThreads), 0, s, B32, nh, rows, dim, ids, weights, n_ids, offsets,
                       n_bags, mode, dtype, out, bad, scratch, cap, segcap);
    if (longs)
      hipLaunchKernelGGL(k_embed_bagw_long<1>, dim3(glong), dim3(kBagThreads), 0, s, B32, nh, rows, dim, ids, weights, n_ids,
                         offsets, bad, scratch, cap, segcap);
  } else {
    hipLaunchKernelGGL(k_embed_bagw<2>, dim3(grid), dim3(kBagThreads), 0, s, B32, nh, rows, dim, ids, weights, n_ids, offsets,
                       n_bags, mode, dtype, out, bad, scratch, cap, segcap);
    if (longs)
      hipLaunchKernelGGL(k_embed_bagw_long<2>, dim3(glong), dim3(kBagThreads), 0, s, B32, nh, rows, dim, ids, weights, n_ids,
                         offsets, bad, scratch, cap, segcap);
  }
  if (longs)
    hipLaunchKernelGGL(k_embed_bagw_finish, dim3(gfin), dim3(kBagThreads), 0, s, dim, bitlevel, n_ids, offsets, mode, dtype, out,
                       scratch, cap, segcap);
  return hipGetLastError();
}
