// w2b_kernels_evalclasses.hip -- word classes by spherical k-means on bit-packed rows (include/word2bits_eval.h, "word
// classes"): which of K centroids is nearest to every row, and what are the rows of every class summed?
//
// Assign.  k_cls_assign is the float-vector scan of w2b_kernels_evalvec.hip with the operand roles swapped.  For
// v_mfma_f32_32x32x2_f32 lane l supplies A[i = l % 32][k = l / 32] and B[k = l / 32][j = l % 32] and receives D[i][j = l % 32]
// for 16 values of i.  The CENTROIDS are the A operand: (float)T_k[a], exact because |T| <= 3 * words < 2^24, in memory in
// fragment order (k_cls_operands: per pair of 32-class tiles and group of 8 columns 2 x 64 float4, lane l of tile t holds
// T[class 32 t + l % 32][columns 8 g + 2 i + l / 32], i = 0 .. 3; +0 for a column >= size or a class >= K, and one zero group
// behind the last pair for the last prefetch).  The ROW is the B operand, decoded from the lane's packed words with integer
// operations exactly as the vector scan decodes it (the sign bit or-ed into 1.0f, at 2 bits into 1.0f or 3.0f).  The zeros
// are REQUIRED: the padding bits of a packed row decode to t = +1, and fmaf(+0, t, acc) == acc for every acc this chain can
// hold.  An accumulator is the chain  acc = +0; acc = fmaf((float)T_k[a], (float)t_c[a], acc)  in column order.
// So a lane owns ONE vocabulary row (l % 32) and 16 of a tile's 32 classes: accumulator e of a tile is class 8 (e / 4) + 4
// (l / 32) + e % 4.  The argmax over the classes is a running (d, k) pair in registers, walked in ascending k over all class
// tiles -- a later class replaces the held one only if its d is greater -- and ONE exchange with lane l ^ 32 at the end, the
// lower k winning on equal d, finishes it: no merge across workgroups, no selection scratch, no K x V matrix in memory.
// A class >= K or a dead one is skipped by its bit in `live`, never by its score (a zero score beats every negative one);
// a row past the vocabulary is dropped by its row number.  The grid is over rows only, VR = 2 row tiles per wavefront,
// because every wavefront must see every class tile.  Regimes as in the vector scan: size <= 512 keeps the packed words of
// the rows in registers for all class tiles, a longer row is walked in chunks of 512 columns that are loaded again for
// every pair of class tiles; the empty asm statement keeps the compiler from decoding the words once for all pairs.
//
// Sums.  Exact integers, so nothing depends on scheduling: a counting sort of the rows by class (k_cls_hist, k_cls_scan,
// k_cls_scatter: integer atomics, the order inside a class does not matter), then k_cls_pool walks the sorted rows in
// segments of 256, lane = column, row id uniform in the wavefront, counting sign / magnitude / both bits as the bag pooling
// of w2b_kernels_embed.hip does, and adds a segment's partial sum of a class to T with int32 atomics.  k_cls_norm sums
// T^2 into N_k (int64); the host turns N into wq and the live bits.
#include "w2b_evalclasses.h"

namespace {

constexpr int CT = 256;        // threads of a workgroup: four wavefronts
constexpr int CROWS = 32;      // rows of a tile
constexpr int VR = 2;          // 32-row tiles of a wavefront
constexpr int VQ = 2;          // 32-class tiles scored at a time
constexpr int VW = 8;          // 64-column blocks whose packed words a lane keeps in registers
constexpr int PSEG = 256;      // sorted rows that one workgroup pools
constexpr int SCAN_T = 1024;   // threads of the scan workgroup

typedef float vf32x16 __attribute__((ext_vector_type(16)));
typedef float cf32x4 __attribute__((ext_vector_type(4)));

inline long long cls_pairs(long long K) { return (K + 32 * VQ - 1) / (32 * VQ); }
inline long long cls_operand_slots(int dim, long long K) { return cls_pairs(K) * ((dim + 7) / 8) * (VQ * 64) + VQ * 64; }

__global__ void k_cls_hist(const int *__restrict__ cl, int words, int *__restrict__ hist) {
  const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (c < words) atomicAdd(hist + cl[c], 1);
}

// one workgroup: start[k] = the members of the classes below k (start[K] = words), cursor = start, counts = hist
__global__ void __launch_bounds__(SCAN_T) k_cls_scan(const int *__restrict__ hist, int K, int *__restrict__ start,
                                                     int *__restrict__ cursor, long long *__restrict__ counts) {
  __shared__ int part[SCAN_T];
  const int per = (K + SCAN_T - 1) / SCAN_T, k0 = (int)threadIdx.x * per, k1 = min(K, k0 + per);
  int sum = 0;
  for (int k = k0; k < k1; k++) sum += hist[k];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < SCAN_T; d <<= 1) {
    const int add = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  int at = part[threadIdx.x] - sum;
  for (int k = k0; k < k1; k++) {
    start[k] = at;
    cursor[k] = at;
    counts[k] = hist[k];
    at += hist[k];
  }
  if (threadIdx.x == SCAN_T - 1) start[K] = part[SCAN_T - 1];
}

__global__ void k_cls_scatter(const int *__restrict__ cl, int words, int *__restrict__ cursor, int *__restrict__ order) {
  const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (c < words) order[atomicAdd(cursor + cl[c], 1)] = c;
}

// B32 = the packed rows as 32-bit halves, nh per row.  Workgroup b pools order[b * PSEG ..): wavefront w the column blocks
// w, w + 4, ..; the rows of one class are one run of the sorted order, and a run's partial sum is added to T when it ends.
template <int BL>
__global__ void __launch_bounds__(CT) k_cls_pool(const uint32_t *__restrict__ B32, int nh, int words, int dim,
                                                 const int *__restrict__ order, const int *__restrict__ cl,
                                                 int *__restrict__ T) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, bit = lane & 31;
  const int p0 = (int)blockIdx.x * PSEG, p1 = min(words, p0 + PSEG);
  const int cbs = (dim + 63) >> 6;
  for (int cb = wave; cb < cbs; cb += CT / 64) {
    const int col = cb * 64 + lane;
    const int hs = cb * BL * 2 + (lane >> 5);       // the half of the sign word that holds this column; magnitude: 2 further
    int A = 0, Bm = 0, Cb = 0, m = 0, cur = -1;     // sign bits, magnitude bits, both, rows of the run; its class
    auto flush = [&]() {
      if (cur >= 0 && col < dim) {
        const int total = BL == 1 ? m - 2 * A : m + 2 * Bm - 2 * A - 4 * Cb;
        atomicAdd(T + (long long)cur * dim + col, total);
      }
      A = Bm = Cb = m = 0;
    };
    for (int q0 = p0; q0 < p1; q0 += 64) {
      const int cnt = min(64, p1 - q0);
      int myrow = 0, mycls = -1;
      if (lane < cnt) {
        myrow = order[q0 + lane];
        mycls = cl[myrow];
      }
      for (int j = 0; j < cnt; j++) {
        const int row = __builtin_amdgcn_readlane(myrow, j), k = __builtin_amdgcn_readlane(mycls, j);
        if (k != cur) {
          flush();
          cur = k;
        }
        const uint32_t *pw = B32 + (long long)row * nh + hs;
        const int sg = (int)((pw[0] >> bit) & 1u);
        A += sg;
        m++;
        if constexpr (BL == 2) {
          const int mg = (int)((pw[2] >> bit) & 1u);
          Bm += mg;
          Cb += sg & mg;
        }
      }
    }
    flush();
  }
}

// one wavefront per class: N[k] = sum_a T[k][a]^2
__global__ void __launch_bounds__(CT) k_cls_norm(const int *__restrict__ T, int K, int dim, long long *__restrict__ N) {
  const int k = (int)blockIdx.x * (CT / 64) + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= K) return;
  long long n = 0;
  for (int a = lane; a < dim; a += 64) {
    const long long t = T[(long long)k * dim + a];
    n += t * t;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(n & 0xFFFFFFFFll), d);
    const int hi = __shfl_xor((int)(n >> 32), d);
    n += ((long long)hi << 32) | (long long)lo;
  }
  if (lane == 0) N[k] = n;
}

// The centroid operands in fragment order, X[((pair * ng + g) * VQ + t) * 64 + lane] (float4): class (pair * VQ + t) * 32 +
// lane % 32, columns 8 g + 2 i + lane / 32 in element i; +0 where the column or the class does not exist, and in the VQ * 64
// slots behind the last pair.  Every slot is written.
__global__ void k_cls_operands(const int *__restrict__ T, int dim, int ng, int K, long long n_main, cf32x4 *__restrict__ X) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_main + VQ * 64; i += stride) {
    cf32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (i < n_main) {
      const int lane = (int)(i & 63), t = (int)((i >> 6) % VQ), g = (int)((i / (64 * VQ)) % ng);
      const long long pair = i / (64ll * VQ * ng), k = (pair * VQ + t) * 32 + (lane & 31);
      if (k < K) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int col = 8 * g + 2 * j + (lane >> 5);
          if (col < dim) o[j] = (float)T[k * dim + col];
        }
      }
    }
    X[i] = o;
  }
}

// B = the packed rows, [words][BL * nb] 64-bit words (nb = ceil(size / 64)); X = the centroid operands, ng = ceil(size / 8)
// groups per pair, cpairs pairs of class tiles; wq [64 * cpairs]; live [2 * cpairs], bit b of word ct = class 32 ct + b.
template <int BL>
__global__ void __launch_bounds__(CT, 2)
k_cls_assign(const uint64_t *__restrict__ B, int nb, int words, const cf32x4 *__restrict__ X, const float *__restrict__ wq,
             const uint32_t *__restrict__ live, int ng, int cpairs, const int *__restrict__ cl, int *__restrict__ cl_new,
             float *__restrict__ score, unsigned long long *__restrict__ moved) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l32 = lane & 31, h = lane >> 5;
  const int r0 = (((int)blockIdx.x * 4 + wave) * VR) * CROWS;
  if (r0 >= words) return;                        // (no barrier in this kernel)
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

  const cf32x4 *p = X + lane;
  cf32x4 bq[2][VQ];                               // [0]: the group about to be multiplied, [1]: the one requested behind it
#pragma unroll
  for (int t = 0; t < VQ; t++) bq[0][t] = p[64 * t];

  float bd[VR];                                   // the best d so far among this lane's classes, and its class (-1: none yet)
  int bk[VR];
#pragma unroll
  for (int r = 0; r < VR; r++) bd[r] = 0.f, bk[r] = -1;

  for (int pr = 0; pr < cpairs; pr++) {
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
          // the next group of this stream (behind the last pair: zeros) into the other half of bq: no copies
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
                acc[r][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[j & 1][t][i], a[r], acc[r][t], 0, 0, 0);
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

    // Accumulator e of tile (r, t) in lane l: class 32 (pr VQ + t) + 8 (e / 4) + 4 (l / 32) + e % 4, row r0 + 32 r + l % 32.
    // For a fixed lane e ascending is class ascending, and so are t and pr.
#pragma unroll
    for (int t = 0; t < VQ; t++) {
      const int ct = pr * VQ + t;
      const uint32_t lm = live[ct];                 // (the same in every lane)
      if (lm == 0u) continue;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const cf32x4 wc = *(const cf32x4 *)(wq + ct * 32 + 8 * g + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int e = 4 * g + i, kb = 8 * g + 4 * h + i;
          if ((lm >> kb) & 1u) {
#pragma unroll
            for (int r = 0; r < VR; r++) {
              const float d = __fmul_rn(acc[r][t][e], wc[i]);
              if (bk[r] < 0 || d > bd[r]) {
                bd[r] = d;
                bk[r] = ct * 32 + kb;
              }
            }
          }
        }
      }
    }
  }

  int nmoved = 0;
#pragma unroll
  for (int r = 0; r < VR; r++) {
    const float od = __shfl_xor(bd[r], 32);
    const int ok = __shfl_xor(bk[r], 32);
    if (ok >= 0 && (bk[r] < 0 || od > bd[r] || (od == bd[r] && ok < bk[r]))) {
      bd[r] = od;
      bk[r] = ok;
    }
    if (bk[r] < 0) {                                // no live class at all
      bk[r] = 0;
      bd[r] = 0.f;
    }
    const int row = r0 + r * CROWS + l32;
    bool mv = false;
    if (h == 0 && row < words) {
      mv = cl[row] != bk[r];
      cl_new[row] = bk[r];
      score[row] = bd[r];
    }
    nmoved += (int)__popcll(__ballot(mv));
  }
  if (lane == 0 && nmoved > 0) atomicAdd(moved, (unsigned long long)nmoved);
}

}  // namespace

long long w2b_cls_class_slots(int K) { return cls_pairs(K) * (32 * VQ); }
size_t w2b_cls_operand_bytes(int dim, int K) { return (size_t)cls_operand_slots(dim, K) * 16; }

hipError_t w2b_launch_cls_sums(const uint64_t *B, int words, int dim, int bitlevel, int K, const int *cl, int *hist, int *start,
                               int *cursor, int *order, int *T, long long *counts, long long *N, void *X, hipStream_t s) {
  if (words <= 0 || K <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)K * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(T, 0, (size_t)K * (size_t)dim * 4, s);
  if (e != hipSuccess) return e;
  const int rb = (words + 255) / 256;
  hipLaunchKernelGGL(k_cls_hist, dim3(rb), dim3(256), 0, s, cl, words, hist);
  hipLaunchKernelGGL(k_cls_scan, dim3(1), dim3(SCAN_T), 0, s, hist, K, start, cursor, counts);
  hipLaunchKernelGGL(k_cls_scatter, dim3(rb), dim3(256), 0, s, cl, words, cursor, order);
  const int nh = 2 * bitlevel * ((dim + 63) / 64), pb = (words + PSEG - 1) / PSEG;
  if (bitlevel == 2)
    hipLaunchKernelGGL(k_cls_pool<2>, dim3(pb), dim3(CT), 0, s, (const uint32_t *)B, nh, words, dim, order, cl, T);
  else
    hipLaunchKernelGGL(k_cls_pool<1>, dim3(pb), dim3(CT), 0, s, (const uint32_t *)B, nh, words, dim, order, cl, T);
  hipLaunchKernelGGL(k_cls_norm, dim3((K + CT / 64 - 1) / (CT / 64)), dim3(CT), 0, s, T, K, dim, N);
  const long long n = cls_operand_slots(dim, K);
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(k_cls_operands, dim3(blocks), dim3(256), 0, s, T, dim, (dim + 7) / 8, K, n - VQ * 64, (cf32x4 *)X);
  return hipGetLastError();
}

hipError_t w2b_launch_cls_assign(const uint64_t *B, int words, int dim, int bitlevel, int K, const void *X, const float *wq,
                                 const uint32_t *live, const int *cl, int *cl_new, float *score, unsigned long long *moved,
                                 hipStream_t s) {
  if (words <= 0 || K <= 0) return hipSuccess;
  const int nb = (dim + 63) / 64, ng = (dim + 7) / 8, cpairs = (int)cls_pairs(K);
  const int gx = (words + 4 * VR * CROWS - 1) / (4 * VR * CROWS);
  if (bitlevel == 2)
    hipLaunchKernelGGL(k_cls_assign<2>, dim3(gx), dim3(CT), 0, s, B, nb, words, (const cf32x4 *)X, wq, live, ng, cpairs, cl,
                       cl_new, score, moved);
  else
    hipLaunchKernelGGL(k_cls_assign<1>, dim3(gx), dim3(CT), 0, s, B, nb, words, (const cf32x4 *)X, wq, live, ng, cpairs, cl,
                       cl_new, score, moved);
  return hipGetLastError();
}
