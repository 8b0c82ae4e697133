// w2b_kernels_embedxent.hip -- softmax cross-entropy of the packed embedding's tied output layer (include/word2bits_embed.h,
// "Cross-entropy") without the [n][m] logits ever being held: the K loop of k_embed_project (w2b_embedproj_body.hpp, the same
// text, so the same logits bit for bit) with two other epilogues.
//
// Statistics (k_xent_stats).  A workgroup of the projection holds W2B_EMBED_XSEG = 256 candidates in its accumulators: four
// wavefronts x 64.  That is one SEGMENT of the header, blockIdx.x its number.  Per pair of vector tiles the epilogue reduces,
// for each of the pair's 64 vectors, the segment's logits instead of storing them: in the accumulator layout the 32 lanes of
// a half wave hold 64 candidates of ONE vector (two per lane), so the maximum over the live ones goes across those lanes by
// shuffles and across the four wavefronts through LDS; then every lane forms its integer terms rint(expneg(l - M_s) 2^32)
// and their sum goes the same way.  Integer adds commute: the split over lanes and wavefronts does not show in U_s.  One
// store of M_s and one of U_s per (vector, segment), into a scratch laid out [segment][vector] so that both this store and
// the finishing kernel's reads are contiguous.  The lane that owns target[i] stores tl[i].  Dead lanes (padding, refused,
// past m) take part in neither reduction: -inf in the maximum, nothing in the sum.  No atomics in the reductions.
// Finishing (k_xent_finish).  One thread per vector: mx = the maximum of M_s over the live segments (U_s != 0: a live
// segment's maximum contributes 2^32), se by the strictly sequential fmaf of the header, the target checked (>= m, or on a
// dead position: the vector is ignored and counted once), tl = +0 for an ignored vector, and the effective target (-1 =
// ignored) for the gradient kernel.
// Gradient (k_xent_grad).  The K loop once more; the epilogue turns each logit into g = expneg(l - mx) / se (- 1 at the
// target; +0 at dead positions and for ignored vectors) and stores it dense, as k_embed_project stores logits, for the
// vectors v0 .. v1 of the launch x a range of candidate positions.  The driver (w2b_embed.cpp) then runs the back-projection
// (w2b_kernels_embedback.hip) on that scratch.
// The arithmetic of expneg, the terms, the se step and g is w2b_embed_shared.h: the text the host twin compiles.
#include "../../include/word2bits_embed.h"
#include "w2b_internal.h"
#define W2B_EMBED_SHARED_DEVICE
#include "w2b_embed_shared.h"
#include "w2b_embedproj_body.hpp"

namespace {

using namespace w2b_proj;

static_assert(W2B_EMBED_XSEG == 4 * PR * 32, "a segment is the candidates of one workgroup of the projection");

// candidates for the launches of a call: ids >= rows become padding and are counted once each
__global__ void k_xent_clean(const long long *__restrict__ cand, long long m, long long rows, long long *__restrict__ clean,
                             unsigned long long *bad) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const long long id = cand[j];
  if (id >= rows) atomicAdd(bad, 1ull);
  clean[j] = id >= rows ? -1ll : id;
}

struct StatsEpilogue {
  static constexpr bool kAllWaves = true;           // the reductions go through LDS: two barriers and one more per pair
  int m, v0, v1;                                    // the launch's vectors v0 .. v1 (indices into the operand staging)
  const long long *__restrict__ target;             // [n]
  float *__restrict__ Mseg;                         // [nseg][v1 - v0]
  unsigned long long *__restrict__ Useg;
  float *__restrict__ tl;                           // [n]
  float (*smax)[64];                                // LDS [4][64]: per wavefront and vector of the pair
  unsigned long long (*ssum)[64];
  __device__ __forceinline__ void operator()(const pf32x16 (&acc)[PR][PV], int pr, int j0, int l32, int h, const bool (&live)[PR],
                                             float q) const {
    const int wave = threadIdx.x >> 6, jl = j0 + 2 * l32;
    const float ninf = __uint_as_float(0xFF800000u);
    // the maximum over the segment's live positions, per vector
#pragma unroll
    for (int t = 0; t < PV; t++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int vi = 32 * t + 8 * (e >> 2) + 4 * h + (e & 3), v = pr * (32 * PV) + vi;
        const float l0 = live[0] ? __fmul_rn(acc[0][t][e], q) : ninf;
        const float l1 = live[1] ? __fmul_rn(acc[1][t][e], q) : ninf;
        if (v >= v0 && v < v1) {
          const long long tg = target[v];
          if (live[0] && tg == jl) tl[v] = l0;
          if (live[1] && tg == jl + 1) tl[v] = l1;
        }
        float mxl = fmaxf(l0, l1);
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) mxl = fmaxf(mxl, __shfl_xor(mxl, d));      // within the half wave
        if (l32 == 0) smax[wave][vi] = mxl;
      }
    __syncthreads();
    // the integer sum of the terms
#pragma unroll
    for (int t = 0; t < PV; t++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int vi = 32 * t + 8 * (e >> 2) + 4 * h + (e & 3);
        const float M = fmaxf(fmaxf(smax[0][vi], smax[1][vi]), fmaxf(smax[2][vi], smax[3][vi]));
        unsigned long long u = 0ull;
        if (live[0]) u += w2b_xent_term(__fmul_rn(acc[0][t][e], q), M);
        if (live[1]) u += w2b_xent_term(__fmul_rn(acc[1][t][e], q), M);
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) u += __shfl_xor(u, d);
        if (l32 == 0) ssum[wave][vi] = u;
      }
    __syncthreads();
    if (threadIdx.x < 64) {
      const int vi = threadIdx.x, v = pr * (32 * PV) + vi;
      if (v >= v0 && v < v1) {
        const long long at = (long long)blockIdx.x * (v1 - v0) + (v - v0);
        const unsigned long long U = ssum[0][vi] + ssum[1][vi] + ssum[2][vi] + ssum[3][vi];
        Mseg[at] = U ? fmaxf(fmaxf(smax[0][vi], smax[1][vi]), fmaxf(smax[2][vi], smax[3][vi])) : 0.f;
        Useg[at] = U;                               // 0: the segment has no live position and does not take part
      }
    }
    __syncthreads();                                // the next pair writes smax / ssum again
  }
};

template <int BL>
__global__ void __launch_bounds__(PT, 2)
k_xent_stats(const uint64_t *__restrict__ T, int nb, long long rows, const long long *__restrict__ cand, int m,
             const pf32x4 *__restrict__ X, int ng, int v0, int v1, int pairs_per_y, const long long *__restrict__ target,
             float *__restrict__ Mseg, unsigned long long *__restrict__ Useg, float *__restrict__ tl) {
  __shared__ float smax[4][64];
  __shared__ unsigned long long ssum[4][64];
  StatsEpilogue epi{m, v0, v1, target, Mseg, Useg, tl, smax, ssum};
  embed_project_body<BL>(T, nb, rows, cand, 0ll, m, X, ng, v0 / (32 * PV), (v1 + 32 * PV - 1) / (32 * PV), pairs_per_y, false,
                         nullptr, epi);
}

// vectors v0 .. v1; Mseg / Useg = [nseg][v1 - v0]; clean = the call's candidates (nullptr: every row, m == rows)
__global__ void k_xent_finish(int v0, int v1, long long m, int nseg, const float *__restrict__ Mseg,
                              const unsigned long long *__restrict__ Useg, const long long *__restrict__ clean,
                              const long long *__restrict__ target, float *__restrict__ mx, float *__restrict__ se,
                              float *__restrict__ tl, long long *__restrict__ teff, unsigned long long *bad) {
  const int v = v0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (v >= v1) return;
  const long long ld = v1 - v0, at = v - v0;
  bool any = false;
  float top = 0.f;
  for (int s = 0; s < nseg; s++)
    if (Useg[s * ld + at]) {
      const float M = Mseg[s * ld + at];
      if (!any || M > top) top = M;
      any = true;
    }
  float sum = 0.f;
  for (int s = 0; s < nseg; s++) {
    const unsigned long long U = Useg[s * ld + at];
    if (U) sum = w2b_xent_se_step(U, Mseg[s * ld + at], top, sum);
  }
  mx[v] = any ? top : 0.f;
  se[v] = sum;
  long long tg = target[v];
  if (tg >= 0) {
    bool ok = tg < m;
    if (ok && clean) ok = clean[tg] >= 0;
    if (!ok) {
      atomicAdd(bad, 1ull);
      tg = -1;
    }
  }
  if (tg < 0) tg = -1, tl[v] = 0.f;
  teff[v] = tg;
}

struct GradEpilogue {
  static constexpr bool kAllWaves = false;
  int m, v0, v1;                                    // the launch's candidate positions are jbase .. jbase + m of the call's
  long long jbase;
  const float *__restrict__ mx, *__restrict__ se;   // [n]
  const long long *__restrict__ teff;               // [n]: the call's target position, -1 = ignored
  float *__restrict__ g;                            // [v1 - v0][m]
  __device__ __forceinline__ void operator()(const pf32x16 (&acc)[PR][PV], int pr, int j0, int l32, int h, const bool (&live)[PR],
                                             float q) const {
    int jl = j0 + 2 * l32;
    asm volatile("" : "+v"(jl));
    const bool have0 = jl < m, have1 = jl + 1 < m;
#pragma unroll
    for (int t = 0; t < PV; t++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int v = (pr * PV + t) * 32 + 8 * (e >> 2) + 4 * h + (e & 3);
        if (v < v0 || v >= v1) continue;
        const long long tg = teff[v];
        const float top = mx[v], sum = se[v];
        const long long at = (long long)(v - v0) * m + jl;
        float f0 = 0.f, f1 = 0.f;
        if (tg >= 0) {
          if (live[0]) f0 = w2b_xent_g(__fmul_rn(acc[0][t][e], q), top, sum, tg == jbase + jl);
          if (live[1]) f1 = w2b_xent_g(__fmul_rn(acc[1][t][e], q), top, sum, tg == jbase + jl + 1);
        }
        float *o = g + at;
        if (have1 && (at & 1) == 0) {
          *reinterpret_cast<float2 *>(o) = make_float2(f0, f1);
        } else {
          if (have0) o[0] = f0;
          if (have1) o[1] = f1;
        }
      }
  }
};

template <int BL>
__global__ void __launch_bounds__(PT, 2)
k_xent_grad(const uint64_t *__restrict__ T, int nb, long long rows, const long long *__restrict__ cand, long long cand_base, int m,
            const pf32x4 *__restrict__ X, int ng, int v0, int v1, int pairs_per_y, long long jbase, const float *__restrict__ mx,
            const float *__restrict__ se, const long long *__restrict__ teff, float *__restrict__ g) {
  GradEpilogue epi{m, v0, v1, jbase, mx, se, teff, g};
  embed_project_body<BL>(T, nb, rows, cand, cand_base, m, X, ng, v0 / (32 * PV), (v1 + 32 * PV - 1) / (32 * PV), pairs_per_y, false,
                         nullptr, epi);
}

// candidate groups x ranges of the pairs that hold vectors v0 .. v1, as w2b_launch_embed_project cuts them
void xent_grid(int m, int v0, int v1, dim3 *grid, int *per_y) {
  const int pairs = (v1 + 32 * PV - 1) / (32 * PV) - v0 / (32 * PV);
  const int gx = (int)(((long long)m + 4 * PR * 32 - 1) / (4 * PR * 32));
  int gy = (PWG + gx - 1) / gx;
  if (gy > pairs) gy = pairs;
  *per_y = (pairs + gy - 1) / gy;
  gy = (pairs + *per_y - 1) / *per_y;
  *grid = dim3((unsigned)gx, (unsigned)gy);
}

}  // namespace

hipError_t w2b_launch_embed_xent_clean(const long long *cand, long long m, long long rows, long long *clean,
                                       unsigned long long *bad, hipStream_t s) {
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_xent_clean, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, cand, m, rows, clean, bad);
  return hipGetLastError();
}

hipError_t w2b_launch_embed_xent_stats(const uint64_t *T, long long rows, int dim, int bitlevel, const void *X, int v0, int v1,
                                       const long long *clean, int m, const long long *target, float *Mseg,
                                       unsigned long long *Useg, float *tl, hipStream_t s) {
  if (v1 <= v0 || m <= 0) return hipSuccess;
  const int nb = (dim + 63) / 64, ng = (dim + 7) / 8;
  dim3 grid;
  int per_y = 1;
  xent_grid(m, v0, v1, &grid, &per_y);
  if (bitlevel == 2)
    hipLaunchKernelGGL(k_xent_stats<2>, grid, dim3(PT), 0, s, T, nb, rows, clean, m, (const pf32x4 *)X, ng, v0, v1, per_y, target,
                       Mseg, Useg, tl);
  else
    hipLaunchKernelGGL(k_xent_stats<1>, grid, dim3(PT), 0, s, T, nb, rows, clean, m, (const pf32x4 *)X, ng, v0, v1, per_y, target,
                       Mseg, Useg, tl);
  return hipGetLastError();
}

hipError_t w2b_launch_embed_xent_finish(int v0, int v1, long long m, int nseg, const float *Mseg, const unsigned long long *Useg,
                                        const long long *clean, const long long *target, float *mx, float *se, float *tl,
                                        long long *teff, unsigned long long *bad, hipStream_t s) {
  if (v1 <= v0) return hipSuccess;
  hipLaunchKernelGGL(k_xent_finish, dim3((unsigned)((v1 - v0 + 255) / 256)), dim3(256), 0, s, v0, v1, m, nseg, Mseg, Useg, clean,
                     target, mx, se, tl, teff, bad);
  return hipGetLastError();
}

hipError_t w2b_launch_embed_xent_grad(const uint64_t *T, long long rows, int dim, int bitlevel, const void *X, int v0, int v1,
                                      const long long *clean, long long jbase, int m, const float *mx, const float *se,
                                      const long long *teff, float *g, hipStream_t s) {
  if (v1 <= v0 || m <= 0) return hipSuccess;
  const int nb = (dim + 63) / 64, ng = (dim + 7) / 8;
  dim3 grid;
  int per_y = 1;
  xent_grid(m, v0, v1, &grid, &per_y);
  const long long *c = clean ? clean + jbase : nullptr;
  if (bitlevel == 2)
    hipLaunchKernelGGL(k_xent_grad<2>, grid, dim3(PT), 0, s, T, nb, rows, c, jbase, m, (const pf32x4 *)X, ng, v0, v1, per_y, jbase, mx,
                       se, teff, g);
  else
    hipLaunchKernelGGL(k_xent_grad<1>, grid, dim3(PT), 0, s, T, nb, rows, c, jbase, m, (const pf32x4 *)X, ng, v0, v1, per_y, jbase, mx,
                       se, teff, g);
  return hipGetLastError();
}
