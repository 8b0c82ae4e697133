// w2b_kernels_embedback.hip -- the packed embedding's back-projection (include/word2bits_embed.h, "Back-projection"):
//   dx[i][a] = S * q,   S = the sum, in segment order, of the float32 chains  P_s = +0;  P_s = fmaf(g[i][j], (float)t_r[a], P_s)
// over the live candidate positions j of segment s (W2B_EMBED_WSEG positions each), r = cand[j].  That is the matrix
// product [n][m] x [m][dim] with the candidates as the K dimension, on v_mfma_f32_32x32x2_f32, whose accumulators are
// sequential fmaf chains in k order (k_vec_scan in w2b_kernels_evalvec.hip and k_embed_project rely on the same fact), with
// the row operand decoded from the packed bits in registers.  It is the weighted bag of w2b_kernels_embed.hip with dense
// weights, n bags at a time: the same chains, the same segments, the same bits.
//
// Operand roles.  A = g: lane l supplies g[i0 + l % 32][j + l / 32].  B = the decoded rows: lane l supplies (float)t of row
// cand[j + l / 32] at column c0 + l % 32.  Accumulator e of lane l is vector 8 (e / 4) + 4 (l / 32) + e % 4, column l % 32:
// a half wave holds 32 adjacent columns of one vector of the row-major [n][dim] output, 128 contiguous bytes per store.
// A workgroup of four wavefronts owns kBackVec = 128 vectors x 128 columns: every wavefront its own 32 columns and ALL
// kBackV = 4 vector tiles, so that one decoded B value feeds four MFMAs.
//
// B operand.  All 32 lanes of a half wave need bits of the same 32-bit half of one row's word.  Per 64 positions lane l
// loads that half (sign, and magnitude at bitlevel 2) of the row of position j0 + l -- ids through cand or base + j,
// clamped to row 0 when the position is dead (padding, >= rows, past m) -- and K step k takes the words of positions 2k and
// 2k + 1 out of lanes 2k and 2k + 1 with v_readlane (wave-uniform, as k_embed_bagw hands out its ids and weights); a lane
// picks the one of its half wave, shifts its column's bit down and puts the float pattern +-1.0f / +-3.0f together with
// integer operations.  A dead position keeps whatever bits it has: its g is +0 in the A operand, and fmaf(+0, t, P) = P for
// every P these chains can hold (P starts at +0 and is never -0), so there is no epilogue fix-up.
//
// A operand.  g[i][j] for 32 vectors at a fixed j is a stride-m access, so it is not issued as such: the workgroup stages a
// tile of 128 vectors x 64 positions through LDS.  Thread (wave w, lane l) loads g[i0 + 4 p + w][j0 + l], p = 0 .. 31: a
// wavefront reads 256 contiguous bytes per instruction, from clamped indices (vector min(., n - 1), position min(., m - 1)),
// replaces the value of a dead position by +0 -- a select, not a multiply: g may hold NaN there -- and writes it to
// tile[position][vector] with a row stride of 129 floats, so that neither the writes (64 positions, one vector) nor the
// reads (32 vectors, one position per half wave) meet in a bank.  The loads of the NEXT tile are issued before the MFMAs of
// the current one and wait in registers (the +0 is selected when the tile is written, behind the barrier: selected where the
// loads are issued, the wavefront would wait for them before its MFMAs).  Both barriers of a tile are reached by every thread: the loop bounds are
// uniform over the workgroup, and a wavefront whose columns lie past dim only skips the MFMAs and the stores.
//
// Segments.  The accumulator tile walks one segment as 512 K steps from +0.  k_embed_back<.., false> then adds P_s into an S it
// keeps in registers and goes on (the path for launches whose vector tiles x column tiles fill the device on their own);
// k_embed_back<.., true> takes ONE segment per workgroup (blockIdx.y) and stores P_s into the scratch part[segment][n][dim] with
// plain vector stores, and k_embed_back_finish adds the segments in order, one thread per element, and multiplies once (the
// k_embed_bagw_finish pattern; no float atomics).  The same operations in the same order: the same bits.  A launch that is
// not the first of a call (a later range of segments, a later chunk of the host form) starts from the S that the one
// before it left in dx, and only the last one multiplies by q.
//
// profiles/embed_backproject_kernel_resources.txt is the register report to check after a toolchain update: no scratch
// access between the first and the last MFMA.
#include <cstdlib>
#include <cstring>

#include "../../include/word2bits_embed.h"
#include "w2b_internal.h"

namespace {

constexpr int kBackThreads = 256;            // four wavefronts, each with its own 32 columns
constexpr int kBackV = 4;                    // 32-vector tiles of a wavefront: the MFMAs per decoded B value
constexpr int kBackVec = 32 * kBackV;        // vectors of a workgroup
constexpr int kBackCol = 128;                // columns of a workgroup
constexpr int kBackK = 64;                   // positions of a staged tile
constexpr int kBackLd = kBackVec + 1;        // floats between two positions of the tile in LDS
constexpr int kBackSegTiles = W2B_EMBED_WSEG / kBackK;
constexpr int kBackFill = 256;               // vector tiles x column tiles from which the in-register path fills the device
constexpr int kBackScratchWG = 1024;         // workgroups a launch of the scratch path aims at (bounds the scratch)

typedef float bf32x16 __attribute__((ext_vector_type(16)));

// T32 = the packed table as 32-bit halves, nh per row; cand = the candidates' rows [m] or nullptr, then position j is row
// cand_base + j; g = [n][.] with ldg floats between two vectors; seg0 = the first segment of this launch, and a workgroup
// walks segments seg0 .. seg0 + nseg - 1 (SCRATCH: the one segment seg0 + blockIdx.y); part = [segments of the launch][n][dim].
template <int BL, bool SCRATCH>
__global__ void __launch_bounds__(kBackThreads, 2)
k_embed_back(const uint32_t *__restrict__ T32, long long nh, int nb, long long rows, const long long *__restrict__ cand,
             long long cand_base, int m, const float *__restrict__ g, long long ldg, int n, int dim, int ncg, int seg0,
             int nseg, int first, int last, float *__restrict__ dx, float *__restrict__ part, unsigned long long *bad) {
  __shared__ float tile[kBackK * kBackLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l32 = lane & 31, h = lane >> 5;
  const int cg = (int)(blockIdx.x % (unsigned)ncg), vg = (int)(blockIdx.x / (unsigned)ncg);
  const int i0 = vg * kBackVec, c0 = cg * kBackCol + wave * 32;
  const bool active = c0 < dim;                              // wave-uniform: this wavefront has columns
  const bool counts = bad && blockIdx.x == 0 && wave == 0;   // who counts the candidates >= rows: once per position
  const int sfirst = SCRATCH ? seg0 + (int)blockIdx.y : seg0;
  const int t_begin = sfirst * kBackSegTiles;
  const int t_end = (int)min((long long)(sfirst + (SCRATCH ? 1 : nseg)) * kBackSegTiles, ((long long)m + kBackK - 1) / kBackK);
  const float q = BL == 1 ? __uint_as_float(0x3EAAAAABu) : 0.25f;
  // the 32-bit half of the row's words that holds this wavefront's columns (a legal one when it has none)
  const int wb = min(c0 >> 6, nb - 1);
  const int hs = 2 * BL * wb + ((c0 >> 5) & 1), hm = hs + 2;

  // one tile's operands, requested: this lane's words of the row of position 64 tt + lane, its 32 values of g
  uint32_t pws = 0u, pwm = 0u;
  float pre[kBackVec / 4];
  bool pdead = true;
  long long nid = -1;                                        // the id of the tile requested next: asked for one tile earlier,
  auto request_id = [&](int tt) {                            // so that the row's address does not wait for it
    const int j = tt * kBackK + lane;                        // (below 2^31: m <= 0x7FFFFF00)
    nid = -1;
    if (tt < t_end && j < m) nid = cand ? cand[j] : cand_base + j;
  };
  auto request = [&](int tt) {
    const int j = tt * kBackK + lane;
    const long long id = nid;
    if (id >= rows && counts) atomicAdd(bad, 1ull);
    const bool dead = id < 0 || id >= rows;
    const uint32_t *row = T32 + (dead ? 0ll : id) * nh;
    pws = row[hs];
    if constexpr (BL == 2) pwm = row[hm];
    const float *gp = g + min(j, m - 1);
#pragma unroll
    for (int p = 0; p < kBackVec / 4; p++) pre[p] = gp[(long long)min(i0 + 4 * p + wave, n - 1) * ldg];
    pdead = dead;
    request_id(tt + 1);                                           // (the +0 is selected where the tile is written: a select here would
  };                                                         //  wait for the loads before the MFMAs they are meant to run under)

  bf32x16 acc[kBackV], S[SCRATCH ? 1 : kBackV];
#pragma unroll
  for (int t = 0; t < kBackV; t++)
#pragma unroll
    for (int e = 0; e < 16; e++) acc[t][e] = 0.f;
  if constexpr (!SCRATCH) {
#pragma unroll
    for (int t = 0; t < kBackV; t++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int v = i0 + 32 * t + 8 * (e >> 2) + 4 * h + (e & 3), c = c0 + l32;
        S[t][e] = (!first && v < n && c < dim) ? dx[(long long)v * dim + c] : 0.f;
      }
  }

  if (t_begin < t_end) {
    request_id(t_begin);
    request(t_begin);
  }
  for (int tt = t_begin; tt < t_end; tt++) {
    __syncthreads();                                         // the tile before this one has been multiplied
#pragma unroll
    for (int p = 0; p < kBackVec / 4; p++) tile[lane * kBackLd + 4 * p + wave] = pdead ? 0.f : pre[p];
    const uint32_t ws = pws, wm = pwm;
    __syncthreads();
    if (tt + 1 < t_end) request(tt + 1);
    if (active) {
      // (eight K steps at a time: unrolled over the whole tile the compiler takes all 64 words out of the lanes at once and
      // runs out of scalar registers)
#pragma unroll 1
      for (int k8 = 0; k8 < kBackK / 2; k8 += 8)
#pragma unroll
      for (int ku = 0; ku < 8; ku++) {                       // K step: positions 64 tt + 2 k + h
        const int k = k8 + ku;
        const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)ws, 2 * k);
        const uint32_t s1 = (uint32_t)__builtin_amdgcn_readlane((int)ws, 2 * k + 1);
        uint32_t pat = 0x3F800000u;
        if constexpr (BL == 2) {
          const uint32_t m0 = (uint32_t)__builtin_amdgcn_readlane((int)wm, 2 * k);
          const uint32_t m1 = (uint32_t)__builtin_amdgcn_readlane((int)wm, 2 * k + 1);
          pat += (((h ? m1 : m0) >> l32) & 1u) * 0x00C00000u;  // 1.0f or 3.0f
        }
        const float tv = __uint_as_float(pat | (((h ? s1 : s0) >> l32) << 31));
        const float *ap = tile + (2 * k + h) * kBackLd + l32;
#pragma unroll
        for (int t = 0; t < kBackV; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[32 * t], tv, acc[t], 0, 0, 0);
      }
    }
    if constexpr (!SCRATCH) {
      if ((tt + 1) % kBackSegTiles == 0 || tt + 1 == t_end) { // the segment ends: S = S + P_s, one add each
#pragma unroll
        for (int t = 0; t < kBackV; t++)
#pragma unroll
          for (int e = 0; e < 16; e++) {
            S[t][e] = __fadd_rn(S[t][e], acc[t][e]);
            acc[t][e] = 0.f;
          }
      }
    }
  }

  if (!active) return;                                       // (behind the last barrier)
  // (the asm keeps the compiler from carrying the 64 masks and offsets of the first loop across the K loop to this one)
  int vb = i0 + 4 * h, c = c0 + l32;
  asm volatile("" : "+v"(vb), "+v"(c));
#pragma unroll
  for (int t = 0; t < kBackV; t++)
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const int v = vb + 32 * t + 8 * (e >> 2) + (e & 3);
      if (v >= n || c >= dim) continue;
      const long long at = (long long)v * dim + c;
      if constexpr (SCRATCH) {
        part[(long long)blockIdx.y * n * dim + at] = acc[t][e];
      } else {
        dx[at] = last ? __fmul_rn(S[t][e], q) : S[t][e];
      }
    }
}

// S = (first ? +0 : what the range before left in dx); S = S + P_s for the nseg segments of part in order; dx = last ? S q : S
__global__ void __launch_bounds__(kBackThreads)
k_embed_back_finish(const float *__restrict__ part, long long total, int nseg, int first, int last, int bitlevel,
                    float *__restrict__ dx) {
  const long long at = (long long)blockIdx.x * kBackThreads + threadIdx.x;
  if (at >= total) return;
  float S = first ? 0.f : dx[at];
  for (int s = 0; s < nseg; s++) S = __fadd_rn(S, part[(long long)s * total + at]);
  dx[at] = last ? __fmul_rn(S, bitlevel == 1 ? __uint_as_float(0x3EAAAAABu) : 0.25f) : S;
}

}  // namespace

// The driver's choice for n vectors: *use_scratch = the segments go through the scratch and the finishing kernel, *segs of
// them per launch, *scratch_bytes of device scratch.  The in-register path when the output tiles alone fill the device or
// there is one segment only; otherwise ranges of segments that make up about kBackScratchWG workgroups, so that the scratch
// is at most kBackScratchWG tiles of 64 KiB: 64 MiB, whatever m is.  W2B_EMBED_BACK_PATH = "registers" / "scratch" overrides
// the choice (for the tests, which cannot cross the switch at small shapes; the bound then holds up to 1024 tiles only).
void w2b_embed_backproject_plan(int dim, long long n, long long m, int *use_scratch, int *segs, long long *scratch_bytes) {
  const long long tiles = ((n + kBackVec - 1) / kBackVec) * (((long long)dim + kBackCol - 1) / kBackCol);
  const long long nseg = (m + W2B_EMBED_WSEG - 1) / W2B_EMBED_WSEG;
  bool scratch = tiles < kBackFill && nseg > 1;
  if (const char *env = getenv("W2B_EMBED_BACK_PATH")) {
    if (!strcmp(env, "registers")) scratch = false;
    if (!strcmp(env, "scratch")) scratch = true;
  }
  long long per = tiles > 0 ? kBackScratchWG / tiles : 1;
  per = per < 1 ? 1 : (per > nseg ? (nseg > 0 ? nseg : 1) : per);
  *use_scratch = scratch ? 1 : 0;
  *segs = (int)per;
  *scratch_bytes = scratch ? per * n * dim * 4 : 0;
}

// n vectors g (ldg floats apart) against the m candidate positions of this launch, which begin a segment: position j is row
// cand[j], or cand_base + j when cand is nullptr.  first = the positions begin the whole list (S starts at +0, else at what
// dx holds), last = they end it (dx = S q, else S).  use_scratch / segs / part as w2b_embed_backproject_plan chose them.
hipError_t w2b_launch_embed_backproject(const uint64_t *T, long long rows, int dim, int bitlevel, const float *g,
                                        long long ldg, long long n, const long long *cand, long long cand_base, int m,
                                        int first, int last, float *dx, int use_scratch, int segs, void *part,
                                        unsigned long long *bad, hipStream_t s) {
  if (n <= 0 || m <= 0) return hipSuccess;
  const int nb = (dim + 63) / 64, ncg = (dim + kBackCol - 1) / kBackCol;
  const long long nh = 2ll * bitlevel * nb;
  const int nseg = (int)(((long long)m + W2B_EMBED_WSEG - 1) / W2B_EMBED_WSEG);
  const uint32_t *T32 = reinterpret_cast<const uint32_t *>(T);
  if (use_scratch) {
    if (segs < 1 || !part) return hipErrorInvalidValue;
    const unsigned gx = (unsigned)(ncg * ((n + kBackVec - 1) / kBackVec));
    const long long total = n * dim;
    for (int s0 = 0; s0 < nseg; s0 += segs) {                // ranges of segments, in order; the finishing step carries S
      const int ns = nseg - s0 < segs ? nseg - s0 : segs;
      const int f = first && s0 == 0, l = last && s0 + ns == nseg;
      const dim3 grid(gx, (unsigned)ns);
      if (bitlevel == 2)
        hipLaunchKernelGGL((k_embed_back<2, true>), grid, dim3(kBackThreads), 0, s, T32, nh, nb, rows, cand, cand_base, m, g, ldg,
                           (int)n, dim, ncg, s0, ns, f, l, dx, (float *)part, bad);
      else
        hipLaunchKernelGGL((k_embed_back<1, true>), grid, dim3(kBackThreads), 0, s, T32, nh, nb, rows, cand, cand_base, m, g, ldg,
                           (int)n, dim, ncg, s0, ns, f, l, dx, (float *)part, bad);
      hipLaunchKernelGGL(k_embed_back_finish, dim3((unsigned)((total + kBackThreads - 1) / kBackThreads)), dim3(kBackThreads), 0, s,
                         (const float *)part, total, ns, f, l, bitlevel, dx);
    }
    return hipGetLastError();
  }
  // ranges of vector groups, so that a grid stays below 2^30 workgroups; only the first range counts refused candidates
  const long long vmax = (long long)kBackVec * ((1ll << 30) / ncg);
  for (long long v0 = 0; v0 < n; v0 += vmax) {
    const long long nv = n - v0 < vmax ? n - v0 : vmax;
    const unsigned gx = (unsigned)(ncg * ((nv + kBackVec - 1) / kBackVec));
    unsigned long long *b = v0 == 0 ? bad : nullptr;
    if (bitlevel == 2)
      hipLaunchKernelGGL((k_embed_back<2, false>), dim3(gx), dim3(kBackThreads), 0, s, T32, nh, nb, rows, cand, cand_base, m,
                         g + v0 * ldg, ldg, (int)nv, dim, ncg, 0, nseg, first, last, dx + v0 * dim, (float *)nullptr, b);
    else
      hipLaunchKernelGGL((k_embed_back<1, false>), dim3(gx), dim3(kBackThreads), 0, s, T32, nh, nb, rows, cand, cand_base, m,
                         g + v0 * ldg, ldg, (int)nv, dim, ncg, 0, nseg, first, last, dx + v0 * dim, (float *)nullptr, b);
  }
  return hipGetLastError();
}
