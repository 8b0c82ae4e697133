// w2b_kernels_groups.hip -- form (i), ROW-GROUP variant of the worker kernel: one Hogwild worker = one workgroup whose
// wavefronts are split into G row groups + a producer wavefront + an adder wavefront.
//
// Why (VERDICT r04, weak #2 / missing #5): below a full device the library runs the reference's row semantics -- every row
// shared by all workers, context rows updated by lossless adds -- at the reference's own scale (-threads 0: 256 workers).
// The plain kernel (w2b_kernels_workers.hip) gives a worker ONE set of columns: at -size 200 that is one 64-lane
// wavefront per CU, and every centre word is a serial chain of memory round trips (table draws -> rows of the first 13
// targets -> sigmoid table -> rows of the last 12 -> ...) with the adds to the hottest context rows on every later wait
// (vmcnt is in order on gfx9): 26 us per centre word where one thread of the reference takes 5.7 us.  Here
//   * the rows of a centre word are spread over G ROW GROUPS (a group = RW wavefronts = one thread per 16-byte column, as
//     in the plain kernel): group g loads the context rows at window positions g, g + G, ... and the distinct target rows
//     number g, g + G, ... -- ALL negative + 1 targets are in flight at once: two memory round trips per centre word (context
//     rows, then -- on purpose only then -- target rows, so that a racy shared target row is open for one round trip);
//   * what crosses groups goes through LDS: the raw context rows (window average, ref :431-449, summed by every thread in
//     window order; the same values feed phase C), the quantized target rows and their gradient scalars (error
//     accumulation, ref :486-488, summed by every thread in TARGET ORDER) -- so every element sees the reference's
//     order of operations exactly as in the plain kernel, and the dot product uses the plain kernel's tree: one worker is
//     bit-identical to the plain kernel (tests/test_gpu_groups.py);
//   * a PRODUCER wavefront runs the scalar side (sentence reader, window draw, unigram-table draws, alpha schedule,
//     duplicate bookkeeping; ref :379-460) one centre word ahead into double-buffered lists -- in two passes, produce() under
//     the data wavefronts' wait for the target rows and prepare() under their error sum --, and the sigmoid table
//     (ref :614-618) sits in LDS -- no memory latency of the scalar side is left on the data wavefronts' path;
//   * an ADDER wavefront issues the lossless adds of the accumulated error to the frequent context rows
//     (`u[c] += e[c]` on the current value, ref :500-502; rows 1..atomic_rank_u) from a copy of the error vector in LDS,
//     in the contiguous layout (instruction e covers dwords [64 e, 64 e + 64) of the row), and books the log-sigmoid
//     terms of the loss (ref :480-483).  It never waits for memory: the queue at the hottest rows' memory lines is no
//     longer in front of the data wavefronts' next loads;
//   * a target row that repeats inside a centre word is taken again, after its first update, by the group that owns
//     it (same threads, program order), one extra pass per repetition -- the CPU's sequential semantics.
//   * the very hottest context rows (P.rc_rows of them) are READ at a copy per XCD that k_refresh_rows, a small kernel on a
//     stream of its own, keeps re-filling from the master rows while the launch runs; their updates stay lossless adds at the
//     master address (a read of a line that the memory side is adding to waits for the adds: DESIGN.md section 3.3c).
// Shapes: -size a multiple of 4 up to 1024 (RW = 1 / 2 / 4 wavefronts per row), window <= 16, negative + 1 <= G * TC,
// tables below 2 GiB, coherent rows, no per-XCD consensus copies; everything else runs the plain kernel.
#include "w2b_device.hpp"

// W2B_GROUPS_DRAIN: a row stored by one row group in word n may be loaded by another group (another wavefront) in word n + 1.
// __syncthreads() on gfx950 does not wait for outstanding vector-memory operations, so without a drain that read-after-write
// across wavefronts relies on the CU issuing its vector memory operations to the memory system in order (what the bit-identity
// tests of tests/test_gpu_groups.py check on every word of a Zipf stream).  1: every data wavefront waits for its stores
// (s_waitcnt vmcnt(0)) before the barrier that ends a word; 2: the adder wavefront waits for its atomic adds as well.  Measured
// in round 6 (profiles/r06_sessions/): see DESIGN.md section 3.3c for what each level costs and which one ships.
#ifndef W2B_GROUPS_DRAIN
#define W2B_GROUPS_DRAIN 1
#endif
#define W2G_CMAX 32      // context rows of a centre word (window <= 16)
#define W2G_TMAX 32      // targets of a centre word (negative + 1 <= G * TC <= 32)

// Phase timers (builds with -DW2B_PHASE_TIMERS; worker 0 only; printed by w2b_trainer_destroy under W2B_DEBUG):
//   producer: [0] produce(), [1] waiting at the barriers;  adder: [2] loss terms + adds issued, [3] barriers
//   data wavefront 0: [4] B0 -> loads issued -> context rows arrived and staged, [5] B1 wait, [6] window average + dot
//   products + g + row updates, [7] B3 wait, [8] error accumulation, [9] B4 wait, [10] phase C, [11] B0 wait, [12] words

namespace {

// what the producer wavefront hands over for ONE centre word (double buffered)
struct GLists {
  int cw, nt, npass, stop;        // stop: nothing to train -- the epoch is finished or the launch is over
  float alpha;
  int n_dup;
  int rc_n;                       // rows 1..rc_n of u are read at this XCD's refreshed copy for this word (0: the copies are not filled yet)
  int pad1;
  int ctx[W2G_CMAX];              // context rows of u, window order (ref :431-436)
  int umult[W2G_CMAX];            // multiplicity at the first occurrence of a row, 0 at later ones
  int tgt[W2G_TMAX];              // target rows of v: [0] = centre word, then the kept negatives (ref :450-460)
  int own[W2G_TMAX];              // own[g * TC + k]: index of the target that group g holds in register slot k (-1: none);
                                  // the n-th DISTINCT row goes to group n % G, slot n / G
  int dup_i[W2G_TMAX];            // repetitions of a row, in target order: index of the target ...
  int dup_g[W2G_TMAX];            // ... and the group that owns its row
};

struct GFixed {                   // LDS record of a worker: compile-time offsets
  GLists lists[2];
  WorkerLds S;                    // the worker's scalars, owned by the producer wavefront
  int pad_[2];
  int sen[W2B_MAX_SEN + 8];
  float exp_table[1000 + 8];
  float gs[W2G_TMAX];             // gradient scalar g of every target (ref :473-475)
  float fs[W2G_TMAX];             // dot product f of every target (loss bookkeeping)
  float red[W2G_TMAX * 4];        // partial dot products of the RW wavefronts of a group
};
static_assert(sizeof(GFixed) % 16 == 0, "the row regions behind GFixed are accessed 16 bytes at a time");

// add_col_contig (w2b_device.hpp) for a wavefront that is number `wig` of its row group: tab[row][256 wig ...] += d,
// transposed so that instruction e covers the dwords [64 e, 64 e + 64) of the wavefront's 1 KiB segment.  All 64 lanes
// take part (idle lanes pass zeros).
__device__ __forceinline__ void add_cols_group(float *tab, int row, int dim, const Col<4> &d, unsigned tab_bytes, int wig, int lane) {
  const int urow = __builtin_amdgcn_readfirstlane(row);
  __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)tab, 0, (int)tab_bytes, 0x27000);
  const int soff = urow * dim * 4;
  const int sel = lane & 3;
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int src = (16 * e + (lane >> 2)) << 2;
    const float p0 = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(d.e[0])));
    const float p1 = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(d.e[1])));
    const float p2 = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(d.e[2])));
    const float p3 = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(d.e[3])));
    const float v = sel == 0 ? p0 : (sel == 1 ? p1 : (sel == 2 ? p2 : p3));
    const int c = wig * 256 + e * 64 + lane;
    if (c < dim) (void)__builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(v, r, c * 4, soff, 16);
  }
}

// QM: quantizer; LOSS: loss bookkeeping; RW: wavefronts per row (16-byte columns: dim <= 256 RW); G: row groups;
// TC: target rows a group holds in registers (negative + 1 <= G * TC).  Wavefronts: [0, G RW) data, G RW producer,
// G RW + 1 adder.  All wavefronts execute the same sequence of workgroup barriers per centre word:
//   B1 (raw context rows staged)  [RW > 1: one per pass: partial dot products staged]  B3 (quantized targets + g staged)
//   B4 (error vector staged)  B0 (end of the word: the next word's lists are published).
template <int QM, bool LOSS, int RW, int G, int TC>
__global__ void __launch_bounds__((G * RW + 2) * 64, (RW == 4 ? 4 : 3)) k_train_groups(const W2bParams P, const long long max_positions) {
  static_assert(G * TC <= W2G_TMAX, "own[] capacity");
  extern __shared__ int smem[];
  W2B_LDS GFixed *const F = (W2B_LDS GFixed *)smem;
  const int dim = P.dim;
  W2B_LDS float *const errbuf = (W2B_LDS float *)((W2B_LDS char *)smem + sizeof(GFixed));   // [dim] accumulated error (ref :486-488)
  W2B_LDS float *const stash = errbuf + dim;                   // [2 window][dim] raw context rows, window order
  W2B_LDS float *const xq = stash + 2 * P.window * dim;        // [negative + 1][dim] quantized target rows (pre-update), target order
  constexpr int NDW = G * RW, NTHR = (NDW + 2) * 64;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool rc_on = P.rc_rows > 0;                                    // a refresher kernel runs beside this launch (k_refresh_rows)
  // s_getreg_b32 hwreg(HW_REG_XCC_ID, 0, 4): the XCD this workgroup runs on
  const int xcd = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & (W2B_NXCD - 1);
  const unsigned rc_bytes = (unsigned)(P.rc_rows * dim * 4);
  float *const rc_copy = P.rc + (long long)xcd * P.rc_rows * dim;
  const int wid = (int)blockIdx.x;
  W2bWorker *const Gw = P.workers + (wid < P.num_threads ? wid : 0);
  if (wid >= P.num_threads || Gw->done) {
    if (rc_on && tid == 0 && wid < P.num_threads) atomicAdd(&P.shared->launch_done, 1);
    return;
  }
  const QParam qp = make_qparam(P);
  W2B_LDS WorkerLds *const S = &F->S;
  W2B_LDS int *const s_sen = F->sen;
  // restore the worker, stage the sigmoid table
  copy_sentence(s_sen, Gw->sen, Gw->sen_len, tid, NTHR);
  for (int i = tid; i < 1000; i += NTHR) F->exp_table[i] = P.exp_table[i];
  if (tid == 0) worker_restore(Gw, S);
  __syncthreads();
  const bool reg_on = P.reg != 0.f;
  const int atomic_rank_v = P.atomic_rank, atomic_rank_u = P.atomic_rank_u;
  double loss_acc = 0.0;
#ifdef W2B_PHASE_TIMERS
  const bool timing_ = (wid == 0) && (lane == 0) && (wave == 0 || wave >= NDW);
  unsigned long long tick_ = __builtin_readcyclecounter();
#endif

  if (wave == NDW) {
    // ------------------------------------------------------------------------------------------ producer wavefront
    const int W = P.window, K = P.negative;
    // unigram-table draws of the NEXT pass, requested at the end of a pass (table_prefetch; lane l: draw l + 1)
    int t_pref = 0;
    bool pref_ok = false;
    // LCG jump-ahead constants of this lane's draw (x_{n+d} = ja x_n + jc, d = lane + 1) and of the whole word's negative draws
    const unsigned long long ja_l = P.jump_a[lane + 1 <= K ? lane + 1 : 0], jc_l = P.jump_c[lane + 1 <= K ? lane + 1 : 0];
    const unsigned long long ja_k = P.jump_a[K], jc_k = P.jump_c[K];
    auto jump_l = [&](unsigned long long x, int) { return ja_l * x + jc_l; };     // (only ever asked for d == lane + 1: one trip)
    auto jump_k = [&](unsigned long long x) { return ja_k * x + jc_k; };
    // one loop pass of TrainModelThread's scalar side (the wavefront-0 block of k_train_workers) into the lists O
    auto produce = [&](W2B_LDS GLists *O, const bool last) {
      unsigned long long rng = S->rng;
      long long cursor = S->cursor, wc = S->wc, last_wc = S->last_wc;
      int sen_len = S->sen_len, sen_pos = S->sen_pos, ovr = S->override_, eof = S->eof;
      int done = 0, cw = 0, nt = 0;
      // (requested first, used last: its round trip runs beside the unigram-table draws'.  The schedule below may store a new
      // alpha in this very pass -- only every 10000 words of this worker, and the other workers' stores land at any time anyway)
      const float alpha_now = __hip_atomic_load(&P.shared->alpha, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      float alpha = 0.f, alpha_own = 0.f;
      bool alpha_set = false;
      if (!last) {
        alpha_set = alpha_schedule_step(P, wc, last_wc, lane, &alpha_own);   // ref :379-393
        if (sen_len == 0) {                                            // ref :394-413
          read_sentence(P, (int *)s_sen, rng, cursor, wc, ovr, eof, sen_len, lane);
          sen_pos = 0;
          pref_ok = false;
          W2B_WAVE_SYNC();
        }
        if (eof || wc > P.train_words / P.total_threads) {            // ref :414-423 (local_iter == 1)
          epoch_end(P, wc, last_wc, lane);
          done = 1;
        } else {
          const int word = (sen_len > 0) ? s_sen[sen_pos] : 0;          // ref :424
          const int b = window_draw(P, rng);                            // ref :428-429
          const int hi = 2 * W + 1 - b;
          {                                                             // ref :431-436 (2 window + 1 <= 33 positions: one trip)
            const int a = b + lane;
            const int c = sen_pos - W + a;
            const bool ok = (a < hi) && (a != W) && (c >= 0) && (c < sen_len);
            const unsigned long long m = __ballot(ok);
            if (ok) O->ctx[__popcll(m & lane_lt_mask(lane))] = s_sen[c];
            cw = __popcll(m);
          }
          if (cw > 0) {                                                 // ref :450-460 (negative <= 31: one trip)
            nt = draw_targets<true>(P, O->tgt, word, rng, jump_l, jump_k, pref_ok, t_pref, lane);
            alpha = alpha_set ? alpha_own : alpha_now;                // (a worker sees the alpha it has just stored, as the plain kernel's load after the store does)
          }
          next_position(sen_pos, sen_len);                              // ref :505-509
        }
        // the next pass's table draws (see t_pref); its window draw comes first
        pref_ok = !done && sen_len != 0;
        if (pref_ok && lane < K) t_pref = table_prefetch(P, rng, jump_l, lane);
      } else pref_ok = false;
      if (lane == 0) {
        S->rng = rng; S->cursor = cursor; S->wc = wc; S->last_wc = last_wc;
        S->sen_len = sen_len; S->sen_pos = sen_pos; S->override_ = ovr; S->eof = eof;
        if (done) S->done = 1;
        O->stop = (done || last) ? 1 : 0;
        O->cw = cw; O->nt = nt; O->npass = 1; O->n_dup = 0; O->alpha = alpha;       // (npass / n_dup: prepare(), below)
        O->rc_n = (P.rc_rows > 0 && __builtin_nontemporal_load(&P.rc_flags[16 + xcd]) != 0) ? P.rc_rows : 0;
      }
    };
    // second half of a pass: the bookkeeping of the lists produce() has written -- which group holds which distinct target row,
    // the repetitions, the context rows' multiplicities.  A pass of its own so that the producer's work spreads over two barrier
    // intervals of the data wavefronts (produce: under their wait for the target rows; prepare: under their error sum) instead
    // of holding one barrier up (phase timers: 3 K of 20 K cycles per word were spent waiting for the producer at B3).
    auto prepare = [&](W2B_LDS GLists *O) {
      W2B_WAVE_SYNC();
      const int cw = __builtin_amdgcn_readfirstlane(O->cw), nt = __builtin_amdgcn_readfirstlane(O->nt);
      if (cw <= 0) return;
      int ndup = 0;
      {
        if (lane < W2G_TMAX) O->own[lane] = -1;
        W2B_WAVE_SYNC();
        // duplicates among the targets: occurrence number and first occurrence of every row
        const int me = (lane < nt) ? O->tgt[lane] : (-1 - lane);
        int occ = 0, root = lane;
        for (int j = 0; j < nt; j++) {
          const int tj = __builtin_amdgcn_readlane(me, j);
          const bool hit = (tj == me) && (j < lane);
          occ += hit ? 1 : 0;
          root = (hit && j < root) ? j : root;
        }
        const bool first = (lane < nt) && (occ == 0);
        const unsigned long long mf = __ballot(first);
        const int n = __popcll(mf & lane_lt_mask(lane));            // number of this row among the distinct rows
        if (first) O->own[(n % G) * TC + n / G] = lane;
        const int nroot = __builtin_amdgcn_ds_bpermute(root << 2, n);
        const bool isdup = (lane < nt) && (occ > 0);
        const unsigned long long md = __ballot(isdup);
        if (isdup) {
          const int dpos = __popcll(md & lane_lt_mask(lane));
          O->dup_i[dpos] = lane;
          O->dup_g[dpos] = nroot % G;
        }
        ndup = __popcll(md);
        // context rows: multiplicity at the first occurrence, 0 at later ones (a row that occurs m times in the window
        // is updated m times, ref :494-503)
        const int mc = (lane < cw) ? O->ctx[lane] : (-1 - lane);
        bool cfirst = true;
        int mult = 0;
        for (int j = 0; j < cw; j++) {
          const int cj = __builtin_amdgcn_readlane(mc, j);
          cfirst = cfirst && !(j < lane && cj == mc);
          mult += (j >= lane && cj == mc) ? 1 : 0;
        }
        if (lane < cw) O->umult[lane] = cfirst ? mult : 0;
      }
      if (lane == 0) { O->npass = 1 + ndup; O->n_dup = ndup; }
    };
    produce(&F->lists[0], max_positions <= 0);
    prepare(&F->lists[0]);
    __syncthreads();                                                    // B0
    for (long long it = 0;; ++it) {
      const W2B_LDS GLists *const L = &F->lists[it & 1];
      if (L->stop) break;
      const int cw = L->cw, npass = L->npass;
      if (cw > 0) __syncthreads();                                      // B1
      W2B_TICK(1);
      produce(&F->lists[(it + 1) & 1], it + 1 >= max_positions);        // (under the data wavefronts' wait for their target rows)
      W2B_TICK(0);
      if (cw > 0) {
        if (RW > 1) for (int ps = 0; ps < npass; ps++) __syncthreads();
        __syncthreads();                                                // B3
        W2B_TICK(1);
        prepare(&F->lists[(it + 1) & 1]);                               // (under the data wavefronts' error sum)
        W2B_TICK(0);
        __syncthreads();                                                // B4
      } else prepare(&F->lists[(it + 1) & 1]);
      __syncthreads();                                                  // B0
    }
  } else if (wave == NDW + 1) {
    // ------------------------------------------------------------------------------------------ adder wavefront
    constexpr int NE = RW * 4;                                          // dwords of a row per lane (contiguous layout)
    __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc((void *)P.u, 0, (int)P.tab_bytes, 0x27000);
    __syncthreads();                                                    // B0
    for (long long it = 0;; ++it) {
      const W2B_LDS GLists *const L = &F->lists[it & 1];
      if (L->stop) break;
      const int cw = L->cw;
      if (cw > 0) {
        const int nt = L->nt, npass = L->npass;
        __syncthreads();                                                // B1
        if (RW > 1) for (int ps = 0; ps < npass; ps++) __syncthreads();
        __syncthreads();                                                // B3
        W2B_TICK(3);
        if (LOSS) {                                                     // ref :480-483: lane j books target j
          for (int j = lane; j < nt; j += 64) loss_acc += (double)log_sigmoid_term(F->fs[j], j == 0);   // target 0 is the centre word
        }
        W2B_TICK(2);
        __syncthreads();                                                // B4
        W2B_TICK(3);
        if (!reg_on && atomic_rank_u > 0) {                             // u[c] += e[c] on the current value (ref :500-502)
          float ev[NE];
#pragma unroll
          for (int e = 0; e < NE; e++) {
            const int c = e * 64 + lane;
            ev[e] = (c < dim) ? errbuf[c] : 0.f;
          }
          for (int j = 0; j < cw; j++) {
            const int m = L->umult[j];
            const int crow = __builtin_amdgcn_readfirstlane(L->ctx[j]);
            if (m > 0 && crow <= atomic_rank_u) {
              const int soff = crow * dim * 4;
              for (int k = 0; k < m; k++) {                             // every one of the m updates is an add of its own
#pragma unroll
                for (int e = 0; e < NE; e++) {
                  const int c = e * 64 + lane;
                  if (c < dim) (void)__builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(ev[e], ru, c * 4, soff, 16);
                }
              }
            }
          }
        }
        W2B_TICK(2);
      }
#if W2B_GROUPS_DRAIN >= 2
      __builtin_amdgcn_s_waitcnt(0);                                    // ... and the adder's lossless adds have returned
#endif
      __syncthreads();                                                  // B0
    }
  } else {
    // ------------------------------------------------------------------------------------------ data wavefronts
    const int g = wave / RW, wig = wave % RW;                           // row group, wavefront inside the group (uniform)
    const int col0 = (wig * 64 + lane) * 4;
    const bool active = col0 < dim;
    constexpr int CA = (W2G_CMAX + G - 1) / G;                          // context rows per group
    constexpr int CB = (G == 3) ? 6 : 4;                                // ... loaded per trip (2 window <= 16: one trip)
    constexpr int LA = (RW == 4) ? 2 : 4, LE = (RW == 4) ? 4 : 8;       // LDS rows read ahead in the window average / the error sum
    const unsigned tab_bytes = P.tab_bytes;
    __syncthreads();                                                    // B0
    for (long long it = 0;; ++it) {
      const W2B_LDS GLists *const L = &F->lists[it & 1];
      if (L->stop) break;
      const int cw = L->cw;
      if (cw > 0) {
        const int nt = L->nt, npass = L->npass;
        const float alpha = L->alpha;
        const float ar2 = (2.f * alpha) * P.reg;                        // 2*alpha*reg (ref :490,:501)
        const int rc_n = L->rc_n;
        float regsq = 0.f;
        // ---- loads: this group's context rows (window positions g, g + G, ...: CB of them per trip -- one trip up to
        // window = 8), then its distinct target rows
        const int mine = (lane < TC) ? L->own[g * TC + lane] : -1;      // lane k: the target in register slot k
        const int trow = (mine >= 0) ? L->tgt[mine] : 0;
        int idx[TC], rows[TC];
        Col<4> x[TC];
#pragma unroll
        for (int k = 0; k < TC; k++) {
          idx[k] = __builtin_amdgcn_readlane(mine, k);
          rows[k] = __builtin_amdgcn_readlane(trow, k);
        }
        for (int j0 = 0; g + j0 * G < cw; j0 += CB) {
          Col<4> r[CB];
#pragma unroll
          for (int jj = 0; jj < CB; jj++) {
            const int j = g + (j0 + jj) * G;
            if (j < cw && active) {
              const int crow = __builtin_amdgcn_readfirstlane(L->ctx[j]);
              // a hot context row is read at this XCD's refreshed copy (its updates are lossless adds at the master address)
              if (crow <= rc_n) r[jj] = load_col<4, W2B_MM_XCD, 0>(rc_copy, crow - 1, dim, col0, rc_bytes);
              else r[jj] = load_col<4, 0, 0>(P.u, crow, dim, col0, tab_bytes);
            }
          }
#pragma unroll
          for (int jj = 0; jj < CB; jj++) {
            const int j = g + (j0 + jj) * G;
            if (j < cw && active) lds_st(stash + j * dim + col0, r[jj]);
          }
        }
        W2B_TICK(4);
        __syncthreads();                                                // B1
        W2B_TICK(5);
        // ---- the target rows are requested only now: a target row is open (read -> dot product -> update -> store) for one
        // memory round trip + its own arithmetic, not for the context rows' round trip as well.  What a racy shared row costs
        // in epoch loss grows with throughput x the time it is open (measured: heldout_zipf12 at 256 workers -1.6 % with the
        // targets requested beside the context rows, -1.1 % like this; planted corpus, configs[2] shape, 8 workers: +2.6 % / +1.3 %)
#pragma unroll
        for (int k = 0; k < TC; k++) {
#pragma unroll
          for (int e = 0; e < 4; e++) x[k].e[e] = 0.f;
          if (idx[k] >= 0 && active) x[k] = load_col<4, 0, 0>(P.v, rows[k], dim, col0, tab_bytes);
        }
        // ---- phase A: context_avg = (1/cw) * sum_j quantize(u[ctx_j]), window order (ref :431-449); LDS reads LA rows ahead
        Col<4> avg;
#pragma unroll
        for (int e = 0; e < 4; e++) avg.e[e] = 0.f;
        if (active) {
          int j0 = 0;
          for (; j0 + LA <= cw; j0 += LA) {                            // whole trips: straight-line code
            Col<4> c[LA];
#pragma unroll
            for (int jj = 0; jj < LA; jj++) c[jj] = lds_ld(stash + (j0 + jj) * dim + col0);
#pragma unroll
            for (int jj = 0; jj < LA; jj++) {
#pragma unroll
              for (int e = 0; e < 4; e++) {
                const float q = quant<QM>(c[jj].e[e], qp);
                avg.e[e] += q;
                if (LOSS && reg_on && g == 0) regsq += q * q;
              }
            }
          }
          for (; j0 < cw; j0++) {
            const Col<4> c = lds_ld(stash + j0 * dim + col0);
#pragma unroll
            for (int e = 0; e < 4; e++) {
              const float q = quant<QM>(c.e[e], qp);
              avg.e[e] += q;
              if (LOSS && reg_on && g == 0) regsq += q * q;
            }
          }
        }
        {
          const float cwf = (float)cw;
#pragma unroll
          for (int e = 0; e < 4; e++) avg.e[e] = active ? avg.e[e] / cwf : 0.f;   // ref :449
        }

        // one target: gradient scalar known -> quantized row to LDS (error accumulation), row update (ref :486-491)
        auto finish_row = [&](const int i, const int row, const float gk, Col<4> xr) {
          const bool by_add = row <= atomic_rank_v;                    // (uniform) lossless add of the delta instead of a store
          Col<4> dl, q4;
#pragma unroll
          for (int e = 0; e < 4; e++) { dl.e[e] = 0.f; q4.e[e] = 0.f; }
          if (active) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
              float xv = xr.e[e];
              // opaque copy: re-derive the quantized value here instead of keeping it alive since the dot product
              if (QM != 0) asm volatile("" : "+v"(xv));
              const float q = quant<QM>(xv, qp);
              if (LOSS && reg_on) regsq += q * q;                       // reg * sum q^2 of every target row (ref :463,:468-471)
              q4.e[e] = q;
              dl.e[e] = gk * avg.e[e] - ar2 * xv;
              xr.e[e] = xv + dl.e[e];
            }
            lds_st(xq + i * dim + col0, q4);
            if (!by_add) store_col<4, 0, 0>(P.v, row, dim, col0, xr, tab_bytes);
          }
          if (by_add) add_cols_group(P.v, row, dim, dl, tab_bytes, wig, lane);
        };
        auto dot_part = [&](const Col<4> &xr) -> float {              // this thread's part of f (ref :466; the plain kernel's tree)
          float t[4];
#pragma unroll
          for (int e = 0; e < 4; e++) t[e] = avg.e[e] * quant<QM>(xr.e[e], qp);
          const float s = (t[0] + t[1]) + (t[2] + t[3]);
          return active ? s : 0.f;
        };
        // ---- phase B, pass 0: the distinct target rows (ref :450-492)
        {
          float p[TC];
#pragma unroll
          for (int k = 0; k < TC; k++) p[k] = dot_part(x[k]);
#pragma unroll
          for (int k = 0; k < TC; k++) p[k] = wave_sum(p[k]);
          float fl = 0.f;
          if (RW == 1) {
#pragma unroll
            for (int k = 0; k < TC; k++) fl = (lane == k) ? p[k] : fl;
            fl = 0.f + fl;                                              // (the plain kernel sums its one wavefront's part onto 0)
          } else {
            if (lane == 0) {
#pragma unroll
              for (int k = 0; k < TC; k++)
                if (idx[k] >= 0) F->red[idx[k] * 4 + wig] = p[k];
            }
            __syncthreads();                                            // B2 (pass 0)
            if (lane < TC && mine >= 0) {
              for (int w = 0; w < RW; w++) fl += F->red[mine * 4 + w];
            }
          }
          float gl = 0.f;
          if (lane < TC && mine >= 0) {
            gl = grad_scalar(fl, mine == 0, alpha, F->exp_table);
            if (wig == 0) {
              F->gs[mine] = gl;
              if (LOSS) F->fs[mine] = fl;
            }
          }
#pragma unroll
          for (int k = 0; k < TC; k++) {
            if (idx[k] >= 0) {
              const float gk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gl), k));
              finish_row(idx[k], rows[k], gk, x[k]);
            }
          }
        }
        // ---- repeated target rows, one pass each, by the group that owns the row (same threads: program order)
        for (int ps = 1; ps < npass; ps++) {
          const int i = L->dup_i[ps - 1];
          const bool here = (L->dup_g[ps - 1] == g);
          const int row = __builtin_amdgcn_readfirstlane(L->tgt[i]);
          Col<4> xx;
#pragma unroll
          for (int e = 0; e < 4; e++) xx.e[e] = 0.f;
          float pp = 0.f;
          if (here) {
            __builtin_amdgcn_s_waitcnt(0);                              // the earlier update of this row has been performed
            if (active) xx = load_col<4, 0, 0>(P.v, row, dim, col0, tab_bytes);
            pp = wave_sum(dot_part(xx));
            if (RW > 1 && lane == 0) F->red[i * 4 + wig] = pp;
          }
          if (RW > 1) __syncthreads();                                  // B2 (pass ps)
          if (here) {
            float f = 0.f;
            if (RW == 1) f = 0.f + pp;
            else for (int w = 0; w < RW; w++) f += F->red[i * 4 + w];
            const float gk = grad_scalar(f, i == 0, alpha, F->exp_table);
            if (wig == 0 && lane == 0) {
              F->gs[i] = gk;
              if (LOSS) F->fs[i] = f;
            }
            finish_row(i, row, gk, xx);
          }
        }
        W2B_TICK(6);
        __syncthreads();                                                // B3
        W2B_TICK(7);
        // ---- error accumulation in target order (ref :486-488).  Round 5 let every row group sum all nt quantized target rows
        // for its own copy of the columns -- G times the same 25-row LDS sum (3.5 K of a word's 20 K cycles).  Round 6: the
        // columns are split over ALL data wavefronts of the worker, one thread per EC consecutive floats, every element still
        // summed by one thread in target order (same bits); the vector goes to LDS once, where the adder wavefront wanted it
        // anyway, and every thread reads its 16-byte column back after B4.
        {
          constexpr int EC = (RW == 4) ? 2 : 1;                         // NDW * 64 threads cover 256 / 512 / 1024 floats
          const int ecol = (wave * 64 + lane) * EC;
          const bool eact = ecol < dim;
          const float gv = (lane < nt) ? F->gs[lane] : 0.f;             // lane i: g of target i (negative + 1 <= 32)
          float er[EC];
#pragma unroll
          for (int e = 0; e < EC; e++) er[e] = 0.f;
          int i0 = 0;
          for (; i0 + LE <= nt; i0 += LE) {                             // whole trips: straight-line code, LDS reads LE rows ahead
            float c[LE][EC];
#pragma unroll
            for (int ii = 0; ii < LE; ii++)
              if (eact) {
#pragma unroll
                for (int e = 0; e < EC; e++) c[ii][e] = xq[(i0 + ii) * dim + ecol + e];
              }
#pragma unroll
            for (int ii = 0; ii < LE; ii++) {
              const float gi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gv), i0 + ii));
              if (eact) {
#pragma unroll
                for (int e = 0; e < EC; e++) er[e] += gi * c[ii][e];
              }
            }
          }
          for (; i0 < nt; i0++) {
            const float gi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gv), i0));
            if (eact) {
#pragma unroll
              for (int e = 0; e < EC; e++) er[e] += gi * xq[i0 * dim + ecol + e];
            }
          }
          if (eact) {
#pragma unroll
            for (int e = 0; e < EC; e++) errbuf[ecol + e] = er[e];
          }
        }
        W2B_TICK(8);
        __syncthreads();                                                // B4
        W2B_TICK(9);
        Col<4> err;
#pragma unroll
        for (int e = 0; e < 4; e++) err.e[e] = 0.f;
        if (active) err = lds_ld(errbuf + col0);
        // ---- phase C: u[ctx_j] += context_avge - 2*alpha*reg*u[ctx_j]   (ref :494-503); the adder wavefront takes the rows
        // that get lossless adds (reg == 0: their delta is the error vector itself)
#pragma unroll
        for (int jj = 0; jj < CA; jj++) {
          const int j = g + jj * G;
          if (j < cw) {
            const int m = L->umult[j];
            if (m > 0) {
              const int crow = __builtin_amdgcn_readfirstlane(L->ctx[j]);
              const bool by_add = crow <= atomic_rank_u;
              if (!(by_add && !reg_on)) {
                Col<4> rr, dl;
#pragma unroll
                for (int e = 0; e < 4; e++) { rr.e[e] = 0.f; dl.e[e] = 0.f; }
                if (active) rr = lds_ld(stash + j * dim + col0);
                for (int k = 0; k < m; k++) {                           // a row that occurs m times in the window is updated m times
                  if (active) {
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                      dl.e[e] = err.e[e] - ar2 * rr.e[e];
                      rr.e[e] = rr.e[e] + dl.e[e];
                    }
                  }
                  if (by_add) add_cols_group(P.u, crow, dim, dl, tab_bytes, wig, lane);
                }
                if (!by_add && active) store_col<4, 0, 0>(P.u, crow, dim, col0, rr, tab_bytes);
              }
            }
          }
        }
        if (LOSS && reg_on) {
          const float s = wave_sum(active ? regsq : 0.f);
          if (lane == 0) loss_acc -= (double)(P.reg * s);               // ref :437-445 and :463-471
        }
        W2B_TICK(10);
        W2B_COUNT(12);
      }
#if W2B_GROUPS_DRAIN >= 1
      __builtin_amdgcn_s_waitcnt(0);                                    // this wavefront's row stores have been acknowledged (see W2B_GROUPS_DRAIN)
#endif
      __syncthreads();                                                  // B0
      W2B_TICK(11);
    }
  }
  // save the worker
  __syncthreads();
  copy_sentence(Gw->sen, s_sen, S->sen_len, tid, NTHR);
  if (LOSS) {
    if (wave == NDW + 1) {                                              // the adder's lanes hold the log-sigmoid terms
      const double lsum = wave_sum_d(loss_acc);
      if (lane == 0) { atomicAdd(&Gw->loss, lsum); atomicAdd(&P.shared->loss_epoch, lsum); }
    } else if (lane == 0 && loss_acc != 0.0) {                          // lane 0 of the data wavefronts: reg terms
      atomicAdd(&Gw->loss, loss_acc);
      atomicAdd(&P.shared->loss_epoch, loss_acc);
    }
  }
  if (rc_on && tid == 0) atomicAdd(&P.shared->launch_done, 1);
  if (tid == NDW * 64) worker_save(P, Gw, S);                           // (lane 0 of the producer)
}

// The refresher of the hottest context rows' read copies: W2B_RC_BLOCKS small workgroups on a stream of their own, beside a
// launch of k_train_groups.  One per XCD (the first to claim it; the others leave) copies rows 1..rc_rows of u from their
// master addresses (agent scope) to this XCD's copies (nt: kept in this XCD's L2, where the workers of the XCD read them)
// over and over until every worker workgroup of the launch has finished.  Nobody waits for a refresher: while an XCD's
// copies are not filled its workers read the master rows.
__global__ void __launch_bounds__(256) k_refresh_rows(const W2bParams P) {
  __shared__ int claim, stop;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, dim = P.dim;
  const int xcd = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & (W2B_NXCD - 1);
  if (tid == 0) { claim = (atomicCAS(&P.rc_flags[xcd], 0, 1) == 0) ? 1 : 0; stop = 0; }
  __syncthreads();
  if (!claim) return;
  const unsigned rc_bytes = (unsigned)(P.rc_rows * dim * 4);
  float *const rc_copy = P.rc + (long long)xcd * P.rc_rows * dim;
  // wall_clock64(): s_memrealtime, a constant 100 MHz on gfx9 whatever the shader clock does
  const unsigned long long t_start = wall_clock64(), t_limit = 100ull * 100000000ull;     // 100 s: never spin forever
  for (long long sweep = 0;; ++sweep) {
    for (int r0 = wave; r0 < P.rc_rows; r0 += 16) {                  // four rows of this wavefront in flight at a time
      for (int c = lane * 4; c < dim; c += 256) {
        Col<4> v[4];
#pragma unroll
        for (int b = 0; b < 4; b++)
          if (r0 + 4 * b < P.rc_rows) v[b] = load_col<4, 0, 0>(P.u, r0 + 4 * b + 1, dim, c, P.tab_bytes);
#pragma unroll
        for (int b = 0; b < 4; b++)
          if (r0 + 4 * b < P.rc_rows) store_col<4, W2B_MM_XCD, 0>(rc_copy, r0 + 4 * b, dim, c, v[b], rc_bytes);
      }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    // ONE thread reads the workers' counter and the clock and publishes the decision: every wavefront takes the same branch
    // (round 5 let every thread load `done` for itself, so wavefronts could disagree about leaving the loop: advisor finding)
    if (tid == 0) {
      if (sweep == 0) __builtin_nontemporal_store(1, &P.rc_flags[16 + xcd]);                  // the copies of this XCD are filled
      const int done = __hip_atomic_load(&P.shared->launch_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (done >= P.num_threads) stop = 1;
      else if (wall_clock64() - t_start > t_limit) {
        // a launch this long outlives its refresher: the XCD's workers go back to the master rows instead of reading copies
        // that nobody re-fills any more
        __builtin_nontemporal_store(0, &P.rc_flags[16 + xcd]);
        stop = 1;
      }
    }
    __syncthreads();
    if (stop) break;
  }
}

// the instantiation of a shape: RW from the row length, (G, TC) fixed per RW
struct GroupShape { int rw, g, tc, threads; };
__host__ inline GroupShape group_shape(int dim) {
  GroupShape s;
  s.rw = dim <= 256 ? 1 : (dim <= 512 ? 2 : 4);
  s.g = s.rw == 4 ? 3 : 4;
  s.tc = s.rw == 4 ? 9 : 7;
  s.threads = (s.g * s.rw + 2) * 64;
  return s;
}

template <typename F>
hipError_t dispatch_groups(const W2bParams &p, bool loss, F &&f) {
  const GroupShape s = group_shape(p.dim);
  return dispatch_q(p.bitlevel, [&](auto qm) -> hipError_t {
    constexpr int QM = decltype(qm)::value;
    if (s.rw == 1) return loss ? f(k_train_groups<QM, true, 1, 4, 7>) : f(k_train_groups<QM, false, 1, 4, 7>);
    if (s.rw == 2) return loss ? f(k_train_groups<QM, true, 2, 4, 7>) : f(k_train_groups<QM, false, 2, 4, 7>);
    return loss ? f(k_train_groups<QM, true, 4, 3, 9>) : f(k_train_groups<QM, false, 4, 3, 9>);
  });
}

}  // namespace

size_t w2b_groups_lds_bytes(int dim, int window, int negative) {
  return sizeof(GFixed) + sizeof(float) * ((size_t)dim + (size_t)2 * window * dim + (size_t)(negative + 1) * dim);
}

// Can the row-group kernel run this shape / these row rules?  (everything else runs the plain kernel)
bool w2b_groups_ok(const W2bParams &p) {
  if (p.dim % 4 != 0 || p.dim > 1024 || p.dim < 4) return false;
  if (p.window > 16 || p.window < 1) return false;
  const GroupShape s = group_shape(p.dim);
  if (p.negative + 1 > s.g * s.tc) return false;
  if (p.tab_bytes == 0) return false;                                    // tables of 4 GiB and more: per-row descriptors (plain kernel)
  if (p.mem_mode != 0 || p.exact || p.wide) return false;                // coherent rows, fast reduction
  if (p.xhot != nullptr && p.xhot_u + p.xhot_v > 0) return false;        // per-XCD copies live in the plain kernel
  if (p.fresh_rank_u > 0) return false;
  if (w2b_groups_lds_bytes(p.dim, p.window, p.negative) > 160 * 1024) return false;
  return true;
}

int w2b_groups_per_cu(const W2bParams &p, bool loss) {
  const GroupShape s = group_shape(p.dim);
  const size_t lds = w2b_groups_lds_bytes(p.dim, p.window, p.negative);
  int nb = 0;
  (void)dispatch_groups(p, loss, [&](auto kern) -> hipError_t {
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, s.threads, lds);
  });
  return nb > 0 ? nb : 1;
}

hipError_t w2b_launch_refresher(const W2bParams &p, hipStream_t st) {
  hipLaunchKernelGGL(k_refresh_rows, dim3(W2B_RC_BLOCKS), dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t w2b_launch_groups(const W2bParams &p, long long max_positions, bool loss, hipStream_t st) {
  const GroupShape s = group_shape(p.dim);
  const size_t lds = w2b_groups_lds_bytes(p.dim, p.window, p.negative);
  return dispatch_groups(p, loss, [&](auto kern) -> hipError_t {
    if (lds > 48 * 1024) {
      const hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(p.num_threads), dim3(s.threads), lds, st, p, max_positions);
    return hipGetLastError();
  });
}
