// w2b_plan.cpp -- the launch policy (w2b_plan.h).  Pure host arithmetic: this file does not see the trainer's device state and
// makes no HIP runtime call; the shape predicates it asks (w2b_block_threads, w2b_resident_plan, w2b_resident_atomic_ok,
// w2b_groups_ok) live beside the kernels they describe and are host arithmetic too.  The measurements behind every rule stand
// next to the rule: they are the project's record.
#include "w2b_plan.h"

#include <cmath>

w2b_tuning w2b_default_tuning() {
  w2b_tuning tn{};
  tn.struct_size = (int32_t)sizeof(w2b_tuning);
  tn.hot_rows_v = tn.hot_rows_u = -1;
  tn.hot_period = 0;         // automatic
  tn.hot_cap = 128;
  tn.force_row_desc = 0;
  tn.grid_per_cu = 0;
  tn.mem_mode = -1;
  tn.atomic_rank = -1;
  tn.atomic_cap = 0;         // 0 = no cap
  tn.hot_weight_permille = 1000 / W2B_NXCD;
  tn.window_refresh = 16;
  return tn;
}

// The fields of W2bParams that follow from the configuration and the tuning knobs alone: what the shape predicates beside the
// kernels read, derived once for the plan and for the launch (make_params in w2b_trainer.cpp adds the device pointers and the
// plan's numbers).
void w2b_shape_params(W2bParams &p, const w2b_config &cfg, const w2b_tuning &tune) {
  p.window_magic = cfg.window > 1 ? (unsigned long long)((((unsigned __int128)1) << 64) / (unsigned __int128)cfg.window) : 0;
  {
    const unsigned long long bytes = (unsigned long long)cfg.vocab_size * cfg.layer1_size * sizeof(float);
    p.tab_bytes = bytes < 0x7fffffffull ? (unsigned)bytes : 0u;   // signed 32-bit scalar offsets
    // w2b_tuning.force_row_desc: run the large-table form (per-row buffer descriptors, what tables >= 2 GiB use) on any size
    if (tune.force_row_desc) p.tab_bytes = 0u;
  }
  p.vocab_size = cfg.vocab_size;
  p.train_words = cfg.train_words;
  p.iter = cfg.iter;
  p.dim = cfg.layer1_size;
  p.window = cfg.window;
  p.negative = cfg.negative;
  p.bitlevel = cfg.bitlevel;
  p.num_threads = cfg.num_threads;
  p.total_threads = cfg.total_threads > 0 ? cfg.total_threads : cfg.num_threads;
  p.mem_mode = cfg.relaxed_coherence;   // 0 coherent (sc1), 1 relaxed (plain); >1 experimental builds only
  if (tune.mem_mode >= 0) p.mem_mode = tune.mem_mode;
  p.exact = cfg.exact_reduction != 0;
  if (p.exact) p.mem_mode = 0;             // the exact mode exists for coherent rows only
  p.xhot_w = (float)tune.hot_weight_permille / 1000.f;
  p.win_refresh = tune.window_refresh;
  (void)w2b_block_threads(cfg.layer1_size, nullptr, &p.wide);   // rows longer than a workgroup has columns
  p.starting_alpha = cfg.alpha;
  p.sample = cfg.sample;
  p.reg = cfg.reg;
}

double w2b_plan_kept(const W2bPlanInputs &in, double c) {
  const double st = (double)in.cfg.sample * (double)in.cfg.train_words;
  return (in.cfg.sample > 0 && st > 0) ? (c < sqrt(c * st) + st ? c : sqrt(c * st) + st) : c;
}

double w2b_plan_rate_v(const W2bPlanInputs &in, double c) {
  return (in.counts_pw > 0 ? in.cfg.negative * pow(c, 0.75) / in.counts_pw : 0) + (in.counts_tot > 0 ? c / in.counts_tot : 0);
}
// the least frequent row's (counts are sorted): the measure of "so small and flat that every row collides"
static double least_frequent_rate_v(const W2bPlanInputs &in) { return w2b_plan_rate_v(in, (double)in.counts[(size_t)(in.cfg.vocab_size - 1)]); }

// How often is row i of v a target (ref :450-460)?  Per centre word: negative * cn_i^0.75 / sum cn^0.75 (the unigram
// table) + cn_i / train_words (as the centre word itself); and row i of u a context row: (window + 1 on average,
// SURVEY A.3) * cn_i / train_words.  The vocabulary is sorted by count, so the rows worth per-XCD copies / lossless adds
// are a prefix; how long a prefix is decided per launch from these rates and the number of workers (hot_rows, atomic_rows_v,
// atomic_rows_u below).
// (a token is a centre / context word only if it survives sub-sampling, ref :403-406: the counts that matter for
// those two roles are the expected KEPT occurrences; the negative draws use the raw counts, ref :112-128)
std::vector<float> w2b_plan_set_counts(W2bPlanInputs &in, const int64_t *cn) {
  const int64_t V = in.cfg.vocab_size;
  std::vector<float> keep((size_t)V, 1.f);
  if (in.cfg.sample > 0) w2b_build_keep_prob(cn, V, in.cfg.sample, in.cfg.train_words, keep.data());
  double pw = 0, tot = 0, tot_kept = 0;
  for (int64_t a = 0; a < V; a++) {
    pw += pow((double)cn[a], 0.75);
    tot += (double)cn[a];
    // (the total of the kept occurrences through the fp32 keep table the kernels use; "</s>" is never a centre or context
    // word, ref :400)
    const double k = in.cfg.sample > 0 ? (double)keep[(size_t)a] : 1.0;
    if (a > 0) tot_kept += (double)cn[a] * (k < 1.0 ? k : 1.0);
  }
  in.counts.assign(cn, cn + V);
  in.counts_pw = pw;
  in.counts_tot = tot;
  in.counts_tot_kept = tot_kept;
  const int n = (int)(V - 1 < W2B_XHOT_MAX ? V - 1 : W2B_XHOT_MAX);
  in.rate_v.assign((size_t)(n > 0 ? n : 0), 0.0);
  in.rate_u.assign((size_t)(n > 0 ? n : 0), 0.0);
  for (int k = 0; k < n; k++) {
    const double c = (double)cn[k + 1];
    // (raw counts for the choice of the rows with copies: measured in round 3 on the text8-sized corpus at 256 workers)
    in.rate_v[k] = w2b_plan_rate_v(in, c);
    in.rate_u[k] = tot > 0 ? (in.cfg.window + 1) * c / tot : 0;
  }
  return keep;
}

// Which worker kernel runs: plain_worker_kernel 0 = automatic (sentence-resident kernel for coherent rows when
// the window fits in LDS; plain kernel for relaxed rows, where caching in L2 already absorbs the re-reads and
// four workgroups per CU win), 1 = plain, 2 = sentence-resident whenever it fits -- coherent rows only: relaxed rows and
// the parity mode always run the plain kernel.  Returns the radius (-1 = not the sentence-resident kernel).
static int resident_radius(const W2bPlanInputs &in, int mode) {
  if (mode == 1 || mode == 3 || in.cfg.exact_reduction) return -1;   // the serial reduction lives in the plain kernel
  if (in.cfg.relaxed_coherence) return -1;              // the sentence-resident kernel exists for coherent rows only
  if (in.tune.mem_mode > 0) return -1;
  if (mode == 0) {
    // Automatic = the plain kernel (round 4).  The sentence-resident kernel keeps every context row PRIVATE to a worker
    // for as long as the row is in its window -- up to 2 x window + 1 positions, where the reference's thread holds a
    // context row for one -- and publishes the worker's accumulated progress when the row leaves.  With hundreds of
    // workers every frequent word is in dozens of windows at once, and the sum of those private progresses over-shoots.
    // Rounds 2-3 chose it wherever it was faster and kept it inside the fidelity gates of the regimes they measured
    // (text8-sized corpus: -1 ... -2.5 %) with a consensus rule for the most frequent context rows; on the first
    // held-out regime (Zipf exponent 1.2 at the configs[2] shape, tests/w2b_testlib.py HELDOUT) that same default is
    // 13 % off the reference's first-epoch loss at 256 workers (28 % without the consensus rule), the plain kernel
    // 0.1-2 %.  It stays available as an explicit choice (plain_worker_kernel = 2, ./word2bits -window-cache 1): the
    // faster kernel at short rows, with this caveat.
    return -1;
  }
  return w2b_resident_plan(in.cfg.layer1_size, in.cfg.window, in.cfg.negative);
}

// How many leading rows of u / v get per-XCD copies for a launch with `workers` concurrent workers / workgroups.
// Explicit numbers (w2b_tuning.hot_rows_*) win; otherwise a row is taken when its expected load -- uses per centre word
// x workers x row length -- reaches W2B_HOT_LOAD: a coherent row queues at its memory line (~7 M read-modify-writes per
// second for a 3200-byte row), workers deliver ~50 K words/s each at 800 floats, and the load should stay well below a
// tenth of that: rate x workers x floats >= 6400 is rate >= 0.016 for 512 workers of 800 floats (about 45 rows of a
// 400 K-word Zipf vocabulary), none for 8 workers and none on flat distributions.  Only for 16-byte columns, coherent
// rows, and not in the parity mode.
static const double W2B_HOT_LOAD = 6400.0;
// Round 4: per-XCD copies are a FULL-DEVICE mechanism.  Measured on the benchmarked regime (profiles/r04_sessions/): with
// up to a few hundred workers the copies cost fidelity whatever their number and merge period (64 workers: 3-5 copies -2.5 %,
// none +0.3 %; 256 workers: 16 copies -3.8 %, none +0.9 %) and buy nothing (the rows do not queue yet); on a full device
// (1024 workers) the picture turns: without copies the hottest rows queue at their memory lines (13.4 M words/s against
// 28.0 M) and 113 + 113 copies with the consensus rule are within 0.1-0.4 % of the reference's epoch loss.  So the automatic
// choice gives copies only when the launch has at least W2B_FULL_DEVICE_WG_PER_CU workgroups per CU; below that every row
// is shared by all workers as in the reference, and the context rows are updated by lossless adds (atomic_rows_u).
static const int W2B_FULL_DEVICE_WG_PER_CU = 3;
static const int W2B_HOT_PERIOD = 16;            // centre words between two merge events of a worker (merge_period)
static long long full_device_workers(int num_cus) { return (long long)W2B_FULL_DEVICE_WG_PER_CU * num_cus; }
static bool full_device(const W2bPlanInputs &in, long long workers) { return workers >= full_device_workers(in.num_cus); }
// Round 5: BETWEEN the reference's own scale (256 threads: the most its bands exist for, and what -threads 0 stays at) and a full
// device, explicit worker counts drifted on the benchmarked regime: +1.0 / +1.3 / +1.6 / +1.5 % of the reference's epoch loss
// at 320 / 440 / 512 / 640 workers with every row shared.  Round 4 had measured "4 copies of v, merged every word" at -0.1 % for
// 440 workers and not adopted it; round 5 measured the range (profiles/r05_sessions/r05q_mid_range.txt): -0.25 / -0.09 / -0.05 /
// -0.45 % at 320 / 440 / 512 / 640, and on the held-out 60 M-token regime +0.18 -> -0.05 % (440) and +0.29 -> +0.03 % (600).  At
// 767 workers it over-shoots (-1.5 % against +0.7 % shared), so the range ends at 2.5 workgroups per CU.  8 copies: -0.7 ... -1.2 %.
static const int W2B_REFERENCE_SCALE = 256, W2B_MID_RANGE_COPIES_V = 4;
static long long mid_range_top(int num_cus) { return 5ll * num_cus / 2; }
static bool mid_range(const W2bPlanInputs &in, long long workers) { return workers > W2B_REFERENCE_SCALE && workers <= mid_range_top(in.num_cus); }

// resident: the sentence-resident kernel, an explicit choice, keeps the rule it was measured with -- the load rule of round 3
// whatever the number of workers.  Only its target rows have copies (its context rows live in LDS); the context rows the load
// rule picks -- the rows that would be hot rows of u -- are merged by consensus and refreshed instead (*uavg,
// w2b_kernels_resident.hip).
static void hot_rows(const W2bPlanInputs &in, const W2bParams &shape, long long workers, bool resident, int *nu, int *nv, int *uavg) {
  *nu = *nv = *uavg = 0;
  if (shape.dim % 4 != 0 || shape.wide || shape.mem_mode != 0 || shape.exact) return;
  const long long vmax = in.cfg.vocab_size - 1 < W2B_XHOT_MAX ? in.cfg.vocab_size - 1 : W2B_XHOT_MAX;
  auto pick = [&](int explicit_n, const std::vector<double> &rate) -> int {
    long long n = 0;
    if (explicit_n >= 0) n = explicit_n;
    else {
      const int cap = in.tune.hot_cap < W2B_XHOT_MAX ? in.tune.hot_cap : W2B_XHOT_MAX;
      while (n < (long long)rate.size() && n < cap && rate[(size_t)n] * (double)workers * in.cfg.layer1_size >= W2B_HOT_LOAD) n++;
    }
    return (int)(n < vmax ? n : (vmax > 0 ? vmax : 0));
  };
  const bool gated = !resident && !full_device(in, workers);
  *nv = (in.tune.hot_rows_v < 0 && gated) ? 0 : pick(in.tune.hot_rows_v, in.rate_v);
  const int u = (in.tune.hot_rows_u < 0 && gated) ? 0 : pick(in.tune.hot_rows_u, in.rate_u);
  *(resident ? uavg : nu) = u;
  if (gated && in.tune.hot_rows_v < 0 && in.tune.hot_rows_u < 0 && mid_range(in, workers)) {   // (see mid_range above)
    const int n = pick(-1, in.rate_v);                   // never more rows than the load rule would take
    *nv = n < W2B_MID_RANGE_COPIES_V ? n : W2B_MID_RANGE_COPIES_V;
  }
}

// Rows 1..n (by count) whose updates are atomic adds at their master address (w2b_tuning.atomic_rank).  A load / modify /
// store of a row is open for about 10 us on this machine (the rows of a chunk are loaded together and written after
// their dot products), during which every other worker's update of the same row is lost; a row that is a target of
// `rate` centre words is hit about 0.6 x workers x rate times per window.  Measured: on small
// flat vocabularies, where that number is between a fraction and a few for EVERY row, atomic adds bring the epoch
// losses of 64 ... 512 workers back to the reference's (planted corpus, 512 workers, first epoch: -1.1 % instead of
// -31 %); on Zipf vocabularies they change nothing that matters (the rows that collide are the hot rows, which have
// their own scheme, and summing the hundreds of stale gradients a hot row collects per window over-shoots) and cost
// 20-30 % of the throughput.  Automatic therefore means: all rows when even the least frequent row collides
// (0.6 x workers x rate >= W2B_ATOMIC_LOAD) and the tables are cache-sized, none otherwise; atomic_cap > 0 limits the
// number of rows.
static const double W2B_ATOMIC_LOAD = 0.25;
static bool have_counts(const W2bPlanInputs &in) { return !in.counts.empty() && in.counts_pw > 0 && in.counts_tot > 0; }
// Is there a kernel that honours atomic ranks for this shape?  Coherent rows, fast reduction, one thread per column; with
// 16-byte columns only the workgroups of at most 256 threads have the ATOM instantiations (-size <= 1024; the row-group
// kernel covers the same range).  Everywhere else the rules below return 0 -- for explicit ranks too -- so that
// w2b_plan_rows / w2b_worker_kernel_info describe what runs (round 4 reported ranks that the kernels silently ignored).
static bool atomics_supported(const W2bParams &shape) {
  int vec = 0;
  const int threads = w2b_block_threads(shape.dim, &vec);
  if (shape.exact || shape.wide || shape.mem_mode != 0) return false;
  if (vec == 4 && threads > 256) return false;
  return true;
}
static int atomic_rows_v(const W2bPlanInputs &in, const W2bParams &shape, long long workers) {
  if (!atomics_supported(shape)) return 0;
  const long long V = in.cfg.vocab_size;
  long long n = 0;
  if (in.tune.atomic_rank >= 0) n = in.tune.atomic_rank;
  else if (have_counts(in)) {
    // ... and the tables are small enough to live in the caches: atomic adds are executed by the memory system, and on
    // tables that do not fit they cost a multiple of a store (uniform ids over 60 K words x 200 floats: 15 M words/s
    // instead of 100 M).  8 MB per table covers the corpora where a flat small vocabulary occurs (planted: 1.7 MB).
    const bool cacheable = (double)V * in.cfg.layer1_size * sizeof(float) <= 8.0e6;
    if (cacheable && 0.6 * (double)workers * least_frequent_rate_v(in) >= W2B_ATOMIC_LOAD) n = V - 1;
    if (in.tune.atomic_cap > 0 && n > in.tune.atomic_cap) n = in.tune.atomic_cap;
  }
  return (int)(n < V - 1 ? n : V - 1);
}

// Context rows (u) updated with atomic adds.  The reference adds a centre word's accumulated error to every context row
// with `u[c] += e[c]` on the row's CURRENT value (ref :500-502): nothing another thread added since the row was read for
// the window average (ref :439) is lost -- the gradient is a whole centre word old, its application is not.  A GPU worker
// that stores `value read in phase A + e` instead erases whatever the other workers added to the row during that centre
// word.  How many others hold the row at that moment: workers x (uses of the row per centre word) -- a row is in a window
// for the whole centre word, on the CPU as here, so this number is the reference's own at the same thread count.  Rows
// for which it reaches W2B_ATOMIC_LOAD (a quarter of a worker) get the add; the vocabulary is sorted by count, so they
// are a prefix.  Measured (profiles/r04_sessions/): the benchmarked regime at 64 / 256 / 1024 workers within 0.9 % of the
// reference's epoch loss with lossless context rows and NO per-XCD copies, against +1.6 / +2.8 / +5.3 % with plain stores;
// cost 1-2 % of the throughput in the transposed 16-byte-column form (add_col_contig).
static int atomic_rows_u(const W2bPlanInputs &in, const W2bParams &shape, long long workers, int atomic_rank_v) {
  const long long V = in.cfg.vocab_size;
  if (!atomics_supported(shape)) return 0;                        // (before an explicit rank: relaxed rows + agent-scope adds do not mix)
  if (in.tune.atomic_rank_u > 0) return (int)(in.tune.atomic_rank_u < V - 1 ? in.tune.atomic_rank_u : V - 1);
  if (in.tune.atomic_rank_u < 0) return 0;
  if (in.tune.atomic_rank >= 0) return atomic_rank_v;            // an explicit atomic_rank speaks for both tables (round-3 meaning)
  // full device with per-XCD copies: the rows that matter are at their copies, and adds for the rows below them cost 7 % of
  // the throughput for nothing measurable (+0.37 % against -0.09 % of the reference's loss)
  if (full_device(in, workers) && in.tune.hot_rows_u != 0) return atomic_rank_v;
  long long n = atomic_rank_v;
  if (!in.counts.empty() && in.counts_tot_kept > 0) {
    long long lo = 0, hi = V - 1;                                 // largest row whose rate still reaches the threshold
    while (lo < hi) {
      const long long mid = (lo + hi + 1) / 2;
      const double rate = (in.cfg.window + 1) * w2b_plan_kept(in, (double)in.counts[(size_t)mid]) / in.counts_tot_kept;
      if ((double)workers * rate >= W2B_ATOMIC_LOAD) lo = mid; else hi = mid - 1;
    }
    if (lo > n) n = lo;
  }
  return (int)(n < V - 1 ? n : V - 1);
}

// The row-group kernel (w2b_kernels_groups.hip; round 5) runs a worker as G row groups + a producer + an adder wavefront:
// all targets of a centre word in flight at once, the scalar side one word ahead, the lossless adds to the frequent context
// rows off the data wavefronts' path.  It implements the SHARED-ROW rules only (every row at its master address, context
// rows 1..atomic_rank_u by lossless adds) -- what the library runs below a full device (hot_rows) -- for 16-byte
// columns up to -size 1024, window <= 16, negative + 1 <= 27/28, tables below 2 GiB.  plain_worker_kernel: 3 = wherever it
// fits, 1 / 2 = never; 0 = automatic:
//   * rows of at most W2B_GROUPS_AUTO_DIM floats (at -size 800 a row already fills four wavefronts, a worker is a 14-wavefront
//     workgroup and its own latency, not the rows, bounds it: 14.7 M words/s at 256 workers where the plain kernel does 10 and
//     a full device 26);
//   * and only where the fidelity budget is not already thin.  With Hogwild rows what a kernel costs in epoch loss grows
//     with its THROUGHPUT x the time a row is open (measured, profiles/r05_sessions/: at equal words/s the two kernels are
//     equally far from the reference; the row-group kernel at equal worker counts is about twice as fast and 0.3 ... 0.8 %
//     further off).  Two regimes sit at the 1.5 % floor with the plain kernel already: vocabularies so small and flat that
//     every row collides (the quantity atomic_rows_v uses: 0.6 x workers x rate of the least frequent row, an eighth of
//     W2B_ATOMIC_LOAD and more -- the planted corpus from 5 workers on), and shards shorter than the library's own guideline
//     of W2B_WORDS_PER_WORKER_MIN words per worker and epoch (explicit -threads 256 on a 6-8 M-token corpus; the CLI warns
//     there).  Both keep the plain kernel.
static const int W2B_GROUPS_AUTO_DIM = 512;
static const long long W2B_WORDS_PER_WORKER_MIN = 50000;
// `shape` carries the row rules of the launch that w2b_groups_ok asks about (fresh_rank_u; the copies are counted here)
static bool groups_run(const W2bPlanInputs &in, const W2bParams &shape, int mode, long long workers, int copies) {
  if (mode == 1 || mode == 2) return false;
  if (mode == 0) {
    if (in.cfg.layer1_size > W2B_GROUPS_AUTO_DIM) return false;
    if (!have_counts(in)) return false;                                                   // (the rules below need the word counts)
    const long long total = in.cfg.total_threads > 0 ? in.cfg.total_threads : workers;
    if (in.cfg.train_words > 0 && in.cfg.train_words / (total > 0 ? total : 1) < W2B_WORDS_PER_WORKER_MIN) return false;
    if (0.6 * (double)workers * least_frequent_rate_v(in) >= W2B_ATOMIC_LOAD / 8) return false;
  }
  if (copies > 0) return false;                        // per-XCD copies live in the plain kernel
  return w2b_groups_ok(shape);
}

// Rows 1..n of u that the row-group kernel reads at refreshed per-XCD copies (w2b_tuning.refresh_rows_u).  Measured
// (profiles/r05_sessions/): what bounds the shared-row mode on a Zipf stream is neither the adds to the hottest context rows
// nor their reads, but the two ON THE SAME LINES -- a read of a line that the memory side is adding to waits for the adds in
// front of it (about 50 ns per operation on the hottest line, whatever the row length: 13-15 M words/s at -size 200 ... 1000).
// With the reads of the 4 hottest rows moved to copies the -size 200 stream runs at 22 M words/s instead of 14 M at 256
// workers.  The price is freshness: a copy lags its master row by a refresher sweep (a few us), which adds to the staleness
// of exactly the rows that are updated most often -- heldout_zipf12 at 256 workers: -1.1 % of the reference's epoch loss
// without copies, -1.35 % with 4, -2.7 % with 16, -3.9 ... -5.6 % with ~25.  So only the very hottest rows are taken: a row
// whose load `workers x uses per centre word` reaches W2B_RC_LOAD -- 4-5 rows of a Zipf(1) vocabulary at 256 workers, 1 at
// 64, none below 40 workers and none on flat vocabularies -- and only among the rows whose updates are lossless adds (a
// stored `copy value + e` would lose every update since the last refresh).
static const double W2B_RC_LOAD = 40.0;
static int refreshed_rows_u(const W2bPlanInputs &in, long long workers, int atomic_rank_u) {
  const long long V = in.cfg.vocab_size;
  long long n = 0;
  if (in.tune.refresh_rows_u < 0) return 0;
  if (in.tune.refresh_rows_u > 0) n = in.tune.refresh_rows_u;
  else if (!in.counts.empty() && in.counts_tot_kept > 0) {
    while (n < W2B_RC_MAX && n + 1 < V &&
           (double)workers * (in.cfg.window + 1) * w2b_plan_kept(in, (double)in.counts[(size_t)(n + 1)]) / in.counts_tot_kept >= W2B_RC_LOAD) n++;
  }
  if (n > W2B_RC_MAX) n = W2B_RC_MAX;
  if (n > atomic_rank_u) n = atomic_rank_u;
  if (n > V - 1) n = V - 1;
  return (int)(n > 0 ? n : 0);
}

// How many workers of the plain kernel run AT ONCE (w2b_tuning.concurrent_workers; 0 = automatic).  A worker is a shard and an LCG
// stream; how many of them are in flight together is an execution detail -- the reference's own threads are scheduled by the OS,
// and a GPU launch with more workers than resident workgroups already runs them in rounds.  Automatic = all of them, except on
// vocabularies so small and flat that every row collides (atomic_rows_v: every row gets lossless adds).  There what decides the
// epoch loss is concurrency x the time a row is open, and a GPU workgroup has a chunk of 13 target rows open for ~10 us where the
// reference's thread has one row open for ~1.5 us: 64 workers at once over-shoot (planted corpus at the configs[2] shape: -1.0 ...
// -2.8 % over five epochs, the ONE stated exception of the 1.5 % floor until round 6), a part of them at a time do not.
// Measured (planted corpus, configs[2] shape, 64 workers, five epochs; profiles/r06_sessions/r06h_planted_concurrency.txt, r06i):
//   at once   epoch losses vs the reference's 64-thread band          accuracy (band 16.9-17.8)
//      64     -0.7 / -1.2 / -1.4 / -2.0 / -2.5 %                       19.9      (rounds 3-5: the exception)
//      32     -0.1 / +0.2 / -0.6 / -1.4 / -1.2 %                       15.5
//      16     +0.3 / +0.4 / +0.1 / -0.3 / +0.1 %                       14.2
//       8     +0.5 / +1.1 / +0.6 / +0.5 / +0.5 %                       14.1
// The losses want few workers at once, the accuracy (which in the reference itself rises from 9.5 at 8 threads to 17.3 at 64) wants
// many: 3/8 of the workers, at least 16, keeps both inside their gates.
static const int W2B_FLAT_CONCURRENCY_NUM = 3, W2B_FLAT_CONCURRENCY_DEN = 8, W2B_FLAT_CONCURRENCY_MIN = 16;
static int concurrent_workers(const W2bPlanInputs &in, int workers, int atomic_rank_v) {
  int c = workers;
  if (in.tune.concurrent_workers > 0) c = in.tune.concurrent_workers;
  else if (workers > W2B_FLAT_CONCURRENCY_MIN && atomic_rank_v >= in.cfg.vocab_size - 1 && in.tune.atomic_rank < 0) {
    c = workers * W2B_FLAT_CONCURRENCY_NUM / W2B_FLAT_CONCURRENCY_DEN;
    if (c < W2B_FLAT_CONCURRENCY_MIN) c = W2B_FLAT_CONCURRENCY_MIN;
  }
  if (c > workers) c = workers;
  return c > 0 ? c : 1;
}

// Merge period: a worker merges every W2B_HOT_PERIOD = 16 centre words.  Round 4 chose 32 on the 22 M-token proxy of the
// benchmarked regime (+0.06 % of the reference's epoch loss at 1024 workers, against +0.9 % at 8).  Round 5 recorded the
// reference on BASELINE configs[1] literally (100 M tokens) and measured both files (profiles/r05_sessions/r05n_balance.txt):
// period 32: -1.16 ... -1.38 % (literal) / +0.27 % (proxy); 16: -0.70 % / +0.67 %; 8: +0.32 % / +1.11 %; 64: -1.10 % / +0.47 %.
// The longer the stream the further stale copies pull the epoch loss down, so the period that centres BOTH is the default;
// it costs ~2 % of the headline throughput against 32.
static int merge_period(const W2bPlanInputs &in, long long workers, bool resident) {
  if (in.tune.hot_period > 0) return in.tune.hot_period;
  // The sentence-resident kernel (an explicit choice; its context rows are private in LDS, only target rows have copies) keeps
  // round 4's period of 32.  Round 5 gave it the mid-range value of the line below -- a resident launch has 2 workgroups per CU, never
  // "a full device" by the 3-per-CU rule -- i.e. a merge after EVERY word: that, not the move from 32 to 16, is what took the
  // cfg5 shape's sentence-resident leg from 0.889 to 0.776 of the roofline between the round-4 and round-5 driver runs (same-box
  // A/B in round 6: 36.9-37.2 M words/s as shipped in round 5, 41.4 M with 32, 38.4 M for the round-4 library;
  // profiles/r06_sessions/r06b_cfg5_ab.txt, r06c_cfg5_resident_period.txt).
  if (resident) return 2 * W2B_HOT_PERIOD;
  return full_device(in, workers) ? W2B_HOT_PERIOD : 1;   // (mid range: every word)
}

// THE decision of a launch, for every consumer (w2b_train_step, w2b_train_tuples_device, w2b_worker_kernel_info,
// w2b_suggested_threads, w2b_plan_rows), in one fixed order: the kernel kind first, because the row rules depend on it (round 3
// decided the kernel in w2b_train_step alone, so the reports could name the sentence-resident kernel while the plain one ran;
// round 5 decided the merge period in a place that did not know which kernel ran).  Recomputed for every launch: a binary
// search over the vocabulary and a few short loops -- 0.1 us (256 workers) to 0.3 us (1024 workers, 114 + 114 copies) of host
// time at the headline shape (400 K words, no sub-sampling; timed in a loop on the host), against tens of ms per launch.
W2bLaunchPlan w2b_plan_launch(const W2bPlanInputs &in, long long workers, bool plain_only) {
  W2bLaunchPlan lp{};
  W2bParams shape{};
  w2b_shape_params(shape, in.cfg, in.tune);
  const int mode = plain_only ? 1 : in.cfg.plain_worker_kernel;
  // 1. sentence-resident?  Atomic row updates (small flat vocabularies) exist in only some forms of that kernel; the others
  //    run the plain kernel.
  lp.atomic_rank_v = atomic_rows_v(in, shape, workers);
  lp.radius = resident_radius(in, mode);
  if (lp.radius >= 0 && lp.atomic_rank_v > 0 && !w2b_resident_atomic_ok(shape, lp.radius)) lp.radius = -1;
  const bool resident = lp.radius >= 0;
  // 2. the row rules of that kernel (the sentence-resident kernel keeps its context rows in LDS: no copies, no adds for u)
  hot_rows(in, shape, workers, resident, &lp.copies_u, &lp.copies_v, &lp.uavg_rank);
  lp.atomic_rank_u = resident ? 0 : atomic_rows_u(in, shape, workers, lp.atomic_rank_v);
  lp.fresh_rank_u = shape.fresh_rank_u = in.tune.fresh_rank_u > 0 ? in.tune.fresh_rank_u : 0;
  // 3. row groups or plain, and what only one of the two has
  const bool groups = !resident && groups_run(in, shape, mode, workers, lp.copies_u + lp.copies_v);
  lp.kernel = resident ? W2B_KERNEL_RESIDENT : (groups ? W2B_KERNEL_GROUPS : W2B_KERNEL_PLAIN);
  lp.refresh_rows_u = groups ? refreshed_rows_u(in, workers, lp.atomic_rank_u) : 0;
  lp.concurrent_workers = lp.kernel == W2B_KERNEL_PLAIN ? concurrent_workers(in, (int)workers, lp.atomic_rank_v) : (int)workers;
  // 4. merging the copies
  lp.full_device = full_device(in, workers) ? 1 : 0;
  lp.merge_period = merge_period(in, workers, resident);
  const long long per_xcd = workers / W2B_NXCD > 0 ? workers / W2B_NXCD : 1;
  const int most = lp.copies_u > lp.copies_v ? lp.copies_u : lp.copies_v;
  lp.xhot_m = most > 0 ? (int)((most + per_xcd - 1) / per_xcd) : 1;       // every copy of an XCD is merged about once per merge_period steps
  return lp;
}

// (judged for a full device: the atomic rule depends on the number of workers, which is what is being asked for)
long long w2b_plan_probe_workers(const W2bPlanInputs &in) { return 2ll * in.num_cus > in.cfg.num_threads ? 2ll * in.num_cus : in.cfg.num_threads; }

// Fewest words of an epoch a worker should have when the library picks the number of workers (W2B_WORDS_PER_WORKER_MIN): alpha is
// re-computed per worker only every 10000 of its own words (ref :379-393), so short shards coarsen the schedule.  20000 in
// rounds 2-3; the text8-sized corpus then ran 850 workers and ended its later epochs 2 % off the reference whatever the
// row-update scheme (256 workers: 0.5 %), i.e. the cap, not a race, was what the gate saw.
long long w2b_plan_suggested_workers(const W2bPlanInputs &in, const W2bLaunchPlan &probe, long long device_workers) {
  long long n = device_workers;
  // A worker adjusts alpha only after >10000 of its own words (ref :379-393): with shards shorter than that no worker
  // ever does and the whole epoch runs at the starting alpha.  Never suggest more workers than leave every shard
  // at least two such periods long (train_words here is the job's global number; 0 = unknown, no cap).
  if (in.cfg.train_words > 0) {
    const long long total = in.cfg.total_threads > 0 && in.cfg.num_threads > 0
                                ? (long long)in.cfg.total_threads / in.cfg.num_threads : 1;   // replicas
    const long long cap = in.cfg.train_words / (W2B_WORDS_PER_WORKER_MIN * (total > 0 ? total : 1));
    if (n > cap) n = cap > 1 ? cap : 1;
  }
  // Not enough words for a full device.  Round 4 stopped at 256 workers here, the reference's own scale: beyond it the
  // shared-row mode drifted (+1.3 ... +1.5 % at 440 workers on the benchmarked regime).  Round 5:
  //   * rows of at most 512 floats stay at 256 workers -- the row-group kernel runs there (22 M words/s at -size 200; with the
  //     mid-range copies the plain kernel would run instead, at half of that);
  //   * longer rows go on to the mid range (257 .. 640 workers, four target rows with copies merged every word: within 0.5 %
  //     of the reference on the benchmarked regime and 35-45 % faster than 256 workers: 13.5 M words/s at 440, 14.3 M at 512-640
  //     on the 22 M-token headline-shape file, where 256 workers run 9.9 M).
  if (probe.radius < 0 && n < full_device_workers(in.num_cus) && n > W2B_REFERENCE_SCALE) {
    const long long mid_top = mid_range_top(in.num_cus);
    const bool short_rows = in.cfg.plain_worker_kernel != 1 && in.cfg.layer1_size <= W2B_GROUPS_AUTO_DIM;
    n = short_rows ? W2B_REFERENCE_SCALE : (n < mid_top ? n : mid_top);
    // (no copies for this trainer -- relaxed rows, flat counts, ...: the reference's scale)
    if (w2b_plan_launch(in, n, true).copies_v == 0) n = W2B_REFERENCE_SCALE;
  }
  return n;
}

// The row rules of a launch without a device (pure host arithmetic on the word counts): what w2b_train_step would decide for
// `workers` concurrent workers on a GPU with `num_cus` compute units.
extern "C" int w2b_plan_rows(const w2b_config *cfg, const w2b_tuning *tune, const int64_t *cn, int32_t num_cus, int32_t workers,
                             w2b_row_plan *out) {
  if (!cfg || !cn || !out || num_cus < 1 || workers < 1 || cfg->vocab_size < 2 || cfg->layer1_size < 1)
    return w2b_internal_fail(W2B_EINVAL, "w2b_plan_rows: bad argument");
  if (tune && tune->struct_size != (int32_t)sizeof(w2b_tuning)) return w2b_internal_fail(W2B_EINVAL, "w2b_plan_rows: struct_size of w2b_tuning");
  W2bPlanInputs in;
  in.cfg = *cfg;
  in.num_cus = num_cus;
  in.tune = tune ? *tune : w2b_default_tuning();
  (void)w2b_plan_set_counts(in, cn);
  // plain_worker_kernel == 2 (sentence-resident whenever it fits) is planned as if it were 1: this report has always described
  // the plain kernel's rules there, and describing the sentence-resident launch instead is a change of behaviour of its own.
  const W2bLaunchPlan lp = w2b_plan_launch(in, workers, cfg->plain_worker_kernel == 2);
  out->copies_u = lp.copies_u;
  out->copies_v = lp.copies_v;
  out->atomic_rank_v = lp.atomic_rank_v;
  out->atomic_rank_u = lp.atomic_rank_u;
  out->full_device = lp.full_device;
  out->merge_period = lp.merge_period;
  out->row_group_kernel = lp.kernel == W2B_KERNEL_GROUPS ? 1 : 0;
  out->refresh_rows_u = lp.refresh_rows_u;
  out->concurrent_workers = lp.concurrent_workers;
  return W2B_OK;
}
