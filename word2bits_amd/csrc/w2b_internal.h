// w2b_internal.h -- structures and launchers shared by the HIP kernels (w2b_kernels_*.hip) and the host side of the
// C ABI (w2b_trainer.cpp, w2b_exchange.cpp, w2b_plan.cpp, w2b_eval.cpp, w2b_embed.cpp).  Not part of the public interface (include/).
// The host units that make no HIP call (w2b_corpus.cpp, w2b_eval_twins.cpp, w2b_eval_text.cpp, w2b_embed_twins.cpp) do not include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define W2B_LCG_A 25214903917ULL   // ref src/word2bits.cpp:352 (same constants at :405,:428,:455)
#define W2B_LCG_C 11ULL
#define W2B_MAX_SEN 1000           // ref src/word2bits.cpp:32
#define W2B_MAXW 16                // max wavefronts per workgroup (1024 threads)
#define W2B_NXCD 8                 // accelerator complex dies of an MI355X, each with its own L2 (HW_REG_XCC_ID: 0..7)
#define W2B_XHOT_MAX 128           // most rows of one table with per-XCD copies

// Racy globals of the reference that all workers share (ref src/word2bits.cpp:51,53):
// alpha and word_count_actual.  One instance in device memory per trainer.
struct W2bShared {
  float alpha;
  int pad0;
  unsigned long long word_count_actual;
  double loss_tuples;   // loss sum of the tuple form (form ii)
  int workers_done;
  int corpus_overrun;   // a worker reached the end of a corpus SLICE (w2b_set_corpus_slice) before its quota: the slice was cut too short
  // replicas (one per GPU): word_count_actual above is LOCAL.  The alpha schedule (ref :391) runs on the global count:
  // what the other replicas had done at the last exchange + the assumption that each of them has advanced like this
  // one since (exact at every exchange; single replica: both fields stay 0 and the schedule is the reference's).
  unsigned long long wca_others;      // sum of the other replicas' word_count_actual at the last exchange
  unsigned long long wca_at_sync;     // this replica's word_count_actual at the last exchange
  double loss_epoch;                  // sum of the workers' total_loss of the running epoch (ref :537-538)
  int launch_done, pad1;              // worker workgroups of the running launch that have finished (the refreshers of the row-group kernel wait for it)
  unsigned long long dbg[16];   // phase timers of workgroup 0 (builds with -DW2B_PHASE_TIMERS only)
};

// Per-worker locals of TrainModelThread (ref src/word2bits.cpp:364-375) that must survive between
// launches because one epoch is cut into several kernel launches.
struct W2bWorker {
  unsigned long long rng;         // next_random
  long long cursor;               // index of the next unread corpus token
  long long word_count, last_word_count;
  double loss;                    // total_loss
  int sen_len, sen_pos;           // sentence_length, sentence_position
  int first_override;             // pending truncated first word of the shard (-2 none)
  int done;                       // epoch finished (local_iter reached 0)
  int sen[W2B_MAX_SEN];           // sen[]
};

struct W2bParams {
  float *u, *v;                   // [vocab_size][dim] fp32 masters
  const float *exp_table;         // [1000]
  const int32_t *table;           // unigram table
  long long table_size;
  const float *keep;              // sub-sampling threshold per word (nullptr when sample <= 0)
  const int32_t *corpus;          // token ids, 0 = </s>
  long long n_tokens;
  int corpus_more;                // the resident tokens are a slice and the file goes on behind them (end of slice != EOF)
  W2bWorker *workers;
  W2bShared *shared;
  const unsigned long long *jump_a, *jump_c;   // LCG jump-ahead: x_{n+k} = jump_a[k]*x_n + jump_c[k]
  long long vocab_size, train_words, iter;
  unsigned tab_bytes;             // bytes of one table when < 4 GiB (32-bit addressing of rows), else 0
  unsigned long long table_magic, window_magic;   // floor(2^64 / table_size), floor(2^64 / window)
  int dim, window, negative, bitlevel, num_threads;
  int total_threads;              // workers across all replicas (quota ref :414, alpha extrapolation)
  int mem_mode;                   // 0 coherent (sc1 row accesses), 1 relaxed (plain cached accesses)
  float *entry;                   // sentence-resident kernel: scratch rows [num_threads][2][slots][dim] (see w2b_kernels_resident.hip)
  // XCD-shared copies of the hottest rows (w2b_device.hpp "XHot"): [W2B_NXCD][copies of u rows 1..xhot_u | copies of v rows
  // 1..xhot_v | entries of the same][dim], then the merge locks [rows][W2B_MAXW].  0 / 0 = every row is accessed at its
  // master address.
  float *xhot;
  int xhot_u, xhot_v;
  int hot_period;                 // centre words between two merge events of a worker / workgroup (power of two)
  int xhot_m;                     // hot rows of each table that one merge event brings up to date
  int uavg_rank;                  // sentence-resident kernel: context rows 1..uavg_rank are merged by consensus and refreshed
  int win_refresh;                // ... at the latest after this many steps in a worker's window (0 = never)
  float xhot_w;                   // weight of one XCD's copy in the consensus of a merge (1 / W2B_NXCD by default)
  float *wide_scratch;            // rows too long for one thread per column: [workgroups][2][dim] (process_word_wide)
  int wide;                       // 1: such rows (1024 threads, every thread owns several columns)
  int atomic_rank;                // rows 1..atomic_rank (by count) of v are updated with fp32 atomic adds: no lost updates (see w2b_tuning)
  int atomic_rank_u;              // the same for u (plain worker / tuple kernels: the context rows' phase C)
  int fresh_rank_u;               // plain kernels, phase C: context rows 1..fresh_rank_u are re-read before their update instead of
                                  // taken from the LDS stash of phase A (the update lands on the current value, ref :500-502)
  int exact;                      // serial dot product in the reference's order (plain worker / tuple kernels)
  // Refreshed read copies of the hottest context rows (row-group kernel, w2b_kernels_groups.hip): rows 1..rc_rows of u are READ
  // at this XCD's copy (nt: served by the XCD's L2) while their updates stay lossless adds at the master address; one
  // refresher workgroup per XCD copies master -> copy in a loop for as long as the launch's workers run.
  int rc_rows;                    // 0 = none
  float *rc;                      // [W2B_NXCD][rc_rows][dim]
  int *rc_flags;                  // [0..8) claim (one refresher per XCD), [16..24) alive (the XCD's copies have been filled in this launch)
  int worker_base;                // plain worker kernel: workgroup b is worker worker_base + b (a launch may cover a slice of the workers:
                                  // w2b_tuning.concurrent_workers)
  float starting_alpha, sample, reg;
};

// the fields above that follow from the configuration and the tuning knobs alone (w2b_plan.cpp): what the shape predicates
// below read.  The launch policy and the trainer's make_params both start from it.
struct w2b_config;
struct w2b_tuning;
void w2b_shape_params(W2bParams &p, const w2b_config &cfg, const w2b_tuning &tune);

// launchers implemented in w2b_kernels_*.hip ------------------------------------------------------
// block size chosen from dim: one thread per 16-byte (or 4-byte) column of a row
int w2b_block_threads(int dim, int *vec_out, int *wide_out = nullptr);
size_t w2b_lds_bytes(int dim, int window, int negative, bool worker_form, bool exact = false);
int w2b_tuple_max_grid(int num_cus);                                   // most workgroups w2b_launch_tuples starts
hipError_t w2b_launch_tuples(const W2bParams &p, long long n, const int32_t *center,
                             const int32_t *ctx_off, const int32_t *ctx, const int32_t *neg,
                             float alpha, int grid, int num_cus, int per_cu_override, bool loss,
                             hipStream_t s);
hipError_t w2b_launch_workers(const W2bParams &p, long long max_positions, bool loss, hipStream_t s, int grid = 0,   // grid workgroups = workers worker_base .. worker_base + grid
                              bool force_generic = false);
bool w2b_workers_lean(const W2bParams &p, bool force_generic);          // does w2b_launch_workers run the lean form of the kernel?
// sentence-resident variant (w2b_kernels_resident.hip): radius >= 0 when it can run for this shape
int w2b_resident_plan(int dim, int window, int negative);
bool w2b_resident_atomic_ok(const W2bParams &p, int radius);           // atomic_rank > 0: can the sentence-resident kernel do it?
long long w2b_resident_scratch_rows(int radius);                       // scratch rows per worker
hipError_t w2b_launch_resident(const W2bParams &p, long long max_positions, int radius, bool loss, hipStream_t s,
                               bool debug = false);
// row-group variant of the worker kernel (w2b_kernels_groups.hip): short rows / few workers, every row shared
bool w2b_groups_ok(const W2bParams &p);                                 // can it run this shape / these row rules?
size_t w2b_groups_lds_bytes(int dim, int window, int negative);
int w2b_groups_per_cu(const W2bParams &p, bool loss);                   // resident workgroups per CU
hipError_t w2b_launch_groups(const W2bParams &p, long long max_positions, bool loss, hipStream_t s);
hipError_t w2b_launch_refresher(const W2bParams &p, hipStream_t s);        // k_refresh_rows, beside a launch of the row-group kernel
#define W2B_RC_MAX 64               // most rows of u with refreshed read copies
#define W2B_RC_BLOCKS 16            // refresher workgroups started per launch (one per XCD claims its copy, the others leave)
int w2b_workers_per_cu(const W2bParams &p, bool loss);                  // resident workgroups per CU, plain kernel
int w2b_resident_per_cu(const W2bParams &p, int radius, bool loss);     // ... sentence-resident kernel
hipError_t w2b_launch_init_net(float *u, float *v, long long n_per_table, const float *lut,
                               hipStream_t s);
hipError_t w2b_launch_export(const float *u, const float *v, float *out, long long n, int bitlevel,
                             hipStream_t s);
hipError_t w2b_launch_export_packed(const float *u, const float *v, unsigned long long *out, long long rows, int dim,
                                    int bitlevel, hipStream_t s);      // bitlevel 1 / 2: include/word2bits_corpus.h layout
// analogy evaluator (w2b_kernels_eval.hip; ref src/compute-accuracy.c:106-110,155-177)
hipError_t w2b_launch_eval_normalize(float *M, long long words, long long size, long long ld, int bitlevel,
                                     int fused, float *len_scratch, hipStream_t s);
hipError_t w2b_launch_eval_queries(const float *M, long long ld, long long nq, const int *b1, const int *b2,
                                   const int *b3, float *Q, int variant, hipStream_t s);
hipError_t w2b_launch_eval_scores(const float *Q, const float *M, int nq, int words, int size, int ld, int fused,
                                  const int *b1, const int *b2, const int *b3, unsigned long long *best,
                                  int variant /* 0: vector-ALU kernel always; else MFMA when fused */, hipStream_t s);
// top-k form of the scan (ref :155-177 with N = k).  Per question: `nunits` slots of `cap` keys (`keys`), one byte per
// slot (`cnt`, zeroed by the caller), k bucket keys (`bkt`, zeroed) and the bound (`bound`, zeroed); w2b_eval_topk_layout
// gives nunits and cap.  out[q * k + j] = the j-th best key (score bits << 32 | ~row), 0 when fewer rows qualify.
void w2b_eval_topk_layout(long long words, int k, bool mfma, int *nunits, int *cap);
hipError_t w2b_launch_eval_topk(const float *Q, const float *M, int nq, int words, int size, int ld, int fused,
                                const int *b1, const int *b2, const int *b3, int k, unsigned long long *bound,
                                unsigned long long *bkt, unsigned long long *keys, unsigned char *cnt,
                                unsigned long long *out, int variant, hipStream_t s);
// the same scan on bit-packed 1-bit rows (w2b_kernels_evalbits.hip).  B = [words][nw] 32-bit halves of the packed rows
// (nw = 2 * ceil(dim / 64)), P = the questions' planes [2 * nw][nqp].  Keys are (uint32)I << 32 | ~row, 0 = no row.
hipError_t w2b_launch_bits_planes(const uint32_t *B, int nw, int dim, int nq, long long nqp, const int *b1, const int *b2,
                                  const int *b3, uint32_t *P, hipStream_t s);
void w2b_bits_layout(long long words, long long nq, int topk, int max_splits, int *splits, int *rows_per_split);
hipError_t w2b_launch_bits_top1(const uint32_t *B, int words, int dim, const uint32_t *P, long long nqp, int nq,
                                const int *b1, const int *b2, const int *b3, unsigned long long *best /* zeroed */,
                                hipStream_t s);
hipError_t w2b_launch_bits_topk(const uint32_t *B, int words, int dim, const uint32_t *P, long long nqp, int nq,
                                const int *b1, const int *b2, const int *b3, int k, int splits, int rows_per_split,
                                unsigned long long *slots /* [nq][splits][k] */, unsigned long long *out /* [nq][k] */,
                                hipStream_t s);
// the merge of the bits top-k form alone: out[q * k + j] = the j-th largest of the question's n = splits * k keys in `slots`
hipError_t w2b_launch_bits_merge(const unsigned long long *slots, int n, int k, int nq, unsigned long long *out,
                                 hipStream_t s);
// The signed multi-word question (w2b_kernels_evalcombine.hip; include/word2bits_eval.h, w2b_eval_combine).  rows / signs =
// [nq][W2B_EVAL_XSTRIDE]: the used slots first, in slot order (sign +1 / -1), then row -1 / sign 0; the rows are also the
// question's exclusion list.  fp32: Q as w2b_launch_eval_queries leaves it, then the list form of the top-k scan.
// bits: P = the questions' FOUR planes [4 * nw][nqp], then the scan into `slots` ([nq][splits][k]) and the merge into `out`;
// splits and rows_per_split from w2b_bits_layout(topk = 1).
#define W2B_EVAL_XSTRIDE 8          // ints per question: W2B_EVAL_MAX_TERMS = 7 slots and one that is always unused
hipError_t w2b_launch_combine_queries(const float *M, long long ld, long long nq, const int *rows, const int *signs,
                                      float *Q, hipStream_t s);
hipError_t w2b_launch_eval_topk_list(const float *Q, const float *M, int nq, int words, int size, int ld, int fused,
                                     const int *rows, int k, unsigned long long *bound, unsigned long long *bkt,
                                     unsigned long long *keys, unsigned char *cnt, unsigned long long *out, int variant,
                                     hipStream_t s);
hipError_t w2b_launch_combine_planes(const uint32_t *B, int nw, int dim, int nq, long long nqp, const int *rows,
                                     const int *signs, uint32_t *P, hipStream_t s);
hipError_t w2b_launch_combine_bits(const uint32_t *B, int words, int dim, const uint32_t *P, long long nqp, int nq,
                                   const int *rows, int k, int splits, int rows_per_split, unsigned long long *slots,
                                   unsigned long long *out, hipStream_t s);
// the merge of the top-k form alone: out[q * k + j] from the slots `keys` / `cnt` that a scan has filled
hipError_t w2b_launch_eval_topk_merge(unsigned long long *keys, unsigned char *cnt, int nunits, int cap, int k, int nq,
                                      unsigned long long *out, hipStream_t s);
// the same scan on bit-packed 2-bit rows (w2b_kernels_evalcodes.hip).  B = [words][nw] 32-bit halves of the packed rows
// (nw = 4 * ceil(dim / 64)), wrow = w(c) per row ([rows_padded], a multiple of 256 rows, 0 past the vocabulary; wtab =
// w by n3, dim + 1 floats), T / Wq = the questions' int8 operands (w2b_codes_operand_bytes) and weights [3][32 * ceil(nq / 32)].
// Keys are score bits << 32 | ~row, 0 = no row.  k = 0: `best` (zeroed) receives the best key of each question; k >= 1:
// `best` is the bound and bkt / keys / cnt the selection state of w2b_launch_eval_topk (zeroed alike, sized by
// w2b_codes_topk_layout), out[q * k + j] the j-th best key.
#define W2B_CODES_KS_MAX 38         // K steps of 32 columns that a wavefront keeps in registers (1216 columns)
size_t w2b_codes_operand_bytes(int dim, long long nq);
void w2b_codes_topk_layout(long long words, int dim, int k, int *nunits, int *cap);
hipError_t w2b_launch_codes_roww(const uint32_t *B, int dim, long long words, long long rows_padded, const float *wtab,
                                 float *wrow, hipStream_t s);
hipError_t w2b_launch_codes_operands(const uint32_t *B, int dim, int nq, const float *wrow, const int *b1, const int *b2,
                                     const int *b3, void *T, float *Wq, hipStream_t s);
hipError_t w2b_launch_codes_scan(const uint32_t *B, int words, int dim, const float *wrow, const void *T, const float *Wq,
                                 int nq, const int *b1, const int *b2, const int *b3, int k, unsigned long long *best,
                                 unsigned long long *bkt, unsigned long long *keys, unsigned char *cnt,
                                 unsigned long long *out, hipStream_t s);
// The 3CosMul question on bit-packed rows (include/word2bits_eval.h, "3CosMul").  2-bit rows: the COSMUL instance of the
// codes scan, with the arguments of w2b_launch_codes_scan's top-k form (k >= 1).  1-bit rows (w2b_kernels_evalcosmul.hip):
// utab = u by agreement count, dim + 1 floats ((float)A / (float)dim); the scan into `slots` ([nq][splits][k]) and the merge
// into `out`, splits and rows_per_split from w2b_bits_layout(topk = 1).  Keys are score bits << 32 | ~row, 0 = no row.
hipError_t w2b_launch_codes_scan_cosmul(const uint32_t *B, int words, int dim, const float *wrow, const void *T,
                                        const float *Wq, int nq, const int *b1, const int *b2, const int *b3, int k,
                                        unsigned long long *bound, unsigned long long *bkt, unsigned long long *keys,
                                        unsigned char *cnt, unsigned long long *out, hipStream_t s);
hipError_t w2b_launch_cosmul_bits(const uint32_t *B, int words, int dim, const float *utab, int nq, const int *b1,
                                  const int *b2, const int *b3, int k, int splits, int rows_per_split,
                                  unsigned long long *slots, unsigned long long *out, hipStream_t s);
// The rank of a given row on bit-packed rows (include/word2bits_eval.h, "rank of a given row"): the arguments of the top-1
// forms (P / T / Wq as w2b_launch_bits_planes / w2b_launch_codes_operands leave them) and the questions' target rows.  cnt
// [nq] (ZEROED by the caller) receives (rows with exactly the target's score << 32 | rows that stand before the target),
// counted over ALL rows; corr [nq][2] receives what the question's own rows and the target itself added to (before, equal),
// tscore [nq] the target's score (1-bit rows: the integer I; 2-bit rows: the float), 0 when the target has no rank.  Each is
// two launches: one lane per question for the target's score and corr, then the scan.
hipError_t w2b_launch_bits_rank(const uint32_t *B, int words, int dim, const uint32_t *P, long long nqp, int nq,
                                const int *b1, const int *b2, const int *b3, const int *target, unsigned long long *cnt,
                                unsigned int *corr, int *tscore, unsigned int *tacc /* [nq][2] scratch */, hipStream_t s);
hipError_t w2b_launch_codes_rank(const uint32_t *B, int words, int dim, const float *wrow, const void *T, const float *Wq,
                                 int nq, const int *b1, const int *b2, const int *b3, const int *target, float *tscore,
                                 unsigned int *corr, unsigned long long *cnt, hipStream_t s);
// The bag question on bit-packed rows (w2b_kernels_evalbag.hip; include/word2bits_eval.h, "bag questions").  bitlevel 1: B =
// the 1-bit rows (nw = 2 * ceil(dim / 64) halves), 2: the 2-bit rows and wrow as above.  ids / off = the chunk's bags, off
// [nq + 1] rebased to ids[0]; T = the two digit planes of the pooled vectors in fragment order (w2b_bag_operand_bytes, ZEROED
// by the caller), NT[nq] (zeroed; bitlevel 2 only) receives sum_a T[a]^2.  The scan: Wq = the questions' weights [32 *
// ceil(nq / 32)] (bitlevel 2; 0 = no answers), xrows / xoff = every question's own rows, ascending without repeats, and
// their bounds [nq + 1], or xoff = nullptr when nothing is excluded; bound / bkt / keys / cnt = the zeroed selection state
// sized by w2b_codes_topk_layout, out[q * k + j] the j-th best key (score bits << 32 | ~row; bitlevel 1: score bits = J).
size_t w2b_bag_operand_bytes(int dim, long long nq);
hipError_t w2b_launch_bag_operands(const uint32_t *B, int dim, int bitlevel, int nq, const int *ids, const int *off, void *T,
                                   unsigned long long *NT, hipStream_t s);
hipError_t w2b_launch_bag_scan(const uint32_t *B, int words, int dim, int bitlevel, const float *wrow, const void *T,
                               const float *Wq, int nq, const int *xrows, const int *xoff, int k, unsigned long long *bound,
                               unsigned long long *bkt, unsigned long long *keys, unsigned char *cnt, unsigned long long *out,
                               hipStream_t s);
// The float-vector question on bit-packed rows (w2b_kernels_evalvec.hip; include/word2bits_eval.h, "vector questions").  B =
// the packed rows as 64-bit words, [words][bitlevel * ceil(dim / 64)]; x = the questions [nq][dim] on the device; X = their
// operands in fragment order (w2b_vec_operand_bytes; the operand kernel writes every byte of it).  The scan: wrow as above
// (bitlevel 2) or wconst = the weight of every 1-bit row; Wx = the questions' weights [w2b_vec_weight_slots(nq)], 0 for a
// question without answers and in the slots past nq; bound / bkt / keys / cnt = the zeroed selection state sized by
// w2b_vec_topk_layout, out[q * k + j] the j-th best key (score bits << 32 | ~row).
size_t w2b_vec_operand_bytes(int dim, long long nq);
long long w2b_vec_weight_slots(long long nq);
void w2b_vec_topk_layout(long long words, int k, int *nunits, int *cap);
hipError_t w2b_launch_vec_operands(const float *x, int dim, int nq, void *X, hipStream_t s);
hipError_t w2b_launch_vec_scan(const uint64_t *B, int words, int dim, int bitlevel, const float *wrow, float wconst,
                               const void *X, const float *Wx, int nq, int k, unsigned long long *bound,
                               unsigned long long *bkt, unsigned long long *keys, unsigned char *cnt, unsigned long long *out,
                               hipStream_t s);
// The document question on bit-packed rows (w2b_kernels_evaldocs.hip; include/word2bits_eval.h, "documents").  A chunk of nq
// queries is tcols columns: query q owns columns qcol[q] .. qcol[q + 1) (a multiple of 16), the first qm[q] of them carry its
// ids >= 0, colrow[x] = the row of column x or -1 for a pad column.  Table: Tab [words][tcols] (int32 I / float32 cos) and
// Rmax [words][nq] (the largest value of a row over a query's own columns); every element is written.  Walk: ids / off = the
// corpus WITHOUT its padding ids (off [n_docs + 1]); slots [nq][ceil(n_docs / W2B_DOCS_PER_BLOCK)][k] receives every
// workgroup's k best keys, out[q * k + j] the j-th best key (score bits << 32 | ~document), all_scores (or null) [nq][n_docs].
#define W2B_DOCS_PER_BLOCK 1024     // documents of one walk workgroup
hipError_t w2b_launch_docs_table(const uint32_t *B, int words, int dim, int bitlevel, const float *wrow, const int *colrow,
                                 int tcols, const int *qcol, const int *qm, int nq, void *Tab, void *Rmax, hipStream_t s);
hipError_t w2b_launch_docs_walk(const void *Tab, const void *Rmax, int tcols, int nq, int dim, int bitlevel, const int *qcol,
                                const int *qm, const int *ids, const long long *off, long long n_docs, int symmetric, int k,
                                unsigned long long *slots, unsigned long long *out, float *all_scores, hipStream_t s);
// The pair question on bit-packed rows (w2b_kernels_evalpairs.hip; include/word2bits_eval.h, "pair similarity").  B = the
// packed rows as 64-bit words, [words][bitlevel * ceil(dim / 64)]; ids / off = a chunk of pairs, off [2 n + 1] rebased to ids[0]:
// bag 2 q is side A of pair q, bag 2 q + 1 side B; every id is < words (ids < 0 are padding), and words > 0.  list = the chunk's
// pairs sorted by path, n_one + n_short + n_long = n of them, the path of a pair being w2b_pairs_path of its bounds (ids = the
// chunk's ids, host memory).  parts [n][3] receives J, N_A, N_B of every pair; every element is written.
#define W2B_PAIRS_LONG_IDS 256      // a pair of more ids than this, padding included, gets a workgroup of its own
#define W2B_PAIRS_PATH_ONE 0
#define W2B_PAIRS_PATH_SHORT 1
#define W2B_PAIRS_PATH_LONG 2
int w2b_pairs_path(int bitlevel, const int *ids, long long a0, long long a1, long long b1);
hipError_t w2b_launch_pairs(const uint64_t *B, int dim, int bitlevel, const int *ids, const int *off, const int *list,
                            int n_one, int n_short, int n_long, long long *parts, hipStream_t s);
// the packed embedding layer (w2b_kernels_embed.hip; include/word2bits_embed.h).  T = the packed table [rows][wpr], ids /
// offsets = int64 device buffers, `bad` = the device counter of ignored ids and clamped bags.  A bag launch needs
// w2b_embed_bag_scratch(...) bytes of device scratch (it zeroes them itself).
#define W2B_EMBED_SPLIT 1024        // ids of a bag that one workgroup pools; longer bags are split into segments of this length
hipError_t w2b_launch_embed_lookup(const uint64_t *T, long long rows, int dim, int bitlevel, const long long *ids, long long n,
                                   int dtype, void *out, unsigned long long *bad, hipStream_t s);
long long w2b_embed_bag_scratch(long long n_ids, long long n_bags, int dim, int *cap_out);
hipError_t w2b_launch_embed_bag(const uint64_t *T, long long rows, int dim, int bitlevel, const long long *ids, long long n_ids,
                                const long long *offsets, long long n_bags, int mode, int dtype, void *out,
                                unsigned long long *bad, void *scratch, hipStream_t s);
// weighted bags: `weights` = float device buffer beside ids; w2b_embed_bagw_scratch(...) bytes of scratch, of which the
// launch zeroes the first *head_bytes itself
long long w2b_embed_bagw_scratch(long long n_ids, long long n_bags, int dim, int *cap_out, long long *segcap_out,
                                 long long *head_bytes);
hipError_t w2b_launch_embed_bag_weighted(const uint64_t *T, long long rows, int dim, int bitlevel, const long long *ids,
                                         const float *weights, long long n_ids, const long long *offsets, long long n_bags,
                                         int mode, int dtype, void *out, unsigned long long *bad, void *scratch, hipStream_t s);
// the projection (w2b_kernels_embedproj.hip; include/word2bits_embed.h, "Projection"): x = the vectors [n][dim] on the device,
// cand = int64 candidate rows [m] or nullptr, then candidate j is row cand_base + j; X = w2b_embed_project_operand_bytes(dim, n)
// bytes of operand staging (written by the launch itself); out = dense [n][m] of dtype.  Two kernels: the operands, the product.
size_t w2b_embed_project_operand_bytes(int dim, long long n);
hipError_t w2b_launch_embed_project(const uint64_t *T, long long rows, int dim, int bitlevel, const float *x, int n,
                                    const long long *cand, long long cand_base, int m, int dtype, void *X, void *out,
                                    unsigned long long *bad, hipStream_t s);
// the back-projection (w2b_kernels_embedback.hip; include/word2bits_embed.h, "Back-projection"): g = [n][.] on the device, ldg
// floats between two vectors; the m candidate positions of a launch begin a segment, position j is row cand[j] or, when cand
// is nullptr, cand_base + j; first / last = the positions begin / end the call's whole list (S is carried in dx between
// launches).  w2b_embed_backproject_plan chooses the path and the scratch (at most 64 MiB, whatever m is) for n vectors.
void w2b_embed_backproject_plan(int dim, long long n, long long m, int *use_scratch, int *segs, long long *scratch_bytes);
hipError_t w2b_launch_embed_backproject(const uint64_t *T, long long rows, int dim, int bitlevel, const float *g,
                                        long long ldg, long long n, const long long *cand, long long cand_base, int m,
                                        int first, int last, float *dx, int use_scratch, int segs, void *part,
                                        unsigned long long *bad, hipStream_t s);
// the cross-entropy (w2b_kernels_embedxent.hip; include/word2bits_embed.h, "Cross-entropy").  X = the operand staging of ALL the
// call's vectors (w2b_launch_vec_operands); a launch takes the vectors v0 .. v1 of it.  clean = the call's candidates with ids
// >= rows made padding by w2b_launch_embed_xent_clean (nullptr: every row, m == rows); target = int64 [n].  Statistics: Mseg /
// Useg = [ceil(m / W2B_EMBED_XSEG)][v1 - v0], tl = [n].  Finishing: mx / se / tl / teff = [n], teff the effective target (-1 =
// ignored).  Gradient: the candidate positions jbase .. jbase + m of the call, g = dense [v1 - v0][m].
hipError_t w2b_launch_embed_xent_clean(const long long *cand, long long m, long long rows, long long *clean,
                                       unsigned long long *bad, hipStream_t s);
hipError_t w2b_launch_embed_xent_stats(const uint64_t *T, long long rows, int dim, int bitlevel, const void *X, int v0, int v1,
                                       const long long *clean, int m, const long long *target, float *Mseg,
                                       unsigned long long *Useg, float *tl, hipStream_t s);
hipError_t w2b_launch_embed_xent_finish(int v0, int v1, long long m, int nseg, const float *Mseg, const unsigned long long *Useg,
                                        const long long *clean, const long long *target, float *mx, float *se, float *tl,
                                        long long *teff, unsigned long long *bad, hipStream_t s);
hipError_t w2b_launch_embed_xent_grad(const uint64_t *T, long long rows, int dim, int bitlevel, const void *X, int v0, int v1,
                                      const long long *clean, long long jbase, int m, const float *mx, const float *se,
                                      const long long *teff, float *g, hipStream_t s);
// the top-k selection (w2b_kernels_embedtopk.hip; include/word2bits_embed.h, "Top-k").  X and clean as for the cross-entropy; one
// call takes the vectors v0 .. v1 against all m candidate positions through its four kernels.  Scratch for v1 - v0 vectors, all
// written before it is read: umax = [.][ceil(m / 64)] keys, thr = [.] keys, count = [.], list = [.][64 k] keys.  vals / pos =
// dense [n][k] of the call; with m == 0 it writes empty lists and touches neither umax nor list.
hipError_t w2b_launch_embed_topk(const uint64_t *T, long long rows, int dim, int bitlevel, const void *X, int v0, int v1,
                                 const long long *clean, int m, int k, unsigned long long *umax, unsigned long long *thr,
                                 unsigned int *count, unsigned long long *list, float *vals, long long *pos, hipStream_t s);
// bit-packed model files (w2b_corpus.cpp; format in include/word2bits_corpus.h)
#include <string>
#include <vector>
bool w2b_internal_is_packed(const unsigned char *d, size_t n);
int w2b_internal_parse_packed(const unsigned char *d, size_t n, std::vector<std::string> &words, std::vector<float> &values,
                              int64_t *dim_out);
// header and vocabulary only: the rows stay packed at d + *data_pos (vocab_size x w2b_packed_words_per_row words, unaligned)
int w2b_internal_parse_packed_head(const unsigned char *d, size_t n, std::vector<std::string> &words, int64_t *dim_out,
                                   int *bitlevel_out, size_t *data_pos);
int w2b_internal_fail(int code, const char *msg);   // sets w2b_last_error() (w2b_trainer.cpp)
struct w2b_trainer;
// what the evaluator needs from a live trainer (w2b_trainer.cpp): device tables, shape, bitlevel, device, stream
void w2b_internal_trainer_view(w2b_trainer *t, float **u, float **v, long long *V, long long *D, int *bitlevel,
                               int *device, hipStream_t *stream);
// per-XCD copies of the hottest rows meet their master rows (before / after every training launch; idempotent)
hipError_t w2b_launch_xhot_fold(const W2bParams &p, hipStream_t s);
hipError_t w2b_launch_wca_pack(const W2bShared *sh, unsigned long long *buf, hipStream_t s);   // buf[0] = local word count
hipError_t w2b_launch_wca_unpack(W2bShared *sh, const unsigned long long *buf, hipStream_t s); // from buf[1] = global sum
// replica exchange, one chunk (w2b_kernels_misc.hip): d = s = w - base;  w += a * s - d, base += a * s
hipError_t w2b_launch_xchg_delta(float *w, const float *base, float *d, float *s_, long long n, hipStream_t s);
hipError_t w2b_launch_xchg_apply(float *w, float *base, const float *d, const float *s_, float a, long long n,
                                 const float *fac /* per-row factors on the sum (k_xchg_factor) or nullptr */, long long first, int dim,
                                 int bitlevel, int cells /* 1: per element the whole sum where it stays in the safe step's quantization cell */,
                                 hipStream_t s);
// cnt[2 V]: contributors per row (in) -> factor on the summed delta (out); rule 0 exponential saturation (rate = expected updates
// per centre word), 1 hard threshold
hipError_t w2b_launch_xchg_factor(float *cnt, const float *rate, float words, float tau_u, float tau_v, long long V, int rule,
                                  int sat_u, int sat_v, hipStream_t s);
hipError_t w2b_launch_xchg_touched(const float *w, const float *base, float *cnt, long long rows, int dim, hipStream_t s);
