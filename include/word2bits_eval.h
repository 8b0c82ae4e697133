/*
 * word2bits_eval.h -- C ABI of the MI355X analogy evaluator (the consumer of the trained vectors file).
 *
 * Replaces the reference's evaluator program, src/compute-accuracy.c (`compute_accuracy <FILE> <bitlevel>
 * <threshold> < questions-words.txt`), whose whole cost is the exhaustive scan of ref :158-177: for every
 * question a [1 x D] . [D x V] product over the normalised matrix followed by a strict-greater arg-max.
 * On the GPU that scan is one batched fp32 product (all questions x all rows) with the arg-max fused into its
 * epilogue (word2bits_amd/csrc/w2b_kernels_eval.hip): on the matrix cores (f32 MFMA = sequential fmaf chains,
 * bit for bit) in fused mode, on the vector ALU (packed mul + add) in the two-rounding mode.
 *
 * Parity contract: answers -- and therefore the stdout transcript -- are IDENTICAL to the reference's, ties
 * included.  Every score is accumulated in the reference's order (a = 0 .. size-1, one accumulator per
 * (question,row) pair), candidates tie-break to the lowest row, and `fused` selects the arithmetic of the build
 * being replaced: 1 = `acc += a*b` is one fused multiply-add (what the reference's Makefile:6 flags,
 * -O3 -march=native, produce on any FMA-capable x86), 0 = two roundings (-ffp-contract=off).  The two builds of
 * the unmodified reference disagree with each other on tie-heavy 1-bit vectors; each mode matches its build.
 *
 * No CPU fallback: W2B_ENOGPU when no device is visible.  Error codes and w2b_last_error() are those of
 * word2bits_hip.h.
 */
#ifndef WORD2BITS_EVAL_H
#define WORD2BITS_EVAL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct w2b_eval w2b_eval;

/* ref src/compute-accuracy.c:80-112: read "<words> <size>", cap words at `threshold` (0 = off, ref :86), read
 * each row (word up to the first ' ', '\n' bytes dropped, at most max_w = 50 characters kept, upper-cased; then
 * `size` raw float32), apply quantize(x, bitlevel) (ref :26-61,106) and divide the row by its length
 * (ref :107-110; float accumulation in column order, a zero row becomes NaN as in the reference).
 * W2B_EIO when the file cannot be opened ("Input file not found", ref :81-84). */
int w2b_eval_load(const char *file, int32_t bitlevel, int64_t threshold, int32_t fused, int32_t device,
                  w2b_eval **out);
void w2b_eval_free(w2b_eval *e);

/* The evaluator on a live trainer (include/word2bits_hip.h), without the file round trip: exactly what
 * w2b_eval_load(file, bitlevel, threshold, ...) would hold after the trainer's vectors had been written to `file` in
 * the binary format (quantize(u+v) with the trainer's bitlevel, ref src/word2bits.cpp:565-574) -- the values stay
 * on the device, `words[i]` is the vocabulary word of row i (w2b_corpus_word), n_words = vocab_size. */
struct w2b_trainer;
int w2b_eval_from_trainer(struct w2b_trainer *t, int64_t n_words, const char *const *words, int32_t bitlevel,
                          int64_t threshold, int32_t fused, w2b_eval **out);

int64_t w2b_eval_words(const w2b_eval *e);                  /* `words` after the threshold, ref :85-86 */
int64_t w2b_eval_size(const w2b_eval *e);                   /* `size`, ref :87 */
const char *w2b_eval_word(const w2b_eval *e, int64_t row);  /* &vocab[row * max_w], ref :99-104 */
/* ref :140-145,152: first row whose upper-cased word equals `upper_word`, or w2b_eval_words() if none */
int64_t w2b_eval_lookup(const w2b_eval *e, const char *upper_word);
/* the normalised matrix M of ref :106-110, [words][size] (parity tests) */
int w2b_eval_get_matrix(w2b_eval *e, float *out);

/* ref :155-177 with N = 1, for `nq` questions at once: vec = (M[b2] - M[b1]) + M[b3]; best[q] = the first row c
 * (c != b1,b2,b3) whose score  sum_a vec[a] * M[c][a]  is the largest one > 0, bestd[q] = that score;
 * best[q] = -1, bestd[q] = 0 when no row scores above 0.  bestd may be NULL. */
int w2b_eval_top1(w2b_eval *e, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3,
                  int32_t *best, float *bestd);

/* ref :155-177 with N = k (the reference ships N = 1): per question the k best rows in the reference's order -- score
 * descending, equal scores in ascending row order (the strict-greater insertion of ref :167) -- among the rows other
 * than b1, b2, b3 whose score is > 0.  best[q*k + j], bestd[q*k + j], j = 0..k-1; a list of fewer than k rows ends in
 * row -1 / score 0 (ref :164-165).  bestd may be NULL.  Scores are the bits w2b_eval_top1 produces, and k = 1 returns
 * exactly what w2b_eval_top1 returns.  1 <= k <= W2B_EVAL_MAX_K, else W2B_EINVAL. */
#define W2B_EVAL_MAX_K 64
int w2b_eval_topk(w2b_eval *e, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3, int32_t k,
                  int32_t *best, float *bestd);
/* The neighbours of a word: vec = M[row], only `row` is skipped.  Equals w2b_eval_topk(b1 = b2 = b3 = rows). */
int w2b_eval_neighbors(w2b_eval *e, int64_t nq, const int32_t *rows, int32_t k, int32_t *best, float *bestd);
/* The general form of both: a question is a sum of signed rows (word2vec's `distance` on a phrase; gensim's
 * most_similar(positive, negative)).  rows / signs are [nq][nt], 1 <= nt <= W2B_EVAL_MAX_TERMS; a slot with sign 0 is unused
 * and its row is ignored.  The same row may stand in several slots: its coefficients add.  Every used slot's row is
 * excluded from that question's answers.  best / bestd are [nq][k] and have the shape of w2b_eval_topk's: best first,
 * equal scores in ascending row order, a short list ends in row -1 / score 0; bestd may be NULL.
 *   fp32 handle: the used slots in slot order; vec[a] starts as M[r0][a] (sign +1) or its exact negation (sign -1), every
 *     further slot is ONE float32 add or subtract of M[rt][a], rounded on its own; the score of row c is the chain that
 *     w2b_eval_top1 runs on that vec (the handle's `fused` mode and w2b_eval_set_kernel variant); answers are the rows
 *     with score > 0.  So slots (+b2, -b1, +b3) give bit for bit what w2b_eval_topk(b1, b2, b3) gives, and one slot (+r)
 *     what w2b_eval_neighbors gives.
 *   bits handle: t[a] = sum over the used slots of sign * s_r[a], an integer in [-nt, nt], zero included;
 *     I(c) = sum_a t[a] * s_c[a], exact; answers are the rows with I > 0, by I descending then row ascending, score
 *     (float)I / (float)size.  Slots (+b2, -b1, +b3) again equal w2b_eval_topk exactly.
 *   codes handle: W2B_EINVAL ("not available in codes mode").  Deliberately: the 2-bit scan keeps three accumulator tiles
 *     per (question, row) next to 104-152 registers of unpacked rows, and a per-question number of terms does not fit that
 *     shape without another kernel design.  (w2b_eval_bag below is that design for sums without signs.)
 * W2B_EINVAL, with the cause in w2b_last_error(): nt outside 1..W2B_EVAL_MAX_TERMS, k outside 1..W2B_EVAL_MAX_K, a sign
 * other than -1, 0, +1, a used slot's row outside [0, words), a question without a used slot.
 * w2b_eval_timing_read counts these launches like the top-k ones, and w2b_eval_set_topk_scratch bounds their scratch. */
#define W2B_EVAL_MAX_TERMS 7
int w2b_eval_combine(w2b_eval *e, int64_t nq, int32_t nt, const int32_t *rows, const int8_t *signs, int32_t k,
                     int32_t *best, float *bestd);
/* Upper bound in bytes for the device scratch (candidate slots) of one top-k launch; 0 = the default, 1 GiB.  The
 * questions are scored in chunks that fit, never smaller than 128 questions.  Results never depend on it. */
int w2b_eval_set_topk_scratch(w2b_eval *e, int64_t bytes);

/* The text form of ./nearest.  Every line of `queries[0..len)` is split on white space and upper-cased (C locale):
 *   one word W        the neighbours of W                    three words A B C    the analogy (B - A) + C
 * and answered by "<words joined by one space>:\n" followed by one line "<rank>\t<word>\t<score %.6f>\n" per result
 * (rank from 1; a short list simply ends).  Empty lines are skipped; any other number of words gives
 * "<words>: expected 1 or 3 words\n", a word that w2b_eval_lookup does not find "<words>: not in vocabulary: <WORD>\n"
 * (the first such word).  All lines are scored in one w2b_eval_topk batch.  *out is malloc'ed; release it with
 * w2b_eval_free_text. */
int w2b_eval_nearest_text(w2b_eval *e, const char *queries, int64_t len, int32_t k, char **out, int64_t *out_len);

/* The text form of `./nearest ... signed`: every non-empty line is 1 to W2B_EVAL_MAX_TERMS tokens +WORD, -WORD or WORD (a
 * bare word counts as +; only the first character of a token is read as a sign), the words upper-cased and looked up as in
 * w2b_eval_nearest_text: "new york", "+king -man +woman".  The answer has the format of w2b_eval_nearest_text; the head is
 * the tokens as given, upper-cased and joined by one space.  Error lines: "<head>: expected 1 to 7 signed words\n" and
 * "<head>: not in vocabulary: <WORD>\n" (the first such word, without its sign).  All valid lines are scored in one
 * w2b_eval_combine batch. */
int w2b_eval_combine_text(w2b_eval *e, const char *queries, int64_t len, int32_t k, char **out, int64_t *out_len);

/* ref :94,113-188: the program's stdout for the question stream `questions[0..len)` (what the reference reads
 * from stdin with scanf("%s")), including "Starting eval...".  *out is malloc'ed; release it with
 * w2b_eval_free_text. */
int w2b_eval_transcript(w2b_eval *e, const char *questions, int64_t len, char **out, int64_t *out_len);
void w2b_eval_free_text(char *text);

/* Which kernel scores the fused (FMA) mode: 1 (default) = the f32 MFMA kernel; 0 = the same fused chain on the vector ALU
 * (v_pk_fma_f32; a cross-check of the MFMA path); n > 1 = MFMA with n question tiles per row tile in the launch order.
 * The two-rounding mode always runs on the vector ALU.  (Round 2 read this from the environment.) */
int w2b_eval_set_kernel(w2b_eval *e, int32_t variant);

/* Device time (HIP events on the evaluator's stream) and launch count of the score kernel (top-1 and top-k; the
 * top-k time includes its merge kernel) since load or since the last call; `macs` = multiply-adds those launches performed (questions x padded rows x padded size). */
int w2b_eval_timing_read(w2b_eval *e, double *kernel_ms, int64_t *launches, double *macs);

/* ---- bits mode: the exact integer scan on bit-packed 1-bit vectors ------------------------------------------------
 * A 1-bit model is one sign per value and is stored that way (include/word2bits_corpus.h).  The same opaque w2b_eval in
 * a second mode keeps the rows packed on the device -- [words][ceil(size / 64)] 64-bit words, 1/32 of the float matrix
 * -- and scans them with xor + popcount (word2bits_amd/csrc/w2b_kernels_evalbits.hip).  All 1-bit rows have the same
 * length, so the cosine ranking is the ranking of the integer
 *     I(c) = sum_a (s_b2[a] - s_b1[a] + s_b3[a]) * s_c[a] = size - 2 * (H(b2,c) - H(b1,c) + H(b3,c))
 * where s_r[a] = -1 where the packed SIGN bit of row r, column a is set (quantize(x, 1) < 0) and +1 elsewhere, and H is
 * the Hamming distance over the `size` columns.  The answer list of a question: the rows c other than b1, b2, b3 with
 * I(c) > 0, by I descending, equal I in ascending row order, k of them, a short list ending in row -1 / score 0.  The
 * reported score is (float)I / (float)size, one correctly rounded division.  The fp32 modes above agree with this
 * ranking wherever I differs and order rows of equal I by rounding noise instead; a row with I == 0, which they
 * sometimes score as a tiny positive number, is never an answer here.
 * On a bits handle w2b_eval_top1 / _topk / _neighbors / _combine / _nearest_text / _combine_text / _transcript /
 * _set_topk_scratch / _timing_read (macs = questions x rows x size) work with these semantics, w2b_eval_set_kernel does nothing and
 * w2b_eval_get_matrix is W2B_EINVAL.
 * Two-bit models have the codes mode below: their rows differ in length, so the ranking needs a per-row float scale. */

/* FILE is a bit-packed .w2bp of bitlevel 1, read without expanding it (bitlevel 2: W2B_EINVAL, see w2b_eval_load_codes), or a file of the
 * reference's binary format, each value reduced to its sign by the bitlevel-1 rule of ref :26-61 (negative iff
 * num < 0: +0, -0 and NaN are positive).  `threshold` caps the rows as in w2b_eval_load; W2B_EIO "Input file not
 * found" when the file cannot be opened. */
int w2b_eval_load_bits(const char *file, int64_t threshold, int32_t device, w2b_eval **out);
/* The same on a live trainer at -bitlevel 1 (else W2B_EINVAL): the rows are packed on the device from u + v, no float
 * leaves it.  What w2b_eval_load_bits holds after the trainer's vectors have been written with -packed. */
int w2b_eval_bits_from_trainer(struct w2b_trainer *t, int64_t n_words, const char *const *words, int64_t threshold,
                               w2b_eval **out);
int32_t w2b_eval_is_bits(const w2b_eval *e);
/* the packed rows, [words][ceil(size / 64)] in the file's layout; W2B_EINVAL on a float handle */
int w2b_eval_get_bits(w2b_eval *e, uint64_t *out);
/* Host twin of the bits kernels (pure C, no device; for tests, as w2b_quantize is for the device quantizer): I(c) of the
 * question (b1, b2, b3) for EVERY row c of packed[words][ceil(dim / 64)], b1, b2, b3 included, into I_out[words]. */
int w2b_bits_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int64_t b1, int64_t b2, int64_t b3,
                         int32_t *I_out);

/* Host twin of the bits form of w2b_eval_combine (pure C, no device): I(c) of the question rows[nt] / signs[nt] for EVERY
 * row c of packed[words][ceil(dim / 64)], the question's own rows included, into I_out[words].  W2B_EINVAL as
 * w2b_eval_combine has it: nt outside 1..W2B_EVAL_MAX_TERMS, a sign other than -1, 0, +1, a used slot's row outside
 * [0, words), no used slot. */
int w2b_bits_combine_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t nt, const int32_t *rows,
                                 const int8_t *signs, int32_t *I_out);

/* ---- codes mode: the integer scan on bit-packed 2-bit vectors ------------------------------------------------------
 * A 2-bit value is t/4 with t in {-1, +1, -3, +3}: the SIGN bit set means negative, the MAGNITUDE bit set means 3 (0.75),
 * clear means 1 (0.25) -- exactly the .w2bp layout of include/word2bits_corpus.h, per 64 columns one sign word then one
 * magnitude word.  The same opaque w2b_eval in a third mode keeps the rows packed on the device, [words][2 * ceil(size /
 * 64)] 64-bit words, 1/16 of the float matrix, and scans them on the i8 matrix cores
 * (word2bits_amd/csrc/w2b_kernels_evalcodes.hip).  For row r:
 *     n3(r) = the number of magnitude bits set among the `size` columns,   N(r) = size + 8 * n3(r)   ( = 16 |r|^2 ),
 *     w(r)  = (float)(1.0 / sqrt((double)N(r)))    -- the double square root and the double division each correctly
 *             rounded, the result rounded to float; w depends on n3 alone: a host-built table of size + 1 floats.
 * For rows x, c:  J(x, c) = sum_a t_x[a] * t_c[a] over the `size` columns, an exact integer, |J| <= 9 * size.
 * The score of row c for the question (b1, b2, b3), in float32, every operation rounded to nearest on its own and
 * nothing contracted into an FMA:
 *     p1 = (float)J(b1,c) * w(b1);  p2 = (float)J(b2,c) * w(b2);  p3 = (float)J(b3,c) * w(b3);
 *     score = ((p2 - p1) + p3) * w(c);
 * (the reference's (M[b2] - M[b1]) + M[b3] order with normalised rows; with b1 = b2 = b3 = r it reduces exactly to
 * ((float)J(r,c) * w(r)) * w(c), so w2b_eval_neighbors stays equal to w2b_eval_topk(rows, rows, rows)).
 * The answer list of a question: the rows c other than b1, b2, b3 with score > 0, by score descending, equal float
 * scores in ascending row order, k of them, a short list ending in row -1 / score 0 -- the key of the fp32 path,
 * score bits << 32 | ~row.  The fp32 modes agree with this ranking wherever two scores differ by more than the fp32
 * path's accumulated rounding error.
 * On a codes handle w2b_eval_top1 / _topk / _neighbors / _nearest_text / _transcript / _set_topk_scratch / _timing_read
 * (macs = 3 x questions x rows x size) work with these semantics, w2b_eval_set_kernel does nothing, w2b_eval_get_matrix
 * and w2b_eval_get_bits are W2B_EINVAL, and w2b_eval_is_bits is 0. */

/* FILE is a bit-packed .w2bp of bitlevel 2, read without expanding it (bitlevel 1: W2B_EINVAL, see w2b_eval_load_bits),
 * or a file of the reference's binary format, each value reduced by the bitlevel-2 rule of ref :26-61 (negative iff
 * num < 0; magnitude .25 iff |num| <= .5, else .75: NaN becomes +.75, +0 and -0 become +.25).  `threshold` and "Input
 * file not found" as in w2b_eval_load_bits. */
int w2b_eval_load_codes(const char *file, int64_t threshold, int32_t device, w2b_eval **out);
/* The same on a live trainer at -bitlevel 2 (else W2B_EINVAL): the rows are packed on the device from u + v.  What
 * w2b_eval_load_codes holds after the trainer's vectors have been written with -packed. */
int w2b_eval_codes_from_trainer(struct w2b_trainer *t, int64_t n_words, const char *const *words, int64_t threshold,
                                w2b_eval **out);
int32_t w2b_eval_is_codes(const w2b_eval *e);
/* the packed rows, [words][2 * ceil(size / 64)] in the file's layout; W2B_EINVAL on any other handle */
int w2b_eval_get_codes(w2b_eval *e, uint64_t *out);
/* Host twin of the codes kernels (pure C, no device): for the question (b1, b2, b3) and EVERY row c of
 * packed[words][2 * ceil(dim / 64)], b1, b2, b3 included, J_out[3][words] = J(b1,c), J(b2,c), J(b3,c) and
 * score_out[words] = the float score.  Either output may be NULL. */
int w2b_codes_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int64_t b1, int64_t b2, int64_t b3,
                          int32_t *J_out, float *score_out);

/* ---- bag questions: the rows nearest to a pooled bag of rows, on both packed modes ----------------------------------
 * "Which words are nearest to this sentence, this ten-word phrase, this document?"  A question is a BAG of rows, pooled as
 * w2b_embed_bag pools it in SUM mode (include/word2bits_embed.h): the unnormalised integer vector
 *     T[a] = sum over the bag's ids r >= 0 of t_r[a],   t = +-1 on a bits handle, t in {+-1, +-3} on a codes handle
 * -- the same row several times adds; |T[a]| <= 3 * W2B_EVAL_MAX_BAG = 12288 -- and scored against every row c by
 *     J(c) = sum_a T[a] * t_c[a]  over the `size` columns, exact,  |J| <= 9 * 4096 * size.
 * A handle with 9 * 4096 * size >= 2^31 (size > 58254) is W2B_EINVAL.  A bits or a codes handle is required; an fp32 handle is
 * W2B_EINVAL.  The scan runs on the i8 matrix cores in both modes (word2bits_amd/csrc/w2b_kernels_evalbag.hip).
 *   bags: offsets is [nq + 1], non-decreasing, offsets[0] == 0, offsets[nq] == n_ids; question q is
 *     ids[offsets[q] .. offsets[q + 1]).  An id < 0 is padding and contributes nothing; an id >= w2b_eval_words(e) is
 *     W2B_EINVAL; a bag of more than W2B_EVAL_MAX_BAG ids, padding included, is W2B_EINVAL.  nq == 0 is W2B_OK.
 *   bits handle: answers are the rows with J > 0, by J descending, equal J in ascending row order; the score is
 *     (float)J / (float)size, one correctly rounded division.  A bag of m <= 7 ids with exclude_own = 1 therefore returns bit
 *     for bit what w2b_eval_combine returns for the same rows with signs all +1.
 *   codes handle: N_T = sum_a T[a]^2 (an int64), wq = (float)(1.0 / sqrt((double)N_T)) -- the double square root and the
 *     double division each correctly rounded, the result rounded to float: the expression of w(r) -- and
 *         score = ((float)J * wq) * w(c),
 *     the conversion rounded to nearest even, both multiplies rounded on their own, nothing contracted.  Answers are the rows
 *     with score > 0, by score descending, equal float scores in ascending row order: the codes key, score bits << 32 | ~row.
 *     A one-id bag [r] has N_T = N(r): with exclude_own = 1 it returns bit for bit what w2b_eval_neighbors returns for r.
 *   empty questions: a bag with no id >= 0, or with T zero in every column, has the empty list: row -1 / score 0 throughout.
 *   exclude_own: 1 = every row that stands in the bag is excluded from that question's answers, as w2b_eval_combine does;
 *     0 = nothing is excluded (document -> words, where the document's own words are wanted); anything else is W2B_EINVAL.
 *   output: 1 <= k <= W2B_EVAL_MAX_K; best / bestd are [nq][k] in the shape of w2b_eval_topk: a short list ends in row -1 /
 *     score 0, bestd may be NULL.
 * Everything is validated before anything is launched -- what does not depend on the handle (k, exclude_own, the offsets, the
 * bag lengths) first, then the handle, then the ids -- with the cause in w2b_last_error(); on error best / bestd are untouched.
 * w2b_eval_set_topk_scratch bounds the scratch of a launch (the operands, 2 * 32 * ceil(size / 32) bytes per question, plus
 * the selection slots); here a chunk is never smaller than 32 questions, and results never depend on it.
 * w2b_eval_timing_read counts these launches (operands + scan + merge), macs = 2 x questions x rows x size. */
#define W2B_EVAL_MAX_BAG 4096
int w2b_eval_bag(w2b_eval *e, int64_t n_ids, const int32_t *ids, int64_t nq, const int64_t *offsets,
                 int32_t exclude_own, int32_t k, int32_t *best, float *bestd);
/* The text form of `./nearest ... bag`: every non-empty line is one bag of 1 to W2B_EVAL_MAX_BAG words, upper-cased and looked
 * up as in w2b_eval_nearest_text; the answer has the format of w2b_eval_nearest_text.  Error lines:
 * "<head>: not in vocabulary: <WORD>\n" (the first such word) and "<head>: expected 1 to 4096 words\n".  All valid lines are
 * scored in one w2b_eval_bag batch. */
int w2b_eval_bag_text(w2b_eval *e, const char *queries, int64_t len, int32_t exclude_own, int32_t k,
                      char **out, int64_t *out_len);
/* Host twin of the bag kernels (pure C, no device): ONE bag ids[0..n) of packed[words][bitlevel * ceil(dim / 64)] scored
 * against EVERY row c, the bag's own rows included: J_out[words] = J(c), score_out[words] = the float score with the
 * semantics above for bitlevel 1 (bits) or 2 (codes); all scores are 0 when T is zero in every column.  Either output may be
 * NULL.  W2B_EINVAL as w2b_eval_bag has it: a bitlevel other than 1 or 2, n outside 0..W2B_EVAL_MAX_BAG, an id >= words,
 * dim > 58254. */
int w2b_bag_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel,
                        int64_t n, const int32_t *ids, int32_t *J_out, float *score_out);

/* ---- vector questions: the rows nearest to a float vector, on all three handle kinds --------------------------------------
 * "Which words are nearest to this vector?" -- word2vec's `distance`, gensim's similar_by_vector -- for a vector that the
 * caller computed itself: a hidden state, a projected sentence, an average with its own weights, a vector of another model of
 * the same width.  Every other question of this header is spelled in row ids; this one is `size` floats, and a packed table is
 * never expanded to answer it.
 *   input: x[q][0 .. size) is question q, in host memory.  Every value must be finite and either 0 or have 2^-60 <= |x| <=
 *     2^60; anything else is W2B_EINVAL, naming the question and the column.  The reason: within that range no product,
 *     partial sum or weight below is subnormal, and none overflows, for any `size` the handles allow (the terms x[a] * t are
 *     multiples of 2^-83 of at most 3 * 2^60, so a partial sum is 0 or between 2^-83 and 2^86; sum x^2 is 0 or between 2^-120
 *     and 2^144) -- so the result does not depend on how an instruction treats subnormals.  normalize is 0 or 1, k is in 1 ..
 *     W2B_EVAL_MAX_K, nq == 0 is W2B_OK.  Nothing is excluded from the answers: there are no "own rows".
 *   query weight: nx = sum_a (double)x[a] * (double)x[a] in column order, the products exact in double, every add rounded on
 *     its own.  normalize == 1: wx = (float)(1.0 / sqrt(nx)) -- the double square root and the double division each correctly
 *     rounded, the result rounded to float: the expression of w(r) in codes mode; normalize == 0: wx = 1.0f.  A question with
 *     nx == 0 has the empty list (row -1 / score 0 throughout), whatever normalize is.  wx is built on the host, as w2b_eval_bag
 *     builds wq.
 *   fp32 handle: vec[a] = x[a] * wx, one float32 multiply per column (exact when wx is 1), and the score of row c is the chain
 *     that w2b_eval_topk runs on that vec, in the handle's `fused` mode and w2b_eval_set_kernel variant.  So with normalize = 0
 *     and x equal to (M[b2] - M[b1]) + M[b3] computed in float32 the scores are bit for bit those of w2b_eval_topk(b1, b2, b3).
 *   bits and codes handles: S(c) in float32 is  acc = +0;  for a = 0 .. size - 1: acc = fmaf(x[a], (float)t_c[a], acc)  -- strictly
 *     sequential in a, one accumulator per (question, row); t = +-1 on a bits handle, t in {+-1, +-3} on a codes handle;
 *     (float)t is exact, so on bits rows every step is one rounded add -- and
 *         score = (S * wx) * w(c),
 *     both multiplies rounded on their own, nothing contracted.  w(c) on a codes handle is the table of codes mode; on a bits
 *     handle it is the constant (float)(1.0 / sqrt((double)size)), the same expression.  The scan runs on the f32 matrix cores,
 *     whose accumulators are exactly such chains, with the row operand decoded from the packed bits in registers
 *     (word2bits_amd/csrc/w2b_kernels_evalvec.hip).
 *   answers: the rows with score > 0, by score descending, equal float scores in ascending row order -- the codes key, score
 *     bits << 32 | ~row -- on all three handle kinds.  best / bestd are [nq][k] in the shape of w2b_eval_topk: a short list ends
 *     in row -1 / score 0, bestd may be NULL.
 * Everything is validated before anything is launched -- k, normalize and nq first (so a NULL handle with a bad k is W2B_EINVAL
 * for the k, as in w2b_eval_bag; the text form checks k and normalize before its handle too), then the handle, then the values -- with the cause in w2b_last_error(); on error best / bestd
 * are untouched.
 * w2b_eval_set_topk_scratch bounds the scratch of a launch (the uploaded vectors and their operands, about 8 * size bytes per
 * question, plus the selection slots); a chunk is never smaller than 32 questions (fp32 handle: 128, as w2b_eval_topk), and
 * results never depend on it.  w2b_eval_timing_read counts these launches (packed handles: operands + scan + merge), macs =
 * questions x rows x size. */
int w2b_eval_vectors(w2b_eval *e, int64_t nq, const float *x /* [nq][size], host */, int32_t normalize,
                     int32_t k, int32_t *best, float *bestd);
/* The text form of `./nearest ... vector`: every non-empty line is `size` numbers separated by white space, each parsed with
 * strtof in the C locale.  The head of an answer is "vector <i>", where i counts the non-empty lines from 1; the answer has the
 * format of w2b_eval_nearest_text.  Error lines: "vector <i>: expected <size> numbers\n" (another count, or a token that is
 * no number) and "vector <i>: value out of range\n" (a value that w2b_eval_vectors refuses).  All valid lines are scored in
 * one w2b_eval_vectors batch. */
int w2b_eval_vectors_text(w2b_eval *e, const char *queries, int64_t len, int32_t normalize, int32_t k,
                          char **out, int64_t *out_len);
/* Host twin of the vector kernels (pure C, explicit fmaf, no device): ONE question x[dim] scored against EVERY row c of
 * packed[words][bitlevel * ceil(dim / 64)], bitlevel 1 (the bits semantics above) or 2 (codes): S_out[words] = S(c),
 * score_out[words] = the float score; all scores are 0 when nx == 0.  Either output may be NULL.  W2B_EINVAL as
 * w2b_eval_vectors has it for the values (naming the column) and normalize, and for a bitlevel other than 1 or 2. */
int w2b_vector_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel,
                           const float *x /* [dim] */, int32_t normalize, float *S_out, float *score_out);

/* ---- 3CosMul: the multiplicative analogy rule, on both packed modes ----------------------------------------------------
 * Every other analogy answer of this header is 3CosAdd, the additive (M[b2] - M[b1]) + M[b3].  This one is 3CosMul (Levy &
 * Goldberg 2014; gensim's most_similar_cosmul): for the question (b1, b2, b3) -- "b1 is to b2 as b3 is to ?", positives b2
 * and b3, negative b1 -- every row c has three similarities u_i, float32, shifted to [0, 1], and the score
 *     score = (u2 * u3) / (u1 + eps),      eps = 1e-6f (the float 0x358637BD).
 * The multiply, the add and the division are each ONE float32 operation rounded to nearest, nothing is contracted, the
 * division is the correctly rounded one.  The additive rule lets one large term dominate; this one balances the three.
 *   bits handle: A_i(c) = size - H(b_i, c), the number of columns on which rows b_i and c agree, an exact integer;
 *     u_i = (float)A_i / (float)size, one correctly rounded division -- (1 + cos) / 2 without the detour.  Both conversions
 *     are exact for size <= 2^24; a handle with a larger size is W2B_EINVAL.  (u depends on A alone: a host-built table of
 *     size + 1 floats, as w(r) is in codes mode.)
 *   codes handle: cos_i = ((float)J(b_i,c) * w(b_i)) * w(c), the expression that w2b_eval_neighbors scores by, J and w as in
 *     codes mode; u_i = (1.0f + cos_i) * 0.5f, one add and one multiply.
 *   no subnormals: on a bits handle u is 0 or >= 2^-24; on a codes handle cos may overshoot +-1 by an ulp, so that 1 + cos is
 *     0, +-2^-24 or +-2^-23 at its smallest and u is 0 or |u| >= 2^-25.  So u2 * u3 is 0 or at least 2^-50 in magnitude, u1 +
 *     eps stays positive (at least eps - 2^-24) and at most 1 + 2^-19, and the quotient is 0 or between 2^-51 and 2^21 in
 *     magnitude: no operand and no result is subnormal, none overflows, and the result does not depend on how an instruction
 *     treats subnormals.
 *   fp32 handle: W2B_EINVAL ("not available on an fp32 handle: load the file with bits or codes"); w2b_eval_load_bits and
 *     w2b_eval_load_codes read the reference's float format and reduce it.  Handles made by *_from_trainer in bits / codes
 *     mode work like loaded ones.
 *   answers: the rows c other than b1, b2, b3 with score > 0, by score descending, equal float scores in ascending row order
 *     -- the codes key, score bits << 32 | ~row, on both handle kinds.  best / bestd are [nq][k] in the shape of
 *     w2b_eval_topk: a short list ends in row -1 / score 0, bestd may be NULL.  1 <= k <= W2B_EVAL_MAX_K; nq == 0 is W2B_OK.
 * Everything is validated before anything is launched -- k and nq first (so a NULL handle with a bad k is W2B_EINVAL for the
 * k, as in w2b_eval_bag), then the handle, then the rows: a row outside [0, words) is W2B_EINVAL, naming the question -- with
 * the cause in w2b_last_error(); on error best / bestd are untouched.
 * w2b_eval_set_topk_scratch bounds the scratch of a launch as it does for w2b_eval_topk on the same handle, and results never
 * depend on it.  w2b_eval_timing_read counts these launches, macs = 3 x questions x rows x size on both handle kinds.
 * The scans: word2bits_amd/csrc/w2b_kernels_evalcosmul.hip (bits: three popcounts per word, a float epilogue behind an exact
 * prefilter) and the COSMUL instance of the codes scan (w2b_kernels_evalcodes.hip: the same matrix-core products, another
 * epilogue). */
int w2b_eval_cosmul(w2b_eval *e, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3,
                    int32_t k, int32_t *best, float *bestd);
/* The text form of `./nearest ... bits|codes cosmul`: the format of w2b_eval_nearest_text, but every non-empty line is
 * three words A B C.  Any other count gives "<words>: expected 3 words\n"; a word that w2b_eval_lookup does not find gives
 * "<words>: not in vocabulary: <WORD>\n" (the first such word).  All valid lines are scored in one w2b_eval_cosmul batch. */
int w2b_eval_cosmul_text(w2b_eval *e, const char *queries, int64_t len, int32_t k, char **out, int64_t *out_len);
/* w2b_eval_transcript byte for byte, except that each question's answer comes from w2b_eval_cosmul with k = 1 (bits and
 * codes handles; `./compute_accuracy FILE <bitlevel> <threshold> bits|codes cosmul`). */
int w2b_eval_transcript_cosmul(w2b_eval *e, const char *questions, int64_t len, char **out, int64_t *out_len);
/* Host twin of the 3CosMul kernels (pure C, no device): ONE question (b1, b2, b3) against EVERY row c of
 * packed[words][bitlevel * ceil(dim / 64)], the question's own rows included: u_out[3][words] = u1, u2, u3 and
 * score_out[words] = the float score, with the semantics above for bitlevel 1 (bits) or 2 (codes).  Either output may be
 * NULL.  W2B_EINVAL: a bitlevel other than 1 or 2, a row outside [0, words), dim > 2^24 at bitlevel 1. */
int w2b_cosmul_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel,
                           int64_t b1, int64_t b2, int64_t b3, float *u_out /* [3][words] or NULL */,
                           float *score_out /* [words] or NULL */);

/* ---- word classes: k-means on the packed rows, word2vec's -classes output -------------------------------------------------
 * "Which words belong together?"  Every other question of this header asks which ROWS are nearest to a question; this one
 * asks the transposed question -- which of K centroids is nearest to every row -- and needs one more pass, the rows of every
 * class summed.  It is spherical k-means as word2vec's k-means block has it: a centroid is the normalised sum of its members'
 * raw vectors, a row goes to the centroid with the largest dot product.  It runs on the integer codes of a bits handle
 * (t = +-1) or a codes handle (t in {+-1, +-3}); an fp32 handle is W2B_EINVAL ("not available on an fp32 handle: load the file
 * with bits or codes").  The row's own length is a positive factor common to all classes and is left out of the comparison.
 * Everything is deterministic, bit for bit:
 *     cl[c] = init[c], or c % K when init is NULL                                          (word2vec: cl[a] = a % clcn)
 *     iters_run = 0; moved = 0; score[c] = +0 for every row
 *     while iters_run < max_iters:
 *       sums    T_k[a] = sum of t_c[a] over the rows c with cl[c] == k, exact integers;
 *               N_k = sum_a T_k[a]^2 (an int64); class k is LIVE iff N_k > 0;
 *               wq_k = (float)(1.0 / sqrt((double)N_k)) -- the expression of wq in w2b_eval_bag: (double)N_k rounded to nearest
 *               even, the double square root and the double division each correctly rounded, the result rounded to float
 *       assign  for every row c and class k:  S_k(c): acc = +0; for a = 0 .. size - 1: acc = fmaf((float)T_k[a], (float)t_c[a], acc)
 *               -- strictly sequential in a, one accumulator per (row, class): the chain of w2b_eval_vectors --
 *               d_k(c) = S_k(c) * wq_k, ONE float32 multiply, rounded on its own, nothing contracted;
 *               the LIVE classes are walked in ascending k: the first one is taken, a later one replaces it iff d_k > d_best;
 *               new[c] = that class, score[c] = its d; no live class at all: new[c] = 0, score[c] = +0
 *       moved = the number of rows with new[c] != cl[c];  cl = new;  iters_run += 1;  stop if moved == 0
 *     finally T_out, counts = the sums and the member counts of the FINAL cl (one more sums pass)
 * Stopping at moved == 0 is exact: the next iteration would reproduce the same sums and the same assignment.  A class that is
 * empty, or whose members cancel in every column, is not live and attracts no row: it stays empty.  Two deliberate departures
 * from word2vec: its `closev = -10` start would drop legitimate scores here (with integer codes |d| reaches 3 * sqrt(size)), and
 * its dead centroids are NaN by accident of 0 / 0 where this rule is spelled out.
 *   no subnormals: S is 0 or an integer-valued float with |S| >= 1, wq >= 2^-31.5, so d is 0 or at least 2^-32 in magnitude; S
 *     is never -0 because the chain starts at +0; nothing overflows.  The result does not depend on how an instruction treats
 *     subnormals.
 *   limits, all W2B_EINVAL with the cause in w2b_last_error(): 1 <= n_classes <= min(words, W2B_EVAL_MAX_CLASSES); 0 <=
 *     max_iters <= 1000; words <= 5592405 (3 * words < 2^24, so (float)T is exact); 9 * words^2 * size < 2^63 (N_k fits an
 *     int64); every init[c] in [0, n_classes) -- the error names the first offending row.
 *   validation order, as in w2b_eval_bag: what does not depend on the handle first, n_classes >= 1 and max_iters (so a NULL
 *     handle with a bad n_classes is W2B_EINVAL for the n_classes), then the handle and the limits that depend on it, then
 *     init.  On error no output is touched.
 *   outputs: cls [words]; score [words], T_out [n_classes][size], counts [n_classes], iters_run and moved (the moved count of
 *     the last iteration run, 0 when none ran) may each be NULL.
 * w2b_eval_classes keeps the class array, the sums and the centroid operands on the device for all iterations
 * (word2bits_amd/csrc/w2b_kernels_evalclasses.hip: the assign is the f32 matrix-core scan of w2b_eval_vectors with the operand
 * roles swapped, the sums a counting sort by class and an integer pooling); per iteration the host sees the moved count and
 * N_k, from which it builds wq_k as w2b_eval_bag builds wq.  Handles made by *_from_trainer in bits / codes mode work like
 * loaded ones.  w2b_eval_timing_read counts one launch per iteration run, macs = iterations run x n_classes x rows x size, and
 * the device time of both passes; w2b_eval_classes_timing splits the last call's time into the assign scans and the sums
 * passes (the one before the first iteration included). */
#define W2B_EVAL_MAX_CLASSES 16384
int w2b_eval_classes(w2b_eval *e, int32_t n_classes, int32_t max_iters, const int32_t *init /* [words] or NULL */,
                     int32_t *cls /* [words] */, float *score /* [words] or NULL */, int32_t *T_out /* [n_classes][size] or NULL */,
                     int64_t *counts /* [n_classes] or NULL */, int32_t *iters_run /* or NULL */, int64_t *moved /* or NULL */);
int w2b_eval_classes_timing(w2b_eval *e, double *assign_ms, double *sums_ms);
/* word2vec's -classes file: one line "<w2b_eval_word(row)> <class>\n" per row in row order, from w2b_eval_classes with init =
 * NULL (`./classes FILE K [iters] [threshold] bits|codes`).  *out is malloc'ed; release it with w2b_eval_free_text. */
int w2b_eval_classes_text(w2b_eval *e, int32_t n_classes, int32_t max_iters, char **out, int64_t *out_len);
/* Host twin of the class kernels (pure C, explicit fmaf, no device): the loop above on packed[words][bitlevel * ceil(dim / 64)],
 * bitlevel 1 (bits) or 2 (codes), with the same validation, outputs and NULL rules. */
int w2b_classes_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, int32_t n_classes, int32_t max_iters,
                     const int32_t *init, int32_t *cls, float *score, int32_t *T_out, int64_t *counts, int32_t *iters_run,
                     int64_t *moved);

/* ---- documents: the corpus texts nearest to a query text, by relaxed word mover's similarity ------------------------------
 * "Which of my documents is closest to this sentence?"  Every other question of this header is answered with ROWS; this one is
 * answered with DOCUMENTS of a corpus that the handle keeps.  The measure is the relaxed word mover's distance (Kusner et al.
 * 2015; gensim's wmdistance is the unrelaxed form) in its similarity form: every word of one text is matched to its best word
 * of the other, and the matches are averaged -- stronger than the cosine of two pooled means, which w2b_eval_bag and
 * w2b_embed_bag offer.  A bits or a codes handle is required; an fp32 handle is W2B_EINVAL ("not available on an fp32 handle:
 * load the file with bits or codes"), as for w2b_eval_cosmul.  Handles made by *_from_trainer in bits / codes mode work like
 * loaded ones.
 *   documents: a corpus is ids[n_ids] plus offsets[n_docs + 1], non-decreasing, offsets[0] == 0, offsets[n_docs] == n_ids, as
 *     in w2b_eval_bag; document d is ids[offsets[d] .. offsets[d + 1]).  An id < 0 is padding and contributes nothing; an id >=
 *     w2b_eval_words(e) is W2B_EINVAL; a document of more than W2B_EVAL_MAX_DOC = 1024 positions, padding included, is
 *     W2B_EINVAL; n_docs <= 0x7FFFFF00.  Queries have the same form and the same limits.  m(X) = the number of ids >= 0 in text
 *     X; a repeated id counts every time.
 *   word pairs: for rows x and c
 *       bits   I(x,c) = size - 2 * H(x,c), an exact integer in [-size, size] (bits mode above);
 *       codes  cos(x,c) = ((float)J(x,c) * w(x)) * w(c), J and w as in codes mode: exactly the expression that
 *              w2b_eval_neighbors scores by, the conversion rounded to nearest even, both multiplies rounded on their own,
 *              nothing contracted; its fixed-point image is F(x,c) = (int64) ldexp(cos(x,c), 50).
 *     A handle with size >= 2^21 is W2B_EINVAL.  Below that limit: 1024 * size < 2^31, so a sum of 1024 values I fits an int32.
 *     cos is never -0 and never NaN: w is finite and positive, (float)J is +0 exactly when J == 0 (so cos = +0) and otherwise a
 *     non-zero integer-valued float, and no product underflows: |(float)J| >= 1 and w >= 1 / sqrt(9 * size) up to an ulp, so a
 *     non-zero cos is at least about 1 / (9 * size) > 2^-25 in magnitude.  A float of that size is a multiple of 2^-48, and
 *     |cos| stays below 2 (it overshoots 1 by a few ulp at most): F is an exact integer below 2^51 in magnitude, the
 *     conversion drops nothing, and 1024 of them sum below 2^61.
 *   directed coverage of X by Y, both texts with m > 0:
 *       bits   R(X->Y) = sum over the positions x of X with id >= 0 of  max over the positions c of Y with id >= 0 of  I(x,c),
 *              an int32;
 *       codes  A(X->Y) = the same sum with F in place of I, an int64.
 *     Sums of integers and maxima of integers: the result depends neither on the order of the positions in either text nor on
 *     how a kernel splits the work, and no float is ever accumulated.  (The maximum may be taken over the floats cos and
 *     converted afterwards: the conversion is monotone and exact.)
 *   scores, float32, each conversion rounded to nearest even and ONE correctly rounded division:
 *       bits   s(X->Y) = (float)R / (float)(m(X) * size);
 *       codes  s(X->Y) = (float)A / ((float)m(X) * 0x1p50f), the divisor being exact.
 *     symmetric = 0: score(Q, D) = s(Q->D), how well every query word is matched in D -- for short queries against long
 *     documents.  symmetric = 1: score = min(s(Q->D), s(D->Q)), the similarity form of RWMD's maximum of its two lower bounds.
 *     Anything else is W2B_EINVAL.  If m(Q) == 0 or m(D) == 0 the score is +0.  No score is subnormal: a non-zero one is at
 *     least 2^-31 (bits) or 2^-60 (codes) in magnitude.
 *   two consequences: a one-id query [r] against the corpus of the one-id documents [c], c = 0 .. words - 1, returns bit for bit
 *     what w2b_eval_bag([r], exclude_own = 0) returns, rows and scores, on both handle kinds and with either `symmetric`; and
 *     permuting the positions inside any document or query changes no output bit.
 *   answers: per query the documents with score > 0, by score descending, equal float scores in ascending document index -- the
 *     codes key, score bits << 32 | ~index.  best / bestd are [nq][k] in the shape of w2b_eval_topk: a short list ends in index
 *     -1 / score 0, bestd may be NULL, 1 <= k <= W2B_EVAL_MAX_K.  Nothing is excluded: a document identical to the query is an
 *     answer.  all_scores is NULL or [nq][n_docs] and receives every score, answers or not (W2B_EINVAL when nq * n_docs > 2^28).
 * Everything is validated before anything is launched -- what does not depend on the handle first (k, symmetric, nq, the
 * offsets, the lengths; so a NULL handle with a bad k is W2B_EINVAL for the k, as in w2b_eval_bag), then the handle (its kind,
 * its size, a corpus being set: a query call without one is W2B_EINVAL), then the ids -- with the cause in w2b_last_error(); on
 * error no output is touched.  nq == 0 is W2B_OK as soon as the checks that need no handle have passed: nothing is asked, so
 * neither the handle nor a corpus is needed.
 * How it runs (word2bits_amd/csrc/w2b_kernels_evaldocs.hip): a vocabulary row occurs in a corpus many times, so per chunk of
 * queries a pair table Tab[c][x] = I or cos of every vocabulary row c against every query position x is built first (each
 * query's columns padded to a whole 64-byte line), with the largest value of each row over a query's own columns beside it;
 * then the corpus ids are streamed once per query of the chunk: Q->D is a per-lane running maximum over the slices Tab[id][the query's columns],
 * D->Q a gather of the row maxima.  w2b_eval_set_topk_scratch bounds the scratch of a chunk of queries; a chunk is never
 * smaller than one query, whose own need is 4 * words * (its ids >= 0 rounded up to 16, plus 1) bytes of table, 8 * k *
 * (ceil(n_docs / 1024) + 1) bytes of selection slots and, with all_scores, 4 * n_docs bytes; results never depend on the
 * bound.  w2b_eval_timing_read counts these launches (one per chunk: table + walk + merge), macs = (query positions x document
 * positions, padding included, summed over all pairs) x size; w2b_eval_docs_timing splits the last call's device time into the
 * table phase and the walk phase (walk + merge). */
#define W2B_EVAL_MAX_DOC 1024
/* copies the corpus to the device and keeps it on the handle; replaces an earlier one; n_docs == 0 drops it.  On error the
 * earlier corpus stays. */
int w2b_eval_docs_set(w2b_eval *e, int64_t n_ids, const int32_t *ids, int64_t n_docs, const int64_t *offsets);
/* The corpus from text: one document per LINE of text[0..len) (every line counts, empty ones too: index = line number - 1),
 * split on white space and upper-cased as w2b_eval_nearest_text does; words that w2b_eval_lookup does not find are dropped
 * and counted in *dropped; a line with more than 1024 known words is W2B_EINVAL naming the line, and the earlier corpus stays.
 * n_docs and dropped may be NULL. */
int w2b_eval_docs_set_text(w2b_eval *e, const char *text, int64_t len, int64_t *n_docs, int64_t *dropped);
int64_t w2b_eval_docs_count(const w2b_eval *e);
int w2b_eval_docs(w2b_eval *e, int64_t n_qids, const int32_t *qids, int64_t nq, const int64_t *qoffsets,
                  int32_t symmetric, int32_t k, int32_t *best, float *bestd, float *all_scores /* [nq][n_docs] or NULL */);
/* The text form of `./nearest ... bits|codes docs CORPUS.txt`: every non-empty line is one query text, upper-cased and looked
 * up as in w2b_eval_nearest_text, unknown words dropped.  The head of an answer is the line's words joined by one space,
 * "<WORDS>:\n", followed by one line "<rank>\t<line number of the document, from 1>\t<score %.6f>\n" per answer.  Error lines:
 * "<head>: no word in vocabulary\n" and "<head>: expected at most 1024 words\n".  All valid lines are scored in one
 * w2b_eval_docs batch. */
int w2b_eval_docs_text(w2b_eval *e, const char *queries, int64_t len, int32_t symmetric, int32_t k,
                       char **out, int64_t *out_len);
int w2b_eval_docs_timing(w2b_eval *e, double *table_ms, double *walk_ms);
/* Host twin of the document kernels (pure C, no device): ONE query qids[0..n_q) against every document, every word pair
 * computed directly from packed[words][bitlevel * ceil(dim / 64)] (no table), bitlevel 1 (bits) or 2 (codes): dir_out[2][n_docs]
 * = R or A of Q->D, then of D->Q, as int64 (0 where either text has m == 0), score_out[n_docs] = the float score.  Either
 * output may be NULL.  W2B_EINVAL as w2b_eval_docs_set and w2b_eval_docs have it, and for a bitlevel other than 1 or 2. */
int w2b_docs_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel,
                         int64_t n_ids, const int32_t *ids, int64_t n_docs, const int64_t *offsets,
                         int64_t n_q, const int32_t *qids, int32_t symmetric,
                         int64_t *dir_out, float *score_out);

/* ---- pair similarity: the cosine of two words or two bags, and its rank correlation with human scores --------------------
 * "How similar are these two words, these two sentences?" -- the second intrinsic evaluation beside the analogies: a list of
 * human-rated pairs (WordSim-353, SimLex, MEN, Rare Words; STS for sentences) is scored and the correlation between the model's
 * cosines and the human scores is reported (gensim's evaluate_word_pairs; for bags n_similarity, the cosine of the two pooled
 * vectors).  Every other question of this header is "one question against all rows, top-k"; this one scores GIVEN pairs.  A bits
 * or a codes handle is required; an fp32 handle is W2B_EINVAL ("not available on an fp32 handle: load the file with bits or
 * codes"), as for w2b_eval_cosmul.  A handle with size > 2^24 is W2B_EINVAL.  Handles made by *_from_trainer in bits / codes mode
 * work like loaded ones.
 *   pairs: one ids[n_ids] array and offsets[2 * np + 1], non-decreasing, offsets[0] == 0, offsets[2 * np] == n_ids: bag 2 p is
 *     side A of pair p, bag 2 p + 1 side B.  An id < 0 is padding and contributes nothing; an id >= w2b_eval_words(e) is
 *     W2B_EINVAL, naming the pair; a bag of more than W2B_EVAL_MAX_BAG ids, padding included, is W2B_EINVAL.  np == 0 is W2B_OK.
 *   integers, exact: per side T[a] = sum over the bag's ids r >= 0 of t_r[a], t = +-1 on a bits handle, t in {+-1, +-3} on a codes
 *     handle -- the pooling of w2b_eval_bag: the same row twice adds twice, |T[a]| <= 3 * 4096 -- and over the `size` columns
 *         J = sum_a T_A[a] * T_B[a],     N_A = sum_a T_A[a]^2,     N_B = sum_a T_B[a]^2,
 *     each an int64 below 12288^2 * 2^24 < 2^53: exact as integers and as doubles.  Integer adds commute, so no split of the work
 *     changes them.  parts (or NULL) receives [np][3] = J, N_A, N_B.
 *   score: built on the host from the three integers the device returns, as w2b_eval_bag builds wq:
 *         score = (float)((double)J / sqrt((double)N_A * (double)N_B)),
 *     the double multiply, the square root and the division each correctly rounded, the result rounded to float.  A pair with
 *     N_A == 0 or N_B == 0 is EMPTY -- a bag with no id >= 0, or one whose T is zero in every column -- and scores +0.  Two
 *     consequences: identical bags score exactly 1.0f (sqrt(fl(N * N)) == N), and on a bits handle a pair of one-word bags [r],
 *     [c] has N_A = N_B = size and scores bit for bit the (float)J / (float)size that w2b_eval_neighbors and w2b_eval_bag give
 *     row c for the question r (J and size are exact in float32, and a double quotient rounded to float is the correctly rounded
 *     float quotient).
 * Everything is validated before anything is launched -- what does not depend on the handle first (the arguments, the offsets,
 * the bag lengths), then the handle, then the ids, as in w2b_eval_bag -- with the cause in w2b_last_error(); on error score and
 * parts are untouched.
 * How it runs (word2bits_amd/csrc/w2b_kernels_evalpairs.hip): lane = column, an id is wave-uniform, so a packed word is one
 * broadcast load; one wavefront per pair, a workgroup per pair of more than 256 ids, one lane per one-word pair (popcounts on
 * whole words).  Large calls run in chunks of whole pairs: w2b_eval_set_topk_scratch bounds the device staging of a launch
 * (the ids, 4 bytes each, and 36 bytes per pair: two bounds, a path entry and the 24 bytes of parts); a chunk is never smaller
 * than 64 pairs, however large they are; results never depend on the chunking.  w2b_eval_timing_read counts these launches (one
 * per chunk), macs = n_ids x size, the pooling adds. */
int w2b_eval_pairs(w2b_eval *e, int64_t n_ids, const int32_t *ids, int64_t np, const int64_t *offsets /* [2 * np + 1] */,
                   float *score /* [np] */, int64_t *parts /* [np][3] = J, N_A, N_B, or NULL */);
/* The text form of ./similarity: a list of rated pairs in, their scores and the two correlations out.  Lines are numbered from 1.
 * A line that is empty (or white space only; a '\r' before the '\n' is dropped) or starts with '#' is no pair.  Every other line
 * is one pair of exactly three fields A, B, gold: if the line contains a tab the fields are its tab-separated parts, each
 * stripped of the blanks around it; otherwise they are its runs of non-blank characters.  A and B are 1 to W2B_EVAL_MAX_BAG words
 * separated by blanks, upper-cased and looked up as w2b_eval_bag_text does; gold is parsed with strtod in the C locale, must be
 * consumed completely and be finite.  Anything else makes the line MALFORMED.  A word that w2b_eval_lookup does not find is
 * dropped from its bag and counted.  All well-formed lines go through one w2b_eval_pairs batch; a pair that comes back EMPTY
 * (above: for example every word of a side unknown) is SKIPPED, the others are SCORED.
 * With details != 0 one line per pair line, in input order:
 *     "<score %.6f>\t<gold as written>\t<A as written>\t<B as written>\n"    or
 *     "skipped\t<gold>\t<A>\t<B>\n"                                          or     "malformed line <n>\n"
 * then always
 *     "pairs: <scored> scored, <skipped> skipped, <malformed> malformed\n"
 *     "words: <looked up> looked up, <oov> not in vocabulary\n"      (every word of a well-formed line is looked up)
 *     "pearson: <%.6f or nan>\n"  "spearman: <%.6f or nan>\n"        (w2b_rank_correlation of gold and (double)score over the
 *                                                                      scored pairs in input order)
 * *out is malloc'ed; release it with w2b_eval_free_text. */
int w2b_eval_pairs_text(w2b_eval *e, const char *pairs, int64_t len, int32_t details, char **out, int64_t *out_len);
/* Host twin of the pair kernels (pure C, no device): the pairs above on packed[words][bitlevel * ceil(dim / 64)], bitlevel 1 (bits)
 * or 2 (codes), T from the unpacked rows.  score and parts may each be NULL.  W2B_EINVAL as w2b_eval_pairs has it for the
 * arguments, the offsets, the bag lengths and the ids, and for a bitlevel other than 1 or 2 and dim > 2^24; on error nothing is
 * written. */
int w2b_pairs_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, int64_t n_ids, const int32_t *ids,
                   int64_t np, const int64_t *offsets, float *score, int64_t *parts);
/* Pearson's r and Spearman's rho of x[n], y[n], in double on the host (no device):
 *     r = sum (x - mx)(y - my) / sqrt(sum (x - mx)^2 * sum (y - my)^2),   mx, my the means;
 *     rho = the same r on the 1-based ranks, equal values sharing the mean of their ranks (scipy's spearmanr).
 * A value is NaN with n < 2, with a zero variance, or when an input is NaN.  Either output may be NULL.  W2B_EINVAL: n < 0, a
 * NULL input with n > 0. */
int w2b_rank_correlation(int64_t n, const double *x, const double *y, double *pearson, double *spearman);

/* ---- rank of a given row: its place in the complete answer list, on both packed modes --------------------------------------
 * Every list question above returns at most W2B_EVAL_MAX_K rows.  This one asks where ONE given row stands, however far down:
 * the position that mean reciprocal rank, hits@k, gensim's rank(w1, w2) and closer_than(w1, w2) (= rank - 1 rows) and a
 * retrieval evaluation with one known correct row are made of.  It matters most on 1-bit models, whose integer scores tie in
 * large blocks with the lowest row first: top-1 alone cannot tell "the answer was second" from "the answer was nowhere".
 * bits and codes handles only, the additive rule (3CosAdd) only.
 *
 * For the question (b1, b2, b3) and the target row g, the COMPLETE LIST is what w2b_eval_topk would return if k were
 * unbounded: the rows c other than b1, b2, b3 with score > 0 (bits: I(c) > 0), by score descending, equal scores in ascending
 * row order.  The scores are those of the handle's mode: on a bits handle the exact integer I, on a codes handle the float32
 * sequence ((p2 - p1) + p3) * w(c) of the codes section, bit for bit.
 *     rank[q]   the 1-based place of g in that list, 0 when g is not in it (g is one of b1, b2, b3, or its score is not > 0).
 *               For a ranked g:  rank = 1 + #{c not in {b1, b2, b3, g} : s(c) > s(g) or (s(c) == s(g) and c < g)}
 *               (a row that beats a ranked g has a positive score automatically).
 *     tied[q]   the number of OTHER rows of the list with exactly the target's score (equal I; equal float); 0 when rank is 0.
 *               With it a caller turns the lowest-row convention into a mean rank over ties.  May be NULL.
 *     score[q]  the score w2b_eval_topk reports for g: (float)I / (float)size on bits, the float on codes; 0 when rank is 0.
 *               May be NULL.
 * Three consequences:
 *   - for k <= 64, 1 <= rank <= k exactly when w2b_eval_topk has g at best[q][rank - 1] with bestd == score bit for bit, and
 *     rank == 0 or rank > k exactly when g is not in that list;
 *   - one question asked with every row of the table as target gives each of 1..m exactly once, m the length of the complete
 *     list, and 0 for the rest;
 *   - inside a block of identical rows the ranks are consecutive in row order (the question's own rows left out of the run).
 *
 * Validation, in this order (as w2b_eval_cosmul): what needs no handle first -- nq < 0, or a NULL rank or input pointer with
 * nq > 0, is W2B_EINVAL even with a NULL handle; nq == 0 is W2B_OK; then the handle (an fp32 handle is W2B_EINVAL "not
 * available on an fp32 handle: load the file with bits or codes"); then the rows (a b1, b2, b3 or target outside [0, words) is
 * W2B_EINVAL naming the question).  On any error no output is touched.  Handles made by *_from_trainer work like loaded ones.
 *
 * Scratch and timing: w2b_eval_set_topk_scratch bounds one launch (the questions' planes or operands plus 8 bytes of counters
 * per question; a chunk is never smaller than 128 questions, and results never depend on the bound).  w2b_eval_timing_read
 * counts one launch per chunk (target score and scan); macs is questions x rows x size on bits and three times that on codes.
 *
 * The kernels count, they do not select: word2bits_amd/csrc/w2b_kernels_evalbits.hip (k_bits_rank) and the RANK epilogue of
 * k_codes_scan in w2b_kernels_evalcodes.hip; DESIGN.md 3.4d. */
int w2b_eval_rank(w2b_eval *e, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3,
                  const int32_t *target, int32_t *rank, int32_t *tied /* or NULL */, float *score /* or NULL */);
/* = w2b_eval_rank(rows, rows, rows, target): the place of target among the neighbours of rows[q] (gensim's rank) */
int w2b_eval_neighbor_rank(w2b_eval *e, int64_t nq, const int32_t *rows, const int32_t *target, int32_t *rank, int32_t *tied,
                           float *score);
/* Host twin (pure C, no device) for one question on packed[words][bitlevel * ceil(dim / 64)], bitlevel 1 (bits) or 2 (codes),
 * built on w2b_bits_scores_host / w2b_codes_scores_host.  tied and score may be NULL.  W2B_EINVAL for a bitlevel other than 1
 * or 2 and for a row outside [0, words); on error nothing is written. */
int w2b_rank_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, int64_t b1, int64_t b2, int64_t b3,
                  int64_t target, int32_t *rank, int32_t *tied, float *score);
/* The text form of `./nearest FILE k [bitlevel] [threshold] bits|codes rank`.  Every non-empty line is two words "A G" (the
 * place of G among the neighbours of A) or four words "A B C G" (the place of G as the answer to A : B = C : ?); words are
 * upper-cased and looked up as in w2b_eval_nearest_text.  The answer line is
 * "<WORDS joined by one space>:\t<rank>\t<tied>\t<score %.6f>\n", with rank 0 "<WORDS>: no rank\n"; error lines are
 * "<WORDS>: expected 2 or 4 words\n" and "<WORDS>: not in vocabulary: <WORD>\n" (the first such word).  All valid lines go
 * through one w2b_eval_rank batch. */
int w2b_eval_rank_text(w2b_eval *e, const char *queries, int64_t len, char **out, int64_t *out_len);
/* `./compute_accuracy FILE <bitlevel> <threshold> bits|codes rank`: the bytes of w2b_eval_transcript (its lines come from
 * the w2b_eval_top1 path as before, with the reference's comparison of words), and after every "Total accuracy: ..." line
 *   "RANKS section: MRR <m>   hits@1 <d>   hits@5 <d>   hits@10 <d>   unranked <d>   (<d> questions)\n"
 *   "RANKS total: MRR <m>   Semantic MRR <m>   Syntactic MRR <m>\n"
 * The target of a question is w2b_eval_lookup(its fourth word); hits@n counts the questions with 1 <= rank <= n, unranked
 * those with rank 0.  <m> is the sum in stream order, in double, of 1.0 / rank (rank 0 adds 0.0) divided by the double count
 * of answered questions of that scope, printed %.4f; a scope without a question prints the three letters nan.  Removing the
 * lines that begin with RANKS leaves w2b_eval_transcript's bytes; with a vocabulary of distinct words hits@1 equals the count
 * of the ACCURACY TOP1 line. */
int w2b_eval_transcript_rank(w2b_eval *e, const char *questions, int64_t len, char **out, int64_t *out_len);

#ifdef __cplusplus
}
#endif
#endif
