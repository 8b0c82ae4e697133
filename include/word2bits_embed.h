/*
 * word2bits_embed.h -- C ABI of the packed embedding layer: row lookup and bag pooling on the MI355X, straight from the
 * bit-packed table of a 1-bit or 2-bit model (the .w2bp layout of include/word2bits_corpus.h), and the output projection
 * (logits) of a batch of float vectors against the same packed rows, with its back-projection (the gradient with respect
 * to those vectors; the expected embedding under a distribution over rows), and the softmax cross-entropy of that projection
 * with its gradient, computed without the logits ever being stored, and the k largest logits per vector with their
 * positions, selected without the logits ever being stored either.
 *
 * The consumer of a packed model that is not the evaluator: a downstream model asks for the rows of a batch of token ids,
 * or for their sum / mean per sentence ("bag").  The rows stay packed on the device, [rows][w2b_packed_words_per_row(dim,
 * bitlevel)] 64-bit words, 1/32 (1/16) of the float table; no float table is ever built, on either side.  The kernels are in
 * word2bits_amd/csrc/w2b_kernels_embed.hip, w2b_kernels_embedproj.hip, w2b_kernels_embedback.hip, w2b_kernels_embedxent.hip and
 * w2b_kernels_embedtopk.hip, the host side in
 * w2b_embed.cpp (the handle, staging and launches), w2b_embed_shared.h (what is refused) and w2b_embed_twins.cpp (the *_host twins).
 *
 * No CPU fallback: W2B_ENOGPU when no device is visible (the *_host functions below are the tests' twins of the kernels,
 * as w2b_bits_scores_host is for the bits kernels).  Error codes and w2b_last_error() are those of word2bits_hip.h.
 *
 * ---- semantics -----------------------------------------------------------------------------------------------------
 * Table.  `packed` is [rows][w2b_packed_words_per_row(dim, bitlevel)]: per 64 columns one word of SIGN bits (set =
 *   negative) and, at bitlevel 2, one word of MAGNITUDE bits (set = 0.75, clear = 0.25).  bitlevel is 1 or 2, anything
 *   else is W2B_EUNSUPPORTED.  1 <= rows <= 0x7FFFFF00, 1 <= dim <= 2^24, else W2B_EINVAL.
 * Lookup.  out[i][0 .. dim) is row ids[i] exactly as w2b_unpack_quantized delivers it: the float32 patterns +-0x3EAAAAAB
 *   (1/3) at bitlevel 1 and +-0.25, +-0.75 at bitlevel 2.  An id < 0 is padding: its output row is +0.0 throughout.
 *   The kernel assembles every value from the bits with integer operations -- there is no float arithmetic on this path,
 *   so the patterns are exact by construction.  Output rows are dense, [n][dim], without padding.
 * Bag.  offsets is [n_bags + 1], non-decreasing, offsets[0] == 0, offsets[n_bags] == n_ids; bag b is
 *   ids[offsets[b] .. offsets[b + 1]).  Per column a, the integer T[a] = sum of t_r[a] over the bag's ids r >= 0, where
 *   t = +-1 at bitlevel 1 and t in {+-1, +-3} at bitlevel 2 (the codes of word2bits_eval.h: value = t / 4).  Padding ids
 *   contribute nothing.  Then, in float32, every operation rounded to nearest on its own:
 *       sum  = (float)T[a] * q       q = 0x3EAAAAAB at bitlevel 1, 0.25f at bitlevel 2: ONE multiply, rounded once
 *       mean = sum / (float)m        m = the number of ids >= 0 in the bag: ONE correctly rounded division
 *   A bag with m == 0 is +0.0.  A bag longer than W2B_EMBED_MAX_BAG ids is W2B_EINVAL: with at most 2^22 ids,
 *   |T| <= 3 * 2^22 < 2^24, so the conversion (float)T is exact, and so is (float)m.  Integer adds commute: the result
 *   does not depend on how the kernels split a bag.
 * Output dtypes.  W2B_EMBED_BF16 and W2B_EMBED_F16 are the float32 result above rounded to nearest even (16-bit
 *   patterns).  .25 and .75 are exact in both; 1/3 becomes 0x3EAB in bf16 and 0x3555 in f16.
 * Weighted bag (w2b_embed_bag_weighted*; torch's per_sample_weights).  Table, ids, offsets, padding, W2B_EMBED_MAX_BAG,
 *   dtypes and modes as for the bag; in addition weights is float32 [n_ids], one per id POSITION.  The weight of a
 *   padding id is ignored and may hold anything.  The weight of an id >= 0 must be finite and either 0 or
 *   2^-60 <= |w| <= 2^60, else W2B_EINVAL: within that range every term and every partial sum is 0 or between 2^-83
 *   and 2^84 (as for the queries of w2b_eval_vectors), nothing is subnormal and nothing overflows, so the result does
 *   not depend on how an instruction treats subnormals.
 *   A float sum depends on its order, so the order is part of the contract.  Per bag and per column a, with t_r[a] the
 *   integer code above ((float)t is exact): the bag's positions, padding included, are cut into SEGMENTS of
 *   W2B_EMBED_WSEG consecutive positions counted from the bag's start.
 *       segment s:  P_s = +0;  for the positions i of s in order with ids[i] >= 0:  P_s = fmaf(w_i, (float)t_ids[i][a], P_s)
 *                   one fused multiply-add per id, strictly sequential, one accumulator per (bag, column)
 *       bag:        S = +0;  for s in order:  S = S + P_s          each ONE float32 add, rounded on its own
 *       sum  = S * q                                               ONE multiply, q as above
 *       mean = sum / (float)m                                      ONE correctly rounded division; m = the number of
 *                                                                  ids >= 0, as in the unweighted mean -- NOT the sum
 *                                                                  of the weights; m == 0 gives +0.0
 *   A bag of at most W2B_EMBED_WSEG positions is therefore one chain.  BF16 / F16 are that float32 result rounded to
 *   nearest even.  The segment rule is what lets a long bag be spread over the device without float atomics and still
 *   have ONE defined result: whichever path pools a bag (its own workgroup, its segments on many workgroups, or one
 *   workgroup walking all its segments when the list of long bags is full), the result is the one above, bit for bit.
 *   Two consequences: with every weight 1.0f all partial sums are integers below 2^24, so sum / mean equal
 *   w2b_embed_bag bit for bit; scaling every weight by 2^s (staying in range) scales sum and mean exactly.
 * Projection (w2b_embed_project*; the tied output layer, sampled-softmax scoring, re-ranking of a candidate list): the
 *   other direction through the same table, logits[i][j] = x[i] . E[cand[j]].  Table, bitlevel, t_r[a] and q as for the bag.
 *   Input: x is float32 [n][dim].  In the host form every value must be finite and either 0 or 2^-60 <= |x| <= 2^60, else
 *   W2B_EINVAL naming the vector and the column: the rule of w2b_eval_vectors, for the same reason (every term and every
 *   partial sum is then 0 or between 2^-83 and 2^86, nothing is subnormal and nothing overflows).
 *   Candidates: cand is int32 [m], or NULL, which means every row in row order; m must then be rows.  A candidate id < 0
 *   is padding: its output column is +0.0 throughout.  The same row may stand several times.  In the host form an id >=
 *   rows is W2B_EINVAL.
 *   Result, float32, for vector i and candidate j with row r = cand[j]:
 *       S = +0;  for a = 0 .. dim - 1:  S = fmaf(x[i][a], (float)t_r[a], S)
 *                   one fused multiply-add per column, strictly sequential in a, one accumulator per (vector, candidate):
 *                   the chain of w2b_eval_vectors
 *       out[i][j] = S * q                                          ONE float32 multiply, rounded on its own
 *   Output: dense [n][m] without padding; BF16 / F16 are that float32 result rounded to nearest even.
 *   Three consequences: with x = the unit vector of column a, out[.][j] is the value lookup(cand[j])[a] bit for bit (1 * q
 *   and 3 * 0.25 are exact); S equals the S_out of w2b_vector_scores_host for the same row and vector bit for bit; scaling
 *   every x by 2^s (staying in range) scales every output exactly.
 * Back-projection (w2b_embed_backproject*; the gradient of the projection with respect to x, and the expected embedding
 *   p @ E under a distribution over rows or candidates): dx[i][a] = sum over j of g[i][j] * E[cand[j]][a].  Table, bitlevel,
 *   t_r[a], q and the candidate rules are those of the projection: cand is int32 [m], or NULL, which means every row in row
 *   order, and m must then be rows; an id < 0 is padding; the same row may stand several times; in the host form an id >=
 *   rows is W2B_EINVAL.  Input: g is float32 [n][m].  Output: dx is float32 [n][dim], dense; there is no 16-bit output (x is
 *   float32, so its gradient is too).
 *   The order is part of the contract, and it is the weighted bag's: per vector i and column a the candidate positions
 *   0 .. m - 1, padding included, are cut into segments of W2B_EMBED_WSEG consecutive positions counted from position 0.
 *   With r = cand[j]:
 *       segment s:  P_s = +0;  for the positions j of s in order with cand[j] >= 0:  P_s = fmaf(g[i][j], (float)t_r[a], P_s)
 *       bag:        S = +0;  for s in order:  S = S + P_s          each ONE float32 add, rounded on its own
 *       dx[i][a] = S * q                                           ONE float32 multiply
 *   g at a padding position is ignored and may hold anything, NaN included.  In the device form the same holds for a
 *   candidate >= rows: it contributes nothing and is counted once in w2b_embed_bad_ids.  In the host form a g on a
 *   candidate >= 0 must be finite and either 0 or 2^-60 <= |g| <= 2^60, else W2B_EINVAL naming the vector and the candidate
 *   position; the device form does not look at the values: what a NaN or a value out of range produces is what the chain
 *   produces on the device, as for x in the projection.  m == 0 gives +0.0 rows.
 *   Four consequences: (a) for m <= W2B_EMBED_MAX_BAG, dx[i] equals w2b_embed_bag_weighted with ids = cand (or 0 .. rows - 1),
 *   weights = g[i], one bag per vector, mode sum, bit for bit; (b) with g[i] the unit vector of position j, dx[i] is
 *   lookup(cand[j]) bit for bit; (c) scaling every g by 2^s (staying in range) scales dx exactly; (d) it is the adjoint of
 *   the projection: at bitlevel 2, where q is exact, and with small integers, so that every sum is exact,
 *   sum_ij g[i][j] * project(x)[i][j] == sum_ia x[i][a] * dx[i][a] holds exactly.
 * Cross-entropy (w2b_embed_xent*; softmax cross-entropy of the tied output layer, and its gradient with respect to x, without
 *   an [n][m] array of logits, probabilities or gradients on the device).  Table, bitlevel, t_r[a], q, x, cand, padding
 *   (id < 0) and the all-rows form (cand == NULL, m == rows) are those of the projection.  In addition target is int32 [n]:
 *   target[i] is a candidate POSITION in [0, m) -- in the all-rows form that is the row --, and target[i] < 0 means that
 *   vector i is ignored (torch's ignore_index).  With l[i][j] = the projection's float32 result for vector i and position j
 *   (the chain, then * q), and LIVE = a position whose candidate is not padding:
 *   1. expneg(r), for float32 r <= 0, is a defined sequence of individually rounded float32 operations, written once in
 *      w2b_embed_shared.h (the host twin and the kernels compile the same text):
 *          r < -64, or not r >= -64:   +0.0 exactly
 *          otherwise   k = rintf(r * LOG2E)                     one multiply, one round to nearest even
 *                      f = fmaf(k, -LN2_HI, r);  f = fmaf(k, -LN2_LO, f)
 *                      p = Horner in f, explicit fmaf, degree 7, coefficients 1/i! rounded to float32 (hex patterns there)
 *                      result = p * 2^k                         2^k built from integer bits; the multiply is exact
 *      Every non-zero result is a normal number >= 2^-93, so nothing depends on how an instruction treats subnormals;
 *      expneg(0) == 1.0f exactly; no result exceeds 1.  Within 1 ulp of exp(r) (0.881 ulp measured on a dense sample).
 *   2. Segment statistics.  The positions 0 .. m - 1, padding included, are cut into segments of W2B_EMBED_XSEG = 256
 *      consecutive positions counted from 0: the candidates ONE workgroup of the projection kernel holds in its accumulators
 *      (four wavefronts x two interleaved 32-candidate tiles), so a segment is reduced where its logits already are.  A
 *      contract constant like W2B_EMBED_WSEG.  Per vector and segment s:
 *          M_s = the maximum of l over the segment's live positions                       exact, independent of order
 *          U_s = the sum over the segment's live positions of (uint64) rint(expneg(l - M_s) * 2^32)
 *                the subtraction ONE float32 operation, the scaling exact, the rounding to nearest even: each term an
 *                integer in [0, 2^32].  Integer adds commute: as in the unweighted bag, the result does not depend on how
 *                lanes, wavefronts or workgroups split a segment.
 *      A segment without a live position does not take part.
 *   3. Per vector.  mx = the maximum of M_s, exact.  se: start at +0, then for s in order
 *          se = fmaf((float)U_s * 2^-32, expneg(M_s - mx), se)
 *      one u64 -> f32 conversion (round to nearest even), one exact scaling, one fused multiply-add per segment, strictly
 *      sequential.  tl = l[i][target[i]].  If no position is live: mx = se = +0.0.  For an ignored vector tl = +0.0; mx and se
 *      are still as above.
 *   4. The loss is (mx - tl) + log(se).  The logarithm is the one step outside the bit-for-bit contract: the C ABI returns
 *      mx, se and tl; the numpy front computes the loss in float64, the torch front in float32 with torch.log.  The loss of
 *      an ignored vector is 0.
 *   5. Gradient.  For a live position g[i][j] = expneg(l - mx) / se: one subtraction, one correctly rounded division; at
 *      j == target[i] one more float32 subtraction, - 1.0f.  g is +0.0 throughout for an ignored vector.  dx[i] is THE
 *      BACK-PROJECTION of g[i] through the same candidates under its existing contract, bit for bit: the W2B_EMBED_WSEG
 *      segments, one fmaf per position, then * q.  Padding positions are ignored, as there.  What does not carry over is the
 *      back-projection's value rule: g is computed, not supplied, and may lie below 2^-60 (never below 2^-93 / 2^31: it is
 *      normal).  A partial sum P_s could only become subnormal through the cancellation of terms below 2^-103, which needs
 *      se > 2^10 times the largest of them; in that corner the result is what the chain produces on the device.
 *   Consequences: (a) mx, tl and every l equal w2b_embed_project_host bit for bit; (b) dx equals
 *   w2b_embed_backproject_host applied to the g of step 5, bit for bit, wherever that function admits the g; (c) permuting
 *   the candidates WITHIN a segment changes neither mx, nor se, nor any U_s; (d) adding a padding-only segment changes
 *   nothing; (e) with m == 1 and target 0: mx == tl, se == 1.0f, dx == +0.0.
 *   Host form: a target >= m, or one that points at a padding position, is W2B_EINVAL naming the vector.  Device form: such
 *   a target, or one on a refused candidate, makes the vector ignored and is counted once in w2b_embed_bad_ids; a candidate
 *   >= rows is dead, as padding is, and is counted once; the values of x are not checked.
 * Top-k (w2b_embed_topk*; greedy and beam decoding, top-k sampling, re-ranking: per vector the k largest logits of the
 *   projection and the candidate positions they stand at, without an [n][m] array on the device).  Table, bitlevel, t_r[a], q,
 *   x, cand, padding (id < 0) and the all-rows form (cand == NULL, m == rows) are those of the projection.
 *   Logit.  l[i][j] is the projection's float32 result (the fmaf chain in column order, then * q), bit for bit.
 *   Live positions.  Only a LIVE position is an answer: one whose candidate is a row of the table.  A padding position never
 *   is.  In the device form a candidate >= rows is never an answer either and is counted once in w2b_embed_bad_ids (in the
 *   projection such a column is +0.0; here it does not exist).
 *   Order.  Logit descending; equal logits in ascending candidate position (the evaluator's tie rule; torch.topk promises
 *   none).  Precisely, the order of the 64-bit key  map(bits of l) << 32 | ~position,  where map is the order-preserving
 *   integer map of float32 bits: all bits of a negative pattern flipped, the sign bit of a non-negative one set.  Negative
 *   logits -- the common case here, unlike in the evaluator, whose keys assume a score > 0 -- therefore rank correctly.  A live
 *   logit cannot be -0.0: the chain starts at +0 and rounds to nearest, so a sum is -0 only if every term is, and the first
 *   step, fmaf(x, t, +0), never gives -0; nor does the product with q > 0 change a sign.  In the device form, where x is not
 *   checked, a NaN stands where that map puts its bits (above +inf with the sign bit clear, below -inf with it set).
 *   Output.  vals[i][0 .. k) float32 and pos[i][0 .. k), best first; pos is a candidate POSITION in [0, m) -- in the all-rows
 *   form that is the row.  With fewer than k live positions the list ends in pos = -1, val = -inf (0xFF800000).
 *   1 <= k <= W2B_EMBED_MAX_K, else W2B_EINVAL.
 *   Consequences: (a) vals, pos equal the first k entries of a stable descending sort of w2b_embed_project_host's row i
 *   restricted to the live positions, the values bit for bit; (b) k = 1 gives vals == mx of w2b_embed_xent for the same
 *   operands (when a position is live); (c) the same row standing at several positions appears once per position, lowest
 *   position first; (d) scaling x by 2^s, s >= 0 (staying in range), scales vals exactly and leaves pos unchanged; (e) the
 *   result does not depend on how the call is cut into ranges of vectors, on how many vectors a launch takes, or on the
 *   order in which workgroups run.
 *
 * ---- out of scope --------------------------------------------------------------------------------------------------
 * Gradients or training through the lookup (the table is read-only); gradients with respect to the table through the
 * projection or the cross-entropy, and second derivatives (the back-projection and the cross-entropy's gradient are
 * once-differentiable: they are not themselves recorded); class weights, label smoothing and 16-bit outputs of the
 * cross-entropy; fusing the back-projection's contraction into the gradient kernel (the next step); bitlevels
 * other than 1 and 2; gradients through the selection, top-p sampling, per-vector candidate lists and 16-bit outputs of the
 * top-k selection; a handle built from a live trainer (w2b_export_packed + w2b_embed_create does it in two calls);
 * float input files.
 */
#ifndef WORD2BITS_EMBED_H
#define WORD2BITS_EMBED_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct w2b_embed w2b_embed;
#define W2B_EMBED_F32 0
#define W2B_EMBED_BF16 1
#define W2B_EMBED_F16 2
#define W2B_EMBED_SUM 0
#define W2B_EMBED_MEAN 1
#define W2B_EMBED_MAX_BAG (1 << 22)
#define W2B_EMBED_WSEG 1024
#define W2B_EMBED_XSEG 256
#define W2B_EMBED_MAX_K 64

/* A bit-packed .w2bp, read without expanding it; `threshold` caps the rows as in w2b_eval_load_bits (0 = off).  What is
 * wrong with the file is reported before a device is asked for: W2B_EIO "Input file not found" when it cannot be opened,
 * W2B_EINVAL when it is not a W2BP1 file (the reference's float format is not read here), W2B_EIO when it is damaged. */
int w2b_embed_load(const char *w2bp_file, int64_t threshold, int32_t device, w2b_embed **out);
/* The same from packed rows in host memory (w2b_export_packed, w2b_pack_quantized); such a handle has no words. */
int w2b_embed_create(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int32_t device, w2b_embed **out);
void w2b_embed_free(w2b_embed *e);
int64_t w2b_embed_rows(const w2b_embed *e);
int64_t w2b_embed_dim(const w2b_embed *e);
int32_t w2b_embed_bitlevel(const w2b_embed *e);
const char *w2b_embed_word(const w2b_embed *e, int64_t row);      /* NULL on a handle made by _create */
int64_t w2b_embed_search(const w2b_embed *e, const char *word);   /* exact bytes, first match; -1 if absent */

/* Host in, host out: validated before anything is launched.  W2B_EINVAL, with the cause in w2b_last_error(), when an id
 * is >= rows, offsets is not as stated above, a bag is longer than W2B_EMBED_MAX_BAG, dtype or mode is not one of the
 * constants, n or a count is negative; then nothing is launched and `out` is untouched.  n == 0 (n_bags == 0) is W2B_OK.
 * out is [n][dim] ([n_bags][dim]) of float (F32) or uint16_t patterns (BF16, F16).  Large calls run in chunks, so the
 * device staging of the host form stays bounded (64 MiB of output, 2^22 ids or one bag); it is separate from the
 * buffers of w2b_embed_reserve. */
int w2b_embed_lookup(w2b_embed *e, int64_t n, const int32_t *ids, int32_t dtype, void *out);
int w2b_embed_bag(w2b_embed *e, int64_t n_ids, const int32_t *ids, int64_t n_bags, const int64_t *offsets,
                  int32_t mode, int32_t dtype, void *out);

/* Device form: operands in library-owned device buffers, asynchronous on the handle's stream.
 * w2b_embed_reserve hands the buffers out: ids_dev = int64[max_ids] (torch's index type), offsets_dev =
 * int64[max_bags + 1], out_dev = [max(max_ids, max_bags)][dim] of `dtype`.  A later call may grow them; earlier pointers
 * are then stale (a call that asks for no more than is there returns the same pointers).  The caller fills ids_dev /
 * offsets_dev (and makes sure its own stream has finished doing so: the handle's stream waits for nobody), launches, and
 * reads out_dev after w2b_embed_synchronize.  W2B_EINVAL when n, n_ids, n_bags or dtype exceed what was reserved.
 * No content of the staging buffers makes a kernel read or write outside its buffers:
 *   an id >= rows gives a zero row (lookup) or contributes nothing, m included (bag), and is counted;
 *   bag bounds are clamped into [0, n_ids] with start <= end; a clamped bag, or one longer than W2B_EMBED_MAX_BAG, is
 *   pooled over its first W2B_EMBED_MAX_BAG ids and counted once.
 * w2b_embed_bad_ids synchronises, returns that device counter and resets it. */
int w2b_embed_reserve(w2b_embed *e, int64_t max_ids, int64_t max_bags, int32_t dtype,
                      void **ids_dev, void **offsets_dev, void **out_dev);
int w2b_embed_lookup_device(w2b_embed *e, int64_t n, int32_t dtype);
int w2b_embed_bag_device(w2b_embed *e, int64_t n_ids, int64_t n_bags, int32_t mode, int32_t dtype);
int w2b_embed_synchronize(w2b_embed *e);
int w2b_embed_bad_ids(w2b_embed *e, int64_t *count);             /* syncs, returns and resets */
/* Device time (HIP events on the handle's stream) and number of lookup / bag calls launched (host-form chunks count one
 * each) since creation or the last call; synchronises.  bytes = the packed words those launches read (ids x words per row
 * x 8, padding ids included) plus the output bytes they wrote. */
int w2b_embed_timing_read(w2b_embed *e, double *kernel_ms, int64_t *launches, double *bytes);

/* Weighted bag, the semantics above.  Host form: validated before anything is launched, the checks of w2b_embed_bag
 * unchanged; weights == NULL with n_ids > 0 is W2B_EINVAL, and so is the first refused weight on an id >= 0, whose index
 * w2b_last_error() names; then `out` is untouched.  n_bags == 0 is W2B_OK.  Large calls are chunked by whole bags as
 * w2b_embed_bag chunks them, the weights staged beside the ids.
 * Device form: w2b_embed_reserve_weights hands out weights_dev = float[max_ids], a buffer of its own beside the three of
 * w2b_embed_reserve: its pointer goes stale only when the weights buffer itself grows (a call that asks for no more than
 * is there returns the same pointer), and growing the others leaves it valid.  The caller fills ids_dev, weights_dev and
 * offsets_dev and launches; out_dev is that of w2b_embed_reserve.  W2B_EINVAL when n_ids exceeds what either reserve call
 * provided, or n_bags / dtype what w2b_embed_reserve provided.  No content of the staging makes a kernel read or write
 * outside its buffers: the clamping rules of the unweighted device form apply, and a weight that the host form would
 * refuse, on an id that is otherwise valid, makes that id contribute nothing (m included) and is counted once in
 * w2b_embed_bad_ids.  w2b_embed_timing_read counts these launches; their bytes include 4 per id for the weights. */
int w2b_embed_bag_weighted(w2b_embed *e, int64_t n_ids, const int32_t *ids, const float *weights,
                           int64_t n_bags, const int64_t *offsets, int32_t mode, int32_t dtype, void *out);
int w2b_embed_reserve_weights(w2b_embed *e, int64_t max_ids, void **weights_dev);   /* float[max_ids] */
int w2b_embed_bag_weighted_device(w2b_embed *e, int64_t n_ids, int64_t n_bags, int32_t mode, int32_t dtype);

/* Projection, the semantics above.  Host form: validated before anything is launched, in this order: what needs no handle
 * (n or m negative or beyond 2^24 vectors / 0x7FFFFF00 candidates, dtype, x == NULL with n > 0, out == NULL with n > 0 and
 * m > 0), then the handle, then the candidates (cand == NULL with m != rows; the first id >= rows), then the first refused
 * value of x; each is W2B_EINVAL with its cause in w2b_last_error(), and `out` is untouched.  n == 0 or m == 0 is W2B_OK.
 * out is [n][m] of float (F32) or uint16_t patterns (BF16, F16).  Large calls run in chunks of whole vectors x whole
 * candidate ranges, about 64 MiB of output per launch; the result does not depend on the chunking.
 * Device form: w2b_embed_reserve_project hands out x_dev = float[max_n][dim], cand_dev = int64[max_m] and out_dev =
 * [max_n][max_m] of `dtype`, buffers of their own beside those of w2b_embed_reserve and w2b_embed_reserve_weights: a pointer
 * goes stale only when that buffer itself grows (a call that asks for no more than is there returns the same pointers).
 * The caller fills x_dev (and cand_dev), launches, and reads out_dev -- dense [n][m] for the n and m of the call -- after
 * w2b_embed_synchronize.  use_cand = 0 means all rows: m must be rows, so max_m must have been >= rows.  W2B_EINVAL when
 * n, m or dtype exceed what was reserved.  No content of the staging makes a kernel read or write outside its buffers: a
 * candidate >= rows gives a +0.0 column and is counted once in w2b_embed_bad_ids.  The values of x are NOT checked there:
 * what a NaN, an infinity or a value outside 2^-60 .. 2^60 produces is simply what the chain produces on the device.
 * w2b_embed_timing_read counts one launch per call (per chunk of the host form); its bytes are n x dim x 4 for x, m x words
 * per row x 8 for the rows (read once per launch), 8 per candidate id when candidates are given, and the output bytes. */
int w2b_embed_project(w2b_embed *e, int64_t n, const float *x, int64_t m, const int32_t *cand /* or NULL */,
                      int32_t dtype, void *out);
int w2b_embed_reserve_project(w2b_embed *e, int64_t max_n, int64_t max_m, int32_t dtype,
                              void **x_dev /* float[max_n][dim] */, void **cand_dev /* int64[max_m] */,
                              void **out_dev /* [max_n][max_m] of dtype */);
int w2b_embed_project_device(w2b_embed *e, int64_t n, int64_t m, int32_t use_cand, int32_t dtype);

/* Back-projection, the semantics above.  Host form: validated before anything is launched, in the projection's order: what
 * needs no handle (n or m negative or beyond 2^24 vectors / 0x7FFFFF00 candidates, g == NULL with n > 0 and m > 0, dx == NULL
 * with n > 0), then the handle, then the candidates (cand == NULL with m != rows; the first id >= rows), then the first
 * refused value of g; each is W2B_EINVAL with its cause in w2b_last_error(), and `dx` is untouched.  n == 0 is W2B_OK; m == 0
 * writes +0.0 rows.  Large calls run in chunks of whole vectors x candidate ranges that are multiples of W2B_EMBED_WSEG,
 * about 64 MiB of g per launch, S carried from one range to the next; the result does not depend on the chunking.
 * Device form: w2b_embed_reserve_backproject hands out g_dev = float[max_n][max_m], cand_dev = int64[max_m] and dx_dev =
 * float[max_n][dim], buffers of their own beside those of the three other reserve calls: a pointer goes stale only when that
 * buffer itself grows (a call that asks for no more than is there returns the same pointers).  The caller fills g_dev --
 * dense [n][m] for the n and m of the call -- (and cand_dev), launches, and reads dx_dev, dense [n][dim], after
 * w2b_embed_synchronize.  use_cand = 0 means all rows: m must be rows.  W2B_EINVAL when n or m exceed what was reserved.  No
 * content of the staging makes a kernel read or write outside its buffers.  The device scratch for the segments' partial
 * sums is at most 64 MiB, whatever m is: when a call's segments go through it (few vectors x columns, many segments), the
 * driver launches ranges of segments in order and the finishing step carries S; both ways give the same bits.
 * w2b_embed_timing_read counts one launch per call (per chunk of the host form); its bytes are n x m x 4 for g, m x words per
 * row x 8 for the rows, 8 per candidate id when candidates are given, and n x dim x 4 of output. */
int w2b_embed_backproject(w2b_embed *e, int64_t n, const float *g, int64_t m, const int32_t *cand /* or NULL */, float *dx);
int w2b_embed_reserve_backproject(w2b_embed *e, int64_t max_n, int64_t max_m,
                                  void **g_dev /* float[max_n][max_m] */, void **cand_dev /* int64[max_m] */,
                                  void **dx_dev /* float[max_n][dim] */);
int w2b_embed_backproject_device(w2b_embed *e, int64_t n, int64_t m, int32_t use_cand);

/* Cross-entropy, the semantics above.  Host form: validated before anything is launched, in the projection's order: what needs
 * no handle (n or m negative or beyond 2^24 vectors / 0x7FFFFF00 candidates; x, target, mx, se or tl == NULL with n > 0), then
 * the handle, then the candidates (cand == NULL with m != rows; the first id >= rows), then the first refused target (>= m, or
 * on a padding position; W2B_EINVAL naming the vector), then the first refused value of x; each is W2B_EINVAL with its cause in
 * w2b_last_error(), and the outputs are untouched.  n == 0 is W2B_OK.  mx, se, tl are float[n]; dx is float[n][dim], or NULL: no
 * gradient is computed.  Large calls run in ranges of 4096 vectors; the candidate list is staged whole (16 bytes a candidate).
 * Device form: w2b_embed_reserve_xent hands out x_dev = float[max_n][dim], cand_dev = int64[max_m], target_dev = int64[max_n],
 * stats_dev = float[3][max_n] and dx_dev = float[max_n][dim], buffers of their own beside those of the four other reserve
 * calls: a pointer goes stale only when that buffer itself grows (the four per-vector buffers grow together with max_n, cand_dev
 * with max_m; a call that asks for no more than is there returns the same pointers).  The caller fills x_dev, target_dev (and
 * cand_dev), launches, and after w2b_embed_synchronize reads stats_dev -- dense [3][n] for the n of the call: mx at 0, se at n,
 * tl at 2 n -- and, with want_dx = 1, dx_dev, dense [n][dim]; with want_dx = 0 dx_dev is not touched.  use_cand = 0 means all
 * rows: m must be rows.  W2B_EINVAL when n or m exceed what was reserved.  No content of the staging makes a kernel read or
 * write outside its buffers: a candidate >= rows is dead, as padding is, and is counted once in w2b_embed_bad_ids; a target >= m,
 * or on a dead position, makes its vector ignored and is counted once; the values of x are NOT checked.
 * Device memory beyond the reserved buffers: the operand staging of the vectors (about n x dim x 4), a second candidate list
 * (8 m), 12 bytes per (vector, segment) of one statistics launch -- at most 64 MiB, or one range of 64 vectors -- and, with
 * want_dx, at most 64 MiB of g (one vector's candidate range is never cut below W2B_EMBED_WSEG positions) plus the
 * back-projection's scratch: no [n][m] array exists.  The environment variable W2B_EMBED_XENT_SCRATCH (bytes, read per call)
 * lowers the 64 MiB of g, so that the chunked gradient can be exercised at a small shape; the result does not depend on it.
 * w2b_embed_timing_read counts one launch for the statistics of a call (per range of the host form) -- bytes n x dim x 4 for x,
 * m x words per row x 8 for the rows, 8 per candidate id when candidates are given, 8 n of targets and 12 n of results -- and
 * one per chunk of the gradient, n_c vectors x m_c candidate positions: 2 x (m_c x words per row x 8, and 8 m_c with
 * candidates) for the rows read by the gradient kernel and by the back-projection, 2 x n_c x m_c x 4 for g written and read,
 * and 2 x n_c x dim x 4 for x and dx. */
int w2b_embed_xent(w2b_embed *e, int64_t n, const float *x, int64_t m, const int32_t *cand /* or NULL */,
                   const int32_t *target, float *mx, float *se, float *tl, float *dx /* or NULL: no gradient */);
int w2b_embed_reserve_xent(w2b_embed *e, int64_t max_n, int64_t max_m, void **x_dev, void **cand_dev /* int64 */,
                           void **target_dev /* int64[max_n] */, void **stats_dev /* float[3][max_n]: mx, se, tl */,
                           void **dx_dev /* float[max_n][dim] */);
int w2b_embed_xent_device(w2b_embed *e, int64_t n, int64_t m, int32_t use_cand, int32_t want_dx);

/* Top-k, the semantics above.  Host form: validated before anything is launched, in the projection's order: what needs no
 * handle (n or m negative or beyond 2^24 vectors / 0x7FFFFF00 candidates; k outside 1 .. W2B_EMBED_MAX_K; x == NULL, vals == NULL
 * or pos == NULL with n > 0), then the handle, then the candidates (cand == NULL with m != rows; the first id >= rows), then the
 * first refused value of x; each is W2B_EINVAL with its cause in w2b_last_error(), and the outputs are untouched.  n == 0 is
 * W2B_OK; m == 0 writes empty lists (pos = -1, val = -inf).  vals is float[n][k], pos int32_t[n][k].  Large calls run in ranges
 * of 4096 vectors; the candidate list is staged whole (16 bytes a candidate).
 * Device form: w2b_embed_reserve_topk hands out x_dev = float[max_n][dim], cand_dev = int64[max_m], vals_dev =
 * float[max_n][max_k] and pos_dev = int64[max_n][max_k] (torch's index type), buffers of their own beside those of the five
 * other reserve calls: a pointer goes stale only when that buffer itself grows (vals_dev and pos_dev grow together with max_n x
 * max_k; a call that asks for no more than is there returns the same pointers).  The caller fills x_dev (and cand_dev),
 * launches, and after w2b_embed_synchronize reads vals_dev and pos_dev -- dense [n][k] for the n and k of the call.  use_cand =
 * 0 means all rows: m must be rows.  W2B_EINVAL when n, m or n x k exceed what was reserved, or k is outside 1 ..
 * W2B_EMBED_MAX_K.  No content of the staging makes a kernel read or write outside its buffers: a candidate >= rows is dead, as
 * padding is, and is counted once in w2b_embed_bad_ids; the values of x are NOT checked.
 * Device memory beyond the reserved buffers: the operand staging of the vectors (about n x dim x 4), a second candidate list
 * (8 m), and the selection scratch: per vector of a range, for every UNIT of 64 consecutive candidate positions the unit's
 * largest key (8 bytes), and a list of 64 k keys of 8 bytes -- the k-th largest of the unit maxima is a threshold that at most
 * k units reach, and only keys at or above it are ever listed --, ceil(m / 64) x 8 + 512 k + 16 bytes a vector.  A range is as
 * many vectors, a multiple of 64, as keep that within 64 MiB, or 64 vectors -- one pair of 32-vector tiles -- if those need
 * more; a call of more vectors runs range after range.  No [n][m] array exists.  The environment variable
 * W2B_EMBED_TOPK_SCRATCH (bytes, read per call) lowers the 64 MiB, so that the ranges can be exercised at a small shape; the
 * result does not depend on it.
 * w2b_embed_timing_read counts one launch per range of vectors (of n_c vectors).  A range runs the K loop over all m
 * candidates TWICE (the unit maxima, then the keys at or above the threshold), so its bytes are 2 x (n_c x dim x 4 for x, m x
 * words per row x 8 for the rows, 8 per candidate id when candidates are given), and n_c x k x 12 of results.  The traffic of
 * the scratch (8 bytes per vector and unit written and read, the listed keys written and read) is not counted. */
int w2b_embed_topk(w2b_embed *e, int64_t n, const float *x, int64_t m, const int32_t *cand /* or NULL */, int32_t k,
                   float *vals /* [n][k] */, int32_t *pos /* [n][k] */);
int w2b_embed_reserve_topk(w2b_embed *e, int64_t max_n, int64_t max_m, int32_t max_k, void **x_dev, void **cand_dev /* int64[max_m] */,
                           void **vals_dev /* float[max_n][max_k] */, void **pos_dev /* int64[max_n][max_k] */);
int w2b_embed_topk_device(w2b_embed *e, int64_t n, int64_t m, int32_t use_cand, int32_t k);

/* Host twins, pure C, no device: float32 results with the semantics above, the validation of the host form.  All of them are in
 * w2b_embed_twins.cpp, a host-only unit that the host sanitizers run on its own. */
int w2b_embed_lookup_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel,
                          int64_t n, const int32_t *ids, float *out);
int w2b_embed_bag_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n_ids,
                       const int32_t *ids, int64_t n_bags, const int64_t *offsets, int32_t mode, float *out);
/* the weighted bag: explicit fmaf per id, the segments and the steps exactly as stated above */
int w2b_embed_bag_weighted_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel,
                                int64_t n_ids, const int32_t *ids, const float *weights,
                                int64_t n_bags, const int64_t *offsets, int32_t mode, float *out);
/* the projection: explicit fmaf per column, then the one multiply */
int w2b_embed_project_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n,
                           const float *x, int64_t m, const int32_t *cand, float *out);
/* the back-projection: explicit fmaf per candidate position, the segments and the steps exactly as stated above */
int w2b_embed_backproject_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n,
                               const float *g, int64_t m, const int32_t *cand, float *dx);

/* the cross-entropy from the definition: explicit loops, the segments of W2B_EMBED_XSEG, dx through the back-projection's chains */
int w2b_embed_xent_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n, const float *x,
                        int64_t m, const int32_t *cand, const int32_t *target, float *mx, float *se, float *tl, float *dx);
float w2b_embed_expneg_host(float r);   /* the shared definition of expneg, for the tests */
/* the top-k selection from the definition: the projection's twin, the keys of the live positions, their k largest in order */
int w2b_embed_topk_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n, const float *x,
                        int64_t m, const int32_t *cand, int32_t k, float *vals, int32_t *pos);

#ifdef __cplusplus
}
#endif
#endif
