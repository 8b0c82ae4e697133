// w2b_embed_twins.cpp -- the host twins of the packed embedding's kernels (include/word2bits_embed.h), all seven: lookup, bags,
// weighted bags, projection, back-projection, cross-entropy and top-k selection.  They are what every GPU test of the embedding compares the
// kernels against.  They restate the header's definitions on the packed rows themselves: one decode of a row into its codes,
// then the stated float32 steps in the stated order.  No handle, no stream and no device call: the unit includes no device
// header, and a program that links nothing but this file and a w2b_internal_fail of its own can run it under a host sanitizer
// (tests/host/embed_*_twin_main.cpp, `make host-check`).  What it refuses comes from w2b_embed_shared.h, as for the host form.
// Every product and sum here is one float32 operation: this file is built with -ffp-contract=off and each function says so again.
#include "w2b_embed_shared.h"

#include <algorithm>
#include <cmath>
#include <functional>
#include <vector>

namespace {
// words of one packed row (w2b_packed_words_per_row of a shape that check_shape has let through)
int64_t words_per_row(int64_t dim, int32_t bitlevel) { return (dim + 63) / 64 * bitlevel; }

// q of the header: a value of the table is its code times q, 1/3 (as 0x3EAAAAAB) at one bit and 1/4 at two
float code_scale(int32_t bitlevel) { return __builtin_bit_cast(float, bitlevel == 1 ? 0x3EAAAAABu : 0x3E800000u); }

// The codes of one packed row, written ONCE: per 64 columns one word of sign bits (set = negative) and, at two bits, one word
// of magnitude bits (set = 3, clear = 1).  t[a] = +-1, or +-1 / +-3; the padding bits of the last block are never looked at.
template <class T>
void decode_row(const uint64_t *row, int64_t dim, int32_t bitlevel, T *t) {
  for (int64_t a = 0; a < dim; a++) {
    const uint64_t *blk = row + (a >> 6) * bitlevel;
    const int sg = (int)((blk[0] >> (a & 63)) & 1u);
    const int mag = bitlevel == 2 && ((blk[1] >> (a & 63)) & 1u) ? 3 : 1;
    t[a] = (T)(sg ? -mag : mag);
  }
}

// what a bag leaves: sum = acc * q, one float32 multiply; mean = sum / (float)m with m the ids >= 0, +0.0 for m == 0
float bag_value(float acc, float q, int32_t mode, int32_t m) {
#pragma clang fp contract(off)
  const float sum = acc * q;
  return mode == W2B_EMBED_MEAN ? (m > 0 ? sum / (float)m : 0.f) : sum;
}
}  // namespace

// The patterns of w2b_unpack_quantized, assembled from the codes with integer operations: no float arithmetic on this path.
extern "C" int w2b_embed_lookup_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n,
                                     const int32_t *ids, float *out) {
#pragma clang fp contract(off)
  const char *who = "w2b_embed_lookup_host";
  if (int rc = check_table(who, packed, rows, dim, bitlevel)) return rc;
  if (int rc = check_ids(who, rows, n, ids)) return rc;
  if (n == 0) return W2B_OK;
  if (!out) return refuse(W2B_EINVAL, who, "null output");
  const int64_t wpr = words_per_row(dim, bitlevel);
  std::vector<int32_t> t((size_t)dim);
  for (int64_t i = 0; i < n; i++) {
    float *o = out + i * dim;
    if (ids[i] < 0) {
      for (int64_t c = 0; c < dim; c++) o[c] = 0.f;
      continue;
    }
    decode_row(packed + (int64_t)ids[i] * wpr, dim, bitlevel, t.data());
    for (int64_t c = 0; c < dim; c++) {
      const int32_t code = t[(size_t)c];
      const uint32_t mag = bitlevel == 1 ? 0x3EAAAAABu : (code == 3 || code == -3 ? 0x3F400000u : 0x3E800000u);
      o[c] = __builtin_bit_cast(float, mag | (code < 0 ? 0x80000000u : 0u));
    }
  }
  return W2B_OK;
}

// T[a] = the integer sum of the codes over the bag's ids >= 0, then the steps of bag_value
extern "C" int w2b_embed_bag_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n_ids,
                                  const int32_t *ids, int64_t n_bags, const int64_t *offsets, int32_t mode, float *out) {
#pragma clang fp contract(off)
  const char *who = "w2b_embed_bag_host";
  if (int rc = check_table(who, packed, rows, dim, bitlevel)) return rc;
  if (int rc = check_ids(who, rows, n_ids, ids)) return rc;
  if (int rc = check_bags(who, n_ids, n_bags, offsets, mode)) return rc;
  if (n_bags == 0) return W2B_OK;
  if (!out) return refuse(W2B_EINVAL, who, "null output");
  const int64_t wpr = words_per_row(dim, bitlevel);
  const float q = code_scale(bitlevel);
  std::vector<int32_t> t((size_t)dim), T((size_t)dim);
  for (int64_t b = 0; b < n_bags; b++) {
    for (int32_t &v : T) v = 0;
    int32_t m = 0;
    for (int64_t i = offsets[b]; i < offsets[b + 1]; i++) {
      if (ids[i] < 0) continue;
      m++;
      decode_row(packed + (int64_t)ids[i] * wpr, dim, bitlevel, t.data());
      for (int64_t c = 0; c < dim; c++) T[(size_t)c] += t[(size_t)c];
    }
    for (int64_t c = 0; c < dim; c++) out[b * dim + c] = bag_value((float)T[(size_t)c], q, mode, m);
  }
  return W2B_OK;
}

// Segments of W2B_EMBED_WSEG positions from the bag's start; P_s = +0, P_s = fmaf(w, (float)t_r[a], P_s) over the segment's
// ids >= 0 in order; S = S + P_s in segment order, one float32 add each; then the steps of bag_value with the unweighted m.
extern "C" int w2b_embed_bag_weighted_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n_ids,
                                           const int32_t *ids, const float *weights, int64_t n_bags, const int64_t *offsets,
                                           int32_t mode, float *out) {
#pragma clang fp contract(off)
  const char *who = "w2b_embed_bag_weighted_host";
  if (int rc = check_table(who, packed, rows, dim, bitlevel)) return rc;
  if (int rc = check_ids(who, rows, n_ids, ids)) return rc;
  if (int rc = check_bags(who, n_ids, n_bags, offsets, mode)) return rc;
  if (int rc = check_weights(who, n_ids, ids, weights)) return rc;
  if (n_bags == 0) return W2B_OK;
  if (!out) return refuse(W2B_EINVAL, who, "null output");
  const int64_t wpr = words_per_row(dim, bitlevel);
  const float q = code_scale(bitlevel);
  std::vector<float> t((size_t)dim), P((size_t)dim), S((size_t)dim);
  for (int64_t b = 0; b < n_bags; b++) {
    for (float &v : S) v = 0.f;
    int32_t m = 0;
    for (int64_t s0 = offsets[b]; s0 < offsets[b + 1]; s0 += W2B_EMBED_WSEG) {      // one segment: one chain per column
      const int64_t s1 = s0 + W2B_EMBED_WSEG < offsets[b + 1] ? s0 + W2B_EMBED_WSEG : offsets[b + 1];
      for (float &v : P) v = 0.f;
      for (int64_t i = s0; i < s1; i++) {
        if (ids[i] < 0) continue;
        m++;
        const float w = weights[i];
        decode_row(packed + (int64_t)ids[i] * wpr, dim, bitlevel, t.data());
        for (int64_t c = 0; c < dim; c++) P[(size_t)c] = fmaf(w, t[(size_t)c], P[(size_t)c]);
      }
      for (int64_t c = 0; c < dim; c++) S[(size_t)c] = S[(size_t)c] + P[(size_t)c];     // one float32 add per segment
    }
    for (int64_t c = 0; c < dim; c++) out[b * dim + c] = bag_value(S[(size_t)c], q, mode, m);
  }
  return W2B_OK;
}

// S = +0; S = fmaf(x[i][a], (float)t_r[a], S) for a = 0 .. dim - 1; out[i][j] = S * q, one float32 multiply.
extern "C" int w2b_embed_project_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n,
                                      const float *x, int64_t m, const int32_t *cand, float *out) {
#pragma clang fp contract(off)
  const char *who = "w2b_embed_project_host";
  if (int rc = project_check_args(who, n, x, m, W2B_EMBED_F32, out)) return rc;
  if (int rc = check_table(who, packed, rows, dim, bitlevel)) return rc;
  if (int rc = project_check_cand(who, rows, m, cand)) return rc;
  if (int rc = project_check_values(who, n, dim, x)) return rc;
  if (n == 0 || m == 0) return W2B_OK;
  const int64_t wpr = words_per_row(dim, bitlevel);
  const float q = code_scale(bitlevel);
  std::vector<float> t((size_t)dim);
  for (int64_t j = 0; j < m; j++) {
    const int64_t r = cand ? (int64_t)cand[j] : j;
    if (r < 0) {                                             // padding: a column of +0.0
      for (int64_t i = 0; i < n; i++) out[i * m + j] = 0.f;
      continue;
    }
    decode_row(packed + r * wpr, dim, bitlevel, t.data());
    for (int64_t i = 0; i < n; i++) {
      const float *xi = x + i * dim;
      float S = 0.f;
      for (int64_t a = 0; a < dim; a++) S = fmaf(xi[a], t[(size_t)a], S);      // strictly sequential, one accumulator
      out[i * m + j] = S * q;
    }
  }
  return W2B_OK;
}

// The back-projection's arithmetic, nothing refused: per vector and column, segments of W2B_EMBED_WSEG candidate positions
// counted from position 0; P_s = +0, P_s = fmaf(g[i][j], (float)t_r[a], P_s) over the live positions of the segment in
// order; S = S + P_s in segment order, one float32 add each; dx = S * q, one float32 multiply.  (w2b_embed_xent_host sends
// its own g through it: a g it has computed, not one a caller supplies.)
static void backproject_chains(const uint64_t *packed, int64_t dim, int32_t bitlevel, int64_t n, const float *g, int64_t m,
                               const int32_t *cand, float *dx) {
#pragma clang fp contract(off)
  const int64_t wpr = words_per_row(dim, bitlevel);
  const float q = code_scale(bitlevel);
  std::vector<float> t((size_t)dim), P((size_t)(n * dim)), S((size_t)(n * dim), 0.f);
  for (int64_t s0 = 0; s0 < m; s0 += W2B_EMBED_WSEG) {       // one segment: one chain per (vector, column)
    const int64_t s1 = s0 + W2B_EMBED_WSEG < m ? s0 + W2B_EMBED_WSEG : m;
    for (size_t k = 0; k < P.size(); k++) P[k] = 0.f;
    for (int64_t j = s0; j < s1; j++) {
      const int64_t r = cand ? (int64_t)cand[j] : j;
      if (r < 0) continue;                                   // padding: g is not looked at
      decode_row(packed + r * wpr, dim, bitlevel, t.data());
      for (int64_t i = 0; i < n; i++) {
        const float w = g[i * m + j];
        float *Pi = P.data() + i * dim;
        for (int64_t a = 0; a < dim; a++) Pi[a] = fmaf(w, t[(size_t)a], Pi[a]);
      }
    }
    for (size_t k = 0; k < S.size(); k++) S[k] = S[k] + P[k];                  // one float32 add per segment
  }
  for (size_t k = 0; k < S.size(); k++) dx[k] = S[k] * q;                       // one float32 multiply
}

// The back-projection: the validation of the host form, then the chains above.
extern "C" int w2b_embed_backproject_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n,
                                          const float *g, int64_t m, const int32_t *cand, float *dx) {
#pragma clang fp contract(off)
  const char *who = "w2b_embed_backproject_host";
  if (int rc = backproject_check_args(who, n, g, m, dx)) return rc;
  if (int rc = check_table(who, packed, rows, dim, bitlevel)) return rc;
  if (int rc = project_check_cand(who, rows, m, cand)) return rc;
  if (int rc = backproject_check_values(who, n, m, cand, g)) return rc;
  if (n == 0) return W2B_OK;
  backproject_chains(packed, dim, bitlevel, n, g, m, cand, dx);
  return W2B_OK;
}

// expneg of include/word2bits_embed.h, "Cross-entropy": the text of w2b_embed_shared.h, which the kernels compile too
extern "C" float w2b_embed_expneg_host(float r) { return w2b_expneg(r); }

// The cross-entropy, from the definition: per vector the logits of the projection (its twin above), the segments of
// W2B_EMBED_XSEG positions with their exact maximum M_s and their integer sum U_s, then mx, the sequential se, tl, and -- when
// dx is wanted -- the g of step 5 sent through the back-projection's chains.
extern "C" int w2b_embed_xent_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n, const float *x,
                                   int64_t m, const int32_t *cand, const int32_t *target, float *mx, float *se, float *tl,
                                   float *dx) {
#pragma clang fp contract(off)
  const char *who = "w2b_embed_xent_host";
  if (int rc = xent_check_args(who, n, x, m, target, mx, se, tl)) return rc;
  if (int rc = check_table(who, packed, rows, dim, bitlevel)) return rc;
  if (int rc = project_check_cand(who, rows, m, cand)) return rc;
  if (int rc = xent_check_targets(who, n, m, cand, target)) return rc;
  if (int rc = project_check_values(who, n, dim, x)) return rc;
  const int64_t nseg = (m + W2B_EMBED_XSEG - 1) / W2B_EMBED_XSEG;
  std::vector<float> l((size_t)m + 1), g(dx ? (size_t)m + 1 : 1), M((size_t)nseg + 1);
  std::vector<uint64_t> U((size_t)nseg + 1);
  for (int64_t i = 0; i < n; i++) {
    if (int rc = w2b_embed_project_host(packed, rows, dim, bitlevel, 1, x + i * dim, m, cand, l.data())) return rc;
    bool any = false;
    float top = 0.f;
    for (int64_t s = 0; s < nseg; s++) {
      const int64_t j0 = s * W2B_EMBED_XSEG, j1 = j0 + W2B_EMBED_XSEG < m ? j0 + W2B_EMBED_XSEG : m;
      bool have = false;
      float Ms = 0.f;
      for (int64_t j = j0; j < j1; j++)
        if (!cand || cand[j] >= 0) {
          if (!have || l[(size_t)j] > Ms) Ms = l[(size_t)j];
          have = true;
        }
      uint64_t Us = 0;
      for (int64_t j = j0; j < j1 && have; j++)
        if (!cand || cand[j] >= 0) Us += w2b_xent_term(l[(size_t)j], Ms);
      M[(size_t)s] = Ms;
      U[(size_t)s] = have ? Us : 0;                          // a live segment has U_s >= 2^32: its maximum contributes 1
      if (have && (!any || Ms > top)) top = Ms;
      any = any || have;
    }
    float sum = 0.f;
    for (int64_t s = 0; s < nseg && any; s++)
      if (U[(size_t)s]) sum = w2b_xent_se_step(U[(size_t)s], M[(size_t)s], top, sum);
    mx[i] = any ? top : 0.f;
    se[i] = sum;
    tl[i] = target[i] >= 0 ? l[(size_t)target[i]] : 0.f;
    if (!dx) continue;
    for (int64_t j = 0; j < m; j++)
      g[(size_t)j] = target[i] >= 0 && (!cand || cand[j] >= 0) ? w2b_xent_g(l[(size_t)j], mx[i], se[i], j == target[i]) : 0.f;
    backproject_chains(packed, dim, bitlevel, 1, g.data(), m, cand, dx + i * dim);
  }
  return W2B_OK;
}

// The top-k selection, from the definition: per vector the logits of the projection (its twin above), the keys of the live
// positions -- the order-preserving map of the logit's bits above the complement of the position --, and the k largest keys
// in descending order; the list ends in pos = -1, val = -inf.
extern "C" int w2b_embed_topk_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n, const float *x,
                                   int64_t m, const int32_t *cand, int32_t k, float *vals, int32_t *pos) {
  const char *who = "w2b_embed_topk_host";
  if (int rc = topk_check_args(who, n, x, m, k, vals, pos)) return rc;
  if (int rc = check_table(who, packed, rows, dim, bitlevel)) return rc;
  if (int rc = project_check_cand(who, rows, m, cand)) return rc;
  if (int rc = project_check_values(who, n, dim, x)) return rc;
  const int64_t block = 32;                                  // vectors whose logits are held at a time: a row is decoded once for them
  std::vector<float> l((size_t)(block * m) + 1);
  std::vector<uint64_t> keys;
  for (int64_t i0 = 0; i0 < n; i0 += block) {
    const int64_t ni = n - i0 < block ? n - i0 : block;
    if (int rc = w2b_embed_project_host(packed, rows, dim, bitlevel, ni, x + i0 * dim, m, cand, l.data())) return rc;
    for (int64_t i = i0; i < i0 + ni; i++) {
      const float *li = l.data() + (i - i0) * m;
      keys.clear();
      for (int64_t j = 0; j < m; j++)
        if (!cand || cand[j] >= 0) keys.push_back(w2b_topk_key(__builtin_bit_cast(uint32_t, li[j]), (uint32_t)j));
      const size_t have = keys.size() < (size_t)k ? keys.size() : (size_t)k;
      std::partial_sort(keys.begin(), keys.begin() + (std::ptrdiff_t)have, keys.end(), std::greater<uint64_t>());
      for (size_t c = 0; c < (size_t)k; c++) {
        const bool live = c < have;
        vals[i * k + (int64_t)c] = __builtin_bit_cast(float, live ? w2b_topk_unmap((uint32_t)(keys[c] >> 32)) : 0xFF800000u);
        pos[i * k + (int64_t)c] = live ? (int32_t)~(uint32_t)keys[c] : -1;
      }
    }
  }
  return W2B_OK;
}
