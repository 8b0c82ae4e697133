// w2b_eval_twins.cpp -- the host twins of the evaluator's kernels (include/word2bits_eval.h): what every GPU test of the
// evaluator compares a kernel against.  Each one restates its definition of the header on the packed rows themselves, in
// integer and float arithmetic one step at a time.  No handle, no stream and no device call: the unit includes no device
// header, and a program that links nothing but this file and a w2b_internal_fail of its own can run it under a host
// sanitizer (tests/host/eval_twins_main.cpp, `make host-check`).  What a twin must refuse or compute exactly as the device
// entry point does comes from w2b_eval_shared.h.  The float sequences are asserted bit for bit: the file is built with
// -ffp-contract=off, and every function with one says so again.
#include "w2b_eval_shared.h"

#include <cstring>

// host twin of the bits kernels: I(c) of every row, from the three Hamming distances of the definition
extern "C" int w2b_bits_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int64_t b1, int64_t b2, int64_t b3,
                                    int32_t *I_out) {
  if (!packed || !I_out || words < 0 || dim < 1 || b1 < 0 || b2 < 0 || b3 < 0 || b1 >= words || b2 >= words || b3 >= words)
    return efail(W2B_EINVAL, "w2b_bits_scores_host: bad argument");
  const int64_t wpr = (dim + 63) / 64;
  const uint64_t *r1 = packed + b1 * wpr, *r2 = packed + b2 * wpr, *r3 = packed + b3 * wpr;
  for (int64_t c = 0; c < words; c++) {
    const uint64_t *rc = packed + c * wpr;
    int64_t h1 = 0, h2 = 0, h3 = 0;
    for (int64_t w = 0; w < wpr; w++) {
      const uint64_t valid = (w + 1) * 64 <= dim ? ~0ull : (1ull << (dim - w * 64)) - 1;    // padding bits do not count
      h1 += __builtin_popcountll((r1[w] ^ rc[w]) & valid);
      h2 += __builtin_popcountll((r2[w] ^ rc[w]) & valid);
      h3 += __builtin_popcountll((r3[w] ^ rc[w]) & valid);
    }
    I_out[c] = (int32_t)(dim - 2 * (h2 - h1 + h3));
  }
  return W2B_OK;
}

// host twin of the bits form of w2b_eval_combine: I(c) = sum over the used slots of sign * (dim - 2 * Hamming(r, c))
extern "C" int w2b_bits_combine_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t nt,
                                            const int32_t *rows, const int8_t *signs, int32_t *I_out) {
  const std::string who = "w2b_bits_combine_scores_host";
  if (!packed || !rows || !signs || !I_out || words < 0 || dim < 1) return efail(W2B_EINVAL, who + ": bad argument");
  if (nt < 1 || nt > W2B_EVAL_MAX_TERMS) return efail(W2B_EINVAL, who + ": the number of terms must be 1..7");
  if (const char *why = bad_terms(nt, rows, signs, words)) return efail(W2B_EINVAL, who + ": " + why);
  const int64_t wpr = (dim + 63) / 64;
  for (int64_t c = 0; c < words; c++) {
    const uint64_t *rc = packed + c * wpr;
    int64_t I = 0;
    for (int32_t t = 0; t < nt; t++) {
      if (signs[t] == 0) continue;
      const uint64_t *rt = packed + (int64_t)rows[t] * wpr;
      int64_t h = 0;
      for (int64_t w = 0; w < wpr; w++) {
        const uint64_t valid = (w + 1) * 64 <= dim ? ~0ull : (1ull << (dim - w * 64)) - 1;    // padding bits do not count
        h += __builtin_popcountll((rt[w] ^ rc[w]) & valid);
      }
      I += signs[t] * (dim - 2 * h);
    }
    I_out[c] = (int32_t)I;
  }
  return W2B_OK;
}

// Host twin of the codes kernels.  The float sequence of the header, one rounding per operation: this file is built with
// -ffp-contract=off and the function's body repeats it, so that no build fuses p * w + p.
extern "C" int w2b_codes_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int64_t b1, int64_t b2, int64_t b3,
                                     int32_t *J_out, float *score_out) {
#pragma clang fp contract(off)
  if (!packed || words < 0 || dim < 1 || b1 < 0 || b2 < 0 || b3 < 0 || b1 >= words || b2 >= words || b3 >= words)
    return efail(W2B_EINVAL, "w2b_codes_scores_host: bad argument");
  const int64_t nb = (dim + 63) / 64, wpr = 2 * nb;
  const std::vector<float> wt = codes_weights(dim);
  auto valid = [&](int64_t b) { return (b + 1) * 64 <= dim ? ~0ull : (1ull << (dim - b * 64)) - 1; };   // padding bits do not count
  auto weight = [&](const uint64_t *r) {
    int64_t n3 = 0;
    for (int64_t b = 0; b < nb; b++) n3 += __builtin_popcountll(r[2 * b + 1] & valid(b));
    return wt[(size_t)n3];
  };
  // sum_a t_x t_c over a block: |t_x t_c| is 1 + 2 m_x + 2 m_c + 4 m_x m_c, its sign that of s_x ^ s_c
  auto dot = [&](const uint64_t *x, const uint64_t *c) {
    int64_t j = 0;
    for (int64_t b = 0; b < nb; b++) {
      const uint64_t v = valid(b), neg = (x[2 * b] ^ c[2 * b]) & v, pos = ~neg & v;
      const uint64_t mx = x[2 * b + 1], mc = c[2 * b + 1];
      auto mag = [&](uint64_t m) {
        return (int64_t)__builtin_popcountll(m) + 2 * __builtin_popcountll(m & mx) + 2 * __builtin_popcountll(m & mc) +
               4 * __builtin_popcountll(m & mx & mc);
      };
      j += mag(pos) - mag(neg);
    }
    return (int32_t)j;
  };
  const uint64_t *r1 = packed + b1 * wpr, *r2 = packed + b2 * wpr, *r3 = packed + b3 * wpr;
  const float w1 = weight(r1), w2 = weight(r2), w3 = weight(r3);
  for (int64_t c = 0; c < words; c++) {
    const uint64_t *rc = packed + c * wpr;
    const int32_t j1 = dot(r1, rc), j2 = dot(r2, rc), j3 = dot(r3, rc);
    if (J_out) {
      J_out[c] = j1;
      J_out[words + c] = j2;
      J_out[2 * words + c] = j3;
    }
    if (score_out) {
      const float p1 = (float)j1 * w1, p2 = (float)j2 * w2, p3 = (float)j3 * w3;
      const float d = p2 - p1;
      const float s = d + p3;
      score_out[c] = s * weight(rc);
    }
  }
  return W2B_OK;
}

// Host twin of the 3CosMul kernels.  The float sequence of the header, one rounding per operation (this file is built with
// -ffp-contract=off, and the function says so again).
extern "C" int w2b_cosmul_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, int64_t b1,
                                      int64_t b2, int64_t b3, float *u_out, float *score_out) {
#pragma clang fp contract(off)
  const std::string who = "w2b_cosmul_scores_host";
  if (!packed || words < 0 || dim < 1) return efail(W2B_EINVAL, who + ": bad argument");
  if (bitlevel != 1 && bitlevel != 2) return efail(W2B_EINVAL, who + ": bitlevel must be 1 or 2");
  if (bitlevel == 1 && dim > kCosmulMaxBits) return efail(W2B_EINVAL, who + ": size must be at most 2^24 on 1-bit rows");
  if (b1 < 0 || b2 < 0 || b3 < 0 || b1 >= words || b2 >= words || b3 >= words)
    return efail(W2B_EINVAL, who + ": question row out of range");
  const int64_t b[3] = {b1, b2, b3};
  const int64_t nb = (dim + 63) / 64, wpr = nb * bitlevel;
  auto valid = [&](int64_t blk) { return (blk + 1) * 64 <= dim ? ~0ull : (1ull << (dim - blk * 64)) - 1; };   // padding bits do not count
  std::vector<float> u((size_t)(3 * words));
  if (bitlevel == 1) {
    const std::vector<float> ut = cosmul_utab(dim);
    for (int t = 0; t < 3; t++) {
      const uint64_t *rt = packed + b[t] * wpr;
      for (int64_t c = 0; c < words; c++) {
        const uint64_t *rc = packed + c * wpr;
        int64_t h = 0;
        for (int64_t w = 0; w < nb; w++) h += __builtin_popcountll((rt[w] ^ rc[w]) & valid(w));
        u[(size_t)(t * words + c)] = ut[(size_t)(dim - h)];
      }
    }
  } else {
    std::vector<int32_t> J((size_t)(3 * words));
    if (int rc = w2b_codes_scores_host(packed, words, dim, b1, b2, b3, J.data(), nullptr)) return rc;
    const std::vector<float> wt = codes_weights(dim);
    auto weight = [&](const uint64_t *r) {
      int64_t n3 = 0;
      for (int64_t blk = 0; blk < nb; blk++) n3 += __builtin_popcountll(r[2 * blk + 1] & valid(blk));
      return wt[(size_t)n3];
    };
    for (int t = 0; t < 3; t++) {
      const float wb = weight(packed + b[t] * wpr);
      for (int64_t c = 0; c < words; c++) {
        const float pj = (float)J[(size_t)(t * words + c)] * wb;
        const float cs = pj * weight(packed + c * wpr);
        const float one = 1.0f + cs;
        u[(size_t)(t * words + c)] = one * 0.5f;
      }
    }
  }
  if (u_out) memcpy(u_out, u.data(), u.size() * 4);
  if (score_out)
    for (int64_t c = 0; c < words; c++)
      score_out[c] = cosmul_score(u[(size_t)c], u[(size_t)(words + c)], u[(size_t)(2 * words + c)]);
  return W2B_OK;
}

// Host twin of the rank question: the definition of the header on the scores of w2b_bits_scores_host / w2b_codes_scores_host,
// one question.  Equal scores are equal integers on 1-bit rows and equal floats on 2-bit rows.
extern "C" int w2b_rank_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, int64_t b1, int64_t b2,
                             int64_t b3, int64_t target, int32_t *rank, int32_t *tied, float *score) {
  const std::string who = "w2b_rank_host";
  if (!packed || !rank || words < 0 || dim < 1) return efail(W2B_EINVAL, who + ": bad argument");
  if (bitlevel != 1 && bitlevel != 2) return efail(W2B_EINVAL, who + ": bitlevel must be 1 or 2");
  if (b1 < 0 || b2 < 0 || b3 < 0 || target < 0 || b1 >= words || b2 >= words || b3 >= words || target >= words)
    return efail(W2B_EINVAL, who + ": row out of range");
  std::vector<int32_t> I;
  std::vector<float> S;
  if (bitlevel == 1) {
    I.resize((size_t)words);
    if (int rc = w2b_bits_scores_host(packed, words, dim, b1, b2, b3, I.data())) return rc;
  } else {
    S.resize((size_t)words);
    if (int rc = w2b_codes_scores_host(packed, words, dim, b1, b2, b3, nullptr, S.data())) return rc;
  }
  // -1 / 0 / +1: does row c stand behind / with / before a row of the target's score?
  auto cmp = [&](int64_t c) {
    if (bitlevel == 1) return I[(size_t)c] > I[(size_t)target] ? 1 : I[(size_t)c] == I[(size_t)target] ? 0 : -1;
    return S[(size_t)c] > S[(size_t)target] ? 1 : S[(size_t)c] == S[(size_t)target] ? 0 : -1;
  };
  const bool own = target == b1 || target == b2 || target == b3;
  const bool ranked = !own && (bitlevel == 1 ? I[(size_t)target] > 0 : S[(size_t)target] > 0.0f);
  int32_t r = 0, t = 0;
  if (ranked) {
    r = 1;
    for (int64_t c = 0; c < words; c++) {
      if (c == b1 || c == b2 || c == b3 || c == target) continue;
      const int k = cmp(c);
      if (k > 0 || (k == 0 && c < target)) r++;
      if (k == 0) t++;
    }
  }
  *rank = r;
  if (tied) *tied = t;
  if (score) *score = !ranked ? 0.0f : bitlevel == 1 ? (float)I[(size_t)target] / (float)dim : S[(size_t)target];
  return W2B_OK;
}

// Host twin of the bag kernels: T from the unpacked rows, J in 64 bits, the float steps of the header one at a time (this
// file is built with -ffp-contract=off, and the function says so again).
extern "C" int w2b_bag_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, int64_t n,
                                   const int32_t *ids, int32_t *J_out, float *score_out) {
#pragma clang fp contract(off)
  const std::string who = "w2b_bag_scores_host";
  if (!packed || words < 0 || dim < 1 || (n > 0 && !ids)) return efail(W2B_EINVAL, who + ": bad argument");
  if (bitlevel != 1 && bitlevel != 2) return efail(W2B_EINVAL, who + ": bitlevel must be 1 or 2");
  if (dim > kBagMaxSize) return efail(W2B_EINVAL, who + ": size must be at most 58254 (9 * 4096 * size < 2^31)");
  if (const char *why = bad_bag(n, ids, words)) return efail(W2B_EINVAL, who + ": " + why);
  const int64_t nb = (dim + 63) / 64, wpr = nb * bitlevel;
  auto t_of = [&](const uint64_t *r, int64_t a) -> int32_t {
    const uint64_t bit = 1ull << (a & 63);
    if (bitlevel == 1) return (r[a >> 6] & bit) ? -1 : 1;
    return ((r[2 * (a >> 6) + 1] & bit) ? 3 : 1) * ((r[2 * (a >> 6)] & bit) ? -1 : 1);
  };
  std::vector<int32_t> T((size_t)dim, 0);
  for (int64_t i = 0; i < n; i++)
    if (ids[i] >= 0)
      for (int64_t a = 0; a < dim; a++) T[(size_t)a] += t_of(packed + (int64_t)ids[i] * wpr, a);
  unsigned long long nt = 0;
  for (int64_t a = 0; a < dim; a++) nt += (unsigned long long)((int64_t)T[(size_t)a] * T[(size_t)a]);
  const float wq = bag_weight(nt);
  const std::vector<float> wt = bitlevel == 2 ? codes_weights(dim) : std::vector<float>();
  for (int64_t c = 0; c < words; c++) {
    const uint64_t *rc = packed + c * wpr;
    int64_t j = 0, n3 = 0;
    for (int64_t a = 0; a < dim; a++) {
      const int32_t t = t_of(rc, a);
      j += (int64_t)T[(size_t)a] * t;
      n3 += t == 3 || t == -3;
    }
    if (J_out) J_out[c] = (int32_t)j;
    if (!score_out) continue;
    if (bitlevel == 1) {
      score_out[c] = (float)(int32_t)j / (float)dim;
    } else {
      const float pj = (float)(int32_t)j * wq;
      score_out[c] = pj * wt[(size_t)n3];
    }
  }
  return W2B_OK;
}

// Host twin of the vector kernels: the fmaf chain of the header in column order, then the two multiplies one at a time (this
// file is built with -ffp-contract=off, and the function says so again).
extern "C" int w2b_vector_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, const float *x,
                                      int32_t normalize, float *S_out, float *score_out) {
#pragma clang fp contract(off)
  const std::string who = "w2b_vector_scores_host";
  if (!packed || !x || words < 0 || dim < 1) return efail(W2B_EINVAL, who + ": bad argument");
  if (bitlevel != 1 && bitlevel != 2) return efail(W2B_EINVAL, who + ": bitlevel must be 1 or 2");
  if (normalize != 0 && normalize != 1) return efail(W2B_EINVAL, who + ": normalize must be 0 or 1");
  const int64_t bad = bad_vector_value(x, dim);
  if (bad >= 0) return efail(W2B_EINVAL, who + ": column " + std::to_string(bad) + ": " + kVectorRange);
  const int64_t nb = (dim + 63) / 64, wpr = nb * bitlevel;
  const float wx = vector_weight(x, dim, normalize);
  const std::vector<float> wt = bitlevel == 2 ? codes_weights(dim) : std::vector<float>();
  const float wbits = (float)(1.0 / sqrt((double)dim));
  for (int64_t c = 0; c < words; c++) {
    const uint64_t *rc = packed + c * wpr;
    float acc = 0.f;
    int64_t n3 = 0;
    for (int64_t a = 0; a < dim; a++) {
      const uint64_t bit = 1ull << (a & 63);
      float t = 1.f;
      if (bitlevel == 2 && (rc[2 * (a >> 6) + 1] & bit)) t = 3.f, n3++;
      if (rc[bitlevel * (a >> 6)] & bit) t = -t;
      acc = fmaf(x[a], t, acc);
    }
    if (S_out) S_out[c] = acc;
    if (!score_out) continue;
    const float ps = acc * wx;
    score_out[c] = ps * (bitlevel == 2 ? wt[(size_t)n3] : wbits);
  }
  return W2B_OK;
}

// Host twin of the document kernels: every (query position, document position) pair from the packed rows themselves, the
// maxima and the sums in 64-bit integers, the float steps of the header one at a time (this file is built with
// -ffp-contract=off, and the function says so again).
extern "C" int w2b_docs_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, int64_t n_ids,
                                    const int32_t *ids, int64_t n_docs, const int64_t *offsets, int64_t n_q,
                                    const int32_t *qids, int32_t symmetric, int64_t *dir_out, float *score_out) {
#pragma clang fp contract(off)
  const std::string who = "w2b_docs_scores_host";
  if (symmetric != 0 && symmetric != 1) return efail(W2B_EINVAL, who + ": symmetric must be 0 or 1");
  if (n_q < 0 || (n_q > 0 && !qids)) return efail(W2B_EINVAL, who + ": bad argument");
  if (n_q > W2B_EVAL_MAX_DOC) return efail(W2B_EINVAL, who + ": a query holds at most 1024 positions");
  if (n_docs > kDocsMaxDocs) return efail(W2B_EINVAL, who + ": at most 0x7FFFFF00 documents");
  const std::string why = bad_texts(n_ids, ids, n_docs, offsets, "document");
  if (!why.empty()) return efail(W2B_EINVAL, who + ": " + why);
  if (!packed || words < 0 || dim < 1) return efail(W2B_EINVAL, who + ": bad argument");
  if (bitlevel != 1 && bitlevel != 2) return efail(W2B_EINVAL, who + ": bitlevel must be 1 or 2");
  if (dim >= kDocsMaxSize) return efail(W2B_EINVAL, who + ": " + kDocsSize);
  if (bad_text_ids(n_ids, ids, words)) return efail(W2B_EINVAL, who + ": document id out of range");
  if (bad_text_ids(n_q, qids, words)) return efail(W2B_EINVAL, who + ": query id out of range");
  const int64_t nb = (dim + 63) / 64, wpr = nb * bitlevel;
  auto valid = [&](int64_t b) { return (b + 1) * 64 <= dim ? ~0ull : (1ull << (dim - b * 64)) - 1; };   // padding bits do not count
  const std::vector<float> wt = bitlevel == 2 ? codes_weights(dim) : std::vector<float>();
  auto weight = [&](const uint64_t *r) {
    int64_t n3 = 0;
    for (int64_t b = 0; b < nb; b++) n3 += __builtin_popcountll(r[2 * b + 1] & valid(b));
    return wt[(size_t)n3];
  };
  // I(x, c), or F(x, c) = (int64) ldexp(cos(x, c), 50)
  auto pair = [&](const uint64_t *x, float wx, const uint64_t *c, float wc) -> int64_t {
    if (bitlevel == 1) {
      int64_t h = 0;
      for (int64_t b = 0; b < nb; b++) h += __builtin_popcountll((x[b] ^ c[b]) & valid(b));
      return dim - 2 * h;
    }
    int64_t j = 0;
    for (int64_t b = 0; b < nb; b++) {
      const uint64_t v = valid(b), neg = (x[2 * b] ^ c[2 * b]) & v, pos = ~neg & v;
      const uint64_t mx = x[2 * b + 1], mc = c[2 * b + 1];
      auto mag = [&](uint64_t m) {
        return (int64_t)__builtin_popcountll(m) + 2 * __builtin_popcountll(m & mx) + 2 * __builtin_popcountll(m & mc) +
               4 * __builtin_popcountll(m & mx & mc);
      };
      j += mag(pos) - mag(neg);
    }
    const float pj = (float)(int32_t)j * wx;
    const float cs = pj * wc;
    return (int64_t)ldexpf(cs, 50);
  };
  std::vector<const uint64_t *> qr;
  std::vector<float> qw;
  for (int64_t i = 0; i < n_q; i++)
    if (qids[i] >= 0) {
      qr.push_back(packed + (int64_t)qids[i] * wpr);
      qw.push_back(bitlevel == 2 ? weight(qr.back()) : 0.f);
    }
  const int64_t mq = (int64_t)qr.size();
  std::vector<int64_t> best_x((size_t)mq);
  for (int64_t d = 0; d < n_docs; d++) {
    int64_t md = 0, r_qd = 0, r_dq = 0;
    for (int64_t i = offsets[d]; i < offsets[d + 1]; i++) {
      if (ids[i] < 0 || mq == 0) continue;
      const uint64_t *c = packed + (int64_t)ids[i] * wpr;
      const float wc = bitlevel == 2 ? weight(c) : 0.f;
      int64_t best_c = 0;
      for (int64_t x = 0; x < mq; x++) {
        const int64_t v = pair(qr[(size_t)x], qw[(size_t)x], c, wc);
        if (md == 0 || v > best_x[(size_t)x]) best_x[(size_t)x] = v;
        if (x == 0 || v > best_c) best_c = v;
      }
      r_dq += best_c;
      md++;
    }
    if (md > 0)
      for (int64_t x = 0; x < mq; x++) r_qd += best_x[(size_t)x];
    if (dir_out) {
      dir_out[d] = r_qd;
      dir_out[n_docs + d] = r_dq;
    }
    if (!score_out) continue;
    float sc = 0.f;
    if (mq > 0 && md > 0) {
      sc = docs_score(bitlevel, r_qd, mq, dim);
      if (symmetric) {
        const float s2 = docs_score(bitlevel, r_dq, md, dim);
        sc = s2 < sc ? s2 : sc;
      }
    }
    score_out[d] = sc;
  }
  return W2B_OK;
}

// Host twin of the pair kernels: both pooled vectors from the unpacked rows, the three sums in 64-bit integers, the double
// steps of the header one at a time (this file is built with -ffp-contract=off, and pair_score says so again).
extern "C" int w2b_pairs_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, int64_t n_ids,
                              const int32_t *ids, int64_t np, const int64_t *offsets, float *score, int64_t *parts) {
  const std::string who = "w2b_pairs_host";
  const std::string why = bad_pairs(n_ids, ids, np, offsets, score, parts);
  if (!why.empty()) return efail(W2B_EINVAL, who + ": " + why);
  if (!packed || words < 0 || dim < 1) return efail(W2B_EINVAL, who + ": bad argument");
  if (bitlevel != 1 && bitlevel != 2) return efail(W2B_EINVAL, who + ": bitlevel must be 1 or 2");
  if (dim > kPairsMaxSize) return efail(W2B_EINVAL, who + ": size must be at most 2^24");
  const int64_t bad = bad_pair_id(ids, np, offsets, words);
  if (bad >= 0) return efail(W2B_EINVAL, who + ": pair " + std::to_string(bad) + ": id out of range");
  const int64_t nb = (dim + 63) / 64, wpr = nb * bitlevel;
  auto t_of = [&](const uint64_t *r, int64_t a) -> int32_t {
    const uint64_t bit = 1ull << (a & 63);
    if (bitlevel == 1) return (r[a >> 6] & bit) ? -1 : 1;
    return ((r[2 * (a >> 6) + 1] & bit) ? 3 : 1) * ((r[2 * (a >> 6)] & bit) ? -1 : 1);
  };
  std::vector<int32_t> T[2] = {std::vector<int32_t>((size_t)dim), std::vector<int32_t>((size_t)dim)};
  for (int64_t p = 0; p < np; p++) {
    for (int side = 0; side < 2; side++) {
      std::fill(T[side].begin(), T[side].end(), 0);
      for (int64_t i = offsets[2 * p + side]; i < offsets[2 * p + side + 1]; i++)
        if (ids[i] >= 0)
          for (int64_t a = 0; a < dim; a++) T[side][(size_t)a] += t_of(packed + (int64_t)ids[i] * wpr, a);
    }
    int64_t j = 0, na = 0, nbb = 0;
    for (int64_t a = 0; a < dim; a++) {
      const int64_t x = T[0][(size_t)a], y = T[1][(size_t)a];
      j += x * y;
      na += x * x;
      nbb += y * y;
    }
    if (score) score[p] = pair_score(j, na, nbb);
    if (parts) parts[3 * p] = j, parts[3 * p + 1] = na, parts[3 * p + 2] = nbb;
  }
  return W2B_OK;
}

namespace {
// Pearson's r of the header; NaN with n < 2 or a zero variance
double pearson_r(const std::vector<double> &x, const std::vector<double> &y) {
#pragma clang fp contract(off)
  const size_t n = x.size();
  if (n < 2) return NAN;
  if (*std::min_element(x.begin(), x.end()) == *std::max_element(x.begin(), x.end()) ||
      *std::min_element(y.begin(), y.end()) == *std::max_element(y.begin(), y.end()))
    return NAN;                                    // (a constant: its deviations from a rounded mean need not be zero)
  double mx = 0, my = 0;
  for (size_t i = 0; i < n; i++) mx += x[i], my += y[i];
  mx /= (double)n;
  my /= (double)n;
  double sxy = 0, sxx = 0, syy = 0;
  for (size_t i = 0; i < n; i++) {
    const double dx = x[i] - mx, dy = y[i] - my;
    sxy += dx * dy;
    sxx += dx * dx;
    syy += dy * dy;
  }
  if (!(sxx > 0) || !(syy > 0)) return NAN;
  return sxy / sqrt(sxx * syy);
}
// 1-based ranks, equal values sharing the mean of their ranks
std::vector<double> mean_ranks(const std::vector<double> &v) {
  const size_t n = v.size();
  std::vector<size_t> idx(n);
  for (size_t i = 0; i < n; i++) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return v[a] < v[b]; });
  std::vector<double> r(n);
  for (size_t i = 0; i < n;) {
    size_t k = i;
    while (k < n && v[idx[k]] == v[idx[i]]) k++;
    const double mean = 0.5 * (double)(i + 1 + k);           // ranks i + 1 .. k
    for (size_t t = i; t < k; t++) r[idx[t]] = mean;
    i = k;
  }
  return r;
}
}  // namespace

extern "C" int w2b_rank_correlation(int64_t n, const double *x, const double *y, double *pearson, double *spearman) {
  if (n < 0 || (n > 0 && (!x || !y))) return efail(W2B_EINVAL, "w2b_rank_correlation: bad argument");
  const std::vector<double> xv(x, x + n), yv(y, y + n);
  bool nan = false;
  for (int64_t i = 0; i < n; i++) nan |= std::isnan(xv[(size_t)i]) || std::isnan(yv[(size_t)i]);
  if (pearson) *pearson = nan ? NAN : pearson_r(xv, yv);
  if (spearman) *spearman = nan ? NAN : pearson_r(mean_ranks(xv), mean_ranks(yv));
  return W2B_OK;
}

// Host twin of the class kernels: the loop of the header, one step at a time (this file is built with -ffp-contract=off, and
// the function says so again).
extern "C" int w2b_classes_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, int32_t n_classes,
                                int32_t max_iters, const int32_t *init, int32_t *cls, float *score, int32_t *T_out,
                                int64_t *counts, int32_t *iters_run, int64_t *moved) {
#pragma clang fp contract(off)
  const std::string who = "w2b_classes_host";
  if (const char *why = bad_classes_args(n_classes, max_iters)) return efail(W2B_EINVAL, who + ": " + why);
  if (!packed || !cls || words < 0 || dim < 1) return efail(W2B_EINVAL, who + ": bad argument");
  if (bitlevel != 1 && bitlevel != 2) return efail(W2B_EINVAL, who + ": bitlevel must be 1 or 2");
  if (const char *why = bad_classes_shape(words, dim, n_classes)) return efail(W2B_EINVAL, who + ": " + why);
  const int64_t bad = bad_classes_init(init, words, n_classes);
  if (bad >= 0) return efail(W2B_EINVAL, who + ": " + classes_init_error(bad));
  const int32_t K = n_classes;
  const int64_t wpr = (dim + 63) / 64 * bitlevel;
  std::vector<int8_t> t((size_t)(words * dim));
  for (int64_t c = 0; c < words; c++) {
    const uint64_t *rc = packed + c * wpr;
    for (int64_t a = 0; a < dim; a++) {
      const uint64_t bit = 1ull << (a & 63);
      int8_t v = 1;
      if (bitlevel == 2 && (rc[2 * (a >> 6) + 1] & bit)) v = 3;
      if (rc[bitlevel * (a >> 6)] & bit) v = (int8_t)-v;
      t[(size_t)(c * dim + a)] = v;
    }
  }
  std::vector<int32_t> cl((size_t)words), nw((size_t)words), T((size_t)K * (size_t)dim);
  std::vector<float> sc((size_t)words, 0.f), Tf((size_t)K * (size_t)dim), wq((size_t)K), acc((size_t)K);
  std::vector<int64_t> cnt((size_t)K);
  std::vector<char> live((size_t)K);
  for (int64_t c = 0; c < words; c++) cl[(size_t)c] = init ? init[c] : (int32_t)(c % K);
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
  const bool fma = __builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2");
#endif
  int32_t it = 0;
  int64_t mv = 0;
  while (it < max_iters) {
    classes_sums_host(t.data(), words, dim, K, cl.data(), T.data(), cnt.data());
    for (int32_t k = 0; k < K; k++) {
      long long n = 0;
      for (int64_t a = 0; a < dim; a++) {
        const long long v = T[(size_t)(k * dim + a)];
        n += v * v;
        Tf[(size_t)(a * K + k)] = (float)v;
      }
      live[(size_t)k] = n > 0;
      wq[(size_t)k] = n > 0 ? classes_weight(n) : 0.f;
    }
    mv = 0;
    for (int64_t c = 0; c < words; c++) {
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
      if (fma) classes_chains_fma(Tf.data(), t.data() + c * dim, dim, K, acc.data());
      else
#endif
        classes_chains_plain(Tf.data(), t.data() + c * dim, dim, K, acc.data());
      int32_t bk = -1;
      float bd = 0.f;
      for (int32_t k = 0; k < K; k++) {
        if (!live[(size_t)k]) continue;
        const float d = acc[(size_t)k] * wq[(size_t)k];
        if (bk < 0 || d > bd) bk = k, bd = d;
      }
      if (bk < 0) bk = 0, bd = 0.f;
      nw[(size_t)c] = bk;
      sc[(size_t)c] = bd;
      mv += bk != cl[(size_t)c];
    }
    cl.swap(nw);
    it++;
    if (mv == 0) break;
  }
  classes_sums_host(t.data(), words, dim, K, cl.data(), T.data(), cnt.data());
  std::copy(cl.begin(), cl.end(), cls);
  if (score) std::copy(sc.begin(), sc.end(), score);
  if (T_out) std::copy(T.begin(), T.end(), T_out);
  if (counts) std::copy(cnt.begin(), cnt.end(), counts);
  if (iters_run) *iters_run = it;
  if (moved) *moved = mv;
  return W2B_OK;
}
