// w2b_eval_shared.h -- what the three host units of the evaluator (w2b_eval.cpp: the device side; w2b_eval_twins.cpp: the
// tests' host twins; w2b_eval_text.cpp: the text forms) must compute or refuse identically, written once: the validators
// with their messages, the weight and score expressions of include/word2bits_eval.h, the limits and the messages that more
// than one of them quotes.  Host arithmetic only: no device header, no handle.  Every definition has internal linkage, so
// the library exports none of them.  A function whose float sequence matters says `fp contract(off)` itself; the others
// hold no multiply next to an add, and every unit that includes this file is built with -ffp-contract=off as well.
#pragma once
#include "../../include/word2bits_eval.h"
#include "../../include/word2bits_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

int w2b_internal_fail(int code, const char *msg);   // sets w2b_last_error() (w2b_trainer.cpp)

namespace {
inline int efail(int code, const std::string &msg) { return w2b_internal_fail(code, msg.c_str()); }

// the C locale's isspace and toupper: the reader upper-cases the vocabulary with what the text forms upper-case a question with
inline bool is_space(unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }
inline char c_upper(char c) { return (c >= 'a' && c <= 'z') ? (char)(c - 32) : c; }

// ------------------------------------------------------------------------------------ codes mode
// w(r) by n3 (include/word2bits_eval.h, "codes mode"): (float)(1.0 / sqrt((double)(dim + 8 n3))), n3 = 0..dim
inline std::vector<float> codes_weights(int64_t dim) {
  std::vector<float> w((size_t)dim + 1);
  for (int64_t n3 = 0; n3 <= dim; n3++) w[(size_t)n3] = (float)(1.0 / sqrt((double)(dim + 8 * n3)));
  return w;
}

// ------------------------------------------------------------------------------------ signed multi-word questions
// what w2b_eval_combine and its host twin refuse in one question's slots (null: nothing)
inline const char *bad_terms(int32_t nt, const int32_t *rows, const int8_t *signs, int64_t words) {
  int used = 0;
  for (int32_t t = 0; t < nt; t++) {
    if (signs[t] < -1 || signs[t] > 1) return "a sign must be -1, 0 or +1";
    if (signs[t] == 0) continue;
    if (rows[t] < 0 || rows[t] >= words) return "question row out of range";
    used++;
  }
  return used ? nullptr : "a question needs at least one slot with a sign";
}

// ------------------------------------------------------------------------------------ 3CosMul
constexpr int64_t kCosmulMaxBits = 1ll << 24;   // the largest 1-bit size whose agreement counts are exact in float32
constexpr float kCosmulEps = 1e-6f;             // 0x358637BD

// u by agreement count on 1-bit rows: (float)A / (float)dim, one correctly rounded division, A = 0..dim
inline std::vector<float> cosmul_utab(int64_t dim) {
  std::vector<float> u((size_t)dim + 1);
  for (int64_t a = 0; a <= dim; a++) u[(size_t)a] = (float)a / (float)dim;
  return u;
}

// score = (u2 * u3) / (u1 + eps), one rounding per operation
inline float cosmul_score(float u1, float u2, float u3) {
#pragma clang fp contract(off)
  const float num = u2 * u3;
  const float den = u1 + kCosmulEps;
  return num / den;
}

// ------------------------------------------------------------------------------------ bag questions
constexpr int64_t kBagMaxSize = 58254;   // the largest size with 9 * 4096 * size < 2^31

// what w2b_eval_bag and its host twin refuse in one bag (null: nothing)
inline const char *bad_bag(int64_t n, const int32_t *ids, int64_t words) {
  if (n < 0 || n > W2B_EVAL_MAX_BAG) return "a bag holds at most 4096 ids";
  for (int64_t i = 0; i < n; i++)
    if (ids[i] >= words) return "bag id out of range";
  return nullptr;
}

// wq of the header from N_T; a question whose vector is zero weighs nothing
inline float bag_weight(unsigned long long nt) { return nt ? (float)(1.0 / sqrt((double)nt)) : 0.f; }

// ------------------------------------------------------------------------------------ vector questions
// what w2b_eval_vectors and its host twin refuse in one question: the first column whose value is not finite, or neither 0
// nor of a magnitude in 2^-60 .. 2^60 (-1: none)
inline int64_t bad_vector_value(const float *x, int64_t dim) {
  for (int64_t a = 0; a < dim; a++) {
    const float m = fabsf(x[a]);
    if (!(m == 0.f || (m >= 0x1p-60f && m <= 0x1p60f))) return a;       // (NaN fails every comparison)
  }
  return -1;
}
const char *const kVectorRange = "a value must be finite and either 0 or of a magnitude in 2^-60 .. 2^60";

// wx of the header: nx in double, column by column; a question whose vector is zero weighs nothing
inline float vector_weight(const float *x, int64_t dim, int32_t normalize) {
#pragma clang fp contract(off)
  double nx = 0.0;
  for (int64_t a = 0; a < dim; a++) {
    const double sq = (double)x[a] * (double)x[a];
    nx = nx + sq;
  }
  if (nx == 0.0) return 0.f;
  return normalize ? (float)(1.0 / sqrt(nx)) : 1.0f;
}

// ------------------------------------------------------------------------------------ documents
constexpr int64_t kDocsMaxSize = 1ll << 21;      // size below it: 1024 * size < 2^31 and ldexp(cos, 50) is an integer
constexpr int64_t kDocsMaxDocs = 0x7FFFFF00ll;

// what w2b_eval_docs_set, w2b_eval_docs and the host twin refuse in texts given as ids + offsets before they look at a handle
// or a table (empty: nothing); `what` = "document" or "query"
inline std::string bad_texts(int64_t n_ids, const int32_t *ids, int64_t n, const int64_t *offsets, const char *what) {
  if (n < 0 || n_ids < 0 || (n > 0 && !offsets) || (n_ids > 0 && !ids)) return "bad argument";
  if (n == 0 ? n_ids != 0 : (offsets[0] != 0 || offsets[n] != n_ids))
    return std::string(what) + " offsets must start at 0 and end at the number of ids";
  for (int64_t d = 0; d < n; d++) {
    if (offsets[d + 1] < offsets[d] || offsets[d + 1] > n_ids) return std::string(what) + " offsets must not decrease";
    if (offsets[d + 1] - offsets[d] > W2B_EVAL_MAX_DOC) return std::string("a ") + what + " holds at most 1024 positions";
  }
  return std::string();
}
inline bool bad_text_ids(int64_t n_ids, const int32_t *ids, int64_t words) {
  for (int64_t i = 0; i < n_ids; i++)
    if (ids[i] >= words) return true;
  return false;
}
const char *const kDocsSize = "size must be below 2^21 (1024 * size < 2^31)";
const char *const kDocsFp32 = "not available on an fp32 handle: load the file with bits or codes";

// the float steps of the header: one directed score from its integer sum
inline float docs_score(int32_t bitlevel, int64_t sum, int64_t m, int64_t dim) {
#pragma clang fp contract(off)
  if (bitlevel == 1) return (float)(int32_t)sum / (float)(int32_t)(m * dim);
  const float div = (float)m * 0x1p50f;          // exact
  return (float)sum / div;
}

// ------------------------------------------------------------------------------------ pair similarity
constexpr int64_t kPairsMaxSize = 1ll << 24;     // 12288^2 * size < 2^53: J, N_A, N_B are exact as doubles

// what w2b_eval_pairs and its host twin refuse before they look at a handle or a table (empty: nothing)
inline std::string bad_pairs(int64_t n_ids, const int32_t *ids, int64_t np, const int64_t *offsets, const float *score,
                             const int64_t *parts) {
  if (np < 0 || n_ids < 0 || (np > 0 && (!offsets || (!score && !parts))) || (n_ids > 0 && !ids)) return "bad argument";
  if (np > (INT64_MAX >> 2)) return "bad argument";
  if (np == 0 ? n_ids != 0 : (offsets[0] != 0 || offsets[2 * np] != n_ids)) return "offsets must start at 0 and end at n_ids";
  for (int64_t b = 0; b < 2 * np; b++) {
    if (offsets[b + 1] < offsets[b] || offsets[b + 1] > n_ids) return "offsets must not decrease";
    if (offsets[b + 1] - offsets[b] > W2B_EVAL_MAX_BAG) return "a bag holds at most 4096 ids";
  }
  return std::string();
}
// the first pair with an id >= words (-1: none)
inline int64_t bad_pair_id(const int32_t *ids, int64_t np, const int64_t *offsets, int64_t words) {
  for (int64_t p = 0; p < np; p++)
    for (int64_t i = offsets[2 * p]; i < offsets[2 * p + 2]; i++)
      if (ids[i] >= words) return p;
  return -1;
}

// the score of the header from the three integers; an empty pair scores +0
inline float pair_score(int64_t j, int64_t na, int64_t nb) {
#pragma clang fp contract(off)
  if (na == 0 || nb == 0) return 0.f;
  const double nn = (double)na * (double)nb;
  const double root = sqrt(nn);
  return (float)((double)j / root);
}

// ------------------------------------------------------------------------------------ word classes
constexpr int64_t kClassesMaxWords = 5592405;                       // 3 * words < 2^24: (float)T is exact

// what w2b_eval_classes and its host twin refuse: first what needs no table, then the table's shape, then `init`
inline const char *bad_classes_args(int32_t n_classes, int32_t max_iters) {
  if (n_classes < 1) return "n_classes must be at least 1";
  if (max_iters < 0 || max_iters > 1000) return "max_iters must be 0..1000";
  return nullptr;
}
inline const char *bad_classes_shape(int64_t words, int64_t size, int32_t n_classes) {
  if (n_classes > W2B_EVAL_MAX_CLASSES || n_classes > words) return "n_classes must be at most min(words, 16384)";
  if (words > kClassesMaxWords) return "words must be at most 5592405 (3 * words < 2^24)";
  if ((unsigned __int128)9 * (unsigned __int128)words * (unsigned __int128)words * (unsigned __int128)size >=
      ((unsigned __int128)1 << 63))
    return "9 * words^2 * size must stay below 2^63";
  return nullptr;
}
inline int64_t bad_classes_init(const int32_t *init, int64_t words, int32_t n_classes) {
  if (init)
    for (int64_t c = 0; c < words; c++)
      if (init[c] < 0 || init[c] >= n_classes) return c;
  return -1;
}
inline std::string classes_init_error(int64_t row) { return "init: row " + std::to_string(row) + ": class out of range"; }

// wq_k of the header from N_k > 0: the expression of bag_weight
inline float classes_weight(long long n) { return (float)(1.0 / sqrt((double)n)); }

// The chains of one row against every class: Tf = (float)T transposed, [size][K]; t = the row's codes; acc [K].  Explicit
// fmaf, strictly in column order per class.  The body is compiled twice, for a processor with FMA instructions (the
// classes vectorise) and for any other one (a library call per step): the same correctly rounded operation either way.
__attribute__((always_inline)) inline void classes_chains_body(const float *Tf, const int8_t *t, int64_t size, int32_t K,
                                                               float *acc) {
  for (int32_t k = 0; k < K; k++) acc[k] = 0.f;
  for (int64_t a = 0; a < size; a++) {
    const float ta = (float)t[a];
    const float *row = Tf + a * K;
    for (int32_t k = 0; k < K; k++) acc[k] = __builtin_fmaf(row[k], ta, acc[k]);
  }
}
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("avx2,fma"))) inline void classes_chains_fma(const float *Tf, const int8_t *t, int64_t size, int32_t K,
                                                                   float *acc) {
  classes_chains_body(Tf, t, size, K, acc);
}
#endif
inline void classes_chains_plain(const float *Tf, const int8_t *t, int64_t size, int32_t K, float *acc) {
  classes_chains_body(Tf, t, size, K, acc);
}

// T [K][size] and counts [K] of the class array cl
inline void classes_sums_host(const int8_t *t, int64_t words, int64_t size, int32_t K, const int32_t *cl, int32_t *T,
                              int64_t *counts) {
  std::fill(T, T + (size_t)K * (size_t)size, 0);
  std::fill(counts, counts + K, (int64_t)0);
  for (int64_t c = 0; c < words; c++) {
    int32_t *Tk = T + (int64_t)cl[c] * size;
    const int8_t *tc = t + c * size;
    for (int64_t a = 0; a < size; a++) Tk[a] += tc[a];
    counts[cl[c]]++;
  }
}
}  // namespace
