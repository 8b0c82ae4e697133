// w2b_embed_shared.h -- what the entry points of the packed embedding (w2b_embed.cpp) and their host twins
// (w2b_embed_twins.cpp) must refuse identically, written once: every validator that needs no handle -- the table's shape, ids,
// bags, weights, dtype, mode and flags, and the checks of w2b_embed_project, w2b_embed_backproject, w2b_embed_xent and
// w2b_embed_topk -- with its message, in the order include/word2bits_embed.h states; and the arithmetic of the cross-entropy
// and the key order of the top-k selection, which the kernels compile as well.  No device header, no handle.  Every
// definition has internal linkage, so the library exports none of them.
#pragma once
#include "../../include/word2bits_embed.h"
#include "../../include/word2bits_hip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

int w2b_internal_fail(int code, const char *msg);   // sets w2b_last_error() (w2b_trainer.cpp)

// ---- the arithmetic of the softmax cross-entropy (include/word2bits_embed.h, "Cross-entropy"), written ONCE: the host twin
// (w2b_embed_twins.cpp) and the kernels (w2b_kernels_embedxent.hip) compile this text.  Every operation is one float32
// operation rounded on its own: explicit fmaf, and products / differences / the quotient through W2B_XF* (on the device the
// *_rn intrinsics, which the compiler never fuses; on the host the plain operator in a unit built with -ffp-contract=off).
// (A kernel file defines W2B_EMBED_SHARED_DEVICE before it includes this header; every other unit sees host functions.)
#if defined(W2B_EMBED_SHARED_DEVICE)
#define W2B_XHD __host__ __device__ inline
#else
#define W2B_XHD inline
#endif
#if defined(W2B_EMBED_SHARED_DEVICE) && defined(__HIP_DEVICE_COMPILE__)
#define W2B_XFMUL(a, b) __fmul_rn((a), (b))
#define W2B_XFSUB(a, b) __fsub_rn((a), (b))
#define W2B_XFDIV(a, b) __fdiv_rn((a), (b))
#else
#define W2B_XFMUL(a, b) ((a) * (b))
#define W2B_XFSUB(a, b) ((a) - (b))
#define W2B_XFDIV(a, b) ((a) / (b))
#endif

#define W2B_XENT_LOG2E 0x3FB8AA3Bu    /* log2(e) rounded to float32 */
#define W2B_XENT_LN2_HI 0x3F317200u   /* 0.693145751953125: the leading 15 bits of ln 2, k * LN2_HI is exact for |k| < 2^9 */
#define W2B_XENT_LN2_LO 0x35BFBE8Eu   /* ln 2 - LN2_HI rounded to float32 */
#define W2B_XENT_C2 0x3F000000u       /* 1/2!  */
#define W2B_XENT_C3 0x3E2AAAABu       /* 1/3!  */
#define W2B_XENT_C4 0x3D2AAAABu       /* 1/4!  */
#define W2B_XENT_C5 0x3C088889u       /* 1/5!  */
#define W2B_XENT_C6 0x3AB60B61u       /* 1/6!  */
#define W2B_XENT_C7 0x39500D01u       /* 1/7!  */

namespace {
W2B_XHD float w2b_xent_bits(uint32_t b) {
  return __builtin_bit_cast(float, b);
}

// expneg(r) for r <= 0: +0.0 exactly unless r >= -64 (so for NaN too), else exp(r) by the steps of the header; every result
// is then p * 2^k with 0.70 < p < 1.42 and -92 <= k <= 0: a normal number >= 2^-93, and expneg(0) == 1.
W2B_XHD float w2b_expneg(float r) {
  if (!(r >= -64.0f)) return 0.0f;
  const float k = rintf(W2B_XFMUL(r, w2b_xent_bits(W2B_XENT_LOG2E)));                // to nearest, ties to even
  float f = fmaf(k, -w2b_xent_bits(W2B_XENT_LN2_HI), r);
  f = fmaf(k, -w2b_xent_bits(W2B_XENT_LN2_LO), f);
  float p = w2b_xent_bits(W2B_XENT_C7);
  p = fmaf(p, f, w2b_xent_bits(W2B_XENT_C6));
  p = fmaf(p, f, w2b_xent_bits(W2B_XENT_C5));
  p = fmaf(p, f, w2b_xent_bits(W2B_XENT_C4));
  p = fmaf(p, f, w2b_xent_bits(W2B_XENT_C3));
  p = fmaf(p, f, w2b_xent_bits(W2B_XENT_C2));
  p = fmaf(p, f, 1.0f);
  p = fmaf(p, f, 1.0f);
  return W2B_XFMUL(p, w2b_xent_bits((uint32_t)((int)k + 127) << 23));                // 2^k from integer bits: exact
}

// one term of U_s: (uint64) rint(expneg(l - M) * 2^32), an integer in [0, 2^32]
W2B_XHD uint64_t w2b_xent_term(float l, float M) {
  const float t = W2B_XFMUL(w2b_expneg(W2B_XFSUB(l, M)), 4294967296.0f);               // exact: 0 or >= 2^-61
  return (uint64_t)rintf(t);
}

// (float)u, u < 2^63, rounded to nearest even, from integer operations alone
W2B_XHD float w2b_xent_u64_to_f32(uint64_t u) {
  if (u == 0) return 0.0f;
  const int lz = __builtin_clzll((unsigned long long)u);
  const uint64_t nrm = u << lz;                                                      // the leading one at bit 63
  uint32_t mant = (uint32_t)(nrm >> 40);                                             // 24 bits
  const uint64_t rest = nrm & ((1ull << 40) - 1), half = 1ull << 39;
  if (rest > half || (rest == half && (mant & 1u))) mant++;
  int ex = 63 - lz;
  if (mant == (1u << 24)) mant >>= 1, ex++;
  return w2b_xent_bits(((uint32_t)(ex + 127) << 23) | (mant & 0x7FFFFFu));
}

// one step of se: se = fmaf((float)U * 2^-32, expneg(M - mx), se)
W2B_XHD float w2b_xent_se_step(uint64_t U, float M, float mx, float se) {
  const float u = W2B_XFMUL(w2b_xent_u64_to_f32(U), 2.3283064365386962890625e-10f);  // * 2^-32: exact
  return fmaf(u, w2b_expneg(W2B_XFSUB(M, mx)), se);
}

// g of a live position of a vector that is not ignored
W2B_XHD float w2b_xent_g(float l, float mx, float se, bool is_target) {
  const float g = W2B_XFDIV(w2b_expneg(W2B_XFSUB(l, mx)), se);
  return is_target ? W2B_XFSUB(g, 1.0f) : g;
}

// ---- the order of the top-k selection (include/word2bits_embed.h, "Top-k"), written ONCE for the host twin and the kernels
// (w2b_kernels_embedtopk.hip).  The order-preserving integer map of float32 bits: all bits of a negative pattern flipped, the
// sign bit of a non-negative one set; unsigned comparison of the images is the comparison of the floats (-0.0 just below
// +0.0, NaNs where their bits put them).
#define W2B_TOPK_UNIT 64              /* candidate positions whose keys one slot of the selection scratch collects */
W2B_XHD uint32_t w2b_topk_map(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
W2B_XHD uint32_t w2b_topk_unmap(uint32_t image) { return (image & 0x80000000u) ? (image & 0x7FFFFFFFu) : ~image; }
// the key of a live logit at candidate position j: larger = better; equal logits rank in ascending position.  Never 0.
W2B_XHD uint64_t w2b_topk_key(uint32_t bits, uint32_t j) { return ((uint64_t)w2b_topk_map(bits) << 32) | (uint32_t)~j; }
}  // namespace

namespace {
constexpr int64_t kProjectMaxVectors = 1ll << 24;   // vectors of one call (their operand staging is indexed with 32 bits)

// "<who>: <what>" becomes w2b_last_error()
inline int refuse(int code, const char *who, const std::string &what) {
  return w2b_internal_fail(code, (std::string(who) + ": " + what).c_str());
}

// ---- arguments that every entry point refuses with the same words
inline int elem_size(int32_t dtype) { return dtype == W2B_EMBED_F32 ? 4 : (dtype == W2B_EMBED_BF16 || dtype == W2B_EMBED_F16) ? 2 : 0; }

inline int check_dtype(const char *who, int32_t dtype) {
  return elem_size(dtype) ? W2B_OK : refuse(W2B_EINVAL, who, "dtype is none of W2B_EMBED_F32 / BF16 / F16");
}

inline int check_mode(const char *who, int32_t mode) {
  if (mode != W2B_EMBED_SUM && mode != W2B_EMBED_MEAN) return refuse(W2B_EINVAL, who, "mode is neither W2B_EMBED_SUM nor W2B_EMBED_MEAN");
  return W2B_OK;
}

// a flag of the device form (use_cand, want_dx)
inline int check_flag(const char *who, const char *name, int32_t value) {
  return value == 0 || value == 1 ? W2B_OK : refuse(W2B_EINVAL, who, std::string(name) + " must be 0 or 1");
}

// a float the host forms and the twins accept: finite, and 0 or within 2^-60 .. 2^60 (no subnormal and no overflow anywhere
// downstream; the rule of w2b_eval_vectors)
inline bool value_in_range(float v) {
  const uint32_t a = __builtin_bit_cast(uint32_t, v) & 0x7FFFFFFFu;
  return a == 0u || (a >= 0x21800000u && a <= 0x5D800000u);
}

// ---- the table, ids, bags and weights (lookup and bags)
// the shape of a table: a handle needs a row (min_rows = 1), a twin takes an empty table (0)
inline int check_shape(const char *who, int64_t rows, int64_t dim, int32_t bitlevel, int64_t min_rows) {
  if (rows < min_rows || rows > 0x7FFFFF00ll || dim < 1 || dim > (1 << 24)) return refuse(W2B_EINVAL, who, "unsupported rows / dim");
  if (bitlevel != 1 && bitlevel != 2) return refuse(W2B_EUNSUPPORTED, who, "bitlevel must be 1 or 2");
  return W2B_OK;
}

// the table a twin is handed
inline int check_table(const char *who, const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel) {
  if (!packed) return refuse(W2B_EINVAL, who, "null table");
  return check_shape(who, rows, dim, bitlevel, 0);
}

inline int check_ids(const char *who, int64_t rows, int64_t n, const int32_t *ids) {
  if (n < 0) return refuse(W2B_EINVAL, who, "negative id count");
  if (n > 0 && !ids) return refuse(W2B_EINVAL, who, "null ids");
  for (int64_t i = 0; i < n; i++)
    if (ids[i] >= rows) {
      char msg[160];
      snprintf(msg, sizeof msg, "%s: ids[%lld] = %d is not below rows = %lld", who, (long long)i, (int)ids[i], (long long)rows);
      return w2b_internal_fail(W2B_EINVAL, msg);
    }
  return W2B_OK;
}

inline int check_bags(const char *who, int64_t n_ids, int64_t n_bags, const int64_t *offsets, int32_t mode) {
  if (n_bags < 0 || n_bags > 0x7FFFFF00ll) return refuse(W2B_EINVAL, who, "bad bag count");
  if (int rc = check_mode(who, mode)) return rc;
  if (!offsets) return n_bags == 0 && n_ids == 0 ? W2B_OK : refuse(W2B_EINVAL, who, "null offsets");
  if (offsets[0] != 0) return refuse(W2B_EINVAL, who, "offsets[0] is not 0");
  for (int64_t b = 0; b < n_bags; b++) {
    if (offsets[b + 1] < offsets[b]) return refuse(W2B_EINVAL, who, "offsets decrease at bag " + std::to_string(b));
    if (offsets[b + 1] - offsets[b] > W2B_EMBED_MAX_BAG)
      return refuse(W2B_EINVAL, who, "bag " + std::to_string(b) + " is longer than W2B_EMBED_MAX_BAG");
  }
  if (offsets[n_bags] != n_ids) return refuse(W2B_EINVAL, who, "offsets[n_bags] is not n_ids");
  return W2B_OK;
}

// the first weight on an id >= 0 that is not finite, or neither 0 nor within 2^-60 .. 2^60
inline int check_weights(const char *who, int64_t n, const int32_t *ids, const float *weights) {
  if (n > 0 && !weights) return refuse(W2B_EINVAL, who, "null weights");
  for (int64_t i = 0; i < n; i++)
    if (ids[i] >= 0 && !value_in_range(weights[i])) {
      char msg[200];
      snprintf(msg, sizeof msg, "%s: weights[%lld] = %g is not finite, or neither 0 nor within 2^-60 .. 2^60", who, (long long)i,
               (double)weights[i]);
      return w2b_internal_fail(W2B_EINVAL, msg);
    }
  return W2B_OK;
}

// ---- the projection (w2b_embed_project*)
// the checks that need no handle and no table: counts, dtype, NULL pointers with non-zero counts
inline int project_check_args(const char *who, int64_t n, const float *x, int64_t m, int32_t dtype, const void *out) {
  if (n < 0 || n > kProjectMaxVectors) return refuse(W2B_EINVAL, who, "bad vector count");
  if (m < 0 || m > 0x7FFFFF00ll) return refuse(W2B_EINVAL, who, "bad candidate count");
  if (int rc = check_dtype(who, dtype)) return rc;
  if (n > 0 && !x) return refuse(W2B_EINVAL, who, "null vectors");
  if (n > 0 && m > 0 && !out) return refuse(W2B_EINVAL, who, "null output");
  return W2B_OK;
}

// candidates: NULL means every row, and m must then be rows; an id >= rows is refused, an id < 0 is padding
inline int project_check_cand(const char *who, int64_t rows, int64_t m, const int32_t *cand) {
  char msg[200];
  if (!cand) {
    if (m == rows) return W2B_OK;
    snprintf(msg, sizeof msg, "%s: without candidates m = %lld must be rows = %lld", who, (long long)m, (long long)rows);
    return w2b_internal_fail(W2B_EINVAL, msg);
  }
  for (int64_t j = 0; j < m; j++)
    if (cand[j] >= rows) {
      snprintf(msg, sizeof msg, "%s: cand[%lld] = %d is not below rows = %lld", who, (long long)j, (int)cand[j], (long long)rows);
      return w2b_internal_fail(W2B_EINVAL, msg);
    }
  return W2B_OK;
}

// the first value that is not finite, or neither 0 nor within 2^-60 .. 2^60
inline int project_check_values(const char *who, int64_t n, int64_t dim, const float *x) {
  for (int64_t i = 0; i < n * dim; i++) {
    if (!value_in_range(x[i])) {
      char msg[200];
      snprintf(msg, sizeof msg, "%s: vector %lld, column %lld: %g is not finite, or neither 0 nor within 2^-60 .. 2^60", who,
               (long long)(i / dim), (long long)(i % dim), (double)x[i]);
      return w2b_internal_fail(W2B_EINVAL, msg);
    }
  }
  return W2B_OK;
}

// ---- the back-projection (w2b_embed_backproject*): its checks that need no handle and no table
inline int backproject_check_args(const char *who, int64_t n, const float *g, int64_t m, const void *dx) {
  if (n < 0 || n > kProjectMaxVectors) return refuse(W2B_EINVAL, who, "bad vector count");
  if (m < 0 || m > 0x7FFFFF00ll) return refuse(W2B_EINVAL, who, "bad candidate count");
  if (n > 0 && m > 0 && !g) return refuse(W2B_EINVAL, who, "null g");
  if (n > 0 && !dx) return refuse(W2B_EINVAL, who, "null output");
  return W2B_OK;
}

// the first g on a candidate >= 0 (every position when cand is NULL) that is not finite, or neither 0 nor within 2^-60 .. 2^60
inline int backproject_check_values(const char *who, int64_t n, int64_t m, const int32_t *cand, const float *g) {
  for (int64_t i = 0; i < n; i++)
    for (int64_t j = 0; j < m; j++) {
      if (cand && cand[j] < 0) continue;
      if (!value_in_range(g[i * m + j])) {
        char msg[200];
        snprintf(msg, sizeof msg, "%s: vector %lld, candidate %lld: %g is not finite, or neither 0 nor within 2^-60 .. 2^60", who,
                 (long long)i, (long long)j, (double)g[i * m + j]);
        return w2b_internal_fail(W2B_EINVAL, msg);
      }
    }
  return W2B_OK;
}

// ---- the cross-entropy (w2b_embed_xent*): its checks that need no handle and no table (dx may be NULL: no gradient)
inline int xent_check_args(const char *who, int64_t n, const float *x, int64_t m, const int32_t *target, const float *mx,
                           const float *se, const float *tl) {
  if (n < 0 || n > kProjectMaxVectors) return refuse(W2B_EINVAL, who, "bad vector count");
  if (m < 0 || m > 0x7FFFFF00ll) return refuse(W2B_EINVAL, who, "bad candidate count");
  if (n > 0 && !x) return refuse(W2B_EINVAL, who, "null vectors");
  if (n > 0 && !target) return refuse(W2B_EINVAL, who, "null targets");
  if (n > 0 && (!mx || !se || !tl)) return refuse(W2B_EINVAL, who, "null output");
  return W2B_OK;
}

// ---- the top-k selection (w2b_embed_topk*): its checks that need no handle and no table
inline int topk_check_k(const char *who, int64_t k) {
  if (k >= 1 && k <= W2B_EMBED_MAX_K) return W2B_OK;
  char msg[160];
  snprintf(msg, sizeof msg, "%s: k = %lld is not within 1 .. W2B_EMBED_MAX_K = %d", who, (long long)k, W2B_EMBED_MAX_K);
  return w2b_internal_fail(W2B_EINVAL, msg);
}

inline int topk_check_args(const char *who, int64_t n, const float *x, int64_t m, int64_t k, const float *vals, const int32_t *pos) {
  if (n < 0 || n > kProjectMaxVectors) return refuse(W2B_EINVAL, who, "bad vector count");
  if (m < 0 || m > 0x7FFFFF00ll) return refuse(W2B_EINVAL, who, "bad candidate count");
  if (int rc = topk_check_k(who, k)) return rc;
  if (n > 0 && !x) return refuse(W2B_EINVAL, who, "null vectors");
  if (n > 0 && (!vals || !pos)) return refuse(W2B_EINVAL, who, "null output");
  return W2B_OK;
}

// the first target that is >= m or points at a padding position (a target < 0 means the vector is ignored)
inline int xent_check_targets(const char *who, int64_t n, int64_t m, const int32_t *cand, const int32_t *target) {
  char msg[200];
  for (int64_t i = 0; i < n; i++) {
    if (target[i] < 0) continue;
    if (target[i] >= m) {
      snprintf(msg, sizeof msg, "%s: vector %lld: target %d is not below m = %lld", who, (long long)i, (int)target[i], (long long)m);
      return w2b_internal_fail(W2B_EINVAL, msg);
    }
    if (cand && cand[target[i]] < 0) {
      snprintf(msg, sizeof msg, "%s: vector %lld: target %d is a padding position", who, (long long)i, (int)target[i]);
      return w2b_internal_fail(W2B_EINVAL, msg);
    }
  }
  return W2B_OK;
}
}  // namespace
