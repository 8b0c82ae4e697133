// w2b_embed_shared.h -- what the host forms of the packed embedding's projection and back-projection (w2b_embed.cpp) and
// their host twins (w2b_embed_twins.cpp) must refuse identically, written once: the validators of w2b_embed_project and
// w2b_embed_backproject with their messages, in the order include/word2bits_embed.h states.  Host arithmetic only: no device header, no handle.  Every definition has
// internal linkage, so the library exports none of them.
#pragma once
#include "../../include/word2bits_embed.h"
#include "../../include/word2bits_hip.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

int w2b_internal_fail(int code, const char *msg);   // sets w2b_last_error() (w2b_trainer.cpp)

namespace {
constexpr int64_t kProjectMaxVectors = 1ll << 24;   // vectors of one call (their operand staging is indexed with 32 bits)

// the checks that need no handle and no table: counts, dtype, NULL pointers with non-zero counts
inline int project_check_args(const char *who, int64_t n, const float *x, int64_t m, bool dtype_ok, const void *out) {
  const std::string w(who);
  if (n < 0 || n > kProjectMaxVectors) return w2b_internal_fail(W2B_EINVAL, (w + ": bad vector count").c_str());
  if (m < 0 || m > 0x7FFFFF00ll) return w2b_internal_fail(W2B_EINVAL, (w + ": bad candidate count").c_str());
  if (!dtype_ok) return w2b_internal_fail(W2B_EINVAL, (w + ": dtype is none of W2B_EMBED_F32 / BF16 / F16").c_str());
  if (n > 0 && !x) return w2b_internal_fail(W2B_EINVAL, (w + ": null vectors").c_str());
  if (n > 0 && m > 0 && !out) return w2b_internal_fail(W2B_EINVAL, (w + ": null output").c_str());
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

// the first value that is not finite, or neither 0 nor within 2^-60 .. 2^60 (the rule of w2b_eval_vectors)
inline int project_check_values(const char *who, int64_t n, int64_t dim, const float *x) {
  for (int64_t i = 0; i < n * dim; i++) {
    uint32_t bits;
    memcpy(&bits, x + i, 4);
    const uint32_t a = bits & 0x7FFFFFFFu;
    if (a != 0u && (a < 0x21800000u || a > 0x5D800000u)) {
      char msg[200];
      snprintf(msg, sizeof msg, "%s: vector %lld, column %lld: %g is not finite, or neither 0 nor within 2^-60 .. 2^60", who,
               (long long)(i / dim), (long long)(i % dim), (double)x[i]);
      return w2b_internal_fail(W2B_EINVAL, msg);
    }
  }
  return W2B_OK;
}

// the back-projection (w2b_embed_backproject*): its checks that need no handle and no table
inline int backproject_check_args(const char *who, int64_t n, const float *g, int64_t m, const void *dx) {
  const std::string w(who);
  if (n < 0 || n > kProjectMaxVectors) return w2b_internal_fail(W2B_EINVAL, (w + ": bad vector count").c_str());
  if (m < 0 || m > 0x7FFFFF00ll) return w2b_internal_fail(W2B_EINVAL, (w + ": bad candidate count").c_str());
  if (n > 0 && m > 0 && !g) return w2b_internal_fail(W2B_EINVAL, (w + ": null g").c_str());
  if (n > 0 && !dx) return w2b_internal_fail(W2B_EINVAL, (w + ": null output").c_str());
  return W2B_OK;
}

// the first g on a candidate >= 0 (every position when cand is NULL) that is not finite, or neither 0 nor within 2^-60 .. 2^60
inline int backproject_check_values(const char *who, int64_t n, int64_t m, const int32_t *cand, const float *g) {
  for (int64_t i = 0; i < n; i++)
    for (int64_t j = 0; j < m; j++) {
      if (cand && cand[j] < 0) continue;
      uint32_t bits;
      memcpy(&bits, g + i * m + j, 4);
      const uint32_t a = bits & 0x7FFFFFFFu;
      if (a != 0u && (a < 0x21800000u || a > 0x5D800000u)) {
        char msg[200];
        snprintf(msg, sizeof msg, "%s: vector %lld, candidate %lld: %g is not finite, or neither 0 nor within 2^-60 .. 2^60", who,
                 (long long)i, (long long)j, (double)g[i * m + j]);
        return w2b_internal_fail(W2B_EINVAL, msg);
      }
    }
  return W2B_OK;
}
}  // namespace
