// w2b_embed_twins.cpp -- the host twins of the packed embedding's projection and back-projection kernels
// (include/word2bits_embed.h, "Projection" and "Back-projection"): what every GPU test of w2b_embed_project and
// w2b_embed_backproject compares the kernels against.  They restate the header's definitions
// on the packed rows themselves, one fused multiply-add per column (per candidate position).  No handle, no stream and no device call: the unit
// includes no device header, and a program that links nothing but this file and a w2b_internal_fail of its own can run it
// under a host sanitizer (tests/host/embed_project_twin_main.cpp, `make host-check`).  What it refuses comes from
// w2b_embed_shared.h, as for the host form.  (The twins of lookup and bags are in w2b_embed.cpp.)
#include "w2b_embed_shared.h"

#include <cmath>
#include <vector>

// S = +0; S = fmaf(x[i][a], (float)t_r[a], S) for a = 0 .. dim - 1; out[i][j] = S * q.  The multiply is one float32 operation:
// this file is built with -ffp-contract=off and the function says so again.
extern "C" int w2b_embed_project_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n,
                                      const float *x, int64_t m, const int32_t *cand, float *out) {
#pragma clang fp contract(off)
  const char *who = "w2b_embed_project_host";
  if (int rc = project_check_args(who, n, x, m, true, out)) return rc;
  if (!packed) return w2b_internal_fail(W2B_EINVAL, "w2b_embed_project_host: null table");
  if (rows < 0 || rows > 0x7FFFFF00ll || dim < 1 || dim > (1 << 24))
    return w2b_internal_fail(W2B_EINVAL, "w2b_embed_project_host: unsupported rows / dim");
  if (bitlevel != 1 && bitlevel != 2) return w2b_internal_fail(W2B_EUNSUPPORTED, "w2b_embed_project_host: bitlevel must be 1 or 2");
  if (int rc = project_check_cand(who, rows, m, cand)) return rc;
  if (int rc = project_check_values(who, n, dim, x)) return rc;
  if (n == 0 || m == 0) return W2B_OK;
  const int64_t wpr = (dim + 63) / 64 * bitlevel;
  uint32_t qbits = bitlevel == 1 ? 0x3EAAAAABu : 0x3E800000u;
  float q;
  memcpy(&q, &qbits, 4);
  std::vector<float> t((size_t)dim);
  for (int64_t j = 0; j < m; j++) {
    const int64_t r = cand ? (int64_t)cand[j] : j;
    if (r < 0) {                                             // padding: a column of +0.0
      for (int64_t i = 0; i < n; i++) out[i * m + j] = 0.f;
      continue;
    }
    const uint64_t *row = packed + r * wpr;
    for (int64_t a = 0; a < dim; a++) {
      const uint64_t *blk = row + (a >> 6) * bitlevel;
      const int sg = (int)((blk[0] >> (a & 63)) & 1u);
      const int mag = bitlevel == 2 && ((blk[1] >> (a & 63)) & 1u) ? 3 : 1;
      t[(size_t)a] = (float)(sg ? -mag : mag);
    }
    for (int64_t i = 0; i < n; i++) {
      const float *xi = x + i * dim;
      float S = 0.f;
      for (int64_t a = 0; a < dim; a++) S = fmaf(xi[a], t[(size_t)a], S);      // strictly sequential, one accumulator
      out[i * m + j] = S * q;
    }
  }
  return W2B_OK;
}

// The back-projection: per vector and column, segments of W2B_EMBED_WSEG candidate positions counted from position 0;
// P_s = +0, P_s = fmaf(g[i][j], (float)t_r[a], P_s) over the live positions of the segment in order; S = S + P_s in segment
// order, one float32 add each; dx = S * q, one float32 multiply.
extern "C" int w2b_embed_backproject_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n,
                                          const float *g, int64_t m, const int32_t *cand, float *dx) {
#pragma clang fp contract(off)
  const char *who = "w2b_embed_backproject_host";
  if (int rc = backproject_check_args(who, n, g, m, dx)) return rc;
  if (!packed) return w2b_internal_fail(W2B_EINVAL, "w2b_embed_backproject_host: null table");
  if (rows < 0 || rows > 0x7FFFFF00ll || dim < 1 || dim > (1 << 24))
    return w2b_internal_fail(W2B_EINVAL, "w2b_embed_backproject_host: unsupported rows / dim");
  if (bitlevel != 1 && bitlevel != 2)
    return w2b_internal_fail(W2B_EUNSUPPORTED, "w2b_embed_backproject_host: bitlevel must be 1 or 2");
  if (int rc = project_check_cand(who, rows, m, cand)) return rc;
  if (int rc = backproject_check_values(who, n, m, cand, g)) return rc;
  if (n == 0) return W2B_OK;
  const int64_t wpr = (dim + 63) / 64 * bitlevel;
  uint32_t qbits = bitlevel == 1 ? 0x3EAAAAABu : 0x3E800000u;
  float q;
  memcpy(&q, &qbits, 4);
  std::vector<float> t((size_t)dim), P((size_t)(n * dim)), S((size_t)(n * dim), 0.f);
  for (int64_t s0 = 0; s0 < m; s0 += W2B_EMBED_WSEG) {       // one segment: one chain per (vector, column)
    const int64_t s1 = s0 + W2B_EMBED_WSEG < m ? s0 + W2B_EMBED_WSEG : m;
    for (size_t k = 0; k < P.size(); k++) P[k] = 0.f;
    for (int64_t j = s0; j < s1; j++) {
      const int64_t r = cand ? (int64_t)cand[j] : j;
      if (r < 0) continue;                                   // padding: g is not looked at
      const uint64_t *row = packed + r * wpr;
      for (int64_t a = 0; a < dim; a++) {
        const uint64_t *blk = row + (a >> 6) * bitlevel;
        const int sg = (int)((blk[0] >> (a & 63)) & 1u);
        const int mag = bitlevel == 2 && ((blk[1] >> (a & 63)) & 1u) ? 3 : 1;
        t[(size_t)a] = (float)(sg ? -mag : mag);
      }
      for (int64_t i = 0; i < n; i++) {
        const float w = g[i * m + j];
        float *Pi = P.data() + i * dim;
        for (int64_t a = 0; a < dim; a++) Pi[a] = fmaf(w, t[(size_t)a], Pi[a]);
      }
    }
    for (size_t k = 0; k < S.size(); k++) S[k] = S[k] + P[k];                  // one float32 add per segment
  }
  for (size_t k = 0; k < S.size(); k++) dx[k] = S[k] * q;                       // one float32 multiply
  return W2B_OK;
}
