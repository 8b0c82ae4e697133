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

// The back-projection's arithmetic, nothing refused: per vector and column, segments of W2B_EMBED_WSEG candidate positions
// counted from position 0; P_s = +0, P_s = fmaf(g[i][j], (float)t_r[a], P_s) over the live positions of the segment in
// order; S = S + P_s in segment order, one float32 add each; dx = S * q, one float32 multiply.  (w2b_embed_xent_host sends
// its own g through it: a g it has computed, not one a caller supplies.)
static void backproject_chains(const uint64_t *packed, int64_t dim, int32_t bitlevel, int64_t n, const float *g, int64_t m,
                               const int32_t *cand, float *dx) {
#pragma clang fp contract(off)
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
}

// The back-projection: the validation of the host form, then the chains above.
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
  if (!packed) return w2b_internal_fail(W2B_EINVAL, "w2b_embed_xent_host: null table");
  if (rows < 0 || rows > 0x7FFFFF00ll || dim < 1 || dim > (1 << 24))
    return w2b_internal_fail(W2B_EINVAL, "w2b_embed_xent_host: unsupported rows / dim");
  if (bitlevel != 1 && bitlevel != 2) return w2b_internal_fail(W2B_EUNSUPPORTED, "w2b_embed_xent_host: bitlevel must be 1 or 2");
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
