// embed_project_twin_main.cpp -- the host twin of the packed embedding's projection (w2b_embed_project_host,
// word2bits_amd/csrc/w2b_embed_twins.cpp) as a program of its own for the host sanitizers: `make -C word2bits_amd/csrc
// host-check` builds it with -fsanitize=address,undefined from this file and w2b_embed_twins.cpp alone (no library, no HIP,
// no GPU) and runs it.  Every buffer has exactly the size the header promises, so a read or a write past it is a report.
// What the twin computes bit for bit is the business of tests/test_embed_project_host.py; here: a good path per bitlevel at
// dims with a partial last word (1, 65, 130), candidates with padding and repeats, cand == NULL, the unit-vector identity,
// and every refusal with `out` untouched.  Prints one line and exits 0; a call that fails, or a refusal that does not come,
// is exit 1.
#include "../../include/word2bits_embed.h"
#include "../../include/word2bits_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

static std::string g_error;
int w2b_internal_fail(int code, const char *msg) {   // the library's is in w2b_trainer.cpp
  g_error = msg ? msg : "";
  return code;
}

namespace {
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {   // xorshift64
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

int g_ok = 0, g_refused = 0;

void fail(const char *what) {
  printf("w2b_embed_project_host: %s: %s\n", what, g_error.c_str());
  exit(1);
}

void refuse(int rc, int code, const char *message, const std::vector<float> &out) {
  if (rc != code || g_error.find(message) == std::string::npos) fail(message);
  for (float v : out)
    if (v != 7.5f) fail("a refused call wrote an output");
  g_refused++;
}

// the value of row r, column a: t / 3 (as 0x3EAAAAAB) at one bit, t / 4 at two
int code_of(const std::vector<uint64_t> &p, int64_t wpr, int bitlevel, int64_t r, int64_t a) {
  const uint64_t *blk = p.data() + r * wpr + (a >> 6) * bitlevel;
  const int s = (int)((blk[0] >> (a & 63)) & 1u);
  const int mag = bitlevel == 2 && ((blk[1] >> (a & 63)) & 1u) ? 3 : 1;
  return s ? -mag : mag;
}
}  // namespace

int main() {
  const int64_t dims[] = {1, 65, 130}, rows = 37, n = 5;
  for (int bitlevel = 1; bitlevel <= 2; bitlevel++)
    for (int64_t dim : dims) {
      const int64_t wpr = (dim + 63) / 64 * bitlevel;
      std::vector<uint64_t> p((size_t)(rows * wpr));
      for (uint64_t &w : p) w = rnd();                    // the padding bits of the last block included: they must not count
      std::vector<float> x((size_t)(n * dim));
      for (float &v : x) v = (float)((int64_t)(rnd() % 2001) - 1000) / 256.f;
      const float q = bitlevel == 1 ? 0.3333333432674407958984375f : 0.25f;

      // candidates with padding and repeats
      const std::vector<int32_t> cand = {3, -1, 3, 36, 0, -7, 36, 12};
      const int64_t m = (int64_t)cand.size();
      std::vector<float> out((size_t)(n * m), 7.5f);
      if (w2b_embed_project_host(p.data(), rows, dim, bitlevel, n, x.data(), m, cand.data(), out.data()) != W2B_OK) fail("call failed");
      g_ok++;
      for (int64_t i = 0; i < n; i++) {
        if (out[(size_t)(i * m + 1)] != 0.f || std::signbit(out[(size_t)(i * m + 1)]) || out[(size_t)(i * m + 5)] != 0.f)
          fail("a padding candidate is a column of +0.0");
        if (out[(size_t)(i * m)] != out[(size_t)(i * m + 2)] || out[(size_t)(i * m + 3)] != out[(size_t)(i * m + 6)])
          fail("a repeated candidate repeats its column");
        float S = 0.f;
        for (int64_t a = 0; a < dim; a++) S = fmaf(x[(size_t)(i * dim + a)], (float)code_of(p, wpr, bitlevel, 12, a), S);
        if (out[(size_t)(i * m + 7)] != S * q) fail("the chain of the header");
      }

      // every row, and the same through an explicit list
      std::vector<float> all((size_t)(n * rows), 7.5f), listed((size_t)(n * rows), 7.5f);
      std::vector<int32_t> every((size_t)rows);
      for (int64_t r = 0; r < rows; r++) every[(size_t)r] = (int32_t)r;
      if (w2b_embed_project_host(p.data(), rows, dim, bitlevel, n, x.data(), rows, nullptr, all.data()) != W2B_OK) fail("cand == NULL");
      if (w2b_embed_project_host(p.data(), rows, dim, bitlevel, n, x.data(), rows, every.data(), listed.data()) != W2B_OK) fail("all rows listed");
      g_ok += 2;
      if (all != listed) fail("cand == NULL is every row in row order");

      // unit vectors: the table's own values
      std::vector<float> unit((size_t)(dim * dim), 0.f), tab((size_t)(dim * rows), 7.5f);
      for (int64_t a = 0; a < dim; a++) unit[(size_t)(a * dim + a)] = 1.f;
      if (w2b_embed_project_host(p.data(), rows, dim, bitlevel, dim, unit.data(), rows, nullptr, tab.data()) != W2B_OK) fail("unit vectors");
      g_ok++;
      for (int64_t a = 0; a < dim; a++)
        for (int64_t r = 0; r < rows; r++)
          if (tab[(size_t)(a * rows + r)] != (float)code_of(p, wpr, bitlevel, r, a) * q) fail("a unit vector reads the table");

      // empty calls
      if (w2b_embed_project_host(p.data(), rows, dim, bitlevel, 0, nullptr, m, cand.data(), nullptr) != W2B_OK) fail("n == 0");
      if (w2b_embed_project_host(p.data(), rows, dim, bitlevel, n, x.data(), 0, cand.data(), nullptr) != W2B_OK) fail("m == 0");
      g_ok += 2;

      // refusals: `out` keeps its 7.5
      std::vector<float> keep((size_t)(n * m), 7.5f);
      auto call = [&](int64_t nn, const float *xx, int64_t mm, const int32_t *cc, float *oo, int bl = 0) {
        return w2b_embed_project_host(p.data(), rows, dim, bl ? bl : bitlevel, nn, xx, mm, cc, oo);
      };
      refuse(call(-1, x.data(), m, cand.data(), keep.data()), W2B_EINVAL, "bad vector count", keep);
      refuse(call(n, x.data(), -1, cand.data(), keep.data()), W2B_EINVAL, "bad candidate count", keep);
      refuse(call(n, nullptr, m, cand.data(), keep.data()), W2B_EINVAL, "null vectors", keep);
      refuse(call(n, x.data(), m, cand.data(), nullptr), W2B_EINVAL, "null output", keep);
      refuse(w2b_embed_project_host(nullptr, rows, dim, bitlevel, n, x.data(), m, cand.data(), keep.data()), W2B_EINVAL, "null table", keep);
      refuse(call(n, x.data(), m, cand.data(), keep.data(), 3), W2B_EUNSUPPORTED, "bitlevel must be 1 or 2", keep);
      refuse(call(n, x.data(), m, nullptr, keep.data()), W2B_EINVAL, "must be rows", keep);
      std::vector<int32_t> bad = cand;
      bad[4] = (int32_t)rows;
      refuse(call(n, x.data(), m, bad.data(), keep.data()), W2B_EINVAL, "cand[4]", keep);
      const float inf = std::numeric_limits<float>::infinity();
      for (float v : {std::nanf(""), inf, -inf, ldexpf(1.f, 61), -ldexpf(1.f, -61), 1e-45f}) {
        std::vector<float> y = x;
        y[(size_t)(2 * dim + dim - 1)] = v;
        const std::string where = "vector 2, column " + std::to_string(dim - 1);
        refuse(call(n, y.data(), m, cand.data(), keep.data()), W2B_EINVAL, where.c_str(), keep);
      }
      std::vector<float> edge = x;                        // the bounds themselves, and zeros of either sign, are fine
      edge[0] = ldexpf(1.f, 60);
      edge[(size_t)(dim - 1)] = -ldexpf(1.f, -60);
      edge[(size_t)dim] = -0.f;
      if (call(n, edge.data(), m, cand.data(), keep.data()) != W2B_OK) fail("2^60, 2^-60 and -0 are allowed");
      g_ok++;
    }
  printf("w2b_embed_project_host: %d calls ok, %d refused\n", g_ok, g_refused);
  return 0;
}
