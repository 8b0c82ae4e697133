// embed_backproject_twin_main.cpp -- the host twin of the packed embedding's back-projection (w2b_embed_backproject_host,
// word2bits_amd/csrc/w2b_embed_twins.cpp) as a program of its own for the host sanitizers: `make -C word2bits_amd/csrc
// host-check` builds it with -fsanitize=address,undefined from this file and w2b_embed_twins.cpp alone (no library, no HIP,
// no GPU) and runs it.  Every buffer has exactly the size the header promises, so a read or a write past it is a report.
// What the twin computes bit for bit is the business of tests/test_embed_backproject_host.py; here the edge shapes: dim
// 1 / 63 / 64 / 65, m 0 / 1 / 1023 / 1024 / 1025 / 2049 with padding first and last (whose g is NaN), cand == NULL, each
// against the segments written out once more, and every refusal with `dx` untouched.  Prints one line and exits 0; a call
// that fails, or a refusal that does not come, is exit 1.
#include "../../include/word2bits_embed.h"
#include "../../include/word2bits_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  printf("w2b_embed_backproject_host: %s: %s\n", what, g_error.c_str());
  exit(1);
}

void refuse(int rc, int code, const char *message, const std::vector<float> &out) {
  if (rc != code || g_error.find(message) == std::string::npos) fail(message);
  for (float v : out)
    if (v != 7.5f) fail("a refused call wrote an output");
  g_refused++;
}

int code_of(const std::vector<uint64_t> &p, int64_t wpr, int bitlevel, int64_t r, int64_t a) {
  const uint64_t *blk = p.data() + r * wpr + (a >> 6) * bitlevel;
  const int s = (int)((blk[0] >> (a & 63)) & 1u);
  const int mag = bitlevel == 2 && ((blk[1] >> (a & 63)) & 1u) ? 3 : 1;
  return s ? -mag : mag;
}

bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }
}  // namespace

int main() {
  const int64_t dims[] = {1, 63, 64, 65}, ms[] = {0, 1, 1023, 1024, 1025, 2049}, rows = 37, n = 3;
  const float nan = std::nanf(""), inf = std::numeric_limits<float>::infinity();
  for (int bitlevel = 1; bitlevel <= 2; bitlevel++)
    for (int64_t dim : dims) {
      const int64_t wpr = (dim + 63) / 64 * bitlevel;
      std::vector<uint64_t> p((size_t)(rows * wpr));
      for (uint64_t &w : p) w = rnd();                    // the padding bits of the last block included: they must not count
      const float q = bitlevel == 1 ? 0.3333333432674407958984375f : 0.25f;
      for (int64_t m : ms) {
        std::vector<int32_t> cand((size_t)m);
        cand.reserve(1);                                  // (an empty list is still a list: data() is not NULL)
        for (int32_t &c : cand) c = (int32_t)(rnd() % (uint64_t)rows);
        if (m >= 3) cand[0] = -1, cand[(size_t)(m - 1)] = -4, cand[(size_t)(m / 2)] = cand[1];   // padding first and last, a repeat
        std::vector<float> g((size_t)(n * m));
        for (float &v : g) v = ldexpf((float)((int64_t)(rnd() % 2001) - 1000), (int)(rnd() % 40) - 20);
        for (int64_t i = 0; i < n && m >= 3; i++) g[(size_t)(i * m)] = nan, g[(size_t)(i * m + m - 1)] = inf;   // on padding: ignored
        std::vector<float> dx((size_t)(n * dim), 7.5f);
        if (w2b_embed_backproject_host(p.data(), rows, dim, bitlevel, n, g.data(), m, cand.data(), dx.data()) != W2B_OK) fail("call failed");
        g_ok++;
        for (int64_t i = 0; i < n; i++)
          for (int64_t a = 0; a < dim; a++) {             // the definition, once more
            float S = 0.f;
            for (int64_t s0 = 0; s0 < m; s0 += W2B_EMBED_WSEG) {
              float P = 0.f;
              for (int64_t j = s0; j < m && j < s0 + W2B_EMBED_WSEG; j++)
                if (cand[(size_t)j] >= 0) P = fmaf(g[(size_t)(i * m + j)], (float)code_of(p, wpr, bitlevel, cand[(size_t)j], a), P);
              S = S + P;
            }
            if (!same_bits(dx[(size_t)(i * dim + a)], S * q)) fail("the segments of the header");
          }
        if (m == 0)
          for (float v : dx)
            if (!same_bits(v, 0.f)) fail("m == 0 writes +0.0");
      }

      // every row, and the same through an explicit list
      std::vector<float> g((size_t)(n * rows));
      for (float &v : g) v = (float)((int64_t)(rnd() % 2001) - 1000) / 256.f;
      std::vector<float> all((size_t)(n * dim), 7.5f), listed((size_t)(n * dim), 7.5f);
      std::vector<int32_t> every((size_t)rows);
      for (int64_t r = 0; r < rows; r++) every[(size_t)r] = (int32_t)r;
      if (w2b_embed_backproject_host(p.data(), rows, dim, bitlevel, n, g.data(), rows, nullptr, all.data()) != W2B_OK) fail("cand == NULL");
      if (w2b_embed_backproject_host(p.data(), rows, dim, bitlevel, n, g.data(), rows, every.data(), listed.data()) != W2B_OK) fail("all rows listed");
      g_ok += 2;
      if (memcmp(all.data(), listed.data(), all.size() * 4) != 0) fail("cand == NULL is every row in row order");

      // one-hot g: the table's own values
      std::vector<float> unit((size_t)(rows * rows), 0.f), tab((size_t)(rows * dim), 7.5f);
      for (int64_t r = 0; r < rows; r++) unit[(size_t)(r * rows + r)] = 1.f;
      if (w2b_embed_backproject_host(p.data(), rows, dim, bitlevel, rows, unit.data(), rows, nullptr, tab.data()) != W2B_OK) fail("one-hot");
      g_ok++;
      for (int64_t r = 0; r < rows; r++)
        for (int64_t a = 0; a < dim; a++)
          if (!same_bits(tab[(size_t)(r * dim + a)], (float)code_of(p, wpr, bitlevel, r, a) * q)) fail("a one-hot g reads the table");

      // n == 0
      if (w2b_embed_backproject_host(p.data(), rows, dim, bitlevel, 0, nullptr, rows, nullptr, nullptr) != W2B_OK) fail("n == 0");
      g_ok++;

      // refusals: `dx` keeps its 7.5
      const std::vector<int32_t> cand = {3, -1, 3, 36, 0, -7, 36, 12};
      const int64_t m = (int64_t)cand.size();
      std::vector<float> gg((size_t)(n * m), 0.5f), keep((size_t)(n * dim), 7.5f);
      auto call = [&](int64_t nn, const float *g_, int64_t mm, const int32_t *cc, float *oo, int bl = 0) {
        return w2b_embed_backproject_host(p.data(), rows, dim, bl ? bl : bitlevel, nn, g_, mm, cc, oo);
      };
      refuse(call(-1, gg.data(), m, cand.data(), keep.data()), W2B_EINVAL, "bad vector count", keep);
      refuse(call(n, gg.data(), -1, cand.data(), keep.data()), W2B_EINVAL, "bad candidate count", keep);
      refuse(call(n, nullptr, m, cand.data(), keep.data()), W2B_EINVAL, "null g", keep);
      refuse(call(n, gg.data(), m, cand.data(), nullptr), W2B_EINVAL, "null output", keep);
      refuse(w2b_embed_backproject_host(nullptr, rows, dim, bitlevel, n, gg.data(), m, cand.data(), keep.data()), W2B_EINVAL, "null table", keep);
      refuse(call(n, gg.data(), m, cand.data(), keep.data(), 3), W2B_EUNSUPPORTED, "bitlevel must be 1 or 2", keep);
      refuse(call(n, gg.data(), m, nullptr, keep.data()), W2B_EINVAL, "must be rows", keep);
      std::vector<int32_t> bad = cand;
      bad[4] = (int32_t)rows;
      refuse(call(n, gg.data(), m, bad.data(), keep.data()), W2B_EINVAL, "cand[4]", keep);
      for (float v : {nan, inf, -inf, ldexpf(1.f, 61), -ldexpf(1.f, -61), 1e-45f}) {
        std::vector<float> y = gg;
        y[(size_t)(2 * m + 7)] = v;
        refuse(call(n, y.data(), m, cand.data(), keep.data()), W2B_EINVAL, "vector 2, candidate 7", keep);
        y = gg;
        y[(size_t)(2 * m + 5)] = v;                       // on a padding candidate: accepted
        std::vector<float> fine((size_t)(n * dim), 7.5f);
        if (call(n, y.data(), m, cand.data(), fine.data()) != W2B_OK) fail("g on a padding candidate is ignored");
        g_ok++;
      }
      std::vector<float> edge = gg;                       // the bounds themselves, and zeros of either sign, are fine
      edge[0] = ldexpf(1.f, 60);
      edge[2] = -ldexpf(1.f, -60);
      edge[3] = -0.f;
      std::vector<float> fine((size_t)(n * dim), 7.5f);
      if (call(n, edge.data(), m, cand.data(), fine.data()) != W2B_OK) fail("2^60, 2^-60 and -0 are allowed");
      g_ok++;
    }
  printf("w2b_embed_backproject_host: %d calls ok, %d refused\n", g_ok, g_refused);
  return 0;
}
