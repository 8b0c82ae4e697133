// embed_xent_twin_main.cpp -- the host twin of the packed embedding's cross-entropy (w2b_embed_xent_host and
// w2b_embed_expneg_host, word2bits_amd/csrc/w2b_embed_twins.cpp) as a program of its own for the host sanitizers: `make -C
// word2bits_amd/csrc host-check` builds it with -fsanitize=address,undefined from this file and w2b_embed_twins.cpp alone (no
// library, no HIP, no GPU) and runs it.  Every buffer has exactly the size the header promises, so a read or a write past it
// is a report.  What the twin computes bit for bit is the business of tests/test_embed_xent_host.py; here the edge shapes:
// dim 1 / 63 / 64 / 65, m 0 / 1 / 255 / 256 / 257 / 1025 with padding first and last, cand == NULL, dx == NULL, targets on
// the first and the last live position and ignored vectors, x of ordinary size and x whose logits lie more than 64 apart,
// with the identities that cost nothing (mx and tl are logits of the projection's twin, m == 1 gives se == 1 and dx == +0,
// an ignored vector has tl == +0 and dx == +0), and every refusal with the outputs untouched.  Prints one line and exits 0;
// a call that fails, or a refusal that does not come, is exit 1.
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
  printf("w2b_embed_xent_host: %s: %s\n", what, g_error.c_str());
  exit(1);
}

bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

struct Out {
  std::vector<float> mx, se, tl, dx;
  Out(int64_t n, int64_t dim) : mx((size_t)n, 7.5f), se((size_t)n, 7.5f), tl((size_t)n, 7.5f), dx((size_t)(n * dim), 7.5f) {}
  bool untouched() const {
    for (const std::vector<float> *v : {&mx, &se, &tl, &dx})
      for (float f : *v)
        if (f != 7.5f) return false;
    return true;
  }
};

void refuse(int rc, int code, const char *message, const Out &o) {
  if (rc != code || g_error.find(message) == std::string::npos) fail(message);
  if (!o.untouched()) fail("a refused call wrote an output");
  g_refused++;
}
}  // namespace

int main() {
  const float nan = std::nanf(""), inf = std::numeric_limits<float>::infinity();
  // expneg: the exact cases
  if (!same_bits(w2b_embed_expneg_host(0.f), 1.f)) fail("expneg(0) == 1");
  for (float r : {-64.00001f, -100.f, -inf, nan})
    if (!same_bits(w2b_embed_expneg_host(r), 0.f)) fail("expneg is +0 below -64 and for NaN");
  for (float r = -64.f; r < 0.f; r += 0.37f) {
    const float v = w2b_embed_expneg_host(r);
    if (!(v >= ldexpf(1.f, -93) && v <= 1.f)) fail("expneg is normal and at most 1");
  }

  const int64_t dims[] = {1, 63, 64, 65}, ms[] = {0, 1, 255, 256, 257, 1025}, rows = 37, n = 3;
  for (int bitlevel = 1; bitlevel <= 2; bitlevel++)
    for (int64_t dim : dims) {
      const int64_t wpr = (dim + 63) / 64 * bitlevel;
      std::vector<uint64_t> p((size_t)(rows * wpr));
      for (uint64_t &w : p) w = rnd();                    // the padding bits of the last block included: they must not count
      for (int64_t m : ms)
        for (int wide = 0; wide < 2; wide++) {
          std::vector<int32_t> cand((size_t)m);
          cand.reserve(1);                                // (an empty list is still a list: data() is not NULL)
          for (int32_t &c : cand) c = (int32_t)(rnd() % (uint64_t)rows);
          if (m >= 3) cand[0] = -1, cand[(size_t)(m - 1)] = -4, cand[(size_t)(m / 2)] = cand[1];   // padding first and last, a repeat
          std::vector<float> x((size_t)(n * dim));
          for (float &v : x) v = ldexpf((float)((int64_t)(rnd() % 33) - 16), wide ? (int)(rnd() % 40) - 10 : -6);
          // targets: the first live position, ignored, the last live position
          const int32_t first = m >= 3 ? 1 : 0, last = m >= 3 ? (int32_t)(m - 2) : (int32_t)(m - 1);
          std::vector<int32_t> target = {m > 0 ? first : -1, -1, m > 0 ? last : -2};
          Out o(n, dim);
          if (w2b_embed_xent_host(p.data(), rows, dim, bitlevel, n, x.data(), m, cand.data(), target.data(), o.mx.data(),
                                  o.se.data(), o.tl.data(), o.dx.data()) != W2B_OK)
            fail("call failed");
          Out s(n, dim);                                  // the statistics alone: dx == NULL
          if (w2b_embed_xent_host(p.data(), rows, dim, bitlevel, n, x.data(), m, cand.data(), target.data(), s.mx.data(),
                                  s.se.data(), s.tl.data(), nullptr) != W2B_OK)
            fail("dx == NULL");
          g_ok += 2;
          std::vector<float> l((size_t)(n * m) + 1);
          if (w2b_embed_project_host(p.data(), rows, dim, bitlevel, n, x.data(), m, cand.data(), l.data()) != W2B_OK) fail("projection");
          for (int64_t i = 0; i < n; i++) {
            if (!same_bits(o.mx[(size_t)i], s.mx[(size_t)i]) || !same_bits(o.se[(size_t)i], s.se[(size_t)i]) ||
                !same_bits(o.tl[(size_t)i], s.tl[(size_t)i]))
              fail("the statistics do not depend on dx");
            bool any = false;
            float top = 0.f;
            for (int64_t j = 0; j < m; j++)
              if (cand[(size_t)j] >= 0 && (!any || l[(size_t)(i * m + j)] > top)) top = l[(size_t)(i * m + j)], any = true;
            if (!same_bits(o.mx[(size_t)i], any ? top : 0.f)) fail("mx is the largest logit of the projection's twin");
            const float want_tl = target[(size_t)i] >= 0 ? l[(size_t)(i * m + target[(size_t)i])] : 0.f;
            if (!same_bits(o.tl[(size_t)i], want_tl)) fail("tl is the target's logit, +0.0 when ignored");
            if (any && !(o.se[(size_t)i] >= 1.f)) fail("se counts the largest term as 1");
            if (!any && !same_bits(o.se[(size_t)i], 0.f)) fail("nothing live: se == +0.0");
            if (target[(size_t)i] < 0 || m == 1)
              for (int64_t a = 0; a < dim; a++)
                if (!same_bits(o.dx[(size_t)(i * dim + a)], 0.f)) fail("dx == +0.0 for an ignored vector and for m == 1");
            if (m == 1 && !same_bits(o.se[(size_t)i], 1.f)) fail("m == 1: se == 1");
          }
          for (float v : s.dx)
            if (v != 7.5f) fail("dx == NULL writes no gradient");
        }

      // every row, and the same through an explicit list
      std::vector<float> x((size_t)(n * dim));
      for (float &v : x) v = (float)((int64_t)(rnd() % 33) - 16) / 64.f;
      std::vector<int32_t> every((size_t)rows), target = {0, (int32_t)(rows - 1), -1};
      for (int64_t r = 0; r < rows; r++) every[(size_t)r] = (int32_t)r;
      Out all(n, dim), listed(n, dim);
      if (w2b_embed_xent_host(p.data(), rows, dim, bitlevel, n, x.data(), rows, nullptr, target.data(), all.mx.data(), all.se.data(),
                              all.tl.data(), all.dx.data()) != W2B_OK)
        fail("cand == NULL");
      if (w2b_embed_xent_host(p.data(), rows, dim, bitlevel, n, x.data(), rows, every.data(), target.data(), listed.mx.data(),
                              listed.se.data(), listed.tl.data(), listed.dx.data()) != W2B_OK)
        fail("all rows listed");
      g_ok += 2;
      if (memcmp(all.mx.data(), listed.mx.data(), (size_t)n * 4) || memcmp(all.se.data(), listed.se.data(), (size_t)n * 4) ||
          memcmp(all.tl.data(), listed.tl.data(), (size_t)n * 4) || memcmp(all.dx.data(), listed.dx.data(), all.dx.size() * 4))
        fail("cand == NULL is every row in row order");

      // n == 0
      if (w2b_embed_xent_host(p.data(), rows, dim, bitlevel, 0, nullptr, rows, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != W2B_OK)
        fail("n == 0");
      g_ok++;

      // refusals: the outputs keep their 7.5
      const std::vector<int32_t> cand = {3, -1, 3, 36, 0, -7, 36, 12};
      const int64_t m = (int64_t)cand.size();
      std::vector<float> xx((size_t)(n * dim), 0.5f);
      const std::vector<int32_t> tg = {0, -1, 7};
      Out keep(n, dim);
      auto call = [&](int64_t nn, const float *x_, int64_t mm, const int32_t *cc, const int32_t *tt, int bl = 0) {
        return w2b_embed_xent_host(p.data(), rows, dim, bl ? bl : bitlevel, nn, x_, mm, cc, tt, keep.mx.data(), keep.se.data(),
                                   keep.tl.data(), keep.dx.data());
      };
      refuse(call(-1, xx.data(), m, cand.data(), tg.data()), W2B_EINVAL, "bad vector count", keep);
      refuse(call(n, xx.data(), -1, cand.data(), tg.data()), W2B_EINVAL, "bad candidate count", keep);
      refuse(call(n, nullptr, m, cand.data(), tg.data()), W2B_EINVAL, "null vectors", keep);
      refuse(call(n, xx.data(), m, cand.data(), nullptr), W2B_EINVAL, "null targets", keep);
      refuse(w2b_embed_xent_host(p.data(), rows, dim, bitlevel, n, xx.data(), m, cand.data(), tg.data(), keep.mx.data(), nullptr,
                                 keep.tl.data(), keep.dx.data()),
             W2B_EINVAL, "null output", keep);
      refuse(w2b_embed_xent_host(nullptr, rows, dim, bitlevel, n, xx.data(), m, cand.data(), tg.data(), keep.mx.data(),
                                 keep.se.data(), keep.tl.data(), keep.dx.data()),
             W2B_EINVAL, "null table", keep);
      refuse(call(n, xx.data(), m, cand.data(), tg.data(), 3), W2B_EUNSUPPORTED, "bitlevel must be 1 or 2", keep);
      refuse(call(n, xx.data(), m, nullptr, tg.data()), W2B_EINVAL, "must be rows", keep);
      std::vector<int32_t> bad = cand;
      bad[4] = (int32_t)rows;
      std::vector<int32_t> bt = tg;
      bt[2] = (int32_t)m;
      refuse(call(n, xx.data(), m, bad.data(), bt.data()), W2B_EINVAL, "cand[4]", keep);            // candidates before targets
      std::vector<float> y = xx;
      y[(size_t)(2 * dim)] = nan;
      refuse(call(n, y.data(), m, cand.data(), bt.data()), W2B_EINVAL, "vector 2: target 8", keep);   // targets before values
      bt[2] = 5;
      refuse(call(n, xx.data(), m, cand.data(), bt.data()), W2B_EINVAL, "vector 2: target 5 is a padding position", keep);
      for (float v : {nan, inf, -inf, ldexpf(1.f, 61), -ldexpf(1.f, -61), 1e-45f}) {
        y = xx;
        y[(size_t)(2 * dim + dim - 1)] = v;
        char where[64];
        snprintf(where, sizeof where, "vector 2, column %lld", (long long)(dim - 1));
        refuse(call(n, y.data(), m, cand.data(), tg.data()), W2B_EINVAL, where, keep);
      }
    }
  printf("w2b_embed_xent_host: %d calls ok, %d refused\n", g_ok, g_refused);
  return 0;
}
