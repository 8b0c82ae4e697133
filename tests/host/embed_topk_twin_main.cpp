// embed_topk_twin_main.cpp -- the host twin of the packed embedding's top-k selection (w2b_embed_topk_host,
// word2bits_amd/csrc/w2b_embed_twins.cpp) as a program of its own for the host sanitizers: `make -C word2bits_amd/csrc
// host-check` builds it with -fsanitize=address,undefined from this file and w2b_embed_twins.cpp alone (no library, no HIP,
// no GPU) and runs it.  Every buffer has exactly the size the header promises, so a read or a write past it is a report.
// What the twin computes bit for bit is the business of tests/test_embed_topk_host.py; here: a good path per bitlevel at
// dims with a partial last word (1, 65, 130), candidates with padding and repeats against a stable sort of the projection's
// twin, cand == NULL, k beyond the live positions, m == 0, and every refusal with the outputs untouched.  Prints one line
// and exits 0; a call that fails, or a refusal that does not come, is exit 1.
#include "../../include/word2bits_embed.h"
#include "../../include/word2bits_hip.h"

#include <algorithm>
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
  printf("w2b_embed_topk_host: %s: %s\n", what, g_error.c_str());
  exit(1);
}

void refuse(int rc, int code, const char *message, const std::vector<float> &vals, const std::vector<int32_t> &pos) {
  if (rc != code || g_error.find(message) == std::string::npos) fail(message);
  for (float v : vals)
    if (v != 7.5f) fail("a refused call wrote values");
  for (int32_t v : pos)
    if (v != 75) fail("a refused call wrote positions");
  g_refused++;
}

uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

// the first k of a stable descending sort of the live positions of one row of logits; -1 / -inf behind them
void expect(const float *l, int64_t m, const int32_t *cand, int k, const float *vals, const int32_t *pos) {
  std::vector<int32_t> order;
  for (int64_t j = 0; j < m; j++)
    if (!cand || cand[j] >= 0) order.push_back((int32_t)j);
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return l[a] > l[b]; });
  for (int c = 0; c < k; c++) {
    if ((size_t)c < order.size()) {
      if (pos[c] != order[(size_t)c] || bits(vals[c]) != bits(l[order[(size_t)c]])) fail("the first k of a stable descending sort");
    } else if (pos[c] != -1 || bits(vals[c]) != 0xFF800000u) {
      fail("the list ends in -1 / -inf");
    }
  }
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
      for (int64_t a = 0; a < dim; a++) x[(size_t)a] = 0.f;                    // vector 0: every logit +0.0, ties throughout

      // candidates with padding and repeats; k below, at and beyond the six live positions
      const std::vector<int32_t> cand = {3, -1, 3, 36, 0, -7, 36, 12};
      const int64_t m = (int64_t)cand.size();
      std::vector<float> l((size_t)(n * m));
      if (w2b_embed_project_host(p.data(), rows, dim, bitlevel, n, x.data(), m, cand.data(), l.data()) != W2B_OK) fail("projection");
      for (int k : {1, 2, 6, 7, 64}) {
        std::vector<float> vals((size_t)(n * k), 7.5f);
        std::vector<int32_t> pos((size_t)(n * k), 75);
        if (w2b_embed_topk_host(p.data(), rows, dim, bitlevel, n, x.data(), m, cand.data(), k, vals.data(), pos.data()) != W2B_OK)
          fail("call failed");
        g_ok++;
        for (int64_t i = 0; i < n; i++) expect(l.data() + i * m, m, cand.data(), k, vals.data() + i * k, pos.data() + i * k);
        if (pos[0] != 0 || (k > 1 && pos[1] != 2)) fail("equal logits rank in ascending position");
      }

      // every row
      std::vector<float> all((size_t)(n * rows));
      if (w2b_embed_project_host(p.data(), rows, dim, bitlevel, n, x.data(), rows, nullptr, all.data()) != W2B_OK) fail("projection");
      for (int k : {1, 37, 38}) {
        std::vector<float> vals((size_t)(n * k), 7.5f);
        std::vector<int32_t> pos((size_t)(n * k), 75);
        if (w2b_embed_topk_host(p.data(), rows, dim, bitlevel, n, x.data(), rows, nullptr, k, vals.data(), pos.data()) != W2B_OK)
          fail("cand == NULL");
        g_ok++;
        for (int64_t i = 0; i < n; i++) expect(all.data() + i * rows, rows, nullptr, k, vals.data() + i * k, pos.data() + i * k);
      }

      // empty calls: n == 0 touches nothing, m == 0 writes empty lists
      const int K = 3;
      std::vector<float> kv((size_t)(n * K), 7.5f);
      std::vector<int32_t> kp((size_t)(n * K), 75);
      if (w2b_embed_topk_host(p.data(), rows, dim, bitlevel, 0, nullptr, m, cand.data(), K, nullptr, nullptr) != W2B_OK) fail("n == 0");
      if (w2b_embed_topk_host(p.data(), rows, dim, bitlevel, n, x.data(), 0, cand.data(), K, kv.data(), kp.data()) != W2B_OK) fail("m == 0");
      g_ok += 2;
      for (size_t c = 0; c < kv.size(); c++)
        if (bits(kv[c]) != 0xFF800000u || kp[c] != -1) fail("m == 0 writes empty lists");

      // refusals: the outputs keep their 7.5 and 75
      std::vector<float> keepv((size_t)(n * K), 7.5f);
      std::vector<int32_t> keepp((size_t)(n * K), 75);
      auto call = [&](int64_t nn, const float *xx, int64_t mm, const int32_t *cc, int kk, float *vv, int32_t *pp, int bl = 0) {
        return w2b_embed_topk_host(p.data(), rows, dim, bl ? bl : bitlevel, nn, xx, mm, cc, kk, vv, pp);
      };
      refuse(call(-1, x.data(), m, cand.data(), K, keepv.data(), keepp.data()), W2B_EINVAL, "bad vector count", keepv, keepp);
      refuse(call(n, x.data(), -1, cand.data(), K, keepv.data(), keepp.data()), W2B_EINVAL, "bad candidate count", keepv, keepp);
      refuse(call(n, x.data(), m, cand.data(), 0, keepv.data(), keepp.data()), W2B_EINVAL, "k = 0", keepv, keepp);
      refuse(call(n, x.data(), m, cand.data(), 65, keepv.data(), keepp.data()), W2B_EINVAL, "k = 65", keepv, keepp);
      refuse(call(n, nullptr, m, cand.data(), K, keepv.data(), keepp.data()), W2B_EINVAL, "null vectors", keepv, keepp);
      refuse(call(n, x.data(), m, cand.data(), K, nullptr, keepp.data()), W2B_EINVAL, "null output", keepv, keepp);
      refuse(call(n, x.data(), m, cand.data(), K, keepv.data(), nullptr), W2B_EINVAL, "null output", keepv, keepp);
      refuse(w2b_embed_topk_host(nullptr, rows, dim, bitlevel, n, x.data(), m, cand.data(), K, keepv.data(), keepp.data()), W2B_EINVAL,
             "null table", keepv, keepp);
      refuse(call(n, x.data(), m, cand.data(), K, keepv.data(), keepp.data(), 3), W2B_EUNSUPPORTED, "bitlevel must be 1 or 2", keepv, keepp);
      refuse(call(n, x.data(), m, nullptr, K, keepv.data(), keepp.data()), W2B_EINVAL, "must be rows", keepv, keepp);
      std::vector<int32_t> bad = cand;
      bad[4] = (int32_t)rows;
      refuse(call(n, x.data(), m, bad.data(), K, keepv.data(), keepp.data()), W2B_EINVAL, "cand[4]", keepv, keepp);
      const float inf = std::numeric_limits<float>::infinity();
      for (float v : {std::nanf(""), inf, -inf, ldexpf(1.f, 61), -ldexpf(1.f, -61), 1e-45f}) {
        std::vector<float> y = x;
        y[(size_t)(2 * dim + dim - 1)] = v;
        const std::string where = "vector 2, column " + std::to_string(dim - 1);
        refuse(call(n, y.data(), m, cand.data(), K, keepv.data(), keepp.data()), W2B_EINVAL, where.c_str(), keepv, keepp);
      }
    }
  printf("w2b_embed_topk_host: %d calls ok, %d refused\n", g_ok, g_refused);
  return 0;
}
