// embed_bag_twin_main.cpp -- the host twins of the packed embedding's lookup and bag kernels (w2b_embed_lookup_host,
// w2b_embed_bag_host, w2b_embed_bag_weighted_host, word2bits_amd/csrc/w2b_embed_twins.cpp) as a program of its own for the
// host sanitizers: `make -C word2bits_amd/csrc host-check` builds it with -fsanitize=address,undefined from this file and
// w2b_embed_twins.cpp alone (no library, no HIP, no GPU) and runs it.  Every buffer has exactly the size the header promises,
// so a read or a write past it is a report.  What the twins compute bit for bit is the business of tests/test_embed_host.py
// and tests/test_embed_weighted_host.py; here: a good path per bitlevel at dims with a partial last word (1, 65, 130), ids
// with padding and repeats, an empty bag, a bag of padding only, a weighted bag of two segments, empty calls, and every
// refusal with `out` untouched.  Prints one line per function and exits 0; a call that fails, or a refusal that does not
// come, is exit 1.
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

struct Count { const char *name; int ok, refused; };
Count g_lookup{"w2b_embed_lookup_host", 0, 0}, g_bag{"w2b_embed_bag_host", 0, 0}, g_bagw{"w2b_embed_bag_weighted_host", 0, 0};

void fail(const Count &c, const char *what) {
  printf("%s: %s: %s\n", c.name, what, g_error.c_str());
  exit(1);
}

void good(Count &c, int rc, const char *what) {
  if (rc != W2B_OK) fail(c, what);
  c.ok++;
}

void refuse(Count &c, int rc, int code, const char *message, const std::vector<float> &out) {
  if (rc != code || g_error.find(c.name) != 0 || g_error.find(message) == std::string::npos) fail(c, message);
  for (float v : out)
    if (v != 7.5f) fail(c, "a refused call wrote an output");
  c.refused++;
}

bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

// the code of row r, column a: its value is code / 3 (as 0x3EAAAAAB) at one bit, code / 4 at two
int code_of(const std::vector<uint64_t> &p, int64_t wpr, int bitlevel, int64_t r, int64_t a) {
  const uint64_t *blk = p.data() + r * wpr + (a >> 6) * bitlevel;
  const int s = (int)((blk[0] >> (a & 63)) & 1u);
  const int mag = bitlevel == 2 && ((blk[1] >> (a & 63)) & 1u) ? 3 : 1;
  return s ? -mag : mag;
}

// one bag of W2B_EMBED_MAX_BAG + 1 padding ids: refused by its length alone, by both bag twins (once: 4 M ids)
void too_long_a_bag() {
  const int64_t n = (int64_t)W2B_EMBED_MAX_BAG + 1, rows = 3;
  const std::vector<uint64_t> p((size_t)rows, 0);
  const std::vector<int32_t> ids((size_t)n, -1);
  const std::vector<float> w((size_t)n, 1.f);
  const std::vector<int64_t> off = {0, n};
  std::vector<float> keep(1, 7.5f);
  refuse(g_bag, w2b_embed_bag_host(p.data(), rows, 1, 1, n, ids.data(), 1, off.data(), W2B_EMBED_MEAN, keep.data()), W2B_EINVAL,
         "longer than W2B_EMBED_MAX_BAG", keep);
  refuse(g_bagw, w2b_embed_bag_weighted_host(p.data(), rows, 1, 1, n, ids.data(), w.data(), 1, off.data(), W2B_EMBED_MEAN, keep.data()),
         W2B_EINVAL, "longer than W2B_EMBED_MAX_BAG", keep);
}
}  // namespace

int main() {
  const int64_t dims[] = {1, 65, 130}, rows = 37;
  const float inf = std::numeric_limits<float>::infinity();
  for (int bitlevel = 1; bitlevel <= 2; bitlevel++)
    for (int64_t dim : dims) {
      const int64_t wpr = (dim + 63) / 64 * bitlevel;
      std::vector<uint64_t> p((size_t)(rows * wpr));
      for (uint64_t &w : p) w = rnd();                    // the padding bits of the last block included: they must not count
      const float q = bitlevel == 1 ? 0.3333333432674407958984375f : 0.25f;

      // bags: ids with padding and repeats, an empty bag, padding only, a single id, and one of two segments (WSEG + 1 ids)
      std::vector<int32_t> ids = {3, -1, 3, 36, 0, -7, 36, 12, /* empty */ /* padding only */ -1, -1, -1, /* single */ 36};
      std::vector<int64_t> off = {0, 8, 8, 11, 12};
      for (int64_t i = 0; i < W2B_EMBED_WSEG + 1; i++) ids.push_back((int32_t)(rnd() % (uint64_t)(rows + 2)) - 2);
      off.push_back((int64_t)ids.size());
      const int64_t n = (int64_t)ids.size(), nb = (int64_t)off.size() - 1;
      std::vector<float> w((size_t)n);
      for (float &v : w) v = (float)((int64_t)(rnd() % 2001) - 1000) / 256.f;
      w[1] = std::nanf("");                               // the weight of a padding id is not looked at
      w[5] = inf;

      // lookup: the patterns of the table, +0.0 rows for padding, a repeated id repeats its row
      std::vector<float> rowsout((size_t)(n * dim), 7.5f);
      good(g_lookup, w2b_embed_lookup_host(p.data(), rows, dim, bitlevel, n, ids.data(), rowsout.data()), "call failed");
      for (int64_t i = 0; i < n; i++)
        for (int64_t a = 0; a < dim; a++) {
          const float want = ids[(size_t)i] < 0 ? 0.f : (float)code_of(p, wpr, bitlevel, ids[(size_t)i], a) * q;
          if (!same_bits(rowsout[(size_t)(i * dim + a)], want)) fail(g_lookup, "a row is the table's row, a padding row is +0.0");
        }

      // bags, unweighted and weighted, sum and mean, against the steps of the header
      for (int32_t mode : {W2B_EMBED_SUM, W2B_EMBED_MEAN}) {
        std::vector<float> bag((size_t)(nb * dim), 7.5f), bagw((size_t)(nb * dim), 7.5f);
        good(g_bag, w2b_embed_bag_host(p.data(), rows, dim, bitlevel, n, ids.data(), nb, off.data(), mode, bag.data()), "call failed");
        good(g_bagw, w2b_embed_bag_weighted_host(p.data(), rows, dim, bitlevel, n, ids.data(), w.data(), nb, off.data(), mode, bagw.data()),
             "call failed");
        for (int64_t b = 0; b < nb; b++)
          for (int64_t a = 0; a < dim; a++) {
            int32_t T = 0, m = 0;
            float S = 0.f;
            for (int64_t s0 = off[(size_t)b]; s0 < off[(size_t)b + 1]; s0 += W2B_EMBED_WSEG) {
              float P = 0.f;
              for (int64_t i = s0; i < s0 + W2B_EMBED_WSEG && i < off[(size_t)b + 1]; i++) {
                if (ids[(size_t)i] < 0) continue;
                const int code = code_of(p, wpr, bitlevel, ids[(size_t)i], a);
                T += code;
                m++;
                P = fmaf(w[(size_t)i], (float)code, P);
              }
              S = S + P;
            }
            const float sum = (float)T * q, sumw = S * q;
            const bool mean = mode == W2B_EMBED_MEAN;
            if (!same_bits(bag[(size_t)(b * dim + a)], mean ? (m > 0 ? sum / (float)m : 0.f) : sum)) fail(g_bag, "the steps of the header");
            if (!same_bits(bagw[(size_t)(b * dim + a)], mean ? (m > 0 ? sumw / (float)m : 0.f) : sumw))
              fail(g_bagw, "the steps of the header");
          }
        for (int64_t a = 0; a < dim; a++) {
          if (!same_bits(bag[(size_t)(dim + a)], 0.f) || !same_bits(bagw[(size_t)(dim + a)], 0.f)) fail(g_bag, "an empty bag is +0.0");
          if (!same_bits(bag[(size_t)(2 * dim + a)], 0.f) || !same_bits(bagw[(size_t)(2 * dim + a)], 0.f))
            fail(g_bag, "a bag of padding only is +0.0, as a mean too");
          if (!same_bits(bag[(size_t)(3 * dim + a)], rowsout[(size_t)(11 * dim + a)])) fail(g_bag, "a single id is its row");
        }
      }

      // empty calls: no ids (all bags empty), no bags, and nothing at all with NULL everywhere
      const std::vector<int64_t> zeros = {0, 0, 0};
      std::vector<float> two((size_t)(2 * dim), 7.5f);
      good(g_lookup, w2b_embed_lookup_host(p.data(), rows, dim, bitlevel, 0, nullptr, nullptr), "n == 0");
      good(g_bag, w2b_embed_bag_host(p.data(), rows, dim, bitlevel, 0, nullptr, 2, zeros.data(), W2B_EMBED_MEAN, two.data()), "n_ids == 0");
      for (float v : two)
        if (!same_bits(v, 0.f)) fail(g_bag, "bags without ids are +0.0");
      good(g_bagw, w2b_embed_bag_weighted_host(p.data(), rows, dim, bitlevel, 0, nullptr, nullptr, 2, zeros.data(), W2B_EMBED_SUM, two.data()),
           "n_ids == 0");
      good(g_bag, w2b_embed_bag_host(p.data(), rows, dim, bitlevel, 0, nullptr, 0, zeros.data(), W2B_EMBED_SUM, nullptr), "n_bags == 0");
      good(g_bag, w2b_embed_bag_host(p.data(), rows, dim, bitlevel, 0, nullptr, 0, nullptr, W2B_EMBED_SUM, nullptr), "n_bags == 0, no offsets");
      good(g_bagw, w2b_embed_bag_weighted_host(p.data(), rows, dim, bitlevel, 0, nullptr, nullptr, 0, zeros.data(), W2B_EMBED_SUM, nullptr),
           "n_bags == 0");
      good(g_lookup, w2b_embed_lookup_host(p.data(), 0, dim, bitlevel, 0, nullptr, nullptr), "rows == 0");

      // refusals, each function in the order of its checks: `out` keeps its 7.5
      const std::vector<int32_t> four = {1, 2, -1, 3};
      std::vector<int32_t> bad = four;
      bad[3] = (int32_t)rows;
      const std::vector<float> w4 = {0.5f, -2.f, std::nanf(""), 0.f};
      const std::vector<int64_t> o4 = {0, 2, 4};
      std::vector<float> keep((size_t)(4 * dim), 7.5f);
      struct Shape { int64_t rows, dim; int bitlevel; int code; const char *message; };
      const Shape shapes[] = {{-1, dim, bitlevel, W2B_EINVAL, "unsupported rows / dim"},
                              {0x7FFFFF01ll, dim, bitlevel, W2B_EINVAL, "unsupported rows / dim"},
                              {rows, 0, bitlevel, W2B_EINVAL, "unsupported rows / dim"},
                              {rows, (1 << 24) + 1, bitlevel, W2B_EINVAL, "unsupported rows / dim"},
                              {rows, dim, 0, W2B_EUNSUPPORTED, "bitlevel must be 1 or 2"},
                              {rows, dim, 3, W2B_EUNSUPPORTED, "bitlevel must be 1 or 2"}};

      auto lookup = [&](int64_t nn, const int32_t *ii, float *oo) { return w2b_embed_lookup_host(p.data(), rows, dim, bitlevel, nn, ii, oo); };
      refuse(g_lookup, w2b_embed_lookup_host(nullptr, rows, dim, bitlevel, 4, four.data(), keep.data()), W2B_EINVAL, "null table", keep);
      for (const Shape &s : shapes)
        refuse(g_lookup, w2b_embed_lookup_host(p.data(), s.rows, s.dim, s.bitlevel, 4, four.data(), keep.data()), s.code, s.message, keep);
      refuse(g_lookup, lookup(-1, four.data(), keep.data()), W2B_EINVAL, "negative id count", keep);
      refuse(g_lookup, lookup(4, nullptr, keep.data()), W2B_EINVAL, "null ids", keep);
      refuse(g_lookup, lookup(4, bad.data(), keep.data()), W2B_EINVAL, "ids[3]", keep);
      refuse(g_lookup, lookup(4, four.data(), nullptr), W2B_EINVAL, "null output", keep);

      // the bag twins share their checks up to the weights: the same calls through both
      for (int weighted = 0; weighted < 2; weighted++) {
        Count &c = weighted ? g_bagw : g_bag;
        auto bagt = [&](const uint64_t *pp, int64_t rr, int64_t dd, int bl, int64_t nn, const int32_t *ii, int64_t bb, const int64_t *ff,
                        int32_t mode, float *oo) {
          return weighted ? w2b_embed_bag_weighted_host(pp, rr, dd, bl, nn, ii, w4.data(), bb, ff, mode, oo)
                          : w2b_embed_bag_host(pp, rr, dd, bl, nn, ii, bb, ff, mode, oo);
        };
        auto call = [&](int64_t nn, const int32_t *ii, int64_t bb, const int64_t *ff, int32_t mode, float *oo) {
          return bagt(p.data(), rows, dim, bitlevel, nn, ii, bb, ff, mode, oo);
        };
        refuse(c, bagt(nullptr, rows, dim, bitlevel, 4, four.data(), 2, o4.data(), 0, keep.data()), W2B_EINVAL, "null table", keep);
        for (const Shape &s : shapes)
          refuse(c, bagt(p.data(), s.rows, s.dim, s.bitlevel, 4, four.data(), 2, o4.data(), 0, keep.data()), s.code, s.message, keep);
        refuse(c, call(-1, four.data(), 2, o4.data(), 0, keep.data()), W2B_EINVAL, "negative id count", keep);
        refuse(c, call(4, nullptr, 2, o4.data(), 0, keep.data()), W2B_EINVAL, "null ids", keep);
        refuse(c, call(4, bad.data(), 2, o4.data(), 0, keep.data()), W2B_EINVAL, "ids[3]", keep);
        refuse(c, call(4, four.data(), -1, o4.data(), 0, keep.data()), W2B_EINVAL, "bad bag count", keep);
        refuse(c, call(4, four.data(), 0x7FFFFF01ll, o4.data(), 0, keep.data()), W2B_EINVAL, "bad bag count", keep);
        refuse(c, call(4, four.data(), 2, o4.data(), 2, keep.data()), W2B_EINVAL, "mode is neither", keep);
        refuse(c, call(4, four.data(), 2, o4.data(), -1, keep.data()), W2B_EINVAL, "mode is neither", keep);
        refuse(c, call(4, four.data(), 2, nullptr, 0, keep.data()), W2B_EINVAL, "null offsets", keep);
        refuse(c, call(0, four.data(), 2, nullptr, 0, keep.data()), W2B_EINVAL, "null offsets", keep);
        const std::vector<int64_t> first = {1, 2, 4}, down = {0, 3, 2}, shortfall = {0, 2, 3};
        refuse(c, call(4, four.data(), 2, first.data(), 0, keep.data()), W2B_EINVAL, "offsets[0] is not 0", keep);
        refuse(c, call(4, four.data(), 2, down.data(), 0, keep.data()), W2B_EINVAL, "offsets decrease at bag 1", keep);
        refuse(c, call(4, four.data(), 2, shortfall.data(), 0, keep.data()), W2B_EINVAL, "offsets[n_bags] is not n_ids", keep);
        refuse(c, call(4, four.data(), 2, o4.data(), 0, nullptr), W2B_EINVAL, "null output", keep);
      }

      // the weights: NULL, and a weight on an id >= 0 that is not finite or out of range (w4 has its NaN on the padding id)
      auto callw = [&](const float *ww) {
        return w2b_embed_bag_weighted_host(p.data(), rows, dim, bitlevel, 4, four.data(), ww, 2, o4.data(), 0, keep.data());
      };
      refuse(g_bagw, callw(nullptr), W2B_EINVAL, "null weights", keep);
      for (float v : {std::nanf(""), inf, -inf, ldexpf(1.f, 61), -ldexpf(1.f, -61), 1e-45f}) {
        std::vector<float> y = w4;
        y[3] = v;
        refuse(g_bagw, callw(y.data()), W2B_EINVAL, "weights[3]", keep);
      }
      std::vector<float> edge = {ldexpf(1.f, 60), -ldexpf(1.f, -60), inf, -0.f};       // the bounds and zeros of either sign are fine
      std::vector<float> fine((size_t)(2 * dim), 7.5f);
      good(g_bagw, w2b_embed_bag_weighted_host(p.data(), rows, dim, bitlevel, 4, four.data(), edge.data(), 2, o4.data(), 0, fine.data()),
           "2^60, 2^-60 and -0 are allowed");
    }
  too_long_a_bag();
  for (const Count *c : {&g_lookup, &g_bag, &g_bagw}) printf("%s: %d calls ok, %d refused\n", c->name, c->ok, c->refused);
  return 0;
}
