// eval_twins_main.cpp -- the evaluator's host twins (word2bits_amd/csrc/w2b_eval_twins.cpp) at the edge shapes of the packing,
// as a program of its own for the host sanitizers: `make -C word2bits_amd/csrc host-check` builds it with
// -fsanitize=address,undefined from this file and w2b_eval_twins.cpp alone (no library, no HIP, no GPU) and runs it.  Every
// input and output buffer has exactly the size the header promises, so a read or a write past it is a report.  What the
// twins compute is the business of tests/test_eval_*_host.py; here only a few identities that cost nothing are checked.
// Prints one line per twin and exits 0; a call that fails, or a refusal that does not come, is exit 1.
#include "../../include/word2bits_eval.h"
#include "../../include/word2bits_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static std::string g_error;
int w2b_internal_fail(int code, const char *msg) {   // the library's is in w2b_trainer.cpp
  g_error = msg ? msg : "";
  return code;
}

namespace {
const int64_t kDims[] = {1, 63, 64, 65, 129};
const int64_t kWords[] = {1, 3};
const int64_t kLengths[] = {0, 1, 2, 65};

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {   // xorshift64
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

// [words][bitlevel * ceil(dim / 64)] random words, the padding bits of the last block included: they must not count
std::vector<uint64_t> model(int64_t words, int64_t dim, int bitlevel) {
  std::vector<uint64_t> p((size_t)(words * ((dim + 63) / 64) * bitlevel));
  for (uint64_t &w : p) w = rnd();
  return p;
}

// n ids in [0, words), every fifth one padding (-1)
std::vector<int32_t> some_ids(int64_t n, int64_t words) {
  std::vector<int32_t> ids((size_t)n);
  for (int64_t i = 0; i < n; i++) ids[(size_t)i] = i % 5 == 4 ? -1 : (int32_t)(rnd() % (uint64_t)words);
  return ids;
}

struct Tally {
  const char *name;
  int ok = 0, refused = 0;
  void good(int rc) {
    if (rc != W2B_OK) {
      printf("%s: call %d failed with %d: %s\n", name, ok + 1, rc, g_error.c_str());
      exit(1);
    }
    ok++;
  }
  void check(bool holds, const char *what) {
    if (!holds) {
      printf("%s: %s does not hold\n", name, what);
      exit(1);
    }
  }
  void refuse(int rc, const char *message) {
    if (rc != W2B_EINVAL || g_error.find(message) == std::string::npos) {
      printf("%s: expected a refusal with \"%s\", got %d: %s\n", name, message, rc, g_error.c_str());
      exit(1);
    }
    refused++;
  }
  ~Tally() { printf("%s: %d calls ok, %d refused\n", name, ok, refused); }
};

void bits_scores() {
  Tally t{"w2b_bits_scores_host"};
  for (int64_t dim : kDims)
    for (int64_t words : kWords) {
      const std::vector<uint64_t> p = model(words, dim, 1);
      std::vector<int32_t> I((size_t)words);
      t.good(w2b_bits_scores_host(p.data(), words, dim, 0, words - 1, words / 2, I.data()));
      t.good(w2b_bits_scores_host(p.data(), words, dim, 0, 0, 0, I.data()));
      t.check(I[0] == dim, "I(b, b) == dim");
      t.refuse(w2b_bits_scores_host(p.data(), words, dim, 0, words, 0, I.data()), "bad argument");
    }
}

void bits_combine() {
  Tally t{"w2b_bits_combine_scores_host"};
  for (int64_t dim : kDims)
    for (int64_t words : kWords) {
      const std::vector<uint64_t> p = model(words, dim, 1);
      std::vector<int32_t> I((size_t)words);
      for (int32_t nt : {1, W2B_EVAL_MAX_TERMS}) {
        std::vector<int32_t> rows((size_t)nt);
        std::vector<int8_t> signs((size_t)nt);
        for (int32_t i = 0; i < nt; i++) rows[(size_t)i] = (int32_t)(i % words), signs[(size_t)i] = (int8_t)(i % 3 == 1 ? -1 : i % 3 == 2 ? 0 : 1);
        t.good(w2b_bits_combine_scores_host(p.data(), words, dim, nt, rows.data(), signs.data(), I.data()));
        if (nt == 1) t.check(I[0] == dim, "I(b, b) == dim");
        rows[0] = (int32_t)words;
        t.refuse(w2b_bits_combine_scores_host(p.data(), words, dim, nt, rows.data(), signs.data(), I.data()),
                 "question row out of range");
      }
    }
}

void codes_scores() {
  Tally t{"w2b_codes_scores_host"};
  for (int64_t dim : kDims)
    for (int64_t words : kWords) {
      const std::vector<uint64_t> p = model(words, dim, 2);
      std::vector<int32_t> J((size_t)(3 * words));
      std::vector<float> s((size_t)words);
      t.good(w2b_codes_scores_host(p.data(), words, dim, 0, words - 1, words / 2, J.data(), s.data()));
      t.good(w2b_codes_scores_host(p.data(), words, dim, 0, 0, 0, nullptr, s.data()));
      t.good(w2b_codes_scores_host(p.data(), words, dim, 0, 0, 0, J.data(), nullptr));
      t.check(J[0] >= dim && J[0] <= 9 * dim, "dim <= J(b, b) <= 9 dim");
      t.refuse(w2b_codes_scores_host(nullptr, words, dim, 0, 0, 0, J.data(), s.data()), "bad argument");
    }
}

void cosmul_scores() {
  Tally t{"w2b_cosmul_scores_host"};
  for (int bitlevel : {1, 2})
    for (int64_t dim : kDims)
      for (int64_t words : kWords) {
        const std::vector<uint64_t> p = model(words, dim, bitlevel);
        std::vector<float> u((size_t)(3 * words)), s((size_t)words);
        t.good(w2b_cosmul_scores_host(p.data(), words, dim, bitlevel, 0, words - 1, words / 2, u.data(), s.data()));
        t.good(w2b_cosmul_scores_host(p.data(), words, dim, bitlevel, 0, 0, 0, nullptr, s.data()));
        for (float x : u) t.check(x >= 0.f && x <= 1.0001f, "0 <= u <= 1");
        t.refuse(w2b_cosmul_scores_host(p.data(), words, dim, bitlevel, 0, -1, 0, u.data(), s.data()),
                 "question row out of range");
      }
}

void bag_scores() {
  Tally t{"w2b_bag_scores_host"};
  for (int bitlevel : {1, 2})
    for (int64_t dim : kDims)
      for (int64_t words : kWords) {
        const std::vector<uint64_t> p = model(words, dim, bitlevel);
        std::vector<int32_t> J((size_t)words);
        std::vector<float> s((size_t)words);
        for (int64_t n : kLengths) {
          std::vector<int32_t> ids = some_ids(n, words);
          t.good(w2b_bag_scores_host(p.data(), words, dim, bitlevel, n, n ? ids.data() : nullptr, J.data(), s.data()));
          if (n == 0) t.check(J[0] == 0 && s[0] == 0.f, "an empty bag scores 0");
          if (n == 0) continue;
          ids[(size_t)(n - 1)] = (int32_t)words;
          t.refuse(w2b_bag_scores_host(p.data(), words, dim, bitlevel, n, ids.data(), J.data(), s.data()), "bag id out of range");
        }
      }
}

void vector_scores() {
  Tally t{"w2b_vector_scores_host"};
  for (int bitlevel : {1, 2})
    for (int64_t dim : kDims)
      for (int64_t words : kWords) {
        const std::vector<uint64_t> p = model(words, dim, bitlevel);
        std::vector<float> x((size_t)dim), S((size_t)words), s((size_t)words);
        for (float &v : x) v = (float)((int64_t)(rnd() % 2001) - 1000) / 256.f;
        for (int normalize : {0, 1}) t.good(w2b_vector_scores_host(p.data(), words, dim, bitlevel, x.data(), normalize, S.data(), s.data()));
        t.good(w2b_vector_scores_host(p.data(), words, dim, bitlevel, x.data(), 1, nullptr, s.data()));
        for (float v : s) t.check(std::fabs(v) <= 1.0001f, "|cosine| <= 1");
        x[(size_t)(dim - 1)] = NAN;
        t.refuse(w2b_vector_scores_host(p.data(), words, dim, bitlevel, x.data(), 1, S.data(), s.data()), "a value must be finite");
      }
}

void docs_scores() {
  Tally t{"w2b_docs_scores_host"};
  for (int bitlevel : {1, 2})
    for (int64_t dim : kDims)
      for (int64_t words : kWords) {
        const std::vector<uint64_t> p = model(words, dim, bitlevel);
        std::vector<int32_t> ids;
        std::vector<int64_t> off(1, 0);
        for (int64_t n : kLengths) {   // one document of every length
          const std::vector<int32_t> d = some_ids(n, words);
          ids.insert(ids.end(), d.begin(), d.end());
          off.push_back((int64_t)ids.size());
        }
        const int64_t n_docs = (int64_t)off.size() - 1;
        std::vector<int64_t> dir((size_t)(2 * n_docs));
        std::vector<float> s((size_t)n_docs);
        for (int64_t nq : kLengths) {
          std::vector<int32_t> q = some_ids(nq, words);
          for (int symmetric : {0, 1})
            t.good(w2b_docs_scores_host(p.data(), words, dim, bitlevel, (int64_t)ids.size(), ids.data(), n_docs, off.data(), nq,
                                        nq ? q.data() : nullptr, symmetric, dir.data(), s.data()));
          t.check(s[0] == 0.f, "an empty document scores 0");
          if (nq == 0) continue;
          q[0] = (int32_t)words;
          t.refuse(w2b_docs_scores_host(p.data(), words, dim, bitlevel, (int64_t)ids.size(), ids.data(), n_docs, off.data(), nq,
                                        q.data(), 1, dir.data(), s.data()),
                   "query id out of range");
        }
        t.good(w2b_docs_scores_host(p.data(), words, dim, bitlevel, 0, nullptr, 0, nullptr, 0, nullptr, 1, nullptr, nullptr));
      }
}

void pairs() {
  Tally t{"w2b_pairs_host"};
  for (int bitlevel : {1, 2})
    for (int64_t dim : kDims)
      for (int64_t words : kWords) {
        const std::vector<uint64_t> p = model(words, dim, bitlevel);
        std::vector<int32_t> ids;
        std::vector<int64_t> off(1, 0);
        for (int64_t na : kLengths)     // every length against every length
          for (int64_t nb : kLengths)
            for (int64_t n : {na, nb}) {
              const std::vector<int32_t> side = some_ids(n, words);
              ids.insert(ids.end(), side.begin(), side.end());
              off.push_back((int64_t)ids.size());
            }
        const int64_t np = ((int64_t)off.size() - 1) / 2;
        std::vector<float> s((size_t)np);
        std::vector<int64_t> parts((size_t)(3 * np));
        t.good(w2b_pairs_host(p.data(), words, dim, bitlevel, (int64_t)ids.size(), ids.data(), np, off.data(), s.data(), parts.data()));
        t.good(w2b_pairs_host(p.data(), words, dim, bitlevel, (int64_t)ids.size(), ids.data(), np, off.data(), s.data(), nullptr));
        t.good(w2b_pairs_host(p.data(), words, dim, bitlevel, (int64_t)ids.size(), ids.data(), np, off.data(), nullptr, parts.data()));
        t.check(s[0] == 0.f && parts[1] == 0, "an empty pair scores 0");
        for (float v : s) t.check(std::fabs(v) <= 1.0001f, "|cosine| <= 1");
        ids.back() = (int32_t)words;
        t.refuse(w2b_pairs_host(p.data(), words, dim, bitlevel, (int64_t)ids.size(), ids.data(), np, off.data(), s.data(), parts.data()),
                 "id out of range");
        t.good(w2b_pairs_host(p.data(), words, dim, bitlevel, 0, nullptr, 0, nullptr, nullptr, nullptr));
      }
}

void classes() {
  Tally t{"w2b_classes_host"};
  for (int bitlevel : {1, 2})
    for (int64_t dim : kDims)
      for (int64_t words : kWords) {
        const std::vector<uint64_t> p = model(words, dim, bitlevel);
        for (int32_t K : {1, 2}) {
          std::vector<int32_t> cls((size_t)words), T((size_t)(K * dim));
          std::vector<float> score((size_t)words);
          std::vector<int64_t> counts((size_t)K);
          int32_t iters = -1;
          int64_t moved = -1;
          if (K > words) {
            t.refuse(w2b_classes_host(p.data(), words, dim, bitlevel, K, 2, nullptr, cls.data(), score.data(), T.data(), counts.data(),
                                      &iters, &moved),
                     "n_classes must be at most min(words, 16384)");
            continue;
          }
          t.good(w2b_classes_host(p.data(), words, dim, bitlevel, K, 2, nullptr, cls.data(), score.data(), T.data(), counts.data(),
                                  &iters, &moved));
          int64_t members = 0;
          for (int64_t c : counts) members += c;
          t.check(members == words && iters >= 1 && iters <= 2, "the counts add up to words, 1 <= iters_run <= 2");
          const std::vector<int32_t> init((size_t)words, K - 1);
          t.good(w2b_classes_host(p.data(), words, dim, bitlevel, K, 2, init.data(), cls.data(), nullptr, nullptr, nullptr, nullptr, nullptr));
          t.refuse(w2b_classes_host(p.data(), words, dim, bitlevel, K, 2, nullptr, nullptr, score.data(), T.data(), counts.data(),
                                    &iters, &moved),
                   "bad argument");
        }
      }
}

void rank_correlation() {
  Tally t{"w2b_rank_correlation"};
  double pearson = 0, spearman = 0;
  const double x2[] = {1.0, 2.0}, y2[] = {5.0, 3.0};
  t.good(w2b_rank_correlation(2, x2, y2, &pearson, &spearman));
  t.check(pearson == -1.0 && spearman == -1.0, "two points the other way round: r == -1");
  const double x5[] = {1.0, 2.0, 2.0, 4.0, 5.0}, y5[] = {1.5, 3.0, 3.0, 3.0, 9.0};   // ties on both sides
  t.good(w2b_rank_correlation(5, x5, y5, &pearson, &spearman));
  t.check(pearson > 0.5 && pearson <= 1.0 && spearman > 0.5 && spearman <= 1.0, "0.5 < r <= 1");
  const double same[] = {2.0, 2.0, 2.0, 2.0, 2.0};
  t.good(w2b_rank_correlation(5, x5, same, &pearson, &spearman));
  t.check(std::isnan(pearson) && std::isnan(spearman), "a constant has no correlation");
  t.good(w2b_rank_correlation(5, x5, y5, nullptr, nullptr));
  t.refuse(w2b_rank_correlation(2, nullptr, y2, &pearson, &spearman), "bad argument");
}
}  // namespace

int main() {
  bits_scores();
  bits_combine();
  codes_scores();
  cosmul_scores();
  bag_scores();
  vector_scores();
  docs_scores();
  pairs();
  classes();
  rank_correlation();
  return 0;
}
