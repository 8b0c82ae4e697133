// rank_twin_main.cpp -- the host twin of the rank question (w2b_rank_host, word2bits_amd/csrc/w2b_eval_twins.cpp) as a
// program of its own for the host sanitizers: `make -C word2bits_amd/csrc host-check` builds it with
// -fsanitize=address,undefined from this file and w2b_eval_twins.cpp alone (no library, no HIP, no GPU) and runs it.  Every
// buffer has exactly the size the header promises, so a read or a write past it is a report.  What the twin computes is the
// business of tests/test_eval_rank_host.py; here: a good path per bitlevel at sizes with a partial last word, the identity
// that one question with every row as target gives 1..m once each, the refusals, and NULL tied / score.
// Prints one line and exits 0; a call that fails, or a refusal that does not come, is exit 1.
#include "../../include/word2bits_eval.h"
#include "../../include/word2bits_hip.h"

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
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {   // xorshift64
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

int g_ok = 0, g_refused = 0;

void fail(const char *what) {
  printf("w2b_rank_host: %s: %s\n", what, g_error.c_str());
  exit(1);
}

void refuse(int rc, const char *message, const int32_t *r, const int32_t *t, const float *s) {
  if (rc != W2B_EINVAL || g_error.find(message) == std::string::npos) fail(message);
  if (*r != 77 || *t != 77 || *s != 7.5f) fail("a refused call wrote an output");
  g_refused++;
}
}  // namespace

int main() {
  const int64_t dims[] = {1, 63, 65, 129}, words = 37;
  for (int bitlevel = 1; bitlevel <= 2; bitlevel++)
    for (int64_t dim : dims) {
      // random words, the padding bits of the last block included (they must not count), and a block of identical rows
      std::vector<uint64_t> p((size_t)(words * ((dim + 63) / 64) * bitlevel));
      for (uint64_t &w : p) w = rnd();
      const size_t wpr = p.size() / (size_t)words;
      for (int64_t r = 11; r < 15; r++)
        for (size_t w = 0; w < wpr; w++) p[(size_t)r * wpr + w] = p[10 * wpr + w];
      const int64_t b1 = 3, b2 = 10, b3 = 20;
      std::vector<int> seen((size_t)words + 1, 0);
      int64_t m = 0;
      for (int64_t g = 0; g < words; g++) {
        int32_t rank = 77, tied = 77, only = 77;
        float score = 7.5f;
        if (w2b_rank_host(p.data(), words, dim, bitlevel, b1, b2, b3, g, &rank, &tied, &score) != W2B_OK) fail("call failed");
        if (w2b_rank_host(p.data(), words, dim, bitlevel, b1, b2, b3, g, &only, nullptr, nullptr) != W2B_OK) fail("NULL tied / score");
        g_ok += 2;
        if (only != rank || rank < 0 || rank > words) fail("rank with and without tied / score");
        if ((rank == 0) != (score == 0.f) || (rank == 0 && tied != 0) || score < 0.f) fail("rank 0 <=> score 0, tied 0");
        if ((g == b1 || g == b2 || g == b3) && rank != 0) fail("an own row has no rank");
        if (rank > 0) {
          seen[(size_t)rank]++;
          m++;
        }
      }
      for (int64_t r = 1; r <= words; r++)
        if (seen[(size_t)r] != (r <= m ? 1 : 0)) fail("every rank 1..m exactly once");
      int32_t r = 77, t = 77;
      float s = 7.5f;
      refuse(w2b_rank_host(p.data(), words, dim, 0, b1, b2, b3, 5, &r, &t, &s), "bitlevel must be 1 or 2", &r, &t, &s);
      refuse(w2b_rank_host(p.data(), words, dim, 3, b1, b2, b3, 5, &r, &t, &s), "bitlevel must be 1 or 2", &r, &t, &s);
      for (int pos = 0; pos < 4; pos++)
        for (int64_t bad : {(int64_t)-1, words}) {
          int64_t rows[4] = {b1, b2, b3, 5};
          rows[pos] = bad;
          refuse(w2b_rank_host(p.data(), words, dim, bitlevel, rows[0], rows[1], rows[2], rows[3], &r, &t, &s), "row out of range", &r,
                 &t, &s);
        }
      refuse(w2b_rank_host(p.data(), words, dim, bitlevel, b1, b2, b3, 5, nullptr, &t, &s), "bad argument", &r, &t, &s);
    }
  printf("w2b_rank_host: %d calls ok, %d refused\n", g_ok, g_refused);
  return 0;
}
