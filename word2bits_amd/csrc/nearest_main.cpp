// nearest_main.cpp -- what is near a word, and the best few answers to an analogy:
//   ./nearest <FILE> <k> [bitlevel] [threshold] [fma|nofma|bits] < queries
// FILE is a vectors file in the reference's binary format or a bit-packed .w2bp file, loaded exactly like
// ./compute_accuracy loads it (ref src/compute-accuracy.c:80-112).  One query per input line: one word = its k
// nearest words, three words A B C = the k best answers to "A is to B as C is to ?" (ref :155-177 with N = k).
// All lines are scored in one batch on the MI355X; the output format is that of w2b_eval_nearest_text.
// "bits" (1-bit models only; bitlevel is ignored): exact integer scores on the bit-packed rows, ties to the lowest row.
#include "../../include/word2bits_eval.h"
#include "../../include/word2bits_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

int main(int argc, char **argv) {
  if (argc < 2) {
    printf("Usage: ./nearest <FILE> <k> [bitlevel] [threshold] [fma|nofma|bits] < queries\nwhere FILE contains word "
           "projections and every input line is one word (its k nearest words) or three words A B C (the k best "
           "answers to A : B = C : ?); 1 <= k <= %d; bits = 1-bit models only: exact integer scores on the bit-packed "
           "rows, ties to the lowest row (bitlevel is ignored)\n", W2B_EVAL_MAX_K);
    return 0;
  }
  const int k = argc > 2 ? atoi(argv[2]) : 10;
  if (k < 1 || k > W2B_EVAL_MAX_K) {
    fprintf(stderr, "nearest: k must be 1..%d\n", W2B_EVAL_MAX_K);
    return 2;
  }
  const int bitlevel = argc > 3 ? atoi(argv[3]) : 0;
  const long long threshold = argc > 4 ? atoi(argv[4]) : 0;
  int fused = 1;
  if (const char *env = getenv("W2B_EVAL_FUSED")) fused = atoi(env) != 0;
  if (argc > 5) fused = strcmp(argv[5], "nofma") != 0;
  int device = 0;
  if (const char *env = getenv("W2B_DEVICE")) device = atoi(env);

  w2b_eval *e = nullptr;
  const bool bits = argc > 5 && !strcmp(argv[5], "bits");
  const int rc = bits ? w2b_eval_load_bits(argv[1], threshold, device, &e)
                      : w2b_eval_load(argv[1], bitlevel, threshold, fused, device, &e);
  if (rc == W2B_EIO && !strcmp(w2b_last_error(), "Input file not found")) {
    printf("Input file not found\n");
    return -1;
  }
  if (rc != W2B_OK) {
    fprintf(stderr, "nearest: %s\n", w2b_last_error());
    return 1;
  }
  std::string in;
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, stdin)) > 0) in.append(buf, n);
  char *txt = nullptr;
  int64_t len = 0;
  if (w2b_eval_nearest_text(e, in.data(), (int64_t)in.size(), k, &txt, &len) != W2B_OK) {
    fprintf(stderr, "nearest: %s\n", w2b_last_error());
    return 1;
  }
  fwrite(txt, 1, (size_t)len, stdout);
  w2b_eval_free_text(txt);
  w2b_eval_free(e);
  return 0;
}
