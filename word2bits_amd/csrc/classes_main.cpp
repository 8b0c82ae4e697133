// classes_main.cpp -- word classes of a packed model, word2vec's `-classes` output:
//   ./classes <FILE> <K> [iters = 10] [threshold = 0] bits|codes
// FILE is a vectors file in the reference's binary format or a bit-packed .w2bp file, loaded exactly like ./nearest loads it in
// that mode.  The rows are clustered into K classes by spherical k-means on the MI355X (w2b_eval_classes: at most `iters`
// iterations from class = row % K, centroids = the normalised sums of their members, ties to the lowest class) and one line
// "<word> <class>" per row goes to stdout, in row order (w2b_eval_classes_text).  Nothing is read from stdin.
// "bits": 1-bit models; "codes": 2-bit models; the mode is the last argument, so `./classes FILE 500 bits` runs the defaults.
// `threshold` caps the rows as it does in ./compute_accuracy.
#include "../../include/word2bits_eval.h"
#include "../../include/word2bits_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv) {
  const char *mode = argc > 3 && argc <= 6 ? argv[argc - 1] : nullptr;   // the last argument; iters and threshold may be left out
  const bool bits = mode && !strcmp(mode, "bits"), codes = mode && !strcmp(mode, "codes");
  if (argc < 3 || !(bits || codes)) {
    printf("Usage: ./classes <FILE> <K> [iters = 10] [threshold = 0] bits|codes\nwhere FILE contains word projections; prints "
           "one line \"<word> <class>\" per row: K classes by k-means on the bit-packed rows, 1 <= K <= %d, at most `iters` "
           "iterations; bits = 1-bit models, codes = 2-bit models\n",
           W2B_EVAL_MAX_CLASSES);
    return argc < 2 ? 0 : 2;
  }
  const int k = atoi(argv[2]);
  const int iters = argc > 4 ? atoi(argv[3]) : 10;
  const long long threshold = argc > 5 ? atoll(argv[4]) : 0;
  int device = 0;
  if (const char *env = getenv("W2B_DEVICE")) device = atoi(env);
  w2b_eval *e = nullptr;
  const int rc = bits ? w2b_eval_load_bits(argv[1], threshold, device, &e) : w2b_eval_load_codes(argv[1], threshold, device, &e);
  if (rc == W2B_EIO && !strcmp(w2b_last_error(), "Input file not found")) {
    printf("Input file not found\n");
    return -1;
  }
  if (rc != W2B_OK) {
    fprintf(stderr, "classes: %s\n", w2b_last_error());
    return 1;
  }
  char *txt = nullptr;
  int64_t len = 0;
  if (w2b_eval_classes_text(e, k, iters, &txt, &len) != W2B_OK) {
    fprintf(stderr, "classes: %s\n", w2b_last_error());
    w2b_eval_free(e);
    return 1;
  }
  fwrite(txt, 1, (size_t)len, stdout);
  w2b_eval_free_text(txt);
  w2b_eval_free(e);
  return 0;
}
