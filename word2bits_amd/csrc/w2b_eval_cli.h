// w2b_eval_cli.h -- what ./compute_accuracy and ./nearest do once their own positional arguments are read: load the
// vectors file, hand all of stdin to one text query of include/word2bits_eval.h, print what it returns.
#pragma once
#include "../../include/word2bits_eval.h"
#include "../../include/word2bits_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

// `mode` is the optional fma|nofma|bits|codes argument (null when absent); `text(e, in, len, &txt, &txt_len)` is the query.
// What the reference prints goes to stdout, what these programs add goes to stderr under `prog`.
template <class Text>
static int w2b_eval_cli(const char *prog, const char *file, int bitlevel, long long threshold, const char *mode, Text text) {
  int fused = 1;
  if (const char *env = getenv("W2B_EVAL_FUSED")) fused = atoi(env) != 0;
  if (mode) fused = strcmp(mode, "nofma") != 0;
  int device = 0;
  if (const char *env = getenv("W2B_DEVICE")) device = atoi(env);

  w2b_eval *e = nullptr;
  const bool bits = mode && !strcmp(mode, "bits"), codes = mode && !strcmp(mode, "codes");
  const int rc = bits    ? w2b_eval_load_bits(file, threshold, device, &e)
                 : codes ? w2b_eval_load_codes(file, threshold, device, &e)
                         : w2b_eval_load(file, bitlevel, threshold, fused, device, &e);
  if (rc == W2B_EIO && !strcmp(w2b_last_error(), "Input file not found")) {
    printf("Input file not found\n");                          // ref :81-84
    return -1;
  }
  if (rc != W2B_OK) {
    fprintf(stderr, "%s: %s\n", prog, w2b_last_error());
    return 1;
  }
  std::string in;
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, stdin)) > 0) in.append(buf, n);
  char *txt = nullptr;
  int64_t len = 0;
  if (text(e, in.data(), (int64_t)in.size(), &txt, &len) != W2B_OK) {
    fprintf(stderr, "%s: %s\n", prog, w2b_last_error());
    return 1;
  }
  fwrite(txt, 1, (size_t)len, stdout);
  w2b_eval_free_text(txt);
  w2b_eval_free(e);
  return 0;
}
