// similarity_main.cpp -- word and sentence pair similarity of a packed model, and its correlation with human scores:
//   ./similarity <FILE> [threshold = 0] bits|codes [summary] < pairs.tsv
// FILE is a vectors file in the reference's binary format or a bit-packed .w2bp file, loaded exactly like ./nearest loads it in
// that mode.  Every input line that is not empty and does not start with '#' is one rated pair "A <tab> B <tab> gold" (or three
// blank-separated fields when the line has no tab: word, word, gold), A and B being one word or a sentence of up to 4096 words;
// WordSim-353, SimLex, MEN and the STS sets come in this form.  All pairs are scored in one batch on the MI355X
// (w2b_eval_pairs_text): the cosine of the two pooled integer vectors, one line per pair, then the counts and Pearson's and
// Spearman's correlation of the scores with the gold column.  `summary` prints the four summary lines alone.
// "bits": 1-bit models; "codes": 2-bit models.  `threshold` caps the rows as it does in ./compute_accuracy.
#include "w2b_eval_cli.h"

static bool is_mode(const char *s) { return !strcmp(s, "bits") || !strcmp(s, "codes"); }

int main(int argc, char **argv) {
  const int mi = argc > 2 && is_mode(argv[2]) ? 2 : 3;          // the mode follows FILE or the threshold
  const bool summary = argc == mi + 2 && !strcmp(argv[mi + 1], "summary");
  if (argc <= mi || !is_mode(argv[mi]) || argc > mi + 2 || (argc == mi + 2 && !summary)) {
    printf("Usage: ./similarity <FILE> [threshold = 0] bits|codes [summary] < pairs.tsv\nwhere FILE contains word projections and "
           "every input line is one rated pair: A <tab> B <tab> gold, A and B one word or a sentence of up to %d words (without a "
           "tab: three blank-separated fields); lines that are empty or start with # are skipped; prints \"<score> <gold> <A> <B>\" "
           "per pair, tab-separated, then the counts and the Pearson and Spearman correlation of the scores with the gold column; "
           "summary = those last four lines alone; bits = 1-bit models, codes = 2-bit models\n",
           W2B_EVAL_MAX_BAG);
    return argc < 2 ? 0 : 2;
  }
  const long long threshold = mi == 3 ? atoll(argv[2]) : 0;
  const int details = summary ? 0 : 1;
  return w2b_eval_cli("similarity", argv[1], 0, threshold, argv[mi],
                      [details](w2b_eval *e, const char *in, int64_t len, char **txt, int64_t *txt_len) {
                        return w2b_eval_pairs_text(e, in, len, details, txt, txt_len);
                      });
}
