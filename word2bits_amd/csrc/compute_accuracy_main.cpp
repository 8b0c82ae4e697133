// compute_accuracy_main.cpp -- drop-in for the reference's evaluator program (ref src/compute-accuracy.c:63-189):
//   ./compute_accuracy <FILE> <bitlevel> <threshold> [fma|nofma|bits|codes] [cosmul|rank] < questions-words.txt
// Same positional arguments, same stdout.  The scan runs on the MI355X through include/word2bits_eval.h.
// The optional 4th argument (or W2B_EVAL_FUSED=0|1) selects which build of the reference the scores are
// bit-identical to: "fma" (default; the reference's own Makefile flags on an FMA-capable host) or "nofma"
// (-ffp-contract=off).  The reference ignores a 4th argument, so scripts can pass it to both.
// "bits" (1-bit models only; <bitlevel> is ignored) keeps the rows bit-packed and answers by the exact integer score
// with ties to the lowest row (include/word2bits_eval.h, "bits mode"); the transcript keeps the reference's format.
// "codes" (2-bit models only; <bitlevel> is ignored) does the same for 2-bit rows: exact integer dot products on the packed
// rows, scaled by the rows' lengths in a fixed float sequence ("codes mode").
// "cosmul" as a 5th argument (after bits or codes) answers every question by the multiplicative rule 3CosMul instead of the
// additive one (w2b_eval_transcript_cosmul); the transcript keeps the reference's format.
// "rank" as a 5th argument (after bits or codes) keeps the transcript and adds, after every "Total accuracy" line, two lines
// that begin with RANKS: the mean reciprocal rank, hits@1 / 5 / 10 and the unranked count of the expected answers
// (w2b_eval_transcript_rank).
#include "w2b_eval_cli.h"

int main(int argc, char **argv) {
  if (argc < 2) {   // ref :73-76
    printf("Usage: ./compute-accuracy <FILE> <bitlevel> <threshold>\nwhere FILE contains word projections, and "
           "threshold is used to reduce vocabulary of the model for fast approximate evaluation (0 = off, "
           "otherwise typical value is 30000)\n");
    // (stdout is the reference's, byte for byte; what this program adds goes to stderr)
    fprintf(stderr, "Optional 4th argument: fma (default) | nofma = the build of the reference whose arithmetic is "
                    "reproduced; bits = 1-bit models only: exact integer scores on the bit-packed rows, ties to the lowest "
                    "row (<bitlevel> is ignored); codes = 2-bit models only: exact integer dot products on the bit-packed "
                    "rows, scaled by the rows' lengths (<bitlevel> is ignored).  Optional 5th argument (after bits or codes): cosmul "
                    "= every question is answered by the multiplicative rule 3CosMul instead of the additive one; rank = two lines that "
                    "begin with RANKS after every Total accuracy line: mean reciprocal rank, hits@1 / 5 / 10 and the unranked count "
                    "of the expected answers\n");
    return 0;
  }
  const int bitlevel = argc > 2 ? atoi(argv[2]) : 0;          // ref :78
  const long long threshold = argc > 3 ? atoi(argv[3]) : 0;   // ref :79
  const bool is_cosmul = argc > 5 && !strcmp(argv[5], "cosmul"), is_rank = argc > 5 && !strcmp(argv[5], "rank");
  return w2b_eval_cli("compute_accuracy", argv[1], bitlevel, threshold, argc > 4 ? argv[4] : nullptr,
                      is_cosmul ? w2b_eval_transcript_cosmul : is_rank ? w2b_eval_transcript_rank : w2b_eval_transcript);
}
