// nearest_main.cpp -- what is near a word, and the best few answers to an analogy:
//   ./nearest <FILE> <k> [bitlevel] [threshold] [fma|nofma|bits|codes] [signed|bag|vector|cosmul|rank|docs CORPUS.txt [oneway]] < queries
// FILE is a vectors file in the reference's binary format or a bit-packed .w2bp file, loaded exactly like
// ./compute_accuracy loads it (ref src/compute-accuracy.c:80-112).  One query per input line: one word = its k
// nearest words, three words A B C = the k best answers to "A is to B as C is to ?" (ref :155-177 with N = k).
// All lines are scored in one batch on the MI355X; the output format is that of w2b_eval_nearest_text.
// "bits" (1-bit models only; bitlevel is ignored): exact integer scores on the bit-packed rows, ties to the lowest row.
// "codes" (2-bit models only; bitlevel is ignored): exact integer dot products on the bit-packed rows, scaled by the rows' lengths.
// "signed" (after the mode; not with codes): every line is 1 to 7 tokens +WORD, -WORD or WORD, a bare word counting as +,
// and is answered with the k rows nearest to that signed sum (w2b_eval_combine_text): "new york", "+king -man +woman".
// "bag" (after the mode; bits and codes only): every line is one bag of 1 to 4096 words and is answered with the k rows
// nearest to their unnormalised sum, the line's own words excluded (w2b_eval_bag_text): a sentence, a ten-word phrase.
// "vector" (after the mode; every mode): every line is `size` numbers, a float vector of the model's width, and is answered
// with the k rows nearest to it by cosine, nothing excluded (w2b_eval_vectors_text with normalize = 1).
// "cosmul" (after the mode; bits and codes only): every line is three words A B C and is answered with the k best answers
// to "A is to B as C is to ?" by the multiplicative rule 3CosMul (w2b_eval_cosmul_text).
// "rank" (after the mode; bits and codes only; k is parsed and ignored): every line is two words A G, the place of G among
// the neighbours of A, or four words A B C G, the place of G as the answer to "A is to B as C is to ?", however far down the
// complete answer list: rank, rows tied with it, score (w2b_eval_rank_text).
// "docs CORPUS.txt [oneway]" (after the mode; bits and codes only): every line of CORPUS.txt is one document, every input line
// one query text, answered with the line numbers of the k documents nearest to it by relaxed word mover's similarity
// (w2b_eval_docs_set_text, w2b_eval_docs_text); words outside the vocabulary are dropped, their number in the corpus is noted
// on stderr; oneway scores how well the query's words are matched in a document alone (symmetric = 0).
#include "w2b_eval_cli.h"

int main(int argc, char **argv) {
  if (argc < 2) {
    printf("Usage: ./nearest <FILE> <k> [bitlevel] [threshold] [fma|nofma|bits|codes] [signed|bag|vector|cosmul|rank|docs CORPUS.txt [oneway]] < queries\nwhere FILE contains word "
           "projections and every input line is one word (its k nearest words) or three words A B C (the k best "
           "answers to A : B = C : ?); 1 <= k <= %d; bits = 1-bit models only: exact integer scores on the bit-packed "
           "rows, ties to the lowest row (bitlevel is ignored); codes = 2-bit models only: exact integer dot products on "
           "the bit-packed rows, scaled by the rows' lengths (bitlevel is ignored); signed (after the mode, not with codes) = every "
           "input line is 1 to %d words, each with an optional + or - in front: the k rows nearest to that signed sum; bag (after "
           "the mode, bits and codes only) = every input line is one bag of 1 to %d words: the k rows nearest to their sum, the "
           "line's own words excluded; vector (after the mode, every mode) = every input line is a float vector of the model's "
           "width, as many numbers as a row has: the k rows nearest to it by cosine, nothing excluded; cosmul (after the mode, "
           "bits and codes only) = every input line is three words A B C: the k best answers to A : B = C : ? by the "
           "multiplicative rule 3CosMul; rank (after the mode, bits and codes only, k is ignored) = every input line is two words "
           "A G or four words A B C G: the place of G among the neighbours of A, or as the answer to A : B = C : ?, in the complete "
           "answer list, the number of rows tied with it and its score; docs CORPUS.txt [oneway] (after the mode, bits and codes only) = every line of CORPUS.txt "
           "is one document, every input line one query text: the line numbers of the k documents nearest to it by relaxed word "
           "mover's similarity, oneway = by how well the query's words are matched alone\n",
           W2B_EVAL_MAX_K, W2B_EVAL_MAX_TERMS, W2B_EVAL_MAX_BAG);
    return 0;
  }
  const int k = argc > 2 ? atoi(argv[2]) : 10;
  if (k < 1 || k > W2B_EVAL_MAX_K) {
    fprintf(stderr, "nearest: k must be 1..%d\n", W2B_EVAL_MAX_K);
    return 2;
  }
  const int bitlevel = argc > 3 ? atoi(argv[3]) : 0;
  const long long threshold = argc > 4 ? atoi(argv[4]) : 0;
  const bool is_signed = argc > 6 && !strcmp(argv[6], "signed"), is_bag = argc > 6 && !strcmp(argv[6], "bag");
  const bool is_vector = argc > 6 && !strcmp(argv[6], "vector"), is_cosmul = argc > 6 && !strcmp(argv[6], "cosmul");
  const bool is_docs = argc > 6 && !strcmp(argv[6], "docs"), is_rank = argc > 6 && !strcmp(argv[6], "rank");
  const int symmetric = argc > 8 && !strcmp(argv[8], "oneway") ? 0 : 1;
  std::string corpus;
  if (is_docs) {
    FILE *f = argc > 7 ? fopen(argv[7], "rb") : nullptr;
    if (!f) {
      printf("Corpus file not found\n");
      return -1;
    }
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) corpus.append(buf, n);
    fclose(f);
  }
  return w2b_eval_cli("nearest", argv[1], bitlevel, threshold, argc > 5 ? argv[5] : nullptr,
                      [&, k, is_signed, is_bag, is_vector, is_cosmul, is_rank](w2b_eval *e, const char *in, int64_t len, char **txt, int64_t *txt_len) {
                        if (is_docs) {
                          int64_t n_docs = 0, dropped = 0;
                          if (int rc = w2b_eval_docs_set_text(e, corpus.data(), (int64_t)corpus.size(), &n_docs, &dropped)) return rc;
                          fprintf(stderr, "nearest: %lld documents, %lld words outside the vocabulary dropped\n", (long long)n_docs,
                                  (long long)dropped);
                          return w2b_eval_docs_text(e, in, len, symmetric, k, txt, txt_len);
                        }
                        if (is_rank) return w2b_eval_rank_text(e, in, len, txt, txt_len);
                        if (is_cosmul) return w2b_eval_cosmul_text(e, in, len, k, txt, txt_len);
                        if (is_vector) return w2b_eval_vectors_text(e, in, len, 1, k, txt, txt_len);
                        if (is_bag) return w2b_eval_bag_text(e, in, len, 1, k, txt, txt_len);
                        return is_signed ? w2b_eval_combine_text(e, in, len, k, txt, txt_len)
                                         : w2b_eval_nearest_text(e, in, len, k, txt, txt_len);
                      });
}
