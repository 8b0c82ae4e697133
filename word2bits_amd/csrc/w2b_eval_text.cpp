// w2b_eval_text.cpp -- the text front ends of include/word2bits_eval.h: the question-stream state machine and the stdout
// transcript of the reference evaluator (ref src/compute-accuracy.c:114-187), and the *_text form of every other question.
// Parsing and printing only.  The unit is written against the public header: a handle is an opaque pointer here, read
// through w2b_eval_word / _words / _size / _is_bits / _is_codes / _docs_count / _lookup, and the GPU is reached through the
// array entry points (w2b_eval_top1, _topk, _cosmul, _rank, _combine, _bag, _vectors, _docs_set, _docs, _pairs, _classes) alone.
// What it refuses in the words of those entry points comes from w2b_eval_shared.h.
#include "w2b_eval_shared.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <locale.h>
#include <utility>

// ------------------------------------------------------------------------------------ transcript
namespace {
// scanf("%s", st) over a buffer.  `hit_end` mirrors feof(stdin): it latches as soon as a read runs into the end
// of the input, which also happens while reading a last token that has no trailing white space.
struct TokenIn {
  const char *p;
  int64_t n, pos = 0;
  bool hit_end = false;
  bool next(std::string &st) {             // false: nothing read, st keeps its old contents
    while (pos < n && is_space((unsigned char)p[pos])) pos++;
    if (pos >= n) { hit_end = true; return false; }
    const int64_t s = pos;
    while (pos < n && !is_space((unsigned char)p[pos])) pos++;
    if (pos >= n) hit_end = true;
    st.assign(p + s, (size_t)(pos - s));
    return true;
  }
};
void upper_inplace(std::string &s) { for (char &c : s) c = c_upper(c); }

struct Step {                // what the loop of ref :114-186 does, in stream order
  enum Kind { SectionEnd, SectionName, Question } kind;
  int qid;                   // QID at that moment
  std::string text;          // section name / expected word (st4)
  int64_t q;                 // index into the batched questions
};

void appendf(std::string &out, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void appendf(std::string &out, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  const int n = vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  out.append(buf, (size_t)(n < (int)sizeof buf ? n : (int)sizeof buf - 1));
}

// a text result leaves the library as a malloc'ed, 0-terminated copy (w2b_eval_free_text)
int text_out(const std::string &txt, const char *who, char **out, int64_t *out_len) {
  char *buf = (char *)malloc(txt.size() + 1);
  if (!buf) return efail(W2B_ENOMEM, std::string(who) + ": out of memory");
  memcpy(buf, txt.data(), txt.size());
  buf[txt.size()] = 0;
  *out = buf;
  if (out_len) *out_len = (int64_t)txt.size();
  return W2B_OK;
}
}  // namespace

namespace {
// "<m>" of the RANKS lines: a mean of reciprocal ranks, or the letters nan for a scope without a question (a computed NaN
// would print with the platform's sign)
std::string mean_text(double sum, int n) {
  if (n == 0) return "nan";
  std::string t;
  appendf(t, "%.4f", sum / (double)n);
  return t;
}
}  // namespace

// `answer(e, nq, b1, b2, b3, best)` scores all answerable questions at once: best[q] = the answer's row or -1.  `ranks`:
// the RANKS lines of w2b_eval_transcript_rank after every "Total accuracy" line, from one w2b_eval_rank batch with each
// question's expected word as the target.
template <class Answer>
static int eval_transcript(w2b_eval *e, const char *questions, int64_t len, char **out, int64_t *out_len, const char *who,
                           Answer answer, bool ranks = false) {
  if (!e || !out || len < 0 || (len > 0 && !questions)) return efail(W2B_EINVAL, std::string(who) + ": bad argument");
  *out = nullptr;
  const int64_t words = w2b_eval_words(e);
  TokenIn in{questions, len};
  std::string st1, st2, st3, st4;
  std::vector<Step> steps;
  std::vector<int32_t> b1s, b2s, b3s, tgts;
  int QID = 0, TQ = 0, TQS = 0;
  // pass 1: parse the stream exactly like the scanf loop; collect the answerable questions
  for (;;) {
    in.next(st1);
    upper_inplace(st1);
    if (st1 == ":" || st1 == "EXIT" || in.hit_end) {                 // ref :119
      steps.push_back({Step::SectionEnd, QID, std::string(), 0});
      QID++;
      in.next(st1);                                                   // section name, printed as read (ref :126-128)
      if (in.hit_end) break;
      steps.push_back({Step::SectionName, QID, st1, 0});
      continue;
    }
    in.next(st2); upper_inplace(st2);
    in.next(st3); upper_inplace(st3);
    in.next(st4); upper_inplace(st4);
    const int64_t r1 = w2b_eval_lookup(e, st1.c_str()), r2 = w2b_eval_lookup(e, st2.c_str()),
                  r3 = w2b_eval_lookup(e, st3.c_str());
    TQ++;
    if (r1 == words || r2 == words || r3 == words) continue;          // ref :149-151
    const int64_t r4 = w2b_eval_lookup(e, st4.c_str());
    if (r4 == words) continue;                                        // ref :152-153
    TQS++;
    steps.push_back({Step::Question, QID, st4, (int64_t)b1s.size()});
    tgts.push_back((int32_t)r4);
    b1s.push_back((int32_t)r1);
    b2s.push_back((int32_t)r2);
    b3s.push_back((int32_t)r3);
  }
  // the scan of ref :155-177 for all of them at once, on the GPU
  std::vector<int32_t> best(b1s.size());
  if (!b1s.empty()) {
    const int rc = answer(e, (int64_t)b1s.size(), b1s.data(), b2s.data(), b3s.data(), best.data());
    if (rc != W2B_OK) return rc;
  }
  std::vector<int32_t> rank(b1s.size());
  if (ranks && !b1s.empty()) {
    const int rc = w2b_eval_rank(e, (int64_t)b1s.size(), b1s.data(), b2s.data(), b3s.data(), tgts.data(), rank.data(), nullptr, nullptr);
    if (rc != W2B_OK) return rc;
  }
  // pass 2: replay the counters and print (ref :120-131,178-187)
  std::string txt = "Starting eval...\n";
  int TCN = 0, CCN = 0, TACN = 0, CACN = 0, SECN = 0, SYCN = 0, SEAC = 0, SYAC = 0;
  // RANKS: sums of 1 / rank in stream order and question counts, of the section, of all, semantic and syntactic questions
  double rs_sec = 0, rs_all = 0, rs_sem = 0, rs_syn = 0;
  int rn_sec = 0, rn_all = 0, rn_sem = 0, rn_syn = 0, hits1 = 0, hits5 = 0, hits10 = 0, unranked = 0;
  for (const Step &s : steps) {
    if (s.kind == Step::SectionEnd) {
      if (TCN == 0) TCN = 1;
      if (s.qid != 0) {
        appendf(txt, "ACCURACY TOP1: %.2f %%  (%d / %d)\n", CCN / (float)TCN * 100, CCN, TCN);
        appendf(txt, "Total accuracy: %.2f %%   Semantic accuracy: %.2f %%   Syntactic accuracy: %.2f %% \n",
                CACN / (float)TACN * 100, SEAC / (float)SECN * 100, SYAC / (float)SYCN * 100);
        if (ranks) {
          appendf(txt, "RANKS section: MRR %s   hits@1 %d   hits@5 %d   hits@10 %d   unranked %d   (%d questions)\n",
                  mean_text(rs_sec, rn_sec).c_str(), hits1, hits5, hits10, unranked, rn_sec);
          appendf(txt, "RANKS total: MRR %s   Semantic MRR %s   Syntactic MRR %s\n", mean_text(rs_all, rn_all).c_str(),
                  mean_text(rs_sem, rn_sem).c_str(), mean_text(rs_syn, rn_syn).c_str());
        }
      }
    } else if (s.kind == Step::SectionName) {
      txt += s.text;
      txt += ":\n";
      TCN = 0;
      CCN = 0;
      rs_sec = 0;
      rn_sec = hits1 = hits5 = hits10 = unranked = 0;
    } else {
      const int32_t c = best[(size_t)s.q];
      const char *bestw = c >= 0 ? w2b_eval_word(e, c) : "";
      if (s.text == bestw) {                                           // strcmp on the words (ref :178)
        CCN++;
        CACN++;
        if (s.qid <= 5) SEAC++; else SYAC++;
      }
      if (s.qid <= 5) SECN++; else SYCN++;
      TCN++;
      TACN++;
      if (ranks) {
        const int32_t r = rank[(size_t)s.q];
        const double rr = r > 0 ? 1.0 / (double)r : 0.0;
        rs_sec += rr, rn_sec++;
        rs_all += rr, rn_all++;
        if (s.qid <= 5) rs_sem += rr, rn_sem++; else rs_syn += rr, rn_syn++;
        hits1 += r == 1, hits5 += r >= 1 && r <= 5, hits10 += r >= 1 && r <= 10, unranked += r == 0;
      }
    }
  }
  appendf(txt, "Questions seen / total: %d %d   %.2f %% \n", TQS, TQ, TQS / (float)TQ * 100);
  return text_out(txt, who, out, out_len);
}

extern "C" int w2b_eval_transcript(w2b_eval *e, const char *questions, int64_t len, char **out, int64_t *out_len) {
  return eval_transcript(e, questions, len, out, out_len, "w2b_eval_transcript",
                         [](w2b_eval *ev, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3, int32_t *best) {
                           return w2b_eval_top1(ev, nq, b1, b2, b3, best, nullptr);
                         });
}

extern "C" int w2b_eval_transcript_cosmul(w2b_eval *e, const char *questions, int64_t len, char **out, int64_t *out_len) {
  return eval_transcript(e, questions, len, out, out_len, "w2b_eval_transcript_cosmul",
                         [](w2b_eval *ev, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3, int32_t *best) {
                           return w2b_eval_cosmul(ev, nq, b1, b2, b3, 1, best, nullptr);
                         });
}

extern "C" int w2b_eval_transcript_rank(w2b_eval *e, const char *questions, int64_t len, char **out, int64_t *out_len) {
  const char *who = "w2b_eval_transcript_rank";
  if (!out || len < 0 || (len > 0 && !questions)) return efail(W2B_EINVAL, std::string(who) + ": bad argument");
  if (!e) return efail(W2B_EINVAL, std::string(who) + ": null handle");
  if (!w2b_eval_is_bits(e) && !w2b_eval_is_codes(e)) return efail(W2B_EINVAL, std::string(who) + ": " + kDocsFp32);
  return eval_transcript(e, questions, len, out, out_len, who,
                         [](w2b_eval *ev, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3, int32_t *best) {
                           return w2b_eval_top1(ev, nq, b1, b2, b3, best, nullptr);
                         },
                         true);
}

// ------------------------------------------------------------------------------------ the forms that answer with lists
namespace {
// one line of a query text: what was understood, or what to say instead
struct QueryLine { std::string head; std::string error; int64_t q; };

// the next line of queries[pos .. len) split on white space, every token upper-cased (ref :118); false at the end
bool next_query_line(const char *queries, int64_t len, int64_t &pos, std::vector<std::string> &tok) {
  if (pos >= len) return false;
  int64_t end = pos;
  while (end < len && queries[end] != '\n') end++;
  tok.clear();
  for (int64_t i = pos; i < end;) {
    while (i < end && is_space((unsigned char)queries[i])) i++;
    const int64_t s0 = i;
    while (i < end && !is_space((unsigned char)queries[i])) i++;
    if (i > s0) {
      tok.emplace_back(queries + s0, (size_t)(i - s0));
      upper_inplace(tok.back());
    }
  }
  pos = end + 1;
  return true;
}

std::string joined(const std::vector<std::string> &tok) {
  std::string head;
  for (size_t i = 0; i < tok.size(); i++) head += (i ? " " : "") + tok[i];
  return head;
}

// What every list-answer form does with its text, after its own argument checks.  Every non-empty line becomes a QueryLine
// whose head is the line's words: parse(tok, ordinal, ln) either appends one question to the vectors it owns or sets
// ln.error, and may replace the head (ordinal counts the non-empty lines from 1, refused ones included).  run(nq, best,
// bestd) is the array entry point on those nq questions, k answers each; it is not called when no line gave a question,
// and its failure is returned with *out left null.  Then per line the head and the error, or the answers up to the first
// -1: the vocabulary word of the row (rows_are_words) or the row + 1, a document's line number.
template <class Parse, class Run>
int text_queries(w2b_eval *e, const char *queries, int64_t len, int32_t k, const char *who, Parse parse, Run run,
                 bool rows_are_words, char **out, int64_t *out_len) {
  *out = nullptr;
  std::vector<QueryLine> lines;
  std::vector<std::string> tok;
  int64_t nq = 0;
  for (int64_t pos = 0; next_query_line(queries, len, pos, tok);) {
    if (tok.empty()) continue;
    QueryLine ln{joined(tok), std::string(), -1};
    parse(tok, (int64_t)lines.size() + 1, ln);
    if (ln.error.empty()) ln.q = nq++;
    lines.push_back(ln);
  }
  std::vector<int32_t> best((size_t)nq * (size_t)k);
  std::vector<float> bestd((size_t)nq * (size_t)k);
  if (nq > 0) {
    const int rc = run(nq, best.data(), bestd.data());
    if (rc != W2B_OK) return rc;
  }
  std::string txt;
  for (const QueryLine &ln : lines) {
    txt += ln.head;
    if (!ln.error.empty()) {
      txt += ": " + ln.error + "\n";
      continue;
    }
    txt += ":\n";
    for (int j = 0; j < k; j++) {
      const int32_t c = best[(size_t)(ln.q * k + j)];
      if (c < 0) break;
      const double score = (double)bestd[(size_t)(ln.q * k + j)];
      if (rows_are_words) appendf(txt, "%d\t%s\t%.6f\n", j + 1, w2b_eval_word(e, c), score);
      else appendf(txt, "%d\t%lld\t%.6f\n", j + 1, (long long)c + 1, score);
    }
  }
  return text_out(txt, who, out, out_len);
}

// a line of one or three words: their rows appended to b[0], b[1], b[2] (one word: its row three times), or the first word
// that is not in the vocabulary
void three_rows(const w2b_eval *e, const std::vector<std::string> &tok, std::vector<int32_t> (&b)[3], QueryLine &ln) {
  int64_t r[3] = {0, 0, 0};
  for (size_t i = 0; i < tok.size(); i++) {
    r[i] = w2b_eval_lookup(e, tok[i].c_str());
    if (r[i] == w2b_eval_words(e)) {
      ln.error = "not in vocabulary: " + tok[i];
      return;
    }
  }
  if (tok.size() == 1) r[1] = r[2] = r[0];
  for (int i = 0; i < 3; i++) b[i].push_back((int32_t)r[i]);
}
}  // namespace

extern "C" int w2b_eval_nearest_text(w2b_eval *e, const char *queries, int64_t len, int32_t k, char **out,
                                     int64_t *out_len) {
  const char *who = "w2b_eval_nearest_text";
  if (!e || !out || len < 0 || (len > 0 && !queries)) return efail(W2B_EINVAL, std::string(who) + ": bad argument");
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, std::string(who) + ": k must be 1..64");
  std::vector<int32_t> b[3];
  return text_queries(
      e, queries, len, k, who,
      [&](const std::vector<std::string> &tok, int64_t, QueryLine &ln) {
        if (tok.size() != 1 && tok.size() != 3) ln.error = "expected 1 or 3 words";
        else three_rows(e, tok, b, ln);
      },
      [&](int64_t nq, int32_t *best, float *bestd) { return w2b_eval_topk(e, nq, b[0].data(), b[1].data(), b[2].data(), k, best, bestd); },
      true, out, out_len);
}

// the 3CosMul form: every non-empty line is three words A B C
extern "C" int w2b_eval_cosmul_text(w2b_eval *e, const char *queries, int64_t len, int32_t k, char **out, int64_t *out_len) {
  const char *who = "w2b_eval_cosmul_text";
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, std::string(who) + ": k must be 1..64");
  if (!out || len < 0 || (len > 0 && !queries)) return efail(W2B_EINVAL, std::string(who) + ": bad argument");
  if (!e) return efail(W2B_EINVAL, std::string(who) + ": null handle");
  if (!w2b_eval_is_bits(e) && !w2b_eval_is_codes(e)) return efail(W2B_EINVAL, std::string(who) + ": " + kDocsFp32);
  std::vector<int32_t> b[3];
  return text_queries(
      e, queries, len, k, who,
      [&](const std::vector<std::string> &tok, int64_t, QueryLine &ln) {
        if (tok.size() != 3) ln.error = "expected 3 words";
        else three_rows(e, tok, b, ln);
      },
      [&](int64_t nq, int32_t *best, float *bestd) { return w2b_eval_cosmul(e, nq, b[0].data(), b[1].data(), b[2].data(), k, best, bestd); },
      true, out, out_len);
}

// the rank form: every non-empty line is "A G" (G among the neighbours of A) or "A B C G" (G as the answer to A : B = C : ?)
extern "C" int w2b_eval_rank_text(w2b_eval *e, const char *queries, int64_t len, char **out, int64_t *out_len) {
  const char *who = "w2b_eval_rank_text";
  if (!out || len < 0 || (len > 0 && !queries)) return efail(W2B_EINVAL, std::string(who) + ": bad argument");
  if (!e) return efail(W2B_EINVAL, std::string(who) + ": null handle");
  if (!w2b_eval_is_bits(e) && !w2b_eval_is_codes(e)) return efail(W2B_EINVAL, std::string(who) + ": " + kDocsFp32);
  *out = nullptr;
  std::vector<QueryLine> lines;
  std::vector<std::string> tok;
  std::vector<int32_t> b[3], tgt;
  for (int64_t pos = 0; next_query_line(queries, len, pos, tok);) {
    if (tok.empty()) continue;
    QueryLine ln{joined(tok), std::string(), -1};
    if (tok.size() != 2 && tok.size() != 4) {
      ln.error = "expected 2 or 4 words";
    } else {
      const std::string g = tok.back();
      tok.pop_back();                                   // one or three words: the question's rows
      three_rows(e, tok, b, ln);
      if (ln.error.empty()) {
        const int64_t r = w2b_eval_lookup(e, g.c_str());
        if (r == w2b_eval_words(e)) {
          ln.error = "not in vocabulary: " + g;
          for (auto &v : b) v.pop_back();
        } else {
          tgt.push_back((int32_t)r);
          ln.q = (int64_t)tgt.size() - 1;
        }
      }
    }
    lines.push_back(ln);
  }
  std::vector<int32_t> rank(tgt.size()), tied(tgt.size());
  std::vector<float> score(tgt.size());
  if (!tgt.empty()) {
    const int rc = w2b_eval_rank(e, (int64_t)tgt.size(), b[0].data(), b[1].data(), b[2].data(), tgt.data(), rank.data(),
                                 tied.data(), score.data());
    if (rc != W2B_OK) return rc;
  }
  std::string txt;
  for (const QueryLine &ln : lines) {
    txt += ln.head;
    if (!ln.error.empty()) txt += ": " + ln.error + "\n";
    else if (rank[(size_t)ln.q] == 0) txt += ": no rank\n";
    else appendf(txt, ":\t%d\t%d\t%.6f\n", rank[(size_t)ln.q], tied[(size_t)ln.q], (double)score[(size_t)ln.q]);
  }
  return text_out(txt, who, out, out_len);
}

// the signed form: +WORD, -WORD or WORD, 1 to W2B_EVAL_MAX_TERMS of them per line; a question always takes all the slots
extern "C" int w2b_eval_combine_text(w2b_eval *e, const char *queries, int64_t len, int32_t k, char **out,
                                     int64_t *out_len) {
  const char *who = "w2b_eval_combine_text";
  if (!e || !out || len < 0 || (len > 0 && !queries)) return efail(W2B_EINVAL, std::string(who) + ": bad argument");
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, std::string(who) + ": k must be 1..64");
  if (w2b_eval_is_codes(e)) return efail(W2B_EINVAL, std::string(who) + ": not available in codes mode");
  std::vector<int32_t> rows;
  std::vector<int8_t> signs;
  return text_queries(
      e, queries, len, k, who,
      [&](const std::vector<std::string> &tok, int64_t, QueryLine &ln) {
        int32_t r[W2B_EVAL_MAX_TERMS] = {0};
        int8_t sg[W2B_EVAL_MAX_TERMS] = {0};
        if (tok.size() > W2B_EVAL_MAX_TERMS) ln.error = "expected 1 to 7 signed words";
        for (size_t i = 0; i < tok.size() && ln.error.empty(); i++) {
          const bool has_sign = tok[i][0] == '+' || tok[i][0] == '-';
          const std::string word = tok[i].substr(has_sign ? 1 : 0);
          const int64_t row = w2b_eval_lookup(e, word.c_str());
          if (row == w2b_eval_words(e)) ln.error = "not in vocabulary: " + word;
          r[i] = (int32_t)row;
          sg[i] = tok[i][0] == '-' ? -1 : 1;
        }
        if (!ln.error.empty()) return;
        rows.insert(rows.end(), r, r + W2B_EVAL_MAX_TERMS);
        signs.insert(signs.end(), sg, sg + W2B_EVAL_MAX_TERMS);
      },
      [&](int64_t nq, int32_t *best, float *bestd) {
        return w2b_eval_combine(e, nq, W2B_EVAL_MAX_TERMS, rows.data(), signs.data(), k, best, bestd);
      },
      true, out, out_len);
}

// the bag form: every non-empty line is one bag of 1 to W2B_EVAL_MAX_BAG words
extern "C" int w2b_eval_bag_text(w2b_eval *e, const char *queries, int64_t len, int32_t exclude_own, int32_t k, char **out,
                                 int64_t *out_len) {
  const char *who = "w2b_eval_bag_text";
  if (!e || !out || len < 0 || (len > 0 && !queries)) return efail(W2B_EINVAL, std::string(who) + ": bad argument");
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, std::string(who) + ": k must be 1..64");
  if (exclude_own != 0 && exclude_own != 1) return efail(W2B_EINVAL, std::string(who) + ": exclude_own must be 0 or 1");
  if (!w2b_eval_is_bits(e) && !w2b_eval_is_codes(e)) return efail(W2B_EINVAL, std::string(who) + ": needs a bits or a codes handle");
  std::vector<int32_t> ids;
  std::vector<int64_t> offsets(1, 0);
  return text_queries(
      e, queries, len, k, who,
      [&](const std::vector<std::string> &tok, int64_t, QueryLine &ln) {
        if (tok.size() > W2B_EVAL_MAX_BAG) ln.error = "expected 1 to 4096 words";
        const size_t at = ids.size();
        for (size_t i = 0; i < tok.size() && ln.error.empty(); i++) {
          const int64_t row = w2b_eval_lookup(e, tok[i].c_str());
          if (row == w2b_eval_words(e)) ln.error = "not in vocabulary: " + tok[i];
          ids.push_back((int32_t)row);
        }
        if (ln.error.empty()) offsets.push_back((int64_t)ids.size());
        else ids.resize(at);
      },
      [&](int64_t nq, int32_t *best, float *bestd) {
        return w2b_eval_bag(e, (int64_t)ids.size(), ids.data(), nq, offsets.data(), exclude_own, k, best, bestd);
      },
      true, out, out_len);
}

// the vector form: every non-empty line is `size` numbers; its head is its number among the non-empty lines
extern "C" int w2b_eval_vectors_text(w2b_eval *e, const char *queries, int64_t len, int32_t normalize, int32_t k, char **out,
                                     int64_t *out_len) {
  const char *who = "w2b_eval_vectors_text";
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, std::string(who) + ": k must be 1..64");
  if (normalize != 0 && normalize != 1) return efail(W2B_EINVAL, std::string(who) + ": normalize must be 0 or 1");
  if (!out || len < 0 || (len > 0 && !queries)) return efail(W2B_EINVAL, std::string(who) + ": bad argument");
  if (!e) return efail(W2B_EINVAL, std::string(who) + ": null handle");
  *out = nullptr;
  static const locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
  if (!c_locale) return efail(W2B_ENOMEM, std::string(who) + ": no C locale");
  const int64_t size = w2b_eval_size(e);
  std::vector<float> x, row((size_t)size);
  return text_queries(
      e, queries, len, k, who,
      [&](const std::vector<std::string> &tok, int64_t ordinal, QueryLine &ln) {
        ln.head = "vector " + std::to_string(ordinal);
        bool numbers = (int64_t)tok.size() == size;
        for (size_t i = 0; i < tok.size() && numbers; i++) {
          char *end = nullptr;
          row[i] = strtof_l(tok[i].c_str(), &end, c_locale);
          numbers = end == tok[i].c_str() + tok[i].size();
        }
        if (!numbers) ln.error = "expected " + std::to_string(size) + " numbers";
        else if (bad_vector_value(row.data(), size) >= 0) ln.error = "value out of range";
        else x.insert(x.end(), row.begin(), row.end());
      },
      [&](int64_t nq, int32_t *best, float *bestd) { return w2b_eval_vectors(e, nq, x.data(), normalize, k, best, bestd); },
      true, out, out_len);
}

// the corpus from text: one document per line, empty lines included; words that are not in the vocabulary are dropped
extern "C" int w2b_eval_docs_set_text(w2b_eval *e, const char *text, int64_t len, int64_t *n_docs, int64_t *dropped) {
  const std::string who = "w2b_eval_docs_set_text";
  if (len < 0 || (len > 0 && !text)) return efail(W2B_EINVAL, who + ": bad argument");
  if (!e) return efail(W2B_EINVAL, who + ": null handle");
  if (!w2b_eval_is_bits(e) && !w2b_eval_is_codes(e)) return efail(W2B_EINVAL, who + ": " + kDocsFp32);
  const int64_t words = w2b_eval_words(e);
  std::vector<int32_t> ids;
  std::vector<int64_t> offsets(1, 0);
  std::vector<std::string> tok;
  int64_t lost = 0;
  for (int64_t pos = 0; next_query_line(text, len, pos, tok);) {
    for (const std::string &w : tok) {
      const int64_t row = w2b_eval_lookup(e, w.c_str());
      if (row == words) lost++;
      else ids.push_back((int32_t)row);
    }
    if ((int64_t)ids.size() - offsets.back() > W2B_EVAL_MAX_DOC)
      return efail(W2B_EINVAL, who + ": line " + std::to_string(offsets.size()) + ": a document holds at most 1024 words");
    offsets.push_back((int64_t)ids.size());
  }
  if (int rc = w2b_eval_docs_set(e, (int64_t)ids.size(), ids.data(), (int64_t)offsets.size() - 1, offsets.data())) return rc;
  if (n_docs) *n_docs = (int64_t)offsets.size() - 1;
  if (dropped) *dropped = lost;
  return W2B_OK;
}

// the document form: every non-empty line is one query text; an answer line names a document by its line number
extern "C" int w2b_eval_docs_text(w2b_eval *e, const char *queries, int64_t len, int32_t symmetric, int32_t k, char **out,
                                  int64_t *out_len) {
  const char *who = "w2b_eval_docs_text";
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, std::string(who) + ": k must be 1..64");
  if (symmetric != 0 && symmetric != 1) return efail(W2B_EINVAL, std::string(who) + ": symmetric must be 0 or 1");
  if (!out || len < 0 || (len > 0 && !queries)) return efail(W2B_EINVAL, std::string(who) + ": bad argument");
  if (!e) return efail(W2B_EINVAL, std::string(who) + ": null handle");
  if (!w2b_eval_is_bits(e) && !w2b_eval_is_codes(e)) return efail(W2B_EINVAL, std::string(who) + ": " + kDocsFp32);
  if (w2b_eval_docs_count(e) == 0) return efail(W2B_EINVAL, std::string(who) + ": no corpus is set (w2b_eval_docs_set)");
  std::vector<int32_t> ids;
  std::vector<int64_t> offsets(1, 0);
  return text_queries(
      e, queries, len, k, who,
      [&](const std::vector<std::string> &tok, int64_t, QueryLine &ln) {
        const size_t at = ids.size();
        for (const std::string &w : tok) {
          const int64_t row = w2b_eval_lookup(e, w.c_str());
          if (row != w2b_eval_words(e)) ids.push_back((int32_t)row);
        }
        if (ids.size() == at) ln.error = "no word in vocabulary";
        else if (ids.size() - at > W2B_EVAL_MAX_DOC) ln.error = "expected at most 1024 words";
        if (ln.error.empty()) offsets.push_back((int64_t)ids.size());
        else ids.resize(at);
      },
      [&](int64_t nq, int32_t *best, float *bestd) {
        return w2b_eval_docs(e, (int64_t)ids.size(), ids.data(), nq, offsets.data(), symmetric, k, best, bestd, nullptr);
      },
      false, out, out_len);
}

// ------------------------------------------------------------------------------------ pair similarity
namespace {
// one pair line of w2b_eval_pairs_text: its fields as written, or its number when it is malformed
struct PairLine {
  bool malformed;
  int64_t number, p;
  std::string gold_text, a_text, b_text;
  double gold;
};

// the blank-separated words of s, upper-cased
std::vector<std::string> upper_words(const std::string &s) {
  std::vector<std::string> tok;
  for (size_t i = 0; i < s.size();) {
    while (i < s.size() && is_space((unsigned char)s[i])) i++;
    const size_t s0 = i;
    while (i < s.size() && !is_space((unsigned char)s[i])) i++;
    if (i > s0) {
      tok.emplace_back(s, s0, i - s0);
      upper_inplace(tok.back());
    }
  }
  return tok;
}

std::string stripped(const std::string &s) {
  size_t a = 0, b = s.size();
  while (a < b && is_space((unsigned char)s[a])) a++;
  while (b > a && is_space((unsigned char)s[b - 1])) b--;
  return s.substr(a, b - a);
}

// the three fields of a pair line: the tab-separated parts when there is a tab, else the runs of non-blank characters
std::vector<std::string> pair_fields(const std::string &line) {
  std::vector<std::string> f;
  if (line.find('\t') != std::string::npos) {
    for (size_t i = 0;;) {
      const size_t t = line.find('\t', i);
      f.push_back(stripped(line.substr(i, t == std::string::npos ? t : t - i)));
      if (t == std::string::npos) break;
      i = t + 1;
    }
    return f;
  }
  for (size_t i = 0; i < line.size();) {
    while (i < line.size() && is_space((unsigned char)line[i])) i++;
    const size_t s0 = i;
    while (i < line.size() && !is_space((unsigned char)line[i])) i++;
    if (i > s0) f.emplace_back(line, s0, i - s0);
  }
  return f;
}
}  // namespace

// the pair form: every pair line is A, B and a gold score; one batch, then the correlations of the scored pairs
extern "C" int w2b_eval_pairs_text(w2b_eval *e, const char *pairs, int64_t len, int32_t details, char **out, int64_t *out_len) {
  const std::string who = "w2b_eval_pairs_text";
  if (!out || len < 0 || (len > 0 && !pairs)) return efail(W2B_EINVAL, who + ": bad argument");
  if (!e) return efail(W2B_EINVAL, who + ": null handle");
  if (!w2b_eval_is_bits(e) && !w2b_eval_is_codes(e)) return efail(W2B_EINVAL, who + ": " + kDocsFp32);
  *out = nullptr;
  static const locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
  if (!c_locale) return efail(W2B_ENOMEM, who + ": no C locale");
  const int64_t words = w2b_eval_words(e);
  std::vector<PairLine> lines;
  std::vector<int32_t> ids;
  std::vector<int64_t> offsets(1, 0);
  int64_t looked = 0, oov = 0, malformed = 0, number = 0;
  for (int64_t pos = 0; pos < len;) {
    int64_t end = pos;
    while (end < len && pairs[end] != '\n') end++;
    std::string line(pairs + pos, (size_t)(end - pos));
    pos = end + 1;
    number++;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (stripped(line).empty() || line[0] == '#') continue;
    PairLine ln{true, number, -1, std::string(), std::string(), std::string(), 0.0};
    const std::vector<std::string> f = pair_fields(line);
    std::vector<std::string> wa, wb;
    if (f.size() == 3 && !f[2].empty()) {
      char *stop = nullptr;
      ln.gold = strtod_l(f[2].c_str(), &stop, c_locale);
      wa = upper_words(f[0]);
      wb = upper_words(f[1]);
      ln.malformed = stop != f[2].c_str() + f[2].size() || !std::isfinite(ln.gold) || wa.empty() || wb.empty() ||
                     wa.size() > W2B_EVAL_MAX_BAG || wb.size() > W2B_EVAL_MAX_BAG;
    }
    if (ln.malformed) {
      malformed++;
    } else {
      ln.a_text = f[0], ln.b_text = f[1], ln.gold_text = f[2];
      ln.p = (int64_t)(offsets.size() - 1) / 2;
      for (const std::vector<std::string> *side : {&wa, &wb}) {
        for (const std::string &w : *side) {
          const int64_t row = w2b_eval_lookup(e, w.c_str());
          looked++;
          if (row == words) oov++;
          else ids.push_back((int32_t)row);
        }
        offsets.push_back((int64_t)ids.size());
      }
    }
    lines.push_back(ln);
  }
  const int64_t np = (int64_t)(offsets.size() - 1) / 2;
  std::vector<float> score((size_t)np);
  std::vector<int64_t> parts((size_t)np * 3);
  if (np > 0)
    if (int rc = w2b_eval_pairs(e, (int64_t)ids.size(), ids.data(), np, offsets.data(), score.data(), parts.data())) return rc;
  std::string txt;
  std::vector<double> x, y;
  int64_t skipped = 0;
  for (const PairLine &ln : lines) {
    if (ln.malformed) {
      if (details) txt += "malformed line " + std::to_string(ln.number) + "\n";
      continue;
    }
    const bool empty = parts[(size_t)(3 * ln.p + 1)] == 0 || parts[(size_t)(3 * ln.p + 2)] == 0;
    if (empty) {
      skipped++;
      if (details) txt += "skipped";
    } else {
      x.push_back(ln.gold);
      y.push_back((double)score[(size_t)ln.p]);
      if (details) appendf(txt, "%.6f", (double)score[(size_t)ln.p]);
    }
    if (details) txt += "\t" + ln.gold_text + "\t" + ln.a_text + "\t" + ln.b_text + "\n";
  }
  double pearson = NAN, spearman = NAN;
  if (int rc = w2b_rank_correlation((int64_t)x.size(), x.data(), y.data(), &pearson, &spearman)) return rc;
  appendf(txt, "pairs: %lld scored, %lld skipped, %lld malformed\n", (long long)x.size(), (long long)skipped, (long long)malformed);
  appendf(txt, "words: %lld looked up, %lld not in vocabulary\n", (long long)looked, (long long)oov);
  for (const auto &c : {std::make_pair("pearson", pearson), std::make_pair("spearman", spearman)}) {
    if (std::isnan(c.second)) txt += std::string(c.first) + ": nan\n";
    else appendf(txt, "%s: %.6f\n", c.first, c.second);
  }
  return text_out(txt, who.c_str(), out, out_len);
}

// ------------------------------------------------------------------------------------ word classes
// word2vec's -classes file: one line "<word> <class>" per row, in row order
extern "C" int w2b_eval_classes_text(w2b_eval *e, int32_t n_classes, int32_t max_iters, char **out, int64_t *out_len) {
  const std::string who = "w2b_eval_classes_text";
  if (const char *why = bad_classes_args(n_classes, max_iters)) return efail(W2B_EINVAL, who + ": " + why);
  if (!e) return efail(W2B_EINVAL, who + ": null handle");
  if (!out) return efail(W2B_EINVAL, who + ": bad argument");
  const int64_t words = w2b_eval_words(e);
  std::vector<int32_t> cls((size_t)(words > 0 ? words : 1));
  if (int rc = w2b_eval_classes(e, n_classes, max_iters, nullptr, cls.data(), nullptr, nullptr, nullptr, nullptr, nullptr))
    return rc;
  std::string txt;
  for (int64_t c = 0; c < words; c++) {
    txt += w2b_eval_word(e, c);
    txt += ' ';
    txt += std::to_string(cls[(size_t)c]);
    txt += '\n';
  }
  return text_out(txt, who.c_str(), out, out_len);
}

extern "C" void w2b_eval_free_text(char *text) { free(text); }
