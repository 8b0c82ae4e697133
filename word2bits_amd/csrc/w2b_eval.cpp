// w2b_eval.cpp -- host side of include/word2bits_eval.h: the vector-file reader, the question-stream state
// machine and the stdout transcript of the reference evaluator (ref src/compute-accuracy.c:80-188), around the
// GPU scan in w2b_kernels_eval.hip.  No arithmetic on scores happens here and there is no CPU fallback.
#include "../../include/word2bits_eval.h"
#include "../../include/word2bits_hip.h"
#include "w2b_internal.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace {
constexpr int64_t kMaxW = 50;            // ref :24 max_w
constexpr int64_t kTile = 256;           // padding unit of rows / questions (covers both kernels' tiles)
constexpr int64_t kChunkQ = 1 << 16;     // questions per launch
constexpr int64_t kTopkScratch = 1ll << 30;   // default bound of the top-k slot scratch of one launch

inline bool is_space(unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }   // isspace, C locale
inline char c_upper(char c) { return (c >= 'a' && c <= 'z') ? (char)(c - 32) : c; }     // toupper, C locale

int efail(int code, const std::string &msg) { return w2b_internal_fail(code, msg.c_str()); }
#define EHIP(x)                                                                                   \
  do {                                                                                            \
    hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess) return efail(W2B_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)
}  // namespace

struct w2b_eval {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t words = 0, size = 0, ld = 0, rows_padded = 0;
  int fused = 1;
  int variant = 1;                                      // W2B_EVAL_KERNEL=0: vector-ALU kernel also in fused mode (default: MFMA)
  std::vector<char> vocab;                              // flat [words * max_w] (+ slack), as ref :88
  std::unordered_map<std::string, int64_t> first;       // upper-cased word -> first row (ref :140)
  float *M = nullptr;                                   // [rows_padded][ld], zero padded, normalised
  // bits mode (w2b_eval_load_bits / w2b_eval_bits_from_trainer): the rows stay packed and M does not exist
  int bits = 0;
  int64_t wpr = 0;                                      // 64-bit words per row
  uint64_t *B = nullptr;                                // [words][wpr], the file's layout
  uint32_t *P = nullptr;                                // per-call: the questions' planes [2 * 2 * wpr][cap_q]
  // per-call scratch (grown on demand)
  float *Q = nullptr;
  int32_t *b123 = nullptr;
  unsigned long long *best = nullptr;
  int64_t cap_q = 0;
  double kernel_ms = 0;                                 // score-kernel time since the last timing_read
  int64_t launches = 0;
  double macs = 0;
  // top-k scratch of one launch: bound / buckets / slot counts / slots / merged keys
  void *tk_buf = nullptr;
  size_t tk_bytes = 0;
  int64_t tk_budget = 0;                                // 0 = kTopkScratch
};

static void eval_release(w2b_eval *e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->M) (void)hipFree(e->M);
  if (e->B) (void)hipFree(e->B);
  if (e->P) (void)hipFree(e->P);
  if (e->Q) (void)hipFree(e->Q);
  if (e->b123) (void)hipFree(e->b123);
  if (e->best) (void)hipFree(e->best);
  if (e->tk_buf) (void)hipFree(e->tk_buf);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

// fscanf(f, "%lld", &x): skip white space, optional sign, digits
static bool scan_ll(const std::vector<unsigned char> &d, size_t &pos, long long *out) {
  while (pos < d.size() && is_space(d[pos])) pos++;
  size_t st = pos;
  if (pos < d.size() && (d[pos] == '+' || d[pos] == '-')) pos++;
  size_t dig = pos;
  while (pos < d.size() && d[pos] >= '0' && d[pos] <= '9') pos++;
  if (pos == dig) return false;
  *out = strtoll(std::string(d.begin() + st, d.begin() + pos).c_str(), nullptr, 10);
  return true;
}

// One row's name as the reference's reader leaves it (ref :97-105): bytes up to the first ' ', '\n' bytes dropped, at
// most max_w characters kept (the rest lands on index max_w = the next row's first byte, overwritten by that row
// later), a terminating 0, then upper-cased.  Consumes from d[pos...].
static void read_name(const unsigned char *d, size_t n, size_t &pos, char *row) {
  long long a = 0;
  for (;;) {
    const bool at_end = pos >= n;
    const unsigned char ch = at_end ? 0xFF : d[pos];              // (char)EOF
    if (!at_end) pos++;
    row[a] = (char)ch;
    if (at_end || ch == ' ') break;
    if (a < kMaxW && ch != '\n') a++;
  }
  row[a] = 0;
  for (long long i = 0; i < kMaxW; i++) row[i] = c_upper(row[i]);
}

// common tail of the two constructors: device buffers, quantize(x, bitlevel) + normalisation of the rows (ref :106-110).
// `host_rows` ([words][size], may be null) or `dev_rows` ([words][size] on the device, may be null) hold the raw values.
static int eval_finish(w2b_eval *e, int32_t bitlevel, const float *host_rows, const float *dev_rows, w2b_eval **out) {
  const long long words = e->words, size = e->size;
  char *vocab = e->vocab.data();
  for (long long b = 0; b < words; b++) e->first.emplace(std::string(vocab + b * kMaxW), b);   // first wins
  auto bail = [&](int rc) { eval_release(e); return rc; };
  if (hipSetDevice(e->device) != hipSuccess) return bail(efail(W2B_EHIP, "hipSetDevice failed"));
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess)
    return bail(efail(W2B_EHIP, "hipStreamCreate failed"));
  const size_t mbytes = (size_t)e->rows_padded * e->ld * 4;
  float *len = nullptr;
  if (hipMalloc(&e->M, mbytes) != hipSuccess || hipMalloc(&len, (size_t)(words + 1) * 4) != hipSuccess)
    return bail(efail(W2B_ENOMEM, "w2b_eval: device allocation failed"));
  hipError_t he = hipMemsetAsync(e->M, 0, mbytes, e->stream);
  if (he == hipSuccess && words > 0 && host_rows)
    he = hipMemcpy2DAsync(e->M, (size_t)e->ld * 4, host_rows, (size_t)size * 4, (size_t)size * 4, (size_t)words,
                          hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess && words > 0 && dev_rows)
    he = hipMemcpy2DAsync(e->M, (size_t)e->ld * 4, dev_rows, (size_t)size * 4, (size_t)size * 4, (size_t)words,
                          hipMemcpyDeviceToDevice, e->stream);
  if (he == hipSuccess) he = w2b_launch_eval_normalize(e->M, words, size, e->ld, bitlevel, e->fused, len, e->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
  (void)hipFree(len);
  if (he != hipSuccess) return bail(efail(W2B_EHIP, std::string("w2b_eval: ") + hipGetErrorString(he)));
  *out = e;
  return W2B_OK;
}

static w2b_eval *eval_new(long long words, long long size, int32_t fused, int32_t device) {
  w2b_eval *e = new w2b_eval;
  e->device = device;
  e->words = words;
  e->size = size;
  e->fused = fused ? 1 : 0;
  e->ld = (size + 15) / 16 * 16;
  e->rows_padded = (words + kTile - 1) / kTile * kTile;
  if (e->rows_padded == 0) e->rows_padded = kTile;
  e->vocab.assign((size_t)(words * kMaxW + kMaxW + 2), 0);
  return e;
}

extern "C" int w2b_eval_load(const char *file, int32_t bitlevel, int64_t threshold, int32_t fused, int32_t device,
                             w2b_eval **out) {
  if (!file || !out) return efail(W2B_EINVAL, "w2b_eval_load: null argument");
  *out = nullptr;
  FILE *f = fopen(file, "rb");
  if (!f) return efail(W2B_EIO, "Input file not found");           // ref :81-84
  std::vector<unsigned char> d;
  {
    fseek(f, 0, SEEK_END);
    const long long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    d.resize(n > 0 ? (size_t)n : 0);
    if (n > 0 && fread(d.data(), 1, (size_t)n, f) != (size_t)n) {
      fclose(f);
      return efail(W2B_EIO, "w2b_eval_load: short read");
    }
    fclose(f);
  }
  if (w2b_internal_is_packed(d.data(), d.size())) {
    // a bit-packed model file (include/word2bits_corpus.h): rebuilt in memory as the bytes of the reference's binary file
    // (ref src/word2bits.cpp:560-576), which then go through the reader below like any other file
    std::vector<std::string> names;
    std::vector<float> values;
    int64_t dim = 0;
    if (w2b_internal_parse_packed(d.data(), d.size(), names, values, &dim) != W2B_OK)
      return efail(W2B_EIO, "w2b_eval_load: damaged bit-packed file");
    std::vector<unsigned char> b;
    char head[64];
    const int hl = snprintf(head, sizeof head, "%lld %lld\n", (long long)names.size(), (long long)dim);
    b.insert(b.end(), head, head + hl);
    for (size_t a = 0; a < names.size(); a++) {
      b.insert(b.end(), names[a].begin(), names[a].end());
      b.push_back(' ');
      const unsigned char *row = (const unsigned char *)(values.data() + a * (size_t)dim);
      b.insert(b.end(), row, row + (size_t)dim * 4);
      b.push_back('\n');
    }
    d.swap(b);
  }
  size_t pos = 0;
  long long words = 0, size = 0;
  if (!scan_ll(d, pos, &words)) return efail(W2B_EIO, "w2b_eval_load: no <words> header");
  if (threshold && words > threshold) words = threshold;            // ref :86
  if (!scan_ll(d, pos, &size)) return efail(W2B_EIO, "w2b_eval_load: no <size> header");
  if (words < 0 || size <= 0 || words > 0x7FFFFF00ll || size > (1 << 24))
    return efail(W2B_EINVAL, "w2b_eval_load: unsupported <words> <size>");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return efail(W2B_ENOGPU, "w2b_eval_load: no HIP device visible (the evaluator has no CPU fallback)");
  if (device < 0 || device >= ndev) return efail(W2B_EINVAL, "w2b_eval_load: bad device index");

  w2b_eval *e = eval_new(words, size, fused, device);
  std::vector<float> raw((size_t)(words * size), 0.f);
  char *vocab = e->vocab.data();
  for (long long b = 0; b < words; b++) {                           // ref :96-105
    read_name(d.data(), d.size(), pos, vocab + b * kMaxW);
    const size_t want = (size_t)size * 4, have = d.size() - pos;
    const size_t take = (want < have ? want : have) / 4 * 4;
    memcpy(raw.data() + b * size, d.data() + pos, take);
    pos = want <= have ? pos + want : d.size();   // a short fread also swallows the 1-3 bytes of a cut float
  }
  d.clear();
  d.shrink_to_fit();
  return eval_finish(e, bitlevel, raw.data(), nullptr, out);
}

// The evaluator on a LIVE trainer: what `compute_accuracy <file> <bitlevel> <threshold>` would load after
// `./word2bits -binary 1` had written <file> from this trainer -- without the file: quantize(u+v) (ref src/word2bits.cpp
// :568-569) is exported on the device straight into the evaluator's matrix, the names go through the same reader
// logic as a file's would (each row of a binary file is "word" + ' ' + floats + '\n', ref :565-574).
extern "C" int w2b_eval_from_trainer(w2b_trainer *t, int64_t n_words, const char *const *words_in, int32_t bitlevel,
                                     int64_t threshold, int32_t fused, w2b_eval **out) {
  if (!t || !out || (n_words > 0 && !words_in)) return efail(W2B_EINVAL, "w2b_eval_from_trainer: null argument");
  *out = nullptr;
  float *u = nullptr, *v = nullptr;
  long long V = 0, D = 0;
  int tb = 0, dev = 0;
  hipStream_t ts = nullptr;
  w2b_internal_trainer_view(t, &u, &v, &V, &D, &tb, &dev, &ts);
  if (n_words != V) return efail(W2B_EINVAL, "w2b_eval_from_trainer: one word per vocabulary row is needed");
  long long words = V;
  if (threshold && words > threshold) words = threshold;            // ref :86
  w2b_eval *e = eval_new(words, D, fused, dev);
  char *vocab = e->vocab.data();
  std::string rowbytes;
  for (long long b = 0; b < words; b++) {
    rowbytes.assign("\n");                                          // what the previous row (or the header) left behind
    rowbytes += words_in[b];
    rowbytes += ' ';
    size_t pos = 0;
    read_name((const unsigned char *)rowbytes.data(), rowbytes.size(), pos, vocab + b * kMaxW);
  }
  if (hipSetDevice(dev) != hipSuccess) { eval_release(e); return efail(W2B_EHIP, "hipSetDevice failed"); }
  float *q = nullptr;
  if (hipMalloc(&q, sizeof(float) * (size_t)(words > 0 ? words : 1) * D) != hipSuccess) {
    eval_release(e);
    return efail(W2B_ENOMEM, "w2b_eval_from_trainer: device allocation failed");
  }
  hipError_t he = w2b_launch_export(u, v, q, words * D, tb, ts);     // quantize(u+v) with the TRAINER's bitlevel
  if (he == hipSuccess) he = hipStreamSynchronize(ts);
  if (he != hipSuccess) {
    (void)hipFree(q);
    eval_release(e);
    return efail(W2B_EHIP, std::string("w2b_eval_from_trainer: ") + hipGetErrorString(he));
  }
  const int rc = eval_finish(e, bitlevel, nullptr, q, out);
  (void)hipFree(q);
  return rc;
}

// ------------------------------------------------------------------------------------ bits mode: the constructors
// device side of the two bits constructors: `host_bits` ([words][wpr], may be unaligned) is uploaded, or the rows are
// produced on the device from the trainer's tables (u != null) on its stream
static int eval_finish_bits(w2b_eval *e, const unsigned char *host_bits, const float *u, const float *v, hipStream_t ts,
                            w2b_eval **out) {
  const long long words = e->words;
  char *vocab = e->vocab.data();
  for (long long b = 0; b < words; b++) e->first.emplace(std::string(vocab + b * kMaxW), b);   // first wins
  auto bail = [&](int rc) { eval_release(e); return rc; };
  if (hipSetDevice(e->device) != hipSuccess) return bail(efail(W2B_EHIP, "hipSetDevice failed"));
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess)
    return bail(efail(W2B_EHIP, "hipStreamCreate failed"));
  const size_t bytes = (size_t)words * (size_t)e->wpr * 8;
  if (hipMalloc(&e->B, bytes ? bytes : 8) != hipSuccess) return bail(efail(W2B_ENOMEM, "w2b_eval: device allocation failed"));
  hipError_t he = hipSuccess;
  if (words > 0 && host_bits) he = hipMemcpy(e->B, host_bits, bytes, hipMemcpyHostToDevice);
  if (words > 0 && u) {
    he = w2b_launch_export_packed(u, v, (unsigned long long *)e->B, words, (int)e->size, 1, ts);
    if (he == hipSuccess) he = hipStreamSynchronize(ts);
  }
  if (he != hipSuccess) return bail(efail(W2B_EHIP, std::string("w2b_eval: ") + hipGetErrorString(he)));
  *out = e;
  return W2B_OK;
}

static w2b_eval *eval_new_bits(long long words, long long size, int32_t device) {
  w2b_eval *e = eval_new(words, size, 1, device);
  e->bits = 1;
  e->wpr = (size + 63) / 64;
  e->ld = 0;
  return e;
}

extern "C" int w2b_eval_load_bits(const char *file, int64_t threshold, int32_t device, w2b_eval **out) {
  if (!file || !out) return efail(W2B_EINVAL, "w2b_eval_load_bits: null argument");
  *out = nullptr;
  FILE *f = fopen(file, "rb");
  if (!f) return efail(W2B_EIO, "Input file not found");           // ref :81-84
  std::vector<unsigned char> d;
  {
    fseek(f, 0, SEEK_END);
    const long long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    d.resize(n > 0 ? (size_t)n : 0);
    if (n > 0 && fread(d.data(), 1, (size_t)n, f) != (size_t)n) {
      fclose(f);
      return efail(W2B_EIO, "w2b_eval_load_bits: short read");
    }
    fclose(f);
  }
  const bool packed = w2b_internal_is_packed(d.data(), d.size());
  std::vector<std::string> names;
  size_t pos = 0;
  long long words = 0, size = 0;
  if (packed) {
    int64_t dim = 0;
    int bitlevel = 0;
    if (w2b_internal_parse_packed_head(d.data(), d.size(), names, &dim, &bitlevel, &pos) != W2B_OK)
      return efail(W2B_EIO, "w2b_eval_load_bits: damaged bit-packed file");
    if (bitlevel != 1)
      return efail(W2B_EINVAL, "w2b_eval_load_bits: a 2-bit model has no integer ranking (rows differ in length); use w2b_eval_load");
    words = (long long)names.size();
    size = dim;
  } else {
    if (!scan_ll(d, pos, &words)) return efail(W2B_EIO, "w2b_eval_load_bits: no <words> header");
    if (!scan_ll(d, pos, &size)) return efail(W2B_EIO, "w2b_eval_load_bits: no <size> header");
  }
  if (threshold && words > threshold) words = threshold;            // ref :86
  if (words < 0 || size <= 0 || words > 0x7FFFFF00ll || size > (1 << 24))
    return efail(W2B_EINVAL, "w2b_eval_load_bits: unsupported <words> <size>");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return efail(W2B_ENOGPU, "w2b_eval_load_bits: no HIP device visible (the evaluator has no CPU fallback)");
  if (device < 0 || device >= ndev) return efail(W2B_EINVAL, "w2b_eval_load_bits: bad device index");

  w2b_eval *e = eval_new_bits(words, size, device);
  char *vocab = e->vocab.data();
  if (packed) {
    // the names as the reader would see them in the float file of the same model ("word" + ' ' after the '\n' before it)
    std::string rowbytes;
    for (long long b = 0; b < words; b++) {
      rowbytes.assign("\n");
      rowbytes += names[(size_t)b];
      rowbytes += ' ';
      size_t p = 0;
      read_name((const unsigned char *)rowbytes.data(), rowbytes.size(), p, vocab + b * kMaxW);
    }
    return eval_finish_bits(e, d.data() + pos, nullptr, nullptr, nullptr, out);   // the file's words, as they are
  }
  // a float file: each row reduced to its signs by the bitlevel-1 rule (ref :26-61: negative iff num < 0)
  std::vector<uint64_t> hb((size_t)(words * e->wpr), 0ull);
  for (long long b = 0; b < words; b++) {                           // ref :96-105
    read_name(d.data(), d.size(), pos, vocab + b * kMaxW);
    const size_t want = (size_t)size * 4, have = d.size() - pos;
    const size_t take = (want < have ? want : have) / 4;
    uint64_t *row = hb.data() + b * e->wpr;
    for (size_t a = 0; a < take; a++) {
      float x;
      memcpy(&x, d.data() + pos + a * 4, 4);
      if (x < 0.f) row[a >> 6] |= 1ull << (a & 63);
    }
    pos = want <= have ? pos + want : d.size();
  }
  return eval_finish_bits(e, (const unsigned char *)hb.data(), nullptr, nullptr, nullptr, out);
}

extern "C" int w2b_eval_bits_from_trainer(w2b_trainer *t, int64_t n_words, const char *const *words_in, int64_t threshold,
                                          w2b_eval **out) {
  if (!t || !out || (n_words > 0 && !words_in)) return efail(W2B_EINVAL, "w2b_eval_bits_from_trainer: null argument");
  *out = nullptr;
  float *u = nullptr, *v = nullptr;
  long long V = 0, D = 0;
  int tb = 0, dev = 0;
  hipStream_t ts = nullptr;
  w2b_internal_trainer_view(t, &u, &v, &V, &D, &tb, &dev, &ts);
  if (tb != 1) return efail(W2B_EINVAL, "w2b_eval_bits_from_trainer: the trainer must be at -bitlevel 1");
  if (n_words != V) return efail(W2B_EINVAL, "w2b_eval_bits_from_trainer: one word per vocabulary row is needed");
  long long words = V;
  if (threshold && words > threshold) words = threshold;            // ref :86
  w2b_eval *e = eval_new_bits(words, D, dev);
  char *vocab = e->vocab.data();
  std::string rowbytes;
  for (long long b = 0; b < words; b++) {
    rowbytes.assign("\n");
    rowbytes += words_in[b];
    rowbytes += ' ';
    size_t pos = 0;
    read_name((const unsigned char *)rowbytes.data(), rowbytes.size(), pos, vocab + b * kMaxW);
  }
  return eval_finish_bits(e, nullptr, u, v, ts, out);
}

extern "C" int32_t w2b_eval_is_bits(const w2b_eval *e) { return e ? e->bits : 0; }

extern "C" int w2b_eval_get_bits(w2b_eval *e, uint64_t *out) {
  if (!e || !out) return efail(W2B_EINVAL, "w2b_eval_get_bits: null argument");
  if (!e->bits) return efail(W2B_EINVAL, "w2b_eval_get_bits: not a bits handle");
  EHIP(hipSetDevice(e->device));
  if (e->words > 0) EHIP(hipMemcpy(out, e->B, (size_t)e->words * (size_t)e->wpr * 8, hipMemcpyDeviceToHost));
  return W2B_OK;
}

// host twin of the bits kernels: I(c) of every row, from the three Hamming distances of the definition
extern "C" int w2b_bits_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int64_t b1, int64_t b2, int64_t b3,
                                    int32_t *I_out) {
  if (!packed || !I_out || words < 0 || dim < 1 || b1 < 0 || b2 < 0 || b3 < 0 || b1 >= words || b2 >= words || b3 >= words)
    return efail(W2B_EINVAL, "w2b_bits_scores_host: bad argument");
  const int64_t wpr = (dim + 63) / 64;
  const uint64_t *r1 = packed + b1 * wpr, *r2 = packed + b2 * wpr, *r3 = packed + b3 * wpr;
  for (int64_t c = 0; c < words; c++) {
    const uint64_t *rc = packed + c * wpr;
    int64_t h1 = 0, h2 = 0, h3 = 0;
    for (int64_t w = 0; w < wpr; w++) {
      const uint64_t valid = (w + 1) * 64 <= dim ? ~0ull : (1ull << (dim - w * 64)) - 1;    // padding bits do not count
      h1 += __builtin_popcountll((r1[w] ^ rc[w]) & valid);
      h2 += __builtin_popcountll((r2[w] ^ rc[w]) & valid);
      h3 += __builtin_popcountll((r3[w] ^ rc[w]) & valid);
    }
    I_out[c] = (int32_t)(dim - 2 * (h2 - h1 + h3));
  }
  return W2B_OK;
}

extern "C" void w2b_eval_free(w2b_eval *e) { eval_release(e); }
extern "C" int64_t w2b_eval_words(const w2b_eval *e) { return e ? e->words : 0; }
extern "C" int64_t w2b_eval_size(const w2b_eval *e) { return e ? e->size : 0; }
extern "C" const char *w2b_eval_word(const w2b_eval *e, int64_t row) {
  if (!e || row < 0 || row >= e->words) return nullptr;
  return e->vocab.data() + row * kMaxW;
}
extern "C" int64_t w2b_eval_lookup(const w2b_eval *e, const char *upper_word) {
  if (!e || !upper_word) return 0;
  auto it = e->first.find(upper_word);
  return it == e->first.end() ? e->words : it->second;
}

extern "C" int w2b_eval_get_matrix(w2b_eval *e, float *out) {
  if (!e || !out) return efail(W2B_EINVAL, "w2b_eval_get_matrix: null argument");
  if (e->bits) return efail(W2B_EINVAL, "w2b_eval_get_matrix: a bits handle holds no float matrix (w2b_eval_get_bits)");
  EHIP(hipSetDevice(e->device));
  if (e->words > 0)
    EHIP(hipMemcpy2D(out, (size_t)e->size * 4, e->M, (size_t)e->ld * 4, (size_t)e->size * 4, (size_t)e->words,
                     hipMemcpyDeviceToHost));
  return W2B_OK;
}

// the per-call buffers of `np` (padded) questions
static int eval_reserve_questions(w2b_eval *e, int64_t np) {
  if (np <= e->cap_q) return W2B_OK;
  if (e->Q) (void)hipFree(e->Q);
  if (e->P) (void)hipFree(e->P);
  if (e->b123) (void)hipFree(e->b123);
  if (e->best) (void)hipFree(e->best);
  e->Q = nullptr; e->P = nullptr; e->b123 = nullptr; e->best = nullptr; e->cap_q = 0;
  const hipError_t qe = e->bits ? hipMalloc(&e->P, (size_t)np * (size_t)e->wpr * 16) : hipMalloc(&e->Q, (size_t)np * e->ld * 4);
  if (qe != hipSuccess || hipMalloc(&e->b123, (size_t)np * 12) != hipSuccess ||
      hipMalloc(&e->best, (size_t)np * 8) != hipSuccess)
    return W2B_ENOMEM;
  e->cap_q = np;
  return W2B_OK;
}

// ------------------------------------------------------------------------------------ bits mode: the scan
// The integer scan of include/word2bits_eval.h ("bits mode") for questions whose rows have been checked; k = 0 is the
// top-1 form (best[nq]), k >= 1 the top-k form (best[nq][k]).  Questions go in chunks; in the top-k form a chunk and
// its row splits are sized so that the slot scratch (splits x k keys per question) stays within the budget, never below
// 128 questions or one split.
static int eval_bits_scan(w2b_eval *e, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3, int32_t k,
                          int32_t *best, float *bestd, const char *who) {
  const int64_t kk = k > 0 ? k : 1;
  const int nw = (int)(2 * e->wpr);
  const uint32_t *B32 = (const uint32_t *)e->B;
  int64_t chunk = kChunkQ;
  int splits = 1, rpb = 1;
  if (k > 0) {
    const int64_t budget = e->tk_budget > 0 ? e->tk_budget : kTopkScratch;
    chunk = nq < kChunkQ ? (nq + 127) / 128 * 128 : kChunkQ;
    if (chunk < 128) chunk = 128;
    for (;;) {
      w2b_bits_layout(e->words, chunk, 1, 0, &splits, &rpb);
      if (chunk * 8 * kk * (splits + 1) <= budget || chunk <= 128) break;
      chunk = chunk / 2 / 128 * 128;
      if (chunk < 128) chunk = 128;
    }
    if (chunk * 8 * kk * (splits + 1) > budget) {
      const int64_t cap = budget / (chunk * 8 * kk) - 1;
      w2b_bits_layout(e->words, chunk, 1, cap > 1 ? (int)cap : 1, &splits, &rpb);
    }
  }
  std::vector<unsigned long long> keys;
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int64_t n = (nq - q0 < chunk) ? nq - q0 : chunk;
    const int64_t np = (n + kTile - 1) / kTile * kTile;
    if (eval_reserve_questions(e, np) != W2B_OK) return efail(W2B_ENOMEM, std::string(who) + ": device allocation failed");
    unsigned long long *merged = e->best, *slots = nullptr;
    if (k > 0) {
      const size_t need = (size_t)n * 8 * kk * (size_t)(splits + 1);
      if (need > e->tk_bytes) {
        if (e->tk_buf) (void)hipFree(e->tk_buf);
        e->tk_buf = nullptr;
        e->tk_bytes = 0;
        if (hipMalloc(&e->tk_buf, need) != hipSuccess) return efail(W2B_ENOMEM, std::string(who) + ": device allocation failed");
        e->tk_bytes = need;
      }
      merged = (unsigned long long *)e->tk_buf;
      slots = merged + n * kk;
    }
    int32_t *d1 = e->b123, *d2 = e->b123 + np, *d3 = e->b123 + 2 * np;
    EHIP(hipMemcpyAsync(d1, b1 + q0, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemcpyAsync(d2, b2 + q0, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemcpyAsync(d3, b3 + q0, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    if (k == 0) EHIP(hipMemsetAsync(e->best, 0, (size_t)np * 8, e->stream));
    hipEvent_t t0, t1;
    EHIP(hipEventCreate(&t0));
    EHIP(hipEventCreate(&t1));
    EHIP(hipEventRecord(t0, e->stream));
    hipError_t le = w2b_launch_bits_planes(B32, nw, (int)e->size, (int)n, np, d1, d2, d3, e->P, e->stream);
    if (le == hipSuccess)
      le = k == 0 ? w2b_launch_bits_top1(B32, (int)e->words, (int)e->size, e->P, np, (int)n, d1, d2, d3, e->best, e->stream)
                  : w2b_launch_bits_topk(B32, (int)e->words, (int)e->size, e->P, np, (int)n, d1, d2, d3, k, splits, rpb, slots,
                                         merged, e->stream);
    if (le == hipSuccess) le = hipEventRecord(t1, e->stream);
    keys.assign((size_t)(n * kk), 0ull);   // (no rows: nothing is launched and every list is empty)
    if (le == hipSuccess && e->words > 0)
      le = hipMemcpyAsync(keys.data(), merged, (size_t)(n * kk) * 8, hipMemcpyDeviceToHost, e->stream);
    if (le == hipSuccess) le = hipStreamSynchronize(e->stream);
    float ms = 0;
    if (le == hipSuccess) le = hipEventElapsedTime(&ms, t0, t1);
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    if (le != hipSuccess) return efail(W2B_EHIP, std::string(who) + ": " + hipGetErrorString(le));
    e->kernel_ms += ms;
    e->launches++;
    e->macs += (double)n * (double)e->words * (double)e->size;
    for (int64_t i = 0; i < n * kk; i++) {
      const unsigned long long key = keys[(size_t)i];
      best[q0 * kk + i] = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)) : -1;
      if (bestd) bestd[q0 * kk + i] = (float)(int32_t)(key >> 32) / (float)e->size;   // one correctly rounded division
    }
  }
  return W2B_OK;
}

extern "C" int w2b_eval_top1(w2b_eval *e, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3,
                             int32_t *best, float *bestd) {
  if (!e || nq < 0 || (nq > 0 && (!b1 || !b2 || !b3 || !best)))
    return efail(W2B_EINVAL, "w2b_eval_top1: bad argument");
  for (int64_t q = 0; q < nq; q++)
    if (b1[q] < 0 || b1[q] >= e->words || b2[q] < 0 || b2[q] >= e->words || b3[q] < 0 || b3[q] >= e->words)
      return efail(W2B_EINVAL, "w2b_eval_top1: question row out of range");
  EHIP(hipSetDevice(e->device));
  if (e->bits) return eval_bits_scan(e, nq, b1, b2, b3, 0, best, bestd, "w2b_eval_top1");
  std::vector<unsigned long long> keys;
  for (int64_t q0 = 0; q0 < nq; q0 += kChunkQ) {
    const int64_t n = (nq - q0 < kChunkQ) ? nq - q0 : kChunkQ;
    const int64_t np = (n + kTile - 1) / kTile * kTile;
    if (eval_reserve_questions(e, np) != W2B_OK) return efail(W2B_ENOMEM, "w2b_eval_top1: device allocation failed");
    int32_t *d1 = e->b123, *d2 = e->b123 + np, *d3 = e->b123 + 2 * np;
    EHIP(hipMemcpyAsync(d1, b1 + q0, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemcpyAsync(d2, b2 + q0, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemcpyAsync(d3, b3 + q0, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemsetAsync(e->Q, 0, (size_t)np * e->ld * 4, e->stream));
    EHIP(hipMemsetAsync(e->best, 0, (size_t)np * 8, e->stream));
    EHIP(w2b_launch_eval_queries(e->M, e->ld, n, d1, d2, d3, e->Q, e->variant, e->stream));
    hipEvent_t t0, t1;
    EHIP(hipEventCreate(&t0));
    EHIP(hipEventCreate(&t1));
    EHIP(hipEventRecord(t0, e->stream));
    hipError_t le = w2b_launch_eval_scores(e->Q, e->M, (int)n, (int)e->words, (int)e->size, (int)e->ld, e->fused, d1, d2, d3,
                                           e->best, e->variant, e->stream);
    if (le == hipSuccess) le = hipEventRecord(t1, e->stream);
    keys.resize((size_t)n);
    if (le == hipSuccess) le = hipMemcpyAsync(keys.data(), e->best, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream);
    if (le == hipSuccess) le = hipStreamSynchronize(e->stream);
    float ms = 0;
    if (le == hipSuccess) le = hipEventElapsedTime(&ms, t0, t1);
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    if (le != hipSuccess) return efail(W2B_EHIP, std::string("w2b_eval_top1: ") + hipGetErrorString(le));
    e->kernel_ms += ms;
    e->launches++;
    e->macs += (double)n * (double)e->words * (double)e->size;   // algorithmic: padding is not work
    for (int64_t q = 0; q < n; q++) {
      const unsigned long long k = keys[(size_t)q];
      best[q0 + q] = k ? (int32_t)(0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull)) : -1;
      if (bestd) {
        const uint32_t bits = (uint32_t)(k >> 32);
        memcpy(&bestd[q0 + q], &bits, 4);
      }
    }
  }
  return W2B_OK;
}


// ------------------------------------------------------------------------------------ top-k
// ref :155-177 with N = k.  The questions go through the scan in chunks sized so that the slot scratch of one launch
// (w2b_internal.h) stays within the budget; a chunk is never smaller than one 128-question tile.
static int eval_topk(w2b_eval *e, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3, int32_t k,
                     int32_t *best, float *bestd, const char *who) {
  if (!e || nq < 0 || (nq > 0 && (!b1 || !b2 || !b3 || !best)))
    return efail(W2B_EINVAL, std::string(who) + ": bad argument");
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, std::string(who) + ": k must be 1..64");
  for (int64_t q = 0; q < nq; q++)
    if (b1[q] < 0 || b1[q] >= e->words || b2[q] < 0 || b2[q] >= e->words || b3[q] < 0 || b3[q] >= e->words)
      return efail(W2B_EINVAL, std::string(who) + ": question row out of range");
  EHIP(hipSetDevice(e->device));
  if (e->bits) return eval_bits_scan(e, nq, b1, b2, b3, k, best, bestd, who);
  int nunits = 0, cap = 0;
  w2b_eval_topk_layout(e->words, k, e->fused && e->variant != 0, &nunits, &cap);
  // per question: bound + k buckets + one byte per slot (zeroed together), k merged keys, nunits slots of cap keys
  const int64_t zero_q = 8 + 8 * (int64_t)k + nunits, per_q = zero_q + 8 * (int64_t)k + 8 * (int64_t)nunits * cap;
  const int64_t budget = e->tk_budget > 0 ? e->tk_budget : kTopkScratch;
  int64_t chunk = budget / per_q / 128 * 128;
  if (chunk < 128) chunk = 128;
  if (chunk > kChunkQ) chunk = kChunkQ;
  std::vector<unsigned long long> keys;
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int64_t n = (nq - q0 < chunk) ? nq - q0 : chunk;
    const int64_t np = (n + kTile - 1) / kTile * kTile;
    if (eval_reserve_questions(e, np) != W2B_OK) return efail(W2B_ENOMEM, std::string(who) + ": device allocation failed");
    const size_t zero_bytes = ((size_t)n * zero_q + 7) / 8 * 8, need = (size_t)n * per_q + 8;
    if (need > e->tk_bytes) {
      if (e->tk_buf) (void)hipFree(e->tk_buf);
      e->tk_buf = nullptr;
      e->tk_bytes = 0;
      if (hipMalloc(&e->tk_buf, need) != hipSuccess) return efail(W2B_ENOMEM, std::string(who) + ": device allocation failed");
      e->tk_bytes = need;
    }
    unsigned long long *bound = (unsigned long long *)e->tk_buf, *bkt = bound + n;
    unsigned char *cnt = (unsigned char *)(bkt + n * k);
    unsigned long long *merged = (unsigned long long *)((char *)e->tk_buf + zero_bytes), *slots = merged + n * k;
    int32_t *d1 = e->b123, *d2 = e->b123 + np, *d3 = e->b123 + 2 * np;
    EHIP(hipMemcpyAsync(d1, b1 + q0, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemcpyAsync(d2, b2 + q0, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemcpyAsync(d3, b3 + q0, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemsetAsync(e->Q, 0, (size_t)np * e->ld * 4, e->stream));
    EHIP(hipMemsetAsync(e->tk_buf, 0, zero_bytes, e->stream));
    EHIP(w2b_launch_eval_queries(e->M, e->ld, n, d1, d2, d3, e->Q, e->variant, e->stream));
    hipEvent_t t0, t1;
    EHIP(hipEventCreate(&t0));
    EHIP(hipEventCreate(&t1));
    EHIP(hipEventRecord(t0, e->stream));
    hipError_t le = w2b_launch_eval_topk(e->Q, e->M, (int)n, (int)e->words, (int)e->size, (int)e->ld, e->fused, d1, d2, d3,
                                         k, bound, bkt, slots, cnt, merged, e->variant, e->stream);
    if (le == hipSuccess) le = hipEventRecord(t1, e->stream);
    keys.assign((size_t)n * k, 0ull);   // (no rows: nothing is launched and every list is empty)
    if (le == hipSuccess && e->words > 0)
      le = hipMemcpyAsync(keys.data(), merged, (size_t)n * k * 8, hipMemcpyDeviceToHost, e->stream);
    if (le == hipSuccess) le = hipStreamSynchronize(e->stream);
    float ms = 0;
    if (le == hipSuccess) le = hipEventElapsedTime(&ms, t0, t1);
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    if (le != hipSuccess) return efail(W2B_EHIP, std::string(who) + ": " + hipGetErrorString(le));
    e->kernel_ms += ms;
    e->launches++;
    e->macs += (double)n * (double)e->words * (double)e->size;
    for (int64_t i = 0; i < n * k; i++) {
      const unsigned long long key = keys[(size_t)i];
      best[q0 * k + i] = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)) : -1;
      if (bestd) {
        const uint32_t bits = (uint32_t)(key >> 32);
        memcpy(&bestd[q0 * k + i], &bits, 4);
      }
    }
  }
  return W2B_OK;
}

extern "C" int w2b_eval_topk(w2b_eval *e, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3,
                             int32_t k, int32_t *best, float *bestd) {
  return eval_topk(e, nq, b1, b2, b3, k, best, bestd, "w2b_eval_topk");
}

// vec = (M[r] - M[r]) + M[r]: M[r] up to the sign of a zero, which no chain that starts at +0 can see
extern "C" int w2b_eval_neighbors(w2b_eval *e, int64_t nq, const int32_t *rows, int32_t k, int32_t *best, float *bestd) {
  return eval_topk(e, nq, rows, rows, rows, k, best, bestd, "w2b_eval_neighbors");
}

extern "C" int w2b_eval_set_topk_scratch(w2b_eval *e, int64_t bytes) {
  if (!e || bytes < 0) return efail(W2B_EINVAL, "w2b_eval_set_topk_scratch: bad argument");
  e->tk_budget = bytes;
  return W2B_OK;
}

extern "C" int w2b_eval_set_kernel(w2b_eval *e, int32_t variant) {
  if (!e) return efail(W2B_EINVAL, "w2b_eval_set_kernel: null evaluator");
  if (e->bits) return W2B_OK;                                         // one kernel: nothing to select
  if (variant < 0 || variant > 64) return efail(W2B_EINVAL, "w2b_eval_set_kernel: variant must be 0..64");
  e->variant = variant;
  return W2B_OK;
}

extern "C" int w2b_eval_timing_read(w2b_eval *e, double *kernel_ms, int64_t *launches, double *macs) {
  if (!e) return efail(W2B_EINVAL, "w2b_eval_timing_read: null handle");
  EHIP(hipSetDevice(e->device));
  const double ms = e->kernel_ms;
  e->kernel_ms = 0;
  if (kernel_ms) *kernel_ms = ms;
  if (launches) *launches = e->launches;
  if (macs) *macs = e->macs;
  e->launches = 0;
  e->macs = 0;
  return W2B_OK;
}

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
}  // namespace

extern "C" int w2b_eval_transcript(w2b_eval *e, const char *questions, int64_t len, char **out, int64_t *out_len) {
  if (!e || !out || len < 0 || (len > 0 && !questions)) return efail(W2B_EINVAL, "w2b_eval_transcript: bad argument");
  *out = nullptr;
  TokenIn in{questions, len};
  std::string st1, st2, st3, st4;
  std::vector<Step> steps;
  std::vector<int32_t> b1s, b2s, b3s;
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
    if (r1 == e->words || r2 == e->words || r3 == e->words) continue;  // ref :149-151
    if (w2b_eval_lookup(e, st4.c_str()) == e->words) continue;          // ref :152-153
    TQS++;
    steps.push_back({Step::Question, QID, st4, (int64_t)b1s.size()});
    b1s.push_back((int32_t)r1);
    b2s.push_back((int32_t)r2);
    b3s.push_back((int32_t)r3);
  }
  // the scan of ref :155-177 for all of them at once, on the GPU
  std::vector<int32_t> best(b1s.size());
  if (!b1s.empty()) {
    const int rc = w2b_eval_top1(e, (int64_t)b1s.size(), b1s.data(), b2s.data(), b3s.data(), best.data(), nullptr);
    if (rc != W2B_OK) return rc;
  }
  // pass 2: replay the counters and print (ref :120-131,178-187)
  std::string txt = "Starting eval...\n";
  int TCN = 0, CCN = 0, TACN = 0, CACN = 0, SECN = 0, SYCN = 0, SEAC = 0, SYAC = 0;
  for (const Step &s : steps) {
    if (s.kind == Step::SectionEnd) {
      if (TCN == 0) TCN = 1;
      if (s.qid != 0) {
        appendf(txt, "ACCURACY TOP1: %.2f %%  (%d / %d)\n", CCN / (float)TCN * 100, CCN, TCN);
        appendf(txt, "Total accuracy: %.2f %%   Semantic accuracy: %.2f %%   Syntactic accuracy: %.2f %% \n",
                CACN / (float)TACN * 100, SEAC / (float)SECN * 100, SYAC / (float)SYCN * 100);
      }
    } else if (s.kind == Step::SectionName) {
      txt += s.text;
      txt += ":\n";
      TCN = 0;
      CCN = 0;
    } else {
      const int32_t c = best[(size_t)s.q];
      const char *bestw = c >= 0 ? e->vocab.data() + (int64_t)c * kMaxW : "";
      if (s.text == bestw) {                                           // strcmp on the words (ref :178)
        CCN++;
        CACN++;
        if (s.qid <= 5) SEAC++; else SYAC++;
      }
      if (s.qid <= 5) SECN++; else SYCN++;
      TCN++;
      TACN++;
    }
  }
  appendf(txt, "Questions seen / total: %d %d   %.2f %% \n", TQS, TQ, TQS / (float)TQ * 100);
  char *buf = (char *)malloc(txt.size() + 1);
  if (!buf) return efail(W2B_ENOMEM, "w2b_eval_transcript: out of memory");
  memcpy(buf, txt.data(), txt.size());
  buf[txt.size()] = 0;
  *out = buf;
  if (out_len) *out_len = (int64_t)txt.size();
  return W2B_OK;
}


// ------------------------------------------------------------------------------------ nearest: the text form
extern "C" int w2b_eval_nearest_text(w2b_eval *e, const char *queries, int64_t len, int32_t k, char **out,
                                     int64_t *out_len) {
  if (!e || !out || len < 0 || (len > 0 && !queries)) return efail(W2B_EINVAL, "w2b_eval_nearest_text: bad argument");
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, "w2b_eval_nearest_text: k must be 1..64");
  *out = nullptr;
  struct Line { std::string head; std::string error; int64_t q; };
  std::vector<Line> lines;
  std::vector<int32_t> b1s, b2s, b3s;
  for (int64_t pos = 0; pos < len;) {
    int64_t end = pos;
    while (end < len && queries[end] != '\n') end++;
    std::vector<std::string> tok;
    for (int64_t i = pos; i < end;) {
      while (i < end && is_space((unsigned char)queries[i])) i++;
      const int64_t s0 = i;
      while (i < end && !is_space((unsigned char)queries[i])) i++;
      if (i > s0) {
        tok.emplace_back(queries + s0, (size_t)(i - s0));
        upper_inplace(tok.back());                                  // ref :118
      }
    }
    pos = end + 1;
    if (tok.empty()) continue;
    Line ln{std::string(), std::string(), -1};
    for (size_t i = 0; i < tok.size(); i++) ln.head += (i ? " " : "") + tok[i];
    if (tok.size() != 1 && tok.size() != 3) {
      ln.error = "expected 1 or 3 words";
    } else {
      int64_t r[3] = {0, 0, 0};
      for (size_t i = 0; i < tok.size() && ln.error.empty(); i++) {
        r[i] = w2b_eval_lookup(e, tok[i].c_str());
        if (r[i] == e->words) ln.error = "not in vocabulary: " + tok[i];
      }
      if (ln.error.empty()) {
        if (tok.size() == 1) r[1] = r[2] = r[0];
        ln.q = (int64_t)b1s.size();
        b1s.push_back((int32_t)r[0]);
        b2s.push_back((int32_t)r[1]);
        b3s.push_back((int32_t)r[2]);
      }
    }
    lines.push_back(ln);
  }
  std::vector<int32_t> best(b1s.size() * (size_t)k);
  std::vector<float> bestd(b1s.size() * (size_t)k);
  if (!b1s.empty()) {
    const int rc = w2b_eval_topk(e, (int64_t)b1s.size(), b1s.data(), b2s.data(), b3s.data(), k, best.data(), bestd.data());
    if (rc != W2B_OK) return rc;
  }
  std::string txt;
  for (const Line &ln : lines) {
    txt += ln.head;
    if (!ln.error.empty()) {
      txt += ": " + ln.error + "\n";
      continue;
    }
    txt += ":\n";
    for (int j = 0; j < k; j++) {
      const int32_t c = best[(size_t)(ln.q * k + j)];
      if (c < 0) break;
      appendf(txt, "%d\t%s\t%.6f\n", j + 1, e->vocab.data() + (int64_t)c * kMaxW, (double)bestd[(size_t)(ln.q * k + j)]);
    }
  }
  char *buf = (char *)malloc(txt.size() + 1);
  if (!buf) return efail(W2B_ENOMEM, "w2b_eval_nearest_text: out of memory");
  memcpy(buf, txt.data(), txt.size());
  buf[txt.size()] = 0;
  *out = buf;
  if (out_len) *out_len = (int64_t)txt.size();
  return W2B_OK;
}

extern "C" void w2b_eval_free_text(char *text) { free(text); }
