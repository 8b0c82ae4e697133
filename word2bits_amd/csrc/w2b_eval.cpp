// w2b_eval.cpp -- host side of include/word2bits_eval.h: the vector-file reader, the question-stream state
// machine and the stdout transcript of the reference evaluator (ref src/compute-accuracy.c:80-188), around the
// GPU scans in w2b_kernels_eval.hip (fp32 rows), w2b_kernels_evalbits.hip (bit-packed 1-bit rows) and
// w2b_kernels_evalcodes.hip (bit-packed 2-bit rows); w2b_kernels_evalcombine.hip has what the signed multi-word question
// adds to the first two, w2b_kernels_evalbag.hip the bag question on both packed forms, w2b_kernels_evalvec.hip
// the float-vector question on them, w2b_kernels_evalcosmul.hip the 3CosMul scan on 1-bit rows, w2b_kernels_evalclasses.hip the
// k-means word classes on both packed forms (whose wq = 1 / sqrt(N_k) the host builds like the bag question's), w2b_kernels_evaldocs.hip the document question on them, w2b_kernels_evalpairs.hip the pair question (whose cosine the host builds from the three integers the device sums, and whose rank correlations are host arithmetic in double).  No arithmetic on scores happens here (the exceptions are question weights: the bag
// question's 1 / sqrt(N_T), built from the integer the device sums, and the vector question's wx with the fp32 handle's
// vec = x * wx; and the 3CosMul table u = A / size of a bits handle) and there is no CPU fallback (w2b_codes_scores_host,
// w2b_bag_scores_host, w2b_vector_scores_host, w2b_cosmul_scores_host, w2b_classes_host, w2b_docs_scores_host and w2b_pairs_host are the tests' twins of the kernels).
#include "../../include/word2bits_eval.h"
#include "../../include/word2bits_hip.h"
#include "w2b_internal.h"
#include "w2b_evalclasses.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <locale.h>
#include <memory>
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
  uint64_t *B = nullptr;                                // [words][wpr], the file's layout (both packed modes)
  uint32_t *P = nullptr;                                // per-call, bits: the questions' planes [2 * 2 * wpr][cap_q];
                                                        // codes: their int8 operands (w2b_codes_operand_bytes)
  // codes mode (w2b_eval_load_codes / w2b_eval_codes_from_trainer): 2-bit rows packed in B; Q holds the questions'
  // weights [3][cap_q]
  int codes = 0;
  float *wrow = nullptr;                                // [rows_padded] w(c), 0 past the vocabulary
  float *utab = nullptr;                                // bits, w2b_eval_cosmul: u by agreement count [size + 1] (made on first use)
  // per-call scratch (grown on demand)
  float *Q = nullptr;
  int32_t *b123 = nullptr;
  // w2b_eval_combine: the questions' rows and signs, each [cap_t][W2B_EVAL_XSTRIDE], and (bits) their four planes
  int32_t *terms = nullptr;
  uint32_t *P4 = nullptr;                               // [4 * 2 * wpr][cap_t]
  int64_t cap_t = 0;
  // w2b_eval_bag: the chunk's bags (weights, ids, bounds, own rows) and the questions' digit planes; w2b_eval_vectors on a
  // packed handle: the chunk's weights and vectors, and their operands in fragment order
  void *bag_buf = nullptr, *bag_T = nullptr;
  size_t bag_bytes = 0, bag_T_bytes = 0;
  unsigned long long *best = nullptr;
  int64_t cap_q = 0;
  double kernel_ms = 0;                                 // score-kernel time since the last timing_read
  int64_t launches = 0;
  double macs = 0;
  double cls_assign_ms = 0, cls_sums_ms = 0;             // w2b_eval_classes: the two shares of its last call's device time
  // w2b_eval_docs: the corpus of w2b_eval_docs_set WITHOUT its padding ids, its bounds [docs_n + 1], the positions it was given
  // with (padding included: the multiply-add count), per-call buffers, and the two shares of the last call's device time
  int32_t *docs_ids = nullptr;
  long long *docs_off = nullptr;
  int64_t docs_n = 0, docs_positions = 0;
  double docs_table_ms = 0, docs_walk_ms = 0;
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
  if (e->wrow) (void)hipFree(e->wrow);
  if (e->utab) (void)hipFree(e->utab);
  if (e->docs_ids) (void)hipFree(e->docs_ids);
  if (e->docs_off) (void)hipFree(e->docs_off);
  if (e->P) (void)hipFree(e->P);
  if (e->Q) (void)hipFree(e->Q);
  if (e->b123) (void)hipFree(e->b123);
  if (e->terms) (void)hipFree(e->terms);
  if (e->P4) (void)hipFree(e->P4);
  if (e->bag_buf) (void)hipFree(e->bag_buf);
  if (e->bag_T) (void)hipFree(e->bag_T);
  if (e->best) (void)hipFree(e->best);
  if (e->tk_buf) (void)hipFree(e->tk_buf);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

namespace {
// a handle under construction: released on every exit that does not hand it to the caller
struct EvalRelease { void operator()(w2b_eval *e) const { eval_release(e); } };
using EvalPtr = std::unique_ptr<w2b_eval, EvalRelease>;
// a device allocation that lives for one constructor call
struct DeviceTemp {
  float *p = nullptr;
  ~DeviceTemp() { if (p) (void)hipFree(p); }
};
}  // namespace

// ------------------------------------------------------------------------------------ the file reader
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

// One row of a float file (ref :96-105): its name into the vocabulary, then `size` floats.  Returns how many whole
// floats of them the file still holds, at *values.
static size_t read_row(const std::vector<unsigned char> &d, size_t &pos, long long size, char *name,
                       const unsigned char **values) {
  read_name(d.data(), d.size(), pos, name);
  const size_t want = (size_t)size * 4, have = d.size() - pos;
  *values = d.data() + pos;
  pos = want <= have ? pos + want : d.size();   // a short fread also swallows the 1-3 bytes of a cut float
  return (want < have ? want : have) / 4;
}

// The names of rows that come without a file, as the reader would see them in the float file of the same model: each
// row of a binary file is "word" + ' ' + floats + '\n' (ref src/word2bits.cpp:565-574), so a name starts after the '\n'
// that the previous row (or the header) left behind.
template <class Get>
static void names_from_words(w2b_eval *e, long long count, Get word) {
  for (long long b = 0; b < count; b++) {
    const std::string rowbytes = std::string("\n") + word(b) + ' ';
    size_t pos = 0;
    read_name((const unsigned char *)rowbytes.data(), rowbytes.size(), pos, e->vocab.data() + b * kMaxW);
  }
}

static int read_whole_file(const char *path, const std::string &who, std::vector<unsigned char> &bytes) {
  FILE *f = fopen(path, "rb");
  if (!f) return efail(W2B_EIO, "Input file not found");           // ref :81-84
  fseek(f, 0, SEEK_END);
  const long long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  bytes.resize(n > 0 ? (size_t)n : 0);
  const bool ok = n <= 0 || fread(bytes.data(), 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  return ok ? W2B_OK : efail(W2B_EIO, who + ": short read");
}

namespace {
struct VectorFile {
  std::vector<unsigned char> d;
  long long words = 0, size = 0;        // <words> after the threshold (ref :86), <size>
  size_t pos = 0;                       // the first row
  bool packed = false;                  // the rows at `pos` are the packed words of a .w2bp, their names are in `names`
  std::vector<std::string> names;
};
}  // namespace

// What both loaders do before they read rows.  A bit-packed model file (include/word2bits_corpus.h) keeps its rows
// packed when `keep_packed` (the bitlevel that the caller scans in packed form: 1 or 2); otherwise it is rebuilt in memory as the bytes of the reference's binary file (ref
// src/word2bits.cpp:560-576), which then go through the reader like any other file.  Everything that is wrong with the
// file is reported before a device is asked for.
static int open_vector_file(const char *file, int keep_packed, int64_t threshold, int32_t device, const std::string &who,
                            VectorFile &f) {
  if (int rc = read_whole_file(file, who, f.d)) return rc;
  f.packed = keep_packed != 0 && w2b_internal_is_packed(f.d.data(), f.d.size());
  if (f.packed) {
    int64_t dim = 0;
    int bitlevel = 0;
    if (w2b_internal_parse_packed_head(f.d.data(), f.d.size(), f.names, &dim, &bitlevel, &f.pos) != W2B_OK)
      return efail(W2B_EIO, who + ": damaged bit-packed file");
    if (keep_packed == 1 && bitlevel != 1)
      return efail(W2B_EINVAL, who + ": a 2-bit model has no integer ranking (rows differ in length); use w2b_eval_load");
    if (keep_packed == 2 && bitlevel != 2)
      return efail(W2B_EINVAL, who + ": a 1-bit model is scanned in bits mode (w2b_eval_load_bits, `bits`)");
    f.words = (long long)f.names.size();
    f.size = dim;
  } else {
    if (w2b_internal_is_packed(f.d.data(), f.d.size())) {
      std::vector<std::string> names;
      std::vector<float> values;
      int64_t dim = 0;
      if (w2b_internal_parse_packed(f.d.data(), f.d.size(), names, values, &dim) != W2B_OK)
        return efail(W2B_EIO, who + ": damaged bit-packed file");
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
      f.d.swap(b);
    }
    if (!scan_ll(f.d, f.pos, &f.words)) return efail(W2B_EIO, who + ": no <words> header");
    if (!scan_ll(f.d, f.pos, &f.size)) return efail(W2B_EIO, who + ": no <size> header");
  }
  if (threshold && f.words > threshold) f.words = threshold;       // ref :86
  if (f.words < 0 || f.size <= 0 || f.words > 0x7FFFFF00ll || f.size > (1 << 24))
    return efail(W2B_EINVAL, who + ": unsupported <words> <size>");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return efail(W2B_ENOGPU, who + ": no HIP device visible (the evaluator has no CPU fallback)");
  if (device < 0 || device >= ndev) return efail(W2B_EINVAL, who + ": bad device index");
  return W2B_OK;
}

// ------------------------------------------------------------------------------------ the constructors
// `packed`: 0 = fp32 rows, 1 = bits mode, 2 = codes mode
static EvalPtr eval_new(long long words, long long size, int32_t fused, int32_t device, int packed) {
  EvalPtr e(new w2b_eval);
  e->device = device;
  e->words = words;
  e->size = size;
  e->fused = fused ? 1 : 0;
  e->bits = packed == 1;
  e->codes = packed == 2;
  e->wpr = (size + 63) / 64 * packed;
  e->ld = packed ? 0 : (size + 15) / 16 * 16;
  e->rows_padded = (words + kTile - 1) / kTile * kTile;
  if (e->rows_padded == 0) e->rows_padded = kTile;
  e->vocab.assign((size_t)(words * kMaxW + kMaxW + 2), 0);
  return e;
}

// once the names are in: the lookup table, the device and the handle's stream
static int eval_open_device(w2b_eval *e) {
  for (long long b = 0; b < e->words; b++) e->first.emplace(std::string(e->vocab.data() + b * kMaxW), b);   // first wins
  if (hipSetDevice(e->device) != hipSuccess) return efail(W2B_EHIP, "hipSetDevice failed");
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess)
    return efail(W2B_EHIP, "hipStreamCreate failed");
  return W2B_OK;
}

// common tail of the two fp32 constructors: device buffers, quantize(x, bitlevel) + normalisation of the rows (ref
// :106-110).  `rows` ([words][size], on the host or on the device as `kind` says) holds the raw values.
static int eval_finish(EvalPtr e, int32_t bitlevel, const float *rows, hipMemcpyKind kind, w2b_eval **out) {
  if (int rc = eval_open_device(e.get())) return rc;
  const long long words = e->words, size = e->size;
  const size_t mbytes = (size_t)e->rows_padded * e->ld * 4;
  DeviceTemp len;
  if (hipMalloc(&e->M, mbytes) != hipSuccess || hipMalloc(&len.p, (size_t)(words + 1) * 4) != hipSuccess)
    return efail(W2B_ENOMEM, "w2b_eval: device allocation failed");
  hipError_t he = hipMemsetAsync(e->M, 0, mbytes, e->stream);
  if (he == hipSuccess && words > 0)
    he = hipMemcpy2DAsync(e->M, (size_t)e->ld * 4, rows, (size_t)size * 4, (size_t)size * 4, (size_t)words, kind, e->stream);
  if (he == hipSuccess) he = w2b_launch_eval_normalize(e->M, words, size, e->ld, bitlevel, e->fused, len.p, e->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
  if (he != hipSuccess) return efail(W2B_EHIP, std::string("w2b_eval: ") + hipGetErrorString(he));
  *out = e.release();
  return W2B_OK;
}

// w(r) by n3 (include/word2bits_eval.h, "codes mode"): (float)(1.0 / sqrt((double)(dim + 8 n3))), n3 = 0..dim
static std::vector<float> codes_weights(int64_t dim) {
  std::vector<float> w((size_t)dim + 1);
  for (int64_t n3 = 0; n3 <= dim; n3++) w[(size_t)n3] = (float)(1.0 / sqrt((double)(dim + 8 * n3)));
  return w;
}

// common tail of the bits and codes constructors: `host_bits` ([words][wpr], may be unaligned) is uploaded, or the rows
// are produced on the device from the trainer's tables (u != null) on its stream; codes: then w(c) of every row
static int eval_finish_bits(EvalPtr e, const unsigned char *host_bits, const float *u, const float *v, hipStream_t ts,
                            w2b_eval **out) {
  if (int rc = eval_open_device(e.get())) return rc;
  const long long words = e->words;
  const size_t bytes = (size_t)words * (size_t)e->wpr * 8;
  if (hipMalloc(&e->B, bytes ? bytes : 8) != hipSuccess) return efail(W2B_ENOMEM, "w2b_eval: device allocation failed");
  hipError_t he = hipSuccess;
  if (words > 0 && host_bits) he = hipMemcpy(e->B, host_bits, bytes, hipMemcpyHostToDevice);
  if (words > 0 && u) {
    he = w2b_launch_export_packed(u, v, (unsigned long long *)e->B, words, (int)e->size, e->codes ? 2 : 1, ts);
    if (he == hipSuccess) he = hipStreamSynchronize(ts);
  }
  DeviceTemp wtab;
  if (he == hipSuccess && e->codes) {
    const std::vector<float> w = codes_weights(e->size);
    if (hipMalloc(&e->wrow, (size_t)e->rows_padded * 4) != hipSuccess || hipMalloc(&wtab.p, w.size() * 4) != hipSuccess)
      return efail(W2B_ENOMEM, "w2b_eval: device allocation failed");
    he = hipMemcpy(wtab.p, w.data(), w.size() * 4, hipMemcpyHostToDevice);
    if (he == hipSuccess)
      he = w2b_launch_codes_roww((const uint32_t *)e->B, (int)e->size, words, e->rows_padded, wtab.p, e->wrow, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
  }
  if (he != hipSuccess) return efail(W2B_EHIP, std::string("w2b_eval: ") + hipGetErrorString(he));
  *out = e.release();
  return W2B_OK;
}

extern "C" int w2b_eval_load(const char *file, int32_t bitlevel, int64_t threshold, int32_t fused, int32_t device,
                             w2b_eval **out) {
  if (!file || !out) return efail(W2B_EINVAL, "w2b_eval_load: null argument");
  *out = nullptr;
  VectorFile f;
  if (int rc = open_vector_file(file, 0, threshold, device, "w2b_eval_load", f)) return rc;
  EvalPtr e = eval_new(f.words, f.size, fused, device, 0);
  std::vector<float> raw((size_t)(f.words * f.size), 0.f);
  for (long long b = 0; b < f.words; b++) {
    const unsigned char *values;
    const size_t take = read_row(f.d, f.pos, f.size, e->vocab.data() + b * kMaxW, &values);
    memcpy(raw.data() + b * f.size, values, take * 4);
  }
  f.d.clear();
  f.d.shrink_to_fit();
  return eval_finish(std::move(e), bitlevel, raw.data(), hipMemcpyHostToDevice, out);
}

extern "C" int w2b_eval_load_bits(const char *file, int64_t threshold, int32_t device, w2b_eval **out) {
  if (!file || !out) return efail(W2B_EINVAL, "w2b_eval_load_bits: null argument");
  *out = nullptr;
  VectorFile f;
  if (int rc = open_vector_file(file, 1, threshold, device, "w2b_eval_load_bits", f)) return rc;
  EvalPtr e = eval_new(f.words, f.size, 1, device, 1);
  if (f.packed) {
    names_from_words(e.get(), f.words, [&](long long b) -> const std::string & { return f.names[(size_t)b]; });
    // the file's words, as they are
    return eval_finish_bits(std::move(e), f.d.data() + f.pos, nullptr, nullptr, nullptr, out);
  }
  // a float file: each row reduced to its signs by the bitlevel-1 rule (ref :26-61: negative iff num < 0)
  std::vector<uint64_t> hb((size_t)(f.words * e->wpr), 0ull);
  for (long long b = 0; b < f.words; b++) {
    const unsigned char *values;
    const size_t take = read_row(f.d, f.pos, f.size, e->vocab.data() + b * kMaxW, &values);
    uint64_t *row = hb.data() + b * e->wpr;
    for (size_t a = 0; a < take; a++) {
      float x;
      memcpy(&x, values + a * 4, 4);
      if (x < 0.f) row[a >> 6] |= 1ull << (a & 63);
    }
  }
  return eval_finish_bits(std::move(e), (const unsigned char *)hb.data(), nullptr, nullptr, nullptr, out);
}

extern "C" int w2b_eval_load_codes(const char *file, int64_t threshold, int32_t device, w2b_eval **out) {
  if (!file || !out) return efail(W2B_EINVAL, "w2b_eval_load_codes: null argument");
  *out = nullptr;
  VectorFile f;
  if (int rc = open_vector_file(file, 2, threshold, device, "w2b_eval_load_codes", f)) return rc;
  EvalPtr e = eval_new(f.words, f.size, 1, device, 2);
  if (f.packed) {
    names_from_words(e.get(), f.words, [&](long long b) -> const std::string & { return f.names[(size_t)b]; });
    return eval_finish_bits(std::move(e), f.d.data() + f.pos, nullptr, nullptr, nullptr, out);
  }
  // a float file: each value reduced by the bitlevel-2 rule (ref :26-61: negative iff num < 0, .25 iff |num| <= .5; NaN
  // fails both comparisons: +.75)
  std::vector<uint64_t> hb((size_t)(f.words * e->wpr), 0ull);
  for (long long b = 0; b < f.words; b++) {
    const unsigned char *values;
    const size_t take = read_row(f.d, f.pos, f.size, e->vocab.data() + b * kMaxW, &values);
    uint64_t *row = hb.data() + b * e->wpr;
    for (size_t a = 0; a < take; a++) {
      float x;
      memcpy(&x, values + a * 4, 4);
      if (x < 0.f) row[2 * (a >> 6)] |= 1ull << (a & 63);
      if (!(fabsf(x) <= .5f)) row[2 * (a >> 6) + 1] |= 1ull << (a & 63);
    }
  }
  return eval_finish_bits(std::move(e), (const unsigned char *)hb.data(), nullptr, nullptr, nullptr, out);
}

namespace {
struct TrainerView {
  float *u = nullptr, *v = nullptr;
  long long V = 0, D = 0;
  int bitlevel = 0, device = 0;
  hipStream_t stream = nullptr;
};
}  // namespace

// The evaluator on a LIVE trainer: what `compute_accuracy <file> <bitlevel> <threshold>` would load after `./word2bits
// -binary 1` (bits: the packed save) had written <file> from this trainer -- without the file.  This is what the two
// forms share: the checks, the trainer's tables and the handle with its names, which go through the same reader logic
// as a file's would.
static int eval_new_from_trainer(w2b_trainer *t, int64_t n_words, const char *const *words_in, int64_t threshold,
                                 int32_t fused, int packed, const std::string &who, TrainerView &tv, EvalPtr &e,
                                 w2b_eval **out) {
  if (!t || !out || (n_words > 0 && !words_in)) return efail(W2B_EINVAL, who + ": null argument");
  *out = nullptr;
  w2b_internal_trainer_view(t, &tv.u, &tv.v, &tv.V, &tv.D, &tv.bitlevel, &tv.device, &tv.stream);
  if (packed && tv.bitlevel != packed)
    return efail(W2B_EINVAL, who + ": the trainer must be at -bitlevel " + std::to_string(packed));
  if (n_words != tv.V) return efail(W2B_EINVAL, who + ": one word per vocabulary row is needed");
  const long long words = threshold && tv.V > threshold ? threshold : tv.V;   // ref :86
  e = eval_new(words, tv.D, fused, tv.device, packed);
  names_from_words(e.get(), words, [&](long long b) { return words_in[b]; });
  return W2B_OK;
}

// fp32: quantize(u+v) (ref src/word2bits.cpp:568-569) is exported on the device straight into the evaluator's matrix
extern "C" int w2b_eval_from_trainer(w2b_trainer *t, int64_t n_words, const char *const *words_in, int32_t bitlevel,
                                     int64_t threshold, int32_t fused, w2b_eval **out) {
  TrainerView tv;
  EvalPtr e;
  if (int rc = eval_new_from_trainer(t, n_words, words_in, threshold, fused, 0, "w2b_eval_from_trainer", tv, e, out))
    return rc;
  const long long words = e->words;
  if (hipSetDevice(tv.device) != hipSuccess) return efail(W2B_EHIP, "hipSetDevice failed");
  DeviceTemp q;
  if (hipMalloc(&q.p, sizeof(float) * (size_t)(words > 0 ? words : 1) * tv.D) != hipSuccess)
    return efail(W2B_ENOMEM, "w2b_eval_from_trainer: device allocation failed");
  // quantize(u+v) with the TRAINER's bitlevel
  hipError_t he = w2b_launch_export(tv.u, tv.v, q.p, words * tv.D, tv.bitlevel, tv.stream);
  if (he == hipSuccess) he = hipStreamSynchronize(tv.stream);
  if (he != hipSuccess) return efail(W2B_EHIP, std::string("w2b_eval_from_trainer: ") + hipGetErrorString(he));
  return eval_finish(std::move(e), bitlevel, q.p, hipMemcpyDeviceToDevice, out);
}

extern "C" int w2b_eval_bits_from_trainer(w2b_trainer *t, int64_t n_words, const char *const *words_in, int64_t threshold,
                                          w2b_eval **out) {
  TrainerView tv;
  EvalPtr e;
  if (int rc = eval_new_from_trainer(t, n_words, words_in, threshold, 1, 1, "w2b_eval_bits_from_trainer", tv, e, out))
    return rc;
  return eval_finish_bits(std::move(e), nullptr, tv.u, tv.v, tv.stream, out);
}

extern "C" int w2b_eval_codes_from_trainer(w2b_trainer *t, int64_t n_words, const char *const *words_in, int64_t threshold,
                                           w2b_eval **out) {
  TrainerView tv;
  EvalPtr e;
  if (int rc = eval_new_from_trainer(t, n_words, words_in, threshold, 1, 2, "w2b_eval_codes_from_trainer", tv, e, out))
    return rc;
  return eval_finish_bits(std::move(e), nullptr, tv.u, tv.v, tv.stream, out);
}

extern "C" int32_t w2b_eval_is_bits(const w2b_eval *e) { return e ? e->bits : 0; }
extern "C" int32_t w2b_eval_is_codes(const w2b_eval *e) { return e ? e->codes : 0; }

extern "C" int w2b_eval_get_codes(w2b_eval *e, uint64_t *out) {
  if (!e || !out) return efail(W2B_EINVAL, "w2b_eval_get_codes: null argument");
  if (!e->codes) return efail(W2B_EINVAL, "w2b_eval_get_codes: not a codes handle");
  EHIP(hipSetDevice(e->device));
  if (e->words > 0) EHIP(hipMemcpy(out, e->B, (size_t)e->words * (size_t)e->wpr * 8, hipMemcpyDeviceToHost));
  return W2B_OK;
}

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

namespace {
// what w2b_eval_combine and its host twin refuse in one question's slots (null: nothing)
const char *bad_terms(int32_t nt, const int32_t *rows, const int8_t *signs, int64_t words) {
  int used = 0;
  for (int32_t t = 0; t < nt; t++) {
    if (signs[t] < -1 || signs[t] > 1) return "a sign must be -1, 0 or +1";
    if (signs[t] == 0) continue;
    if (rows[t] < 0 || rows[t] >= words) return "question row out of range";
    used++;
  }
  return used ? nullptr : "a question needs at least one slot with a sign";
}
}  // namespace

// host twin of the bits form of w2b_eval_combine: I(c) = sum over the used slots of sign * (dim - 2 * Hamming(r, c))
extern "C" int w2b_bits_combine_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t nt,
                                            const int32_t *rows, const int8_t *signs, int32_t *I_out) {
  const std::string who = "w2b_bits_combine_scores_host";
  if (!packed || !rows || !signs || !I_out || words < 0 || dim < 1) return efail(W2B_EINVAL, who + ": bad argument");
  if (nt < 1 || nt > W2B_EVAL_MAX_TERMS) return efail(W2B_EINVAL, who + ": the number of terms must be 1..7");
  if (const char *why = bad_terms(nt, rows, signs, words)) return efail(W2B_EINVAL, who + ": " + why);
  const int64_t wpr = (dim + 63) / 64;
  for (int64_t c = 0; c < words; c++) {
    const uint64_t *rc = packed + c * wpr;
    int64_t I = 0;
    for (int32_t t = 0; t < nt; t++) {
      if (signs[t] == 0) continue;
      const uint64_t *rt = packed + (int64_t)rows[t] * wpr;
      int64_t h = 0;
      for (int64_t w = 0; w < wpr; w++) {
        const uint64_t valid = (w + 1) * 64 <= dim ? ~0ull : (1ull << (dim - w * 64)) - 1;    // padding bits do not count
        h += __builtin_popcountll((rt[w] ^ rc[w]) & valid);
      }
      I += signs[t] * (dim - 2 * h);
    }
    I_out[c] = (int32_t)I;
  }
  return W2B_OK;
}

// Host twin of the codes kernels.  The float sequence of the header, one rounding per operation: this file is built with
// -ffp-contract=off and the function's body repeats it, so that no build fuses p * w + p.
extern "C" int w2b_codes_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int64_t b1, int64_t b2, int64_t b3,
                                     int32_t *J_out, float *score_out) {
#pragma clang fp contract(off)
  if (!packed || words < 0 || dim < 1 || b1 < 0 || b2 < 0 || b3 < 0 || b1 >= words || b2 >= words || b3 >= words)
    return efail(W2B_EINVAL, "w2b_codes_scores_host: bad argument");
  const int64_t nb = (dim + 63) / 64, wpr = 2 * nb;
  const std::vector<float> wt = codes_weights(dim);
  auto valid = [&](int64_t b) { return (b + 1) * 64 <= dim ? ~0ull : (1ull << (dim - b * 64)) - 1; };   // padding bits do not count
  auto weight = [&](const uint64_t *r) {
    int64_t n3 = 0;
    for (int64_t b = 0; b < nb; b++) n3 += __builtin_popcountll(r[2 * b + 1] & valid(b));
    return wt[(size_t)n3];
  };
  // sum_a t_x t_c over a block: |t_x t_c| is 1 + 2 m_x + 2 m_c + 4 m_x m_c, its sign that of s_x ^ s_c
  auto dot = [&](const uint64_t *x, const uint64_t *c) {
    int64_t j = 0;
    for (int64_t b = 0; b < nb; b++) {
      const uint64_t v = valid(b), neg = (x[2 * b] ^ c[2 * b]) & v, pos = ~neg & v;
      const uint64_t mx = x[2 * b + 1], mc = c[2 * b + 1];
      auto mag = [&](uint64_t m) {
        return (int64_t)__builtin_popcountll(m) + 2 * __builtin_popcountll(m & mx) + 2 * __builtin_popcountll(m & mc) +
               4 * __builtin_popcountll(m & mx & mc);
      };
      j += mag(pos) - mag(neg);
    }
    return (int32_t)j;
  };
  const uint64_t *r1 = packed + b1 * wpr, *r2 = packed + b2 * wpr, *r3 = packed + b3 * wpr;
  const float w1 = weight(r1), w2 = weight(r2), w3 = weight(r3);
  for (int64_t c = 0; c < words; c++) {
    const uint64_t *rc = packed + c * wpr;
    const int32_t j1 = dot(r1, rc), j2 = dot(r2, rc), j3 = dot(r3, rc);
    if (J_out) {
      J_out[c] = j1;
      J_out[words + c] = j2;
      J_out[2 * words + c] = j3;
    }
    if (score_out) {
      const float p1 = (float)j1 * w1, p2 = (float)j2 * w2, p3 = (float)j3 * w3;
      const float d = p2 - p1;
      const float s = d + p3;
      score_out[c] = s * weight(rc);
    }
  }
  return W2B_OK;
}

namespace {
constexpr int64_t kCosmulMaxBits = 1ll << 24;   // the largest 1-bit size whose agreement counts are exact in float32
constexpr float kCosmulEps = 1e-6f;             // 0x358637BD

// u by agreement count on 1-bit rows: (float)A / (float)dim, one correctly rounded division, A = 0..dim
std::vector<float> cosmul_utab(int64_t dim) {
  std::vector<float> u((size_t)dim + 1);
  for (int64_t a = 0; a <= dim; a++) u[(size_t)a] = (float)a / (float)dim;
  return u;
}

// score = (u2 * u3) / (u1 + eps), one rounding per operation
inline float cosmul_score(float u1, float u2, float u3) {
#pragma clang fp contract(off)
  const float num = u2 * u3;
  const float den = u1 + kCosmulEps;
  return num / den;
}
}  // namespace

// Host twin of the 3CosMul kernels.  The float sequence of the header, one rounding per operation (this file is built with
// -ffp-contract=off, and the function says so again).
extern "C" int w2b_cosmul_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, int64_t b1,
                                      int64_t b2, int64_t b3, float *u_out, float *score_out) {
#pragma clang fp contract(off)
  const std::string who = "w2b_cosmul_scores_host";
  if (!packed || words < 0 || dim < 1) return efail(W2B_EINVAL, who + ": bad argument");
  if (bitlevel != 1 && bitlevel != 2) return efail(W2B_EINVAL, who + ": bitlevel must be 1 or 2");
  if (bitlevel == 1 && dim > kCosmulMaxBits) return efail(W2B_EINVAL, who + ": size must be at most 2^24 on 1-bit rows");
  if (b1 < 0 || b2 < 0 || b3 < 0 || b1 >= words || b2 >= words || b3 >= words)
    return efail(W2B_EINVAL, who + ": question row out of range");
  const int64_t b[3] = {b1, b2, b3};
  const int64_t nb = (dim + 63) / 64, wpr = nb * bitlevel;
  auto valid = [&](int64_t blk) { return (blk + 1) * 64 <= dim ? ~0ull : (1ull << (dim - blk * 64)) - 1; };   // padding bits do not count
  std::vector<float> u((size_t)(3 * words));
  if (bitlevel == 1) {
    const std::vector<float> ut = cosmul_utab(dim);
    for (int t = 0; t < 3; t++) {
      const uint64_t *rt = packed + b[t] * wpr;
      for (int64_t c = 0; c < words; c++) {
        const uint64_t *rc = packed + c * wpr;
        int64_t h = 0;
        for (int64_t w = 0; w < nb; w++) h += __builtin_popcountll((rt[w] ^ rc[w]) & valid(w));
        u[(size_t)(t * words + c)] = ut[(size_t)(dim - h)];
      }
    }
  } else {
    std::vector<int32_t> J((size_t)(3 * words));
    if (int rc = w2b_codes_scores_host(packed, words, dim, b1, b2, b3, J.data(), nullptr)) return rc;
    const std::vector<float> wt = codes_weights(dim);
    auto weight = [&](const uint64_t *r) {
      int64_t n3 = 0;
      for (int64_t blk = 0; blk < nb; blk++) n3 += __builtin_popcountll(r[2 * blk + 1] & valid(blk));
      return wt[(size_t)n3];
    };
    for (int t = 0; t < 3; t++) {
      const float wb = weight(packed + b[t] * wpr);
      for (int64_t c = 0; c < words; c++) {
        const float pj = (float)J[(size_t)(t * words + c)] * wb;
        const float cs = pj * weight(packed + c * wpr);
        const float one = 1.0f + cs;
        u[(size_t)(t * words + c)] = one * 0.5f;
      }
    }
  }
  if (u_out) memcpy(u_out, u.data(), u.size() * 4);
  if (score_out)
    for (int64_t c = 0; c < words; c++)
      score_out[c] = cosmul_score(u[(size_t)c], u[(size_t)(words + c)], u[(size_t)(2 * words + c)]);
  return W2B_OK;
}

namespace {
constexpr int64_t kBagMaxSize = 58254;   // the largest size with 9 * 4096 * size < 2^31

// what w2b_eval_bag and its host twin refuse in one bag (null: nothing)
const char *bad_bag(int64_t n, const int32_t *ids, int64_t words) {
  if (n < 0 || n > W2B_EVAL_MAX_BAG) return "a bag holds at most 4096 ids";
  for (int64_t i = 0; i < n; i++)
    if (ids[i] >= words) return "bag id out of range";
  return nullptr;
}

// wq of the header from N_T; a question whose vector is zero weighs nothing
inline float bag_weight(unsigned long long nt) { return nt ? (float)(1.0 / sqrt((double)nt)) : 0.f; }
}  // namespace

// Host twin of the bag kernels: T from the unpacked rows, J in 64 bits, the float steps of the header one at a time (this
// file is built with -ffp-contract=off, and the function says so again).
extern "C" int w2b_bag_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, int64_t n,
                                   const int32_t *ids, int32_t *J_out, float *score_out) {
#pragma clang fp contract(off)
  const std::string who = "w2b_bag_scores_host";
  if (!packed || words < 0 || dim < 1 || (n > 0 && !ids)) return efail(W2B_EINVAL, who + ": bad argument");
  if (bitlevel != 1 && bitlevel != 2) return efail(W2B_EINVAL, who + ": bitlevel must be 1 or 2");
  if (dim > kBagMaxSize) return efail(W2B_EINVAL, who + ": size must be at most 58254 (9 * 4096 * size < 2^31)");
  if (const char *why = bad_bag(n, ids, words)) return efail(W2B_EINVAL, who + ": " + why);
  const int64_t nb = (dim + 63) / 64, wpr = nb * bitlevel;
  auto t_of = [&](const uint64_t *r, int64_t a) -> int32_t {
    const uint64_t bit = 1ull << (a & 63);
    if (bitlevel == 1) return (r[a >> 6] & bit) ? -1 : 1;
    return ((r[2 * (a >> 6) + 1] & bit) ? 3 : 1) * ((r[2 * (a >> 6)] & bit) ? -1 : 1);
  };
  std::vector<int32_t> T((size_t)dim, 0);
  for (int64_t i = 0; i < n; i++)
    if (ids[i] >= 0)
      for (int64_t a = 0; a < dim; a++) T[(size_t)a] += t_of(packed + (int64_t)ids[i] * wpr, a);
  unsigned long long nt = 0;
  for (int64_t a = 0; a < dim; a++) nt += (unsigned long long)((int64_t)T[(size_t)a] * T[(size_t)a]);
  const float wq = bag_weight(nt);
  const std::vector<float> wt = bitlevel == 2 ? codes_weights(dim) : std::vector<float>();
  for (int64_t c = 0; c < words; c++) {
    const uint64_t *rc = packed + c * wpr;
    int64_t j = 0, n3 = 0;
    for (int64_t a = 0; a < dim; a++) {
      const int32_t t = t_of(rc, a);
      j += (int64_t)T[(size_t)a] * t;
      n3 += t == 3 || t == -3;
    }
    if (J_out) J_out[c] = (int32_t)j;
    if (!score_out) continue;
    if (bitlevel == 1) {
      score_out[c] = (float)(int32_t)j / (float)dim;
    } else {
      const float pj = (float)(int32_t)j * wq;
      score_out[c] = pj * wt[(size_t)n3];
    }
  }
  return W2B_OK;
}

namespace {
// what w2b_eval_vectors and its host twin refuse in one question: the first column whose value is not finite, or neither 0
// nor of a magnitude in 2^-60 .. 2^60 (-1: none)
int64_t bad_vector_value(const float *x, int64_t dim) {
  for (int64_t a = 0; a < dim; a++) {
    const float m = fabsf(x[a]);
    if (!(m == 0.f || (m >= 0x1p-60f && m <= 0x1p60f))) return a;       // (NaN fails every comparison)
  }
  return -1;
}
const char *const kVectorRange = "a value must be finite and either 0 or of a magnitude in 2^-60 .. 2^60";

// wx of the header: nx in double, column by column; a question whose vector is zero weighs nothing
float vector_weight(const float *x, int64_t dim, int32_t normalize) {
#pragma clang fp contract(off)
  double nx = 0.0;
  for (int64_t a = 0; a < dim; a++) {
    const double sq = (double)x[a] * (double)x[a];
    nx = nx + sq;
  }
  if (nx == 0.0) return 0.f;
  return normalize ? (float)(1.0 / sqrt(nx)) : 1.0f;
}
}  // namespace

// Host twin of the vector kernels: the fmaf chain of the header in column order, then the two multiplies one at a time (this
// file is built with -ffp-contract=off, and the function says so again).
extern "C" int w2b_vector_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, const float *x,
                                      int32_t normalize, float *S_out, float *score_out) {
#pragma clang fp contract(off)
  const std::string who = "w2b_vector_scores_host";
  if (!packed || !x || words < 0 || dim < 1) return efail(W2B_EINVAL, who + ": bad argument");
  if (bitlevel != 1 && bitlevel != 2) return efail(W2B_EINVAL, who + ": bitlevel must be 1 or 2");
  if (normalize != 0 && normalize != 1) return efail(W2B_EINVAL, who + ": normalize must be 0 or 1");
  const int64_t bad = bad_vector_value(x, dim);
  if (bad >= 0) return efail(W2B_EINVAL, who + ": column " + std::to_string(bad) + ": " + kVectorRange);
  const int64_t nb = (dim + 63) / 64, wpr = nb * bitlevel;
  const float wx = vector_weight(x, dim, normalize);
  const std::vector<float> wt = bitlevel == 2 ? codes_weights(dim) : std::vector<float>();
  const float wbits = (float)(1.0 / sqrt((double)dim));
  for (int64_t c = 0; c < words; c++) {
    const uint64_t *rc = packed + c * wpr;
    float acc = 0.f;
    int64_t n3 = 0;
    for (int64_t a = 0; a < dim; a++) {
      const uint64_t bit = 1ull << (a & 63);
      float t = 1.f;
      if (bitlevel == 2 && (rc[2 * (a >> 6) + 1] & bit)) t = 3.f, n3++;
      if (rc[bitlevel * (a >> 6)] & bit) t = -t;
      acc = fmaf(x[a], t, acc);
    }
    if (S_out) S_out[c] = acc;
    if (!score_out) continue;
    const float ps = acc * wx;
    score_out[c] = ps * (bitlevel == 2 ? wt[(size_t)n3] : wbits);
  }
  return W2B_OK;
}

namespace {
constexpr int64_t kDocsMaxSize = 1ll << 21;      // size below it: 1024 * size < 2^31 and ldexp(cos, 50) is an integer
constexpr int64_t kDocsMaxDocs = 0x7FFFFF00ll;
constexpr int64_t kDocsMaxAll = 1ll << 28;       // nq * n_docs of an all_scores request

// what w2b_eval_docs_set, w2b_eval_docs and the host twin refuse in texts given as ids + offsets before they look at a handle
// or a table (empty: nothing); `what` = "document" or "query"
std::string bad_texts(int64_t n_ids, const int32_t *ids, int64_t n, const int64_t *offsets, const char *what) {
  if (n < 0 || n_ids < 0 || (n > 0 && !offsets) || (n_ids > 0 && !ids)) return "bad argument";
  if (n == 0 ? n_ids != 0 : (offsets[0] != 0 || offsets[n] != n_ids))
    return std::string(what) + " offsets must start at 0 and end at the number of ids";
  for (int64_t d = 0; d < n; d++) {
    if (offsets[d + 1] < offsets[d] || offsets[d + 1] > n_ids) return std::string(what) + " offsets must not decrease";
    if (offsets[d + 1] - offsets[d] > W2B_EVAL_MAX_DOC) return std::string("a ") + what + " holds at most 1024 positions";
  }
  return std::string();
}
bool bad_text_ids(int64_t n_ids, const int32_t *ids, int64_t words) {
  for (int64_t i = 0; i < n_ids; i++)
    if (ids[i] >= words) return true;
  return false;
}
const char *const kDocsSize = "size must be below 2^21 (1024 * size < 2^31)";
const char *const kDocsFp32 = "not available on an fp32 handle: load the file with bits or codes";

// the float steps of the header: one directed score from its integer sum
inline float docs_score(int32_t bitlevel, int64_t sum, int64_t m, int64_t dim) {
#pragma clang fp contract(off)
  if (bitlevel == 1) return (float)(int32_t)sum / (float)(int32_t)(m * dim);
  const float div = (float)m * 0x1p50f;          // exact
  return (float)sum / div;
}
}  // namespace

// Host twin of the document kernels: every (query position, document position) pair from the packed rows themselves, the
// maxima and the sums in 64-bit integers, the float steps of the header one at a time (this file is built with
// -ffp-contract=off, and the function says so again).
extern "C" int w2b_docs_scores_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, int64_t n_ids,
                                    const int32_t *ids, int64_t n_docs, const int64_t *offsets, int64_t n_q,
                                    const int32_t *qids, int32_t symmetric, int64_t *dir_out, float *score_out) {
#pragma clang fp contract(off)
  const std::string who = "w2b_docs_scores_host";
  if (symmetric != 0 && symmetric != 1) return efail(W2B_EINVAL, who + ": symmetric must be 0 or 1");
  if (n_q < 0 || (n_q > 0 && !qids)) return efail(W2B_EINVAL, who + ": bad argument");
  if (n_q > W2B_EVAL_MAX_DOC) return efail(W2B_EINVAL, who + ": a query holds at most 1024 positions");
  if (n_docs > kDocsMaxDocs) return efail(W2B_EINVAL, who + ": at most 0x7FFFFF00 documents");
  const std::string why = bad_texts(n_ids, ids, n_docs, offsets, "document");
  if (!why.empty()) return efail(W2B_EINVAL, who + ": " + why);
  if (!packed || words < 0 || dim < 1) return efail(W2B_EINVAL, who + ": bad argument");
  if (bitlevel != 1 && bitlevel != 2) return efail(W2B_EINVAL, who + ": bitlevel must be 1 or 2");
  if (dim >= kDocsMaxSize) return efail(W2B_EINVAL, who + ": " + kDocsSize);
  if (bad_text_ids(n_ids, ids, words)) return efail(W2B_EINVAL, who + ": document id out of range");
  if (bad_text_ids(n_q, qids, words)) return efail(W2B_EINVAL, who + ": query id out of range");
  const int64_t nb = (dim + 63) / 64, wpr = nb * bitlevel;
  auto valid = [&](int64_t b) { return (b + 1) * 64 <= dim ? ~0ull : (1ull << (dim - b * 64)) - 1; };   // padding bits do not count
  const std::vector<float> wt = bitlevel == 2 ? codes_weights(dim) : std::vector<float>();
  auto weight = [&](const uint64_t *r) {
    int64_t n3 = 0;
    for (int64_t b = 0; b < nb; b++) n3 += __builtin_popcountll(r[2 * b + 1] & valid(b));
    return wt[(size_t)n3];
  };
  // I(x, c), or F(x, c) = (int64) ldexp(cos(x, c), 50)
  auto pair = [&](const uint64_t *x, float wx, const uint64_t *c, float wc) -> int64_t {
    if (bitlevel == 1) {
      int64_t h = 0;
      for (int64_t b = 0; b < nb; b++) h += __builtin_popcountll((x[b] ^ c[b]) & valid(b));
      return dim - 2 * h;
    }
    int64_t j = 0;
    for (int64_t b = 0; b < nb; b++) {
      const uint64_t v = valid(b), neg = (x[2 * b] ^ c[2 * b]) & v, pos = ~neg & v;
      const uint64_t mx = x[2 * b + 1], mc = c[2 * b + 1];
      auto mag = [&](uint64_t m) {
        return (int64_t)__builtin_popcountll(m) + 2 * __builtin_popcountll(m & mx) + 2 * __builtin_popcountll(m & mc) +
               4 * __builtin_popcountll(m & mx & mc);
      };
      j += mag(pos) - mag(neg);
    }
    const float pj = (float)(int32_t)j * wx;
    const float cs = pj * wc;
    return (int64_t)ldexpf(cs, 50);
  };
  std::vector<const uint64_t *> qr;
  std::vector<float> qw;
  for (int64_t i = 0; i < n_q; i++)
    if (qids[i] >= 0) {
      qr.push_back(packed + (int64_t)qids[i] * wpr);
      qw.push_back(bitlevel == 2 ? weight(qr.back()) : 0.f);
    }
  const int64_t mq = (int64_t)qr.size();
  std::vector<int64_t> best_x((size_t)mq);
  for (int64_t d = 0; d < n_docs; d++) {
    int64_t md = 0, r_qd = 0, r_dq = 0;
    for (int64_t i = offsets[d]; i < offsets[d + 1]; i++) {
      if (ids[i] < 0 || mq == 0) continue;
      const uint64_t *c = packed + (int64_t)ids[i] * wpr;
      const float wc = bitlevel == 2 ? weight(c) : 0.f;
      int64_t best_c = 0;
      for (int64_t x = 0; x < mq; x++) {
        const int64_t v = pair(qr[(size_t)x], qw[(size_t)x], c, wc);
        if (md == 0 || v > best_x[(size_t)x]) best_x[(size_t)x] = v;
        if (x == 0 || v > best_c) best_c = v;
      }
      r_dq += best_c;
      md++;
    }
    if (md > 0)
      for (int64_t x = 0; x < mq; x++) r_qd += best_x[(size_t)x];
    if (dir_out) {
      dir_out[d] = r_qd;
      dir_out[n_docs + d] = r_dq;
    }
    if (!score_out) continue;
    float sc = 0.f;
    if (mq > 0 && md > 0) {
      sc = docs_score(bitlevel, r_qd, mq, dim);
      if (symmetric) {
        const float s2 = docs_score(bitlevel, r_dq, md, dim);
        sc = s2 < sc ? s2 : sc;
      }
    }
    score_out[d] = sc;
  }
  return W2B_OK;
}

namespace {
constexpr int64_t kPairsMaxSize = 1ll << 24;     // 12288^2 * size < 2^53: J, N_A, N_B are exact as doubles

// what w2b_eval_pairs and its host twin refuse before they look at a handle or a table (empty: nothing)
std::string bad_pairs(int64_t n_ids, const int32_t *ids, int64_t np, const int64_t *offsets, const float *score,
                      const int64_t *parts) {
  if (np < 0 || n_ids < 0 || (np > 0 && (!offsets || (!score && !parts))) || (n_ids > 0 && !ids)) return "bad argument";
  if (np > (INT64_MAX >> 2)) return "bad argument";
  if (np == 0 ? n_ids != 0 : (offsets[0] != 0 || offsets[2 * np] != n_ids)) return "offsets must start at 0 and end at n_ids";
  for (int64_t b = 0; b < 2 * np; b++) {
    if (offsets[b + 1] < offsets[b] || offsets[b + 1] > n_ids) return "offsets must not decrease";
    if (offsets[b + 1] - offsets[b] > W2B_EVAL_MAX_BAG) return "a bag holds at most 4096 ids";
  }
  return std::string();
}
// the first pair with an id >= words (-1: none)
int64_t bad_pair_id(const int32_t *ids, int64_t np, const int64_t *offsets, int64_t words) {
  for (int64_t p = 0; p < np; p++)
    for (int64_t i = offsets[2 * p]; i < offsets[2 * p + 2]; i++)
      if (ids[i] >= words) return p;
  return -1;
}

// the score of the header from the three integers; an empty pair scores +0
inline float pair_score(int64_t j, int64_t na, int64_t nb) {
#pragma clang fp contract(off)
  if (na == 0 || nb == 0) return 0.f;
  const double nn = (double)na * (double)nb;
  const double root = sqrt(nn);
  return (float)((double)j / root);
}
}  // namespace

// Host twin of the pair kernels: both pooled vectors from the unpacked rows, the three sums in 64-bit integers, the double
// steps of the header one at a time (this file is built with -ffp-contract=off, and pair_score says so again).
extern "C" int w2b_pairs_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, int64_t n_ids,
                              const int32_t *ids, int64_t np, const int64_t *offsets, float *score, int64_t *parts) {
  const std::string who = "w2b_pairs_host";
  const std::string why = bad_pairs(n_ids, ids, np, offsets, score, parts);
  if (!why.empty()) return efail(W2B_EINVAL, who + ": " + why);
  if (!packed || words < 0 || dim < 1) return efail(W2B_EINVAL, who + ": bad argument");
  if (bitlevel != 1 && bitlevel != 2) return efail(W2B_EINVAL, who + ": bitlevel must be 1 or 2");
  if (dim > kPairsMaxSize) return efail(W2B_EINVAL, who + ": size must be at most 2^24");
  const int64_t bad = bad_pair_id(ids, np, offsets, words);
  if (bad >= 0) return efail(W2B_EINVAL, who + ": pair " + std::to_string(bad) + ": id out of range");
  const int64_t nb = (dim + 63) / 64, wpr = nb * bitlevel;
  auto t_of = [&](const uint64_t *r, int64_t a) -> int32_t {
    const uint64_t bit = 1ull << (a & 63);
    if (bitlevel == 1) return (r[a >> 6] & bit) ? -1 : 1;
    return ((r[2 * (a >> 6) + 1] & bit) ? 3 : 1) * ((r[2 * (a >> 6)] & bit) ? -1 : 1);
  };
  std::vector<int32_t> T[2] = {std::vector<int32_t>((size_t)dim), std::vector<int32_t>((size_t)dim)};
  for (int64_t p = 0; p < np; p++) {
    for (int side = 0; side < 2; side++) {
      std::fill(T[side].begin(), T[side].end(), 0);
      for (int64_t i = offsets[2 * p + side]; i < offsets[2 * p + side + 1]; i++)
        if (ids[i] >= 0)
          for (int64_t a = 0; a < dim; a++) T[side][(size_t)a] += t_of(packed + (int64_t)ids[i] * wpr, a);
    }
    int64_t j = 0, na = 0, nbb = 0;
    for (int64_t a = 0; a < dim; a++) {
      const int64_t x = T[0][(size_t)a], y = T[1][(size_t)a];
      j += x * y;
      na += x * x;
      nbb += y * y;
    }
    if (score) score[p] = pair_score(j, na, nbb);
    if (parts) parts[3 * p] = j, parts[3 * p + 1] = na, parts[3 * p + 2] = nbb;
  }
  return W2B_OK;
}

namespace {
// Pearson's r of the header; NaN with n < 2 or a zero variance
double pearson_r(const std::vector<double> &x, const std::vector<double> &y) {
#pragma clang fp contract(off)
  const size_t n = x.size();
  if (n < 2) return NAN;
  if (*std::min_element(x.begin(), x.end()) == *std::max_element(x.begin(), x.end()) ||
      *std::min_element(y.begin(), y.end()) == *std::max_element(y.begin(), y.end()))
    return NAN;                                    // (a constant: its deviations from a rounded mean need not be zero)
  double mx = 0, my = 0;
  for (size_t i = 0; i < n; i++) mx += x[i], my += y[i];
  mx /= (double)n;
  my /= (double)n;
  double sxy = 0, sxx = 0, syy = 0;
  for (size_t i = 0; i < n; i++) {
    const double dx = x[i] - mx, dy = y[i] - my;
    sxy += dx * dy;
    sxx += dx * dx;
    syy += dy * dy;
  }
  if (!(sxx > 0) || !(syy > 0)) return NAN;
  return sxy / sqrt(sxx * syy);
}
// 1-based ranks, equal values sharing the mean of their ranks
std::vector<double> mean_ranks(const std::vector<double> &v) {
  const size_t n = v.size();
  std::vector<size_t> idx(n);
  for (size_t i = 0; i < n; i++) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return v[a] < v[b]; });
  std::vector<double> r(n);
  for (size_t i = 0; i < n;) {
    size_t k = i;
    while (k < n && v[idx[k]] == v[idx[i]]) k++;
    const double mean = 0.5 * (double)(i + 1 + k);           // ranks i + 1 .. k
    for (size_t t = i; t < k; t++) r[idx[t]] = mean;
    i = k;
  }
  return r;
}
}  // namespace

extern "C" int w2b_rank_correlation(int64_t n, const double *x, const double *y, double *pearson, double *spearman) {
  if (n < 0 || (n > 0 && (!x || !y))) return efail(W2B_EINVAL, "w2b_rank_correlation: bad argument");
  const std::vector<double> xv(x, x + n), yv(y, y + n);
  bool nan = false;
  for (int64_t i = 0; i < n; i++) nan |= std::isnan(xv[(size_t)i]) || std::isnan(yv[(size_t)i]);
  if (pearson) *pearson = nan ? NAN : pearson_r(xv, yv);
  if (spearman) *spearman = nan ? NAN : pearson_r(mean_ranks(xv), mean_ranks(yv));
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
  if (e->codes) return efail(W2B_EINVAL, "w2b_eval_get_matrix: a codes handle holds no float matrix (w2b_eval_get_codes)");
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
  hipError_t qe = e->bits ? hipMalloc(&e->P, (size_t)np * (size_t)e->wpr * 16)
                          : e->codes ? hipMalloc(&e->P, w2b_codes_operand_bytes((int)e->size, np))
                                     : hipMalloc(&e->Q, (size_t)np * e->ld * 4);
  if (qe == hipSuccess && e->codes) qe = hipMalloc(&e->Q, (size_t)np * 12);
  if (qe != hipSuccess || hipMalloc(&e->b123, (size_t)np * 12) != hipSuccess ||
      hipMalloc(&e->best, (size_t)np * 8) != hipSuccess)
    return W2B_ENOMEM;
  e->cap_q = np;
  return W2B_OK;
}

// the per-call buffers of `np` (padded) signed multi-word questions, next to those of eval_reserve_questions
static int eval_reserve_terms(w2b_eval *e, int64_t np) {
  if (np <= e->cap_t) return W2B_OK;
  if (e->terms) (void)hipFree(e->terms);
  if (e->P4) (void)hipFree(e->P4);
  e->terms = nullptr; e->P4 = nullptr; e->cap_t = 0;
  if (hipMalloc(&e->terms, (size_t)np * W2B_EVAL_XSTRIDE * 8) != hipSuccess) return W2B_ENOMEM;
  if (e->bits && hipMalloc(&e->P4, (size_t)np * (size_t)e->wpr * 32) != hipSuccess) return W2B_ENOMEM;
  e->cap_t = np;
  return W2B_OK;
}

// one of the two per-call buffers of w2b_eval_bag
static int eval_reserve_bag(void **buf, size_t *have, size_t need) {
  if (need <= *have) return W2B_OK;
  if (*buf) (void)hipFree(*buf);
  *buf = nullptr;
  *have = 0;
  if (hipMalloc(buf, need) != hipSuccess) return W2B_ENOMEM;
  *have = need;
  return W2B_OK;
}

// the top-k scratch of one launch
static int eval_reserve_topk(w2b_eval *e, size_t need) {
  if (need <= e->tk_bytes) return W2B_OK;
  if (e->tk_buf) (void)hipFree(e->tk_buf);
  e->tk_buf = nullptr;
  e->tk_bytes = 0;
  if (hipMalloc(&e->tk_buf, need) != hipSuccess) return W2B_ENOMEM;
  e->tk_bytes = need;
  return W2B_OK;
}

// ------------------------------------------------------------------------------------ the scan (ref :155-177)
// Every query goes through eval_scan_chunks in chunks of questions.  What a question is made of is an input struct
// (Rows3: the three rows of the reference's question; Terms: the signed rows of w2b_eval_combine) whose upload(...) puts
// a chunk on the device.  What differs between the forms of the scan is a Scan* struct:
//   chunk, kk     questions per launch and keys per question, sized by the constructor
//   scratch(n)    bytes of top-k scratch that a chunk of n questions needs
//   before(...)   what is enqueued ahead of the timed window; leaves `keys` at the chunk's [n][kk] result keys
//   timed(...)    the launches that the kernel time covers
//   score(key)    the score in a key's high half
namespace {
struct Rows3 {   // b1, b2, b3 of every question; on the device d1, d2, d3 [np]
  const int32_t *b1, *b2, *b3;
  int32_t *d1 = nullptr, *d2 = nullptr, *d3 = nullptr;
  int upload(w2b_eval *e, int64_t q0, int64_t n, int64_t np) {
    d1 = e->b123, d2 = e->b123 + np, d3 = e->b123 + 2 * np;
    EHIP(hipMemcpyAsync(d1, b1 + q0, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemcpyAsync(d2, b2 + q0, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemcpyAsync(d3, b3 + q0, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    return W2B_OK;
  }
};

// rows / signs [nq][W2B_EVAL_XSTRIDE] as the kernels read them: the used slots first, in slot order, then row -1 / sign 0
struct Terms {
  const int32_t *rows, *signs;
  int32_t *drows = nullptr, *dsigns = nullptr;
  int upload(w2b_eval *e, int64_t q0, int64_t n, int64_t np) {
    if (eval_reserve_terms(e, np) != W2B_OK) return efail(W2B_ENOMEM, "w2b_eval_combine: device allocation failed");
    drows = e->terms, dsigns = e->terms + np * W2B_EVAL_XSTRIDE;
    const size_t bytes = (size_t)n * W2B_EVAL_XSTRIDE * 4;
    EHIP(hipMemcpyAsync(drows, rows + q0 * W2B_EVAL_XSTRIDE, bytes, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemcpyAsync(dsigns, signs + q0 * W2B_EVAL_XSTRIDE, bytes, hipMemcpyHostToDevice, e->stream));
    return W2B_OK;
  }
};

inline float f32_score(unsigned long long key) {
  const uint32_t bits = (uint32_t)(key >> 32);
  float x;
  memcpy(&x, &bits, 4);
  return x;
}

struct ScanTop1 {   // fp32 rows, the best row
  w2b_eval *e;
  int64_t chunk = kChunkQ, kk = 1;
  const unsigned long long *keys = nullptr;
  size_t scratch(int64_t) const { return 0; }
  int before(int64_t n, int64_t np, const Rows3 &d) {
    EHIP(hipMemsetAsync(e->Q, 0, (size_t)np * e->ld * 4, e->stream));
    EHIP(hipMemsetAsync(e->best, 0, (size_t)np * 8, e->stream));
    EHIP(w2b_launch_eval_queries(e->M, e->ld, n, d.d1, d.d2, d.d3, e->Q, e->variant, e->stream));
    keys = e->best;
    return W2B_OK;
  }
  hipError_t timed(int64_t n, int64_t, const Rows3 &d) {
    return w2b_launch_eval_scores(e->Q, e->M, (int)n, (int)e->words, (int)e->size, (int)e->ld, e->fused, d.d1, d.d2, d.d3, e->best,
                                  e->variant, e->stream);
  }
  float score(unsigned long long key) const { return f32_score(key); }
};

// The selection state of one top-k launch (w2b_internal.h): per question the bound, k buckets and one byte per slot
// (zeroed together), k merged keys, nunits slots of cap keys.  A chunk of questions is sized so that it stays within the
// budget, never smaller than one 128-question tile.
struct TopkScratch {
  int32_t k = 0;
  int nunits = 0, cap = 0;
  int64_t zero_q = 0, per_q = 0;
  unsigned long long *bound = nullptr, *bkt = nullptr, *merged = nullptr, *slots = nullptr;
  unsigned char *cnt = nullptr;
  int64_t chunk(int64_t budget_or_0) {
    zero_q = 8 + 8 * (int64_t)k + nunits;
    per_q = zero_q + 8 * (int64_t)k + 8 * (int64_t)nunits * cap;
    const int64_t budget = budget_or_0 > 0 ? budget_or_0 : kTopkScratch;
    int64_t c = budget / per_q / 128 * 128;
    if (c < 128) c = 128;
    return c > kChunkQ ? kChunkQ : c;
  }
  size_t bytes(int64_t n) const { return (size_t)n * per_q + 8; }
  size_t place(void *buf, int64_t n) {   // returns the bytes to zero
    const size_t zero_bytes = ((size_t)n * zero_q + 7) / 8 * 8;
    bound = (unsigned long long *)buf;
    bkt = bound + n;
    cnt = (unsigned char *)(bkt + n * k);
    merged = (unsigned long long *)((char *)buf + zero_bytes);
    slots = merged + n * k;
    return zero_bytes;
  }
};

// fp32 rows, the k best (N = k)
struct ScanTopK {
  w2b_eval *e;
  int32_t k;
  TopkScratch t;
  int64_t chunk, kk;
  const unsigned long long *keys = nullptr;
  ScanTopK(w2b_eval *e_, int32_t k_) : e(e_), k(k_), kk(k_) {
    t.k = k;
    w2b_eval_topk_layout(e->words, k, e->fused && e->variant != 0, &t.nunits, &t.cap);
    chunk = t.chunk(e->tk_budget);
  }
  size_t scratch(int64_t n) const { return t.bytes(n); }
  int clear(int64_t n, int64_t np) {   // Q and the selection state, zeroed
    const size_t zero_bytes = t.place(e->tk_buf, n);
    EHIP(hipMemsetAsync(e->Q, 0, (size_t)np * e->ld * 4, e->stream));
    EHIP(hipMemsetAsync(e->tk_buf, 0, zero_bytes, e->stream));
    keys = t.merged;
    return W2B_OK;
  }
  int before(int64_t n, int64_t np, const Rows3 &d) {
    if (int rc = clear(n, np)) return rc;
    EHIP(w2b_launch_eval_queries(e->M, e->ld, n, d.d1, d.d2, d.d3, e->Q, e->variant, e->stream));
    return W2B_OK;
  }
  hipError_t timed(int64_t n, int64_t, const Rows3 &d) {
    return w2b_launch_eval_topk(e->Q, e->M, (int)n, (int)e->words, (int)e->size, (int)e->ld, e->fused, d.d1, d.d2, d.d3, k, t.bound,
                                t.bkt, t.slots, t.cnt, t.merged, e->variant, e->stream);
  }
  float score(unsigned long long key) const { return f32_score(key); }
};

// fp32 rows, the signed multi-word question: its own query vector, then the list form of the same top-k scan
struct ScanCombine : ScanTopK {
  using ScanTopK::ScanTopK;
  int before(int64_t n, int64_t np, const Terms &d) {
    if (int rc = clear(n, np)) return rc;
    EHIP(w2b_launch_combine_queries(e->M, e->ld, n, d.drows, d.dsigns, e->Q, e->stream));
    return W2B_OK;
  }
  hipError_t timed(int64_t n, int64_t, const Terms &d) {
    return w2b_launch_eval_topk_list(e->Q, e->M, (int)n, (int)e->words, (int)e->size, (int)e->ld, e->fused, d.drows, k, t.bound,
                                     t.bkt, t.slots, t.cnt, t.merged, e->variant, e->stream);
  }
};

// The scan on 2-bit rows of include/word2bits_eval.h ("codes mode"); k = 0 is the top-1 form.  The keys are the fp32
// scans' (score bits << 32 | ~row), and the top-k form uses their selection state.
struct ScanCodes {
  w2b_eval *e;
  int32_t k;
  TopkScratch t;
  int64_t chunk = kChunkQ, kk;
  const unsigned long long *keys = nullptr;
  ScanCodes(w2b_eval *e_, int32_t k_) : e(e_), k(k_), kk(k_ > 0 ? k_ : 1) {
    if (k == 0) return;
    t.k = k;
    w2b_codes_topk_layout(e->words, (int)e->size, k, &t.nunits, &t.cap);
    chunk = t.chunk(e->tk_budget);
  }
  size_t scratch(int64_t n) const { return k > 0 ? t.bytes(n) : 0; }
  int before(int64_t n, int64_t np, const Rows3 &) {
    if (k == 0) {
      EHIP(hipMemsetAsync(e->best, 0, (size_t)np * 8, e->stream));
      keys = e->best;
    } else {
      EHIP(hipMemsetAsync(e->tk_buf, 0, t.place(e->tk_buf, n), e->stream));
      keys = t.merged;
    }
    return W2B_OK;
  }
  hipError_t timed(int64_t n, int64_t, const Rows3 &d) {
    const uint32_t *B32 = (const uint32_t *)e->B;
    hipError_t le = w2b_launch_codes_operands(B32, (int)e->size, (int)n, e->wrow, d.d1, d.d2, d.d3, e->P, e->Q, e->stream);
    if (le != hipSuccess) return le;
    return w2b_launch_codes_scan(B32, (int)e->words, (int)e->size, e->wrow, e->P, e->Q, (int)n, d.d1, d.d2, d.d3, k,
                                 k == 0 ? e->best : t.bound, t.bkt, t.slots, t.cnt, t.merged, e->stream);
  }
  float score(unsigned long long key) const { return f32_score(key); }
};

// The integer scan of include/word2bits_eval.h ("bits mode"); k = 0 is the top-1 form (best[nq]), k >= 1 the top-k form
// (best[nq][k]).  In the top-k form a chunk and its row splits are sized so that the slot scratch (splits x k keys per
// question) stays within the budget, never below 128 questions or one split.
struct ScanBits {
  w2b_eval *e;
  int32_t k;
  int64_t chunk = kChunkQ, kk;
  int splits = 1, rpb = 1;
  const unsigned long long *keys = nullptr;
  unsigned long long *merged = nullptr, *slots = nullptr;
  ScanBits(w2b_eval *e_, int64_t nq, int32_t k_) : e(e_), k(k_), kk(k_ > 0 ? k_ : 1) {
    if (k == 0) return;
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
  size_t scratch(int64_t n) const { return k > 0 ? (size_t)n * 8 * kk * (size_t)(splits + 1) : 0; }
  template <class In>
  int before(int64_t n, int64_t np, const In &) {
    if (k == 0) EHIP(hipMemsetAsync(e->best, 0, (size_t)np * 8, e->stream));
    merged = k == 0 ? e->best : (unsigned long long *)e->tk_buf;
    slots = k == 0 ? nullptr : merged + n * kk;
    keys = merged;
    return W2B_OK;
  }
  hipError_t timed(int64_t n, int64_t np, const Rows3 &d) {
    const uint32_t *B32 = (const uint32_t *)e->B;
    hipError_t le = w2b_launch_bits_planes(B32, (int)(2 * e->wpr), (int)e->size, (int)n, np, d.d1, d.d2, d.d3, e->P, e->stream);
    if (le != hipSuccess) return le;
    return k == 0 ? w2b_launch_bits_top1(B32, (int)e->words, (int)e->size, e->P, np, (int)n, d.d1, d.d2, d.d3, e->best, e->stream)
                  : w2b_launch_bits_topk(B32, (int)e->words, (int)e->size, e->P, np, (int)n, d.d1, d.d2, d.d3, k, splits, rpb,
                                         slots, merged, e->stream);
  }
  // the signed multi-word question (k >= 1): four planes per question, the bit-sliced scan, the same merge
  hipError_t timed(int64_t n, int64_t np, const Terms &d) {
    const uint32_t *B32 = (const uint32_t *)e->B;
    hipError_t le = w2b_launch_combine_planes(B32, (int)(2 * e->wpr), (int)e->size, (int)n, np, d.drows, d.dsigns, e->P4, e->stream);
    if (le != hipSuccess) return le;
    return w2b_launch_combine_bits(B32, (int)e->words, (int)e->size, e->P4, np, (int)n, d.drows, k, splits, rpb, slots, merged,
                                   e->stream);
  }
  float score(unsigned long long key) const { return (float)(int32_t)(key >> 32) / (float)e->size; }   // one correctly rounded division
};

// The 3CosMul question (include/word2bits_eval.h, "3CosMul"): the chunks, scratch and selection state of the three-row scans
// above, another scan kernel, float keys on both handle kinds.
struct ScanCosmulBits : ScanBits {
  using ScanBits::ScanBits;
  hipError_t timed(int64_t n, int64_t, const Rows3 &d) {
    return w2b_launch_cosmul_bits((const uint32_t *)e->B, (int)e->words, (int)e->size, e->utab, (int)n, d.d1, d.d2, d.d3, k,
                                  splits, rpb, slots, merged, e->stream);
  }
  float score(unsigned long long key) const { return f32_score(key); }
};
struct ScanCosmulCodes : ScanCodes {
  using ScanCodes::ScanCodes;
  hipError_t timed(int64_t n, int64_t, const Rows3 &d) {
    const uint32_t *B32 = (const uint32_t *)e->B;
    hipError_t le = w2b_launch_codes_operands(B32, (int)e->size, (int)n, e->wrow, d.d1, d.d2, d.d3, e->P, e->Q, e->stream);
    if (le != hipSuccess) return le;
    return w2b_launch_codes_scan_cosmul(B32, (int)e->words, (int)e->size, e->wrow, e->P, e->Q, (int)n, d.d1, d.d2, d.d3, k,
                                        t.bound, t.bkt, t.slots, t.cnt, t.merged, e->stream);
  }
};

struct EventPair;

// The bags of w2b_eval_bag.  A chunk's ids go up as they are, its bounds rebased to the chunk's first id; with `exclude`
// also every question's own rows, sorted and without repeats, and their bounds.  One device buffer, in this order:
// N_T [np32] (64-bit), wq [np32], bounds [n + 1], own bounds [n + 1], ids, own rows (np32 = n rounded up to 32).
struct Bags {
  const int32_t *ids;
  const int64_t *offsets;
  bool exclude;
  std::vector<int32_t> h_off, h_xoff, h_x;      // what the asynchronous copies read
  unsigned long long *d_nt = nullptr;
  float *d_wq = nullptr;
  int32_t *d_off = nullptr, *d_xoff = nullptr, *d_ids = nullptr, *d_x = nullptr;
  int64_t np32 = 0;
  int upload(w2b_eval *e, int64_t q0, int64_t n, int64_t) {
    const int64_t i0 = offsets[q0], m = offsets[q0 + n] - i0;
    h_off.resize((size_t)n + 1);
    for (int64_t q = 0; q <= n; q++) h_off[(size_t)q] = (int32_t)(offsets[q0 + q] - i0);
    h_xoff.assign(1, 0);
    h_x.clear();
    if (exclude)
      for (int64_t q = 0; q < n; q++) {
        const size_t at = h_x.size();
        for (int64_t i = offsets[q0 + q]; i < offsets[q0 + q + 1]; i++)
          if (ids[i] >= 0) h_x.push_back(ids[i]);
        std::sort(h_x.begin() + (long)at, h_x.end());
        h_x.erase(std::unique(h_x.begin() + (long)at, h_x.end()), h_x.end());
        h_xoff.push_back((int32_t)h_x.size());
      }
    np32 = (n + 31) / 32 * 32;
    const size_t ints = 2 * ((size_t)n + 1) + (size_t)m + h_x.size();
    if (eval_reserve_bag(&e->bag_buf, &e->bag_bytes, (size_t)np32 * 12 + ints * 4) != W2B_OK)
      return efail(W2B_ENOMEM, "w2b_eval_bag: device allocation failed");
    d_nt = (unsigned long long *)e->bag_buf;
    d_wq = (float *)(d_nt + np32);
    d_off = (int32_t *)(d_wq + np32);
    d_xoff = d_off + n + 1;
    d_ids = d_xoff + n + 1;
    d_x = d_ids + m;
    EHIP(hipMemcpyAsync(d_off, h_off.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, e->stream));
    if (m > 0) EHIP(hipMemcpyAsync(d_ids, ids + i0, (size_t)m * 4, hipMemcpyHostToDevice, e->stream));
    if (exclude) {
      EHIP(hipMemcpyAsync(d_xoff, h_xoff.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, e->stream));
      if (!h_x.empty()) EHIP(hipMemcpyAsync(d_x, h_x.data(), h_x.size() * 4, hipMemcpyHostToDevice, e->stream));
    }
    return W2B_OK;
  }
};

// The bag question on a bits or a codes handle (include/word2bits_eval.h, "bag questions"): two digit planes per question,
// the i8 scan, the selection state and the merge of the codes scan.  A chunk is sized so that its operands and its
// selection state stay within the budget, never below one 32-question tile.
struct ScanBag {
  w2b_eval *e;
  int32_t k;
  TopkScratch t;
  int64_t chunk, kk;
  const unsigned long long *keys = nullptr;
  ScanBag(w2b_eval *e_, int32_t k_) : e(e_), k(k_), kk(k_) {
    t.k = k;
    w2b_codes_topk_layout(e->words, (int)e->size, k, &t.nunits, &t.cap);
    (void)t.chunk(0);                                                   // (sets per_q)
    const int64_t per_q = t.per_q + 64 * ((e->size + 31) / 32);
    const int64_t budget = e->tk_budget > 0 ? e->tk_budget : kTopkScratch;
    chunk = budget / per_q / 32 * 32;
    if (chunk < 32) chunk = 32;
    if (chunk > kChunkQ) chunk = kChunkQ;
  }
  size_t scratch(int64_t n) const { return t.bytes(n); }
  int before(int64_t n, int64_t np, const Bags &d);
  hipError_t timed(int64_t n, int64_t, const Bags &d) {
    return w2b_launch_bag_scan((const uint32_t *)e->B, (int)e->words, (int)e->size, e->codes ? 2 : 1, e->wrow, e->bag_T, d.d_wq,
                               (int)n, d.d_x, d.exclude ? d.d_xoff : nullptr, k, t.bound, t.bkt, t.slots, t.cnt, t.merged,
                               e->stream);
  }
  float score(unsigned long long key) const {
    return e->codes ? f32_score(key) : (float)(int32_t)(key >> 32) / (float)e->size;   // bits: one correctly rounded division
  }
};

// The questions of w2b_eval_vectors: x [nq][size] on the host and their weights wx [nq].  A packed handle gets a chunk's
// weights [w2b_vec_weight_slots(n)] and vectors [n][size] in one device buffer; an fp32 handle gets vec = x * wx, one float32
// multiply per column, which ScanVectorsF::before copies into the zeroed query matrix, and a list of rows to exclude that
// names no row (W2B_EVAL_XSTRIDE times -1 per question).
struct Vectors {
  const float *x;
  const float *wx;
  std::vector<float> h_w, h_vec;                // what the asynchronous copies read
  float *d_w = nullptr, *d_x = nullptr;
  int32_t *d_none = nullptr;
  int upload(w2b_eval *e, int64_t q0, int64_t n, int64_t np) {
#pragma clang fp contract(off)
    const int64_t size = e->size;
    if (e->bits || e->codes) {
      const int64_t slots = w2b_vec_weight_slots(n);
      if (eval_reserve_bag(&e->bag_buf, &e->bag_bytes, (size_t)(slots + n * size) * 4) != W2B_OK)
        return efail(W2B_ENOMEM, "w2b_eval_vectors: device allocation failed");
      d_w = (float *)e->bag_buf;
      d_x = d_w + slots;
      h_w.assign((size_t)slots, 0.f);
      std::copy(wx + q0, wx + q0 + n, h_w.begin());
      EHIP(hipMemcpyAsync(d_w, h_w.data(), (size_t)slots * 4, hipMemcpyHostToDevice, e->stream));
      EHIP(hipMemcpyAsync(d_x, x + q0 * size, (size_t)(n * size) * 4, hipMemcpyHostToDevice, e->stream));
      return W2B_OK;
    }
    if (eval_reserve_terms(e, np) != W2B_OK) return efail(W2B_ENOMEM, "w2b_eval_vectors: device allocation failed");
    d_none = e->terms;
    EHIP(hipMemsetAsync(d_none, 0xFF, (size_t)n * W2B_EVAL_XSTRIDE * 4, e->stream));
    h_vec.resize((size_t)(n * size));
    for (int64_t q = 0; q < n; q++)
      for (int64_t a = 0; a < size; a++) h_vec[(size_t)(q * size + a)] = x[(q0 + q) * size + a] * wx[q0 + q];
    return W2B_OK;
  }
};

// fp32 rows: the uploaded query vectors, then the list form of the top-k scan with nothing to exclude
struct ScanVectorsF : ScanTopK {
  using ScanTopK::ScanTopK;
  int before(int64_t n, int64_t np, const Vectors &d) {
    if (int rc = clear(n, np)) return rc;
    EHIP(hipMemcpy2DAsync(e->Q, (size_t)e->ld * 4, d.h_vec.data(), (size_t)e->size * 4, (size_t)e->size * 4, (size_t)n,
                          hipMemcpyHostToDevice, e->stream));
    return W2B_OK;
  }
  hipError_t timed(int64_t n, int64_t, const Vectors &d) {
    return w2b_launch_eval_topk_list(e->Q, e->M, (int)n, (int)e->words, (int)e->size, (int)e->ld, e->fused, d.d_none, k, t.bound,
                                     t.bkt, t.slots, t.cnt, t.merged, e->variant, e->stream);
  }
};

// The vector question on a bits or a codes handle (include/word2bits_eval.h, "vector questions"): the operands in fragment
// order, the f32 matrix-core scan on the packed rows, the selection state and the merge of the codes scan.  A chunk is sized
// so that its vectors, their operands and its selection state stay within the budget, never below one 32-question tile.
struct ScanVectors {
  w2b_eval *e;
  int32_t k;
  TopkScratch t;
  int64_t chunk, kk;
  const unsigned long long *keys = nullptr;
  ScanVectors(w2b_eval *e_, int32_t k_) : e(e_), k(k_), kk(k_) {
    t.k = k;
    w2b_vec_topk_layout(e->words, k, &t.nunits, &t.cap);
    (void)t.chunk(0);                                                   // (sets per_q)
    const int64_t per_q = t.per_q + 4 * e->size + 32 * ((e->size + 7) / 8) + 4;
    const int64_t budget = e->tk_budget > 0 ? e->tk_budget : kTopkScratch;
    chunk = budget / per_q / 32 * 32;
    if (chunk < 32) chunk = 32;
    if (chunk > kChunkQ) chunk = kChunkQ;
  }
  size_t scratch(int64_t n) const { return t.bytes(n); }
  int before(int64_t n, int64_t, const Vectors &) {
    if (eval_reserve_bag(&e->bag_T, &e->bag_T_bytes, w2b_vec_operand_bytes((int)e->size, n)) != W2B_OK)
      return efail(W2B_ENOMEM, "w2b_eval_vectors: device allocation failed");
    EHIP(hipMemsetAsync(e->tk_buf, 0, t.place(e->tk_buf, n), e->stream));
    keys = t.merged;
    return W2B_OK;
  }
  hipError_t timed(int64_t n, int64_t, const Vectors &d) {
    const hipError_t le = w2b_launch_vec_operands(d.d_x, (int)e->size, (int)n, e->bag_T, e->stream);
    if (le != hipSuccess) return le;
    return w2b_launch_vec_scan(e->B, (int)e->words, (int)e->size, e->codes ? 2 : 1, e->wrow,
                               (float)(1.0 / sqrt((double)e->size)), e->bag_T, d.d_w, (int)n, k, t.bound, t.bkt, t.slots, t.cnt,
                               t.merged, e->stream);
  }
  float score(unsigned long long key) const { return f32_score(key); }
};

struct EventPair {   // the two ends of a timed window
  hipEvent_t t[2] = {nullptr, nullptr};
  hipError_t create() {
    hipError_t he = hipSuccess;
    for (hipEvent_t &x : t)
      if (he == hipSuccess) he = hipEventCreate(&x);
    return he;
  }
  ~EventPair() {
    for (hipEvent_t x : t)
      if (x) (void)hipEventDestroy(x);
  }
};

// The operands are built ahead of the scan's window, in a window of their own that is added to the kernel time: on a codes
// handle the host has to see N_T between the two (wq = 1 / sqrt(N_T) in correctly rounded double operations, the
// expression of w(r), which the host also builds).
int ScanBag::before(int64_t n, int64_t, const Bags &d) {
  const size_t tbytes = w2b_bag_operand_bytes((int)e->size, n);
  if (eval_reserve_bag(&e->bag_T, &e->bag_T_bytes, tbytes) != W2B_OK) return efail(W2B_ENOMEM, "w2b_eval_bag: device allocation failed");
  EHIP(hipMemsetAsync(e->tk_buf, 0, t.place(e->tk_buf, n), e->stream));
  keys = t.merged;
  EHIP(hipMemsetAsync(e->bag_T, 0, tbytes, e->stream));
  EHIP(hipMemsetAsync(d.d_nt, 0, (size_t)d.np32 * 12, e->stream));     // N_T and wq
  EventPair ev;
  EHIP(ev.create());
  EHIP(hipEventRecord(ev.t[0], e->stream));
  EHIP(w2b_launch_bag_operands((const uint32_t *)e->B, (int)e->size, e->codes ? 2 : 1, (int)n, d.d_ids, d.d_off, e->bag_T, d.d_nt,
                               e->stream));
  EHIP(hipEventRecord(ev.t[1], e->stream));
  std::vector<unsigned long long> nt((size_t)n, 0ull);
  if (e->codes) EHIP(hipMemcpyAsync(nt.data(), d.d_nt, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
  EHIP(hipStreamSynchronize(e->stream));
  float ms = 0;
  EHIP(hipEventElapsedTime(&ms, ev.t[0], ev.t[1]));
  e->kernel_ms += ms;
  if (e->codes) {
    std::vector<float> wq((size_t)n);
    for (int64_t q = 0; q < n; q++) wq[(size_t)q] = bag_weight(nt[(size_t)q]);
    EHIP(hipMemcpy(d.d_wq, wq.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  }
  return W2B_OK;
}
}  // namespace

// `terms` = accumulator tiles per (question, row) for the multiply-add count; 0 = what the handle's three-row scan has
template <class Scan, class In>
static int eval_scan_chunks(w2b_eval *e, Scan &&m, In in, int64_t nq, int32_t *best, float *bestd, const std::string &who,
                            double terms = 0) {
  std::vector<unsigned long long> keys;
  for (int64_t q0 = 0; q0 < nq; q0 += m.chunk) {
    const int64_t n = (nq - q0 < m.chunk) ? nq - q0 : m.chunk;
    const int64_t np = (n + kTile - 1) / kTile * kTile;
    if (eval_reserve_questions(e, np) != W2B_OK || eval_reserve_topk(e, m.scratch(n)) != W2B_OK)
      return efail(W2B_ENOMEM, who + ": device allocation failed");
    if (int rc = in.upload(e, q0, n, np)) return rc;
    if (int rc = m.before(n, np, in)) return rc;
    EventPair ev;
    EHIP(ev.create());
    EHIP(hipEventRecord(ev.t[0], e->stream));
    hipError_t le = m.timed(n, np, in);
    if (le == hipSuccess) le = hipEventRecord(ev.t[1], e->stream);
    keys.assign((size_t)(n * m.kk), 0ull);   // (no rows: nothing is launched and every list is empty)
    if (le == hipSuccess && e->words > 0)
      le = hipMemcpyAsync(keys.data(), m.keys, (size_t)(n * m.kk) * 8, hipMemcpyDeviceToHost, e->stream);
    if (le == hipSuccess) le = hipStreamSynchronize(e->stream);
    float ms = 0;
    if (le == hipSuccess) le = hipEventElapsedTime(&ms, ev.t[0], ev.t[1]);
    if (le != hipSuccess) return efail(W2B_EHIP, who + ": " + hipGetErrorString(le));
    e->kernel_ms += ms;
    e->launches++;
    e->macs += (terms > 0 ? terms : e->codes ? 3.0 : 1.0) * (double)n * (double)e->words * (double)e->size;   // algorithmic: padding is not work
    for (int64_t i = 0; i < n * m.kk; i++) {
      const unsigned long long key = keys[(size_t)i];
      best[q0 * m.kk + i] = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)) : -1;
      if (bestd) bestd[q0 * m.kk + i] = m.score(key);
    }
  }
  return W2B_OK;
}

// all three public queries: the checks, then the form of the scan.  k = 0 asks for the best row alone.
static int eval_scan(w2b_eval *e, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3, bool topk, int32_t k,
                     int32_t *best, float *bestd, const std::string &who) {
  if (!e || nq < 0 || (nq > 0 && (!b1 || !b2 || !b3 || !best))) return efail(W2B_EINVAL, who + ": bad argument");
  if (topk && (k < 1 || k > W2B_EVAL_MAX_K)) return efail(W2B_EINVAL, who + ": k must be 1..64");
  for (int64_t q = 0; q < nq; q++)
    if (b1[q] < 0 || b1[q] >= e->words || b2[q] < 0 || b2[q] >= e->words || b3[q] < 0 || b3[q] >= e->words)
      return efail(W2B_EINVAL, who + ": question row out of range");
  EHIP(hipSetDevice(e->device));
  const Rows3 in{b1, b2, b3};
  if (e->bits) return eval_scan_chunks(e, ScanBits(e, nq, k), in, nq, best, bestd, who);
  if (e->codes) return eval_scan_chunks(e, ScanCodes(e, k), in, nq, best, bestd, who);
  if (topk) return eval_scan_chunks(e, ScanTopK(e, k), in, nq, best, bestd, who);
  return eval_scan_chunks(e, ScanTop1{e}, in, nq, best, bestd, who);
}

// The signed multi-word question: the checks, the slots of every question compacted (used slots first, in slot order),
// then the list form of the top-k scan.
extern "C" int w2b_eval_combine(w2b_eval *e, int64_t nq, int32_t nt, const int32_t *rows, const int8_t *signs, int32_t k,
                                int32_t *best, float *bestd) {
  const std::string who = "w2b_eval_combine";
  if (!e || nq < 0 || (nq > 0 && (!rows || !signs || !best))) return efail(W2B_EINVAL, who + ": bad argument");
  if (e->codes) return efail(W2B_EINVAL, who + ": not available in codes mode");
  if (nt < 1 || nt > W2B_EVAL_MAX_TERMS) return efail(W2B_EINVAL, who + ": the number of terms must be 1..7");
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, who + ": k must be 1..64");
  std::vector<int32_t> xr((size_t)nq * W2B_EVAL_XSTRIDE, -1), xs((size_t)nq * W2B_EVAL_XSTRIDE, 0);
  for (int64_t q = 0; q < nq; q++) {
    if (const char *why = bad_terms(nt, rows + q * nt, signs + q * nt, e->words)) return efail(W2B_EINVAL, who + ": " + why);
    size_t at = (size_t)q * W2B_EVAL_XSTRIDE;
    for (int32_t t = 0; t < nt; t++)
      if (signs[q * nt + t] != 0) {
        xr[at] = rows[q * nt + t];
        xs[at++] = signs[q * nt + t];
      }
  }
  EHIP(hipSetDevice(e->device));
  const Terms in{xr.data(), xs.data()};
  if (e->bits) return eval_scan_chunks(e, ScanBits(e, nq, k), in, nq, best, bestd, who);
  return eval_scan_chunks(e, ScanCombine(e, k), in, nq, best, bestd, who);
}

// The bag question: every check first -- those that need no handle, then the handle, then the ids -- and then the chunks.
extern "C" int w2b_eval_bag(w2b_eval *e, int64_t n_ids, const int32_t *ids, int64_t nq, const int64_t *offsets,
                            int32_t exclude_own, int32_t k, int32_t *best, float *bestd) {
  const std::string who = "w2b_eval_bag";
  if (nq < 0 || n_ids < 0 || (nq > 0 && (!offsets || !best)) || (n_ids > 0 && !ids)) return efail(W2B_EINVAL, who + ": bad argument");
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, who + ": k must be 1..64");
  if (exclude_own != 0 && exclude_own != 1) return efail(W2B_EINVAL, who + ": exclude_own must be 0 or 1");
  if (nq == 0 ? n_ids != 0 : (offsets[0] != 0 || offsets[nq] != n_ids))
    return efail(W2B_EINVAL, who + ": offsets must start at 0 and end at n_ids");
  for (int64_t q = 0; q < nq; q++) {
    if (offsets[q + 1] < offsets[q] || offsets[q + 1] > n_ids) return efail(W2B_EINVAL, who + ": offsets must not decrease");
    if (offsets[q + 1] - offsets[q] > W2B_EVAL_MAX_BAG) return efail(W2B_EINVAL, who + ": a bag holds at most 4096 ids");
  }
  if (!e) return efail(W2B_EINVAL, who + ": null handle");
  if (!e->bits && !e->codes) return efail(W2B_EINVAL, who + ": needs a bits or a codes handle");
  if (e->size > kBagMaxSize) return efail(W2B_EINVAL, who + ": size must be at most 58254 (9 * 4096 * size < 2^31)");
  for (int64_t i = 0; i < n_ids; i++)
    if (ids[i] >= e->words) return efail(W2B_EINVAL, who + ": bag id out of range");
  if (nq == 0) return W2B_OK;
  EHIP(hipSetDevice(e->device));
  Bags in{ids, offsets, exclude_own == 1};
  return eval_scan_chunks(e, ScanBag(e, k), std::move(in), nq, best, bestd, who, 2.0);
}

// The vector question: what does not depend on the handle first, then the handle, then the values; the weights; the chunks.
extern "C" int w2b_eval_vectors(w2b_eval *e, int64_t nq, const float *x, int32_t normalize, int32_t k, int32_t *best,
                                float *bestd) {
  const std::string who = "w2b_eval_vectors";
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, who + ": k must be 1..64");
  if (normalize != 0 && normalize != 1) return efail(W2B_EINVAL, who + ": normalize must be 0 or 1");
  if (nq < 0 || (nq > 0 && (!x || !best))) return efail(W2B_EINVAL, who + ": bad argument");
  if (!e) return efail(W2B_EINVAL, who + ": null handle");
  for (int64_t q = 0; q < nq; q++) {
    const int64_t bad = bad_vector_value(x + q * e->size, e->size);
    if (bad >= 0)
      return efail(W2B_EINVAL, who + ": question " + std::to_string(q) + ", column " + std::to_string(bad) + ": " + kVectorRange);
  }
  if (nq == 0) return W2B_OK;
  std::vector<float> wx((size_t)nq);
  for (int64_t q = 0; q < nq; q++) wx[(size_t)q] = vector_weight(x + q * e->size, e->size, normalize);
  EHIP(hipSetDevice(e->device));
  Vectors in{x, wx.data()};
  if (e->bits || e->codes) return eval_scan_chunks(e, ScanVectors(e, k), std::move(in), nq, best, bestd, who, 1.0);
  return eval_scan_chunks(e, ScanVectorsF(e, k), std::move(in), nq, best, bestd, who, 1.0);
}

// The 3CosMul question: what does not depend on the handle first, then the handle, then the rows; the chunks.
extern "C" int w2b_eval_cosmul(w2b_eval *e, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3, int32_t k,
                               int32_t *best, float *bestd) {
  const std::string who = "w2b_eval_cosmul";
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, who + ": k must be 1..64");
  if (nq < 0 || (nq > 0 && (!b1 || !b2 || !b3 || !best))) return efail(W2B_EINVAL, who + ": bad argument");
  if (!e) return efail(W2B_EINVAL, who + ": null handle");
  if (!e->bits && !e->codes)
    return efail(W2B_EINVAL, who + ": not available on an fp32 handle: load the file with bits or codes");
  if (e->bits && e->size > kCosmulMaxBits) return efail(W2B_EINVAL, who + ": size must be at most 2^24 on a bits handle");
  for (int64_t q = 0; q < nq; q++)
    if (b1[q] < 0 || b1[q] >= e->words || b2[q] < 0 || b2[q] >= e->words || b3[q] < 0 || b3[q] >= e->words)
      return efail(W2B_EINVAL, who + ": question " + std::to_string(q) + ": row out of range");
  if (nq == 0) return W2B_OK;
  EHIP(hipSetDevice(e->device));
  if (e->bits && !e->utab) {
    const std::vector<float> u = cosmul_utab(e->size);
    if (hipMalloc(&e->utab, u.size() * 4) != hipSuccess) return efail(W2B_ENOMEM, who + ": device allocation failed");
    EHIP(hipMemcpy(e->utab, u.data(), u.size() * 4, hipMemcpyHostToDevice));
  }
  const Rows3 in{b1, b2, b3};
  if (e->bits) return eval_scan_chunks(e, ScanCosmulBits(e, nq, k), in, nq, best, bestd, who, 3.0);
  return eval_scan_chunks(e, ScanCosmulCodes(e, k), in, nq, best, bestd, who, 3.0);
}

// ------------------------------------------------------------------------------------ documents
// The corpus of the document question: every check first -- what needs no handle, then the handle, then the ids -- then the
// ids >= 0 alone go to the device with their own bounds (padding contributes nothing, so the walk never sees it).
extern "C" int w2b_eval_docs_set(w2b_eval *e, int64_t n_ids, const int32_t *ids, int64_t n_docs, const int64_t *offsets) {
  const std::string who = "w2b_eval_docs_set";
  if (n_docs > kDocsMaxDocs) return efail(W2B_EINVAL, who + ": at most 0x7FFFFF00 documents");
  const std::string why = bad_texts(n_ids, ids, n_docs, offsets, "document");
  if (!why.empty()) return efail(W2B_EINVAL, who + ": " + why);
  if (!e) return efail(W2B_EINVAL, who + ": null handle");
  if (!e->bits && !e->codes) return efail(W2B_EINVAL, who + ": " + kDocsFp32);
  if (e->size >= kDocsMaxSize) return efail(W2B_EINVAL, who + ": " + kDocsSize);
  if (bad_text_ids(n_ids, ids, e->words)) return efail(W2B_EINVAL, who + ": document id out of range");
  EHIP(hipSetDevice(e->device));
  EHIP(hipStreamSynchronize(e->stream));          // (every call ends synchronised: nothing reads the corpus that is replaced)
  std::vector<int32_t> h_ids;
  std::vector<long long> h_off((size_t)n_docs + 1, 0);
  h_ids.reserve((size_t)n_ids);
  for (int64_t d = 0; d < n_docs; d++) {
    for (int64_t i = offsets[d]; i < offsets[d + 1]; i++)
      if (ids[i] >= 0) h_ids.push_back(ids[i]);
    h_off[(size_t)d + 1] = (long long)h_ids.size();
  }
  int32_t *d_ids = nullptr;
  long long *d_off = nullptr;
  if (n_docs > 0) {
    if (hipMalloc(&d_ids, h_ids.size() * 4 + 4) != hipSuccess || hipMalloc(&d_off, h_off.size() * 8) != hipSuccess) {
      if (d_ids) (void)hipFree(d_ids);
      return efail(W2B_ENOMEM, who + ": device allocation failed");
    }
    hipError_t he = hipMemcpy(d_off, h_off.data(), h_off.size() * 8, hipMemcpyHostToDevice);
    if (he == hipSuccess && !h_ids.empty()) he = hipMemcpy(d_ids, h_ids.data(), h_ids.size() * 4, hipMemcpyHostToDevice);
    if (he != hipSuccess) {
      (void)hipFree(d_ids);
      (void)hipFree(d_off);
      return efail(W2B_EHIP, who + ": " + hipGetErrorString(he));
    }
  }
  if (e->docs_ids) (void)hipFree(e->docs_ids);
  if (e->docs_off) (void)hipFree(e->docs_off);
  e->docs_ids = d_ids;
  e->docs_off = d_off;
  e->docs_n = n_docs;
  e->docs_positions = n_ids;
  return W2B_OK;
}

extern "C" int64_t w2b_eval_docs_count(const w2b_eval *e) { return e ? e->docs_n : 0; }

namespace {
inline int64_t docs_pad16(int64_t m) { return (m + 15) / 16 * 16; }
inline size_t docs_align(size_t b) { return (b + 255) / 256 * 256; }
}  // namespace

// The document question: every check first, then the chunks of queries.  A chunk is the longest run of queries whose
// scratch stays within the bound of w2b_eval_set_topk_scratch, never less than one query; per chunk the pair table (timed
// as the table phase), then the walk and the merge (the walk phase).
extern "C" int w2b_eval_docs(w2b_eval *e, int64_t n_qids, const int32_t *qids, int64_t nq, const int64_t *qoffsets,
                             int32_t symmetric, int32_t k, int32_t *best, float *bestd, float *all_scores) {
  const std::string who = "w2b_eval_docs";
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, who + ": k must be 1..64");
  if (symmetric != 0 && symmetric != 1) return efail(W2B_EINVAL, who + ": symmetric must be 0 or 1");
  if (nq > 0 && !best) return efail(W2B_EINVAL, who + ": bad argument");
  const std::string why = bad_texts(n_qids, qids, nq, qoffsets, "query");
  if (!why.empty()) return efail(W2B_EINVAL, who + ": " + why);
  if (nq == 0) return W2B_OK;                      // nothing is asked: no handle and no corpus is needed
  if (!e) return efail(W2B_EINVAL, who + ": null handle");
  if (!e->bits && !e->codes) return efail(W2B_EINVAL, who + ": " + kDocsFp32);
  if (e->size >= kDocsMaxSize) return efail(W2B_EINVAL, who + ": " + kDocsSize);
  if (e->docs_n == 0) return efail(W2B_EINVAL, who + ": no corpus is set (w2b_eval_docs_set)");
  if (all_scores && (__int128)nq * e->docs_n > kDocsMaxAll)
    return efail(W2B_EINVAL, who + ": all_scores holds at most 2^28 scores (nq * n_docs)");
  if (bad_text_ids(n_qids, qids, e->words)) return efail(W2B_EINVAL, who + ": query id out of range");
  e->docs_table_ms = e->docs_walk_ms = 0;
  EHIP(hipSetDevice(e->device));
  const int64_t words = e->words, n_docs = e->docs_n;
  const int bl = e->codes ? 2 : 1;
  const int64_t splits = (n_docs + W2B_DOCS_PER_BLOCK - 1) / W2B_DOCS_PER_BLOCK;
  const int64_t budget = e->tk_budget > 0 ? e->tk_budget : kTopkScratch;
  // one query's own need: its columns of the table and its column of row maxima, its slots and merged keys, its scores
  auto need = [&](int64_t m) {
    return (docs_pad16(m) + 1) * words * 4 + (splits + 1) * k * 8 + (all_scores ? n_docs * 4 : 0);
  };
  std::vector<int32_t> h_col, h_qcol, h_qm;
  std::vector<unsigned long long> keys;
  std::vector<float> h_all;
  EventPair ev, ev2;
  EHIP(ev.create());
  EHIP(ev2.create());
  for (int64_t q0 = 0; q0 < nq;) {
    // the chunk: its queries side by side as columns, each one's ids >= 0 first, padded to a whole 64-byte line
    h_col.clear();
    h_qcol.assign(1, 0);
    h_qm.clear();
    int64_t n = 0, used = 0, positions = 0;
    while (q0 + n < nq && n < 32768) {
      int64_t m = 0;
      for (int64_t i = qoffsets[q0 + n]; i < qoffsets[q0 + n + 1]; i++) m += qids[i] >= 0;
      if (n > 0 && used + need(m) > budget) break;
      used += need(m);
      for (int64_t i = qoffsets[q0 + n]; i < qoffsets[q0 + n + 1]; i++)
        if (qids[i] >= 0) h_col.push_back(qids[i]);
      h_col.resize((size_t)(h_qcol.back() + docs_pad16(m)), -1);
      h_qcol.push_back((int32_t)h_col.size());
      h_qm.push_back((int32_t)m);
      positions += qoffsets[q0 + n + 1] - qoffsets[q0 + n];
      n++;
    }
    const int64_t tcols = (int64_t)h_col.size();
    // one buffer for the chunk's descriptors, one for its scratch
    const size_t o_qcol = docs_align((size_t)tcols * 4), o_qm = o_qcol + docs_align((size_t)(n + 1) * 4);
    if (eval_reserve_bag(&e->bag_buf, &e->bag_bytes, o_qm + docs_align((size_t)n * 4)) != W2B_OK)
      return efail(W2B_ENOMEM, who + ": device allocation failed");
    int32_t *d_col = (int32_t *)e->bag_buf, *d_qcol = (int32_t *)((char *)e->bag_buf + o_qcol),
            *d_qm = (int32_t *)((char *)e->bag_buf + o_qm);
    const size_t o_rmax = docs_align((size_t)words * (size_t)tcols * 4), o_slots = o_rmax + docs_align((size_t)words * (size_t)n * 4);
    const size_t o_merged = o_slots + docs_align((size_t)n * (size_t)splits * k * 8), o_all = o_merged + docs_align((size_t)n * k * 8);
    if (eval_reserve_topk(e, o_all + (all_scores ? docs_align((size_t)n * (size_t)n_docs * 4) : 0) + 256) != W2B_OK)
      return efail(W2B_ENOMEM, who + ": device allocation failed");
    char *tk = (char *)e->tk_buf;
    unsigned long long *d_slots = (unsigned long long *)(tk + o_slots), *d_merged = (unsigned long long *)(tk + o_merged);
    float *d_all = all_scores ? (float *)(tk + o_all) : nullptr;
    if (tcols > 0) EHIP(hipMemcpyAsync(d_col, h_col.data(), (size_t)tcols * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemcpyAsync(d_qcol, h_qcol.data(), (size_t)(n + 1) * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemcpyAsync(d_qm, h_qm.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipEventRecord(ev.t[0], e->stream));
    hipError_t le = w2b_launch_docs_table((const uint32_t *)e->B, (int)words, (int)e->size, bl, e->wrow, d_col, (int)tcols, d_qcol,
                                          d_qm, (int)n, tk, tk + o_rmax, e->stream);
    if (le == hipSuccess) le = hipEventRecord(ev.t[1], e->stream);
    if (le == hipSuccess) le = hipEventRecord(ev2.t[0], e->stream);
    if (le == hipSuccess)
      le = w2b_launch_docs_walk(tk, tk + o_rmax, (int)tcols, (int)n, (int)e->size, bl, d_qcol, d_qm, e->docs_ids, e->docs_off, n_docs,
                                symmetric, k, d_slots, d_merged, d_all, e->stream);
    if (le == hipSuccess) le = hipEventRecord(ev2.t[1], e->stream);
    keys.assign((size_t)(n * k), 0ull);
    if (le == hipSuccess) le = hipMemcpyAsync(keys.data(), d_merged, (size_t)(n * k) * 8, hipMemcpyDeviceToHost, e->stream);
    if (all_scores) {
      h_all.resize((size_t)(n * n_docs));
      if (le == hipSuccess) le = hipMemcpyAsync(h_all.data(), d_all, h_all.size() * 4, hipMemcpyDeviceToHost, e->stream);
    }
    if (le == hipSuccess) le = hipStreamSynchronize(e->stream);
    float ms = 0, ms2 = 0;
    if (le == hipSuccess) le = hipEventElapsedTime(&ms, ev.t[0], ev.t[1]);
    if (le == hipSuccess) le = hipEventElapsedTime(&ms2, ev2.t[0], ev2.t[1]);
    if (le != hipSuccess) return efail(W2B_EHIP, who + ": " + hipGetErrorString(le));
    e->docs_table_ms += ms;
    e->docs_walk_ms += ms2;
    e->kernel_ms += (double)ms + (double)ms2;
    e->launches++;
    e->macs += (double)positions * (double)e->docs_positions * (double)e->size;
    for (int64_t i = 0; i < n * k; i++) {
      const unsigned long long key = keys[(size_t)i];
      best[q0 * k + i] = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)) : -1;
      if (bestd) bestd[q0 * k + i] = f32_score(key);
    }
    if (all_scores) std::copy(h_all.begin(), h_all.end(), all_scores + q0 * n_docs);
    q0 += n;
  }
  return W2B_OK;
}

extern "C" int w2b_eval_docs_timing(w2b_eval *e, double *table_ms, double *walk_ms) {
  if (!e) return efail(W2B_EINVAL, "w2b_eval_docs_timing: null handle");
  if (table_ms) *table_ms = e->docs_table_ms;
  if (walk_ms) *walk_ms = e->docs_walk_ms;
  return W2B_OK;
}

// ------------------------------------------------------------------------------------ pair similarity
namespace {
constexpr int64_t kPairsChunk = 1 << 20;         // pairs per launch at most
constexpr int64_t kPairsChunkIds = 1ll << 30;    // ids per launch at most: the chunk's bounds are 32-bit
constexpr int64_t kPairsMinChunk = 64;           // pairs that a launch takes whatever the budget is
constexpr int64_t kPairsPerPair = 36;            // staging bytes of a pair beside its ids: two bounds, a path entry, the parts
}  // namespace

// The pair question: every check first -- what needs no handle, then the handle, then the ids -- then chunks of whole pairs.
// A chunk's staging is one device buffer: parts [n][3] (64-bit), bounds [2 n + 1], the pairs sorted by path [n], the ids.  The
// integers of all chunks are collected first and the outputs written at the end: an error in a later chunk leaves them untouched.
extern "C" int w2b_eval_pairs(w2b_eval *e, int64_t n_ids, const int32_t *ids, int64_t np, const int64_t *offsets, float *score,
                              int64_t *parts) {
  const std::string who = "w2b_eval_pairs";
  const std::string why = bad_pairs(n_ids, ids, np, offsets, score, parts);
  if (!why.empty()) return efail(W2B_EINVAL, who + ": " + why);
  if (np > 0 && !score) return efail(W2B_EINVAL, who + ": bad argument");
  if (!e) return efail(W2B_EINVAL, who + ": null handle");
  if (!e->bits && !e->codes) return efail(W2B_EINVAL, who + ": not available on an fp32 handle: load the file with bits or codes");
  if (e->size > kPairsMaxSize) return efail(W2B_EINVAL, who + ": size must be at most 2^24");
  const int64_t bad = bad_pair_id(ids, np, offsets, e->words);
  if (bad >= 0) return efail(W2B_EINVAL, who + ": pair " + std::to_string(bad) + ": id out of range");
  if (np == 0) return W2B_OK;
  EHIP(hipSetDevice(e->device));
  const int bl = e->codes ? 2 : 1;
  const int64_t budget = e->tk_budget > 0 ? e->tk_budget : kTopkScratch;
  std::vector<int64_t> all((size_t)np * 3, 0);
  std::vector<int32_t> h_off, h_list[3], h_sorted;
  EventPair ev;
  EHIP(ev.create());
  for (int64_t p0 = 0; p0 < np;) {
    const int64_t i0 = offsets[2 * p0];
    int64_t n = 0, used = 0;
    while (p0 + n < np && n < kPairsChunk) {
      const int64_t m1 = offsets[2 * (p0 + n) + 2] - offsets[2 * (p0 + n)], need = kPairsPerPair + 4 * m1;
      if (n >= kPairsMinChunk && used + need > budget) break;
      if (n > 0 && offsets[2 * (p0 + n) + 2] - i0 > kPairsChunkIds) break;
      used += need;
      n++;
    }
    const int64_t m = offsets[2 * (p0 + n)] - i0;
    if (e->words > 0) {                            // (no rows: every id is padding and every pair is empty)
      h_off.resize((size_t)(2 * n + 1));
      for (int64_t b = 0; b <= 2 * n; b++) h_off[(size_t)b] = (int32_t)(offsets[2 * p0 + b] - i0);
      for (auto &l : h_list) l.clear();
      for (int64_t q = 0; q < n; q++)
        h_list[w2b_pairs_path(bl, ids + i0, h_off[(size_t)(2 * q)], h_off[(size_t)(2 * q + 1)], h_off[(size_t)(2 * q + 2)])]
            .push_back((int32_t)q);
      h_sorted.clear();
      for (const auto &l : h_list) h_sorted.insert(h_sorted.end(), l.begin(), l.end());
      const size_t o_off = (size_t)n * 24, o_list = o_off + (size_t)(2 * n + 1) * 4, o_ids = o_list + (size_t)n * 4;
      if (eval_reserve_bag(&e->bag_buf, &e->bag_bytes, o_ids + (size_t)m * 4 + 4) != W2B_OK)
        return efail(W2B_ENOMEM, who + ": device allocation failed");
      char *buf = (char *)e->bag_buf;
      long long *d_parts = (long long *)buf;
      int32_t *d_off = (int32_t *)(buf + o_off), *d_list = (int32_t *)(buf + o_list), *d_ids = (int32_t *)(buf + o_ids);
      EHIP(hipMemcpyAsync(d_off, h_off.data(), h_off.size() * 4, hipMemcpyHostToDevice, e->stream));
      EHIP(hipMemcpyAsync(d_list, h_sorted.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
      if (m > 0) EHIP(hipMemcpyAsync(d_ids, ids + i0, (size_t)m * 4, hipMemcpyHostToDevice, e->stream));
      EHIP(hipEventRecord(ev.t[0], e->stream));
      hipError_t le = w2b_launch_pairs(e->B, (int)e->size, bl, d_ids, d_off, d_list, (int)h_list[W2B_PAIRS_PATH_ONE].size(),
                                       (int)h_list[W2B_PAIRS_PATH_SHORT].size(), (int)h_list[W2B_PAIRS_PATH_LONG].size(), d_parts,
                                       e->stream);
      if (le == hipSuccess) le = hipEventRecord(ev.t[1], e->stream);
      if (le == hipSuccess)
        le = hipMemcpyAsync(all.data() + 3 * p0, d_parts, (size_t)n * 24, hipMemcpyDeviceToHost, e->stream);
      if (le == hipSuccess) le = hipStreamSynchronize(e->stream);
      float ms = 0;
      if (le == hipSuccess) le = hipEventElapsedTime(&ms, ev.t[0], ev.t[1]);
      if (le != hipSuccess) return efail(W2B_EHIP, who + ": " + hipGetErrorString(le));
      e->kernel_ms += ms;
    }
    e->launches++;
    e->macs += (double)m * (double)e->size;
    p0 += n;
  }
  for (int64_t p = 0; p < np; p++) score[p] = pair_score(all[(size_t)(3 * p)], all[(size_t)(3 * p + 1)], all[(size_t)(3 * p + 2)]);
  if (parts) memcpy(parts, all.data(), all.size() * 8);
  return W2B_OK;
}

extern "C" int w2b_eval_top1(w2b_eval *e, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3,
                             int32_t *best, float *bestd) {
  return eval_scan(e, nq, b1, b2, b3, false, 0, best, bestd, "w2b_eval_top1");
}

extern "C" int w2b_eval_topk(w2b_eval *e, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3,
                             int32_t k, int32_t *best, float *bestd) {
  return eval_scan(e, nq, b1, b2, b3, true, k, best, bestd, "w2b_eval_topk");
}

// vec = (M[r] - M[r]) + M[r]: M[r] up to the sign of a zero, which no chain that starts at +0 can see
extern "C" int w2b_eval_neighbors(w2b_eval *e, int64_t nq, const int32_t *rows, int32_t k, int32_t *best, float *bestd) {
  return eval_scan(e, nq, rows, rows, rows, true, k, best, bestd, "w2b_eval_neighbors");
}

extern "C" int w2b_eval_set_topk_scratch(w2b_eval *e, int64_t bytes) {
  if (!e || bytes < 0) return efail(W2B_EINVAL, "w2b_eval_set_topk_scratch: bad argument");
  e->tk_budget = bytes;
  return W2B_OK;
}

extern "C" int w2b_eval_set_kernel(w2b_eval *e, int32_t variant) {
  if (!e) return efail(W2B_EINVAL, "w2b_eval_set_kernel: null evaluator");
  if (e->bits || e->codes) return W2B_OK;                             // one kernel: nothing to select
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

// `answer(e, nq, b1, b2, b3, best)` scores all answerable questions at once: best[q] = the answer's row or -1
template <class Answer>
static int eval_transcript(w2b_eval *e, const char *questions, int64_t len, char **out, int64_t *out_len, const char *who,
                           Answer answer) {
  if (!e || !out || len < 0 || (len > 0 && !questions)) return efail(W2B_EINVAL, std::string(who) + ": bad argument");
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
    const int rc = answer(e, (int64_t)b1s.size(), b1s.data(), b2s.data(), b3s.data(), best.data());
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


// ------------------------------------------------------------------------------------ nearest: the text form
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

// the answer text: per line its head, then the error or the list of question `q` in best / bestd [..][k]
std::string query_answers(const w2b_eval *e, const std::vector<QueryLine> &lines, int32_t k, const std::vector<int32_t> &best,
                          const std::vector<float> &bestd) {
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
      appendf(txt, "%d\t%s\t%.6f\n", j + 1, e->vocab.data() + (int64_t)c * kMaxW, (double)bestd[(size_t)(ln.q * k + j)]);
    }
  }
  return txt;
}
}  // namespace

extern "C" int w2b_eval_nearest_text(w2b_eval *e, const char *queries, int64_t len, int32_t k, char **out,
                                     int64_t *out_len) {
  if (!e || !out || len < 0 || (len > 0 && !queries)) return efail(W2B_EINVAL, "w2b_eval_nearest_text: bad argument");
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, "w2b_eval_nearest_text: k must be 1..64");
  *out = nullptr;
  std::vector<QueryLine> lines;
  std::vector<int32_t> b1s, b2s, b3s;
  std::vector<std::string> tok;
  for (int64_t pos = 0; next_query_line(queries, len, pos, tok);) {
    if (tok.empty()) continue;
    QueryLine ln{joined(tok), std::string(), -1};
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
  const std::string txt = query_answers(e, lines, k, best, bestd);
  return text_out(txt, "w2b_eval_nearest_text", out, out_len);
}

// the 3CosMul form: every non-empty line is three words A B C
extern "C" int w2b_eval_cosmul_text(w2b_eval *e, const char *queries, int64_t len, int32_t k, char **out, int64_t *out_len) {
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, "w2b_eval_cosmul_text: k must be 1..64");
  if (!out || len < 0 || (len > 0 && !queries)) return efail(W2B_EINVAL, "w2b_eval_cosmul_text: bad argument");
  if (!e) return efail(W2B_EINVAL, "w2b_eval_cosmul_text: null handle");
  if (!e->bits && !e->codes)
    return efail(W2B_EINVAL, "w2b_eval_cosmul_text: not available on an fp32 handle: load the file with bits or codes");
  *out = nullptr;
  std::vector<QueryLine> lines;
  std::vector<int32_t> b1s, b2s, b3s;
  std::vector<std::string> tok;
  for (int64_t pos = 0; next_query_line(queries, len, pos, tok);) {
    if (tok.empty()) continue;
    QueryLine ln{joined(tok), std::string(), -1};
    if (tok.size() != 3) {
      ln.error = "expected 3 words";
    } else {
      int64_t r[3] = {0, 0, 0};
      for (size_t i = 0; i < 3 && ln.error.empty(); i++) {
        r[i] = w2b_eval_lookup(e, tok[i].c_str());
        if (r[i] == e->words) ln.error = "not in vocabulary: " + tok[i];
      }
      if (ln.error.empty()) {
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
    const int rc = w2b_eval_cosmul(e, (int64_t)b1s.size(), b1s.data(), b2s.data(), b3s.data(), k, best.data(), bestd.data());
    if (rc != W2B_OK) return rc;
  }
  return text_out(query_answers(e, lines, k, best, bestd), "w2b_eval_cosmul_text", out, out_len);
}

// the signed form: +WORD, -WORD or WORD, 1 to W2B_EVAL_MAX_TERMS of them per line
extern "C" int w2b_eval_combine_text(w2b_eval *e, const char *queries, int64_t len, int32_t k, char **out,
                                     int64_t *out_len) {
  if (!e || !out || len < 0 || (len > 0 && !queries)) return efail(W2B_EINVAL, "w2b_eval_combine_text: bad argument");
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, "w2b_eval_combine_text: k must be 1..64");
  if (e->codes) return efail(W2B_EINVAL, "w2b_eval_combine_text: not available in codes mode");
  *out = nullptr;
  std::vector<QueryLine> lines;
  std::vector<int32_t> rows;
  std::vector<int8_t> signs;
  std::vector<std::string> tok;
  for (int64_t pos = 0; next_query_line(queries, len, pos, tok);) {
    if (tok.empty()) continue;
    QueryLine ln{joined(tok), std::string(), -1};
    int32_t r[W2B_EVAL_MAX_TERMS] = {0};
    int8_t sg[W2B_EVAL_MAX_TERMS] = {0};
    if (tok.size() > W2B_EVAL_MAX_TERMS) ln.error = "expected 1 to 7 signed words";
    for (size_t i = 0; i < tok.size() && ln.error.empty(); i++) {
      const bool has_sign = tok[i][0] == '+' || tok[i][0] == '-';
      const std::string word = tok[i].substr(has_sign ? 1 : 0);
      const int64_t row = w2b_eval_lookup(e, word.c_str());
      if (row == e->words) ln.error = "not in vocabulary: " + word;
      r[i] = (int32_t)row;
      sg[i] = tok[i][0] == '-' ? -1 : 1;
    }
    if (ln.error.empty()) {
      ln.q = (int64_t)(rows.size() / W2B_EVAL_MAX_TERMS);
      rows.insert(rows.end(), r, r + W2B_EVAL_MAX_TERMS);
      signs.insert(signs.end(), sg, sg + W2B_EVAL_MAX_TERMS);
    }
    lines.push_back(ln);
  }
  const size_t nq = rows.size() / W2B_EVAL_MAX_TERMS;
  std::vector<int32_t> best(nq * (size_t)k);
  std::vector<float> bestd(nq * (size_t)k);
  if (nq > 0) {
    const int rc = w2b_eval_combine(e, (int64_t)nq, W2B_EVAL_MAX_TERMS, rows.data(), signs.data(), k, best.data(), bestd.data());
    if (rc != W2B_OK) return rc;
  }
  return text_out(query_answers(e, lines, k, best, bestd), "w2b_eval_combine_text", out, out_len);
}

// the bag form: every non-empty line is one bag of 1 to W2B_EVAL_MAX_BAG words
extern "C" int w2b_eval_bag_text(w2b_eval *e, const char *queries, int64_t len, int32_t exclude_own, int32_t k, char **out,
                                 int64_t *out_len) {
  if (!e || !out || len < 0 || (len > 0 && !queries)) return efail(W2B_EINVAL, "w2b_eval_bag_text: bad argument");
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, "w2b_eval_bag_text: k must be 1..64");
  if (exclude_own != 0 && exclude_own != 1) return efail(W2B_EINVAL, "w2b_eval_bag_text: exclude_own must be 0 or 1");
  if (!e->bits && !e->codes) return efail(W2B_EINVAL, "w2b_eval_bag_text: needs a bits or a codes handle");
  *out = nullptr;
  std::vector<QueryLine> lines;
  std::vector<int32_t> ids;
  std::vector<int64_t> offsets(1, 0);
  std::vector<std::string> tok;
  for (int64_t pos = 0; next_query_line(queries, len, pos, tok);) {
    if (tok.empty()) continue;
    QueryLine ln{joined(tok), std::string(), -1};
    if (tok.size() > W2B_EVAL_MAX_BAG) ln.error = "expected 1 to 4096 words";
    const size_t at = ids.size();
    for (size_t i = 0; i < tok.size() && ln.error.empty(); i++) {
      const int64_t row = w2b_eval_lookup(e, tok[i].c_str());
      if (row == e->words) ln.error = "not in vocabulary: " + tok[i];
      ids.push_back((int32_t)row);
    }
    if (ln.error.empty()) {
      ln.q = (int64_t)offsets.size() - 1;
      offsets.push_back((int64_t)ids.size());
    } else {
      ids.resize(at);
    }
    lines.push_back(ln);
  }
  const size_t nq = offsets.size() - 1;
  std::vector<int32_t> best(nq * (size_t)k);
  std::vector<float> bestd(nq * (size_t)k);
  if (nq > 0) {
    const int rc = w2b_eval_bag(e, (int64_t)ids.size(), ids.data(), (int64_t)nq, offsets.data(), exclude_own, k, best.data(),
                                bestd.data());
    if (rc != W2B_OK) return rc;
  }
  return text_out(query_answers(e, lines, k, best, bestd), "w2b_eval_bag_text", out, out_len);
}

// the vector form: every non-empty line is `size` numbers
extern "C" int w2b_eval_vectors_text(w2b_eval *e, const char *queries, int64_t len, int32_t normalize, int32_t k, char **out,
                                     int64_t *out_len) {
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, "w2b_eval_vectors_text: k must be 1..64");
  if (normalize != 0 && normalize != 1) return efail(W2B_EINVAL, "w2b_eval_vectors_text: normalize must be 0 or 1");
  if (!out || len < 0 || (len > 0 && !queries)) return efail(W2B_EINVAL, "w2b_eval_vectors_text: bad argument");
  if (!e) return efail(W2B_EINVAL, "w2b_eval_vectors_text: null handle");
  *out = nullptr;
  static const locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
  if (!c_locale) return efail(W2B_ENOMEM, "w2b_eval_vectors_text: no C locale");
  std::vector<QueryLine> lines;
  std::vector<float> x, row((size_t)e->size);
  std::vector<std::string> tok;
  for (int64_t pos = 0; next_query_line(queries, len, pos, tok);) {
    if (tok.empty()) continue;
    QueryLine ln{"vector " + std::to_string(lines.size() + 1), std::string(), -1};
    bool numbers = (int64_t)tok.size() == e->size;
    for (size_t i = 0; i < tok.size() && numbers; i++) {
      char *end = nullptr;
      row[i] = strtof_l(tok[i].c_str(), &end, c_locale);
      numbers = end == tok[i].c_str() + tok[i].size();
    }
    if (!numbers) {
      ln.error = "expected " + std::to_string(e->size) + " numbers";
    } else if (bad_vector_value(row.data(), e->size) >= 0) {
      ln.error = "value out of range";
    } else {
      ln.q = (int64_t)(x.size() / (size_t)e->size);
      x.insert(x.end(), row.begin(), row.end());
    }
    lines.push_back(ln);
  }
  const size_t nq = x.size() / (size_t)e->size;
  std::vector<int32_t> best(nq * (size_t)k);
  std::vector<float> bestd(nq * (size_t)k);
  if (nq > 0) {
    const int rc = w2b_eval_vectors(e, (int64_t)nq, x.data(), normalize, k, best.data(), bestd.data());
    if (rc != W2B_OK) return rc;
  }
  return text_out(query_answers(e, lines, k, best, bestd), "w2b_eval_vectors_text", out, out_len);
}

// the corpus from text: one document per line, empty lines included; words that are not in the vocabulary are dropped
extern "C" int w2b_eval_docs_set_text(w2b_eval *e, const char *text, int64_t len, int64_t *n_docs, int64_t *dropped) {
  const std::string who = "w2b_eval_docs_set_text";
  if (len < 0 || (len > 0 && !text)) return efail(W2B_EINVAL, who + ": bad argument");
  if (!e) return efail(W2B_EINVAL, who + ": null handle");
  if (!e->bits && !e->codes) return efail(W2B_EINVAL, who + ": " + kDocsFp32);
  std::vector<int32_t> ids;
  std::vector<int64_t> offsets(1, 0);
  std::vector<std::string> tok;
  int64_t lost = 0;
  for (int64_t pos = 0; next_query_line(text, len, pos, tok);) {
    for (const std::string &w : tok) {
      const int64_t row = w2b_eval_lookup(e, w.c_str());
      if (row == e->words) lost++;
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
  const std::string who = "w2b_eval_docs_text";
  if (k < 1 || k > W2B_EVAL_MAX_K) return efail(W2B_EINVAL, who + ": k must be 1..64");
  if (symmetric != 0 && symmetric != 1) return efail(W2B_EINVAL, who + ": symmetric must be 0 or 1");
  if (!out || len < 0 || (len > 0 && !queries)) return efail(W2B_EINVAL, who + ": bad argument");
  if (!e) return efail(W2B_EINVAL, who + ": null handle");
  if (!e->bits && !e->codes) return efail(W2B_EINVAL, who + ": " + kDocsFp32);
  if (e->docs_n == 0) return efail(W2B_EINVAL, who + ": no corpus is set (w2b_eval_docs_set)");
  *out = nullptr;
  std::vector<QueryLine> lines;
  std::vector<int32_t> ids;
  std::vector<int64_t> offsets(1, 0);
  std::vector<std::string> tok;
  for (int64_t pos = 0; next_query_line(queries, len, pos, tok);) {
    if (tok.empty()) continue;
    QueryLine ln{joined(tok), std::string(), -1};
    const size_t at = ids.size();
    for (const std::string &w : tok) {
      const int64_t row = w2b_eval_lookup(e, w.c_str());
      if (row != e->words) ids.push_back((int32_t)row);
    }
    if (ids.size() == at) ln.error = "no word in vocabulary";
    else if (ids.size() - at > W2B_EVAL_MAX_DOC) ln.error = "expected at most 1024 words";
    if (ln.error.empty()) {
      ln.q = (int64_t)offsets.size() - 1;
      offsets.push_back((int64_t)ids.size());
    } else {
      ids.resize(at);
    }
    lines.push_back(ln);
  }
  const size_t nq = offsets.size() - 1;
  std::vector<int32_t> best(nq * (size_t)k);
  std::vector<float> bestd(nq * (size_t)k);
  if (nq > 0) {
    const int rc = w2b_eval_docs(e, (int64_t)ids.size(), ids.data(), (int64_t)nq, offsets.data(), symmetric, k, best.data(),
                                 bestd.data(), nullptr);
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
      const int32_t d = best[(size_t)(ln.q * k + j)];
      if (d < 0) break;
      appendf(txt, "%d\t%lld\t%.6f\n", j + 1, (long long)d + 1, (double)bestd[(size_t)(ln.q * k + j)]);
    }
  }
  return text_out(txt, who.c_str(), out, out_len);
}

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
  if (!e->bits && !e->codes) return efail(W2B_EINVAL, who + ": not available on an fp32 handle: load the file with bits or codes");
  *out = nullptr;
  static const locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
  if (!c_locale) return efail(W2B_ENOMEM, who + ": no C locale");
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
          if (row == e->words) oov++;
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

extern "C" void w2b_eval_free_text(char *text) { free(text); }

// ------------------------------------------------------------------------------------ word classes
namespace {
constexpr int64_t kClassesMaxWords = 5592405;                       // 3 * words < 2^24: (float)T is exact

// what w2b_eval_classes and its host twin refuse: first what needs no table, then the table's shape, then `init`
const char *bad_classes_args(int32_t n_classes, int32_t max_iters) {
  if (n_classes < 1) return "n_classes must be at least 1";
  if (max_iters < 0 || max_iters > 1000) return "max_iters must be 0..1000";
  return nullptr;
}
const char *bad_classes_shape(int64_t words, int64_t size, int32_t n_classes) {
  if (n_classes > W2B_EVAL_MAX_CLASSES || n_classes > words) return "n_classes must be at most min(words, 16384)";
  if (words > kClassesMaxWords) return "words must be at most 5592405 (3 * words < 2^24)";
  if ((unsigned __int128)9 * (unsigned __int128)words * (unsigned __int128)words * (unsigned __int128)size >=
      ((unsigned __int128)1 << 63))
    return "9 * words^2 * size must stay below 2^63";
  return nullptr;
}
int64_t bad_classes_init(const int32_t *init, int64_t words, int32_t n_classes) {
  if (init)
    for (int64_t c = 0; c < words; c++)
      if (init[c] < 0 || init[c] >= n_classes) return c;
  return -1;
}
std::string classes_init_error(int64_t row) { return "init: row " + std::to_string(row) + ": class out of range"; }

// wq_k of the header from N_k > 0: the expression of bag_weight
inline float classes_weight(long long n) { return (float)(1.0 / sqrt((double)n)); }

// The chains of one row against every class: Tf = (float)T transposed, [size][K]; t = the row's codes; acc [K].  Explicit
// fmaf, strictly in column order per class.  The body is compiled twice, for a processor with FMA instructions (the
// classes vectorise) and for any other one (a library call per step): the same correctly rounded operation either way.
__attribute__((always_inline)) inline void classes_chains_body(const float *Tf, const int8_t *t, int64_t size, int32_t K,
                                                               float *acc) {
  for (int32_t k = 0; k < K; k++) acc[k] = 0.f;
  for (int64_t a = 0; a < size; a++) {
    const float ta = (float)t[a];
    const float *row = Tf + a * K;
    for (int32_t k = 0; k < K; k++) acc[k] = __builtin_fmaf(row[k], ta, acc[k]);
  }
}
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("avx2,fma"))) void classes_chains_fma(const float *Tf, const int8_t *t, int64_t size, int32_t K,
                                                            float *acc) {
  classes_chains_body(Tf, t, size, K, acc);
}
#endif
void classes_chains_plain(const float *Tf, const int8_t *t, int64_t size, int32_t K, float *acc) {
  classes_chains_body(Tf, t, size, K, acc);
}

// T [K][size] and counts [K] of the class array cl
void classes_sums_host(const int8_t *t, int64_t words, int64_t size, int32_t K, const int32_t *cl, int32_t *T, int64_t *counts) {
  std::fill(T, T + (size_t)K * (size_t)size, 0);
  std::fill(counts, counts + K, (int64_t)0);
  for (int64_t c = 0; c < words; c++) {
    int32_t *Tk = T + (int64_t)cl[c] * size;
    const int8_t *tc = t + c * size;
    for (int64_t a = 0; a < size; a++) Tk[a] += tc[a];
    counts[cl[c]]++;
  }
}
}  // namespace

// Host twin of the class kernels: the loop of the header, one step at a time (this file is built with -ffp-contract=off, and
// the function says so again).
extern "C" int w2b_classes_host(const uint64_t *packed, int64_t words, int64_t dim, int32_t bitlevel, int32_t n_classes,
                                int32_t max_iters, const int32_t *init, int32_t *cls, float *score, int32_t *T_out,
                                int64_t *counts, int32_t *iters_run, int64_t *moved) {
#pragma clang fp contract(off)
  const std::string who = "w2b_classes_host";
  if (const char *why = bad_classes_args(n_classes, max_iters)) return efail(W2B_EINVAL, who + ": " + why);
  if (!packed || !cls || words < 0 || dim < 1) return efail(W2B_EINVAL, who + ": bad argument");
  if (bitlevel != 1 && bitlevel != 2) return efail(W2B_EINVAL, who + ": bitlevel must be 1 or 2");
  if (const char *why = bad_classes_shape(words, dim, n_classes)) return efail(W2B_EINVAL, who + ": " + why);
  const int64_t bad = bad_classes_init(init, words, n_classes);
  if (bad >= 0) return efail(W2B_EINVAL, who + ": " + classes_init_error(bad));
  const int32_t K = n_classes;
  const int64_t wpr = (dim + 63) / 64 * bitlevel;
  std::vector<int8_t> t((size_t)(words * dim));
  for (int64_t c = 0; c < words; c++) {
    const uint64_t *rc = packed + c * wpr;
    for (int64_t a = 0; a < dim; a++) {
      const uint64_t bit = 1ull << (a & 63);
      int8_t v = 1;
      if (bitlevel == 2 && (rc[2 * (a >> 6) + 1] & bit)) v = 3;
      if (rc[bitlevel * (a >> 6)] & bit) v = (int8_t)-v;
      t[(size_t)(c * dim + a)] = v;
    }
  }
  std::vector<int32_t> cl((size_t)words), nw((size_t)words), T((size_t)K * (size_t)dim);
  std::vector<float> sc((size_t)words, 0.f), Tf((size_t)K * (size_t)dim), wq((size_t)K), acc((size_t)K);
  std::vector<int64_t> cnt((size_t)K);
  std::vector<char> live((size_t)K);
  for (int64_t c = 0; c < words; c++) cl[(size_t)c] = init ? init[c] : (int32_t)(c % K);
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
  const bool fma = __builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2");
#endif
  int32_t it = 0;
  int64_t mv = 0;
  while (it < max_iters) {
    classes_sums_host(t.data(), words, dim, K, cl.data(), T.data(), cnt.data());
    for (int32_t k = 0; k < K; k++) {
      long long n = 0;
      for (int64_t a = 0; a < dim; a++) {
        const long long v = T[(size_t)(k * dim + a)];
        n += v * v;
        Tf[(size_t)(a * K + k)] = (float)v;
      }
      live[(size_t)k] = n > 0;
      wq[(size_t)k] = n > 0 ? classes_weight(n) : 0.f;
    }
    mv = 0;
    for (int64_t c = 0; c < words; c++) {
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
      if (fma) classes_chains_fma(Tf.data(), t.data() + c * dim, dim, K, acc.data());
      else
#endif
        classes_chains_plain(Tf.data(), t.data() + c * dim, dim, K, acc.data());
      int32_t bk = -1;
      float bd = 0.f;
      for (int32_t k = 0; k < K; k++) {
        if (!live[(size_t)k]) continue;
        const float d = acc[(size_t)k] * wq[(size_t)k];
        if (bk < 0 || d > bd) bk = k, bd = d;
      }
      if (bk < 0) bk = 0, bd = 0.f;
      nw[(size_t)c] = bk;
      sc[(size_t)c] = bd;
      mv += bk != cl[(size_t)c];
    }
    cl.swap(nw);
    it++;
    if (mv == 0) break;
  }
  classes_sums_host(t.data(), words, dim, K, cl.data(), T.data(), cnt.data());
  std::copy(cl.begin(), cl.end(), cls);
  if (score) std::copy(sc.begin(), sc.end(), score);
  if (T_out) std::copy(T.begin(), T.end(), T_out);
  if (counts) std::copy(cnt.begin(), cnt.end(), counts);
  if (iters_run) *iters_run = it;
  if (moved) *moved = mv;
  return W2B_OK;
}

namespace {
// every device buffer of one w2b_eval_classes call, carved out of one allocation
struct ClassesBuffers {
  char *base = nullptr;
  int32_t *cl[2] = {nullptr, nullptr}, *hist = nullptr, *start = nullptr, *cursor = nullptr, *order = nullptr, *T = nullptr;
  float *score = nullptr, *wq = nullptr;
  uint32_t *live = nullptr;
  long long *counts = nullptr, *N = nullptr;
  unsigned long long *moved = nullptr;
  void *X = nullptr;
  ~ClassesBuffers() { if (base) (void)hipFree(base); }
  bool make(int64_t words, int64_t size, int32_t K) {
    const int64_t slots = w2b_cls_class_slots(K);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) / 256 * 256; return o; };
    const size_t o_cl0 = take((size_t)words * 4), o_cl1 = take((size_t)words * 4), o_score = take((size_t)words * 4);
    const size_t o_order = take((size_t)words * 4), o_hist = take((size_t)K * 4), o_start = take((size_t)(K + 1) * 4);
    const size_t o_cursor = take((size_t)K * 4), o_T = take((size_t)K * (size_t)size * 4), o_counts = take((size_t)K * 8);
    const size_t o_N = take((size_t)K * 8), o_wq = take((size_t)slots * 4), o_live = take((size_t)slots / 8);
    const size_t o_moved = take(8), o_X = take(w2b_cls_operand_bytes((int)size, K));
    if (hipMalloc(&base, at) != hipSuccess) { base = nullptr; return false; }
    cl[0] = (int32_t *)(base + o_cl0); cl[1] = (int32_t *)(base + o_cl1); score = (float *)(base + o_score);
    order = (int32_t *)(base + o_order); hist = (int32_t *)(base + o_hist); start = (int32_t *)(base + o_start);
    cursor = (int32_t *)(base + o_cursor); T = (int32_t *)(base + o_T); counts = (long long *)(base + o_counts);
    N = (long long *)(base + o_N); wq = (float *)(base + o_wq); live = (uint32_t *)(base + o_live);
    moved = (unsigned long long *)(base + o_moved); X = base + o_X;
    return true;
  }
};
}  // namespace

// Word classes: every check first, then the loop of the header with the class array, the sums and the centroid operands on
// the device throughout; per iteration the host sees the moved count and N_k (from which it builds wq_k and the live bits,
// as w2b_eval_bag builds wq).  Each iteration ends with the sums of its new class array: what the next one scores against,
// and after the last one the T_out and counts of the result.
extern "C" int w2b_eval_classes(w2b_eval *e, int32_t n_classes, int32_t max_iters, const int32_t *init, int32_t *cls,
                                float *score, int32_t *T_out, int64_t *counts, int32_t *iters_run, int64_t *moved) {
  const std::string who = "w2b_eval_classes";
  if (const char *why = bad_classes_args(n_classes, max_iters)) return efail(W2B_EINVAL, who + ": " + why);
  if (!e) return efail(W2B_EINVAL, who + ": null handle");
  if (!e->bits && !e->codes)
    return efail(W2B_EINVAL, who + ": not available on an fp32 handle: load the file with bits or codes");
  if (!cls) return efail(W2B_EINVAL, who + ": bad argument");
  if (const char *why = bad_classes_shape(e->words, e->size, n_classes)) return efail(W2B_EINVAL, who + ": " + why);
  const int64_t bad = bad_classes_init(init, e->words, n_classes);
  if (bad >= 0) return efail(W2B_EINVAL, who + ": " + classes_init_error(bad));
  EHIP(hipSetDevice(e->device));
  const int32_t K = n_classes;
  const int words = (int)e->words, size = (int)e->size, bl = e->codes ? 2 : 1;
  const int64_t slots = w2b_cls_class_slots(K);
  ClassesBuffers d;
  if (!d.make(words, size, K)) return efail(W2B_ENOMEM, who + ": device allocation failed");
  std::vector<int32_t> h_cl((size_t)words);
  for (int64_t c = 0; c < words; c++) h_cl[(size_t)c] = init ? init[c] : (int32_t)(c % K);
  EHIP(hipMemcpy(d.cl[0], h_cl.data(), (size_t)words * 4, hipMemcpyHostToDevice));
  EHIP(hipMemsetAsync(d.score, 0, (size_t)words * 4, e->stream));
  EventPair ev, ev2;
  EHIP(ev.create());
  EHIP(ev2.create());
  std::vector<long long> h_N((size_t)K);
  std::vector<float> h_wq((size_t)slots);
  std::vector<uint32_t> h_live((size_t)slots / 32);
  // the host's share of an iteration: wq and the live bits from N, for the next assign
  auto weights_up = [&]() -> int {
    std::fill(h_wq.begin(), h_wq.end(), 0.f);
    std::fill(h_live.begin(), h_live.end(), 0u);
    for (int32_t k = 0; k < K; k++)
      if (h_N[(size_t)k] > 0) {
        h_wq[(size_t)k] = classes_weight(h_N[(size_t)k]);
        h_live[(size_t)k >> 5] |= 1u << (k & 31);
      }
    EHIP(hipMemcpy(d.wq, h_wq.data(), (size_t)slots * 4, hipMemcpyHostToDevice));
    EHIP(hipMemcpy(d.live, h_live.data(), (size_t)slots / 8, hipMemcpyHostToDevice));
    return W2B_OK;
  };
  auto sums = [&](const int32_t *cl) {
    return w2b_launch_cls_sums(e->B, words, size, bl, K, cl, d.hist, d.start, d.cursor, d.order, d.T, d.counts, d.N, d.X,
                               e->stream);
  };
  float ms = 0;
  e->cls_assign_ms = e->cls_sums_ms = 0;
  EHIP(hipEventRecord(ev.t[0], e->stream));
  EHIP(sums(d.cl[0]));
  EHIP(hipEventRecord(ev.t[1], e->stream));
  EHIP(hipMemcpyAsync(h_N.data(), d.N, (size_t)K * 8, hipMemcpyDeviceToHost, e->stream));
  EHIP(hipStreamSynchronize(e->stream));
  EHIP(hipEventElapsedTime(&ms, ev.t[0], ev.t[1]));
  e->cls_sums_ms += ms;
  int cur = 0;
  int32_t it = 0;
  unsigned long long mv = 0;
  while (it < max_iters) {
    if (int rc = weights_up()) return rc;
    EHIP(hipMemsetAsync(d.moved, 0, 8, e->stream));
    EHIP(hipEventRecord(ev.t[0], e->stream));
    EHIP(w2b_launch_cls_assign(e->B, words, size, bl, K, d.X, d.wq, d.live, d.cl[cur], d.cl[cur ^ 1], d.score, d.moved,
                               e->stream));
    EHIP(hipEventRecord(ev.t[1], e->stream));
    EHIP(hipEventRecord(ev2.t[0], e->stream));
    EHIP(sums(d.cl[cur ^ 1]));
    EHIP(hipEventRecord(ev2.t[1], e->stream));
    EHIP(hipMemcpyAsync(&mv, d.moved, 8, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipMemcpyAsync(h_N.data(), d.N, (size_t)K * 8, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    EHIP(hipEventElapsedTime(&ms, ev.t[0], ev.t[1]));
    e->cls_assign_ms += ms;
    EHIP(hipEventElapsedTime(&ms, ev2.t[0], ev2.t[1]));
    e->cls_sums_ms += ms;
    e->launches++;
    e->macs += (double)K * (double)words * (double)size;
    cur ^= 1;
    it++;
    if (mv == 0) break;
  }
  e->kernel_ms += e->cls_assign_ms + e->cls_sums_ms;
  std::vector<float> h_score(score ? (size_t)words : 0);
  std::vector<int32_t> h_T(T_out ? (size_t)K * (size_t)size : 0);
  std::vector<long long> h_counts(counts ? (size_t)K : 0);
  EHIP(hipMemcpy(h_cl.data(), d.cl[cur], (size_t)words * 4, hipMemcpyDeviceToHost));
  if (score) EHIP(hipMemcpy(h_score.data(), d.score, (size_t)words * 4, hipMemcpyDeviceToHost));
  if (T_out) EHIP(hipMemcpy(h_T.data(), d.T, h_T.size() * 4, hipMemcpyDeviceToHost));
  if (counts) EHIP(hipMemcpy(h_counts.data(), d.counts, (size_t)K * 8, hipMemcpyDeviceToHost));
  std::copy(h_cl.begin(), h_cl.end(), cls);
  if (score) std::copy(h_score.begin(), h_score.end(), score);
  if (T_out) std::copy(h_T.begin(), h_T.end(), T_out);
  if (counts) std::copy(h_counts.begin(), h_counts.end(), counts);
  if (iters_run) *iters_run = it;
  if (moved) *moved = (int64_t)mv;
  return W2B_OK;
}

extern "C" int w2b_eval_classes_timing(w2b_eval *e, double *assign_ms, double *sums_ms) {
  if (!e) return efail(W2B_EINVAL, "w2b_eval_classes_timing: null handle");
  if (assign_ms) *assign_ms = e->cls_assign_ms;
  if (sums_ms) *sums_ms = e->cls_sums_ms;
  return W2B_OK;
}

// word2vec's -classes file: one line "<word> <class>" per row, in row order
extern "C" int w2b_eval_classes_text(w2b_eval *e, int32_t n_classes, int32_t max_iters, char **out, int64_t *out_len) {
  const std::string who = "w2b_eval_classes_text";
  if (const char *why = bad_classes_args(n_classes, max_iters)) return efail(W2B_EINVAL, who + ": " + why);
  if (!e) return efail(W2B_EINVAL, who + ": null handle");
  if (!out) return efail(W2B_EINVAL, who + ": bad argument");
  std::vector<int32_t> cls((size_t)(e->words > 0 ? e->words : 1));
  if (int rc = w2b_eval_classes(e, n_classes, max_iters, nullptr, cls.data(), nullptr, nullptr, nullptr, nullptr, nullptr))
    return rc;
  std::string txt;
  for (int64_t c = 0; c < e->words; c++) {
    txt += e->vocab.data() + c * kMaxW;
    txt += ' ';
    txt += std::to_string(cls[(size_t)c]);
    txt += '\n';
  }
  return text_out(txt, who.c_str(), out, out_len);
}
