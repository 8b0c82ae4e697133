// w2b_eval.cpp -- the device side of include/word2bits_eval.h: the one host unit of the evaluator that sees `struct
// w2b_eval` and makes HIP calls.
//   the handle      struct w2b_eval and eval_release; the accessors (w2b_eval_words, _size, _word, _lookup, _is_bits,
//                   _is_codes, _docs_count) that the text forms read it through
//   the loaders     the vector-file reader of the reference evaluator (ref src/compute-accuracy.c:80-112), bit-packed
//                   files, the views of a live trainer; w2b_eval_get_matrix / _bits / _codes
//   the scan        every list question goes through eval_scan_chunks: an input struct (Rows3, Terms, Bags, Vectors) puts
//                   a chunk of questions on the device, a Scan* struct sizes the chunk and launches one form of the scan
//                   (fp32 rows: w2b_kernels_eval.hip; 1-bit rows: _evalbits; 2-bit rows: _evalcodes; and _evalcombine,
//                   _evalbag, _evalvec, _evalcosmul for the questions of those names)
//   the drivers     documents (_evaldocs), pairs (_evalpairs), word classes (_evalclasses) and the rank of a given row (the
//                   count epilogues of _evalbits and _evalcodes), which chunk by themselves
//   the setters     the scratch bound, the kernel variant, the timing read-outs
// No arithmetic on scores happens here.  What the host does compute are question weights and tables, by the expressions
// of w2b_eval_shared.h that the host twins use too: the bag question's and the classes' 1 / sqrt(N), the vector question's
// wx (and the fp32 handle's vec = x * wx), the 3CosMul table u = A / size of a bits handle, w(r) by n3 of a codes handle,
// and the pair question's cosine from the three integers the device sums.  There is no CPU fallback: the host twins of the
// kernels (w2b_eval_twins.cpp) are the tests' yardstick, and the text forms (w2b_eval_text.cpp) call the entry points of
// this file like any other user of the header.
#include "w2b_eval_shared.h"
#include "w2b_internal.h"
#include "w2b_evalclasses.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <unordered_map>

namespace {
constexpr int64_t kMaxW = 50;            // ref :24 max_w
constexpr int64_t kTile = 256;           // padding unit of rows / questions (covers both kernels' tiles)
constexpr int64_t kChunkQ = 1 << 16;     // questions per launch
constexpr int64_t kTopkScratch = 1ll << 30;   // default bound of the top-k slot scratch of one launch

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
  // w2b_eval_rank: per question of a chunk the two counters, their correction, the target's score and row (kRankBytes each)
  void *rank_buf = nullptr;
  int64_t rank_cap = 0;
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
  if (e->rank_buf) (void)hipFree(e->rank_buf);
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
constexpr int64_t kDocsMaxAll = 1ll << 28;       // nq * n_docs of an all_scores request
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

// ------------------------------------------------------------------------------------ rank of a given row
// The place of a given row in the complete answer list (include/word2bits_eval.h, "rank of a given row"): the products of
// the three-row scans with a count for an epilogue, so no selection state -- per question one 64-bit counter pair that the
// scan adds to, what the question's own rows and the target itself added to it (the scan excludes nothing), and the
// target's score.  A chunk is sized so that its planes or operands and its counters stay within the scratch bound, never
// below 128 questions.  The results of all chunks are collected first: an error in a later chunk leaves the outputs untouched.
namespace {
constexpr int64_t kRankBytes = 32;   // device bytes per question: counters 8, correction 8, score 4, row 4, (bits) target acc and row 8
}

static int eval_rank(w2b_eval *e, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3, const int32_t *target,
                     int32_t *rank, int32_t *tied, float *score, const std::string &who) {
  if (nq < 0 || (nq > 0 && (!b1 || !b2 || !b3 || !target || !rank))) return efail(W2B_EINVAL, who + ": bad argument");
  if (nq == 0) return W2B_OK;
  if (!e) return efail(W2B_EINVAL, who + ": null handle");
  if (!e->bits && !e->codes)
    return efail(W2B_EINVAL, who + ": not available on an fp32 handle: load the file with bits or codes");
  for (int64_t q = 0; q < nq; q++)
    if (b1[q] < 0 || b1[q] >= e->words || b2[q] < 0 || b2[q] >= e->words || b3[q] < 0 || b3[q] >= e->words || target[q] < 0 ||
        target[q] >= e->words)
      return efail(W2B_EINVAL, who + ": question " + std::to_string(q) + ": row out of range");
  EHIP(hipSetDevice(e->device));
  const int64_t per_q = (e->bits ? e->wpr * 16 : (e->size + 31) / 32 * 96) + 8;     // planes / operands, and the counters
  int64_t chunk = (e->tk_budget > 0 ? e->tk_budget : kTopkScratch) / per_q / 128 * 128;
  if (chunk < 128) chunk = 128;
  if (chunk > kChunkQ) chunk = kChunkQ;
  std::vector<int32_t> r_rank((size_t)nq), r_tied((size_t)nq);
  std::vector<float> r_score((size_t)nq);
  std::vector<uint32_t> cnt, corr, ts;
  const uint32_t *B32 = (const uint32_t *)e->B;
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int64_t n = (nq - q0 < chunk) ? nq - q0 : chunk;
    const int64_t np = (n + kTile - 1) / kTile * kTile;
    if (eval_reserve_questions(e, np) != W2B_OK) return efail(W2B_ENOMEM, who + ": device allocation failed");
    if (np > e->rank_cap) {
      if (e->rank_buf) (void)hipFree(e->rank_buf);
      e->rank_buf = nullptr;
      e->rank_cap = 0;
      if (hipMalloc(&e->rank_buf, (size_t)(np * kRankBytes)) != hipSuccess) return efail(W2B_ENOMEM, who + ": device allocation failed");
      e->rank_cap = np;
    }
    unsigned long long *d_cnt = (unsigned long long *)e->rank_buf;
    uint32_t *d_corr = (uint32_t *)(d_cnt + np), *d_ts = d_corr + 2 * np, *d_tacc = d_ts + 2 * np;
    int32_t *d_tgt = (int32_t *)(d_ts + np);
    Rows3 in{b1, b2, b3};
    if (int rc = in.upload(e, q0, n, np)) return rc;
    EHIP(hipMemsetAsync(e->rank_buf, 0, (size_t)(np * kRankBytes), e->stream));
    EHIP(hipMemcpyAsync(d_tgt, target + q0, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    EventPair ev;
    EHIP(ev.create());
    EHIP(hipEventRecord(ev.t[0], e->stream));
    hipError_t le;
    if (e->bits) {
      le = w2b_launch_bits_planes(B32, (int)(2 * e->wpr), (int)e->size, (int)n, np, in.d1, in.d2, in.d3, e->P, e->stream);
      if (le == hipSuccess)
        le = w2b_launch_bits_rank(B32, (int)e->words, (int)e->size, e->P, np, (int)n, in.d1, in.d2, in.d3, d_tgt, d_cnt, d_corr,
                                  (int *)d_ts, d_tacc, e->stream);
    } else {
      le = w2b_launch_codes_operands(B32, (int)e->size, (int)n, e->wrow, in.d1, in.d2, in.d3, e->P, e->Q, e->stream);
      if (le == hipSuccess)
        le = w2b_launch_codes_rank(B32, (int)e->words, (int)e->size, e->wrow, e->P, e->Q, (int)n, in.d1, in.d2, in.d3, d_tgt,
                                   (float *)d_ts, d_corr, d_cnt, e->stream);
    }
    if (le == hipSuccess) le = hipEventRecord(ev.t[1], e->stream);
    cnt.assign((size_t)(2 * n), 0u);
    corr.assign((size_t)(2 * n), 0u);
    ts.assign((size_t)n, 0u);
    if (le == hipSuccess) le = hipMemcpyAsync(cnt.data(), d_cnt, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream);
    if (le == hipSuccess) le = hipMemcpyAsync(corr.data(), d_corr, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream);
    if (le == hipSuccess) le = hipMemcpyAsync(ts.data(), d_ts, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream);
    if (le == hipSuccess) le = hipStreamSynchronize(e->stream);
    float ms = 0;
    if (le == hipSuccess) le = hipEventElapsedTime(&ms, ev.t[0], ev.t[1]);
    if (le != hipSuccess) return efail(W2B_EHIP, who + ": " + hipGetErrorString(le));
    e->kernel_ms += ms;
    e->launches++;
    e->macs += (e->codes ? 3.0 : 1.0) * (double)n * (double)e->words * (double)e->size;
    for (int64_t i = 0; i < n; i++) {
      const uint32_t t = ts[(size_t)i];
      const bool ranked = t != 0u;          // both score forms are > 0 for a ranked target
      r_rank[(size_t)(q0 + i)] = ranked ? (int32_t)(1u + cnt[(size_t)(2 * i)] - corr[(size_t)(2 * i)]) : 0;
      r_tied[(size_t)(q0 + i)] = ranked ? (int32_t)(cnt[(size_t)(2 * i + 1)] - corr[(size_t)(2 * i + 1)]) : 0;
      r_score[(size_t)(q0 + i)] = !ranked ? 0.f : e->bits ? (float)(int32_t)t / (float)e->size : f32_score((unsigned long long)t << 32);
    }
  }
  memcpy(rank, r_rank.data(), (size_t)nq * 4);
  if (tied) memcpy(tied, r_tied.data(), (size_t)nq * 4);
  if (score) memcpy(score, r_score.data(), (size_t)nq * 4);
  return W2B_OK;
}

extern "C" int w2b_eval_rank(w2b_eval *e, int64_t nq, const int32_t *b1, const int32_t *b2, const int32_t *b3,
                             const int32_t *target, int32_t *rank, int32_t *tied, float *score) {
  return eval_rank(e, nq, b1, b2, b3, target, rank, tied, score, "w2b_eval_rank");
}

extern "C" int w2b_eval_neighbor_rank(w2b_eval *e, int64_t nq, const int32_t *rows, const int32_t *target, int32_t *rank,
                                      int32_t *tied, float *score) {
  return eval_rank(e, nq, rows, rows, rows, target, rank, tied, score, "w2b_eval_neighbor_rank");
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

// ------------------------------------------------------------------------------------ word classes
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
