// w2b_embed.cpp -- host side of include/word2bits_embed.h: the handle, the .w2bp loader, validation, the device staging
// (one set of buffers handed to the caller by w2b_embed_reserve, a separate bounded one for the host form), the chunking
// of host-form calls (weighted bags stage their weights beside the ids), timing, and the host twins of the kernels in w2b_kernels_embed.hip.
// The projection (w2b_kernels_embedproj.hip) has staging of its own in both forms; its twin is in the host-only w2b_embed_twins.cpp and
// what both must refuse in w2b_embed_shared.h; the same holds for the back-projection (w2b_kernels_embedback.hip), whose scratch for
// the segments' partial sums follows the call.  The table stays packed on the
// device; no float table exists on either side and there is no CPU fallback (the *_host twins are for tests).
#include "../../include/word2bits_embed.h"
#include "../../include/word2bits_corpus.h"
#include "../../include/word2bits_hip.h"
#include "w2b_internal.h"
#include "w2b_embed_shared.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

namespace {
constexpr int64_t kHostOutBytes = 64ll << 20;     // output staging of one host-form chunk
constexpr int64_t kHostIds = 1ll << 22;           // ids of one host-form chunk (a single bag may be this long)
constexpr size_t kMaxPending = 256;               // event pairs kept before they are folded into the sums

int efail(int code, const std::string &msg) { return w2b_internal_fail(code, msg.c_str()); }
#define EHIP(x)                                                                                   \
  do {                                                                                            \
    hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess) return efail(W2B_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

int elem_size(int32_t dtype) { return dtype == W2B_EMBED_F32 ? 4 : (dtype == W2B_EMBED_BF16 || dtype == W2B_EMBED_F16) ? 2 : 0; }

// device staging of one form
struct Staging {
  long long *ids = nullptr, *offsets = nullptr;
  void *out = nullptr, *scratch = nullptr;
  int64_t cap_ids = 0, cap_bags = -1, out_bytes = 0, scratch_bytes = 0;
  float *weights = nullptr;                  // weighted bags only: a buffer and a scratch of their own
  void *wscratch = nullptr;
  int64_t cap_weights = 0, wscratch_bytes = 0;
};
// device staging of one form of the projection: buffers of their own, each of which only moves when it grows itself
struct ProjStaging {
  float *x = nullptr;                        // [cap_n][dim]
  long long *cand = nullptr;                 // [cap_m]
  void *out = nullptr, *operands = nullptr;  // [n][m] of a dtype; the vectors in fragment order (for cap_n vectors)
  int64_t cap_n = 0, cap_m = 0, out_bytes = 0, operand_bytes = 0;
};
// device staging of one form of the back-projection: buffers of their own again; the scratch follows the call
struct BackStaging {
  float *g = nullptr;                        // [cap_n][cap_m] reserved; a call's g is dense [n][m]
  long long *cand = nullptr;                 // [cap_m]
  float *dx = nullptr;                       // [cap_n][dim]
  void *scratch = nullptr;                   // the segments' partial sums, when the driver sends them through the scratch
  int64_t g_elems = 0, cap_m = 0, cap_n = 0, scratch_bytes = 0;
};
// device staging of one form of the cross-entropy: buffers of their own once more.  What a caller fills or reads (x, cand,
// target, stats, dx) moves only when that buffer itself grows; the rest follows the call.
struct XentStaging {
  float *x = nullptr;                        // [cap_n][dim]
  long long *cand = nullptr, *clean = nullptr;   // [cap_m]: the caller's candidates; ids >= rows made padding
  long long *target = nullptr, *teff = nullptr;  // [cap_n]: the caller's targets; the effective ones (-1 = ignored)
  float *stats = nullptr;                    // [3][n] for the n of a call: mx, se, tl
  float *dx = nullptr;                       // [cap_n][dim]
  void *operands = nullptr;                  // the vectors in fragment order (for cap_n vectors)
  float *mseg = nullptr;                     // [nseg][vectors of a statistics launch]
  unsigned long long *useg = nullptr;
  float *g = nullptr;                        // the gradient's dense scratch, at most kXentScratch bytes
  void *bscratch = nullptr;                  // the back-projection's own scratch
  int64_t cap_n = 0, cap_m = 0, operand_bytes = 0, seg_slots = 0, g_bytes = 0, bscratch_bytes = 0;
};
struct Pending { hipEvent_t a, b; };
constexpr int64_t kXentScratch = 64ll << 20;      // bytes of g per gradient launch, and of segment statistics per statistics launch
}  // namespace

struct w2b_embed {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t rows = 0, dim = 0, wpr = 0;
  int bitlevel = 0;
  bool has_words = false;
  std::vector<std::string> names;
  std::unordered_map<std::string, int64_t> first;
  uint64_t *T = nullptr;                     // [rows][wpr], the file's layout
  unsigned long long *bad = nullptr;         // device counter
  Staging user, host;
  ProjStaging puser, phost;
  BackStaging buser, bhost;
  XentStaging xuser, xhost;
  std::vector<Pending> pending;
  double kernel_ms = 0, bytes = 0;
  int64_t launches = 0;
};

namespace {
void free_staging(Staging &s) {
  if (s.ids) (void)hipFree(s.ids);
  if (s.offsets) (void)hipFree(s.offsets);
  if (s.out) (void)hipFree(s.out);
  if (s.scratch) (void)hipFree(s.scratch);
  if (s.weights) (void)hipFree(s.weights);
  if (s.wscratch) (void)hipFree(s.wscratch);
  s = Staging();
}

void free_project(ProjStaging &s) {
  if (s.x) (void)hipFree(s.x);
  if (s.cand) (void)hipFree(s.cand);
  if (s.out) (void)hipFree(s.out);
  if (s.operands) (void)hipFree(s.operands);
  s = ProjStaging();
}

void free_back(BackStaging &s) {
  if (s.g) (void)hipFree(s.g);
  if (s.cand) (void)hipFree(s.cand);
  if (s.dx) (void)hipFree(s.dx);
  if (s.scratch) (void)hipFree(s.scratch);
  s = BackStaging();
}

void free_xent(XentStaging &s) {
  void *all[] = {s.x, s.cand, s.clean, s.target, s.teff, s.stats, s.dx, s.operands, s.mseg, s.useg, s.g, s.bscratch};
  for (void *p : all)
    if (p) (void)hipFree(p);
  s = XentStaging();
}

void embed_release(w2b_embed *e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  for (Pending &p : e->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  free_staging(e->user);
  free_staging(e->host);
  free_project(e->puser);
  free_project(e->phost);
  free_back(e->buser);
  free_back(e->bhost);
  free_xent(e->xuser);
  free_xent(e->xhost);
  if (e->T) (void)hipFree(e->T);
  if (e->bad) (void)hipFree(e->bad);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}
struct EmbedRelease { void operator()(w2b_embed *e) const { embed_release(e); } };
using EmbedPtr = std::unique_ptr<w2b_embed, EmbedRelease>;

// ------------------------------------------------------------------------------------ validation (host form and twins)
int check_shape(int64_t rows, int64_t dim, int32_t bitlevel, int64_t min_rows, const char *who) {
  if (rows < min_rows || rows > 0x7FFFFF00ll || dim < 1 || dim > (1 << 24))
    return efail(W2B_EINVAL, std::string(who) + ": unsupported rows / dim");
  if (w2b_packed_words_per_row(dim, bitlevel) < 0)
    return efail(W2B_EUNSUPPORTED, std::string(who) + ": bitlevel must be 1 or 2");
  return W2B_OK;
}

int check_ids(int64_t rows, int64_t n, const int32_t *ids, const char *who) {
  if (n < 0) return efail(W2B_EINVAL, std::string(who) + ": negative id count");
  if (n > 0 && !ids) return efail(W2B_EINVAL, std::string(who) + ": null ids");
  for (int64_t i = 0; i < n; i++)
    if (ids[i] >= rows) {
      char msg[160];
      snprintf(msg, sizeof msg, "%s: ids[%lld] = %d is not below rows = %lld", who, (long long)i, (int)ids[i], (long long)rows);
      return efail(W2B_EINVAL, msg);
    }
  return W2B_OK;
}

int check_bags(int64_t n_ids, int64_t n_bags, const int64_t *offsets, int32_t mode, const char *who) {
  const std::string w(who);
  if (n_bags < 0 || n_bags > 0x7FFFFF00ll) return efail(W2B_EINVAL, w + ": bad bag count");
  if (mode != W2B_EMBED_SUM && mode != W2B_EMBED_MEAN) return efail(W2B_EINVAL, w + ": mode is neither W2B_EMBED_SUM nor W2B_EMBED_MEAN");
  if (!offsets) return n_bags == 0 && n_ids == 0 ? W2B_OK : efail(W2B_EINVAL, w + ": null offsets");
  if (offsets[0] != 0) return efail(W2B_EINVAL, w + ": offsets[0] is not 0");
  for (int64_t b = 0; b < n_bags; b++) {
    if (offsets[b + 1] < offsets[b]) return efail(W2B_EINVAL, w + ": offsets decrease at bag " + std::to_string(b));
    if (offsets[b + 1] - offsets[b] > W2B_EMBED_MAX_BAG)
      return efail(W2B_EINVAL, w + ": bag " + std::to_string(b) + " is longer than W2B_EMBED_MAX_BAG");
  }
  if (offsets[n_bags] != n_ids) return efail(W2B_EINVAL, w + ": offsets[n_bags] is not n_ids");
  return W2B_OK;
}

// the first weight on an id >= 0 that is not finite, or neither 0 nor within 2^-60 .. 2^60
int check_weights(int64_t n, const int32_t *ids, const float *weights, const char *who) {
  if (n > 0 && !weights) return efail(W2B_EINVAL, std::string(who) + ": null weights");
  for (int64_t i = 0; i < n; i++) {
    uint32_t bits;
    memcpy(&bits, weights + i, 4);
    const uint32_t a = bits & 0x7FFFFFFFu;
    if (ids[i] >= 0 && a != 0u && (a < 0x21800000u || a > 0x5D800000u)) {
      char msg[200];
      snprintf(msg, sizeof msg, "%s: weights[%lld] = %g is not finite, or neither 0 nor within 2^-60 .. 2^60", who, (long long)i,
               (double)weights[i]);
      return efail(W2B_EINVAL, msg);
    }
  }
  return W2B_OK;
}

// ------------------------------------------------------------------------------------ device side of the handle
int device_visible(int32_t device, const char *who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return efail(W2B_ENOGPU, std::string(who) + ": no HIP device visible (the embedding has no CPU fallback)");
  if (device < 0 || device >= ndev) return efail(W2B_EINVAL, std::string(who) + ": bad device index");
  return W2B_OK;
}

// `bits` = [rows][wpr] packed words in host memory, possibly unaligned (inside a file image)
int embed_finish(EmbedPtr e, const unsigned char *bits, w2b_embed **out) {
  EHIP(hipSetDevice(e->device));
  EHIP(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  const size_t bytes = (size_t)e->rows * (size_t)e->wpr * 8;
  if (hipMalloc(&e->T, bytes) != hipSuccess || hipMalloc(&e->bad, 8) != hipSuccess)
    return efail(W2B_ENOMEM, "w2b_embed: device allocation failed");
  EHIP(hipMemcpy(e->T, bits, bytes, hipMemcpyHostToDevice));
  EHIP(hipMemset(e->bad, 0, 8));
  *out = e.release();
  return W2B_OK;
}

template <class P>
int grow(w2b_embed *e, P *&p, int64_t &have, int64_t want_bytes, int64_t new_have) {
  EHIP(hipStreamSynchronize(e->stream));          // nothing in flight may still use the old buffer
  if (p) (void)hipFree(p);
  p = nullptr;
  have = 0;
  void *q = nullptr;
  if (hipMalloc(&q, (size_t)(want_bytes > 0 ? want_bytes : 8)) != hipSuccess)
    return efail(W2B_ENOMEM, "w2b_embed: device allocation failed");
  p = (P *)q;
  have = new_have;
  return W2B_OK;
}

// buffers for max_ids ids, max_bags bags (< 0: none) and out_bytes of output; only ever grows
int ensure(w2b_embed *e, Staging &s, int64_t max_ids, int64_t max_bags, int64_t out_bytes) {
  if (max_ids > s.cap_ids || !s.ids)
    if (int rc = grow(e, s.ids, s.cap_ids, max_ids * 8, max_ids)) return rc;
  if (max_bags > s.cap_bags || (max_bags >= 0 && !s.offsets))
    if (int rc = grow(e, s.offsets, s.cap_bags, (max_bags + 1) * 8, max_bags)) return rc;
  out_bytes = (out_bytes + 15) / 16 * 16;
  if (out_bytes > s.out_bytes || !s.out)
    if (int rc = grow(e, s.out, s.out_bytes, out_bytes, out_bytes)) return rc;
  if (s.cap_bags > 0) {
    int cap = 0;
    const int64_t need = w2b_embed_bag_scratch(s.cap_ids, s.cap_bags, (int)e->dim, &cap);
    if (need > s.scratch_bytes)
      if (int rc = grow(e, s.scratch, s.scratch_bytes, need, need)) return rc;
  }
  return W2B_OK;
}

// the weights buffer for max_ids ids, and the scratch of a weighted launch of n_ids ids in n_bags bags; only ever grow
int ensure_weighted(w2b_embed *e, Staging &s, int64_t max_ids, int64_t n_ids, int64_t n_bags) {
  if (max_ids > s.cap_weights || !s.weights)
    if (int rc = grow(e, s.weights, s.cap_weights, max_ids * 4, max_ids)) return rc;
  if (n_bags > 0) {
    int cap = 0;
    long long segcap = 0, head = 0;
    const int64_t need = w2b_embed_bagw_scratch(n_ids, n_bags, (int)e->dim, &cap, &segcap, &head);
    if (need > s.wscratch_bytes)
      if (int rc = grow(e, s.wscratch, s.wscratch_bytes, need, need)) return rc;
  }
  return W2B_OK;
}

// the projection's buffers for max_n vectors, max_m candidates and out_bytes of output; only ever grow, each on its own
int ensure_project(w2b_embed *e, ProjStaging &s, int64_t max_n, int64_t max_m, int64_t out_bytes) {
  if (max_n > s.cap_n || !s.x)
    if (int rc = grow(e, s.x, s.cap_n, max_n * e->dim * 4, max_n)) return rc;
  const int64_t need = (int64_t)w2b_embed_project_operand_bytes((int)e->dim, s.cap_n);
  if (need > s.operand_bytes || !s.operands)
    if (int rc = grow(e, s.operands, s.operand_bytes, need, need)) return rc;
  if (max_m > s.cap_m || !s.cand)
    if (int rc = grow(e, s.cand, s.cap_m, max_m * 8, max_m)) return rc;
  out_bytes = (out_bytes + 15) / 16 * 16;
  if (out_bytes > s.out_bytes || !s.out)
    if (int rc = grow(e, s.out, s.out_bytes, out_bytes, out_bytes)) return rc;
  return W2B_OK;
}

// the back-projection's buffers for max_n vectors and max_m candidates (g holds max_n * max_m values); only ever grow, each
// on its own
int ensure_back(w2b_embed *e, BackStaging &s, int64_t max_n, int64_t max_m) {
  if (max_n * max_m > s.g_elems || !s.g)
    if (int rc = grow(e, s.g, s.g_elems, max_n * max_m * 4, max_n * max_m)) return rc;
  if (max_m > s.cap_m || !s.cand)
    if (int rc = grow(e, s.cand, s.cap_m, max_m * 8, max_m)) return rc;
  if (max_n > s.cap_n || !s.dx)
    if (int rc = grow(e, s.dx, s.cap_n, max_n * e->dim * 4, max_n)) return rc;
  return W2B_OK;
}

int fold_pending(w2b_embed *e) {
  EHIP(hipStreamSynchronize(e->stream));
  for (Pending &p : e->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) e->kernel_ms += ms;
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  e->pending.clear();
  return W2B_OK;
}

// one timed launch on the handle's stream
template <class Launch>
int timed(w2b_embed *e, double bytes, Launch &&launch) {
  if (e->pending.size() >= kMaxPending)
    if (int rc = fold_pending(e)) return rc;
  Pending p{nullptr, nullptr};
  if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) {
    if (p.a) (void)hipEventDestroy(p.a);
    return efail(W2B_EHIP, "w2b_embed: hipEventCreate failed");
  }
  hipError_t he = hipEventRecord(p.a, e->stream);
  if (he == hipSuccess) he = launch();
  if (he == hipSuccess) he = hipEventRecord(p.b, e->stream);
  if (he != hipSuccess) {
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
    return efail(W2B_EHIP, std::string("w2b_embed launch: ") + hipGetErrorString(he));
  }
  e->pending.push_back(p);
  e->launches++;
  e->bytes += bytes;
  return W2B_OK;
}

int launch_lookup(w2b_embed *e, Staging &s, int64_t n, int32_t dtype) {
  const double bytes = (double)n * (double)e->wpr * 8 + (double)n * (double)e->dim * elem_size(dtype);
  return timed(e, bytes, [&] {
    return w2b_launch_embed_lookup(e->T, e->rows, (int)e->dim, e->bitlevel, s.ids, n, dtype, s.out, e->bad, e->stream);
  });
}

int launch_bag(w2b_embed *e, Staging &s, int64_t n_ids, int64_t n_bags, int32_t mode, int32_t dtype) {
  const double bytes = (double)n_ids * (double)e->wpr * 8 + (double)n_bags * (double)e->dim * elem_size(dtype);
  return timed(e, bytes, [&] {
    return w2b_launch_embed_bag(e->T, e->rows, (int)e->dim, e->bitlevel, s.ids, n_ids, s.offsets, n_bags, mode, dtype, s.out,
                                e->bad, s.scratch, e->stream);
  });
}

int launch_bag_weighted(w2b_embed *e, Staging &s, int64_t n_ids, int64_t n_bags, int32_t mode, int32_t dtype) {
  const double bytes = (double)n_ids * ((double)e->wpr * 8 + 4) + (double)n_bags * (double)e->dim * elem_size(dtype);
  return timed(e, bytes, [&] {
    return w2b_launch_embed_bag_weighted(e->T, e->rows, (int)e->dim, e->bitlevel, s.ids, s.weights, n_ids, s.offsets, n_bags,
                                         mode, dtype, s.out, e->bad, s.wscratch, e->stream);
  });
}

// n vectors against m candidates: those of s.cand, or the rows cand_base .. cand_base + m when !use_cand
int launch_project(w2b_embed *e, ProjStaging &s, int64_t n, int64_t m, bool use_cand, int64_t cand_base, int32_t dtype) {
  const double bytes = (double)n * (double)e->dim * 4 + (double)m * (double)e->wpr * 8 + (use_cand ? (double)m * 8 : 0.0) +
                       (double)n * (double)m * elem_size(dtype);
  return timed(e, bytes, [&] {
    return w2b_launch_embed_project(e->T, e->rows, (int)e->dim, e->bitlevel, s.x, (int)n, use_cand ? s.cand : nullptr, cand_base,
                                    (int)m, dtype, s.operands, s.out, e->bad, e->stream);
  });
}

// n vectors of s.g (dense, m apart) against m candidate positions that begin a segment: those of s.cand, or the rows
// cand_base .. cand_base + m when !use_cand.  The scratch follows the call (it waits for the stream only when it has to grow).
int launch_backproject(w2b_embed *e, BackStaging &s, int64_t n, int64_t m, bool use_cand, int64_t cand_base, bool first,
                       bool last) {
  int use_scratch = 0, segs = 1;
  long long need = 0;
  w2b_embed_backproject_plan((int)e->dim, n, m, &use_scratch, &segs, &need);
  if (need > s.scratch_bytes)
    if (int rc = grow(e, s.scratch, s.scratch_bytes, need, need)) return rc;
  const double bytes = (double)n * (double)m * 4 + (double)m * (double)e->wpr * 8 + (use_cand ? (double)m * 8 : 0.0) +
                       (double)n * (double)e->dim * 4;
  return timed(e, bytes, [&] {
    return w2b_launch_embed_backproject(e->T, e->rows, (int)e->dim, e->bitlevel, s.g, m, n, use_cand ? s.cand : nullptr, cand_base,
                                        (int)m, first, last, s.dx, use_scratch, segs, s.scratch, e->bad, e->stream);
  });
}

// the cross-entropy's caller-facing buffers for max_n vectors and max_m candidates; only ever grow, each on its own
int ensure_xent(w2b_embed *e, XentStaging &s, int64_t max_n, int64_t max_m) {
  if (max_n > s.cap_n || !s.x) {
    int64_t have = 0;
    s.cap_n = 0;                                           // (a failed allocation leaves nothing reserved)
    if (int rc = grow(e, s.x, have, max_n * e->dim * 4, max_n)) return rc;
    if (int rc = grow(e, s.target, have, max_n * 8, max_n)) return rc;
    if (int rc = grow(e, s.teff, have, max_n * 8, max_n)) return rc;
    if (int rc = grow(e, s.stats, have, max_n * 12, max_n)) return rc;
    if (int rc = grow(e, s.dx, have, max_n * e->dim * 4, max_n)) return rc;
    s.cap_n = max_n;
  }
  const int64_t need = (int64_t)w2b_embed_project_operand_bytes((int)e->dim, s.cap_n);
  if (need > s.operand_bytes || !s.operands)
    if (int rc = grow(e, s.operands, s.operand_bytes, need, need)) return rc;
  if (max_m > s.cap_m || !s.cand) {
    int64_t have = 0;
    s.cap_m = 0;
    if (int rc = grow(e, s.cand, have, max_m * 8, max_m)) return rc;
    if (int rc = grow(e, s.clean, have, max_m * 8, max_m)) return rc;
    s.cap_m = max_m;
  }
  return W2B_OK;
}

// the bytes of g a gradient launch may use: kXentScratch, or less by W2B_EMBED_XENT_SCRATCH (bytes, read per call; for tests
// of the chunked path at small shapes)
int64_t xent_scratch_bytes() {
  int64_t b = kXentScratch;
  if (const char *env = getenv("W2B_EMBED_XENT_SCRATCH")) {
    const long long v = atoll(env);
    if (v > 0 && v < b) b = v;
  }
  return b;
}

// The whole call on the staging s: n vectors of s.x against m candidates (those of s.cand, or every row), targets in s.target;
// mx / se / tl into s.stats = [3][n], and dx into s.dx when want_dx.  The statistics run in ranges of vectors whose segment
// scratch stays within kXentScratch, the gradient in ranges of whole vectors whose g fits the scratch (or, when one vector's m
// candidates do not fit, of one vector x candidate ranges that are multiples of W2B_EMBED_WSEG, S carried by the back-projection).
int launch_xent(w2b_embed *e, XentStaging &s, int64_t n, int64_t m, bool use_cand, bool want_dx) {
  const int dim = (int)e->dim;
  const int64_t nseg = (m + W2B_EMBED_XSEG - 1) / W2B_EMBED_XSEG;
  float *mx = s.stats, *se = s.stats + n, *tl = s.stats + 2 * n;
  const long long *clean = use_cand ? s.clean : nullptr;
  const double cand_bytes = use_cand ? (double)m * 8 : 0.0, row_bytes = (double)m * (double)e->wpr * 8;
  // statistics: ranges of vectors, multiples of 64 (the pairs of the operand staging)
  int64_t sv = nseg > 0 ? kXentScratch / 12 / nseg / 64 * 64 : n;
  sv = sv < 64 ? 64 : sv;
  if (sv > n) sv = n;
  if (sv * nseg > s.seg_slots || !s.mseg) {
    const int64_t slots = sv * nseg > 0 ? sv * nseg : 1;
    int64_t have = 0;
    if (int rc = grow(e, s.mseg, have, slots * 4, slots)) return rc;
    if (int rc = grow(e, s.useg, s.seg_slots, slots * 8, slots)) return rc;
  }
  const double bytes = (double)n * dim * 4 + row_bytes + cand_bytes + (double)n * 8 + (double)n * 12;
  int rc = timed(e, bytes, [&] {
    hipError_t he = w2b_launch_vec_operands(s.x, dim, (int)n, s.operands, e->stream);
    if (he == hipSuccess && use_cand) he = w2b_launch_embed_xent_clean(s.cand, m, e->rows, s.clean, e->bad, e->stream);
    for (int64_t v0 = 0; v0 < n && he == hipSuccess; v0 += sv) {
      const int64_t v1 = v0 + sv < n ? v0 + sv : n;
      he = w2b_launch_embed_xent_stats(e->T, e->rows, dim, e->bitlevel, s.operands, (int)v0, (int)v1, clean, (int)m, s.target,
                                       s.mseg, s.useg, tl, e->stream);
      if (he == hipSuccess)
        he = w2b_launch_embed_xent_finish((int)v0, (int)v1, m, (int)nseg, s.mseg, s.useg, clean, s.target, mx, se, tl, s.teff,
                                          e->bad, e->stream);
    }
    return he;
  });
  if (rc || !want_dx) return rc;
  if (m == 0) {                                            // an empty sum: +0.0 rows, no launch
    EHIP(hipMemsetAsync(s.dx, 0, (size_t)(n * e->dim) * 4, e->stream));
    return W2B_OK;
  }
  // the gradient: whole vectors that fit the scratch, or one vector x candidate ranges
  const int64_t room = xent_scratch_bytes() / 4;
  int64_t gv = room / m, cm = m;
  if (gv < 1) {
    gv = 1;
    cm = room / W2B_EMBED_WSEG * W2B_EMBED_WSEG;
    if (cm < W2B_EMBED_WSEG) cm = W2B_EMBED_WSEG;
    if (cm > m) cm = m;
  }
  if (gv > n) gv = n;
  if (gv * cm * 4 > s.g_bytes || !s.g)
    if (int rc2 = grow(e, s.g, s.g_bytes, gv * cm * 4, gv * cm * 4)) return rc2;
  for (int64_t v0 = 0; v0 < n; v0 += gv) {
    const int64_t nv = n - v0 < gv ? n - v0 : gv;
    for (int64_t j0 = 0; j0 < m; j0 += cm) {
      const int64_t cj = m - j0 < cm ? m - j0 : cm;
      int use_scratch = 0, segs = 1;
      long long need = 0;
      w2b_embed_backproject_plan(dim, nv, cj, &use_scratch, &segs, &need);
      if (need > s.bscratch_bytes)
        if (int rc2 = grow(e, s.bscratch, s.bscratch_bytes, need, need)) return rc2;
      const double cb = use_cand ? (double)cj * 8 : 0.0;
      const double gbytes = 2.0 * (double)nv * dim * 4 + 2.0 * ((double)cj * (double)e->wpr * 8 + cb) + 2.0 * (double)nv * (double)cj * 4;
      rc = timed(e, gbytes, [&] {
        hipError_t he = w2b_launch_embed_xent_grad(e->T, e->rows, dim, e->bitlevel, s.operands, (int)v0, (int)(v0 + nv), clean, j0,
                                                   (int)cj, mx, se, s.teff, s.g, e->stream);
        if (he == hipSuccess)
          he = w2b_launch_embed_backproject(e->T, e->rows, dim, e->bitlevel, s.g, cj, nv, clean ? clean + j0 : nullptr, j0, (int)cj,
                                            j0 == 0, j0 + cj == m, s.dx + v0 * e->dim, use_scratch, segs, s.bscratch, e->bad,
                                            e->stream);
        return he;
      });
      if (rc) return rc;
    }
  }
  return W2B_OK;
}
}  // namespace

// ------------------------------------------------------------------------------------ constructors and accessors
extern "C" int w2b_embed_load(const char *w2bp_file, int64_t threshold, int32_t device, w2b_embed **out) {
  if (!w2bp_file || !out) return efail(W2B_EINVAL, "w2b_embed_load: null argument");
  *out = nullptr;
  FILE *f = fopen(w2bp_file, "rb");
  if (!f) return efail(W2B_EIO, "Input file not found");
  fseek(f, 0, SEEK_END);
  const long long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<unsigned char> d(n > 0 ? (size_t)n : 0);
  const bool ok = n <= 0 || fread(d.data(), 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  if (!ok) return efail(W2B_EIO, "w2b_embed_load: short read");
  if (!w2b_internal_is_packed(d.data(), d.size()))
    return efail(W2B_EINVAL, "w2b_embed_load: not a W2BP1 bit-packed file (float files are not read here)");
  EmbedPtr e(new w2b_embed);
  int64_t dim = 0;
  int bitlevel = 0;
  size_t pos = 0;
  if (w2b_internal_parse_packed_head(d.data(), d.size(), e->names, &dim, &bitlevel, &pos) != W2B_OK)
    return efail(W2B_EIO, "w2b_embed_load: damaged bit-packed file");
  if (threshold > 0 && (int64_t)e->names.size() > threshold) e->names.resize((size_t)threshold);
  e->rows = (int64_t)e->names.size();
  e->dim = dim;
  e->bitlevel = bitlevel;
  e->device = device;
  if (int rc = check_shape(e->rows, dim, bitlevel, 1, "w2b_embed_load")) return rc;
  e->wpr = w2b_packed_words_per_row(dim, bitlevel);
  if (int rc = device_visible(device, "w2b_embed_load")) return rc;
  e->has_words = true;
  for (int64_t r = 0; r < e->rows; r++) e->first.emplace(e->names[(size_t)r], r);     // the first row wins
  return embed_finish(std::move(e), d.data() + pos, out);
}

extern "C" int w2b_embed_create(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int32_t device,
                                w2b_embed **out) {
  if (!packed || !out) return efail(W2B_EINVAL, "w2b_embed_create: null argument");
  *out = nullptr;
  if (int rc = check_shape(rows, dim, bitlevel, 1, "w2b_embed_create")) return rc;
  if (int rc = device_visible(device, "w2b_embed_create")) return rc;
  EmbedPtr e(new w2b_embed);
  e->rows = rows;
  e->dim = dim;
  e->bitlevel = bitlevel;
  e->device = device;
  e->wpr = w2b_packed_words_per_row(dim, bitlevel);
  return embed_finish(std::move(e), (const unsigned char *)packed, out);
}

extern "C" void w2b_embed_free(w2b_embed *e) { embed_release(e); }
extern "C" int64_t w2b_embed_rows(const w2b_embed *e) { return e ? e->rows : 0; }
extern "C" int64_t w2b_embed_dim(const w2b_embed *e) { return e ? e->dim : 0; }
extern "C" int32_t w2b_embed_bitlevel(const w2b_embed *e) { return e ? e->bitlevel : 0; }
extern "C" const char *w2b_embed_word(const w2b_embed *e, int64_t row) {
  return e && e->has_words && row >= 0 && row < e->rows ? e->names[(size_t)row].c_str() : nullptr;
}
extern "C" int64_t w2b_embed_search(const w2b_embed *e, const char *word) {
  if (!e || !word) return -1;
  const auto it = e->first.find(word);
  return it == e->first.end() ? -1 : it->second;
}

// ------------------------------------------------------------------------------------ host form
extern "C" int w2b_embed_lookup(w2b_embed *e, int64_t n, const int32_t *ids, int32_t dtype, void *out) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_lookup: null handle");
  const int es = elem_size(dtype);
  if (!es) return efail(W2B_EINVAL, "w2b_embed_lookup: dtype is none of W2B_EMBED_F32 / BF16 / F16");
  if (int rc = check_ids(e->rows, n, ids, "w2b_embed_lookup")) return rc;
  if (n == 0) return W2B_OK;
  if (!out) return efail(W2B_EINVAL, "w2b_embed_lookup: null output");
  EHIP(hipSetDevice(e->device));
  const int64_t row_bytes = e->dim * es;
  int64_t chunk = kHostOutBytes / row_bytes;
  chunk = chunk < 1 ? 1 : (chunk > kHostIds ? kHostIds : chunk);
  std::vector<long long> wide;
  for (int64_t i0 = 0; i0 < n; i0 += chunk) {
    const int64_t c = n - i0 < chunk ? n - i0 : chunk;
    if (int rc = ensure(e, e->host, c, -1, c * row_bytes)) return rc;
    wide.assign(ids + i0, ids + i0 + c);
    EHIP(hipMemcpyAsync(e->host.ids, wide.data(), (size_t)c * 8, hipMemcpyHostToDevice, e->stream));
    if (int rc = launch_lookup(e, e->host, c, dtype)) return rc;
    EHIP(hipMemcpyAsync((char *)out + i0 * row_bytes, e->host.out, (size_t)(c * row_bytes), hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
  }
  return W2B_OK;
}

extern "C" int w2b_embed_bag(w2b_embed *e, int64_t n_ids, const int32_t *ids, int64_t n_bags, const int64_t *offsets,
                             int32_t mode, int32_t dtype, void *out) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_bag: null handle");
  const int es = elem_size(dtype);
  if (!es) return efail(W2B_EINVAL, "w2b_embed_bag: dtype is none of W2B_EMBED_F32 / BF16 / F16");
  if (int rc = check_ids(e->rows, n_ids, ids, "w2b_embed_bag")) return rc;
  if (int rc = check_bags(n_ids, n_bags, offsets, mode, "w2b_embed_bag")) return rc;
  if (n_bags == 0) return W2B_OK;
  if (!out) return efail(W2B_EINVAL, "w2b_embed_bag: null output");
  EHIP(hipSetDevice(e->device));
  const int64_t row_bytes = e->dim * es;
  int64_t max_bags = kHostOutBytes / row_bytes;
  if (max_bags < 1) max_bags = 1;
  std::vector<long long> wide, off;
  for (int64_t b0 = 0; b0 < n_bags;) {
    int64_t b1 = b0 + 1;                                   // bags b0 .. b1 - 1: at least one, then while they fit
    while (b1 < n_bags && b1 - b0 < max_bags && offsets[b1 + 1] - offsets[b0] <= kHostIds) b1++;
    const int64_t i0 = offsets[b0], ci = offsets[b1] - i0, cb = b1 - b0;
    if (int rc = ensure(e, e->host, ci > 0 ? ci : 1, cb, cb * row_bytes)) return rc;
    wide.assign(ids + i0, ids + i0 + ci);
    off.resize((size_t)cb + 1);
    for (int64_t b = 0; b <= cb; b++) off[(size_t)b] = offsets[b0 + b] - i0;
    if (ci > 0) EHIP(hipMemcpyAsync(e->host.ids, wide.data(), (size_t)ci * 8, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemcpyAsync(e->host.offsets, off.data(), (size_t)(cb + 1) * 8, hipMemcpyHostToDevice, e->stream));
    if (int rc = launch_bag(e, e->host, ci, cb, mode, dtype)) return rc;
    EHIP(hipMemcpyAsync((char *)out + b0 * row_bytes, e->host.out, (size_t)(cb * row_bytes), hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    b0 = b1;
  }
  return W2B_OK;
}

extern "C" int w2b_embed_bag_weighted(w2b_embed *e, int64_t n_ids, const int32_t *ids, const float *weights, int64_t n_bags,
                                      const int64_t *offsets, int32_t mode, int32_t dtype, void *out) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_bag_weighted: null handle");
  const int es = elem_size(dtype);
  if (!es) return efail(W2B_EINVAL, "w2b_embed_bag_weighted: dtype is none of W2B_EMBED_F32 / BF16 / F16");
  if (int rc = check_ids(e->rows, n_ids, ids, "w2b_embed_bag_weighted")) return rc;
  if (int rc = check_bags(n_ids, n_bags, offsets, mode, "w2b_embed_bag_weighted")) return rc;
  if (int rc = check_weights(n_ids, ids, weights, "w2b_embed_bag_weighted")) return rc;
  if (n_bags == 0) return W2B_OK;
  if (!out) return efail(W2B_EINVAL, "w2b_embed_bag_weighted: null output");
  EHIP(hipSetDevice(e->device));
  const int64_t row_bytes = e->dim * es;
  int64_t max_bags = kHostOutBytes / row_bytes;
  if (max_bags < 1) max_bags = 1;
  std::vector<long long> wide, off;
  for (int64_t b0 = 0; b0 < n_bags;) {                     // the chunks of w2b_embed_bag
    int64_t b1 = b0 + 1;
    while (b1 < n_bags && b1 - b0 < max_bags && offsets[b1 + 1] - offsets[b0] <= kHostIds) b1++;
    const int64_t i0 = offsets[b0], ci = offsets[b1] - i0, cb = b1 - b0;
    if (int rc = ensure(e, e->host, ci > 0 ? ci : 1, cb, cb * row_bytes)) return rc;
    if (int rc = ensure_weighted(e, e->host, e->host.cap_ids, ci, cb)) return rc;
    wide.assign(ids + i0, ids + i0 + ci);
    off.resize((size_t)cb + 1);
    for (int64_t b = 0; b <= cb; b++) off[(size_t)b] = offsets[b0 + b] - i0;
    if (ci > 0) {
      EHIP(hipMemcpyAsync(e->host.ids, wide.data(), (size_t)ci * 8, hipMemcpyHostToDevice, e->stream));
      EHIP(hipMemcpyAsync(e->host.weights, weights + i0, (size_t)ci * 4, hipMemcpyHostToDevice, e->stream));
    }
    EHIP(hipMemcpyAsync(e->host.offsets, off.data(), (size_t)(cb + 1) * 8, hipMemcpyHostToDevice, e->stream));
    if (int rc = launch_bag_weighted(e, e->host, ci, cb, mode, dtype)) return rc;
    EHIP(hipMemcpyAsync((char *)out + b0 * row_bytes, e->host.out, (size_t)(cb * row_bytes), hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    b0 = b1;
  }
  return W2B_OK;
}

extern "C" int w2b_embed_project(w2b_embed *e, int64_t n, const float *x, int64_t m, const int32_t *cand, int32_t dtype,
                                 void *out) {
  const char *who = "w2b_embed_project";
  const int es = elem_size(dtype);
  if (int rc = project_check_args(who, n, x, m, es != 0, out)) return rc;
  if (!e) return efail(W2B_EINVAL, "w2b_embed_project: null handle");
  if (int rc = project_check_cand(who, e->rows, m, cand)) return rc;
  if (int rc = project_check_values(who, n, e->dim, x)) return rc;
  if (n == 0 || m == 0) return W2B_OK;
  EHIP(hipSetDevice(e->device));
  // whole vectors x whole candidate ranges, about kHostOutBytes of output per launch
  const int64_t nv = n < 4096 ? n : 4096;
  int64_t cm = kHostOutBytes / (es * nv);
  if (cm > kHostIds) cm = kHostIds;
  if (cm >= 64) cm = cm / 64 * 64;
  cm = cm < 1 ? 1 : (cm > m ? m : cm);
  std::vector<long long> wide;
  std::vector<char> part;
  for (int64_t i0 = 0; i0 < n; i0 += nv) {
    const int64_t ci = n - i0 < nv ? n - i0 : nv;
    if (int rc = ensure_project(e, e->phost, nv, cm, nv * cm * es)) return rc;
    EHIP(hipMemcpyAsync(e->phost.x, x + i0 * e->dim, (size_t)(ci * e->dim) * 4, hipMemcpyHostToDevice, e->stream));
    for (int64_t j0 = 0; j0 < m; j0 += cm) {
      const int64_t cj = m - j0 < cm ? m - j0 : cm;
      if (cand) {
        wide.assign(cand + j0, cand + j0 + cj);
        EHIP(hipMemcpyAsync(e->phost.cand, wide.data(), (size_t)cj * 8, hipMemcpyHostToDevice, e->stream));
      }
      if (int rc = launch_project(e, e->phost, ci, cj, cand != nullptr, j0, dtype)) return rc;
      if (cj == m) {                                       // the chunk's rows are the caller's rows
        EHIP(hipMemcpyAsync((char *)out + i0 * m * es, e->phost.out, (size_t)(ci * m * es), hipMemcpyDeviceToHost, e->stream));
        EHIP(hipStreamSynchronize(e->stream));
      } else {                                             // a range of columns: through host memory, row by row
        part.resize((size_t)(ci * cj * es));
        EHIP(hipMemcpyAsync(part.data(), e->phost.out, part.size(), hipMemcpyDeviceToHost, e->stream));
        EHIP(hipStreamSynchronize(e->stream));
        for (int64_t i = 0; i < ci; i++)
          memcpy((char *)out + ((i0 + i) * m + j0) * es, part.data() + i * cj * es, (size_t)(cj * es));
      }
    }
  }
  return W2B_OK;
}

extern "C" int w2b_embed_backproject(w2b_embed *e, int64_t n, const float *g, int64_t m, const int32_t *cand, float *dx) {
  const char *who = "w2b_embed_backproject";
  if (int rc = backproject_check_args(who, n, g, m, dx)) return rc;
  if (!e) return efail(W2B_EINVAL, "w2b_embed_backproject: null handle");
  if (int rc = project_check_cand(who, e->rows, m, cand)) return rc;
  if (int rc = backproject_check_values(who, n, m, cand, g)) return rc;
  if (n == 0) return W2B_OK;
  if (m == 0) {
    memset(dx, 0, (size_t)(n * e->dim) * 4);
    return W2B_OK;
  }
  EHIP(hipSetDevice(e->device));
  // whole vectors x candidate ranges that are multiples of W2B_EMBED_WSEG, about kHostOutBytes of g per launch (and of dx
  // per range of vectors); S is carried in the device's dx from one candidate range to the next
  int64_t nv = kHostOutBytes / (e->dim * 4);
  nv = nv < 1 ? 1 : (nv > 4096 ? 4096 : nv);
  if (nv > n) nv = n;
  int64_t cm = kHostOutBytes / (4 * nv) / W2B_EMBED_WSEG * W2B_EMBED_WSEG;   // (at least 4096: nv <= 4096)
  if (cm > kHostIds) cm = kHostIds;
  if (cm > m) cm = m;
  std::vector<long long> wide;
  for (int64_t i0 = 0; i0 < n; i0 += nv) {
    const int64_t ci = n - i0 < nv ? n - i0 : nv;
    if (int rc = ensure_back(e, e->bhost, nv, cm)) return rc;
    for (int64_t j0 = 0; j0 < m; j0 += cm) {
      const int64_t cj = m - j0 < cm ? m - j0 : cm;
      if (cand) {
        wide.assign(cand + j0, cand + j0 + cj);
        EHIP(hipMemcpyAsync(e->bhost.cand, wide.data(), (size_t)cj * 8, hipMemcpyHostToDevice, e->stream));
      }
      EHIP(hipMemcpy2DAsync(e->bhost.g, (size_t)cj * 4, g + i0 * m + j0, (size_t)m * 4, (size_t)cj * 4, (size_t)ci,
                            hipMemcpyHostToDevice, e->stream));
      if (int rc = launch_backproject(e, e->bhost, ci, cj, cand != nullptr, j0, j0 == 0, j0 + cj == m)) return rc;
      EHIP(hipStreamSynchronize(e->stream));               // (wide and the staging are written again for the next range)
    }
    EHIP(hipMemcpyAsync(dx + i0 * e->dim, e->bhost.dx, (size_t)(ci * e->dim) * 4, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
  }
  return W2B_OK;
}

extern "C" int w2b_embed_xent(w2b_embed *e, int64_t n, const float *x, int64_t m, const int32_t *cand, const int32_t *target,
                              float *mx, float *se, float *tl, float *dx) {
  const char *who = "w2b_embed_xent";
  if (int rc = xent_check_args(who, n, x, m, target, mx, se, tl)) return rc;
  if (!e) return efail(W2B_EINVAL, "w2b_embed_xent: null handle");
  if (int rc = project_check_cand(who, e->rows, m, cand)) return rc;
  if (int rc = xent_check_targets(who, n, m, cand, target)) return rc;
  if (int rc = project_check_values(who, n, e->dim, x)) return rc;
  if (n == 0) return W2B_OK;
  EHIP(hipSetDevice(e->device));
  // ranges of whole vectors (they are independent); the candidate list is staged whole, 16 bytes per candidate
  const int64_t nv = n < 4096 ? n : 4096;
  if (int rc = ensure_xent(e, e->xhost, nv, m > 0 ? m : 1)) return rc;
  XentStaging &s = e->xhost;
  std::vector<long long> wide;
  if (cand && m > 0) {
    wide.assign(cand, cand + m);
    EHIP(hipMemcpyAsync(s.cand, wide.data(), (size_t)m * 8, hipMemcpyHostToDevice, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
  }
  for (int64_t i0 = 0; i0 < n; i0 += nv) {
    const int64_t ci = n - i0 < nv ? n - i0 : nv;
    wide.assign(target + i0, target + i0 + ci);
    EHIP(hipMemcpyAsync(s.x, x + i0 * e->dim, (size_t)(ci * e->dim) * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemcpyAsync(s.target, wide.data(), (size_t)ci * 8, hipMemcpyHostToDevice, e->stream));
    if (int rc = launch_xent(e, s, ci, m, cand != nullptr, dx != nullptr)) return rc;
    EHIP(hipMemcpyAsync(mx + i0, s.stats, (size_t)ci * 4, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipMemcpyAsync(se + i0, s.stats + ci, (size_t)ci * 4, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipMemcpyAsync(tl + i0, s.stats + 2 * ci, (size_t)ci * 4, hipMemcpyDeviceToHost, e->stream));
    if (dx) EHIP(hipMemcpyAsync(dx + i0 * e->dim, s.dx, (size_t)(ci * e->dim) * 4, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
  }
  return W2B_OK;
}

// ------------------------------------------------------------------------------------ device form
extern "C" int w2b_embed_reserve_xent(w2b_embed *e, int64_t max_n, int64_t max_m, void **x_dev, void **cand_dev,
                                      void **target_dev, void **stats_dev, void **dx_dev) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_reserve_xent: null handle");
  if (max_n < 0 || max_n > kProjectMaxVectors || max_m < 0 || max_m > 0x7FFFFF00ll || max_n * e->dim > (1ll << 40))
    return efail(W2B_EINVAL, "w2b_embed_reserve_xent: bad sizes");
  EHIP(hipSetDevice(e->device));
  if (int rc = ensure_xent(e, e->xuser, max_n, max_m)) return rc;
  if (x_dev) *x_dev = e->xuser.x;
  if (cand_dev) *cand_dev = e->xuser.cand;
  if (target_dev) *target_dev = e->xuser.target;
  if (stats_dev) *stats_dev = e->xuser.stats;
  if (dx_dev) *dx_dev = e->xuser.dx;
  return W2B_OK;
}

extern "C" int w2b_embed_xent_device(w2b_embed *e, int64_t n, int64_t m, int32_t use_cand, int32_t want_dx) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_xent_device: null handle");
  if (n < 0 || m < 0) return efail(W2B_EINVAL, "w2b_embed_xent_device: negative count");
  if (use_cand != 0 && use_cand != 1) return efail(W2B_EINVAL, "w2b_embed_xent_device: use_cand must be 0 or 1");
  if (want_dx != 0 && want_dx != 1) return efail(W2B_EINVAL, "w2b_embed_xent_device: want_dx must be 0 or 1");
  if (n == 0) return W2B_OK;
  XentStaging &s = e->xuser;
  if (!s.x || !s.cand || n > s.cap_n || m > s.cap_m)
    return efail(W2B_EINVAL, "w2b_embed_xent_device: more than w2b_embed_reserve_xent has set aside");
  if (!use_cand && m != e->rows) return efail(W2B_EINVAL, "w2b_embed_xent_device: without candidates m must be rows");
  EHIP(hipSetDevice(e->device));
  return launch_xent(e, s, n, m, use_cand != 0, want_dx != 0);
}

extern "C" int w2b_embed_reserve_backproject(w2b_embed *e, int64_t max_n, int64_t max_m, void **g_dev, void **cand_dev,
                                             void **dx_dev) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_reserve_backproject: null handle");
  if (max_n < 0 || max_n > kProjectMaxVectors || max_m < 0 || max_m > 0x7FFFFF00ll || max_n * max_m > (1ll << 40) ||
      max_n * e->dim > (1ll << 40))
    return efail(W2B_EINVAL, "w2b_embed_reserve_backproject: bad sizes");
  EHIP(hipSetDevice(e->device));
  if (int rc = ensure_back(e, e->buser, max_n, max_m)) return rc;
  if (g_dev) *g_dev = e->buser.g;
  if (cand_dev) *cand_dev = e->buser.cand;
  if (dx_dev) *dx_dev = e->buser.dx;
  return W2B_OK;
}

extern "C" int w2b_embed_backproject_device(w2b_embed *e, int64_t n, int64_t m, int32_t use_cand) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_backproject_device: null handle");
  if (n < 0 || m < 0) return efail(W2B_EINVAL, "w2b_embed_backproject_device: negative count");
  if (use_cand != 0 && use_cand != 1) return efail(W2B_EINVAL, "w2b_embed_backproject_device: use_cand must be 0 or 1");
  if (n == 0) return W2B_OK;
  BackStaging &s = e->buser;
  if (!s.g || !s.cand || !s.dx || n > s.cap_n || m > s.cap_m || n * m > s.g_elems)
    return efail(W2B_EINVAL, "w2b_embed_backproject_device: more than w2b_embed_reserve_backproject has set aside");
  if (!use_cand && m != e->rows) return efail(W2B_EINVAL, "w2b_embed_backproject_device: without candidates m must be rows");
  EHIP(hipSetDevice(e->device));
  if (m == 0) {                                            // an empty sum: +0.0 rows, no launch
    EHIP(hipMemsetAsync(s.dx, 0, (size_t)(n * e->dim) * 4, e->stream));
    return W2B_OK;
  }
  return launch_backproject(e, s, n, m, use_cand != 0, 0, true, true);
}

extern "C" int w2b_embed_reserve_project(w2b_embed *e, int64_t max_n, int64_t max_m, int32_t dtype, void **x_dev,
                                         void **cand_dev, void **out_dev) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_reserve_project: null handle");
  const int es = elem_size(dtype);
  if (!es) return efail(W2B_EINVAL, "w2b_embed_reserve_project: dtype is none of W2B_EMBED_F32 / BF16 / F16");
  if (max_n < 0 || max_n > kProjectMaxVectors || max_m < 0 || max_m > 0x7FFFFF00ll || max_n * max_m > (1ll << 40))
    return efail(W2B_EINVAL, "w2b_embed_reserve_project: bad sizes");
  EHIP(hipSetDevice(e->device));
  if (int rc = ensure_project(e, e->puser, max_n, max_m, max_n * max_m * es)) return rc;
  if (x_dev) *x_dev = e->puser.x;
  if (cand_dev) *cand_dev = e->puser.cand;
  if (out_dev) *out_dev = e->puser.out;
  return W2B_OK;
}

extern "C" int w2b_embed_project_device(w2b_embed *e, int64_t n, int64_t m, int32_t use_cand, int32_t dtype) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_project_device: null handle");
  const int es = elem_size(dtype);
  if (!es) return efail(W2B_EINVAL, "w2b_embed_project_device: dtype is none of W2B_EMBED_F32 / BF16 / F16");
  if (n < 0 || m < 0) return efail(W2B_EINVAL, "w2b_embed_project_device: negative count");
  if (use_cand != 0 && use_cand != 1) return efail(W2B_EINVAL, "w2b_embed_project_device: use_cand must be 0 or 1");
  if (n == 0 || m == 0) return W2B_OK;
  const ProjStaging &s = e->puser;
  if (!s.x || !s.cand || !s.out || n > s.cap_n || m > s.cap_m || n * m * es > s.out_bytes)
    return efail(W2B_EINVAL, "w2b_embed_project_device: more than w2b_embed_reserve_project has set aside");
  if (!use_cand && m != e->rows) return efail(W2B_EINVAL, "w2b_embed_project_device: without candidates m must be rows");
  EHIP(hipSetDevice(e->device));
  return launch_project(e, e->puser, n, m, use_cand != 0, 0, dtype);
}

extern "C" int w2b_embed_reserve(w2b_embed *e, int64_t max_ids, int64_t max_bags, int32_t dtype, void **ids_dev,
                                 void **offsets_dev, void **out_dev) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_reserve: null handle");
  const int es = elem_size(dtype);
  if (!es) return efail(W2B_EINVAL, "w2b_embed_reserve: dtype is none of W2B_EMBED_F32 / BF16 / F16");
  if (max_ids < 0 || max_bags < 0 || max_bags > 0x7FFFFF00ll || max_ids > (1ll << 40))
    return efail(W2B_EINVAL, "w2b_embed_reserve: bad sizes");
  EHIP(hipSetDevice(e->device));
  const int64_t out_rows = max_ids > max_bags ? max_ids : max_bags;
  if (int rc = ensure(e, e->user, max_ids, max_bags, out_rows * e->dim * es)) return rc;
  if (ids_dev) *ids_dev = e->user.ids;
  if (offsets_dev) *offsets_dev = e->user.offsets;
  if (out_dev) *out_dev = e->user.out;
  return W2B_OK;
}

extern "C" int w2b_embed_lookup_device(w2b_embed *e, int64_t n, int32_t dtype) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_lookup_device: null handle");
  const int es = elem_size(dtype);
  if (!es) return efail(W2B_EINVAL, "w2b_embed_lookup_device: dtype is none of W2B_EMBED_F32 / BF16 / F16");
  if (n < 0) return efail(W2B_EINVAL, "w2b_embed_lookup_device: negative id count");
  if (n == 0) return W2B_OK;
  if (!e->user.ids || !e->user.out || n > e->user.cap_ids || n * e->dim * es > e->user.out_bytes)
    return efail(W2B_EINVAL, "w2b_embed_lookup_device: more than w2b_embed_reserve has set aside");
  EHIP(hipSetDevice(e->device));
  return launch_lookup(e, e->user, n, dtype);
}

extern "C" int w2b_embed_bag_device(w2b_embed *e, int64_t n_ids, int64_t n_bags, int32_t mode, int32_t dtype) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_bag_device: null handle");
  const int es = elem_size(dtype);
  if (!es) return efail(W2B_EINVAL, "w2b_embed_bag_device: dtype is none of W2B_EMBED_F32 / BF16 / F16");
  if (mode != W2B_EMBED_SUM && mode != W2B_EMBED_MEAN)
    return efail(W2B_EINVAL, "w2b_embed_bag_device: mode is neither W2B_EMBED_SUM nor W2B_EMBED_MEAN");
  if (n_ids < 0 || n_bags < 0) return efail(W2B_EINVAL, "w2b_embed_bag_device: negative count");
  if (n_bags == 0) return W2B_OK;
  const Staging &s = e->user;
  if (!s.ids || !s.offsets || !s.out || !s.scratch || n_ids > s.cap_ids || n_bags > s.cap_bags ||
      n_bags * e->dim * es > s.out_bytes)
    return efail(W2B_EINVAL, "w2b_embed_bag_device: more than w2b_embed_reserve has set aside");
  EHIP(hipSetDevice(e->device));
  return launch_bag(e, e->user, n_ids, n_bags, mode, dtype);
}

extern "C" int w2b_embed_reserve_weights(w2b_embed *e, int64_t max_ids, void **weights_dev) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_reserve_weights: null handle");
  if (max_ids < 0 || max_ids > (1ll << 40)) return efail(W2B_EINVAL, "w2b_embed_reserve_weights: bad size");
  EHIP(hipSetDevice(e->device));
  Staging &s = e->user;                                    // the scratch for what w2b_embed_reserve has set aside so far
  const int64_t ids = max_ids < s.cap_ids ? max_ids : s.cap_ids;
  if (int rc = ensure_weighted(e, s, max_ids, ids, s.cap_bags)) return rc;
  if (weights_dev) *weights_dev = s.weights;
  return W2B_OK;
}

extern "C" int w2b_embed_bag_weighted_device(w2b_embed *e, int64_t n_ids, int64_t n_bags, int32_t mode, int32_t dtype) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_bag_weighted_device: null handle");
  const int es = elem_size(dtype);
  if (!es) return efail(W2B_EINVAL, "w2b_embed_bag_weighted_device: dtype is none of W2B_EMBED_F32 / BF16 / F16");
  if (mode != W2B_EMBED_SUM && mode != W2B_EMBED_MEAN)
    return efail(W2B_EINVAL, "w2b_embed_bag_weighted_device: mode is neither W2B_EMBED_SUM nor W2B_EMBED_MEAN");
  if (n_ids < 0 || n_bags < 0) return efail(W2B_EINVAL, "w2b_embed_bag_weighted_device: negative count");
  if (n_bags == 0) return W2B_OK;
  Staging &s = e->user;
  if (!s.ids || !s.offsets || !s.out || n_ids > s.cap_ids || n_bags > s.cap_bags || n_bags * e->dim * es > s.out_bytes)
    return efail(W2B_EINVAL, "w2b_embed_bag_weighted_device: more than w2b_embed_reserve has set aside");
  if (!s.weights || n_ids > s.cap_weights)
    return efail(W2B_EINVAL, "w2b_embed_bag_weighted_device: more than w2b_embed_reserve_weights has set aside");
  EHIP(hipSetDevice(e->device));
  // the scratch follows the call (it waits for the stream only when it has to grow); the weights buffer stays as it is
  if (int rc = ensure_weighted(e, s, s.cap_weights, n_ids, n_bags)) return rc;
  return launch_bag_weighted(e, s, n_ids, n_bags, mode, dtype);
}

extern "C" int w2b_embed_synchronize(w2b_embed *e) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_synchronize: null handle");
  EHIP(hipSetDevice(e->device));
  EHIP(hipStreamSynchronize(e->stream));
  return W2B_OK;
}

extern "C" int w2b_embed_bad_ids(w2b_embed *e, int64_t *count) {
  if (!e || !count) return efail(W2B_EINVAL, "w2b_embed_bad_ids: null argument");
  EHIP(hipSetDevice(e->device));
  EHIP(hipStreamSynchronize(e->stream));
  unsigned long long c = 0;
  EHIP(hipMemcpy(&c, e->bad, 8, hipMemcpyDeviceToHost));
  EHIP(hipMemset(e->bad, 0, 8));
  *count = (int64_t)c;
  return W2B_OK;
}

extern "C" int w2b_embed_timing_read(w2b_embed *e, double *kernel_ms, int64_t *launches, double *bytes) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_timing_read: null handle");
  EHIP(hipSetDevice(e->device));
  if (int rc = fold_pending(e)) return rc;
  if (kernel_ms) *kernel_ms = e->kernel_ms;
  if (launches) *launches = e->launches;
  if (bytes) *bytes = e->bytes;
  e->kernel_ms = 0;
  e->launches = 0;
  e->bytes = 0;
  return W2B_OK;
}

// ------------------------------------------------------------------------------------ host twins
static inline float bits_f32(uint32_t b) { float x; memcpy(&x, &b, 4); return x; }

extern "C" int w2b_embed_lookup_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n,
                                     const int32_t *ids, float *out) {
  if (!packed) return efail(W2B_EINVAL, "w2b_embed_lookup_host: null table");
  if (int rc = check_shape(rows, dim, bitlevel, 0, "w2b_embed_lookup_host")) return rc;
  if (int rc = check_ids(rows, n, ids, "w2b_embed_lookup_host")) return rc;
  if (n == 0) return W2B_OK;
  if (!out) return efail(W2B_EINVAL, "w2b_embed_lookup_host: null output");
  const int64_t wpr = w2b_packed_words_per_row(dim, bitlevel);
  for (int64_t i = 0; i < n; i++) {
    float *o = out + i * dim;
    if (ids[i] < 0) {
      for (int64_t c = 0; c < dim; c++) o[c] = 0.f;
      continue;
    }
    const uint64_t *row = packed + (int64_t)ids[i] * wpr;
    for (int64_t c = 0; c < dim; c++) {
      const uint64_t *blk = row + (c >> 6) * bitlevel;
      const uint32_t s = (uint32_t)(blk[0] >> (c & 63)) & 1u;
      const uint32_t mag = bitlevel == 1 ? 0x3EAAAAABu : (((blk[1] >> (c & 63)) & 1u) ? 0x3F400000u : 0x3E800000u);
      o[c] = bits_f32(mag | (s << 31));
    }
  }
  return W2B_OK;
}

extern "C" int w2b_embed_bag_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n_ids,
                                  const int32_t *ids, int64_t n_bags, const int64_t *offsets, int32_t mode, float *out) {
  if (!packed) return efail(W2B_EINVAL, "w2b_embed_bag_host: null table");
  if (int rc = check_shape(rows, dim, bitlevel, 0, "w2b_embed_bag_host")) return rc;
  if (int rc = check_ids(rows, n_ids, ids, "w2b_embed_bag_host")) return rc;
  if (int rc = check_bags(n_ids, n_bags, offsets, mode, "w2b_embed_bag_host")) return rc;
  if (n_bags == 0) return W2B_OK;
  if (!out) return efail(W2B_EINVAL, "w2b_embed_bag_host: null output");
  const int64_t wpr = w2b_packed_words_per_row(dim, bitlevel);
  const float q = bitlevel == 1 ? bits_f32(0x3EAAAAABu) : 0.25f;
  std::vector<int32_t> T((size_t)dim);
  for (int64_t b = 0; b < n_bags; b++) {
    std::fill(T.begin(), T.end(), 0);
    int32_t m = 0;
    for (int64_t i = offsets[b]; i < offsets[b + 1]; i++) {
      if (ids[i] < 0) continue;
      m++;
      const uint64_t *row = packed + (int64_t)ids[i] * wpr;
      for (int64_t c = 0; c < dim; c++) {
        const uint64_t *blk = row + (c >> 6) * bitlevel;
        const int s = (int)((blk[0] >> (c & 63)) & 1u);
        const int mag = bitlevel == 2 && ((blk[1] >> (c & 63)) & 1u) ? 3 : 1;
        T[(size_t)c] += s ? -mag : mag;
      }
    }
    float *o = out + b * dim;
    for (int64_t c = 0; c < dim; c++) {
      const float sum = (float)T[(size_t)c] * q;             // one float32 multiply (no contraction: -ffp-contract=off)
      o[c] = mode == W2B_EMBED_MEAN ? (m > 0 ? sum / (float)m : 0.f) : sum;
    }
  }
  return W2B_OK;
}

extern "C" int w2b_embed_bag_weighted_host(const uint64_t *packed, int64_t rows, int64_t dim, int32_t bitlevel, int64_t n_ids,
                                           const int32_t *ids, const float *weights, int64_t n_bags, const int64_t *offsets,
                                           int32_t mode, float *out) {
  if (!packed) return efail(W2B_EINVAL, "w2b_embed_bag_weighted_host: null table");
  if (int rc = check_shape(rows, dim, bitlevel, 0, "w2b_embed_bag_weighted_host")) return rc;
  if (int rc = check_ids(rows, n_ids, ids, "w2b_embed_bag_weighted_host")) return rc;
  if (int rc = check_bags(n_ids, n_bags, offsets, mode, "w2b_embed_bag_weighted_host")) return rc;
  if (int rc = check_weights(n_ids, ids, weights, "w2b_embed_bag_weighted_host")) return rc;
  if (n_bags == 0) return W2B_OK;
  if (!out) return efail(W2B_EINVAL, "w2b_embed_bag_weighted_host: null output");
  const int64_t wpr = w2b_packed_words_per_row(dim, bitlevel);
  const float q = bitlevel == 1 ? bits_f32(0x3EAAAAABu) : 0.25f;
  std::vector<float> P((size_t)dim), S((size_t)dim);
  for (int64_t b = 0; b < n_bags; b++) {
    std::fill(S.begin(), S.end(), 0.f);
    int32_t m = 0;
    for (int64_t s0 = offsets[b]; s0 < offsets[b + 1]; s0 += W2B_EMBED_WSEG) {      // one segment: one chain per column
      const int64_t s1 = std::min<int64_t>(s0 + W2B_EMBED_WSEG, offsets[b + 1]);
      std::fill(P.begin(), P.end(), 0.f);
      for (int64_t i = s0; i < s1; i++) {
        if (ids[i] < 0) continue;
        m++;
        const float w = weights[i];
        const uint64_t *row = packed + (int64_t)ids[i] * wpr;
        for (int64_t c = 0; c < dim; c++) {
          const uint64_t *blk = row + (c >> 6) * bitlevel;
          const int sg = (int)((blk[0] >> (c & 63)) & 1u);
          const int mag = bitlevel == 2 && ((blk[1] >> (c & 63)) & 1u) ? 3 : 1;
          P[(size_t)c] = fmaf(w, (float)(sg ? -mag : mag), P[(size_t)c]);
        }
      }
      for (int64_t c = 0; c < dim; c++) S[(size_t)c] = S[(size_t)c] + P[(size_t)c];     // one float32 add per segment
    }
    float *o = out + b * dim;
    for (int64_t c = 0; c < dim; c++) {
      const float sum = S[(size_t)c] * q;                    // one float32 multiply (no contraction: -ffp-contract=off)
      o[c] = mode == W2B_EMBED_MEAN ? (m > 0 ? sum / (float)m : 0.f) : sum;
    }
  }
  return W2B_OK;
}
