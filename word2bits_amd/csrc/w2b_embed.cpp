// w2b_embed.cpp -- host side of include/word2bits_embed.h: the handle, the .w2bp loader, the device staging (per feature one
// set of buffers handed to the caller by w2b_embed_reserve*, and a separate bounded one for the host form; every buffer is a
// DevBuf, which only moves when it grows itself), the chunking of host-form calls, the launches and timing.  What needs no
// handle is not here: every validator is in w2b_embed_shared.h, every host twin in the host-only w2b_embed_twins.cpp.  The
// table stays packed on the device; no float table exists on either side and there is no CPU fallback (the *_host twins are
// for tests).
#include "../../include/word2bits_embed.h"
#include "../../include/word2bits_corpus.h"
#include "../../include/word2bits_hip.h"
#include "w2b_internal.h"
#include "w2b_embed_shared.h"

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
constexpr int64_t kXentScratch = 64ll << 20;      // bytes of g per gradient launch, and of segment statistics per statistics launch
constexpr int64_t kTopkScratch = 64ll << 20;      // bytes of unit maxima and key lists per range of vectors (or one pair of vector tiles)

int efail(int code, const std::string &msg) { return w2b_internal_fail(code, msg.c_str()); }
#define EHIP(x)                                                                                   \
  do {                                                                                            \
    hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess) return efail(W2B_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

// One device buffer that the handle owns: the pointer and its capacity, in whatever unit its owner counts (ids, vectors,
// bytes).  Empty until reserve() below has grown it; freed with the handle.
template <class T>
struct DevBuf {
  T *p = nullptr;
  int64_t cap = 0;
  explicit DevBuf(int64_t cap0 = 0) : cap(cap0) {}
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// device staging of one form of lookup and bags
struct Staging {
  DevBuf<long long> ids, offsets{-1};        // [cap] and [cap + 1]; -1: no offsets buffer (a lookup reserves none)
  DevBuf<void> out, scratch;                 // bytes
  DevBuf<float> weights;                     // weighted bags only: a buffer [cap] and a scratch (bytes) of their own
  DevBuf<void> wscratch;
};
// device staging of one form of the projection: buffers of their own
struct ProjStaging {
  DevBuf<float> x;                           // [cap][dim]
  DevBuf<long long> cand;                    // [cap]
  DevBuf<void> out, operands;                // bytes: [n][m] of a dtype; the vectors in fragment order (for x.cap vectors)
};
// device staging of one form of the back-projection: buffers of their own again; the scratch follows the call
struct BackStaging {
  DevBuf<float> g;                           // cap = max_n * max_m values reserved; a call's g is dense [n][m]
  DevBuf<long long> cand;                    // [cap]
  DevBuf<float> dx;                          // [cap][dim]
  DevBuf<void> scratch;                      // bytes: the segments' partial sums, when the driver sends them through the scratch
};
// device staging of one form of the cross-entropy: buffers of their own once more.  What a caller fills or reads (x, cand,
// target, stats, dx) moves only when that buffer itself grows; the rest follows the call.
struct XentStaging {
  DevBuf<float> x;                           // [cap][dim]; target, teff, stats and dx share its capacity
  DevBuf<long long> target, teff;            // the caller's targets; the effective ones (-1 = ignored)
  DevBuf<float> stats;                       // [3][n] for the n of a call: mx, se, tl
  DevBuf<float> dx;                          // [cap][dim]
  DevBuf<long long> cand, clean;             // [cap], one capacity: the caller's candidates; ids >= rows made padding
  DevBuf<void> operands;                     // bytes: the vectors in fragment order (for x.cap vectors)
  DevBuf<float> mseg;                        // [nseg][vectors of a statistics launch]; useg shares its capacity (slots)
  DevBuf<unsigned long long> useg;
  DevBuf<float> g;                           // bytes: the gradient's dense scratch, at most kXentScratch
  DevBuf<void> bscratch;                     // bytes: the back-projection's own scratch
};
// device staging of one form of the top-k selection: buffers of their own.  What a caller fills or reads (x, cand, vals, pos)
// moves only when that buffer itself grows; the rest follows the call.
struct TopkStaging {
  DevBuf<float> x;                           // [cap][dim]
  DevBuf<long long> cand, clean;             // [cap], one capacity: the caller's candidates; ids >= rows made padding
  DevBuf<float> vals;                        // cap = max_n * max_k values reserved; a call's results are dense [n][k]
  DevBuf<long long> pos;                     // shares the capacity of vals
  DevBuf<void> operands;                     // bytes: the vectors in fragment order (for x.cap vectors)
  DevBuf<void> umax, list, head;             // bytes, for one range of vectors: [.][units] maxima, [.][64 k] keys, [2][.] threshold and count
};
struct Pending { hipEvent_t a, b; };
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
  TopkStaging tuser, thost;
  std::vector<Pending> pending;
  double kernel_ms = 0, bytes = 0;
  int64_t launches = 0;
};

namespace {
void embed_release(w2b_embed *e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  for (Pending &p : e->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  if (e->T) (void)hipFree(e->T);
  if (e->bad) (void)hipFree(e->bad);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;                                  // (every DevBuf of the staging frees itself)
}
struct EmbedRelease { void operator()(w2b_embed *e) const { embed_release(e); } };
using EmbedPtr = std::unique_ptr<w2b_embed, EmbedRelease>;

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

// Have at least `want` units, `bytes` bytes, in b.  Nothing happens when b is that large already: no call that grows nothing
// waits for the stream, and a buffer only moves when it grows itself.  A failed allocation leaves b empty.
template <class T>
int reserve(w2b_embed *e, DevBuf<T> &b, int64_t want, int64_t bytes) {
  if (want <= b.cap && b.p) return W2B_OK;
  EHIP(hipStreamSynchronize(e->stream));          // nothing in flight may still use the old buffer
  b.reset();
  void *q = nullptr;
  if (hipMalloc(&q, (size_t)(bytes > 0 ? bytes : 8)) != hipSuccess)
    return efail(W2B_ENOMEM, "w2b_embed: device allocation failed");
  b.p = (T *)q;
  b.cap = want;
  return W2B_OK;
}

// A scratch of `bytes` bytes that follows the call: as reserve(), but a call that needs no scratch allocates none.
int reserve_scratch(w2b_embed *e, DevBuf<void> &b, int64_t bytes) { return bytes > 0 ? reserve(e, b, bytes, bytes) : W2B_OK; }

// Buffers that share one capacity: when one of them could not grow (rc), none of them stays reserved, so the *_device calls
// that check the first of them refuse.
template <class... B>
int all_or_none(int rc, B &...b) {
  if (rc) (b.reset(), ...);
  return rc;
}

// buffers for max_ids ids, max_bags bags (< 0: none) and out_bytes of output; only ever grows
int ensure(w2b_embed *e, Staging &s, int64_t max_ids, int64_t max_bags, int64_t out_bytes) {
  if (int rc = reserve(e, s.ids, max_ids, max_ids * 8)) return rc;
  if (max_bags >= 0)
    if (int rc = reserve(e, s.offsets, max_bags, (max_bags + 1) * 8)) return rc;
  out_bytes = (out_bytes + 15) / 16 * 16;
  if (int rc = reserve(e, s.out, out_bytes, out_bytes)) return rc;
  if (s.offsets.cap > 0) {
    int cap = 0;
    if (int rc = reserve_scratch(e, s.scratch, w2b_embed_bag_scratch(s.ids.cap, s.offsets.cap, (int)e->dim, &cap))) return rc;
  }
  return W2B_OK;
}

// the weights buffer for max_ids ids, and the scratch of a weighted launch of n_ids ids in n_bags bags; only ever grow
int ensure_weighted(w2b_embed *e, Staging &s, int64_t max_ids, int64_t n_ids, int64_t n_bags) {
  if (int rc = reserve(e, s.weights, max_ids, max_ids * 4)) return rc;
  if (n_bags > 0) {
    int cap = 0;
    long long segcap = 0, head = 0;
    if (int rc = reserve_scratch(e, s.wscratch, w2b_embed_bagw_scratch(n_ids, n_bags, (int)e->dim, &cap, &segcap, &head))) return rc;
  }
  return W2B_OK;
}

// the projection's buffers for max_n vectors, max_m candidates and out_bytes of output; only ever grow, each on its own
int ensure_project(w2b_embed *e, ProjStaging &s, int64_t max_n, int64_t max_m, int64_t out_bytes) {
  if (int rc = reserve(e, s.x, max_n, max_n * e->dim * 4)) return rc;
  const int64_t need = (int64_t)w2b_embed_project_operand_bytes((int)e->dim, s.x.cap);
  if (int rc = reserve(e, s.operands, need, need)) return rc;
  if (int rc = reserve(e, s.cand, max_m, max_m * 8)) return rc;
  out_bytes = (out_bytes + 15) / 16 * 16;
  return reserve(e, s.out, out_bytes, out_bytes);
}

// the back-projection's buffers for max_n vectors and max_m candidates (g holds max_n * max_m values); only ever grow, each
// on its own
int ensure_back(w2b_embed *e, BackStaging &s, int64_t max_n, int64_t max_m) {
  if (int rc = reserve(e, s.g, max_n * max_m, max_n * max_m * 4)) return rc;
  if (int rc = reserve(e, s.cand, max_m, max_m * 8)) return rc;
  return reserve(e, s.dx, max_n, max_n * e->dim * 4);
}

// the cross-entropy's caller-facing buffers for max_n vectors and max_m candidates; only ever grow, each on its own
int ensure_xent(w2b_embed *e, XentStaging &s, int64_t max_n, int64_t max_m) {
  int rc = reserve(e, s.x, max_n, max_n * e->dim * 4);
  if (!rc) rc = reserve(e, s.target, max_n, max_n * 8);
  if (!rc) rc = reserve(e, s.teff, max_n, max_n * 8);
  if (!rc) rc = reserve(e, s.stats, max_n, max_n * 12);
  if (!rc) rc = reserve(e, s.dx, max_n, max_n * e->dim * 4);
  if (all_or_none(rc, s.x, s.target, s.teff, s.stats, s.dx)) return rc;
  const int64_t need = (int64_t)w2b_embed_project_operand_bytes((int)e->dim, s.x.cap);
  if ((rc = reserve(e, s.operands, need, need))) return rc;
  rc = reserve(e, s.cand, max_m, max_m * 8);
  if (!rc) rc = reserve(e, s.clean, max_m, max_m * 8);
  return all_or_none(rc, s.cand, s.clean);
}

// the top-k selection's caller-facing buffers for max_n vectors, max_m candidates and max_n * max_k results; only ever grow,
// each on its own
int ensure_topk(w2b_embed *e, TopkStaging &s, int64_t max_n, int64_t max_m, int64_t max_k) {
  int rc = reserve(e, s.x, max_n, max_n * e->dim * 4);
  if (rc) return rc;
  const int64_t need = (int64_t)w2b_embed_project_operand_bytes((int)e->dim, s.x.cap);
  if ((rc = reserve(e, s.operands, need, need))) return rc;
  rc = reserve(e, s.cand, max_m, max_m * 8);
  if (!rc) rc = reserve(e, s.clean, max_m, max_m * 8);
  if (all_or_none(rc, s.cand, s.clean)) return rc;
  rc = reserve(e, s.vals, max_n * max_k, max_n * max_k * 4);
  if (!rc) rc = reserve(e, s.pos, max_n * max_k, max_n * max_k * 8);
  return all_or_none(rc, s.vals, s.pos);
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
    return w2b_launch_embed_lookup(e->T, e->rows, (int)e->dim, e->bitlevel, s.ids.p, n, dtype, s.out.p, e->bad, e->stream);
  });
}

int launch_bag(w2b_embed *e, Staging &s, int64_t n_ids, int64_t n_bags, int32_t mode, int32_t dtype) {
  const double bytes = (double)n_ids * (double)e->wpr * 8 + (double)n_bags * (double)e->dim * elem_size(dtype);
  return timed(e, bytes, [&] {
    return w2b_launch_embed_bag(e->T, e->rows, (int)e->dim, e->bitlevel, s.ids.p, n_ids, s.offsets.p, n_bags, mode, dtype, s.out.p,
                                e->bad, s.scratch.p, e->stream);
  });
}

int launch_bag_weighted(w2b_embed *e, Staging &s, int64_t n_ids, int64_t n_bags, int32_t mode, int32_t dtype) {
  const double bytes = (double)n_ids * ((double)e->wpr * 8 + 4) + (double)n_bags * (double)e->dim * elem_size(dtype);
  return timed(e, bytes, [&] {
    return w2b_launch_embed_bag_weighted(e->T, e->rows, (int)e->dim, e->bitlevel, s.ids.p, s.weights.p, n_ids, s.offsets.p, n_bags,
                                         mode, dtype, s.out.p, e->bad, s.wscratch.p, e->stream);
  });
}

// n vectors against m candidates: those of s.cand, or the rows cand_base .. cand_base + m when !use_cand
int launch_project(w2b_embed *e, ProjStaging &s, int64_t n, int64_t m, bool use_cand, int64_t cand_base, int32_t dtype) {
  const double bytes = (double)n * (double)e->dim * 4 + (double)m * (double)e->wpr * 8 + (use_cand ? (double)m * 8 : 0.0) +
                       (double)n * (double)m * elem_size(dtype);
  return timed(e, bytes, [&] {
    return w2b_launch_embed_project(e->T, e->rows, (int)e->dim, e->bitlevel, s.x.p, (int)n, use_cand ? s.cand.p : nullptr, cand_base,
                                    (int)m, dtype, s.operands.p, s.out.p, e->bad, e->stream);
  });
}

// n vectors of s.g (dense, m apart) against m candidate positions that begin a segment: those of s.cand, or the rows
// cand_base .. cand_base + m when !use_cand.  The scratch follows the call (it waits for the stream only when it has to grow).
int launch_backproject(w2b_embed *e, BackStaging &s, int64_t n, int64_t m, bool use_cand, int64_t cand_base, bool first,
                       bool last) {
  int use_scratch = 0, segs = 1;
  long long need = 0;
  w2b_embed_backproject_plan((int)e->dim, n, m, &use_scratch, &segs, &need);
  if (int rc = reserve_scratch(e, s.scratch, need)) return rc;
  const double bytes = (double)n * (double)m * 4 + (double)m * (double)e->wpr * 8 + (use_cand ? (double)m * 8 : 0.0) +
                       (double)n * (double)e->dim * 4;
  return timed(e, bytes, [&] {
    return w2b_launch_embed_backproject(e->T, e->rows, (int)e->dim, e->bitlevel, s.g.p, m, n, use_cand ? s.cand.p : nullptr,
                                        cand_base, (int)m, first, last, s.dx.p, use_scratch, segs, s.scratch.p, e->bad, e->stream);
  });
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
  float *mx = s.stats.p, *se = s.stats.p + n, *tl = s.stats.p + 2 * n;
  const long long *clean = use_cand ? s.clean.p : nullptr;
  const double cand_bytes = use_cand ? (double)m * 8 : 0.0, row_bytes = (double)m * (double)e->wpr * 8;
  // statistics: ranges of vectors, multiples of 64 (the pairs of the operand staging)
  int64_t sv = nseg > 0 ? kXentScratch / 12 / nseg / 64 * 64 : n;
  sv = sv < 64 ? 64 : sv;
  if (sv > n) sv = n;
  const int64_t slots = sv * nseg > 0 ? sv * nseg : 1;
  int rc = reserve(e, s.mseg, slots, slots * 4);
  if (!rc) rc = reserve(e, s.useg, slots, slots * 8);
  if (all_or_none(rc, s.mseg, s.useg)) return rc;
  const double bytes = (double)n * dim * 4 + row_bytes + cand_bytes + (double)n * 8 + (double)n * 12;
  rc = timed(e, bytes, [&] {
    hipError_t he = w2b_launch_vec_operands(s.x.p, dim, (int)n, s.operands.p, e->stream);
    if (he == hipSuccess && use_cand) he = w2b_launch_embed_xent_clean(s.cand.p, m, e->rows, s.clean.p, e->bad, e->stream);
    for (int64_t v0 = 0; v0 < n && he == hipSuccess; v0 += sv) {
      const int64_t v1 = v0 + sv < n ? v0 + sv : n;
      he = w2b_launch_embed_xent_stats(e->T, e->rows, dim, e->bitlevel, s.operands.p, (int)v0, (int)v1, clean, (int)m, s.target.p,
                                       s.mseg.p, s.useg.p, tl, e->stream);
      if (he == hipSuccess)
        he = w2b_launch_embed_xent_finish((int)v0, (int)v1, m, (int)nseg, s.mseg.p, s.useg.p, clean, s.target.p, mx, se, tl,
                                          s.teff.p, e->bad, e->stream);
    }
    return he;
  });
  if (rc || !want_dx) return rc;
  if (m == 0) {                                            // an empty sum: +0.0 rows, no launch
    EHIP(hipMemsetAsync(s.dx.p, 0, (size_t)(n * e->dim) * 4, e->stream));
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
  if ((rc = reserve(e, s.g, gv * cm * 4, gv * cm * 4))) return rc;
  for (int64_t v0 = 0; v0 < n; v0 += gv) {
    const int64_t nv = n - v0 < gv ? n - v0 : gv;
    for (int64_t j0 = 0; j0 < m; j0 += cm) {
      const int64_t cj = m - j0 < cm ? m - j0 : cm;
      int use_scratch = 0, segs = 1;
      long long need = 0;
      w2b_embed_backproject_plan(dim, nv, cj, &use_scratch, &segs, &need);
      if ((rc = reserve_scratch(e, s.bscratch, need))) return rc;
      const double cb = use_cand ? (double)cj * 8 : 0.0;
      const double gbytes = 2.0 * (double)nv * dim * 4 + 2.0 * ((double)cj * (double)e->wpr * 8 + cb) + 2.0 * (double)nv * (double)cj * 4;
      rc = timed(e, gbytes, [&] {
        hipError_t he = w2b_launch_embed_xent_grad(e->T, e->rows, dim, e->bitlevel, s.operands.p, (int)v0, (int)(v0 + nv), clean, j0,
                                                   (int)cj, mx, se, s.teff.p, s.g.p, e->stream);
        if (he == hipSuccess)
          he = w2b_launch_embed_backproject(e->T, e->rows, dim, e->bitlevel, s.g.p, cj, nv, clean ? clean + j0 : nullptr, j0, (int)cj,
                                            j0 == 0, j0 + cj == m, s.dx.p + v0 * e->dim, use_scratch, segs, s.bscratch.p, e->bad,
                                            e->stream);
        return he;
      });
      if (rc) return rc;
    }
  }
  return W2B_OK;
}

// the bytes of unit maxima and key lists a range of vectors may use: kTopkScratch, or less by W2B_EMBED_TOPK_SCRATCH (bytes,
// read per call; for tests of the ranges of vectors at small shapes)
int64_t topk_scratch_bytes() {
  int64_t b = kTopkScratch;
  if (const char *env = getenv("W2B_EMBED_TOPK_SCRATCH")) {
    const long long v = atoll(env);
    if (v > 0 && v < b) b = v;
  }
  return b;
}

// The whole call on the staging s: n vectors of s.x against m candidates (those of s.cand, or every row); the k best of every
// vector into s.vals / s.pos = [n][k].  Ranges of vectors, multiples of 64 (the pairs of the operand staging), whose unit maxima
// and key lists stay within the scratch -- or one pair, if that needs more: per range the four kernels of
// w2b_kernels_embedtopk.hip, each K loop over all m candidates.
int launch_topk(w2b_embed *e, TopkStaging &s, int64_t n, int64_t m, bool use_cand, int64_t k) {
  const int dim = (int)e->dim;
  const int64_t nunits = (m + W2B_TOPK_UNIT - 1) / W2B_TOPK_UNIT, per_vector = nunits * 8 + W2B_TOPK_UNIT * k * 8 + 16;
  int64_t sv = topk_scratch_bytes() / per_vector / 64 * 64;
  sv = sv < 64 ? 64 : sv;
  if (sv > n) sv = n;
  if (int rc = reserve_scratch(e, s.umax, sv * nunits * 8)) return rc;
  if (int rc = reserve_scratch(e, s.list, sv * W2B_TOPK_UNIT * k * 8)) return rc;
  if (int rc = reserve_scratch(e, s.head, sv * 16)) return rc;
  const long long *clean = use_cand ? s.clean.p : nullptr;
  unsigned long long *thr = (unsigned long long *)s.head.p;
  unsigned int *count = (unsigned int *)(thr + sv);
  for (int64_t v0 = 0; v0 < n; v0 += sv) {
    const int64_t v1 = v0 + sv < n ? v0 + sv : n, nv = v1 - v0;
    const double bytes = 2.0 * ((double)nv * dim * 4 + (double)m * (double)e->wpr * 8 + (use_cand ? (double)m * 8 : 0.0)) + (double)nv * (double)k * 12;
    int rc = timed(e, bytes, [&] {
      hipError_t he = hipSuccess;
      if (v0 == 0) {                                       // once per call: the operands, the cleaned candidates
        he = w2b_launch_vec_operands(s.x.p, dim, (int)n, s.operands.p, e->stream);
        if (he == hipSuccess && use_cand) he = w2b_launch_embed_xent_clean(s.cand.p, m, e->rows, s.clean.p, e->bad, e->stream);
      }
      if (he == hipSuccess)
        he = w2b_launch_embed_topk(e->T, e->rows, dim, e->bitlevel, s.operands.p, (int)v0, (int)v1, clean, (int)m, (int)k,
                                   (unsigned long long *)s.umax.p, thr, count, (unsigned long long *)s.list.p, s.vals.p, s.pos.p,
                                   e->stream);
      return he;
    });
    if (rc) return rc;
  }
  return W2B_OK;
}

// The host form of both bag calls (`weighted` says which: the weights of a call without ids may be NULL).  Chunks of whole
// bags b0 .. b1 - 1: at least one, then while they fit the staging; a weighted call stages its weights beside the ids.
int bag_host_form(w2b_embed *e, const char *who, bool weighted, int64_t n_ids, const int32_t *ids, const float *weights,
                  int64_t n_bags, const int64_t *offsets, int32_t mode, int32_t dtype, void *out) {
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (int rc = check_dtype(who, dtype)) return rc;
  if (int rc = check_ids(who, e->rows, n_ids, ids)) return rc;
  if (int rc = check_bags(who, n_ids, n_bags, offsets, mode)) return rc;
  if (weighted)
    if (int rc = check_weights(who, n_ids, ids, weights)) return rc;
  if (n_bags == 0) return W2B_OK;
  if (!out) return refuse(W2B_EINVAL, who, "null output");
  EHIP(hipSetDevice(e->device));
  Staging &s = e->host;
  const int64_t row_bytes = e->dim * elem_size(dtype);
  int64_t max_bags = kHostOutBytes / row_bytes;
  if (max_bags < 1) max_bags = 1;
  std::vector<long long> wide, off;
  for (int64_t b0 = 0; b0 < n_bags;) {
    int64_t b1 = b0 + 1;
    while (b1 < n_bags && b1 - b0 < max_bags && offsets[b1 + 1] - offsets[b0] <= kHostIds) b1++;
    const int64_t i0 = offsets[b0], ci = offsets[b1] - i0, cb = b1 - b0;
    if (int rc = ensure(e, s, ci > 0 ? ci : 1, cb, cb * row_bytes)) return rc;
    if (weighted)
      if (int rc = ensure_weighted(e, s, s.ids.cap, ci, cb)) return rc;
    wide.assign(ids + i0, ids + i0 + ci);
    off.resize((size_t)cb + 1);
    for (int64_t b = 0; b <= cb; b++) off[(size_t)b] = offsets[b0 + b] - i0;
    if (ci > 0) {
      EHIP(hipMemcpyAsync(s.ids.p, wide.data(), (size_t)ci * 8, hipMemcpyHostToDevice, e->stream));
      if (weighted) EHIP(hipMemcpyAsync(s.weights.p, weights + i0, (size_t)ci * 4, hipMemcpyHostToDevice, e->stream));
    }
    EHIP(hipMemcpyAsync(s.offsets.p, off.data(), (size_t)(cb + 1) * 8, hipMemcpyHostToDevice, e->stream));
    if (int rc = weighted ? launch_bag_weighted(e, s, ci, cb, mode, dtype) : launch_bag(e, s, ci, cb, mode, dtype)) return rc;
    EHIP(hipMemcpyAsync((char *)out + b0 * row_bytes, s.out.p, (size_t)(cb * row_bytes), hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    b0 = b1;
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
  if (int rc = check_shape("w2b_embed_load", e->rows, dim, bitlevel, 1)) return rc;
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
  if (int rc = check_shape("w2b_embed_create", rows, dim, bitlevel, 1)) return rc;
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
  const char *who = "w2b_embed_lookup";
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (int rc = check_dtype(who, dtype)) return rc;
  if (int rc = check_ids(who, e->rows, n, ids)) return rc;
  if (n == 0) return W2B_OK;
  if (!out) return refuse(W2B_EINVAL, who, "null output");
  EHIP(hipSetDevice(e->device));
  const int64_t row_bytes = e->dim * elem_size(dtype);
  int64_t chunk = kHostOutBytes / row_bytes;
  chunk = chunk < 1 ? 1 : (chunk > kHostIds ? kHostIds : chunk);
  std::vector<long long> wide;
  for (int64_t i0 = 0; i0 < n; i0 += chunk) {
    const int64_t c = n - i0 < chunk ? n - i0 : chunk;
    if (int rc = ensure(e, e->host, c, -1, c * row_bytes)) return rc;
    wide.assign(ids + i0, ids + i0 + c);
    EHIP(hipMemcpyAsync(e->host.ids.p, wide.data(), (size_t)c * 8, hipMemcpyHostToDevice, e->stream));
    if (int rc = launch_lookup(e, e->host, c, dtype)) return rc;
    EHIP(hipMemcpyAsync((char *)out + i0 * row_bytes, e->host.out.p, (size_t)(c * row_bytes), hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
  }
  return W2B_OK;
}

extern "C" int w2b_embed_bag(w2b_embed *e, int64_t n_ids, const int32_t *ids, int64_t n_bags, const int64_t *offsets,
                             int32_t mode, int32_t dtype, void *out) {
  return bag_host_form(e, "w2b_embed_bag", false, n_ids, ids, nullptr, n_bags, offsets, mode, dtype, out);
}

extern "C" int w2b_embed_bag_weighted(w2b_embed *e, int64_t n_ids, const int32_t *ids, const float *weights, int64_t n_bags,
                                      const int64_t *offsets, int32_t mode, int32_t dtype, void *out) {
  return bag_host_form(e, "w2b_embed_bag_weighted", true, n_ids, ids, weights, n_bags, offsets, mode, dtype, out);
}

extern "C" int w2b_embed_project(w2b_embed *e, int64_t n, const float *x, int64_t m, const int32_t *cand, int32_t dtype,
                                 void *out) {
  const char *who = "w2b_embed_project";
  if (int rc = project_check_args(who, n, x, m, dtype, out)) return rc;
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (int rc = project_check_cand(who, e->rows, m, cand)) return rc;
  if (int rc = project_check_values(who, n, e->dim, x)) return rc;
  if (n == 0 || m == 0) return W2B_OK;
  EHIP(hipSetDevice(e->device));
  // whole vectors x whole candidate ranges, about kHostOutBytes of output per launch
  const int es = elem_size(dtype);
  const int64_t nv = n < 4096 ? n : 4096;
  int64_t cm = kHostOutBytes / (es * nv);
  if (cm > kHostIds) cm = kHostIds;
  if (cm >= 64) cm = cm / 64 * 64;
  cm = cm < 1 ? 1 : (cm > m ? m : cm);
  ProjStaging &s = e->phost;
  std::vector<long long> wide;
  std::vector<char> part;
  for (int64_t i0 = 0; i0 < n; i0 += nv) {
    const int64_t ci = n - i0 < nv ? n - i0 : nv;
    if (int rc = ensure_project(e, s, nv, cm, nv * cm * es)) return rc;
    EHIP(hipMemcpyAsync(s.x.p, x + i0 * e->dim, (size_t)(ci * e->dim) * 4, hipMemcpyHostToDevice, e->stream));
    for (int64_t j0 = 0; j0 < m; j0 += cm) {
      const int64_t cj = m - j0 < cm ? m - j0 : cm;
      if (cand) {
        wide.assign(cand + j0, cand + j0 + cj);
        EHIP(hipMemcpyAsync(s.cand.p, wide.data(), (size_t)cj * 8, hipMemcpyHostToDevice, e->stream));
      }
      if (int rc = launch_project(e, s, ci, cj, cand != nullptr, j0, dtype)) return rc;
      if (cj == m) {                                       // the chunk's rows are the caller's rows
        EHIP(hipMemcpyAsync((char *)out + i0 * m * es, s.out.p, (size_t)(ci * m * es), hipMemcpyDeviceToHost, e->stream));
        EHIP(hipStreamSynchronize(e->stream));
      } else {                                             // a range of columns: through host memory, row by row
        part.resize((size_t)(ci * cj * es));
        EHIP(hipMemcpyAsync(part.data(), s.out.p, part.size(), hipMemcpyDeviceToHost, e->stream));
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
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
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
  BackStaging &s = e->bhost;
  std::vector<long long> wide;
  for (int64_t i0 = 0; i0 < n; i0 += nv) {
    const int64_t ci = n - i0 < nv ? n - i0 : nv;
    if (int rc = ensure_back(e, s, nv, cm)) return rc;
    for (int64_t j0 = 0; j0 < m; j0 += cm) {
      const int64_t cj = m - j0 < cm ? m - j0 : cm;
      if (cand) {
        wide.assign(cand + j0, cand + j0 + cj);
        EHIP(hipMemcpyAsync(s.cand.p, wide.data(), (size_t)cj * 8, hipMemcpyHostToDevice, e->stream));
      }
      EHIP(hipMemcpy2DAsync(s.g.p, (size_t)cj * 4, g + i0 * m + j0, (size_t)m * 4, (size_t)cj * 4, (size_t)ci,
                            hipMemcpyHostToDevice, e->stream));
      if (int rc = launch_backproject(e, s, ci, cj, cand != nullptr, j0, j0 == 0, j0 + cj == m)) return rc;
      EHIP(hipStreamSynchronize(e->stream));               // (wide and the staging are written again for the next range)
    }
    EHIP(hipMemcpyAsync(dx + i0 * e->dim, s.dx.p, (size_t)(ci * e->dim) * 4, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
  }
  return W2B_OK;
}

extern "C" int w2b_embed_xent(w2b_embed *e, int64_t n, const float *x, int64_t m, const int32_t *cand, const int32_t *target,
                              float *mx, float *se, float *tl, float *dx) {
  const char *who = "w2b_embed_xent";
  if (int rc = xent_check_args(who, n, x, m, target, mx, se, tl)) return rc;
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (int rc = project_check_cand(who, e->rows, m, cand)) return rc;
  if (int rc = xent_check_targets(who, n, m, cand, target)) return rc;
  if (int rc = project_check_values(who, n, e->dim, x)) return rc;
  if (n == 0) return W2B_OK;
  EHIP(hipSetDevice(e->device));
  // ranges of whole vectors (they are independent); the candidate list is staged whole, 16 bytes per candidate
  const int64_t nv = n < 4096 ? n : 4096;
  XentStaging &s = e->xhost;
  if (int rc = ensure_xent(e, s, nv, m > 0 ? m : 1)) return rc;
  std::vector<long long> wide;
  if (cand && m > 0) {
    wide.assign(cand, cand + m);
    EHIP(hipMemcpyAsync(s.cand.p, wide.data(), (size_t)m * 8, hipMemcpyHostToDevice, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
  }
  for (int64_t i0 = 0; i0 < n; i0 += nv) {
    const int64_t ci = n - i0 < nv ? n - i0 : nv;
    wide.assign(target + i0, target + i0 + ci);
    EHIP(hipMemcpyAsync(s.x.p, x + i0 * e->dim, (size_t)(ci * e->dim) * 4, hipMemcpyHostToDevice, e->stream));
    EHIP(hipMemcpyAsync(s.target.p, wide.data(), (size_t)ci * 8, hipMemcpyHostToDevice, e->stream));
    if (int rc = launch_xent(e, s, ci, m, cand != nullptr, dx != nullptr)) return rc;
    EHIP(hipMemcpyAsync(mx + i0, s.stats.p, (size_t)ci * 4, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipMemcpyAsync(se + i0, s.stats.p + ci, (size_t)ci * 4, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipMemcpyAsync(tl + i0, s.stats.p + 2 * ci, (size_t)ci * 4, hipMemcpyDeviceToHost, e->stream));
    if (dx) EHIP(hipMemcpyAsync(dx + i0 * e->dim, s.dx.p, (size_t)(ci * e->dim) * 4, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
  }
  return W2B_OK;
}

extern "C" int w2b_embed_topk(w2b_embed *e, int64_t n, const float *x, int64_t m, const int32_t *cand, int32_t k, float *vals,
                              int32_t *pos) {
  const char *who = "w2b_embed_topk";
  if (int rc = topk_check_args(who, n, x, m, k, vals, pos)) return rc;
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (int rc = project_check_cand(who, e->rows, m, cand)) return rc;
  if (int rc = project_check_values(who, n, e->dim, x)) return rc;
  if (n == 0) return W2B_OK;
  EHIP(hipSetDevice(e->device));
  // ranges of whole vectors (they are independent); the candidate list is staged whole, 16 bytes per candidate
  const int64_t nv = n < 4096 ? n : 4096;
  TopkStaging &s = e->thost;
  if (int rc = ensure_topk(e, s, nv, m > 0 ? m : 1, k)) return rc;
  std::vector<long long> wide;
  if (cand && m > 0) {
    wide.assign(cand, cand + m);
    EHIP(hipMemcpyAsync(s.cand.p, wide.data(), (size_t)m * 8, hipMemcpyHostToDevice, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
  }
  wide.resize((size_t)(nv * k));
  for (int64_t i0 = 0; i0 < n; i0 += nv) {
    const int64_t ci = n - i0 < nv ? n - i0 : nv;
    EHIP(hipMemcpyAsync(s.x.p, x + i0 * e->dim, (size_t)(ci * e->dim) * 4, hipMemcpyHostToDevice, e->stream));
    if (int rc = launch_topk(e, s, ci, m, cand != nullptr, k)) return rc;
    EHIP(hipMemcpyAsync(vals + i0 * k, s.vals.p, (size_t)(ci * k) * 4, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipMemcpyAsync(wide.data(), s.pos.p, (size_t)(ci * k) * 8, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    for (int64_t c = 0; c < ci * k; c++) pos[i0 * k + c] = (int32_t)wide[(size_t)c];
  }
  return W2B_OK;
}

// ------------------------------------------------------------------------------------ device form
extern "C" int w2b_embed_reserve_topk(w2b_embed *e, int64_t max_n, int64_t max_m, int32_t max_k, void **x_dev, void **cand_dev,
                                      void **vals_dev, void **pos_dev) {
  const char *who = "w2b_embed_reserve_topk";
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (int rc = topk_check_k(who, max_k)) return rc;
  if (max_n < 0 || max_n > kProjectMaxVectors || max_m < 0 || max_m > 0x7FFFFF00ll || max_n * e->dim > (1ll << 40))
    return refuse(W2B_EINVAL, who, "bad sizes");
  EHIP(hipSetDevice(e->device));
  TopkStaging &s = e->tuser;
  if (int rc = ensure_topk(e, s, max_n, max_m, max_k)) return rc;
  if (x_dev) *x_dev = s.x.p;
  if (cand_dev) *cand_dev = s.cand.p;
  if (vals_dev) *vals_dev = s.vals.p;
  if (pos_dev) *pos_dev = s.pos.p;
  return W2B_OK;
}

extern "C" int w2b_embed_topk_device(w2b_embed *e, int64_t n, int64_t m, int32_t use_cand, int32_t k) {
  const char *who = "w2b_embed_topk_device";
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (n < 0 || m < 0) return refuse(W2B_EINVAL, who, "negative count");
  if (int rc = check_flag(who, "use_cand", use_cand)) return rc;
  if (int rc = topk_check_k(who, k)) return rc;
  if (n == 0) return W2B_OK;
  TopkStaging &s = e->tuser;
  if (!s.x.p || !s.cand.p || !s.vals.p || n > s.x.cap || m > s.cand.cap || n * k > s.vals.cap)
    return refuse(W2B_EINVAL, who, "more than w2b_embed_reserve_topk has set aside");
  if (!use_cand && m != e->rows) return refuse(W2B_EINVAL, who, "without candidates m must be rows");
  EHIP(hipSetDevice(e->device));
  return launch_topk(e, s, n, m, use_cand != 0, k);
}

extern "C" int w2b_embed_reserve_xent(w2b_embed *e, int64_t max_n, int64_t max_m, void **x_dev, void **cand_dev,
                                      void **target_dev, void **stats_dev, void **dx_dev) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_reserve_xent: null handle");
  if (max_n < 0 || max_n > kProjectMaxVectors || max_m < 0 || max_m > 0x7FFFFF00ll || max_n * e->dim > (1ll << 40))
    return efail(W2B_EINVAL, "w2b_embed_reserve_xent: bad sizes");
  EHIP(hipSetDevice(e->device));
  XentStaging &s = e->xuser;
  if (int rc = ensure_xent(e, s, max_n, max_m)) return rc;
  if (x_dev) *x_dev = s.x.p;
  if (cand_dev) *cand_dev = s.cand.p;
  if (target_dev) *target_dev = s.target.p;
  if (stats_dev) *stats_dev = s.stats.p;
  if (dx_dev) *dx_dev = s.dx.p;
  return W2B_OK;
}

extern "C" int w2b_embed_xent_device(w2b_embed *e, int64_t n, int64_t m, int32_t use_cand, int32_t want_dx) {
  const char *who = "w2b_embed_xent_device";
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (n < 0 || m < 0) return refuse(W2B_EINVAL, who, "negative count");
  if (int rc = check_flag(who, "use_cand", use_cand)) return rc;
  if (int rc = check_flag(who, "want_dx", want_dx)) return rc;
  if (n == 0) return W2B_OK;
  XentStaging &s = e->xuser;
  if (!s.x.p || !s.cand.p || n > s.x.cap || m > s.cand.cap) return refuse(W2B_EINVAL, who, "more than w2b_embed_reserve_xent has set aside");
  if (!use_cand && m != e->rows) return refuse(W2B_EINVAL, who, "without candidates m must be rows");
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
  BackStaging &s = e->buser;
  if (int rc = ensure_back(e, s, max_n, max_m)) return rc;
  if (g_dev) *g_dev = s.g.p;
  if (cand_dev) *cand_dev = s.cand.p;
  if (dx_dev) *dx_dev = s.dx.p;
  return W2B_OK;
}

extern "C" int w2b_embed_backproject_device(w2b_embed *e, int64_t n, int64_t m, int32_t use_cand) {
  const char *who = "w2b_embed_backproject_device";
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (n < 0 || m < 0) return refuse(W2B_EINVAL, who, "negative count");
  if (int rc = check_flag(who, "use_cand", use_cand)) return rc;
  if (n == 0) return W2B_OK;
  BackStaging &s = e->buser;
  if (!s.g.p || !s.cand.p || !s.dx.p || n > s.dx.cap || m > s.cand.cap || n * m > s.g.cap)
    return refuse(W2B_EINVAL, who, "more than w2b_embed_reserve_backproject has set aside");
  if (!use_cand && m != e->rows) return refuse(W2B_EINVAL, who, "without candidates m must be rows");
  EHIP(hipSetDevice(e->device));
  if (m == 0) {                                            // an empty sum: +0.0 rows, no launch
    EHIP(hipMemsetAsync(s.dx.p, 0, (size_t)(n * e->dim) * 4, e->stream));
    return W2B_OK;
  }
  return launch_backproject(e, s, n, m, use_cand != 0, 0, true, true);
}

extern "C" int w2b_embed_reserve_project(w2b_embed *e, int64_t max_n, int64_t max_m, int32_t dtype, void **x_dev,
                                         void **cand_dev, void **out_dev) {
  const char *who = "w2b_embed_reserve_project";
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (int rc = check_dtype(who, dtype)) return rc;
  if (max_n < 0 || max_n > kProjectMaxVectors || max_m < 0 || max_m > 0x7FFFFF00ll || max_n * max_m > (1ll << 40))
    return refuse(W2B_EINVAL, who, "bad sizes");
  EHIP(hipSetDevice(e->device));
  ProjStaging &s = e->puser;
  if (int rc = ensure_project(e, s, max_n, max_m, max_n * max_m * elem_size(dtype))) return rc;
  if (x_dev) *x_dev = s.x.p;
  if (cand_dev) *cand_dev = s.cand.p;
  if (out_dev) *out_dev = s.out.p;
  return W2B_OK;
}

extern "C" int w2b_embed_project_device(w2b_embed *e, int64_t n, int64_t m, int32_t use_cand, int32_t dtype) {
  const char *who = "w2b_embed_project_device";
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (int rc = check_dtype(who, dtype)) return rc;
  if (n < 0 || m < 0) return refuse(W2B_EINVAL, who, "negative count");
  if (int rc = check_flag(who, "use_cand", use_cand)) return rc;
  if (n == 0 || m == 0) return W2B_OK;
  ProjStaging &s = e->puser;
  if (!s.x.p || !s.cand.p || !s.out.p || n > s.x.cap || m > s.cand.cap || n * m * elem_size(dtype) > s.out.cap)
    return refuse(W2B_EINVAL, who, "more than w2b_embed_reserve_project has set aside");
  if (!use_cand && m != e->rows) return refuse(W2B_EINVAL, who, "without candidates m must be rows");
  EHIP(hipSetDevice(e->device));
  return launch_project(e, s, n, m, use_cand != 0, 0, dtype);
}

extern "C" int w2b_embed_reserve(w2b_embed *e, int64_t max_ids, int64_t max_bags, int32_t dtype, void **ids_dev,
                                 void **offsets_dev, void **out_dev) {
  const char *who = "w2b_embed_reserve";
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (int rc = check_dtype(who, dtype)) return rc;
  if (max_ids < 0 || max_bags < 0 || max_bags > 0x7FFFFF00ll || max_ids > (1ll << 40)) return refuse(W2B_EINVAL, who, "bad sizes");
  EHIP(hipSetDevice(e->device));
  const int64_t out_rows = max_ids > max_bags ? max_ids : max_bags;
  if (int rc = ensure(e, e->user, max_ids, max_bags, out_rows * e->dim * elem_size(dtype))) return rc;
  if (ids_dev) *ids_dev = e->user.ids.p;
  if (offsets_dev) *offsets_dev = e->user.offsets.p;
  if (out_dev) *out_dev = e->user.out.p;
  return W2B_OK;
}

extern "C" int w2b_embed_lookup_device(w2b_embed *e, int64_t n, int32_t dtype) {
  const char *who = "w2b_embed_lookup_device";
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (int rc = check_dtype(who, dtype)) return rc;
  if (n < 0) return refuse(W2B_EINVAL, who, "negative id count");
  if (n == 0) return W2B_OK;
  Staging &s = e->user;
  if (!s.ids.p || !s.out.p || n > s.ids.cap || n * e->dim * elem_size(dtype) > s.out.cap)
    return refuse(W2B_EINVAL, who, "more than w2b_embed_reserve has set aside");
  EHIP(hipSetDevice(e->device));
  return launch_lookup(e, s, n, dtype);
}

extern "C" int w2b_embed_bag_device(w2b_embed *e, int64_t n_ids, int64_t n_bags, int32_t mode, int32_t dtype) {
  const char *who = "w2b_embed_bag_device";
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (int rc = check_dtype(who, dtype)) return rc;
  if (int rc = check_mode(who, mode)) return rc;
  if (n_ids < 0 || n_bags < 0) return refuse(W2B_EINVAL, who, "negative count");
  if (n_bags == 0) return W2B_OK;
  Staging &s = e->user;
  if (!s.ids.p || !s.offsets.p || !s.out.p || !s.scratch.p || n_ids > s.ids.cap || n_bags > s.offsets.cap ||
      n_bags * e->dim * elem_size(dtype) > s.out.cap)
    return refuse(W2B_EINVAL, who, "more than w2b_embed_reserve has set aside");
  EHIP(hipSetDevice(e->device));
  return launch_bag(e, s, n_ids, n_bags, mode, dtype);
}

extern "C" int w2b_embed_reserve_weights(w2b_embed *e, int64_t max_ids, void **weights_dev) {
  if (!e) return efail(W2B_EINVAL, "w2b_embed_reserve_weights: null handle");
  if (max_ids < 0 || max_ids > (1ll << 40)) return efail(W2B_EINVAL, "w2b_embed_reserve_weights: bad size");
  EHIP(hipSetDevice(e->device));
  Staging &s = e->user;                                    // the scratch for what w2b_embed_reserve has set aside so far
  const int64_t ids = max_ids < s.ids.cap ? max_ids : s.ids.cap;
  if (int rc = ensure_weighted(e, s, max_ids, ids, s.offsets.cap)) return rc;
  if (weights_dev) *weights_dev = s.weights.p;
  return W2B_OK;
}

extern "C" int w2b_embed_bag_weighted_device(w2b_embed *e, int64_t n_ids, int64_t n_bags, int32_t mode, int32_t dtype) {
  const char *who = "w2b_embed_bag_weighted_device";
  if (!e) return refuse(W2B_EINVAL, who, "null handle");
  if (int rc = check_dtype(who, dtype)) return rc;
  if (int rc = check_mode(who, mode)) return rc;
  if (n_ids < 0 || n_bags < 0) return refuse(W2B_EINVAL, who, "negative count");
  if (n_bags == 0) return W2B_OK;
  Staging &s = e->user;
  if (!s.ids.p || !s.offsets.p || !s.out.p || n_ids > s.ids.cap || n_bags > s.offsets.cap ||
      n_bags * e->dim * elem_size(dtype) > s.out.cap)
    return refuse(W2B_EINVAL, who, "more than w2b_embed_reserve has set aside");
  if (!s.weights.p || n_ids > s.weights.cap) return refuse(W2B_EINVAL, who, "more than w2b_embed_reserve_weights has set aside");
  EHIP(hipSetDevice(e->device));
  // the scratch follows the call (it waits for the stream only when it has to grow); the weights buffer stays as it is
  if (int rc = ensure_weighted(e, s, s.weights.cap, n_ids, n_bags)) return rc;
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
