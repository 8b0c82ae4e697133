// w2b_trainer.cpp -- host side of the C ABI declared in include/word2bits_hip.h.
// Owns device memory, streams, events and the RCCL communicator; all arithmetic of the hot
// path lives in w2b_kernels.hip.  There is deliberately no CPU fallback in this file.
#include "../../include/word2bits_hip.h"
#include "../../include/word2bits_corpus.h"
#include "w2b_internal.h"
#include "w2b_plan.h"

#include <rccl/rccl.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
// shared with the other host translation units of the library (w2b_eval.cpp)
int w2b_internal_fail(int code, const char *msg) { return fail(code, msg ? msg : ""); }
#define HIPCHK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess)                                                                 \
      return fail(W2B_EHIP, std::string(#x) + ": " + hipGetErrorString(e_));              \
  } while (0)
#define NCCLCHK(x)                                                                        \
  do {                                                                                    \
    ncclResult_t r_ = (x);                                                                \
    if (r_ != ncclSuccess)                                                                \
      return fail(W2B_ERCCL, std::string(#x) + ": " + ncclGetErrorString(r_));            \
  } while (0)

struct w2b_trainer {
  W2bPlanInputs in;             // configuration, tuning knobs, compute units, word-count statistics: what the launch policy reads (w2b_plan.h)
  int device = 0;
  hipStream_t stream = nullptr;
  float *uv = nullptr;          // u followed by v (one allocation: one all-reduce)
  float *base = nullptr;        // snapshot for the delta-sum replica sync
  long long table_elems = 0;    // vocab_size * layer1_size
  float *exp_table = nullptr;
  int32_t *table = nullptr;
  long long table_size = 0;
  float *keep = nullptr;
  float *entry = nullptr;       // scratch rows of the sentence-resident kernel
  size_t entry_floats = 0;
  float *wide_scratch = nullptr;        // process_word_wide: [workgroups][2][dim]
  size_t wide_floats = 0;
  // XCD-shared copies of the hottest rows (XHot in w2b_device.hpp)
  float *xhot = nullptr;        // [W2B_NXCD]{copies [nu + nv][dim], entries [nu + nv][dim], merge locks [nu + nv][W2B_MAXW]}
  size_t xhot_floats = 0;
  float *rc = nullptr;          // row-group kernel: 64 ints of flags + refreshed per-XCD copies of the hottest context rows
  size_t rc_floats = 0;
  hipStream_t rc_stream = nullptr;   // the refresher kernel's stream
  hipEvent_t rc_go = nullptr, rc_end = nullptr;
  int xhot_nu = -1, xhot_nv = -1;       // layout the buffer currently has (-1: none)
  bool xhot_master_changed = true;      // the master rows may differ from what the copies were folded into
  bool debug = false;           // W2B_DEBUG was set when the trainer was created (diagnostics on stderr)
  const int32_t *corpus = nullptr;
  int32_t *corpus_owned = nullptr;
  long long n_tokens = 0;
  bool corpus_more = false;     // the tokens are a slice of the file and the file continues behind it
  W2bWorker *workers = nullptr;
  W2bShared *shared = nullptr;
  unsigned long long *jump_a = nullptr, *jump_c = nullptr;
  std::vector<long long> shard_start;
  std::vector<int> shard_override;
  bool shards_set = false;
  // staging for the host-pointer tuple form
  int32_t *st_center = nullptr, *st_off = nullptr, *st_ctx = nullptr, *st_neg = nullptr;
  size_t cap_center = 0, cap_off = 0, cap_ctx = 0, cap_neg = 0;
  // timing
  bool timing = false;
  std::vector<hipEvent_t> ev;    // pairs
  std::vector<hipEvent_t> ev_pool;
  // RCCL
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
  // non-blocking progress: after every launch the shared block is copied into a pinned ring slot behind an event
  static const int kPoll = 4;
  W2bShared *poll_host = nullptr;          // pinned [kPoll]
  hipEvent_t poll_ev[kPoll] = {nullptr, nullptr, nullptr, nullptr};
  long long launches = 0;                  // w2b_train_step calls since w2b_epoch_begin
  unsigned long long *wca_buf = nullptr;   // [2]: this replica's word_count_actual, the sum over all replicas
  // replica exchange (see "multi-GPU" below): two exchange streams, chunk staging buffers, events
  hipStream_t xs[2] = {nullptr, nullptr};
  float *xd[2] = {nullptr, nullptr}, *xsum[2] = {nullptr, nullptr};   // per slot: own delta / sum over the replicas
  struct XRange { long long off, len; };    // floats of [u || v]
  std::vector<XRange> x_ranges;             // the chunks of the exchange in progress (full: the whole model; hot tier: two prefixes)
  bool x_open = false;                      // the exchange in progress has begun and not ended
  long long x_words_full = 0;               // centre words since the previous exchange
  hipEvent_t x_evd[2] = {nullptr, nullptr}, x_evs[2] = {nullptr, nullptr}, x_evc = nullptr;   // delta / sum of a slot complete; counts summed
  float *xcnt = nullptr;                    // [2 * vocab_size]: replicas that changed each row, then the row's factor on the summed delta (mode 2)
  float *xrate = nullptr;                   // [2 * vocab_size]: expected updates of every row of [u || v] per trained centre word (from the word counts)
  std::vector<float> xrate_host;            // (host copy: empty = no word counts yet)
  bool x_fac_pending = false;               // xcnt holds contributor counts that k_xchg_factor has not yet turned into factors
  bool x_use_cnt = false;                   // the exchange in progress damps the saturated rows' sums by xcnt
  int x_sat_u = 0, x_sat_v = 0;             // rows 1..x_sat_* of u / v count as saturated in the exchange in progress
  long long x_words_sync = 0;               // x_words_full at the begin of the exchange in progress (the n of the combination rule)
  long long x_words = 0;                    // centre words this replica can have trained since the previous exchange (launches x
                                            // positions x workers: the same number on every replica of a symmetric job)
  long long xchunk = 0;                     // floats per chunk
  hipEvent_t x_train = nullptr;             // "the launches issued so far": the exchange streams wait for it
  hipEvent_t x_done[2] = {nullptr, nullptr};     // last operation of the latest exchange on each exchange stream
  bool x_any_done = false;                       // x_done[] have been recorded at least once
  bool x_pending = false;                   // the training stream has not yet waited for x_done
  std::vector<hipEvent_t> x_ev;             // (begin, end) pairs of the exchanges since the last w2b_sync_stats
  long long sync_count = 0;
  long long sync_bytes = 0;
};

// --------------------------------------------------------------------------------- host tables
extern "C" const char *w2b_version(void) { return "word2bits-hip 0.1 (gfx950)"; }
extern "C" const char *w2b_last_error(void) { return g_err.c_str(); }

extern "C" int w2b_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" int w2b_device_compute_units(int32_t device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return 0;
  return prop.multiProcessorCount;
}

// ref src/word2bits.cpp:614-618 -- float expf of the host libm, exactly as the reference builds it
extern "C" void w2b_build_exp_table(float *out) {
  for (int i = 0; i < W2B_EXP_TABLE_SIZE; i++) {
    const float arg = (i / (float)W2B_EXP_TABLE_SIZE * 2 - 1) * W2B_MAX_EXP;
    const float e = expf(arg);
    out[i] = e / (e + 1);
  }
}

// ref src/word2bits.cpp:112-128
extern "C" int w2b_build_unigram_table(const int64_t *cn, int64_t V, int32_t *table, int64_t tsz) {
  if (!cn || !table || V <= 0 || tsz <= 0) return fail(W2B_EINVAL, "w2b_build_unigram_table: bad argument");
  std::vector<double> w((size_t)V);
  double total = 0;
  for (int64_t a = 0; a < V; a++) {
    w[a] = pow((double)cn[a], 0.75);
    total += w[a];
  }
  int64_t i = 0;
  double edge = w[0] / total;
  for (int64_t a = 0; a < tsz; a++) {
    table[a] = (int32_t)i;
    if (a / (double)tsz > edge) {
      i++;
      if (i < V) edge += w[i] / total;
    }
    if (i >= V) i = V - 1;
  }
  return W2B_OK;
}

// ref src/word2bits.cpp:403-404
extern "C" void w2b_build_keep_prob(const int64_t *cn, int64_t V, float sample, int64_t train_words,
                                    float *out) {
  const float st = sample * train_words;
  for (int64_t i = 0; i < V; i++) out[i] = (sqrtf(cn[i] / st) + 1) * st / cn[i];
}

// ref src/word2bits.cpp:73-108 (host twin of the device quantizer; used by the save path of the CLI)
extern "C" float w2b_quantize(float x, int32_t bitlevel) {
  if (bitlevel == 0) return x;
  const float sgn = x < 0 ? -1.f : 1.f;
  if (bitlevel == 1) return sgn / 3;
  const float mag = x * sgn;
  float lvl = 0;
  if (bitlevel == 2) lvl = (mag >= 0 && mag <= .5f) ? .25f : .75f;
  if (bitlevel >= 4) {
    const int steps = 1 << (bitlevel - 1);
    const float scaled = mag * (float)steps;
    int k = (int)(scaled + .5f);
    if (k > steps) k = steps;
    lvl = k / (float)steps;
  }
  return sgn * lvl;
}

// --------------------------------------------------------------------------------- lifetime
// Everything a training launch passes to its kernel: the shape (w2b_shape_params), the trainer's device memory, the plan's numbers.
static W2bParams make_params(const w2b_trainer *t, const W2bLaunchPlan &lp) {
  W2bParams p{};
  w2b_shape_params(p, t->in.cfg, t->in.tune);
  p.u = t->uv;
  p.v = t->uv + t->table_elems;
  p.exp_table = t->exp_table;
  p.table = t->table;
  p.table_size = t->table_size;
  p.keep = (t->in.cfg.sample > 0) ? t->keep : nullptr;
  p.corpus = t->corpus;
  p.n_tokens = t->n_tokens;
  p.corpus_more = t->corpus_more ? 1 : 0;
  p.workers = t->workers;
  p.shared = t->shared;
  p.jump_a = t->jump_a;
  p.jump_c = t->jump_c;
  p.table_magic = t->table_size > 1 ? (unsigned long long)((((unsigned __int128)1) << 64) / (unsigned __int128)t->table_size) : 0;
  p.entry = t->entry;
  p.wide_scratch = t->wide_scratch;
  p.xhot = nullptr;                    // set by xhot_prepare() for the launch that uses the copies
  p.xhot_u = lp.copies_u;
  p.xhot_v = lp.copies_v;
  p.hot_period = lp.merge_period;
  p.xhot_m = lp.xhot_m;
  p.uavg_rank = lp.uavg_rank;
  p.atomic_rank = lp.atomic_rank_v;
  p.atomic_rank_u = lp.atomic_rank_u;
  p.fresh_rank_u = lp.fresh_rank_u;
  p.rc_rows = 0;                       // set by rc_prepare() for a launch of the row-group kernel
  p.rc = nullptr;
  p.rc_flags = nullptr;
  p.worker_base = 0;
  return p;
}

// Device buffer of at least `need` elements, grown on demand: the stream drains before the old buffer is freed (a launch in
// flight may still use it).  *grown is set when the buffer is a new one (its contents are undefined).
template <class T>
static int grow(w2b_trainer *t, T **buf, size_t *cap, size_t need, bool *grown = nullptr) {
  if (need <= *cap) return W2B_OK;
  HIPCHK(hipStreamSynchronize(t->stream));
  if (*buf) HIPCHK(hipFree(*buf));
  *buf = nullptr;
  *cap = 0;
  HIPCHK(hipMalloc(buf, sizeof(T) * need));
  *cap = need;
  if (grown) *grown = true;
  return W2B_OK;
}

extern "C" int w2b_trainer_create(const w2b_config *cfg, w2b_trainer **out) {
  if (!cfg || !out) return fail(W2B_EINVAL, "w2b_trainer_create: null argument");
  *out = nullptr;
  if (cfg->vocab_size < 2 || cfg->layer1_size < 1 || cfg->window < 1 || cfg->negative < 0 ||
      cfg->num_threads < 1 || cfg->bitlevel < 0 || cfg->bitlevel > 31 || cfg->iter < 0 ||
      cfg->worker_offset < 0 || cfg->total_threads < 0 ||
      (cfg->total_threads > 0 && cfg->worker_offset + cfg->num_threads > cfg->total_threads))
    return fail(W2B_EINVAL, "w2b_trainer_create: bad configuration value");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(W2B_ENOGPU, "no HIP device visible (this library has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(W2B_EINVAL, "device ordinal out of range");
  HIPCHK(hipSetDevice(cfg->device));
  w2b_trainer *t = new w2b_trainer();
  // every HIPCHK below returns on failure: the guard releases what was allocated so far
  struct Guard { w2b_trainer *t; ~Guard() { if (t) w2b_trainer_destroy(t); } } guard{t};
  t->in.cfg = *cfg;
  t->device = cfg->device;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
  t->in.num_cus = prop.multiProcessorCount;
  t->debug = getenv("W2B_DEBUG") != nullptr;
  t->in.tune = w2b_default_tuning();
  HIPCHK(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
  t->table_elems = (long long)cfg->vocab_size * cfg->layer1_size;
  HIPCHK(hipMalloc(&t->uv, sizeof(float) * 2 * t->table_elems));
  HIPCHK(hipMemsetAsync(t->uv, 0, sizeof(float) * 2 * t->table_elems, t->stream));
  HIPCHK(hipMalloc(&t->exp_table, sizeof(float) * (W2B_EXP_TABLE_SIZE + 8)));
  {
    std::vector<float> et(W2B_EXP_TABLE_SIZE + 8, 0.f);
    w2b_build_exp_table(et.data());
    HIPCHK(hipMemcpy(t->exp_table, et.data(), sizeof(float) * et.size(), hipMemcpyHostToDevice));
  }
  HIPCHK(hipMalloc(&t->shared, sizeof(W2bShared)));
  {
    W2bShared sh{};
    sh.alpha = cfg->alpha;
    HIPCHK(hipMemcpy(t->shared, &sh, sizeof sh, hipMemcpyHostToDevice));
  }
  HIPCHK(hipMalloc(&t->workers, sizeof(W2bWorker) * cfg->num_threads));
  HIPCHK(hipMemset(t->workers, 0, sizeof(W2bWorker) * cfg->num_threads));
  {
    // LCG jump-ahead table: x_{n+k} = A^k x_n + C (A^k - 1)/(A - 1)   (mod 2^64)
    const int nj = (cfg->negative + 2 > 66) ? cfg->negative + 2 : 66;
    std::vector<unsigned long long> ja(nj), jc(nj);
    ja[0] = 1;
    jc[0] = 0;
    for (int k = 1; k < nj; k++) {
      ja[k] = ja[k - 1] * W2B_LCG_A;
      jc[k] = jc[k - 1] * W2B_LCG_A + W2B_LCG_C;
    }
    HIPCHK(hipMalloc(&t->jump_a, sizeof(unsigned long long) * nj));
    HIPCHK(hipMalloc(&t->jump_c, sizeof(unsigned long long) * nj));
    HIPCHK(hipMemcpy(t->jump_a, ja.data(), sizeof(unsigned long long) * nj, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t->jump_c, jc.data(), sizeof(unsigned long long) * nj, hipMemcpyHostToDevice));
  }
  HIPCHK(hipStreamSynchronize(t->stream));
  guard.t = nullptr;
  *out = t;
  return W2B_OK;
}

static int xchg_fence(w2b_trainer *t);      // the training stream waits for a replica exchange in flight (below)
static void xchg_teardown(w2b_trainer *t);  // streams, events and buffers of the replica exchange

extern "C" void w2b_trainer_destroy(w2b_trainer *t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  if (t->stream) (void)hipStreamSynchronize(t->stream);
  if (t->debug && t->shared) {
    W2bShared sh;
    if (hipMemcpy(&sh, t->shared, sizeof sh, hipMemcpyDeviceToHost) == hipSuccess) {
      fprintf(stderr, "w2b debug: phase ticks (100 MHz wall clock) of workgroup 0:");
      for (int k = 0; k < 16; k++) fprintf(stderr, " [%d]=%llu", k, sh.dbg[k]);
      fprintf(stderr, "\n");
    }
  }
  if (t->rc_stream) { (void)hipStreamSynchronize(t->rc_stream); (void)hipStreamDestroy(t->rc_stream); }
  if (t->rc_go) (void)hipEventDestroy(t->rc_go);
  if (t->rc_end) (void)hipEventDestroy(t->rc_end);
  if (t->comm) ncclCommDestroy(t->comm);
  for (hipEvent_t e : t->ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : t->ev_pool) (void)hipEventDestroy(e);
  for (hipEvent_t e : t->poll_ev) if (e) (void)hipEventDestroy(e);
  if (t->poll_host) (void)hipHostFree(t->poll_host);
  for (hipStream_t q : t->xs) if (q) (void)hipStreamSynchronize(q);
  for (hipEvent_t e : t->x_ev) (void)hipEventDestroy(e);
  xchg_teardown(t);
  void *ptrs[] = {t->uv, t->wca_buf, t->exp_table, t->table, t->keep, t->entry, t->xhot, t->rc, t->wide_scratch, t->corpus_owned, t->workers, t->shared,
                  t->jump_a, t->jump_c, t->st_center, t->st_off, t->st_ctx, t->st_neg};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  if (t->stream) (void)hipStreamDestroy(t->stream);
  delete t;
}


// --------------------------------------------------------------------------------- tuning knobs
extern "C" int w2b_get_tuning(w2b_trainer *t, w2b_tuning *out) {
  if (!t || !out) return fail(W2B_EINVAL, "w2b_get_tuning: null argument");
  *out = t->in.tune;
  return W2B_OK;
}

extern "C" int w2b_set_tuning(w2b_trainer *t, const w2b_tuning *in) {
  if (!t || !in) return fail(W2B_EINVAL, "w2b_set_tuning: null argument");
  if (in->struct_size != (int32_t)sizeof(w2b_tuning))
    return fail(W2B_EINVAL, "w2b_set_tuning: struct_size does not match this library's w2b_tuning");
  if (in->hot_rows_v < -1 || in->hot_rows_v > W2B_XHOT_MAX || in->hot_rows_u < -1 || in->hot_rows_u > W2B_XHOT_MAX)
    return fail(W2B_EINVAL, "w2b_set_tuning: hot_rows_* must be -1 (automatic) or 0..128");
  if (in->hot_period < 0 || in->hot_period > 4096 || (in->hot_period & (in->hot_period - 1)) != 0)
    return fail(W2B_EINVAL, "w2b_set_tuning: hot_period must be 0 (automatic) or a power of two in 1..4096");
  if (in->hot_cap < 0 || in->hot_cap > W2B_XHOT_MAX) return fail(W2B_EINVAL, "w2b_set_tuning: hot_cap must be 0..128");
  if (in->grid_per_cu < 0 || in->grid_per_cu > 32) return fail(W2B_EINVAL, "w2b_set_tuning: grid_per_cu must be 0..32");
#ifdef W2B_EXPERIMENTAL_MEMMODES
  if (in->mem_mode < -1 || in->mem_mode > 3) return fail(W2B_EINVAL, "w2b_set_tuning: mem_mode must be -1..3");
#else
  if (in->mem_mode < -1 || in->mem_mode > 1) return fail(W2B_EINVAL, "w2b_set_tuning: mem_mode must be -1, 0 or 1");
#endif
  if (in->atomic_rank < -1 || in->atomic_cap < 0) return fail(W2B_EINVAL, "w2b_set_tuning: atomic_rank >= -1, atomic_cap >= 0");
  if (in->window_refresh < 0) return fail(W2B_EINVAL, "w2b_set_tuning: window_refresh must be >= 0");
  if (in->atomic_rank_u < -1) return fail(W2B_EINVAL, "w2b_set_tuning: atomic_rank_u >= -1");
  if (in->fresh_rank_u < -1) return fail(W2B_EINVAL, "w2b_set_tuning: fresh_rank_u >= -1");
  if (in->exchange_sat_updates < 0) return fail(W2B_EINVAL, "w2b_set_tuning: exchange_sat_updates >= 0");
  if (in->hot_weight_permille < 1 || in->hot_weight_permille > 1000)
    return fail(W2B_EINVAL, "w2b_set_tuning: hot_weight_permille must be 1..1000");
  if (in->refresh_rows_u < -1 || in->refresh_rows_u > W2B_RC_MAX) return fail(W2B_EINVAL, "w2b_set_tuning: refresh_rows_u must be -1 .. 64");
  if (in->exchange_rule < 0 || in->exchange_rule > 2 || in->exchange_tau_u < 0 || in->exchange_tau_v < 0 || in->concurrent_workers < 0)
    return fail(W2B_EINVAL, "w2b_set_tuning: exchange_rule must be 0, 1 or 2, exchange_tau_* >= 0, concurrent_workers >= 0");
  t->in.tune = *in;
  return W2B_OK;
}

#define NEED(t)                                                                  \
  do {                                                                           \
    if (!(t)) return fail(W2B_EINVAL, "null trainer");                          \
    HIPCHK(hipSetDevice((t)->device));                                           \
  } while (0)

// --------------------------------------------------------------------------------- model
extern "C" int w2b_init_net(w2b_trainer *t) {
  NEED(t);
  if (int rc = xchg_fence(t)) return rc;
  // ref :343-361: value_k = ((x_k & 0xFFFF) / 65536.f) - 0.5 with x_0 = 1; the low 16 bits have
  // period 65536, so a LUT indexed by the draw number modulo 65536 reproduces the sequence.
  std::vector<float> lut(65536);
  unsigned long long x = 1;
  for (int k = 0; k < 65536; k++) {
    x = x * W2B_LCG_A + W2B_LCG_C;
    lut[k] = (float)(((x & 0xFFFF) / (float)65536) - 0.5);
  }
  float *dl = nullptr;
  HIPCHK(hipMalloc(&dl, sizeof(float) * 65536));
  HIPCHK(hipMemcpyAsync(dl, lut.data(), sizeof(float) * 65536, hipMemcpyHostToDevice, t->stream));
  HIPCHK(w2b_launch_init_net(t->uv, t->uv + t->table_elems, t->table_elems, dl, t->stream));
  t->xhot_master_changed = true;
  if (t->base)
    HIPCHK(hipMemcpyAsync(t->base, t->uv, sizeof(float) * 2 * t->table_elems, hipMemcpyDeviceToDevice,
                          t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipFree(dl));
  return W2B_OK;
}

extern "C" int w2b_set_model(w2b_trainer *t, const float *u, const float *v) {
  NEED(t);
  if (!u || !v) return fail(W2B_EINVAL, "w2b_set_model: null table");
  if (int rc = xchg_fence(t)) return rc;
  const size_t bytes = sizeof(float) * t->table_elems;
  HIPCHK(hipMemcpyAsync(t->uv, u, bytes, hipMemcpyHostToDevice, t->stream));
  HIPCHK(hipMemcpyAsync(t->uv + t->table_elems, v, bytes, hipMemcpyHostToDevice, t->stream));
  t->xhot_master_changed = true;
  if (t->base) HIPCHK(hipMemcpyAsync(t->base, t->uv, 2 * bytes, hipMemcpyDeviceToDevice, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  return W2B_OK;
}

extern "C" int w2b_get_model(w2b_trainer *t, float *u, float *v) {
  NEED(t);
  const size_t bytes = sizeof(float) * t->table_elems;
  if (int rc = xchg_fence(t)) return rc;
  HIPCHK(hipStreamSynchronize(t->stream));
  if (u) HIPCHK(hipMemcpy(u, t->uv, bytes, hipMemcpyDeviceToHost));
  if (v) HIPCHK(hipMemcpy(v, t->uv + t->table_elems, bytes, hipMemcpyDeviceToHost));
  return W2B_OK;
}

extern "C" int w2b_model_device_ptrs(w2b_trainer *t, void **u_dev, void **v_dev) {
  NEED(t);
  if (int rc = xchg_fence(t)) return rc;
  HIPCHK(hipStreamSynchronize(t->stream));
  t->xhot_master_changed = true;           // the caller may write the tables (replica exchange on a view of them)
  if (u_dev) *u_dev = t->uv;
  if (v_dev) *v_dev = t->uv + t->table_elems;
  return W2B_OK;
}

void w2b_internal_trainer_view(w2b_trainer *t, float **u, float **v, long long *V, long long *D, int *bitlevel,
                               int *device, hipStream_t *stream) {
  (void)xchg_fence(t);
  *u = t->uv;
  *v = t->uv + t->table_elems;
  *V = t->in.cfg.vocab_size;
  *D = t->in.cfg.layer1_size;
  *bitlevel = t->in.cfg.bitlevel;
  *device = t->device;
  *stream = t->stream;
}

extern "C" int w2b_export_quantized(w2b_trainer *t, float *out) {
  NEED(t);
  if (!out) return fail(W2B_EINVAL, "w2b_export_quantized: null output");
  if (int rc = xchg_fence(t)) return rc;
  // exported in slabs so that a 14.8 GB table does not need a second full-size device buffer
  const long long slab = 64ll << 20;
  float *tmp = nullptr;
  const long long n = t->table_elems;
  HIPCHK(hipMalloc(&tmp, sizeof(float) * (n < slab ? n : slab)));
  for (long long o = 0; o < n; o += slab) {
    const long long m = (n - o < slab) ? n - o : slab;
    hipError_t e = w2b_launch_export(t->uv + o, t->uv + t->table_elems + o, tmp, m, t->in.cfg.bitlevel, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out + o, tmp, sizeof(float) * m, hipMemcpyDeviceToHost, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) {
      (void)hipFree(tmp);
      return fail(W2B_EHIP, std::string("w2b_export_quantized: ") + hipGetErrorString(e));
    }
  }
  HIPCHK(hipFree(tmp));
  return W2B_OK;
}

// quantize(u+v) bit-packed (bitlevel 1 / 2): 1/32 resp. 1/16 of the bytes of w2b_export_quantized cross the bus
extern "C" int w2b_export_packed(w2b_trainer *t, uint64_t *out) {
  NEED(t);
  if (!out) return fail(W2B_EINVAL, "w2b_export_packed: null output");
  const int64_t wpr = w2b_packed_words_per_row(t->in.cfg.layer1_size, t->in.cfg.bitlevel);
  if (wpr < 0) return fail(W2B_EUNSUPPORTED, "w2b_export_packed: bit-packed output exists for -bitlevel 1 and 2");
  if (int rc = xchg_fence(t)) return rc;
  const long long V = t->in.cfg.vocab_size, slab_rows = (32ll << 20) / wpr > 0 ? (32ll << 20) / wpr : 1;   // <= 256 MB of words
  unsigned long long *tmp = nullptr;
  HIPCHK(hipMalloc(&tmp, sizeof(unsigned long long) * (size_t)((V < slab_rows ? V : slab_rows) * wpr)));
  for (long long r = 0; r < V; r += slab_rows) {
    const long long m = (V - r < slab_rows) ? V - r : slab_rows;
    const long long o = r * t->in.cfg.layer1_size;
    hipError_t e = w2b_launch_export_packed(t->uv + o, t->uv + t->table_elems + o, tmp, m, t->in.cfg.layer1_size,
                                            t->in.cfg.bitlevel, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out + r * wpr, tmp, sizeof(uint64_t) * (size_t)(m * wpr), hipMemcpyDeviceToHost, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) {
      (void)hipFree(tmp);
      return fail(W2B_EHIP, std::string("w2b_export_packed: ") + hipGetErrorString(e));
    }
  }
  HIPCHK(hipFree(tmp));
  return W2B_OK;
}

// --------------------------------------------------------------------------------- sampler state
extern "C" int w2b_set_unigram_table(w2b_trainer *t, const int32_t *table, int64_t tsz) {
  NEED(t);
  if (!table || tsz <= 0) return fail(W2B_EINVAL, "w2b_set_unigram_table: bad argument");
  HIPCHK(hipStreamSynchronize(t->stream));
  if (t->table) HIPCHK(hipFree(t->table));
  t->table = nullptr;
  HIPCHK(hipMalloc(&t->table, sizeof(int32_t) * tsz));
  HIPCHK(hipMemcpy(t->table, table, sizeof(int32_t) * tsz, hipMemcpyHostToDevice));
  t->table_size = tsz;
  return W2B_OK;
}

static int xchg_upload_rates(w2b_trainer *t);   // per-row update rates for the replica exchange's combination rule (below)

extern "C" int w2b_set_vocab_counts(w2b_trainer *t, const int64_t *cn, int64_t table_size) {
  NEED(t);
  if (!cn) return fail(W2B_EINVAL, "w2b_set_vocab_counts: null counts");
  const int64_t V = t->in.cfg.vocab_size;
  const std::vector<float> keep = w2b_plan_set_counts(t->in, cn);
  if (!t->keep) HIPCHK(hipMalloc(&t->keep, sizeof(float) * V));
  HIPCHK(hipMemcpy(t->keep, keep.data(), sizeof(float) * V, hipMemcpyHostToDevice));
  if (int rc = xchg_upload_rates(t)) return rc;
  if (table_size > 0) {
    std::vector<int32_t> tab((size_t)table_size);
    int rc = w2b_build_unigram_table(cn, V, tab.data(), table_size);
    if (rc) return rc;
    return w2b_set_unigram_table(t, tab.data(), table_size);
  }
  return W2B_OK;
}

extern "C" int w2b_set_exp_table(w2b_trainer *t, const float *et) {
  NEED(t);
  if (!et) return fail(W2B_EINVAL, "w2b_set_exp_table: null");
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipMemcpy(t->exp_table, et, sizeof(float) * W2B_EXP_TABLE_SIZE, hipMemcpyHostToDevice));
  return W2B_OK;
}

// --------------------------------------------------------------------------------- timing helpers
static hipError_t timing_begin(w2b_trainer *t) {
  if (!t->timing) return hipSuccess;
  hipEvent_t a, b;
  if (t->ev_pool.size() >= 2) {
    a = t->ev_pool.back(); t->ev_pool.pop_back();
    b = t->ev_pool.back(); t->ev_pool.pop_back();
  } else {
    hipError_t e = hipEventCreate(&a);
    if (e != hipSuccess) return e;
    e = hipEventCreate(&b);
    if (e != hipSuccess) return e;
  }
  t->ev.push_back(a);
  t->ev.push_back(b);
  return hipEventRecord(a, t->stream);
}
static hipError_t timing_end(w2b_trainer *t) {
  if (!t->timing) return hipSuccess;
  return hipEventRecord(t->ev.back(), t->stream);
}

extern "C" int w2b_timing_enable(w2b_trainer *t, int32_t on) {
  if (!t) return fail(W2B_EINVAL, "null trainer");
  t->timing = on != 0;
  return W2B_OK;
}

extern "C" int w2b_timing_read(w2b_trainer *t, double *kernel_ms, int64_t *launches) {
  NEED(t);
  HIPCHK(hipStreamSynchronize(t->stream));
  double ms = 0;
  for (size_t i = 0; i + 1 < t->ev.size(); i += 2) {
    float m = 0;
    HIPCHK(hipEventElapsedTime(&m, t->ev[i], t->ev[i + 1]));
    ms += m;
  }
  if (kernel_ms) *kernel_ms = ms;
  if (launches) *launches = (int64_t)(t->ev.size() / 2);
  for (hipEvent_t e : t->ev) t->ev_pool.push_back(e);
  t->ev.clear();
  return W2B_OK;
}

// per-launch durations of the same events (does NOT reset: w2b_timing_read does)
extern "C" int w2b_timing_launches(w2b_trainer *t, double *ms_out, int64_t capacity, int64_t *launches) {
  NEED(t);
  HIPCHK(hipStreamSynchronize(t->stream));
  const int64_t n = (int64_t)(t->ev.size() / 2);
  if (launches) *launches = n;
  for (int64_t i = 0; i < n && i < capacity && ms_out; i++) {
    float m = 0;
    HIPCHK(hipEventElapsedTime(&m, t->ev[(size_t)(2 * i)], t->ev[(size_t)(2 * i + 1)]));
    ms_out[i] = m;
  }
  return W2B_OK;
}

extern "C" int w2b_synchronize(w2b_trainer *t) {
  NEED(t);
  if (int rc = xchg_fence(t)) return rc;
  HIPCHK(hipStreamSynchronize(t->stream));
  return W2B_OK;
}

// --------------------------------------------------------------------------------- form (i): workers
extern "C" int w2b_set_corpus_slice(w2b_trainer *t, const int32_t *ids, int64_t n, int32_t more_follows) {
  int rc = w2b_set_corpus(t, ids, n);
  if (rc == W2B_OK) t->corpus_more = more_follows != 0;
  return rc;
}

extern "C" int w2b_set_corpus(w2b_trainer *t, const int32_t *ids, int64_t n) {
  NEED(t);
  if (!ids || n < 0) return fail(W2B_EINVAL, "w2b_set_corpus: bad argument");
  t->corpus_more = false;
  for (int64_t i = 0; i < n; i++)       // a bad id would be an out-of-bounds row access on the device
    if (ids[i] < 0 || ids[i] >= t->in.cfg.vocab_size) return fail(W2B_EINVAL, "w2b_set_corpus: token id out of range");
  HIPCHK(hipStreamSynchronize(t->stream));
  if (t->corpus_owned) HIPCHK(hipFree(t->corpus_owned));
  t->corpus_owned = nullptr;
  HIPCHK(hipMalloc(&t->corpus_owned, sizeof(int32_t) * (n > 0 ? n : 1)));
  HIPCHK(hipMemcpy(t->corpus_owned, ids, sizeof(int32_t) * n, hipMemcpyHostToDevice));
  t->corpus = t->corpus_owned;
  t->n_tokens = n;
  return W2B_OK;
}

extern "C" int w2b_set_corpus_device(w2b_trainer *t, const void *ids_dev, int64_t n) {
  NEED(t);
  if (!ids_dev || n < 0) return fail(W2B_EINVAL, "w2b_set_corpus_device: bad argument");
  HIPCHK(hipStreamSynchronize(t->stream));
  if (t->corpus_owned) HIPCHK(hipFree(t->corpus_owned));
  t->corpus_owned = nullptr;
  t->corpus = (const int32_t *)ids_dev;
  t->corpus_more = false;
  t->n_tokens = n;
  return W2B_OK;
}

extern "C" int w2b_set_shards(w2b_trainer *t, const int64_t *starts, const int32_t *ov) {
  if (!t || !starts) return fail(W2B_EINVAL, "w2b_set_shards: bad argument");
  const int nw = t->in.cfg.num_threads;
  for (int i = 0; i < nw; i++) {
    if (starts[i] < 0 || (t->corpus && starts[i] > t->n_tokens))
      return fail(W2B_EINVAL, "w2b_set_shards: shard start outside the token stream");
    if (ov && ov[i] != -2 && ov[i] != -1 && (ov[i] < 0 || ov[i] >= t->in.cfg.vocab_size))
      return fail(W2B_EINVAL, "w2b_set_shards: first_override is neither -2, -1 nor a word id");
  }
  t->shard_start.assign(starts, starts + nw);
  t->shard_override.assign(nw, -2);
  if (ov) t->shard_override.assign(ov, ov + nw);
  t->shards_set = true;
  return W2B_OK;
}

extern "C" int w2b_epoch_begin(w2b_trainer *t) {
  NEED(t);
  if (!t->corpus || !t->shards_set) return fail(W2B_ESTATE, "w2b_epoch_begin: corpus/shards not set");
  for (long long st : t->shard_start)
    if (st > t->n_tokens) return fail(W2B_EINVAL, "w2b_epoch_begin: shard start outside the token stream");
  if (t->in.cfg.negative > 0 && !t->table) return fail(W2B_ESTATE, "w2b_epoch_begin: unigram table not set");
  if (t->in.cfg.sample > 0 && !t->keep) return fail(W2B_ESTATE, "w2b_epoch_begin: vocab counts not set");
  const int nw = t->in.cfg.num_threads;
  std::vector<W2bWorker> w((size_t)nw);
  memset(w.data(), 0, sizeof(W2bWorker) * nw);
  for (int i = 0; i < nw; i++) {
    w[i].rng = (unsigned long long)(t->in.cfg.worker_offset + i);   // global worker id, ref :368
    w[i].cursor = t->shard_start[i];           // ref :377
    w[i].first_override = t->shard_override[i];
  }
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipMemcpy(t->workers, w.data(), sizeof(W2bWorker) * nw, hipMemcpyHostToDevice));
  int zero = 0;
  double dzero = 0;
  HIPCHK(hipMemcpy(&t->shared->workers_done, &zero, sizeof zero, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(&t->shared->loss_epoch, &dzero, sizeof dzero, hipMemcpyHostToDevice));
  t->launches = 0;
  return W2B_OK;
}

// ---- applying a launch plan (w2b_plan.h decides; nothing below does): buffers large enough, cleared / folded as the launch needs
// buffer, flags and counters of the refreshed copies (W2bLaunchPlan::refresh_rows_u) for one launch of the row-group kernel
static int rc_prepare(w2b_trainer *t, W2bParams &p, const W2bLaunchPlan &lp) {
  if (lp.refresh_rows_u <= 0) return W2B_OK;
  if (int rc = grow(t, &t->rc, &t->rc_floats, 64 + (size_t)W2B_NXCD * W2B_RC_MAX * t->in.cfg.layer1_size)) return rc;   // 64 ints of flags, then the copies
  if (!t->rc_stream) {
    HIPCHK(hipStreamCreateWithFlags(&t->rc_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&t->rc_go, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&t->rc_end, hipEventDisableTiming));
  }
  HIPCHK(hipMemsetAsync(t->rc, 0, 64 * sizeof(int), t->stream));                    // claims and alive flags of this launch
  HIPCHK(hipMemsetAsync(&t->shared->launch_done, 0, sizeof(int), t->stream));
  p.rc_rows = lp.refresh_rows_u;
  p.rc_flags = reinterpret_cast<int *>(t->rc);
  p.rc = t->rc + 64;
  return W2B_OK;
}

// scratch rows of process_word_wide for `workgroups` workgroups
static int wide_prepare(w2b_trainer *t, W2bParams &p, long long workgroups) {
  if (!p.wide) return W2B_OK;
  if (int rc = grow(t, &t->wide_scratch, &t->wide_floats, (size_t)workgroups * 2 * t->in.cfg.layer1_size)) return rc;
  p.wide_scratch = t->wide_scratch;
  return W2B_OK;
}

// Buffer of the XCD-shared hot rows for one launch; folds the copies into the masters first when the layout changed or
// somebody wrote the master rows since the last launch.
static int xhot_prepare(w2b_trainer *t, W2bParams &p) {
  const int nu = p.xhot_u, nv = p.xhot_v;
  if (nu + nv == 0) return W2B_OK;
  const size_t need = (size_t)W2B_NXCD * ((size_t)2 * (nu + nv) * t->in.cfg.layer1_size + (size_t)(nu + nv) * W2B_MAXW);
  bool fresh = (nu != t->xhot_nu || nv != t->xhot_nv);
  if (int rc = grow(t, &t->xhot, &t->xhot_floats, need, &fresh)) return rc;
  p.xhot = t->xhot;
  if (fresh) {         // copy == entry (== 0) everywhere: the fold below adopts the master rows
    HIPCHK(hipMemsetAsync(t->xhot, 0, sizeof(float) * need, t->stream));
    t->xhot_nu = nu;
    t->xhot_nv = nv;
    t->xhot_master_changed = true;
  }
  if (t->xhot_master_changed) HIPCHK(w2b_launch_xhot_fold(p, t->stream));
  t->xhot_master_changed = false;
  return W2B_OK;
}

// as many workers as the device holds at once (the occupancy of the kernel that would run -- sentence-resident or plain), capped
// by what the corpus supports (w2b_plan_suggested_workers)
extern "C" int w2b_suggested_threads(w2b_trainer *t, int32_t *out) {
  NEED(t);
  if (!out) return fail(W2B_EINVAL, "w2b_suggested_threads: null");
  const W2bLaunchPlan lp = w2b_plan_launch(t->in, w2b_plan_probe_workers(t->in));
  W2bParams p{};
  w2b_shape_params(p, t->in.cfg, t->in.tune);
  const int per_cu = lp.radius >= 0 ? w2b_resident_per_cu(p, lp.radius, t->in.cfg.compute_loss != 0)
                                    : w2b_workers_per_cu(p, t->in.cfg.compute_loss != 0);
  *out = (int32_t)w2b_plan_suggested_workers(t->in, lp, (long long)per_cu * t->in.num_cus);
  return W2B_OK;
}

extern "C" int w2b_worker_kernel_info(w2b_trainer *t, int32_t *resident, int32_t *radius, int32_t *column_bytes,
                                      int32_t *workgroups_per_cu, int32_t *hot_rows) {
  NEED(t);
  const W2bLaunchPlan lp = w2b_plan_launch(t->in, t->in.cfg.num_threads);
  W2bParams p{};
  w2b_shape_params(p, t->in.cfg, t->in.tune);
  const bool loss = t->in.cfg.compute_loss != 0;
  if (resident) *resident = lp.kernel;      // 0 plain, 1 sentence-resident, 2 row groups
  if (radius) *radius = lp.radius;
  if (hot_rows) *hot_rows = lp.copies_v;
  int vec = 0;
  (void)w2b_block_threads(t->in.cfg.layer1_size, &vec);
  if (column_bytes) *column_bytes = 4 * (lp.radius >= 0 ? 4 : vec);
  if (workgroups_per_cu)
    *workgroups_per_cu = lp.kernel == W2B_KERNEL_RESIDENT ? w2b_resident_per_cu(p, lp.radius, loss)
                                                          : (lp.kernel == W2B_KERNEL_GROUPS ? w2b_groups_per_cu(p, loss) : w2b_workers_per_cu(p, loss));
  return W2B_OK;
}

extern "C" int w2b_train_step(w2b_trainer *t, int64_t max_positions) {
  NEED(t);
  if (!t->corpus || !t->shards_set) return fail(W2B_ESTATE, "w2b_train_step: corpus/shards not set");
  if (max_positions <= 0) return fail(W2B_EINVAL, "w2b_train_step: max_positions must be positive");
  const W2bLaunchPlan lp = w2b_plan_launch(t->in, t->in.cfg.num_threads);
  if (lp.kernel == W2B_KERNEL_RESIDENT)    // scratch rows of the sentence-resident kernel
    if (int rc = grow(t, &t->entry, &t->entry_floats,
                      (size_t)t->in.cfg.num_threads * (size_t)w2b_resident_scratch_rows(lp.radius) * t->in.cfg.layer1_size)) return rc;
  W2bParams p = make_params(t, lp);
  if (int rc = xhot_prepare(t, p)) return rc;
  if (int rc = wide_prepare(t, p, t->in.cfg.num_threads)) return rc;

  t->x_words += (long long)max_positions * t->in.cfg.num_threads;
  t->x_words_full += (long long)max_positions * t->in.cfg.num_threads;
  HIPCHK(timing_begin(t));
  if (lp.kernel == W2B_KERNEL_RESIDENT) HIPCHK(w2b_launch_resident(p, max_positions, lp.radius, t->in.cfg.compute_loss != 0, t->stream, t->debug));
  else if (lp.kernel == W2B_KERNEL_GROUPS) {
    if (int rc = rc_prepare(t, p, lp)) return rc;
    // The refresher runs beside the launch on a stream of its own and ends when the workers have.  Order (advisor, round 5):
    // rc_go (flags and counter of this launch cleared) -> the WORKERS on the training stream -> the refresher on its stream,
    // waiting for rc_go only.  Wherever the two kernels cannot run side by side (streams sharing a hardware queue, serialised
    // launches for debugging) the refresher then starts after the workers, finds launch_done == num_threads, does one sweep
    // and exits -- round 5 launched it first, where it would have spun until its time-out with the workers queued behind it.
    // A failed worker launch returns before the refresher is enqueued.
    if (p.rc_rows > 0) HIPCHK(hipEventRecord(t->rc_go, t->stream));
    HIPCHK(w2b_launch_groups(p, max_positions, t->in.cfg.compute_loss != 0, t->stream));
    if (p.rc_rows > 0) {
      HIPCHK(hipStreamWaitEvent(t->rc_stream, t->rc_go, 0));
      HIPCHK(w2b_launch_refresher(p, t->rc_stream));
      HIPCHK(hipEventRecord(t->rc_end, t->rc_stream));
    }
  }
  else {
    // plain kernel: all workers at once, or -- W2bLaunchPlan::concurrent_workers -- in slices of that many, one slice after
    // the other on the stream (every worker still advances by max_positions per call)
    const int conc = lp.concurrent_workers;
    W2bParams q = p;
    for (int base = 0; base < t->in.cfg.num_threads; base += conc) {
      q.worker_base = base;
      q.num_threads = t->in.cfg.num_threads;
      HIPCHK(w2b_launch_workers(q, max_positions, t->in.cfg.compute_loss != 0, t->stream, base + conc < t->in.cfg.num_threads ? conc : t->in.cfg.num_threads - base));
    }
  }
  HIPCHK(timing_end(t));
  if (p.rc_rows > 0) HIPCHK(hipStreamWaitEvent(t->stream, t->rc_end, 0));   // (what follows on this stream also follows the refresher's end)
  HIPCHK(w2b_launch_xhot_fold(p, t->stream));      // the master rows are complete again when the stream is idle
  {   // progress snapshot of this launch for w2b_epoch_poll (asynchronous; pinned host memory)
    if (!t->poll_host) {
      HIPCHK(hipHostMalloc((void **)&t->poll_host, sizeof(W2bShared) * w2b_trainer::kPoll, hipHostMallocDefault));
      for (int i = 0; i < w2b_trainer::kPoll; i++) HIPCHK(hipEventCreateWithFlags(&t->poll_ev[i], hipEventDisableTiming));
    }
    const int slot = (int)(t->launches % w2b_trainer::kPoll);
    HIPCHK(hipMemcpyAsync(&t->poll_host[slot], t->shared, sizeof(W2bShared), hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipEventRecord(t->poll_ev[slot], t->stream));
    t->launches++;
  }
  return W2B_OK;
}

extern "C" int w2b_epoch_poll(w2b_trainer *t, int32_t lag, int32_t *finished, int64_t *wca, float *alpha,
                              double *loss_sum) {
  NEED(t);
  if (lag < 0 || lag >= w2b_trainer::kPoll) return fail(W2B_EINVAL, "w2b_epoch_poll: lag must be 0..3");
  if (t->launches - lag <= 0) {              // nothing launched that far back yet
    if (finished) *finished = 0;
    if (wca) *wca = 0;
    if (alpha) *alpha = t->in.cfg.alpha;
    if (loss_sum) *loss_sum = 0;
    return W2B_OK;
  }
  const int slot = (int)((t->launches - 1 - lag) % w2b_trainer::kPoll);
  HIPCHK(hipEventSynchronize(t->poll_ev[slot]));
  const W2bShared &sh = t->poll_host[slot];
  if (sh.corpus_overrun)
    return fail(W2B_ESTATE, "a worker reached the end of its corpus slice before its quota (w2b_set_corpus_slice: slice too short)");
  if (finished) *finished = (sh.workers_done >= t->in.cfg.num_threads) ? 1 : 0;
  if (wca) *wca = (int64_t)sh.word_count_actual;
  if (alpha) *alpha = sh.alpha;
  if (loss_sum) *loss_sum = sh.loss_epoch;
  return W2B_OK;
}

extern "C" int w2b_epoch_status(w2b_trainer *t, int32_t *finished, int64_t *wca, float *alpha,
                                double *loss_sum) {
  NEED(t);
  if (int rc = xchg_fence(t)) return rc;
  HIPCHK(hipStreamSynchronize(t->stream));
  W2bShared sh;
  HIPCHK(hipMemcpy(&sh, t->shared, sizeof sh, hipMemcpyDeviceToHost));
  if (sh.corpus_overrun)
    return fail(W2B_ESTATE, "a worker reached the end of its corpus slice before its quota (w2b_set_corpus_slice: slice too short)");
  if (finished) *finished = (sh.workers_done >= t->in.cfg.num_threads) ? 1 : 0;
  if (wca) *wca = (int64_t)sh.word_count_actual;
  if (alpha) *alpha = sh.alpha;
  if (loss_sum) {
    const int nw = t->in.cfg.num_threads;
    std::vector<double> w((size_t)nw);              // only the 8-byte loss field of every worker travels
    HIPCHK(hipMemcpy2D(w.data(), sizeof(double), &t->workers[0].loss, sizeof(W2bWorker), sizeof(double), nw,
                       hipMemcpyDeviceToHost));
    double s = 0;
    for (int i = 0; i < nw; i++) s += w[i];         // ref :537-538, in worker order
    *loss_sum = s;
  }
  return W2B_OK;
}

// --------------------------------------------------------------------------------- form (ii): tuples
extern "C" int w2b_train_tuples_device(w2b_trainer *t, int64_t n, const void *center, const void *ctx_off,
                                       const void *ctx, const void *neg, float alpha, int32_t grid) {
  NEED(t);
  if (n < 0 || !center || !ctx_off || !ctx || (!neg && t->in.cfg.negative > 0))
    return fail(W2B_EINVAL, "w2b_train_tuples_device: bad argument");
  if (n == 0) return W2B_OK;
  // the plain kernel's row rules (per-XCD copies of the hottest rows of both tables, ...); the load estimate uses the
  // workgroups that will run
  long long wgs = grid > 0 ? grid : (long long)(t->in.tune.grid_per_cu > 0 ? t->in.tune.grid_per_cu : 4) * t->in.num_cus;
  if (wgs > n) wgs = n;
  W2bParams p = make_params(t, w2b_plan_launch(t->in, wgs, true));
  {
    if (int rc = xhot_prepare(t, p)) return rc;
    if (p.wide) {                          // (an explicit grid: the scratch rows are per workgroup)
      if (grid <= 0) grid = (int32_t)(n < 2ll * t->in.num_cus ? n : 2ll * t->in.num_cus);
      if (int rc = wide_prepare(t, p, grid)) return rc;
    }
  }
  HIPCHK(timing_begin(t));
  HIPCHK(w2b_launch_tuples(p, n, (const int32_t *)center, (const int32_t *)ctx_off, (const int32_t *)ctx,
                           (const int32_t *)neg, alpha, grid > 0 ? grid : 0, t->in.num_cus, t->in.tune.grid_per_cu,
                           t->in.cfg.compute_loss != 0, t->stream));
  HIPCHK(timing_end(t));
  HIPCHK(w2b_launch_xhot_fold(p, t->stream));
  return W2B_OK;
}

extern "C" int w2b_train_tuples(w2b_trainer *t, int64_t n, const int32_t *center, const int32_t *ctx_off,
                                const int32_t *ctx, const int32_t *neg, float alpha, int32_t serial,
                                double *loss_out) {
  NEED(t);
  if (n < 0 || !center || !ctx_off || !ctx || (!neg && t->in.cfg.negative > 0))
    return fail(W2B_EINVAL, "w2b_train_tuples: bad argument");
  const int K = t->in.cfg.negative;
  const int64_t V = t->in.cfg.vocab_size;
  // validate ids on the host: a bad row index would be an out-of-bounds device access
  for (int64_t i = 0; i < n; i++) {
    if (center[i] < 0 || center[i] >= V) return fail(W2B_EINVAL, "w2b_train_tuples: centre id out of range");
    if (ctx_off[i + 1] < ctx_off[i] || ctx_off[i + 1] - ctx_off[i] > 2 * t->in.cfg.window)
      return fail(W2B_EINVAL, "w2b_train_tuples: context list longer than 2*window or CSR not monotone");
    for (int j = 0; j < K; j++)
      if (neg[i * K + j] >= V) return fail(W2B_EINVAL, "w2b_train_tuples: negative id out of range");
  }
  const int64_t nctx = n ? ctx_off[n] : 0;
  if (n && ctx_off[0] != 0) return fail(W2B_EINVAL, "w2b_train_tuples: ctx_off[0] must be 0");
  for (int64_t j = 0; j < nctx; j++)
    if (ctx[j] < 0 || ctx[j] >= V) return fail(W2B_EINVAL, "w2b_train_tuples: context id out of range");
  if (n == 0) {
    if (loss_out) *loss_out = 0;
    return W2B_OK;
  }
  int rc;
  if ((rc = grow(t, &t->st_center, &t->cap_center, n))) return rc;
  if ((rc = grow(t, &t->st_off, &t->cap_off, n + 1))) return rc;
  if ((rc = grow(t, &t->st_ctx, &t->cap_ctx, nctx > 0 ? nctx : 1))) return rc;
  if ((rc = grow(t, &t->st_neg, &t->cap_neg, (size_t)n * (K > 0 ? K : 1)))) return rc;
  HIPCHK(hipMemcpyAsync(t->st_center, center, sizeof(int32_t) * n, hipMemcpyHostToDevice, t->stream));
  HIPCHK(hipMemcpyAsync(t->st_off, ctx_off, sizeof(int32_t) * (n + 1), hipMemcpyHostToDevice, t->stream));
  if (nctx) HIPCHK(hipMemcpyAsync(t->st_ctx, ctx, sizeof(int32_t) * nctx, hipMemcpyHostToDevice, t->stream));
  if (K) HIPCHK(hipMemcpyAsync(t->st_neg, neg, sizeof(int32_t) * n * K, hipMemcpyHostToDevice, t->stream));
  double zero = 0;
  if (t->in.cfg.compute_loss)
    HIPCHK(hipMemcpyAsync(&t->shared->loss_tuples, &zero, sizeof zero, hipMemcpyHostToDevice, t->stream));
  rc = w2b_train_tuples_device(t, n, t->st_center, t->st_off, t->st_ctx, t->st_neg, alpha, serial ? 1 : 0);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(t->stream));
  if (loss_out) {
    *loss_out = 0;
    if (t->in.cfg.compute_loss)
      HIPCHK(hipMemcpy(loss_out, &t->shared->loss_tuples, sizeof(double), hipMemcpyDeviceToHost));
  }
  return W2B_OK;
}

// --------------------------------------------------------------------------------- multi-GPU (RCCL)
extern "C" int w2b_comm_unique_id(void *out128) {
  if (!out128) return fail(W2B_EINVAL, "w2b_comm_unique_id: null");
  static_assert(sizeof(ncclUniqueId) == W2B_UNIQUE_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  NCCLCHK(ncclGetUniqueId(&id));
  memcpy(out128, &id, sizeof id);
  return W2B_OK;
}

// Buffers, streams and events of the replica exchange (first use).  xs[0] is the ELEMENTWISE stream (delta / apply /
// touched kernels, the begin / end events), xs[1] the COLLECTIVE stream: RCCL serialises the collectives of one
// communicator anyway, so one stream carries all of them, and the elementwise kernels of chunk c + 1 run while the
// collective of chunk c is on the links (round 3 alternated whole chunks between two streams and claimed an overlap of
// the two collectives that RCCL does not give).
static void xchg_teardown(w2b_trainer *t) {
  for (int k = 0; k < 2; k++) {
    if (t->xs[k]) (void)hipStreamSynchronize(t->xs[k]);
    if (t->xd[k]) (void)hipFree(t->xd[k]);
    if (t->xsum[k]) (void)hipFree(t->xsum[k]);
    if (t->x_done[k]) (void)hipEventDestroy(t->x_done[k]);
    if (t->x_evd[k]) (void)hipEventDestroy(t->x_evd[k]);
    if (t->x_evs[k]) (void)hipEventDestroy(t->x_evs[k]);
    if (t->xs[k]) (void)hipStreamDestroy(t->xs[k]);
    t->xd[k] = t->xsum[k] = nullptr;
    t->x_done[k] = t->x_evd[k] = t->x_evs[k] = nullptr;
    t->xs[k] = nullptr;
  }
  if (t->x_train) (void)hipEventDestroy(t->x_train);
  if (t->x_evc) (void)hipEventDestroy(t->x_evc);
  t->x_train = t->x_evc = nullptr;
  t->x_any_done = false;
  if (t->xcnt) (void)hipFree(t->xcnt);
  if (t->xrate) (void)hipFree(t->xrate);
  if (t->base) (void)hipFree(t->base);
  t->xcnt = nullptr;
  t->xrate = nullptr;
  t->base = nullptr;
}

// Expected updates of every row of [u || v] per trained centre word, from the word counts (what w2b_plan_set_counts computes for the
// leading rows, for all of them): a context row (u) is updated once per window it is in -- window + 1 windows per kept
// occurrence on average --, a target row (v) once per draw from the unigram table (ref :112-128, 455-458: raw
// counts; row 0 is remapped, never drawn) and once as the centre word.  "Kept": what survives sub-sampling (ref :403-406).
static int xchg_upload_rates(w2b_trainer *t) {
  if (!t->xrate || t->in.counts.empty() || t->in.counts_tot_kept <= 0 || t->in.counts_pw <= 0) return W2B_OK;
  const long long V = t->in.cfg.vocab_size;
  std::vector<float> r((size_t)(2 * V), 0.f);
  for (long long a = 1; a < V; a++) {
    const double c = (double)t->in.counts[(size_t)a], k = w2b_plan_kept(t->in, c) / t->in.counts_tot_kept;
    r[(size_t)a] = (float)((t->in.cfg.window + 1) * k);
    r[(size_t)(V + a)] = (float)(t->in.cfg.negative * pow(c, 0.75) / t->in.counts_pw + k);
  }
  HIPCHK(hipMemcpy(t->xrate, r.data(), sizeof(float) * 2 * V, hipMemcpyHostToDevice));
  t->xrate_host.swap(r);
  return W2B_OK;
}

static int xchg_setup(w2b_trainer *t) {
  if (t->base) return W2B_OK;
  const long long n = 2 * t->table_elems;
  // chunks of at most 64 M floats (256 MB): small enough that the elementwise kernels of one chunk overlap with the
  // collective of the other, large enough that a ring all-reduce over xGMI runs at its bus bandwidth
  t->xchunk = n < (64ll << 20) ? ((n + 3) & ~3ll) : (64ll << 20);
  hipError_t e = hipMalloc(&t->base, sizeof(float) * n);
  for (int k = 0; k < 2 && e == hipSuccess; k++) {
    e = hipMalloc(&t->xd[k], sizeof(float) * t->xchunk);
    if (e == hipSuccess) e = hipMalloc(&t->xsum[k], sizeof(float) * t->xchunk);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&t->xs[k], hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->x_done[k], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->x_evd[k], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->x_evs[k], hipEventDisableTiming);
  }
  if (e == hipSuccess && !t->wca_buf) e = hipMalloc(&t->wca_buf, 2 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc(&t->xcnt, sizeof(float) * 2 * t->in.cfg.vocab_size);
  if (e == hipSuccess) e = hipMemsetAsync(t->xcnt, 0, sizeof(float) * 2 * t->in.cfg.vocab_size, t->stream);
  if (e == hipSuccess) e = hipMalloc(&t->xrate, sizeof(float) * 2 * t->in.cfg.vocab_size);
  if (e == hipSuccess) e = hipMemsetAsync(t->xrate, 0, sizeof(float) * 2 * t->in.cfg.vocab_size, t->stream);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&t->x_train, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&t->x_evc, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMemcpyAsync(t->base, t->uv, sizeof(float) * n, hipMemcpyDeviceToDevice, t->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  if (e != hipSuccess) {
    xchg_teardown(t);                          // everything or nothing: a retry starts from scratch
    return fail(W2B_EHIP, std::string("replica exchange setup: ") + hipGetErrorString(e));
  }
  if (int rc = xchg_upload_rates(t)) { xchg_teardown(t); return rc; }   // (word counts given later: w2b_set_vocab_counts uploads them)
  return W2B_OK;
}

// The training stream (and with it every reader of the model) waits for the exchange in flight.
static int xchg_fence(w2b_trainer *t) {
  if (!t->x_pending) return W2B_OK;
  for (int k = 0; k < 2; k++) HIPCHK(hipStreamWaitEvent(t->stream, t->x_done[k], 0));
  t->x_pending = false;
  t->xhot_master_changed = true;
  return W2B_OK;
}

extern "C" int w2b_comm_init(w2b_trainer *t, int32_t nranks, int32_t rank, const void *id128) {
  NEED(t);
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(W2B_EINVAL, "w2b_comm_init: bad rank");
  t->nranks = nranks;
  t->rank = rank;
  // replicas of one and no id: nothing to exchange.  With an id a communicator of size 1 is created all the same, so
  // that the whole exchange path (delta, all-reduce, apply, progress counters) can run on a one-GPU machine.
  if (nranks == 1 && !id128) return W2B_OK;
  if (!id128) return fail(W2B_EINVAL, "w2b_comm_init: null id");
  ncclUniqueId id;
  memcpy(&id, id128, sizeof id);
  NCCLCHK(ncclCommInitRank(&t->comm, nranks, id, rank));
  if (int rc = xchg_setup(t)) {                 // leave the trainer as a single replica, not half-initialised
    ncclCommDestroy(t->comm);
    t->comm = nullptr;
    t->nranks = 1;
    t->rank = 0;
    return rc;
  }
  return W2B_OK;
}

extern "C" int w2b_comm_count(w2b_trainer *t, int32_t *nranks_out) {
  if (!t || !nranks_out) return fail(W2B_EINVAL, "w2b_comm_count: null argument");
  *nranks_out = 0;
  if (!t->comm) return W2B_OK;
  int n = 0;
  NCCLCHK(ncclCommCount(t->comm, &n));
  *nranks_out = n;
  return W2B_OK;
}

// ---- one exchange = a list of RANGES of [u || v], each at most one staging buffer long.  A FULL exchange covers the whole
// model in chunks.  (Round 4's HOT-TIER exchange -- the leading rows of both tables only, after every launch -- measured no
// gain over the full exchanges alone and was removed from the ABI in round 5: DESIGN.md Appendix A.)
static long long xchg_chunks(const w2b_trainer *t) { return (long long)t->x_ranges.size(); }

static void xchg_add_range(w2b_trainer *t, long long off, long long len) {
  for (long long o = 0; o < len; o += t->xchunk) {
    const long long m = len - o < t->xchunk ? len - o : t->xchunk;
    t->x_ranges.push_back({off + o, m});
  }
}

extern "C" int w2b_exchange_init(w2b_trainer *t) {
  NEED(t);
  return xchg_setup(t);
}

// Which rows are SATURATED -- have been updated so often in this replica over `words` centre words that the replica's
// delta is no longer a small step.  A row that is a target (v) / a context row (u) of `rate` centre words has received
// rate x words updates; at alpha = 0.05 a few dozen updates move a row most of the way, so W2B_SAT_UPDATES = 32 of them
// make it saturated.  The vocabulary is sorted by count: a prefix per table.
static const double W2B_SAT_UPDATES = 32.0;
static void xchg_saturated_prefix(const w2b_trainer *t, long long words, int *sat_u, int *sat_v) {
  *sat_u = *sat_v = 0;
  const long long V = t->in.cfg.vocab_size;
  if (t->in.counts.empty() || t->in.counts_tot <= 0 || words <= 0) return;
  const double sat = t->in.tune.exchange_sat_updates > 0 ? (double)t->in.tune.exchange_sat_updates : W2B_SAT_UPDATES;
  auto prefix = [&](bool is_v) -> int {
    long long lo = 0, hi = V - 1;
    while (lo < hi) {
      const long long mid = (lo + hi + 1) / 2;
      const double c = (double)t->in.counts[(size_t)mid];
      const double rate = is_v ? w2b_plan_rate_v(t->in, c) : (t->in.cfg.window + 1) * c / t->in.counts_tot;
      if (rate * (double)words >= sat) lo = mid; else hi = mid - 1;
    }
    return (int)lo;
  };
  *sat_u = prefix(false);
  *sat_v = prefix(true);
}

static void xchg_abort(w2b_trainer *t) {       // an exchange that failed between begin and end: forget its (begin, end) events
  if (t->x_open && t->x_ev.size() >= 2) {
    (void)hipEventDestroy(t->x_ev.back()); t->x_ev.pop_back();
    (void)hipEventDestroy(t->x_ev.back()); t->x_ev.pop_back();
  }
  t->x_open = false;
}

static int xchg_begin(w2b_trainer *t) {
  if (!t->base) return fail(W2B_ESTATE, "replica exchange: w2b_comm_init / w2b_exchange_init first (while all replicas "
                                        "still hold the same model)");
  if (t->x_open) return fail(W2B_ESTATE, "replica exchange: the previous exchange was not ended (w2b_exchange_end)");
  while (t->x_ev.size() >= 512) {            // nobody reads the timings (w2b_sync_stats): keep the list bounded
    HIPCHK(hipEventSynchronize(t->x_ev[1]));
    (void)hipEventDestroy(t->x_ev[0]);
    (void)hipEventDestroy(t->x_ev[1]);
    t->x_ev.erase(t->x_ev.begin(), t->x_ev.begin() + 2);
  }
  // the exchange sees every launch issued so far (and nothing forces the launches issued later to wait for a FULL exchange)
  HIPCHK(hipEventRecord(t->x_train, t->stream));
  for (int k = 0; k < 2; k++) HIPCHK(hipStreamWaitEvent(t->xs[k], t->x_train, 0));
  // ... and follows the PREVIOUS exchange on both of its streams: the collective stream's first operations of this exchange
  // (word counts, per-row contributor counts: they read `base`, write `xcnt`) must not run beside the previous exchange's
  // last apply on the elementwise stream (reads `xcnt`, writes `base`).  x_done[0] is recorded after the elementwise stream
  // has waited for the collective one (xchg_end), so it covers both.
  if (t->x_any_done) for (int k = 0; k < 2; k++) HIPCHK(hipStreamWaitEvent(t->xs[k], t->x_done[0], 0));
  hipEvent_t a, b;
  HIPCHK(hipEventCreate(&a));
  HIPCHK(hipEventCreate(&b));
  t->x_ev.push_back(a);
  t->x_ev.push_back(b);
  t->x_open = true;
  {
    const hipError_t e = hipEventRecord(a, t->xs[0]);
    if (e != hipSuccess) { xchg_abort(t); return fail(W2B_EHIP, std::string("replica exchange begin: ") + hipGetErrorString(e)); }
  }
  t->x_ranges.clear();
  xchg_add_range(t, 0, 2 * t->table_elems);
  xchg_saturated_prefix(t, t->x_words_full, &t->x_sat_u, &t->x_sat_v);    // over the words since the last exchange
  t->x_words_sync = t->x_words_full;
  t->x_fac_pending = false;
  return W2B_OK;
}
static int xchg_delta(w2b_trainer *t, long long c) {
  const auto &r = t->x_ranges[(size_t)c];
  const int k = (int)(c & 1);
  HIPCHK(w2b_launch_xchg_delta(t->uv + r.off, t->base + r.off, t->xd[k], t->xsum[k], r.len, t->xs[0]));
  return W2B_OK;
}
// ---- the combination rule of mode 2: a per-row factor on the SUM of the replicas' deltas (k_xchg_factor has the formulas).
// Round 6 measured three families on 8 replicas x 128 workers against the single replica with the same 1024 workers
// (tests/experiments/replica_rules.py, replica_truth.py; profiles/r06_sessions/):
//   * the hard threshold of rounds 4-5 (mean of the contributors from 32 expected updates on, sum below): -9.0 % of the single
//     replica's epoch loss at 131 K words per replica between two exchanges, -9.9 % at 16 K;
//   * exponential saturation (rule 2): -7.4 % (tau = 64; 8: -14 %, 32: -8.1 %, 128: -7.7 %, 256: -9.1 %);
//   * the per-row least-squares factor of a truth run's delta on the replicas' summed delta (0.75 at one update, falling only
//     logarithmically: 0.45 at 256 updates) -- optimal for ONE interval from a common model, and divergent in closed loop: -18 %,
//     the final model worthless.  It is dominated by the drift of the fp32 masters (which no forward value sees) and over-relaxes the
//     elements near a sign flip (which every forward value sees).  Not shipped; the measurement stays in the experiment scripts.
//   * rule 0, the default: exponential saturation decides every element's QUANTIZED value, and where the whole sum lands in the
//     same quantization cell it is taken instead (k_xchg_apply) -- the forward values of the stable rule, the masters' inertia of a
//     shared model: -2.9 % at 131 K words per replica on the 22 M-token proxy (-0.3 % with doubling intervals), -0.5 % on the
//     literal configs[1] stream at 1 M words.  ONE BIT ONLY: there a forward value is a sign and a master's magnitude is pure inertia.
//     With more bits the magnitude is part of the forward value and the cells do harm -- two bits, same proxy at 86 K words: cells
//     -9.4 %, saturation alone -1.9 %, the sign alone as the criterion diverges (four bits: cells -6.3 %; profiles/r06_sessions/r06o,
//     r06p) -- so every other bitlevel runs the saturation factor alone.
// contributor counts in xcnt -> factors on the summed delta (k_xchg_factor), once per exchange, on stream q
static const double W2B_XCHG_TAU_U = 64.0, W2B_XCHG_TAU_V = 64.0;   // updates that move a row most of the way
static int xchg_factor(w2b_trainer *t, hipStream_t q) {
  if (!t->x_fac_pending) return W2B_OK;
  const int rule = t->in.tune.exchange_rule;
  const float tau_u = t->in.tune.exchange_tau_u > 0 ? (float)t->in.tune.exchange_tau_u : (float)W2B_XCHG_TAU_U;
  const float tau_v = t->in.tune.exchange_tau_v > 0 ? (float)t->in.tune.exchange_tau_v : (float)W2B_XCHG_TAU_V;
  HIPCHK(w2b_launch_xchg_factor(t->xcnt, t->xrate_host.empty() ? nullptr : t->xrate, (float)t->x_words_sync, tau_u, tau_v, t->in.cfg.vocab_size,
                                rule, t->x_sat_u, t->x_sat_v, q));
  t->x_fac_pending = false;
  return W2B_OK;
}
static int xchg_apply(w2b_trainer *t, long long c, float scale) {
  const auto &r = t->x_ranges[(size_t)c];
  const int k = (int)(c & 1);
  if (t->x_use_cnt) if (int rc = xchg_factor(t, t->xs[0])) return rc;
  HIPCHK(w2b_launch_xchg_apply(t->uv + r.off, t->base + r.off, t->xd[k], t->xsum[k], scale, r.len, t->x_use_cnt ? t->xcnt : nullptr,
                               r.off, t->in.cfg.layer1_size, t->in.cfg.bitlevel, (t->in.tune.exchange_rule == 0 && t->in.cfg.bitlevel == 1) ? 1 : 0, t->xs[0]));
  return W2B_OK;
}
// per row of [u || v]: has this replica changed it since the last exchange?
static int xchg_touched(w2b_trainer *t, hipStream_t s) {
  const long long V = t->in.cfg.vocab_size, D = t->in.cfg.layer1_size;
  return w2b_launch_xchg_touched(t->uv, t->base, t->xcnt, 2 * V, (int)D, s) == hipSuccess ? W2B_OK : fail(W2B_EHIP, "k_xchg_touched");
}

static int xchg_end(w2b_trainer *t) {
  t->x_words_full = 0;
  t->x_words = 0;
  // x_ev.back() = the end of this exchange: the elementwise stream waits for the collective stream's last operation first
  HIPCHK(hipEventRecord(t->x_done[1], t->xs[1]));
  HIPCHK(hipStreamWaitEvent(t->xs[0], t->x_done[1], 0));
  HIPCHK(hipEventRecord(t->x_ev.back(), t->xs[0]));
  HIPCHK(hipEventRecord(t->x_done[0], t->xs[0]));
  t->x_any_done = true;
  t->x_open = false;
  t->x_pending = true;
  t->sync_count++;
  long long bytes = 0;
  for (const auto &r : t->x_ranges) bytes += r.len * (long long)sizeof(float);
  t->sync_bytes += bytes;
  return W2B_OK;
}

// The library's own collective.  Software pipeline over the chunks: E = xs[0] (elementwise), C = xs[1] (collective)
//      E: delta(0) delta(1) apply(0) delta(2) apply(1) ...          C: sum(0) sum(1) sum(2) ...
// with events delta(c) -> sum(c) -> apply(c); slot c & 1 of the staging buffers is free again when apply(c) has been issued
// on E before delta(c + 2).
static int xchg_run_rccl(w2b_trainer *t, int32_t mode) {
  hipStream_t E = t->xs[0], Cs = t->xs[1];
  // progress first (16 bytes): every replica learns the global word count -- the alpha schedule (ref :391) is exact
  // at every exchange and extrapolates in between (W2bShared::wca_others)
  HIPCHK(w2b_launch_wca_pack(t->shared, t->wca_buf, Cs));
  NCCLCHK(ncclAllReduce(t->wca_buf, t->wca_buf + 1, 1, ncclUint64, ncclSum, t->comm, Cs));
  HIPCHK(w2b_launch_wca_unpack(t->shared, t->wca_buf, Cs));
  const float scale = mode == 1 ? 1.f / (float)t->nranks : 1.f;
  t->x_use_cnt = mode == 2;
  if (mode == 2) {          // who has trained which row since the last exchange (2 V floats), before the first apply
    if (int rc = xchg_touched(t, Cs)) return rc;
    NCCLCHK(ncclAllReduce(t->xcnt, t->xcnt, (size_t)(2 * t->in.cfg.vocab_size), ncclFloat, ncclSum, t->comm, Cs));
    t->x_fac_pending = true;
    if (int rc = xchg_factor(t, Cs)) return rc;
    HIPCHK(hipEventRecord(t->x_evc, Cs));
    HIPCHK(hipStreamWaitEvent(E, t->x_evc, 0));
  }
  const long long nc = xchg_chunks(t);
  auto issue_delta_sum = [&](long long c) -> int {
    const int k = (int)(c & 1);
    if (int rc = xchg_delta(t, c)) return rc;
    HIPCHK(hipEventRecord(t->x_evd[k], E));
    HIPCHK(hipStreamWaitEvent(Cs, t->x_evd[k], 0));
    NCCLCHK(ncclAllReduce(t->xsum[k], t->xsum[k], (size_t)t->x_ranges[(size_t)c].len, ncclFloat, ncclSum, t->comm, Cs));
    HIPCHK(hipEventRecord(t->x_evs[k], Cs));
    return W2B_OK;
  };
  if (nc > 0) if (int rc = issue_delta_sum(0)) return rc;
  for (long long c = 0; c < nc; c++) {
    if (c + 1 < nc) if (int rc = issue_delta_sum(c + 1)) return rc;
    HIPCHK(hipStreamWaitEvent(E, t->x_evs[c & 1], 0));
    if (int rc = xchg_apply(t, c, scale)) return rc;
  }
  return W2B_OK;
}

extern "C" int64_t w2b_suggested_exchange_words(int64_t train_words_per_epoch, int32_t replicas) {
  if (replicas < 1) replicas = 1;
  long long words = train_words_per_epoch / replicas / 32;
  if (words < 32768) words = 32768;
  if (words > 1048576) words = 1048576;
  return words;
}

extern "C" int w2b_sync_replicas(w2b_trainer *t, int32_t mode) {
  NEED(t);
  if (!t->comm) return W2B_OK;             // a single replica without a communicator: nothing to exchange
  if (mode < 0 || mode > 2) return fail(W2B_EINVAL, "w2b_sync_replicas: unknown mode");
  if (int rc = xchg_begin(t)) return rc;
  if (int rc = xchg_run_rccl(t, mode)) { xchg_abort(t); return rc; }
  return xchg_end(t);
}

// ---- the same exchange for a host that brings its own collective (MPI, torch.distributed over gloo / RCCL, ...):
//   w2b_exchange_begin -> (w2b_exchange_counts, <sum over the replicas>) -> for every chunk: w2b_exchange_delta,
//   <sum *buf over the replicas, in place>, w2b_exchange_apply -> w2b_exchange_end.  The buffer handed out is device
// memory; the library's kernels run on its elementwise exchange stream, so w2b_exchange_delta returns after the delta is
// complete (the host's collective may use any stream or the CPU) and w2b_exchange_apply expects the sum to be complete
// when it is called.
static int xchg_begin_host(w2b_trainer *t, int64_t *n_chunks, int64_t *local_word_count) {
  if (int rc = xchg_begin(t)) return rc;
  t->x_use_cnt = false;
  if (n_chunks) *n_chunks = xchg_chunks(t);
  if (local_word_count) {
    hipError_t e = w2b_launch_wca_pack(t->shared, t->wca_buf, t->xs[0]);
    unsigned long long v = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&v, t->wca_buf, sizeof v, hipMemcpyDeviceToHost, t->xs[0]);
    if (e == hipSuccess) e = hipStreamSynchronize(t->xs[0]);
    if (e != hipSuccess) { xchg_abort(t); return fail(W2B_EHIP, std::string("w2b_exchange_begin: ") + hipGetErrorString(e)); }
    *local_word_count = (int64_t)v;
  }
  return W2B_OK;
}
extern "C" int w2b_exchange_begin(w2b_trainer *t, int64_t *n_chunks, int64_t *local_word_count) {
  NEED(t);
  return xchg_begin_host(t, n_chunks, local_word_count);
}
extern "C" int w2b_exchange_counts(w2b_trainer *t, void **buf_dev, int64_t *elems) {
  NEED(t);
  if (!t->base || !t->x_open) return fail(W2B_ESTATE, "w2b_exchange_counts: w2b_exchange_begin first");
  if (!buf_dev || !elems) return fail(W2B_EINVAL, "w2b_exchange_counts: null argument");
  if (int rc = xchg_touched(t, t->xs[0])) return rc;
  HIPCHK(hipStreamSynchronize(t->xs[0]));
  t->x_use_cnt = true;
  t->x_fac_pending = true;                   // (the host sums the counts; the first w2b_exchange_apply turns them into factors)
  *buf_dev = t->xcnt;
  *elems = 2 * t->in.cfg.vocab_size;
  return W2B_OK;
}

extern "C" int w2b_exchange_delta(w2b_trainer *t, int64_t chunk, void **buf_dev, int64_t *elems) {
  NEED(t);
  if (!t->base || !t->x_open) return fail(W2B_ESTATE, "w2b_exchange_delta: w2b_exchange_begin first");
  if (chunk < 0 || chunk >= xchg_chunks(t) || !buf_dev || !elems) return fail(W2B_EINVAL, "w2b_exchange_delta: bad argument");
  if (int rc = xchg_delta(t, chunk)) return rc;
  HIPCHK(hipStreamSynchronize(t->xs[0]));
  *buf_dev = t->xsum[chunk & 1];
  *elems = t->x_ranges[(size_t)chunk].len;
  return W2B_OK;
}
extern "C" int w2b_exchange_apply(w2b_trainer *t, int64_t chunk, float scale) {
  NEED(t);
  if (!t->base || !t->x_open) return fail(W2B_ESTATE, "w2b_exchange_apply: w2b_exchange_begin first");
  if (chunk < 0 || chunk >= xchg_chunks(t)) return fail(W2B_EINVAL, "w2b_exchange_apply: bad chunk");
  return xchg_apply(t, chunk, scale);
}
extern "C" int w2b_exchange_end(w2b_trainer *t, int64_t word_count_all_replicas) {
  NEED(t);
  if (!t->base || !t->x_open) return fail(W2B_ESTATE, "w2b_exchange_end: w2b_exchange_begin first");
  if (word_count_all_replicas >= 0) {        // the alpha schedule runs on the global count (ref :391)
    unsigned long long v = (unsigned long long)word_count_all_replicas;
    HIPCHK(hipMemcpyAsync(t->wca_buf + 1, &v, sizeof v, hipMemcpyHostToDevice, t->xs[0]));
    HIPCHK(hipStreamSynchronize(t->xs[0]));
    HIPCHK(w2b_launch_wca_unpack(t->shared, t->wca_buf, t->xs[0]));
  }
  return xchg_end(t);
}

extern "C" int w2b_sync_stats(w2b_trainer *t, int64_t *exchanges, double *device_ms) {
  if (!t) return fail(W2B_EINVAL, "null trainer");
  HIPCHK(hipSetDevice(t->device));
  if (exchanges) *exchanges = t->sync_count;
  double ms = 0;
  if (t->x_open) return fail(W2B_ESTATE, "w2b_sync_stats: an exchange is in progress (w2b_exchange_end first)");
  for (size_t i = 0; i + 1 < t->x_ev.size(); i += 2) {      // begin -> end of every exchange, read after the fact
    HIPCHK(hipEventSynchronize(t->x_ev[i + 1]));
    float m = 0;
    HIPCHK(hipEventElapsedTime(&m, t->x_ev[i], t->x_ev[i + 1]));
    ms += m;
  }
  for (hipEvent_t e : t->x_ev) (void)hipEventDestroy(e);
  t->x_ev.clear();
  if (device_ms) *device_ms = ms;
  t->sync_count = 0;
  t->sync_bytes = 0;
  return W2B_OK;
}
