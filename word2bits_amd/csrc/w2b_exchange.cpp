// w2b_exchange.cpp -- the replica exchange of the C ABI in include/word2bits_hip.h (w2b_comm_*, w2b_sync_replicas,
// w2b_exchange_*, w2b_sync_stats): every replica adds what the others have trained since the previous exchange.  All of its
// state is a W2bExchange; the trainer's side of the seam is w2b_exchange.h.  The arithmetic is in w2b_kernels_misc.hip.
#include "w2b_exchange.h"
#include "w2b_host.h"

#include <cmath>
#include <cstring>
#include <memory>

// xs[0] is the ELEMENTWISE stream (delta / apply / touched kernels, the begin / end events), xs[1] the COLLECTIVE stream: RCCL
// serialises the collectives of one communicator anyway, so one stream carries all of them, and the elementwise kernels of
// chunk c + 1 run while the collective of chunk c is on the links.  The destructor synchronises both; the members then
// release themselves in reverse order of declaration: events, buffers, streams, communicator.
struct W2bExchange {
  const W2bExchangeView v;                  // all that is read of the trainer
  struct Comm { ncclComm_t c = nullptr; ~Comm() { if (c) ncclCommDestroy(c); } } comm;   // c null: phase API only (w2b_exchange_init)
  int nranks = 1;
  W2bStream xs[2];
  W2bDevBuf<float> base;                    // [u || v] as it was after the previous exchange: the same on every replica
  W2bDevBuf<float> xd[2], xsum[2];          // per slot: own delta / sum over the replicas
  W2bDevBuf<float> xcnt;                    // [2 * vocab_size]: replicas that changed each row, then the row's factor on the summed delta (mode 2)
  W2bDevBuf<float> xrate;                   // [2 * vocab_size]: expected updates of every row of [u || v] per trained centre word (from the word counts)
  bool have_rates = false;                  // xrate has been filled (false = no word counts yet)
  W2bDevBuf<unsigned long long> wca_buf;    // [2]: this replica's word_count_actual, the sum over all replicas
  long long xchunk = 0;                     // floats per chunk
  struct XRange { long long off, len; };    // floats of [u || v]
  std::vector<XRange> x_ranges;             // the chunks of the exchange in progress: the whole model, each at most one staging buffer long
  bool x_open = false;                      // the exchange in progress has begun and not ended
  long long x_words_full = 0;               // centre words since the previous exchange
  long long x_words_sync = 0;               // x_words_full at the begin of the exchange in progress (the n of the combination rule)
  bool x_fac_pending = false;               // xcnt holds contributor counts that k_xchg_factor has not yet turned into factors
  bool x_use_cnt = false;                   // the exchange in progress damps the saturated rows' sums by xcnt
  int x_sat_u = 0, x_sat_v = 0;             // rows 1..x_sat_* of u / v count as saturated in the exchange in progress
  W2bEvent x_evd[2], x_evs[2], x_evc;       // delta / sum of a slot complete; counts summed
  W2bEvent x_train;                         // "the launches issued so far": the exchange streams wait for it
  W2bEvent x_done[2];                       // last operation of the latest exchange on each exchange stream
  bool x_any_done = false;                  // x_done[] have been recorded at least once
  bool x_pending = false;                   // the training stream has not yet waited for x_done
  std::vector<W2bEvent> x_ev;               // (begin, end) pairs of the exchanges since the last w2b_sync_stats
  long long sync_count = 0;

  explicit W2bExchange(const W2bExchangeView &view) : v(view) {}
  ~W2bExchange() { for (W2bStream &q : xs) if (q) (void)hipStreamSynchronize(q); }
};

// ---- the trainer's five operations (w2b_exchange.h)
int w2b_xchg_fence(W2bExchange *x, bool *waited) {
  if (!x || !x->x_pending) return W2B_OK;
  for (int k = 0; k < 2; k++) HIPCHK(hipStreamWaitEvent(x->v.stream, x->x_done[k], 0));
  x->x_pending = false;
  *waited = true;
  return W2B_OK;
}

hipError_t w2b_xchg_rebase(W2bExchange *x, hipStream_t s) {
  if (!x) return hipSuccess;
  return hipMemcpyAsync(x->base, x->v.uv, sizeof(float) * 2 * x->v.table_elems, hipMemcpyDeviceToDevice, s);
}

void w2b_xchg_add_words(W2bExchange *x, long long words) { if (x) x->x_words_full += words; }

// Expected updates of every row of [u || v] per trained centre word, from the word counts (what w2b_plan_set_counts computes for the
// leading rows, for all of them): a context row (u) is updated once per window it is in -- window + 1 windows per kept
// occurrence on average --, a target row (v) once per draw from the unigram table (ref :112-128, 455-458: raw
// counts; row 0 is remapped, never drawn) and once as the centre word.  "Kept": what survives sub-sampling (ref :403-406).
int w2b_xchg_upload_rates(W2bExchange *x) {
  if (!x) return W2B_OK;
  const W2bPlanInputs &in = x->v.in;
  if (in.counts.empty() || in.counts_tot_kept <= 0 || in.counts_pw <= 0) return W2B_OK;
  const long long V = in.cfg.vocab_size;
  std::vector<float> r((size_t)(2 * V), 0.f);
  for (long long a = 1; a < V; a++) {
    const double c = (double)in.counts[(size_t)a], k = w2b_plan_kept(in, c) / in.counts_tot_kept;
    r[(size_t)a] = (float)((in.cfg.window + 1) * k);
    r[(size_t)(V + a)] = (float)(in.cfg.negative * pow(c, 0.75) / in.counts_pw + k);
  }
  HIPCHK(hipMemcpy(x->xrate, r.data(), sizeof(float) * 2 * V, hipMemcpyHostToDevice));
  x->have_rates = true;
  return W2B_OK;
}

void w2b_xchg_destroy(W2bExchange *x) { delete x; }

// ---- creation: everything or nothing (a retry starts from scratch), and base := model on the training stream
#define TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)
static hipError_t xchg_alloc(W2bExchange *x) {
  const long long n = 2 * x->v.table_elems, V2 = 2 * x->v.in.cfg.vocab_size;
  // chunks of at most 64 M floats (256 MB): small enough that the elementwise kernels of one chunk overlap with the
  // collective of the other, large enough that a ring all-reduce over xGMI runs at its bus bandwidth
  x->xchunk = n < (64ll << 20) ? ((n + 3) & ~3ll) : (64ll << 20);
  TRY(x->base.alloc((size_t)n));
  for (int k = 0; k < 2; k++) {
    TRY(x->xd[k].alloc((size_t)x->xchunk));
    TRY(x->xsum[k].alloc((size_t)x->xchunk));
    TRY(x->xs[k].create());
    TRY(x->x_done[k].create());
    TRY(x->x_evd[k].create());
    TRY(x->x_evs[k].create());
  }
  TRY(x->wca_buf.alloc(2));
  TRY(x->xcnt.alloc((size_t)V2));
  TRY(hipMemsetAsync(x->xcnt, 0, sizeof(float) * V2, x->v.stream));
  TRY(x->xrate.alloc((size_t)V2));
  TRY(hipMemsetAsync(x->xrate, 0, sizeof(float) * V2, x->v.stream));
  TRY(x->x_train.create());
  TRY(x->x_evc.create());
  TRY(w2b_xchg_rebase(x, x->v.stream));
  return hipStreamSynchronize(x->v.stream);
}
#undef TRY

static int xchg_setup(w2b_trainer *t) {
  if (t->xchg) return W2B_OK;
  std::unique_ptr<W2bExchange> x(new W2bExchange(W2bExchangeView{t->uv, t->table_elems, t->stream, t->shared, t->in}));
  const hipError_t e = xchg_alloc(x.get());
  if (e != hipSuccess) return fail(W2B_EHIP, std::string("replica exchange setup: ") + hipGetErrorString(e));
  if (int rc = w2b_xchg_upload_rates(x.get())) return rc;   // (word counts given later: w2b_set_vocab_counts uploads them)
  t->xchg = x.release();
  return W2B_OK;
}

extern "C" int w2b_comm_unique_id(void *out128) {
  if (!out128) return fail(W2B_EINVAL, "w2b_comm_unique_id: null");
  static_assert(sizeof(ncclUniqueId) == W2B_UNIQUE_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  NCCLCHK(ncclGetUniqueId(&id));
  memcpy(out128, &id, sizeof id);
  return W2B_OK;
}

extern "C" int w2b_comm_init(w2b_trainer *t, int32_t nranks, int32_t rank, const void *id128) {
  NEED(t);
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(W2B_EINVAL, "w2b_comm_init: bad rank");
  // replicas of one and no id: nothing to exchange.  With an id a communicator of size 1 is created all the same, so
  // that the whole exchange path (delta, all-reduce, apply, progress counters) can run on a one-GPU machine.
  if (nranks == 1 && !id128) return W2B_OK;
  if (!id128) return fail(W2B_EINVAL, "w2b_comm_init: null id");
  ncclUniqueId id;
  memcpy(&id, id128, sizeof id);
  W2bExchange::Comm comm;
  NCCLCHK(ncclCommInitRank(&comm.c, nranks, id, rank));
  if (int rc = xchg_setup(t)) return rc;          // the trainer stays a single replica, not half-initialised
  std::swap(t->xchg->comm.c, comm.c);
  t->xchg->nranks = nranks;
  return W2B_OK;
}

extern "C" int w2b_comm_count(w2b_trainer *t, int32_t *nranks_out) {
  if (!t || !nranks_out) return fail(W2B_EINVAL, "w2b_comm_count: null argument");
  *nranks_out = 0;
  if (!t->xchg || !t->xchg->comm.c) return W2B_OK;
  int n = 0;
  NCCLCHK(ncclCommCount(t->xchg->comm.c, &n));
  *nranks_out = n;
  return W2B_OK;
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
static void xchg_saturated_prefix(const W2bPlanInputs &in, long long words, int *sat_u, int *sat_v) {
  *sat_u = *sat_v = 0;
  const long long V = in.cfg.vocab_size;
  if (in.counts.empty() || in.counts_tot <= 0 || words <= 0) return;
  const double sat = in.tune.exchange_sat_updates > 0 ? (double)in.tune.exchange_sat_updates : W2B_SAT_UPDATES;
  auto prefix = [&](bool is_v) -> int {
    long long lo = 0, hi = V - 1;
    while (lo < hi) {
      const long long mid = (lo + hi + 1) / 2;
      const double c = (double)in.counts[(size_t)mid];
      const double rate = is_v ? w2b_plan_rate_v(in, c) : (in.cfg.window + 1) * c / in.counts_tot;
      if (rate * (double)words >= sat) lo = mid; else hi = mid - 1;
    }
    return (int)lo;
  };
  *sat_u = prefix(false);
  *sat_v = prefix(true);
}

static void xchg_abort(W2bExchange *x) {       // an exchange that failed between begin and end: forget its (begin, end) events
  if (x->x_open && x->x_ev.size() >= 2) x->x_ev.resize(x->x_ev.size() - 2);
  x->x_open = false;
}

static int xchg_begin(W2bExchange *x) {
  if (!x) return fail(W2B_ESTATE, "replica exchange: w2b_comm_init / w2b_exchange_init first (while all replicas "
                                  "still hold the same model)");
  if (x->x_open) return fail(W2B_ESTATE, "replica exchange: the previous exchange was not ended (w2b_exchange_end)");
  while (x->x_ev.size() >= 512) {            // nobody reads the timings (w2b_sync_stats): keep the list bounded
    HIPCHK(hipEventSynchronize(x->x_ev[1]));
    x->x_ev.erase(x->x_ev.begin(), x->x_ev.begin() + 2);
  }
  // the exchange sees every launch issued so far (and nothing forces the launches issued later to wait for it)
  HIPCHK(hipEventRecord(x->x_train, x->v.stream));
  for (int k = 0; k < 2; k++) HIPCHK(hipStreamWaitEvent(x->xs[k], x->x_train, 0));
  // ... and follows the PREVIOUS exchange on both of its streams: the collective stream's first operations of this exchange
  // (word counts, per-row contributor counts: they read `base`, write `xcnt`) must not run beside the previous exchange's
  // last apply on the elementwise stream (reads `xcnt`, writes `base`).  x_done[0] is recorded after the elementwise stream
  // has waited for the collective one (xchg_end), so it covers both.
  if (x->x_any_done) for (int k = 0; k < 2; k++) HIPCHK(hipStreamWaitEvent(x->xs[k], x->x_done[0], 0));
  W2bEvent a, b;
  HIPCHK(a.create(hipEventDefault));
  HIPCHK(b.create(hipEventDefault));
  x->x_ev.push_back(std::move(a));
  x->x_ev.push_back(std::move(b));
  x->x_open = true;
  const hipError_t e = hipEventRecord(x->x_ev[x->x_ev.size() - 2], x->xs[0]);
  if (e != hipSuccess) { xchg_abort(x); return fail(W2B_EHIP, std::string("replica exchange begin: ") + hipGetErrorString(e)); }
  x->x_ranges.clear();
  for (long long o = 0, n = 2 * x->v.table_elems; o < n; o += x->xchunk) x->x_ranges.push_back({o, n - o < x->xchunk ? n - o : x->xchunk});
  xchg_saturated_prefix(x->v.in, x->x_words_full, &x->x_sat_u, &x->x_sat_v);    // over the words since the last exchange
  x->x_words_sync = x->x_words_full;
  x->x_fac_pending = false;
  return W2B_OK;
}
static int xchg_delta(W2bExchange *x, long long c) {
  const auto &r = x->x_ranges[(size_t)c];
  const int k = (int)(c & 1);
  HIPCHK(w2b_launch_xchg_delta(x->v.uv + r.off, x->base + r.off, x->xd[k], x->xsum[k], r.len, x->xs[0]));
  return W2B_OK;
}
// ---- the combination rule of mode 2: a per-row factor on the SUM of the replicas' deltas (k_xchg_factor has the formulas;
// DESIGN.md section 3.5 has what was measured, rule against rule).  Rule 1 is a hard threshold: the mean of the contributors
// for the saturated rows (xchg_saturated_prefix), the sum for the others.  Rule 2 is exponential saturation: from the sum to
// the mean as the expected updates of a row (xrate x words) pass tau.  Rule 0, the default, lets rule 2 decide every element's
// QUANTIZED value and takes the whole sum wherever that lands in the same quantization cell (k_xchg_apply) -- at ONE BIT
// only, where a forward value is a sign and a master's magnitude pure inertia; every other bitlevel runs rule 2's factor alone.
// contributor counts in xcnt -> factors on the summed delta, once per exchange, on stream q
static const double W2B_XCHG_TAU_U = 64.0, W2B_XCHG_TAU_V = 64.0;   // updates that move a row most of the way
static int xchg_factor(W2bExchange *x, hipStream_t q) {
  if (!x->x_fac_pending) return W2B_OK;
  const w2b_tuning &tune = x->v.in.tune;
  const float tau_u = tune.exchange_tau_u > 0 ? (float)tune.exchange_tau_u : (float)W2B_XCHG_TAU_U;
  const float tau_v = tune.exchange_tau_v > 0 ? (float)tune.exchange_tau_v : (float)W2B_XCHG_TAU_V;
  HIPCHK(w2b_launch_xchg_factor(x->xcnt, x->have_rates ? x->xrate.p : nullptr, (float)x->x_words_sync, tau_u, tau_v, x->v.in.cfg.vocab_size,
                                tune.exchange_rule, x->x_sat_u, x->x_sat_v, q));
  x->x_fac_pending = false;
  return W2B_OK;
}
static int xchg_apply(W2bExchange *x, long long c, float scale) {
  const auto &r = x->x_ranges[(size_t)c];
  const int k = (int)(c & 1);
  const w2b_config &cfg = x->v.in.cfg;
  if (x->x_use_cnt) if (int rc = xchg_factor(x, x->xs[0])) return rc;
  HIPCHK(w2b_launch_xchg_apply(x->v.uv + r.off, x->base + r.off, x->xd[k], x->xsum[k], scale, r.len, x->x_use_cnt ? x->xcnt.p : nullptr,
                               r.off, cfg.layer1_size, cfg.bitlevel, (x->v.in.tune.exchange_rule == 0 && cfg.bitlevel == 1) ? 1 : 0, x->xs[0]));
  return W2B_OK;
}
// per row of [u || v]: has this replica changed it since the last exchange?
static int xchg_touched(W2bExchange *x, hipStream_t s) {
  const long long V = x->v.in.cfg.vocab_size, D = x->v.in.cfg.layer1_size;
  return w2b_launch_xchg_touched(x->v.uv, x->base, x->xcnt, 2 * V, (int)D, s) == hipSuccess ? W2B_OK : fail(W2B_EHIP, "k_xchg_touched");
}

static int xchg_end(W2bExchange *x) {
  x->x_words_full = 0;
  // x_ev.back() = the end of this exchange: the elementwise stream waits for the collective stream's last operation first
  HIPCHK(hipEventRecord(x->x_done[1], x->xs[1]));
  HIPCHK(hipStreamWaitEvent(x->xs[0], x->x_done[1], 0));
  HIPCHK(hipEventRecord(x->x_ev.back(), x->xs[0]));
  HIPCHK(hipEventRecord(x->x_done[0], x->xs[0]));
  x->x_any_done = true;
  x->x_open = false;
  x->x_pending = true;
  x->sync_count++;
  return W2B_OK;
}

// The library's own collective.  Software pipeline over the chunks: E = xs[0] (elementwise), C = xs[1] (collective)
//      E: delta(0) delta(1) apply(0) delta(2) apply(1) ...          C: sum(0) sum(1) sum(2) ...
// with events delta(c) -> sum(c) -> apply(c); slot c & 1 of the staging buffers is free again when apply(c) has been issued
// on E before delta(c + 2).
static int xchg_run_rccl(W2bExchange *x, int32_t mode) {
  hipStream_t E = x->xs[0], Cs = x->xs[1];
  const ncclComm_t comm = x->comm.c;
  // progress first (16 bytes): every replica learns the global word count -- the alpha schedule (ref :391) is exact
  // at every exchange and extrapolates in between (W2bShared::wca_others)
  HIPCHK(w2b_launch_wca_pack(x->v.shared, x->wca_buf, Cs));
  NCCLCHK(ncclAllReduce(x->wca_buf, x->wca_buf + 1, 1, ncclUint64, ncclSum, comm, Cs));
  HIPCHK(w2b_launch_wca_unpack(x->v.shared, x->wca_buf, Cs));
  const float scale = mode == 1 ? 1.f / (float)x->nranks : 1.f;
  x->x_use_cnt = mode == 2;
  if (mode == 2) {          // who has trained which row since the last exchange (2 V floats), before the first apply
    if (int rc = xchg_touched(x, Cs)) return rc;
    NCCLCHK(ncclAllReduce(x->xcnt, x->xcnt, (size_t)(2 * x->v.in.cfg.vocab_size), ncclFloat, ncclSum, comm, Cs));
    x->x_fac_pending = true;
    if (int rc = xchg_factor(x, Cs)) return rc;
    HIPCHK(hipEventRecord(x->x_evc, Cs));
    HIPCHK(hipStreamWaitEvent(E, x->x_evc, 0));
  }
  const long long nc = (long long)x->x_ranges.size();
  auto issue_delta_sum = [&](long long c) -> int {
    const int k = (int)(c & 1);
    if (int rc = xchg_delta(x, c)) return rc;
    HIPCHK(hipEventRecord(x->x_evd[k], E));
    HIPCHK(hipStreamWaitEvent(Cs, x->x_evd[k], 0));
    NCCLCHK(ncclAllReduce(x->xsum[k], x->xsum[k], (size_t)x->x_ranges[(size_t)c].len, ncclFloat, ncclSum, comm, Cs));
    HIPCHK(hipEventRecord(x->x_evs[k], Cs));
    return W2B_OK;
  };
  if (nc > 0) if (int rc = issue_delta_sum(0)) return rc;
  for (long long c = 0; c < nc; c++) {
    if (c + 1 < nc) if (int rc = issue_delta_sum(c + 1)) return rc;
    HIPCHK(hipStreamWaitEvent(E, x->x_evs[c & 1], 0));
    if (int rc = xchg_apply(x, c, scale)) return rc;
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
  W2bExchange *x = t->xchg;
  if (!x || !x->comm.c) return W2B_OK;     // a single replica without a communicator: nothing to exchange
  if (mode < 0 || mode > 2) return fail(W2B_EINVAL, "w2b_sync_replicas: unknown mode");
  if (int rc = xchg_begin(x)) return rc;
  if (int rc = xchg_run_rccl(x, mode)) { xchg_abort(x); return rc; }
  return xchg_end(x);
}

// ---- the same exchange for a host that brings its own collective (MPI, torch.distributed over gloo / RCCL, ...):
//   w2b_exchange_begin -> (w2b_exchange_counts, <sum over the replicas>) -> for every chunk: w2b_exchange_delta,
//   <sum *buf over the replicas, in place>, w2b_exchange_apply -> w2b_exchange_end.  The buffer handed out is device
// memory; the library's kernels run on its elementwise exchange stream, so w2b_exchange_delta returns after the delta is
// complete (the host's collective may use any stream or the CPU) and w2b_exchange_apply expects the sum to be complete
// when it is called.
extern "C" int w2b_exchange_begin(w2b_trainer *t, int64_t *n_chunks, int64_t *local_word_count) {
  NEED(t);
  W2bExchange *x = t->xchg;
  if (int rc = xchg_begin(x)) return rc;
  x->x_use_cnt = false;
  if (n_chunks) *n_chunks = (int64_t)x->x_ranges.size();
  if (local_word_count) {
    hipError_t e = w2b_launch_wca_pack(x->v.shared, x->wca_buf, x->xs[0]);
    unsigned long long v = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&v, x->wca_buf, sizeof v, hipMemcpyDeviceToHost, x->xs[0]);
    if (e == hipSuccess) e = hipStreamSynchronize(x->xs[0]);
    if (e != hipSuccess) { xchg_abort(x); return fail(W2B_EHIP, std::string("w2b_exchange_begin: ") + hipGetErrorString(e)); }
    *local_word_count = (int64_t)v;
  }
  return W2B_OK;
}
extern "C" int w2b_exchange_counts(w2b_trainer *t, void **buf_dev, int64_t *elems) {
  NEED(t);
  W2bExchange *x = t->xchg;
  if (!x || !x->x_open) return fail(W2B_ESTATE, "w2b_exchange_counts: w2b_exchange_begin first");
  if (!buf_dev || !elems) return fail(W2B_EINVAL, "w2b_exchange_counts: null argument");
  if (int rc = xchg_touched(x, x->xs[0])) return rc;
  HIPCHK(hipStreamSynchronize(x->xs[0]));
  x->x_use_cnt = true;
  x->x_fac_pending = true;                   // (the host sums the counts; the first w2b_exchange_apply turns them into factors)
  *buf_dev = x->xcnt;
  *elems = 2 * x->v.in.cfg.vocab_size;
  return W2B_OK;
}

extern "C" int w2b_exchange_delta(w2b_trainer *t, int64_t chunk, void **buf_dev, int64_t *elems) {
  NEED(t);
  W2bExchange *x = t->xchg;
  if (!x || !x->x_open) return fail(W2B_ESTATE, "w2b_exchange_delta: w2b_exchange_begin first");
  if (chunk < 0 || chunk >= (int64_t)x->x_ranges.size() || !buf_dev || !elems) return fail(W2B_EINVAL, "w2b_exchange_delta: bad argument");
  if (int rc = xchg_delta(x, chunk)) return rc;
  HIPCHK(hipStreamSynchronize(x->xs[0]));
  *buf_dev = x->xsum[chunk & 1];
  *elems = x->x_ranges[(size_t)chunk].len;
  return W2B_OK;
}
extern "C" int w2b_exchange_apply(w2b_trainer *t, int64_t chunk, float scale) {
  NEED(t);
  W2bExchange *x = t->xchg;
  if (!x || !x->x_open) return fail(W2B_ESTATE, "w2b_exchange_apply: w2b_exchange_begin first");
  if (chunk < 0 || chunk >= (int64_t)x->x_ranges.size()) return fail(W2B_EINVAL, "w2b_exchange_apply: bad chunk");
  return xchg_apply(x, chunk, scale);
}
extern "C" int w2b_exchange_end(w2b_trainer *t, int64_t word_count_all_replicas) {
  NEED(t);
  W2bExchange *x = t->xchg;
  if (!x || !x->x_open) return fail(W2B_ESTATE, "w2b_exchange_end: w2b_exchange_begin first");
  if (word_count_all_replicas >= 0) {        // the alpha schedule runs on the global count (ref :391)
    unsigned long long v = (unsigned long long)word_count_all_replicas;
    HIPCHK(hipMemcpyAsync(x->wca_buf + 1, &v, sizeof v, hipMemcpyHostToDevice, x->xs[0]));
    HIPCHK(hipStreamSynchronize(x->xs[0]));
    HIPCHK(w2b_launch_wca_unpack(x->v.shared, x->wca_buf, x->xs[0]));
  }
  return xchg_end(x);
}

extern "C" int w2b_sync_stats(w2b_trainer *t, int64_t *exchanges, double *device_ms) {
  NEED(t);
  W2bExchange *x = t->xchg;
  if (exchanges) *exchanges = x ? x->sync_count : 0;
  double ms = 0;
  if (x && x->x_open) return fail(W2B_ESTATE, "w2b_sync_stats: an exchange is in progress (w2b_exchange_end first)");
  for (size_t i = 0; x && i + 1 < x->x_ev.size(); i += 2) {      // begin -> end of every exchange, read after the fact
    HIPCHK(hipEventSynchronize(x->x_ev[i + 1]));
    float m = 0;
    HIPCHK(hipEventElapsedTime(&m, x->x_ev[i], x->x_ev[i + 1]));
    ms += m;
  }
  if (device_ms) *device_ms = ms;
  if (!x) return W2B_OK;
  x->x_ev.clear();
  x->sync_count = 0;
  return W2B_OK;
}
