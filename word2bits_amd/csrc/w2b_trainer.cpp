// w2b_trainer.cpp -- host side of the C ABI declared in include/word2bits_hip.h: lifetime, model, sampler state, launches,
// tuples.  Owns the trainer's device memory, streams and events; all arithmetic of the hot path lives in w2b_kernels_*.hip, the
// launch policy in w2b_plan.cpp, the replica exchange in w2b_exchange.cpp.  There is deliberately no CPU fallback in this file.
#include "../../include/word2bits_corpus.h"
#include "w2b_exchange.h"
#include "w2b_host.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static thread_local std::string g_err;
// shared with the other host translation units of the library (fail() of w2b_host.h, w2b_eval.cpp)
int w2b_internal_fail(int code, const char *msg) { g_err = msg ? msg : ""; return code; }

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
  p.table_size = (long long)t->table.cap;
  p.keep = (t->in.cfg.sample > 0) ? t->keep : nullptr;
  p.corpus = t->corpus;
  p.n_tokens = t->n_tokens;
  p.corpus_more = t->corpus_more ? 1 : 0;
  p.workers = t->workers;
  p.shared = t->shared;
  p.jump_a = t->jump_a;
  p.jump_c = t->jump_c;
  p.table_magic = p.table_size > 1 ? (unsigned long long)((((unsigned __int128)1) << 64) / (unsigned __int128)p.table_size) : 0;
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
static int grow(w2b_trainer *t, W2bDevBuf<T> &buf, size_t need, bool *grown = nullptr) {
  if (need <= buf.cap) return W2B_OK;
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(buf.alloc(need));
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
  {
    const char *g = getenv("W2B_GENERIC_WORKER");
    t->generic_worker = g && g[0] == '1' && g[1] == 0;
  }
  t->in.tune = w2b_default_tuning();
  HIPCHK(t->stream.create());
  t->table_elems = (long long)cfg->vocab_size * cfg->layer1_size;
  HIPCHK(t->uv.alloc((size_t)(2 * t->table_elems)));
  HIPCHK(hipMemsetAsync(t->uv, 0, sizeof(float) * 2 * t->table_elems, t->stream));
  HIPCHK(t->exp_table.alloc(W2B_EXP_TABLE_SIZE + 8));
  {
    std::vector<float> et(W2B_EXP_TABLE_SIZE + 8, 0.f);
    w2b_build_exp_table(et.data());
    HIPCHK(hipMemcpy(t->exp_table, et.data(), sizeof(float) * et.size(), hipMemcpyHostToDevice));
  }
  HIPCHK(t->shared.alloc(1));
  {
    W2bShared sh{};
    sh.alpha = cfg->alpha;
    HIPCHK(hipMemcpy(t->shared, &sh, sizeof sh, hipMemcpyHostToDevice));
  }
  HIPCHK(t->workers.alloc((size_t)cfg->num_threads));
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
    HIPCHK(t->jump_a.alloc((size_t)nj));
    HIPCHK(t->jump_c.alloc((size_t)nj));
    HIPCHK(hipMemcpy(t->jump_a, ja.data(), sizeof(unsigned long long) * nj, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t->jump_c, jc.data(), sizeof(unsigned long long) * nj, hipMemcpyHostToDevice));
  }
  HIPCHK(hipStreamSynchronize(t->stream));
  guard.t = nullptr;
  *out = t;
  return W2B_OK;
}

// Every stream is synchronised before anything is released; the members of w2b_trainer then release themselves.
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
  if (t->rc_stream) (void)hipStreamSynchronize(t->rc_stream);
  w2b_xchg_destroy(t->xchg);
  if (t->poll_host) (void)hipHostFree(t->poll_host);
  delete t;
}

// readers of the model wait for a replica exchange in flight, which has written the master rows
static int xchg_fence(w2b_trainer *t) {
  bool waited = false;
  const int rc = w2b_xchg_fence(t->xchg, &waited);
  if (waited) t->xhot_master_changed = true;
  return rc;
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
  W2bDevBuf<float> dl;
  HIPCHK(dl.alloc(65536));
  HIPCHK(hipMemcpyAsync(dl, lut.data(), sizeof(float) * 65536, hipMemcpyHostToDevice, t->stream));
  HIPCHK(w2b_launch_init_net(t->uv, t->uv + t->table_elems, t->table_elems, dl, t->stream));
  t->xhot_master_changed = true;
  HIPCHK(w2b_xchg_rebase(t->xchg, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
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
  HIPCHK(w2b_xchg_rebase(t->xchg, t->stream));
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
  W2bDevBuf<float> tmp;
  const long long n = t->table_elems;
  HIPCHK(tmp.alloc((size_t)(n < slab ? n : slab)));
  for (long long o = 0; o < n; o += slab) {
    const long long m = (n - o < slab) ? n - o : slab;
    hipError_t e = w2b_launch_export(t->uv + o, t->uv + t->table_elems + o, tmp, m, t->in.cfg.bitlevel, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out + o, tmp, sizeof(float) * m, hipMemcpyDeviceToHost, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) return fail(W2B_EHIP, std::string("w2b_export_quantized: ") + hipGetErrorString(e));
  }
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
  W2bDevBuf<unsigned long long> tmp;
  HIPCHK(tmp.alloc((size_t)((V < slab_rows ? V : slab_rows) * wpr)));
  for (long long r = 0; r < V; r += slab_rows) {
    const long long m = (V - r < slab_rows) ? V - r : slab_rows;
    const long long o = r * t->in.cfg.layer1_size;
    hipError_t e = w2b_launch_export_packed(t->uv + o, t->uv + t->table_elems + o, tmp, m, t->in.cfg.layer1_size,
                                            t->in.cfg.bitlevel, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out + r * wpr, tmp, sizeof(uint64_t) * (size_t)(m * wpr), hipMemcpyDeviceToHost, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) return fail(W2B_EHIP, std::string("w2b_export_packed: ") + hipGetErrorString(e));
  }
  return W2B_OK;
}

// --------------------------------------------------------------------------------- sampler state
extern "C" int w2b_set_unigram_table(w2b_trainer *t, const int32_t *table, int64_t tsz) {
  NEED(t);
  if (!table || tsz <= 0) return fail(W2B_EINVAL, "w2b_set_unigram_table: bad argument");
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(t->table.alloc((size_t)tsz));
  HIPCHK(hipMemcpy(t->table, table, sizeof(int32_t) * tsz, hipMemcpyHostToDevice));
  return W2B_OK;
}

extern "C" int w2b_set_vocab_counts(w2b_trainer *t, const int64_t *cn, int64_t table_size) {
  NEED(t);
  if (!cn) return fail(W2B_EINVAL, "w2b_set_vocab_counts: null counts");
  const int64_t V = t->in.cfg.vocab_size;
  const std::vector<float> keep = w2b_plan_set_counts(t->in, cn);
  if (!t->keep) HIPCHK(t->keep.alloc((size_t)V));
  HIPCHK(hipMemcpy(t->keep, keep.data(), sizeof(float) * V, hipMemcpyHostToDevice));
  if (int rc = w2b_xchg_upload_rates(t->xchg)) return rc;
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
  W2bEvent a, b;
  if (t->ev_pool.size() >= 2) {
    a = std::move(t->ev_pool.back()); t->ev_pool.pop_back();
    b = std::move(t->ev_pool.back()); t->ev_pool.pop_back();
  } else {
    hipError_t e = a.create(hipEventDefault);
    if (e == hipSuccess) e = b.create(hipEventDefault);
    if (e != hipSuccess) return e;
  }
  t->ev.push_back(std::move(a));
  t->ev.push_back(std::move(b));
  return hipEventRecord(t->ev[t->ev.size() - 2], t->stream);
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
  for (W2bEvent &e : t->ev) t->ev_pool.push_back(std::move(e));
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
  HIPCHK(t->corpus_owned.alloc((size_t)(n > 0 ? n : 1)));
  HIPCHK(hipMemcpy(t->corpus_owned, ids, sizeof(int32_t) * n, hipMemcpyHostToDevice));
  t->corpus = t->corpus_owned;
  t->n_tokens = n;
  return W2B_OK;
}

extern "C" int w2b_set_corpus_device(w2b_trainer *t, const void *ids_dev, int64_t n) {
  NEED(t);
  if (!ids_dev || n < 0) return fail(W2B_EINVAL, "w2b_set_corpus_device: bad argument");
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(t->corpus_owned.reset());
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
  if (int rc = grow(t, t->rc, 64 + (size_t)W2B_NXCD * W2B_RC_MAX * t->in.cfg.layer1_size)) return rc;   // 64 ints of flags, then the copies
  if (!t->rc_stream) {
    HIPCHK(t->rc_stream.create());
    HIPCHK(t->rc_go.create());
    HIPCHK(t->rc_end.create());
  }
  HIPCHK(hipMemsetAsync(t->rc, 0, 64 * sizeof(int), t->stream));                    // claims and alive flags of this launch
  HIPCHK(hipMemsetAsync(&t->shared->launch_done, 0, sizeof(int), t->stream));
  p.rc_rows = lp.refresh_rows_u;
  p.rc_flags = reinterpret_cast<int *>(t->rc.p);
  p.rc = t->rc + 64;
  return W2B_OK;
}

// scratch rows of process_word_wide for `workgroups` workgroups
static int wide_prepare(w2b_trainer *t, W2bParams &p, long long workgroups) {
  if (!p.wide) return W2B_OK;
  if (int rc = grow(t, t->wide_scratch, (size_t)workgroups * 2 * t->in.cfg.layer1_size)) return rc;
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
  if (int rc = grow(t, t->xhot, need, &fresh)) return rc;
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

extern "C" int w2b_worker_kernel_lean(w2b_trainer *t, int32_t *lean) {
  NEED(t);
  if (!lean) return fail(W2B_EINVAL, "w2b_worker_kernel_lean: null");
  const W2bLaunchPlan lp = w2b_plan_launch(t->in, t->in.cfg.num_threads);
  const W2bParams p = make_params(t, lp);
  *lean = (lp.kernel == W2B_KERNEL_PLAIN && w2b_workers_lean(p, t->generic_worker)) ? 1 : 0;
  return W2B_OK;
}

extern "C" int w2b_train_step(w2b_trainer *t, int64_t max_positions) {
  NEED(t);
  if (!t->corpus || !t->shards_set) return fail(W2B_ESTATE, "w2b_train_step: corpus/shards not set");
  if (max_positions <= 0) return fail(W2B_EINVAL, "w2b_train_step: max_positions must be positive");
  const W2bLaunchPlan lp = w2b_plan_launch(t->in, t->in.cfg.num_threads);
  if (lp.kernel == W2B_KERNEL_RESIDENT)    // scratch rows of the sentence-resident kernel
    if (int rc = grow(t, t->entry,
                      (size_t)t->in.cfg.num_threads * (size_t)w2b_resident_scratch_rows(lp.radius) * t->in.cfg.layer1_size)) return rc;
  W2bParams p = make_params(t, lp);
  if (int rc = xhot_prepare(t, p)) return rc;
  if (int rc = wide_prepare(t, p, t->in.cfg.num_threads)) return rc;

  w2b_xchg_add_words(t->xchg, (long long)max_positions * t->in.cfg.num_threads);
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
      HIPCHK(w2b_launch_workers(q, max_positions, t->in.cfg.compute_loss != 0, t->stream, base + conc < t->in.cfg.num_threads ? conc : t->in.cfg.num_threads - base,
                                t->generic_worker));
    }
  }
  HIPCHK(timing_end(t));
  if (p.rc_rows > 0) HIPCHK(hipStreamWaitEvent(t->stream, t->rc_end, 0));   // (what follows on this stream also follows the refresher's end)
  HIPCHK(w2b_launch_xhot_fold(p, t->stream));      // the master rows are complete again when the stream is idle
  {   // progress snapshot of this launch for w2b_epoch_poll (asynchronous; pinned host memory)
    if (!t->poll_host) {
      HIPCHK(hipHostMalloc((void **)&t->poll_host, sizeof(W2bShared) * w2b_trainer::kPoll, hipHostMallocDefault));
      for (int i = 0; i < w2b_trainer::kPoll; i++) HIPCHK(t->poll_ev[i].create());
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
  if ((rc = grow(t, t->st_center, n))) return rc;
  if ((rc = grow(t, t->st_off, n + 1))) return rc;
  if ((rc = grow(t, t->st_ctx, nctx > 0 ? nctx : 1))) return rc;
  if ((rc = grow(t, t->st_neg, (size_t)n * (K > 0 ? K : 1)))) return rc;
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
