// w2b_host.h -- what the host units of the trainer's C ABI share (w2b_trainer.cpp, w2b_exchange.cpp): the error helpers and
// struct w2b_trainer.  Internal, like w2b_internal.h.
#pragma once
#include "../../include/word2bits_hip.h"
#include "w2b_internal.h"
#include "w2b_owned.h"
#include "w2b_plan.h"

#include <rccl/rccl.h>

#include <string>
#include <vector>

inline int fail(int code, const std::string &msg) { return w2b_internal_fail(code, msg.c_str()); }   // sets w2b_last_error()
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
#define NEED(t)                                                                  \
  do {                                                                           \
    if (!(t)) return fail(W2B_EINVAL, "null trainer");                          \
    HIPCHK(hipSetDevice((t)->device));                                           \
  } while (0)

struct W2bExchange;   // w2b_exchange.h

// Members release themselves (w2b_owned.h) in reverse order of declaration: the streams come first, so they go last.
struct w2b_trainer {
  W2bPlanInputs in;             // configuration, tuning knobs, compute units, word-count statistics: what the launch policy reads (w2b_plan.h)
  int device = 0;
  W2bStream stream;
  W2bStream rc_stream;          // the refresher kernel's stream
  W2bDevBuf<float> uv;          // u followed by v (one allocation: one all-reduce)
  long long table_elems = 0;    // vocab_size * layer1_size
  W2bDevBuf<float> exp_table;
  W2bDevBuf<int32_t> table;     // unigram table (cap = its size)
  W2bDevBuf<float> keep;
  W2bDevBuf<float> entry;       // scratch rows of the sentence-resident kernel
  W2bDevBuf<float> wide_scratch;        // process_word_wide: [workgroups][2][dim]
  // XCD-shared copies of the hottest rows (XHot in w2b_device.hpp)
  W2bDevBuf<float> xhot;        // [W2B_NXCD]{copies [nu + nv][dim], entries [nu + nv][dim], merge locks [nu + nv][W2B_MAXW]}
  W2bDevBuf<float> rc;          // row-group kernel: 64 ints of flags + refreshed per-XCD copies of the hottest context rows
  W2bEvent rc_go, rc_end;
  int xhot_nu = -1, xhot_nv = -1;       // layout the buffer currently has (-1: none)
  bool xhot_master_changed = true;      // the master rows may differ from what the copies were folded into
  bool debug = false;           // W2B_DEBUG was set when the trainer was created (diagnostics on stderr)
  bool generic_worker = false;  // W2B_GENERIC_WORKER=1 was set when the trainer was created: the plain worker kernel runs its generic form
  const int32_t *corpus = nullptr;
  W2bDevBuf<int32_t> corpus_owned;
  long long n_tokens = 0;
  bool corpus_more = false;     // the tokens are a slice of the file and the file continues behind it
  W2bDevBuf<W2bWorker> workers;
  W2bDevBuf<W2bShared> shared;
  W2bDevBuf<unsigned long long> jump_a, jump_c;
  std::vector<long long> shard_start;
  std::vector<int> shard_override;
  bool shards_set = false;
  W2bDevBuf<int32_t> st_center, st_off, st_ctx, st_neg;   // staging for the host-pointer tuple form
  // timing
  bool timing = false;
  std::vector<W2bEvent> ev;      // pairs
  std::vector<W2bEvent> ev_pool;
  // non-blocking progress: after every launch the shared block is copied into a pinned ring slot behind an event
  static const int kPoll = 4;
  W2bShared *poll_host = nullptr;          // pinned [kPoll]
  W2bEvent poll_ev[kPoll];
  long long launches = 0;                  // w2b_train_step calls since w2b_epoch_begin
  W2bExchange *xchg = nullptr;             // the replica exchange: null until w2b_comm_init / w2b_exchange_init
};
